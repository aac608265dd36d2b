"""CPU checks of tests/nonfinite_ref.py: the references of tests/test_nonfinite.py alone have to meet the conditions that make a comparison
by class fair -- inputs non-zero and O(1) (bf16 cases exact in bf16), the class of every sum independent of the order of its terms (each
reference runs forwards and reversed), and every case covers what it is there for (a non-finite element, at least half finite, a finite
neighbour of the non-finite region).  The builders assert all of that themselves; this file calls every builder the GPU tests call, with
the same arguments, and checks the numpy pool rule on groups whose answer is written down here by hand.  No GPU."""
import numpy as np
import pytest

import nonfinite_ref as R

NAN, INF = np.nan, R.INF


def test_cls_and_comparison_helpers():
    a = np.array([0.0, -0.0, 1e38, INF, -INF, NAN, R.FLT_MAX])
    assert R.cls(a).tolist() == [0, 0, 0, 1, 2, 3, 0]
    ref = np.array([1.0, INF, NAN, -2.0])
    assert R.assert_matches(np.array([1.0 + 5e-6, INF, NAN, -2.0]), ref, 1e-5) > 0
    with pytest.raises(AssertionError):
        R.assert_matches(np.array([1.0, NAN, NAN, -2.0]), ref, 1e-5)          # NaN where +Inf belongs
    with pytest.raises(AssertionError):
        R.assert_matches(np.array([1.0, INF, NAN, NAN]), ref, 1e-5)           # NaN where a finite value belongs
    with pytest.raises(AssertionError):
        R.assert_matches(np.array([1.0, -INF, NAN, -2.0]), ref, 1e-5)         # the sign of an Inf
    with pytest.raises(AssertionError):
        R.assert_matches(np.array([1.001, INF, NAN, -2.0]), ref, 1e-5)        # the finite part is still held to the tolerance
    assert R.bf16_exact(np.array([1.5, -0.75, INF, NAN], np.float32)) and not R.bf16_exact(np.array([1.0 + 2.0 ** -12], np.float32))
    with pytest.raises(AssertionError):
        R.check_coverage(np.ones((4, 4)), "all finite")
    with pytest.raises(AssertionError):
        R.check_coverage(np.full((4, 4), NAN), "nothing finite")
    with pytest.raises(AssertionError):
        R.check_inputs(np.array([1.0, 0.0]))
    with pytest.raises(AssertionError):
        R.check_inputs(np.array([1.0, 1e30]))


def test_order_dependence_is_noticed():
    """a sum whose class DOES depend on the order (a finite partial sum that overflows) is refused by order_checked"""
    terms = np.array([R.FLT_MAX, R.FLT_MAX, -R.FLT_MAX], np.float32)

    def fn(rev):
        s = np.float32(0)
        for v in (terms[::-1] if rev else terms):
            s = np.float32(s + v)
        return np.array([s], np.float64)
    with pytest.raises(AssertionError):
        R.order_checked(fn, "overflowing partial sum")


def test_duplicates_are_separate_terms():
    """a*Inf + (-b)*Inf is NaN entry by entry (a coalesced matrix would give +Inf); an Inf of one sign stays that Inf; absent rows stay finite"""
    row, col, val = np.array([0, 0, 1, 2]), np.array([1, 1, 1, 0]), np.array([0.75, -0.5, 0.75, 1.0], np.float32)
    x = np.array([[[1.0], [INF], [2.0]]])
    y = R.hop_ref(3, row, col, val, x)
    assert R.cls(y)[0, :, 0].tolist() == [R.NAN, R.PINF, R.FIN] and y[0, 2, 0] == 1.0
    y = R.hop_ref(3, row, col, val, x, z=np.full((1, 3, 1), NAN), beta=0.0)
    assert R.cls(y)[0, 2, 0] == R.FIN                                          # beta == 0: z is not a term
    assert R.cls(R.hop_ref(3, row, col, val, x, z=np.full((1, 3, 1), -INF), alpha=2.0, beta=1.0))[0, :, 0].tolist() == [R.NAN, R.NAN, R.NINF]


@pytest.mark.parametrize("C", [1, 4, 16, 64, 300])
@pytest.mark.parametrize("poison", R.HOP_POISONS)
def test_hop_cases_meet_the_conditions(poison, C):
    row, col, val, mk, x, ref = R.hop_case(poison, C)
    deg = np.bincount(row, minlength=mk["n"])
    assert deg[mk["hub"]] >= 700 and 64 < deg[mk["wave_row"]] <= 128 and all(deg[i] == 0 for i in mk["iso"])
    for r, c in mk["dup"]:
        assert ((row == r) & (col == c)).sum() == 2 and np.sign(val[(row == r) & (col == c)]).sum() == 0
    assert (R.cls(x[0]) == R.FIN).all()


@pytest.mark.parametrize("t", sorted(R.SERIES_POISON_T))
@pytest.mark.parametrize("N", [3, 16])
@pytest.mark.parametrize("f,H", R.SERIES_FH)
def test_series_cases_meet_the_conditions(f, H, N, t):
    stack, W, bias, ref, touched = R.series_case(f, H, N, t, R.SERIES_POISON_T[t])
    assert touched.sum() == min(H, t + 1, R.SERIES_T - t, R.SERIES_T - H + 1)


def test_series_fh_covers_every_ragged_tail():
    """the scalar-load shapes cover H*f mod 4 = 1, 2, 3 (the last 4-wide k step is ragged) and the 16-byte shapes are there too"""
    assert {(H * f) % 4 for f, H in R.SERIES_FH if f % 4} == {1, 2, 3}
    assert any(f % 4 == 0 for f, H in R.SERIES_FH)
    assert sorted(R.SERIES_POISON_T) == [20, 31, 32, R.SERIES_T - 1]


@pytest.mark.parametrize("geom", [dict(stride=2, padl=2, padr=1), dict(dil=2, padl=3, padr=1), dict(dil=3),
                                  dict(padl=4), dict(dil=2, padl=8)])
@pytest.mark.parametrize("t", sorted(R.SERIES_POISON_T))
def test_series_geometries_meet_the_conditions(geom, t):
    for f, H in ((1, 5), (3, 7)):
        if (H - 1) * geom.get("dil", 1) < geom.get("padl", 0):
            continue
        R.series_case(f, H, 3, t, R.SERIES_POISON_T[t], **geom)


def test_window_gather_against_a_hand_count():
    nwin, taps = R.window_taps(10, 3, stride=2, padl=1, padr=1, dil=2)
    assert nwin == 4 and taps.tolist() == [[-1, 1, 3], [1, 3, 5], [3, 5, 7], [5, 7, 9]]
    assert R.windows_touching(3, 10, 3, 2, 1, 1, 2).tolist() == [True, True, True, False]
    stack = np.arange(1, 11, dtype=np.float64).reshape(1, 1, 1, 10, 1)
    W = np.array([1.0, 10.0, 100.0]).reshape(1, 3, 1, 1)
    out = R.windows_ref(stack, W, None, 2, 1, 1, 2)
    assert out[0, 0, :, 0].tolist() == [0 + 20 + 400, 2 + 40 + 600, 4 + 60 + 800, 6 + 80 + 1000]


def test_series_gradient_references():
    """the input gradient is the transpose of the forward: <windows_ref(x), g> == <x, series_dgrad_ref(g)>, and the weight gradient likewise"""
    rng = np.random.default_rng(3)
    K, S, n, T, f, H, N = 2, 2, 3, 12, 3, 5, 4
    x, W, g = rng.standard_normal((K, S, n, T, f)), rng.standard_normal((K, H, f, N)), rng.standard_normal((S, n, T - H + 1, N))
    lhs = (R.windows_ref(x, W) * g).sum()
    assert abs(lhs - (x * R.series_dgrad_ref(g, W, T)).sum()) <= 1e-10 * abs(lhs)
    assert abs(lhs - (W * R.series_wgrad_ref(x, g, H)).sum()) <= 1e-10 * abs(lhs)
    g[1, 2, 4] = INF
    G = R.order_checked(lambda rev: R.series_dgrad_ref(g, np.abs(W), T, reverse=rev), "dgrad")
    nonfin = (R.cls(G) != R.FIN).any(axis=(0, 4))
    want = np.zeros((S, n, T), bool)
    want[1, 2, 4:4 + H] = True
    assert np.array_equal(nonfin, want)


def test_ring_layout():
    rows = np.arange(2 * 3, dtype=np.float32).reshape(1, 1, 1, 3, 2)           # three time rows of two channels
    ring = R.ring_of(rows, head=1, ring_ld=8)
    assert ring[0, 0, 0, :6].tolist() == [4.0, 5.0, 0.0, 1.0, 2.0, 3.0] and np.isnan(ring[0, 0, 0, 6:]).all()


# ---------------------------------------------------------------------------------------------------------------- the pool rule
HAND = {       # group name -> (relu + pool value, arg-max, plain max value) for pool 2 and pool 4
    2: {"tie": (1.5, 0, 1.5), "tie0": (0.0, 0, 0.0), "neg": (0.0, 1, -0.5), "nan@0": (NAN, 0, NAN), "nan@1": (NAN, 1, NAN), "nan-nan": (NAN, 0, NAN),
        "-inf": (0.0, 1, -1.0), "-inf+": (0.75, 1, 0.75), "+inf": (INF, 1, INF), "+inf-nan": (NAN, 1, NAN), "-0": (0.0, 0, 0.0), "0-0": (0.0, 0, 0.0),
        "-0neg": (0.0, 0, 0.0), "plain": (1.0, 1, 1.0)},
    4: {"tie": (1.5, 1, 1.5), "tie0": (0.0, 0, 0.0), "neg": (0.0, 1, -0.5), "nan@0": (NAN, 0, NAN), "nan@1": (NAN, 1, NAN), "nan@2": (NAN, 2, NAN),
        "nan@3": (NAN, 3, NAN), "nan-nan": (NAN, 1, NAN), "-inf": (0.0, 1, -1.0), "-inf+": (0.75, 2, 0.75), "+inf": (INF, 1, INF),
        "+inf-nan": (NAN, 2, NAN), "-0": (0.0, 0, 0.0), "0-0": (0.0, 0, 0.0), "-0neg": (0.0, 1, 0.0), "plain": (1.0, 1, 1.0)},
}


@pytest.mark.parametrize("pool", [2, 4])
def test_pool_rule_on_the_crafted_groups(pool):
    groups = R.pool_groups(pool)
    names = [g[0] for g in groups]
    assert set(names) == set(HAND[pool]) and len(set(names)) == len(names)
    wanted = {"tie", "tie0", "neg", "nan-nan", "-inf", "+inf", "-0"} | {"nan@%d" % m for m in range(pool)}
    assert wanted <= set(names)
    y = R.pool_input(pool, 3)
    z, idx = R.pool_rule(y, pool, relu=True)
    m, midx = R.pool_rule(y, pool, relu=False)
    assert np.array_equal(idx, midx)
    for g, name in enumerate(names):
        zv, bi, mv = HAND[pool][name]
        for got, want in ((z[0, g, 0], zv), (m[0, g, 0], mv)):
            assert R.cls(got) == R.cls(want) and (want != want or got == want), (name, got, want)
        assert idx[0, g, 0] == bi, (name, idx[0, g, 0], bi)
    # against numpy's own NaN-propagating maximum (values; the arg-max has no numpy counterpart with this tie rule)
    with np.errstate(invalid="ignore"):
        ref = np.maximum.reduce(y.reshape(2, -1, pool, 3), axis=2)
        assert np.array_equal(R.cls(m), R.cls(ref)) and (m[R.cls(ref) == 0] == ref[R.cls(ref) == 0]).all()
        relu = np.where(ref > 0, ref, np.where(np.isnan(ref), ref, 0))
        assert np.array_equal(R.cls(z), R.cls(relu)) and (z[R.cls(relu) == 0] == relu[R.cls(relu) == 0]).all()
    R.check_coverage(z, "pool %d" % pool, neighbour_axis=1)
    assert (z[R.cls(z) == 0] >= 0).all() and not np.signbit(z[R.cls(z) == 0]).any()        # relu: +0, never -0


@pytest.mark.parametrize("pool", [2, 4])
def test_pool_backward_rule(pool):
    y = R.pool_input(pool, 3)
    for relu in (True, False):
        z, idx = R.pool_rule(y, pool, relu)
        gz = np.arange(1, z.size + 1, dtype=np.float32).reshape(z.shape)
        gy = R.pool_bwd_rule(gz, z, idx, pool, relu).reshape(z.shape[0], z.shape[1], pool, z.shape[2])
        assert ((gy != 0).sum(axis=2) <= 1).all()
        sent = np.take_along_axis(gy, idx[:, :, None, :].astype(np.int64), axis=2)[:, :, 0]
        with np.errstate(invalid="ignore"):
            assert np.array_equal(sent, np.where(z > 0, gz, 0) if relu else gz)


# ---------------------------------------------------------------------------------------------------------------- projections
@pytest.mark.parametrize("N", [3, 16, 70])
@pytest.mark.parametrize("Kc", [3, 33, 64])
def test_project_cases_meet_the_conditions(Kc, N):
    terms, W, bias, ref = R.project_case(Kc, N)
    assert R.cls(ref[0]).tolist() == [R.NAN] * N                    # NaN in: NaN out, whatever else the row holds
    assert set(R.cls(ref[64]).tolist()) <= {R.PINF, R.NINF, R.NAN}  # +Inf in every k of the row: the sign of the weight sum, or Inf - Inf
    assert all(c == (R.NINF if w > 0 else R.PINF) for c, w in zip(R.cls(ref[129]), W[1, Kc - 1]))
    terms, W, ref = R.project_large_case(Kc, N)
    assert np.abs(ref[7]).max() > 1e34 and np.abs(ref[100]).max() > 1e34


@pytest.mark.parametrize("Kc,N", [(3, 3), (33, 16), (32, 16), (64, 64), (64, 70)])
def test_mapped_project_cases_meet_the_conditions(Kc, N):
    terms, W, bias, rowmap, ref = R.mapped_case(Kc, N)
    assert len(set(rowmap.tolist())) == R.MAPPED_M and rowmap.max() < R.MAPPED_NV and not np.array_equal(rowmap, np.sort(rowmap))
    assert (R.cls(ref[0]) == R.FIN).all()


def test_series_weight_gradient_reference_with_a_geometry():
    """<windows_ref(x), g> == <W, series_wgrad_ref(x, g)> with a window step, padding and dilation"""
    rng = np.random.default_rng(4)
    K, S, n, T, f, H, N = 2, 2, 3, 20, 3, 5, 4
    for st, pl, pr, d in ((2, 2, 1, 1), (1, 3, 1, 2), (3, 0, 2, 1), (1, 8, 0, 2)):
        x, W = rng.standard_normal((K, S, n, T, f)), rng.standard_normal((K, H, f, N))
        y = R.windows_ref(x, W, None, st, pl, pr, d)
        g = rng.standard_normal(y.shape)
        lhs = (y * g).sum()
        assert abs(lhs - (W * R.series_wgrad_ref(x, g, H, st, pl, d)).sum()) <= 1e-10 * abs(lhs)
        assert abs(lhs - (x * R.series_dgrad_ref(g, W, T, st, pl, d)).sum()) <= 1e-10 * abs(lhs)
