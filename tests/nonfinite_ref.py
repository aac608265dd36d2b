"""References and case builders of tests/test_nonfinite.py: where +-Inf and NaN have to come out.  Plain numpy, float64, no GPU and no scipy
(scipy coalesces duplicate entries; DESIGN.md section 4 keeps them as separate terms, so a*Inf + (-b)*Inf is NaN).

Every reference is evaluated PER STORED TERM under np.errstate(invalid="ignore", over="ignore").  Outputs are compared by class -- cls():
0 finite, 1 +Inf, 2 -Inf, 3 NaN -- element by element, and by the kernel's usual tolerance on the finite elements.  That comparison is only
fair when the class of a sum does not depend on the order of its terms, which holds under the input conditions checked here: finite operands
non-zero and O(1) (no finite partial sum overflows), so a NaN term gives NaN, +Inf with -Inf gives NaN, otherwise the Inf's sign or finite.
Each reference therefore runs in the given term order and in the reversed one and asserts equal classes (order_checked), and each case
asserts its own coverage (check_coverage): a non-finite element exists, at least half are finite, and -- where the case is about locality --
a finite element sits directly next to the non-finite region.  A case that misses one of these is an error of the test, never a skip.

tests/test_nonfinite_ref.py runs all of this on the CPU; tests/test_nonfinite.py feeds the same cases to the kernels."""
import numpy as np

FIN, PINF, NINF, NAN = 0, 1, 2, 3
INF = float("inf")
FLT_MAX = float(np.finfo(np.float32).max)


def cls(a):
    """0 finite, 1 +Inf, 2 -Inf, 3 NaN, element by element"""
    a = np.asarray(a, np.float64)
    c = np.zeros(a.shape, np.int8)
    c[a == np.inf] = PINF
    c[a == -np.inf] = NINF
    c[np.isnan(a)] = NAN
    return c


def class_mismatch(out, ref):
    """indices (at most 8) where the classes differ, for the assertion message"""
    bad = np.argwhere(cls(out) != cls(ref))
    return [(tuple(int(v) for v in i), float(np.asarray(out, np.float64)[tuple(i)]), float(np.asarray(ref, np.float64)[tuple(i)])) for i in bad[:8]]


def finite_err(out, ref):
    """conftest.rel_err restricted to the elements the reference has finite: max|out - ref| / max|ref| over them (0 when there are none)"""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    m = np.isfinite(ref)
    if not m.any():
        return 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(np.where(m, out, 0.0) - np.where(m, ref, 0.0)).max()
    den = np.abs(ref[m]).max()
    return float(d / (den if den > 0 else 1.0))


def assert_matches(out, ref, tol, what=""):
    """class equality everywhere, the tolerance on the finite part"""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    bad = class_mismatch(out, ref)
    assert not bad, "%s: %d elements of another class than the reference; (index, got, want): %s" % (what, int((cls(out) != cls(ref)).sum()), bad)
    e = finite_err(out, ref)
    assert e <= tol, (what, e, tol)
    return e


def check_inputs(*finite_operands):
    """the input conditions: operands (weights, operand values, the finite part of the activations) non-zero and O(1)"""
    for a in finite_operands:
        a = np.asarray(a, np.float64)
        f = a[np.isfinite(a)]
        assert f.size and (f != 0).all() and np.abs(f).max() <= 16.0 and np.abs(f).min() >= 2.0 ** -10, (np.abs(f).min(), np.abs(f).max())


def bf16_exact(a):
    """True when every finite value of a survives a round trip through bfloat16 (the low 16 bits of its fp32 pattern are zero)"""
    a = np.ascontiguousarray(a, np.float32)
    return bool(((a.view(np.uint32) & 0xFFFF) == 0)[np.isfinite(a)].all())


def to_bf16_grid(a):
    """a rounded (toward zero) onto the bf16 grid, as float32; zeros are moved to the grid's neighbour so that operands stay non-zero"""
    a = np.ascontiguousarray(a, np.float32).copy()
    a.view(np.uint32)[...] &= np.uint32(0xFFFF0000)
    a[a == 0] = 0.5
    return a


def check_coverage(ref, what, neighbour_axis=None):
    """the coverage conditions of one case on its reference output; neighbour_axis: the axis (window / vertex / row) along which a finite
    element has to sit directly next to a non-finite one"""
    c = cls(ref)
    nonfin = c != FIN
    assert nonfin.any(), "%s: the reference output is finite everywhere -- the poison reaches nothing" % what
    assert 2 * int((~nonfin).sum()) >= c.size, "%s: fewer than half of the reference output is finite" % what
    if neighbour_axis is not None:
        a = np.moveaxis(nonfin, neighbour_axis, -1)
        edge = (a[..., 1:] != a[..., :-1])
        assert edge.any(), "%s: no finite element next to the non-finite region along axis %d" % (what, neighbour_axis)


def order_checked(fn, what):
    """fn(reverse) -> the reference in the given term order (False) and in the reversed one (True); equal classes, the first is returned"""
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = fn(False), fn(True)
    assert np.array_equal(cls(a), cls(b)), "%s: the class of the reference depends on the order of its terms" % what
    m = cls(a) == FIN
    assert not m.any() or np.abs(a[m] - b[m]).max() <= 1e-12 * max(1.0, np.abs(a[m]).max()), what      # fp64 rounding of the two orders, no more
    return a


# ---------------------------------------------------------------------------------------------------------------- A1: hops
def hop_graph(n=600, avg_deg=5, seed=0):
    """(row, col, val, marks): a random pattern of n * avg_deg entries plus a hub row of 700+ entries (several lane-group segments and a
    fix-up), a row of 80 entries (the wave-row range), two isolated vertices, two duplicate (row, col) pairs with values of opposite sign and
    one column that no entry references.  marks names the special vertices.  Values are non-zero, O(1) and exact in bf16."""
    rng = np.random.default_rng(seed)
    hub, wave_row, iso, unref = 5, 17, (3, n // 2), n - 7
    dup = ((40, 41), (n - 2, 9))                       # (row, col) of the duplicate pairs
    m = n * avg_deg
    row, col = rng.integers(0, n, m), rng.integers(0, n, m)
    row = np.concatenate([row, np.full(720, hub), np.full(80, wave_row)])
    col = np.concatenate([col, rng.integers(0, n, 720), rng.integers(0, n, 80)])
    dup_cols = [c for _, c in dup]
    keep = ~np.isin(row, iso) & (col != unref) & ~np.isin(col, dup_cols)       # the duplicate pairs' columns are referenced by them alone
    row, col = row[keep], col[keep]
    val = rng.choice([-1.5, -1.0, -0.75, -0.5, 0.5, 0.75, 1.0, 1.5], row.shape[0])
    for r, c in dup:
        row, col, val = np.concatenate([row, [r, r]]), np.concatenate([col, [c, c]]), np.concatenate([val, [0.75, -0.5]])
    # clamped indices point at vertex 0 and n - 1: both are referenced by ordinary entries too
    row, col, val = np.concatenate([row, [8, 9]]), np.concatenate([col, [0, n - 1]]), np.concatenate([val, [1.0, -1.0]])
    marks = dict(hub=hub, wave_row=wave_row, iso=iso, unref=unref, dup=dup, n=n)
    return row.astype(np.int64), col.astype(np.int64), val.astype(np.float32), marks


def hop_ref(n, row, col, val, x, z=None, alpha=1.0, beta=0.0, z2=None, gamma=0.0, reverse=False):
    """y = alpha * (L x) + beta * z + gamma * z2 with L x summed entry by entry (np.add.at: duplicates are separate terms); x (nb, n_cols, C).
    z / z2 enter only with a non-zero factor, as in the kernel (beta == 0 never reads z)."""
    x = np.asarray(x, np.float64)
    order = np.arange(row.shape[0])[::-1] if reverse else np.arange(row.shape[0])
    s = np.zeros((x.shape[0], n, x.shape[2]))
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(x.shape[0]):
            np.add.at(s[b], row[order], val[order].astype(np.float64)[:, None] * x[b, col[order]])
        y = alpha * s
        if z is not None and beta != 0.0:
            y = y + beta * np.asarray(z, np.float64)
        if z2 is not None and gamma != 0.0:
            y = y + gamma * np.asarray(z2, np.float64)
    return y


HOP_POISONS = ("hub_inf", "inf_minus_inf", "dup_inf", "ends_nan", "unref_nan")


def hop_case(poison, C, seed=1, nb=2):
    """(row, col, val, marks, x, ref) of one A1 poison on rows of C floats; the poison sits in sample 1 only, sample 0 stays finite"""
    row, col, val, mk = hop_graph(seed=0)
    n = mk["n"]
    rng = np.random.default_rng([seed, C])
    x = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], (nb, n, C)).astype(np.float32)
    locality = 1
    if poison == "hub_inf":                    # +Inf in an X row the hub references
        x[1, col[row == mk["hub"]][3]] = INF
    elif poison == "inf_minus_inf":            # +Inf and -Inf in two rows that share a neighbour: NaN there
        r = mk["wave_row"]
        c0, c1 = col[row == r][:2]
        assert c0 != c1
        sgn = np.sign(val[row == r][:2])
        x[1, c0], x[1, c1] = INF * sgn[0], -INF * sgn[1]
    elif poison == "dup_inf":                  # +Inf in the column of a duplicate pair: a*Inf + (-b)*Inf = NaN
        x[1, mk["dup"][0][1]] = INF
    elif poison == "ends_nan":                 # the targets of clamped indices
        x[1, 0, :], x[1, n - 1, :] = np.nan, np.nan
    elif poison == "unref_nan":                # a row that no entry references: the whole output stays finite
        assert not (col == mk["unref"]).any()
        x[1, mk["unref"]] = np.nan
        locality = None
    else:
        raise KeyError(poison)
    what = "hop %s C=%d" % (poison, C)
    check_inputs(val, x)
    assert bf16_exact(val) and bf16_exact(x)
    ref = order_checked(lambda rev: hop_ref(n, row, col, val, x, reverse=rev), what)
    if poison == "unref_nan":
        assert (cls(ref) == FIN).all(), what
    else:
        check_coverage(ref, what, neighbour_axis=locality)
        assert (cls(ref[0]) == FIN).all(), what
        if poison == "inf_minus_inf":
            assert (cls(ref[1, mk["wave_row"]]) == NAN).all(), what
        if poison == "dup_inf":
            assert (cls(ref[1, mk["dup"][0][0]]) == NAN).all(), what
    return row, col, val, mk, x, ref


# ---------------------------------------------------------------------------------------------------------------- A3: time windows
def window_taps(T, H, stride=1, padl=0, padr=0, dil=1):
    """(nwin, t[w, h]): the time row of tap h of window w (outside 0 <= t < T: zero padding, an absent term)"""
    He = (H - 1) * dil + 1
    nwin = (T + padl + padr - He) // stride + 1
    assert nwin >= 1
    return nwin, np.arange(nwin)[:, None] * stride - padl + np.arange(H)[None, :] * dil


def windows_ref(stack, W, bias=None, stride=1, padl=0, padr=0, dil=1, reverse=False, einsum=False):
    """out[s, i, w, :] = sum_k sum_h sum_c stack[k, s, i, t(w, h), c] * W[k, h, c, :] (+ bias[i, :]); stack (K, S, n, T, f), W (K, H, f, N),
    taps outside the series are absent.  einsum=False: one term (k, h, c) after the other, in the given or the reversed order;
    einsum=True: the explicit window gather contracted by np.einsum (the padding as zeros: the weights are finite)."""
    stack, W = np.asarray(stack, np.float64), np.asarray(W, np.float64)
    K, S, n, T, f = stack.shape
    H, N = W.shape[1], W.shape[3]
    nwin, taps = window_taps(T, H, stride, padl, padr, dil)
    inside = (taps >= 0) & (taps < T)
    with np.errstate(invalid="ignore", over="ignore"):
        if einsum:
            g = np.where(inside[None, None, None, :, :, None], stack[:, :, :, np.clip(taps, 0, T - 1), :], 0.0)      # (K, S, n, nwin, H, f)
            out = np.einsum("ksiwhc,khcm->siwm", g, W)
        else:
            out = np.zeros((S, n, nwin, N))
            terms = [(k, h, c) for k in range(K) for h in range(H) for c in range(f)]
            for k, h, c in (terms[::-1] if reverse else terms):
                ws = np.nonzero(inside[:, h])[0]
                out[:, :, ws, :] += stack[k][:, :, taps[ws, h], c][..., None] * W[k, h, c]
        if bias is not None:
            out = out + np.asarray(bias, np.float64).reshape(1, n, 1, N)
    return out


def windows_touching(t, T, H, stride=1, padl=0, padr=0, dil=1):
    """bool[nwin]: the windows one of whose taps is time row t"""
    return (window_taps(T, H, stride, padl, padr, dil)[1] == t).any(axis=1)


SERIES_FH = [(1, 5), (1, 15), (2, 3), (3, 7), (5, 3), (4, 3), (8, 5)]      # every H*f mod 4 of the scalar-load form, and the 16-byte form
SERIES_T = 48
SERIES_POISON_T = {20: INF, 31: np.nan, 32: -INF, SERIES_T - 1: INF}       # inside a block, the block edge from both sides, the last row
POISON_AT = (1, 1, 2)                                                       # (term, recording, vertex) of the poisoned time row


def series_case(f, H, N, t, value, n=5, K=2, S=2, T=SERIES_T, stride=1, padl=0, padr=0, dil=1, seed=0, bf16=False):
    """(stack (K, S, n, T, f) float32, W (K, H, f, N), bias (n, N), ref (S, n, nwin, N), touched bool[nwin]) with time row t of POISON_AT set
    to value in every channel (value None: nothing is poisoned, for the cases that poison another operand).  Asserted: the conditions, that exactly the touched windows of that (recording, vertex) are non-finite, and
    that a clean window lies directly next to them."""
    rng = np.random.default_rng([seed, f, H, N, t % 1000, stride, dil, padl])
    vals = np.array([-1.5, -1.0, -0.75, -0.5, 0.5, 0.75, 1.0, 1.5], np.float32)
    stack = rng.choice(vals, (K, S, n, T, f)).astype(np.float32)
    W = rng.choice(vals, (K, H, f, N)).astype(np.float32)
    bias = rng.choice(vals, (n, N)).astype(np.float32)
    k, s, i = POISON_AT
    if value is not None:
        stack[k, s, i, t, :] = value
    what = "series f=%d H=%d N=%d t=%d stride=%d pads=(%d,%d) dil=%d" % (f, H, N, t, stride, padl, padr, dil)
    check_inputs(stack, W, bias)
    assert bf16_exact(stack) and bf16_exact(W) and bf16_exact(bias)
    ref = order_checked(lambda rev: windows_ref(stack, W, bias, stride, padl, padr, dil, reverse=rev), what)
    ein = windows_ref(stack, W, bias, stride, padl, padr, dil, einsum=True)
    assert np.array_equal(cls(ein), cls(ref)) and finite_err(ein, ref) <= 1e-12, what
    touched = windows_touching(t, T, H, stride, padl, padr, dil)
    if value is None:                                   # the clean twin of a case
        assert (cls(ref) == FIN).all(), what
        return stack, W, bias, ref, touched
    want = np.zeros(ref.shape[:3], bool)
    want[s, i, touched] = True
    assert np.array_equal((cls(ref) != FIN).any(axis=3), want) and np.array_equal((cls(ref) != FIN).all(axis=3), want), what
    check_coverage(ref, what, neighbour_axis=2)
    return stack, W, bias, ref, touched


def series_dgrad_ref(g, W, T, stride=1, padl=0, dil=1, reverse=False):
    """G[k, s, i, t, c] = sum over the (window w, tap h) pairs with t = w*stride - padl + h*dil of sum_m g[s, i, w, m] * W[k, h, c, m];
    g (S, n, nwin, N) -> (K, S, n, T, f).  Gradient that falls into the padding is dropped; a time row no window covers gets zero."""
    g, W = np.asarray(g, np.float64), np.asarray(W, np.float64)
    S, n, nwin, N = g.shape
    K, H, f, _ = W.shape
    G = np.zeros((K, S, n, T, f))
    terms = [(h, m) for h in range(H) for m in range(N)]
    with np.errstate(invalid="ignore", over="ignore"):
        for h, m in (terms[::-1] if reverse else terms):
            t = np.arange(nwin) * stride - padl + h * dil
            ws = np.nonzero((t >= 0) & (t < T))[0]
            G[:, :, :, t[ws], :] += g[None, :, :, ws, m, None] * W[:, h, :, m][:, None, None, None, :]
    return G


def series_wgrad_ref(stack, g, H, stride=1, padl=0, dil=1, reverse=False):
    """dW[k, h, c, m] = sum_{s, i, w} stack[k, s, i, w*stride - padl + h*dil, c] * g[s, i, w, m] over the taps inside the recording, one window w
    after the other (recordings and vertices of a window summed by einsum)"""
    stack, g = np.asarray(stack, np.float64), np.asarray(g, np.float64)
    K, T, f, nwin, N = stack.shape[0], stack.shape[3], stack.shape[4], g.shape[2], g.shape[3]
    dW = np.zeros((K, H, f, N))
    ws = range(nwin)[::-1] if reverse else range(nwin)
    with np.errstate(invalid="ignore", over="ignore"):
        for w in ws:
            t = w * stride - padl + np.arange(H) * dil
            hs = np.nonzero((t >= 0) & (t < T))[0]
            dW[:, hs] += np.einsum("ksihc,sim->khcm", stack[:, :, :, t[hs]], g[:, :, w])
    return dW


def ring_of(rows, head, ring_ld, fill=np.nan):
    """rows (K, S, n, C, f): the C time rows before a chunk, oldest first -> the ring (K, S, n, ring_ld) whose slot (head + j) mod C holds row
    j; the floats behind the C slots are `fill`"""
    K, S, n, C, f = rows.shape
    ring = np.full((K, S, n, ring_ld), fill, np.float32)
    for j in range(C):
        slot = (head + j) % C
        ring[..., slot * f:(slot + 1) * f] = rows[:, :, :, j]
    return ring


# ---------------------------------------------------------------------------------------------------------------- A4: relu + max-pool
def pool_rule(y, pool, relu=True):
    """THE rule, member by member: members ascending, the first maximum wins, a NaN takes over once and stays; then (relu) best > 0 ? best :
    (NaN ? NaN : 0).  y (q, n, F) -> (z (q, n/pool, F) float32, arg-max (q, n/pool, F) uint8)"""
    y = np.asarray(y)
    y = y if y.dtype == np.float64 else y.astype(np.float32)          # float64: a reference output is pooled; else the kernel's own type
    q, n, F = y.shape
    assert n % pool == 0
    z = np.empty((q, n // pool, F), y.dtype)
    idx = np.empty((q, n // pool, F), np.uint8)
    for b in range(q):
        for j in range(n // pool):
            for c in range(F):
                best, bi = y[b, j * pool, c], 0
                for m in range(1, pool):
                    v = y[b, j * pool + m, c]
                    if v > best or (v != v and best == best):
                        best, bi = v, m
                if relu:
                    best = best if best > 0 else (best if best != best else y.dtype.type(0.0))
                z[b, j, c], idx[b, j, c] = best, bi
    return z, idx


def pool_bwd_rule(gz, z, idx, pool, relu=True):
    """the gradient goes to the arg-max member and only there; with relu only where z > 0 (a NaN z passes nothing, as torch's relu)"""
    gz, z = np.asarray(gz, np.float32), np.asarray(z, np.float32)
    q, np_, F = z.shape
    gy = np.zeros((q, np_, pool, F), np.float32)
    with np.errstate(invalid="ignore"):
        g = np.where(z > 0, gz, np.float32(0.0)) if relu else gz
    b, j, c = np.meshgrid(np.arange(q), np.arange(np_), np.arange(F), indexing="ij")
    gy[b, j, idx.astype(np.int64), c] = g
    return gy.reshape(q, np_ * pool, F)


def pool_groups(pool):
    """the crafted groups of A4 as rows of `pool` members: (name, members)"""
    n, i = np.nan, INF
    base = {2: [("tie", [1.5, 1.5]), ("tie0", [0.0, 0.0]), ("neg", [-1.0, -0.5]), ("nan@0", [n, 2.0]), ("nan@1", [2.0, n]), ("nan-nan", [n, n]),
                ("-inf", [-i, -1.0]), ("-inf+", [-i, 0.75]), ("+inf", [0.5, i]), ("+inf-nan", [i, n]), ("-0", [-0.0, 0.0]), ("0-0", [0.0, -0.0]),
                ("-0neg", [-0.0, -1.0]), ("plain", [0.5, 1.0])],
            4: [("tie", [0.5, 1.5, 1.5, 1.0]), ("tie0", [0.0, -1.0, 0.0, 0.0]), ("neg", [-1.0, -0.5, -2.0, -0.5]), ("nan@0", [n, 2.0, 1.0, 3.0]),
                ("nan@1", [2.0, n, 1.0, 3.0]), ("nan@2", [2.0, 1.0, n, 3.0]), ("nan@3", [2.0, 1.0, 3.0, n]), ("nan-nan", [1.0, n, 2.0, n]),
                ("-inf", [-i, -1.0, -i, -2.0]), ("-inf+", [-1.0, -i, 0.75, 0.5]), ("+inf", [0.5, i, 1.0, i]), ("+inf-nan", [0.5, i, n, 1.0]),
                ("-0", [-0.0, 0.0, -0.0, 0.0]), ("0-0", [0.0, -0.0, -1.0, -0.0]), ("-0neg", [-1.0, -0.0, -2.0, -0.0]), ("plain", [0.5, 1.0, 0.25, -1.0])]}
    return base[pool]


def pool_input(pool, F, q=2):
    """y (q, G*pool, F): group g of sample 0 is crafted group g in every column; sample 1 holds the groups rotated by the column, so that one
    row of a kernel's tile sees different rules side by side"""
    groups = pool_groups(pool)
    G = len(groups)
    y = np.empty((q, G * pool, F), np.float32)
    for b in range(q):
        for g in range(G):
            for c in range(F):
                y[b, g * pool:(g + 1) * pool, c] = groups[(g + b * c) % G][1]
    return y


# ---------------------------------------------------------------------------------------------------------------- A2: projections
def project_ref(terms, W, bias=None, reverse=False):
    """out[m, :] = sum_t sum_c terms[t][m, c] * W[t, c, :] (+ bias[:]), one (t, c) term after the other"""
    W = np.asarray(W, np.float64)
    T, Kc, N = W.shape
    M = terms[0].shape[0]
    out = np.zeros((M, N))
    order = [(t, c) for t in range(T) for c in range(Kc)]
    with np.errstate(invalid="ignore", over="ignore"):
        for t, c in (order[::-1] if reverse else order):
            out += np.asarray(terms[t], np.float64)[:, c, None] * W[t, c]
        if bias is not None:
            out = out + np.asarray(bias, np.float64)
    return out


PROJECT_POISON_ROWS = (0, 64, 129)


def project_case(Kc, N, M=130, nterms=3, seed=0):
    """(terms [nterms x (M, Kc)] float32, W (nterms, Kc, N), bias (N,), ref): NaN at A[0][0][0], +Inf in the whole middle row 64 of term 2,
    -Inf at A[1][M-1][Kc-1]"""
    rng = np.random.default_rng([seed, Kc, N])
    vals = np.array([-1.5, -1.0, -0.75, -0.5, 0.5, 0.75, 1.0, 1.5], np.float32)
    terms = [rng.choice(vals, (M, Kc)).astype(np.float32) for _ in range(nterms)]
    W = rng.choice(vals, (nterms, Kc, N)).astype(np.float32)
    bias = rng.choice(vals, (N,)).astype(np.float32)
    terms[0][0, 0] = np.nan
    terms[2][64, :] = INF
    terms[1][M - 1, Kc - 1] = -INF
    what = "project Kc=%d N=%d" % (Kc, N)
    check_inputs(W, bias, *terms)
    assert bf16_exact(W) and all(bf16_exact(t) for t in terms)
    ref = order_checked(lambda rev: project_ref(terms, W, bias, reverse=rev), what)
    check_coverage(ref, what, neighbour_axis=0)
    rows = np.zeros(M, bool)
    rows[list(PROJECT_POISON_ROWS)] = True
    assert np.array_equal((cls(ref) != FIN).all(axis=1), rows) and np.array_equal((cls(ref) != FIN).any(axis=1), rows), what
    return terms, W, bias, ref


def project_large_case(Kc, N, M=130, nterms=3, seed=0):
    """the separate case of large FINITE inputs: row 7 of term 0 at 3.0e38 (inside the bf16 range) and row 100 of term 1 at FLT_MAX (bf16
    rounds it to Inf), the weights of every term at +-1e-3 so that each exact product and the whole sum stay finite: the reference output is
    finite everywhere"""
    rng = np.random.default_rng([seed, Kc, N, 1])
    vals = np.array([-1.5, -1.0, -0.75, -0.5, 0.5, 0.75, 1.0, 1.5], np.float32)
    terms = [rng.choice(vals, (M, Kc)).astype(np.float32) for _ in range(nterms)]
    W = (rng.choice(vals, (nterms, Kc, N)) * np.float32(1e-3)).astype(np.float32)
    terms[0][7, :] = np.float32(3.0e38)
    terms[1][100, :] = np.float32(FLT_MAX)
    ref = order_checked(lambda rev: project_ref(terms, W, None, reverse=rev), "project large Kc=%d N=%d" % (Kc, N))
    assert (cls(ref) == FIN).all() and np.abs(ref).max() < 0.5 * FLT_MAX      # fp32 can hold every partial sum in any order
    return terms, W, ref


MAPPED_NV, MAPPED_M = 200, 130


def mapped_case(Kc, N, seed=0, q=2):
    """a projection through a row map: tile row m is vertex rowmap[m] (130 of 200 vertices, permuted) -- its output row and its row in term
    0, which lies in the caller's labels (q, 200, Kc); terms 1 and 2 are compact (q, 130, Kc) and read at row m.  Poisons, sample 1 only:
    NaN at term 0 [rowmap[0]][0], +Inf in row 64 of term 2, -Inf at the last element of the last row of term 1, and NaN in a whole vertex of
    term 0 that the map does not name (it reaches nothing).  -> (terms, W (3, Kc, N), bias (N,), rowmap int32, ref (q, 130, N) by tile row)"""
    rng = np.random.default_rng([seed, Kc, N, 7])
    vals = np.array([-1.5, -1.0, -0.75, -0.5, 0.5, 0.75, 1.0, 1.5], np.float32)
    perm = rng.permutation(MAPPED_NV)
    rowmap, unmapped = perm[:MAPPED_M].astype(np.int32), int(perm[MAPPED_M])
    terms = [rng.choice(vals, (q, MAPPED_NV, Kc)).astype(np.float32)] + [rng.choice(vals, (q, MAPPED_M, Kc)).astype(np.float32) for _ in range(2)]
    W = rng.choice(vals, (3, Kc, N)).astype(np.float32)
    bias = rng.choice(vals, (N,)).astype(np.float32)
    terms[0][1, rowmap[0], 0] = np.nan
    terms[0][1, unmapped, :] = np.nan
    terms[2][1, 64, :] = INF
    terms[1][1, MAPPED_M - 1, Kc - 1] = -INF
    check_inputs(W, bias, *terms)
    assert bf16_exact(W) and all(bf16_exact(t) for t in terms)
    what = "mapped Kc=%d N=%d" % (Kc, N)
    ref = np.stack([order_checked(lambda rev: project_ref([terms[0][b][rowmap], terms[1][b], terms[2][b]], W, bias, reverse=rev), what) for b in range(q)])
    check_coverage(ref, what, neighbour_axis=1)
    rows = np.zeros((q, MAPPED_M), bool)
    rows[1, [0, 64, MAPPED_M - 1]] = True
    assert np.array_equal((cls(ref) != FIN).any(axis=2), rows), what
    return terms, W, bias, rowmap, ref
