"""cheb_series_relu_pool_chunked / F.cheb_time_windows_relu_pool_chunked (DESIGN.md 3.10 "Time chunks through the pooled epilogue"): the causal
layer walked time_chunk rows at a time through the streaming ring with relu, dropout and the vertex max-pool in the projection's epilogue.

  1. bit identity with the composition at the SAME time_chunk: y = forward_series(..., padding="causal", dilation=d, time_chunk=Tc), relu, the
     mask of F.dropout_keep_mask times scale, the max over pool groups in torch.  z, d series and dW torch.equal; d bias within TOL_GRAD (it is
     summed chunk by chunk: another order by design); two runs of the new call bit-identical in everything.
  2. the fp64 oracle on the materialised causal windows (O.tgcn_cheb_h_forward / O.cheb_time_conv_forward, O.layer_backward, the numpy mask of
     tests/test_dropout_mask.py): z within TOL, gradients within TOL_GRAD.  The pooled gradient is zero on the groups where fp32 cannot be
     expected to route as fp64 does -- a kept member within MARGIN of zero, or the two largest within MARGIN of each other -- decided from
     the fp64 values alone, before anything runs on the device; they are a fraction of a percent (asserted below 2 %).
  3. no vacuous pass: 40 % .. 98 % of z positive in every case, and at least one window crosses a chunk boundary.
  4. chunking changes neither z nor the mask: Tc = 64 (one chunk) against Tc = 1.
  5. the two C entries against the entries they are built from, bit for bit; refused calls leave the outputs untouched.
  6. NaN / Inf come out where the composition puts them; a reordered operand gives the composition's result and drops the same elements.
  7. the capability: the peak memory of a training step.

Shapes: S = 2, T = 23, K = 3; n = 38 at degree 12 with pool 2 (n = 2 mod 4: the last quad has two waves without a vertex) and n = 52 at degree 2
with pool 4; (H, d) in {(4, 2), (3, 1), (1, 1)}: ring 6, ring 2, no ring; f in {4, 3, 1}; g in {5, 40}: one Philox call per element, and the
quad path with more than one column tile; p in {0, 0.3}; bias and none; both layouts; both classes; the chunk lengths of
test_series_time_chunk.chunk_lengths -- below, at and above the ring, 16, and 64 (one chunk)."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cheb_oracle as O
from test_dropout_mask import keep_mask, scale_of
from test_hip_parity import _random_graph
from test_series_channels import TOL, TOL_GRAD, _dev, _to_series
from test_series_time_chunk import chunk_lengths
import test_series_dilation as D

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]

S_REC, T_ROWS, K_TERMS = 2, 23, D.K_TERMS
GRAPHS = {"dense38-pool2": (38, 12, 2), "sparse52-pool4": (52, 2, 4)}        # vertices, average degree, pool
GEOMS = [(4, 2), (3, 1), (1, 1)]                                             # (H, dilation): C = 6, 2 and no ring at all
SEED = (0x2468ACE << 32) | 0x13579BDF                                        # a 62-bit key with both halves set
P_DROP = 0.3
MARGIN = 1e-4            # of max |y|: ten times the output bound -- closer than that, fp32 and fp64 may pick another arg-max or another sign


def test_the_shapes_hit_what_they_are_here_for():
    assert 38 % 4 == 2 and 38 % 2 == 0 and 52 % 4 == 0 and 0 < SEED < 2 ** 62 and SEED >> 32 and SEED & 0xFFFFFFFF
    assert chunk_lengths(4, 2) == [1, 6, 7, 16, 64] and chunk_lengths(3, 1) == [1, 2, 3, 16, 64] and chunk_lengths(1, 1) == [1, 16, 64]
    assert 5 % 4 and 40 % 4 == 0 and 40 > 32               # per-element Philox; the quad path, NT = 4 with a ragged last tile


def _params(cls, graph, f, g, H, seed):
    """graph, weight and bias from numpy alone, so that the fp64 side of a case can be formed without a device"""
    n, deg, pool = GRAPHS[graph]
    rng = np.random.default_rng(seed)
    row, col, val = _random_graph(n, deg, rng)
    val = val * 0.4
    bound = 1.0 / np.sqrt(f * K_TERMS)
    W = rng.uniform(-bound, bound, (K_TERMS, H, f, g)).astype(np.float32)
    bias = rng.uniform(-0.5, 0.5, (1, n, g) if cls == "TGCNCheb_H" else (g,)).astype(np.float32) * np.float32(0.2)
    return n, pool, row, col, val, W, bias


class Setup:
    """one class on one graph: the layer, its operand, the new call, the composition's layer call and the fp64 references"""

    def __init__(self, cls, graph, f, g, H, seed):
        import tgcn_amd
        from tgcn_amd import functional as F
        n, pool, row, col, val, W, bias = _params(cls, graph, f, g, H, seed)
        self.cls, self.F, self.n, self.pool, self.reordered = cls, F, n, pool, None
        if cls == "TGCNCheb_H":
            self.L = O.coo_to_csr(row, col, val, n)
            self.op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val))
            self.layer = tgcn_amd.TGCNCheb_H(self.op, f, g, K_TERMS, H).cuda()
            self.extra = ()
            self.mode, self.fmode, self.bias_kind = "power", F.MODE_POWER, F.BIAS_VERTEX_CHANNEL
            self.forward64 = lambda xw, b: O.tgcn_cheb_h_forward(self.L, xw, self.W64(), b)
            self.bias_grad = lambda go: go.astype(np.float64).sum(axis=0, keepdims=True)
        else:
            ei = np.stack([row, col]).astype(np.int64)
            r, c, lap = O.edge_laplacian(ei, None, n)
            self.L = O.coo_to_csr(r, c, lap, n)
            self.layer = tgcn_amd.ChebTimeConv(f, g, K_TERMS, H).cuda()
            self.extra = (_dev(ei),)
            self.op = self.layer._operand(torch.empty(1, n, 1, device="cuda"), self.extra[0], None)
            self.mode, self.fmode, self.bias_kind = "chebyshev", F.MODE_CHEBYSHEV, F.BIAS_CHANNEL
            self.forward64 = lambda xw, b: O.cheb_time_conv_forward(xw, ei, None, self.W64(), b)
            self.bias_grad = lambda go: go.astype(np.float64).sum(axis=(0, 1))
        with torch.no_grad():
            self.layer.weight.copy_(_dev(W))
            self.layer.bias.copy_(_dev(bias))

    def W64(self):
        return self.layer.weight.detach().cpu().numpy()

    def _functional_args(self, s, kind, bias):
        op = self.op
        if kind is not None:
            if self.reordered is None:
                self.reordered = self.op.reordered(kind)
            op = self.reordered
        W = self.layer.weight if s.dim() == 4 else self.layer.weight.reshape(K_TERMS, self.layer.weight.shape[1], -1)
        return op, s, W, self.layer.bias.reshape(-1) if bias else None, self.bias_kind if bias else self.F.BIAS_NONE, self.fmode

    def fused(self, s, kind, bias, tc, p, as_series, d):
        """the new call: the module-level entry on the layer's own operand with its bias, the functional twin otherwise"""
        import tgcn_amd
        if kind is None and bias:
            return tgcn_amd.cheb_series_relu_pool_chunked(self.layer, s, *self.extra, time_chunk=tc, pool=self.pool, p=p, seed=SEED,
                                                          as_series=as_series, dilation=d)
        return self.F.cheb_time_windows_relu_pool_chunked(*self._functional_args(s, kind, bias), self.pool, tc, p=p, seed=SEED, as_series=as_series,
                                                          dilation=d)

    def layer_out(self, s, kind, bias, tc, as_series, d):
        kw = dict(as_series=as_series, padding="causal", dilation=d, time_chunk=tc)
        if kind is None and bias:
            return self.layer.forward_series(s, *self.extra, **kw)
        return self.F.cheb_time_windows(*self._functional_args(s, kind, bias), **kw)

    def composition(self, s, kind, bias, tc, p, as_series, d):
        """the chunked layer, relu, the mask from F.dropout_keep_mask times scale, the max over pool groups in torch -> (z, y, m)"""
        y = self.layer_out(s, kind, bias, tc, as_series, d)
        S, T, n, N, pool = S_REC, T_ROWS, self.n, y.shape[-1], self.pool
        t, m = torch.relu(y), None
        if p:
            _, scale = self.F.dropout_params(p)
            m = self.F.dropout_keep_mask(SEED, 0, S * T * n * N, p, "cuda").view(S, T, n, N).to(torch.float32) * scale
            m = m.permute(0, 2, 1, 3) if as_series else m.reshape(S * T, n, N)
            t = t * m
        if as_series:
            return t.reshape(S, n // pool, pool, T, N).max(dim=2).values, y, m
        return t.reshape(S * T, n // pool, pool, N).max(dim=2).values, y, m


def _run(su, series, gz, call):
    """(z, d series, dW, db) of one forward + backward; gz in z's layout.  A single channel is given as a 3-D series."""
    su.layer.zero_grad()
    st = _dev(series[..., 0] if series.shape[3] == 1 else series).requires_grad_(True)
    z = call(st)
    z.backward(_dev(gz))
    g = lambda t: None if t is None else t.detach().clone()
    return z.detach(), st.grad.reshape(series.shape).clone(), g(su.layer.weight.grad), g(su.layer.bias.grad)


def _oracle(su, series, H, d, bias, p, rng):
    """fp64: z, the pooled gradient gz (zero on the groups of the module docstring's rule 2), d series, dW, db -- window-major"""
    S, T, n, pool = S_REC, T_ROWS, su.n, su.pool
    left = (H - 1) * d
    xw = D.windows_dilated(series, H, d, left, 0).astype(np.float64)
    assert xw.shape[0] == S * T                                  # causal: a window for every time row
    y = su.forward64(xw, su.layer.bias.detach().cpu().numpy() if bias else None)
    N = y.shape[2]
    keep = keep_mask(SEED, np.arange(y.size, dtype=np.uint64), p).reshape(y.shape) if p else np.ones(y.shape, dtype=bool)
    scale = np.float64(scale_of(p)) if p else 1.0
    t = (np.maximum(y, 0.0) * np.where(keep, scale, 0.0)).reshape(S * T, n // pool, pool, N)
    z, arg = t.max(axis=2), t.argmax(axis=2)                      # argmax: the first maximum, as the kernels take it
    thr = MARGIN * np.abs(y).max()
    near_zero = (keep & (np.abs(y) < thr)).reshape(t.shape).any(axis=2)
    top2 = np.sort(t, axis=2)[:, :, -2:]
    tie = (top2[:, :, 1] > 0) & (top2[:, :, 1] - top2[:, :, 0] < thr * scale)
    stable = ~(near_zero | tie)
    assert stable.mean() > 0.98, stable.mean()
    gz = rng.standard_normal(z.shape).astype(np.float32) * stable
    gy = np.zeros(t.shape, dtype=np.float32)
    np.put_along_axis(gy, arg[:, :, None], (np.where(z > 0, gz, 0) * np.float32(scale)).astype(np.float32)[:, :, None], axis=2)
    gy = gy.reshape(y.shape)
    gxw, gW = O.layer_backward(su.L, xw, su.W64(), gy, su.mode)
    return z, gz, D.fold_dilated(gxw, S, T, d, left, 0), gW, su.bias_grad(gy)


def _window_major(z_series):
    S, m, T, N = z_series.shape
    return z_series.permute(0, 2, 1, 3).reshape(S * T, m, N)


@gpu
@pytest.mark.parametrize("cls", D.CLASSES)
@pytest.mark.parametrize("graph", sorted(GRAPHS))
@pytest.mark.parametrize("g", [5, 40])
@pytest.mark.parametrize("f", [4, 3, 1], ids=["f4", "f3", "single-channel"])
@pytest.mark.parametrize("H,d", GEOMS, ids=["H4_d2", "H3_d1", "H1"])
def test_values_and_gradients_vs_the_composition_and_the_oracle(H, d, f, g, graph, cls, gpu_device):
    su = Setup(cls, graph, f, g, H, seed=H + 7 * d + f + g)
    S, T, n, pool = S_REC, T_ROWS, su.n, su.pool
    rng = np.random.default_rng([T, H, d, f, g, n])
    series = rng.standard_normal((S, n, T, f)).astype(np.float32)
    chunks = chunk_lengths(H, d)
    assert H == 1 or any(tc < T for tc in chunks)               # 3. a window of (H-1)*d + 1 > 1 rows crosses a chunk boundary
    for p in (0.0, P_DROP):
        for bias in (True, False):
            z64, gz, gs, gW, gb = _oracle(su, series, H, d, bias, p, rng)
            frac64 = float((z64 > 0).mean())
            assert 0.40 <= frac64 <= 0.98, frac64
            gz_s = np.ascontiguousarray(_to_series(gz, S, T))
            by_tc = {}
            for tc in chunks:
                for lay in (False, True):
                    got = _run(su, series, gz_s if lay else gz, lambda s: su.fused(s, None, bias, tc, p, lay, d))
                    want = _run(su, series, gz_s if lay else gz, lambda s: su.composition(s, None, bias, tc, p, lay, d)[0])
                    again = _run(su, series, gz_s if lay else gz, lambda s: su.fused(s, None, bias, tc, p, lay, d))
                    z = got[0]
                    assert tuple(z.shape) == ((S, n // pool, T, g) if lay else (S * T, n // pool, g)) and z.is_contiguous()
                    tag = (p, bias, tc, lay)
                    # 1. the composition at the same Tc, and a second run
                    for a, b, c, what in zip(got, want, again, ("z", "d series", "dW", "db")):
                        if what == "db" and not bias:
                            assert a is None or not a.any()
                            continue
                        assert torch.equal(a, c), (tag, what, "two runs differ")
                        if what == "db":
                            e = rel_err(a.cpu().numpy(), b.cpu().numpy())
                            assert e <= TOL_GRAD, (tag, what, e)
                        else:
                            assert torch.equal(a, b), (tag, what, float((a - b).abs().max()))
                    # 2. the oracle
                    zw = (_window_major(z) if lay else z).cpu().numpy()
                    frac = float((zw > 0).mean())
                    e = dict(z=rel_err(zw, z64), ds=rel_err(got[1].cpu().numpy(), gs), dW=rel_err(got[2].cpu().numpy(), gW))
                    if bias:
                        e["db"] = rel_err(got[3].cpu().numpy().reshape(gb.shape), gb)
                    print(cls, graph, (H, d, f, g), "p", p, "bias" if bias else "no bias", "Tc", tc, "series" if lay else "windows", e,
                          "positive %.3f (fp64 %.3f)" % (frac, frac64))
                    assert 0.40 <= frac <= 0.98, (tag, frac)     # 3.
                    assert e.pop("z") <= TOL, tag
                    assert max(e.values()) <= TOL_GRAD, (tag, e)
                    if not lay:
                        by_tc[tc] = z
                    else:
                        assert torch.equal(_window_major(z), by_tc[tc]), tag        # one mask, one set of values for both layouts
            # 4. one chunk against chunks of one row
            a, b = by_tc[64].cpu().numpy(), by_tc[1].cpu().numpy()
            assert rel_err(a, b) <= TOL, (p, bias)
            if p:
                assert np.array_equal(a == 0, b == 0), (p, bias)           # zero in the same places
                m = keep_mask(SEED, np.arange(S * T * n * g, dtype=np.uint64), p).reshape(S * T, n // pool, pool, g)
                dropped_all = ~m.any(axis=2)                                # a group with every member dropped is zero at any Tc
                assert dropped_all.any() and not a[dropped_all].any() and not b[dropped_all].any()


# ---------------------------------------------------------------------------------------------------------------- one case, kept
ONE = (4, 2, 4, 40)        # H, d, f, g


@functools.lru_cache(maxsize=None)
def _one(cls):
    H, d, f, g = ONE
    su = Setup(cls, "sparse52-pool4", f, g, H, seed=5)
    rng = np.random.default_rng(11)
    series = rng.standard_normal((S_REC, su.n, T_ROWS, f)).astype(np.float32)
    return su, series, rng.standard_normal((S_REC * T_ROWS, su.n // su.pool, g)).astype(np.float32)


@gpu
@pytest.mark.parametrize("cls", D.CLASSES)
def test_the_one_sided_backwards_match_the_two_sided_one(cls, gpu_device):
    """a frozen layer and a series without grad: the gradients that remain are torch.equal to the full backward's"""
    su, series, gz = _one(cls)
    d = ONE[1]
    full = _run(su, series, gz, lambda s: su.fused(s, None, True, 7, P_DROP, False, d))
    su.layer.requires_grad_(False)
    try:
        frozen = _run(su, series, gz, lambda s: su.fused(s, None, True, 7, P_DROP, False, d))
    finally:
        su.layer.requires_grad_(True)
    assert frozen[2] is None and frozen[3] is None and torch.equal(frozen[0], full[0]) and torch.equal(frozen[1], full[1])
    su.layer.zero_grad()
    z = su.fused(_dev(series), None, True, 7, P_DROP, False, d)
    z.backward(_dev(gz))
    assert torch.equal(su.layer.weight.grad, full[2]) and torch.equal(su.layer.bias.grad, full[3])
    with torch.no_grad():       # no arg-max is stored without grad mode; the values do not depend on it
        assert torch.equal(su.fused(_dev(series), None, True, 7, P_DROP, False, d), full[0])


@gpu
@pytest.mark.parametrize("cls", D.CLASSES)
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
def test_nan_and_inf_come_out_where_the_composition_puts_them(as_series, cls, gpu_device):
    su, series, _ = _one(cls)
    d = ONE[1]
    x = series.copy()
    x[0, 5, 7, 1] = np.nan
    x[1, 30, 14, 2] = np.inf
    with torch.no_grad():
        z = su.fused(_dev(x), None, True, 5, 0.5, as_series, d)
        want, y, m = su.composition(_dev(x), None, True, 5, 0.5, as_series, d)
    # the case holds what it is here for: a +Inf of the layer's output that the mask drops (0 * Inf = NaN), one it keeps, NaN and finite values
    assert (torch.isposinf(y) & (m == 0)).any() and (torch.isposinf(y) & (m > 0)).any() and torch.isnan(y).any()
    assert torch.isnan(z).any() and torch.isposinf(z).any() and torch.isfinite(z).any()
    assert torch.equal(torch.isnan(z), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(z, nan=-1.0), torch.nan_to_num(want, nan=-1.0))


@gpu
@pytest.mark.parametrize("cls", D.CLASSES)
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
def test_a_reordered_operand_gives_the_composition_and_drops_the_same_elements(as_series, cls, gpu_device):
    su, series, gz = _one(cls)
    d = ONE[1]
    gzl = np.ascontiguousarray(_to_series(gz, S_REC, T_ROWS)) if as_series else gz
    for p in (0.0, P_DROP):
        got = _run(su, series, gzl, lambda s: su.fused(s, "degree", True, 7, p, as_series, d))
        assert su.reordered.perm is not None and not su.F.series_pool_is_fused(su.reordered)
        want = _run(su, series, gzl, lambda s: su.composition(s, "degree", True, 7, p, as_series, d)[0])
        plain = _run(su, series, gzl, lambda s: su.fused(s, None, True, 7, p, as_series, d))
        for a, b, what in zip(got[:3], want[:3], ("z", "d series", "dW")):
            assert torch.equal(a, b), (p, what)
        assert rel_err(got[3].cpu().numpy(), want[3].cpu().numpy()) <= TOL_GRAD
        assert rel_err(got[0].cpu().numpy(), plain[0].cpu().numpy()) <= TOL
        if p:
            m = keep_mask(SEED, np.arange(S_REC * T_ROWS * su.n * ONE[3], dtype=np.uint64), p).reshape(S_REC * T_ROWS, su.n // su.pool, su.pool, ONE[3])
            zw = (_window_major(got[0]) if as_series else got[0]).cpu().numpy()
            assert (~m.any(axis=2)).any() and not zw[~m.any(axis=2)].any()


# ---------------------------------------------------------------------------------------------------------------- the C ABI directly
def _rows(t, as_series, S, T):
    """(S, vertices, T, N) view of a tensor in either layout"""
    return t if as_series else t.view(S, T, t.shape[1], t.shape[2]).permute(0, 2, 1, 3)


@gpu
@pytest.mark.parametrize("f,N", [(4, 24), (3, 5)], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("H,d", GEOMS, ids=["H4_d2", "H3_d1", "H1"])
@pytest.mark.parametrize("n,pool", [(38, 2), (52, 4)])
def test_entry_one_against_the_entries_it_is_built_from(n, pool, H, d, f, N, gpu_device):
    """seed NULL: torch.equal to tgcn_cheb_project_series_stream_pool_f32 on the same stack and ring, NaN-filled rows outside
    [out_t0, out_t0 + Tc) untouched, the same ring afterwards.  With a seed: z and idx equal tgcn_relu_dropout_pool_f32 applied to the
    _stream_at entry's rows embedded at out_t0 in a whole output."""
    from tgcn_amd import _lib
    from tgcn_amd import functional as F
    L = _lib.lib()
    S, Tc, K, T, t0 = 2, 7, 3, 23, 11
    Cr = (H - 1) * d
    gen = torch.Generator(device="cuda").manual_seed(H * 10 + f + n)
    stack = torch.randn((K, S, n, Tc * f), device="cuda", generator=gen)
    W, bias = torch.randn((K, H * f, N), device="cuda", generator=gen), torch.randn((N,), device="cuda", generator=gen)
    ring0, head = (torch.randn((K, S, n, Cr * f), device="cuda", generator=gen), Cr - 1) if Cr else (None, 0)
    args = (_lib.stream_ptr(), S, n, Tc, f, H, N, K, _lib.ptr(stack), _lib.ptr(W), _lib.ptr(bias), 1)
    ref, ring_ref = torch.full((S, n // pool, Tc, N), float("nan"), device="cuda"), (ring0.clone() if Cr else None)
    _lib.check(L.tgcn_cheb_project_series_stream_pool_f32(*args, _lib.ptr(ref), pool, _lib.ptr(ring_ref), Cr * f, head, None, d))
    assert not torch.isnan(ref).any() and (ref == 0).any() and (ref > 0).any()
    thr, scale = F.dropout_params(0.5)
    seed_t = torch.tensor([SEED], dtype=torch.int64, device="cuda")
    for as_series in (1, 0):
        shape = (S, n // pool, T, N) if as_series else (S * T, n // pool, N)
        z, idx, ring = torch.full(shape, float("nan"), device="cuda"), torch.full(shape, 9, dtype=torch.uint8, device="cuda"), (ring0.clone() if Cr else None)
        _lib.check(L.tgcn_cheb_project_series_stream_pool_at_f32(*args, _lib.ptr(z), _lib.ptr(idx), pool, T, t0, as_series, _lib.ptr(ring), Cr * f, head,
                                                                 d, None, 0, 1.0))
        rows, irows = _rows(z, as_series, S, T), _rows(idx, as_series, S, T)
        assert torch.equal(rows[:, :, t0:t0 + Tc], ref), as_series
        assert torch.isnan(rows[:, :, :t0]).all() and torch.isnan(rows[:, :, t0 + Tc:]).all()
        assert (irows[:, :, :t0] == 9).all() and (irows[:, :, t0 + Tc:] == 9).all() and (irows[:, :, t0:t0 + Tc] < pool).all()
        assert Cr == 0 or torch.equal(ring, ring_ref)
        # with a seed: the _stream_at entry's rows inside a whole output, then the stand-alone relu + dropout + pool pass
        yshape = (S, n, T, N) if as_series else (S * T, n, N)
        y, ring_y = torch.zeros(yshape, device="cuda"), (ring0.clone() if Cr else None)
        _lib.check(L.tgcn_cheb_project_series_stream_at_f32(*args, _lib.ptr(y), T, t0, as_series, _lib.ptr(ring_y), Cr * f, head, d))
        zr, ir = torch.empty(shape, device="cuda"), torch.empty(shape, dtype=torch.uint8, device="cuda")
        q, fN = (S, T * N) if as_series else (S * T, N)
        _lib.check(L.tgcn_relu_dropout_pool_f32(_lib.stream_ptr(), _lib.ptr(y), _lib.ptr(zr), _lib.ptr(ir), q, n, fN, pool, N, _lib.ptr(seed_t), thr, scale))
        z2, idx2, ring2 = torch.full(shape, float("nan"), device="cuda"), torch.full(shape, 9, dtype=torch.uint8, device="cuda"), (ring0.clone() if Cr else None)
        _lib.check(L.tgcn_cheb_project_series_stream_pool_at_f32(*args, _lib.ptr(z2), _lib.ptr(idx2), pool, T, t0, as_series, _lib.ptr(ring2), Cr * f, head,
                                                                 d, _lib.ptr(seed_t), thr, scale))
        got, want = _rows(z2, as_series, S, T)[:, :, t0:t0 + Tc], _rows(zr, as_series, S, T)[:, :, t0:t0 + Tc]
        assert torch.equal(got, want) and not torch.equal(got, ref), as_series
        assert torch.equal(_rows(idx2, as_series, S, T)[:, :, t0:t0 + Tc], _rows(ir, as_series, S, T)[:, :, t0:t0 + Tc]), as_series
        assert torch.isnan(_rows(z2, as_series, S, T)[:, :, :t0]).all() and torch.isnan(_rows(z2, as_series, S, T)[:, :, t0 + Tc:]).all()
        assert Cr == 0 or torch.equal(ring2, ring_ref)


@gpu
@pytest.mark.parametrize("as_series", [0, 1], ids=["window-major", "series"])
@pytest.mark.parametrize("n,pool,N", [(38, 2, 5), (52, 4, 40)])
def test_entry_two_is_the_rows_of_the_whole_routing(n, pool, N, as_series, gpu_device):
    from tgcn_amd import _lib
    L = _lib.lib()
    S, T = 2, 23
    gen = torch.Generator(device="cuda").manual_seed(n + N + as_series)
    shape, yshape = ((S, n // pool, T, N), (S, n, T, N)) if as_series else ((S * T, n // pool, N), (S * T, n, N))
    z = torch.relu(torch.randn(shape, device="cuda", generator=gen))
    gz = torch.randn(shape, device="cuda", generator=gen)
    idx = torch.randint(0, pool, shape, device="cuda", generator=gen).to(torch.uint8)
    q, fN = (S, T * N) if as_series else (S * T, N)
    for scale in (1.0, 1.4285714626312256):
        whole = torch.full(yshape, float("nan"), device="cuda")
        _lib.check(L.tgcn_relu_pool_bwd_f32(_lib.stream_ptr(), _lib.ptr((gz * scale).contiguous()), _lib.ptr(z), _lib.ptr(idx), _lib.ptr(whole), q, n, fN, pool))
        assert (whole == 0).any() and (whole != 0).any() and not torch.isnan(whole).any()
        for t0, rows in ((0, 1), (0, T), (5, 9), (T - 3, 3), (22, 1)):
            slab = torch.full((S, n, rows, N) if as_series else (S * rows, n, N), float("nan"), device="cuda")
            _lib.check(L.tgcn_relu_pool_bwd_rows_f32(_lib.stream_ptr(), _lib.ptr(gz), _lib.ptr(z), _lib.ptr(idx), _lib.ptr(slab), S, n, T, t0, rows, N, pool,
                                                     as_series, scale))
            assert torch.equal(_rows(slab, as_series, S, rows), _rows(whole, as_series, S, T)[:, :, t0:t0 + rows]), (scale, t0, rows)


@gpu
def test_refused_calls_launch_nothing(gpu_device):
    """an error code through the C ABI, the outputs untouched"""
    from tgcn_amd import _lib
    L = _lib.lib()
    n, S, T, Tc, f, H, N, K, d, pool = 12, 1, 30, 6, 4, 3, 8, 2, 2, 4
    stack, W = torch.zeros(K, S, n, Tc * f, device="cuda"), torch.zeros(K, H * f, N, device="cuda")
    ring = torch.zeros(K, S, n, 4 * f, device="cuda")
    z, idx = torch.full((S, n // pool, T, N), float("nan"), device="cuda"), torch.full((S, n // pool, T, N), 9, dtype=torch.uint8, device="cuda")
    seed_t = torch.tensor([SEED], dtype=torch.int64, device="cuda")
    at = lambda out_t0=0, head=0, pl=pool, scale=2.0, seed=seed_t: L.tgcn_cheb_project_series_stream_pool_at_f32(
        _lib.stream_ptr(), S, n, Tc, f, H, N, K, _lib.ptr(stack), _lib.ptr(W), None, 0, _lib.ptr(z), _lib.ptr(idx), pl, T, out_t0, 1, _lib.ptr(ring), 4 * f,
        head, d, _lib.ptr(seed), 1 << 31, scale)
    assert at(out_t0=25) == -1 and at(head=4) == -1 and at(pl=3) == -1 and at(pl=8) == -1 and at(scale=0.5) == -1      # TGCN_ERR_INVALID
    assert at(out_t0=25, seed=None) == -1 and at(head=4, seed=None) == -1
    gy = torch.full((S, n, 5, N), float("nan"), device="cuda")
    gz = torch.zeros(S, n // pool, T, N, device="cuda")
    rw = lambda t0=0, rows=5, pl=pool, scale=1.0: L.tgcn_relu_pool_bwd_rows_f32(_lib.stream_ptr(), _lib.ptr(gz), _lib.ptr(gz), _lib.ptr(idx), _lib.ptr(gy), S, n,
                                                                               T, t0, rows, N, pl, 1, scale)
    assert rw(t0=26) == -1 and rw(t0=-1) == -1 and rw(rows=0) == -1 and rw(pl=5) == -1 and rw(scale=float("nan")) == -1
    torch.cuda.synchronize()
    assert torch.isnan(z).all() and (idx == 9).all() and torch.isnan(gy).all() and not ring.any()


# ---------------------------------------------------------------------------------------------------------------- the capability: peak memory
@gpu
def test_a_chunked_pooled_training_step_holds_a_quarter_of_the_output(gpu_device):
    """n = 4096 (sparse), S = 1, T = 512, f = 1, N = 32, K = 8, H = 3, d = 1, time_chunk = 32, pool 4, p = 0.1, forward + backward with all three
    gradients.  Y = 4 S n T N bytes is the layer's full output, 268 MB; the series is Y / 32.
    Both existing forms hold Y or more above a baseline that already counts the series: the fused unchunked call allocates the output's
    gradient gy (Y) in its backward, next to the hop stack and G; forward_series(time_chunk=32) followed by the pool pass allocates the
    output (Y) and its gradient.
    The new call holds z (Y / 4), idx (Y / 16), gz (Y / 4) and d series (Y / 32), which any form of the step must, and beyond them only
    chunk-sized buffers: one slab of Tc + C = 34 of 512 rows of the output's gradient, 34 / 512 Y = 0.066 Y; one chunk stack and one chunk G
    of K S n Tc f floats = Y / 64 each, 0.031 Y together; the ring, the working weight and the hops' chunk-sized workspaces and temporaries, a
    few chunk tensors of S n Tc f floats = Y / 512 each -- about 0.1 Y.  The condition, peak - bytes(z, idx, gz, d series) < Y / 4, is
    derived, not measured."""
    import tgcn_amd
    from tgcn_amd import functional as F
    n, S, T, f, N, K, H, Tc, pool, p = 4096, 1, 512, 1, 32, 8, 3, 32, 4, 0.1
    rng = np.random.default_rng(0)
    row, col, val = _random_graph(n, 4, rng)
    op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val * 0.2))
    layer = tgcn_amd.TGCNCheb_H(op, f, N, K, H).cuda()
    x = torch.randn(S, n, T, f, device="cuda", requires_grad=True)
    thr, scale = F.dropout_params(p)
    seed_t = torch.tensor([SEED], dtype=torch.int64, device="cuda")
    Y = 4 * S * n * T * N
    assert Y == 268435456

    forms = {
        "fused, unchunked": lambda: tgcn_amd.cheb_series_relu_dropout_pool(layer, x, p=p, pool=pool, seed=seed_t, as_series=True, padding="causal"),
        "chunked, then the pool pass": lambda: F.ReluDropoutPoolFn.apply(
            layer.forward_series(x, as_series=True, padding="causal", time_chunk=Tc).reshape(S, n, T * N), pool, N, seed_t, thr, scale).view(S, n // pool, T, N),
        "chunked and pooled": lambda: tgcn_amd.cheb_series_relu_pool_chunked(layer, x, time_chunk=Tc, pool=pool, p=p, seed=seed_t, as_series=True),
    }

    def step(form):
        layer.zero_grad(set_to_none=True)
        x.grad = None
        z = form()
        assert tuple(z.shape) == (S, n // pool, T, N)
        z.backward(torch.ones_like(z))
        assert x.grad is not None and layer.weight.grad is not None and layer.bias.grad is not None
        del z

    peaks = {}
    for name, form in forms.items():
        step(form)                                                       # warm-up: the operand's schedules and transpose are built and cached
        layer.zero_grad(set_to_none=True)
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(form)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
    held = Y // 4 + Y // 16 + Y // 4 + Y // 32                           # z, idx, gz, d series
    print({k: round(v / Y, 4) for k, v in peaks.items()}, "in units of the full output's bytes; z + idx + gz + d series = %.4f" % (held / Y))
    assert peaks["fused, unchunked"] >= Y and peaks["chunked, then the pool pass"] >= Y, peaks
    assert peaks["chunked and pooled"] - held < Y // 4, (peaks, held)
