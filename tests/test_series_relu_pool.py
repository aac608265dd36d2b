"""relu + vertex max-pool as the epilogue of the streaming time-window layers (cheb_series_relu_pool / cheb_stream_relu_pool, DESIGN.md 3.10
"relu + pool epilogue"), on the 48-vertex random graph of tests/test_series_dilation.py, both classes, K = 3.

  1. bitwise: z and the arg-max bytes are torch.equal to tgcn_relu_pool_f32 applied to forward_series(..., as_series=True) of the same
     geometry (transposed for the window-major layout) -- pool 2 and 4, f in {4, 3, one channel}, N in {5, 40, 72}, with and without a
     bias, three geometries at T = 23 (a tail block) and T = 70 (three window blocks, the last partial); a 50-vertex graph at pool 2 (waves
     without a vertex in the last quad); H = 1, f = 1, N = 40 (the scratch larger than the GEMM's LDS); the horizon staged in chunks.
  2. oracle: z within 1e-5 of max|.| of relu + pool of the fp64 oracle on the materialised windows (a max is 1-Lipschitz, so the project's
     output bound carries over).
  3. gradients: torch.equal to those of the hand-written composition (the same gy through the same, bit-reproducible kernels), and within
     2e-5 of the fp64 oracle's backward fed with gz routed through the GPU's arg-max and z > 0; one-sided backwards.
  4. a reordered operand (the unfused route) against the plain one, 1e-5.
  5. streaming: chunk by chunk torch.equal to tgcn_relu_pool_f32 of forward_stream on a twin state, the rings equal; host-head against
     capturable twins; pooled and unpooled steps alternating on one state; a two-layer chain through GraphedStream.
  6. memory: the peak above the pre-call level stays below the bytes of the unpooled output, which is never allocated."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cheb_oracle as O
from test_hip_parity import _random_graph
from test_series_channels import TOL, TOL_GRAD, _dev, _to_series
from test_series_dilation import CLASSES, K_TERMS, N_VERT, S_REC, Setup, _reference, nwin_of, padding_arg
from test_series_stream import edge_index_of

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]

H_TAPS = 5
T_LENS = (23, 70)
# (kwargs, (stride, left, right, dilation)) at H = 5
GEOS = [(dict(), (1, 0, 0, 1)), (dict(stride=2, padding=1), (2, 1, 1, 1)), (dict(padding="causal", dilation=2), (1, 8, 0, 2))]


def _nwin(T, H, geo):
    stride, left, right, dil = geo
    return (T + left + right - (H - 1) * dil - 1) // stride + 1


def test_the_shapes_hit_what_they_are_here_for():
    assert _nwin(23, H_TAPS, GEOS[0][1]) == 19 and _nwin(70, H_TAPS, GEOS[0][1]) == 66          # one tail block; 32 + 32 + 2
    assert _nwin(23, H_TAPS, GEOS[1][1]) == 11 and _nwin(70, H_TAPS, GEOS[1][1]) == 34          # with a step: 32 + 2
    assert _nwin(70, H_TAPS, GEOS[2][1]) == 70                                                  # two phases of 35 windows: 32 + 3 each
    assert N_VERT % 4 == 0 and 50 % 4 == 2 and 50 % 2 == 0


def relu_pool(y, pool):
    """tgcn_relu_pool_f32 on a (S, n, nwin, N) layer output through its (S, n, nwin*N) view -> (z, idx), both (S, n/pool, nwin, N)"""
    from tgcn_amd import _lib
    S, n, nwin, N = y.shape
    y = y.contiguous()
    z = torch.full((S, n // pool, nwin, N), float("nan"), device="cuda")
    idx = torch.full((S, n // pool, nwin, N), 255, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().tgcn_relu_pool_f32(_lib.stream_ptr(), _lib.ptr(y), _lib.ptr(z), _lib.ptr(idx), S, n, nwin * N, pool))
    return z, idx


def window_major(z):
    """(S, m, nwin, N) -> (S*nwin, m, N)"""
    S, m, nwin, N = z.shape
    return z.permute(0, 2, 1, 3).reshape(S * nwin, m, N)


class Pooler:
    """cheb_series_relu_pool on the layer's own operand with its bias; F.cheb_time_windows_relu_pool for no bias or another operand"""

    def __init__(self, su, seed):
        self.su = su
        self.extra = () if su.cls == "TGCNCheb_H" else (edge_index_of(seed), None)

    def weight(self, s):
        W = self.su.layer.weight
        return W if s.dim() == 4 else W.reshape(K_TERMS, W.shape[1], -1)

    def fused(self, s, pool, bias=True, op=None, **kw):
        import tgcn_amd
        su = self.su
        if bias and op is None:
            return tgcn_amd.cheb_series_relu_pool(su.layer, s, *self.extra, pool=pool, **kw)
        return su.F.cheb_time_windows_relu_pool(op or su.op, s, self.weight(s), su.layer.bias.reshape(-1) if bias else None,
                                                su.bias_kind if bias else su.F.BIAS_NONE, su.fmode, pool, **kw)

    def layer_out(self, s, bias=True, **kw):
        """forward_series (the module with its bias, the functional entry without)"""
        return self.su.call(s, None, bias, **kw)

    def composition(self, s, pool, as_series, bias=True, **kw):
        """what a caller writes by hand: gcn_pool_4(relu(out).view(S, n, -1))"""
        import tgcn_amd
        pool_fn = tgcn_amd.gcn_pool_4 if pool == 4 else tgcn_amd.gcn_pool
        out = self.layer_out(s, bias, as_series=as_series, **kw)
        if not as_series:
            return pool_fn(torch.relu(out))
        S, n, nwin, N = out.shape
        return pool_fn(torch.relu(out).view(S, n, -1)).view(S, n // pool, nwin, N)


def _series(S, n, T, f, seed):
    x = torch.randn(S, n, T, f, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    return x[..., 0].contiguous() if f == 1 else x


def _saved_idx(z):
    """the arg-max bytes the fused forward kept for its backward"""
    idx = z.grad_fn.saved_tensors[2]
    assert idx.dtype == torch.uint8 and idx.shape == z.shape
    return idx


def _assert_bitwise(po, x, pool, bias, kw, tag):
    with torch.no_grad():
        z_ref, idx_ref = relu_pool(po.layer_out(x, bias, as_series=True, **kw), pool)
    assert not torch.isnan(z_ref).any() and int(idx_ref.max()) < pool and (z_ref > 0).any() and (z_ref == 0).any(), tag
    z_s = po.fused(x, pool, bias, as_series=True, **kw)
    assert z_s.is_contiguous() and torch.equal(z_s, z_ref), tag
    assert torch.equal(_saved_idx(z_s), idx_ref), tag
    z_w = po.fused(x, pool, bias, **kw)
    assert z_w.is_contiguous() and torch.equal(z_w, window_major(z_ref)), tag
    assert torch.equal(_saved_idx(z_w), window_major(idx_ref)), tag
    with torch.no_grad():           # without grad mode no arg-max is stored; the values do not depend on it
        assert torch.equal(po.fused(x, pool, bias, as_series=True, **kw), z_ref), tag


# ---------------------------------------------------------------------------------------------------------------- 1. bitwise
@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("N", [5, 40, 72])
@pytest.mark.parametrize("f", [4, 3, 1])
def test_fused_equals_relu_pool_of_the_layer_bit_for_bit(f, N, cls, gpu_device):
    """every pool, bias, geometry and length for one (f, N, class): NT = 1 / 4 / 4 with two column blocks at N = 72"""
    su = Setup(cls, f, N, H_TAPS, seed=f + N)
    po = Pooler(su, f + N)
    for T in T_LENS:
        x = _series(S_REC, N_VERT, T, f, T + f)
        for kw, geo in GEOS:
            for pool in (2, 4):
                for bias in (True, False):
                    _assert_bitwise(po, x, pool, bias, kw, (T, kw, pool, bias))


def _layer_on(cls, n, f, g, H, seed, K=K_TERMS):
    """Setup's construction on a graph of n vertices -> (layer, graph arguments of the module calls)"""
    import tgcn_amd
    row, col, val = _random_graph(n, 6, np.random.default_rng(seed), hubs=((2, n - 1),))
    torch.manual_seed(seed)
    if cls == "TGCNCheb_H":
        layer, extra = tgcn_amd.TGCNCheb_H(tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val * 0.4)), f, g, K, H).cuda(), ()
    else:
        layer, extra = tgcn_amd.ChebTimeConv(f, g, K, H).cuda(), (_dev(np.stack([row, col]).astype(np.int64)), None)
    with torch.no_grad():
        layer.bias.uniform_(-0.5, 0.5)
    return layer, extra


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("f,N", [(4, 40), (3, 5)])
def test_fifty_vertices_at_pool_two_leave_two_waves_of_the_last_quad_without_a_vertex(f, N, cls, gpu_device):
    import tgcn_amd
    n = 50
    layer, extra = _layer_on(cls, n, f, N, H_TAPS, seed=50 + f)
    for T in T_LENS:
        x = _series(S_REC, n, T, f, T)
        for kw, geo in GEOS:
            with torch.no_grad():
                z_ref, idx_ref = relu_pool(layer.forward_series(x, *extra, as_series=True, **kw), 2)
            z = tgcn_amd.cheb_series_relu_pool(layer, x, *extra, pool=2, as_series=True, **kw)
            assert tuple(z.shape) == (S_REC, 25, _nwin(T, H_TAPS, geo), N)
            assert torch.equal(z, z_ref) and torch.equal(_saved_idx(z), idx_ref), (T, kw)
            z = tgcn_amd.cheb_series_relu_pool(layer, x, *extra, pool=2, **kw)
            assert torch.equal(z, window_major(z_ref)) and torch.equal(_saved_idx(z), window_major(idx_ref)), (T, kw)
    with pytest.raises(tgcn_amd._lib.TgcnError, match="not a multiple of pool"):
        tgcn_amd.cheb_series_relu_pool(layer, x, *extra, pool=4)


def _plans(H, f, N, pool=4):
    from tgcn_amd import _lib
    L = _lib.lib()
    out = []
    for q in (lambda *a: L.tgcn_series_conv_plan(H, f, N, int(f % 4 == 0), 1, *a), lambda *a: L.tgcn_series_pool_plan(H, f, N, int(f % 4 == 0), 1, pool, *a)):
        hc, lds = C.c_int32(-1), C.c_int32(-1)
        assert q(C.byref(hc), C.byref(lds)) == 0
        out.append((hc.value, lds.value))
    return out


@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_one_tap_of_one_channel_where_the_scratch_is_larger_than_the_gemms_lds(cls, gpu_device):
    (hc0, lds0), (hc1, lds1) = _plans(1, 1, 40)
    assert hc0 == hc1 == 1 and lds0 < 12 * 1024 and lds1 == 4 * 32 * 64 * 4 > lds0
    su = Setup(cls, 1, 40, 1, seed=41)
    po = Pooler(su, 41)
    for T in T_LENS:
        x = _series(S_REC, N_VERT, T, 1, T)
        for pool in (2, 4):
            for bias in (True, False):
                _assert_bitwise(po, x, pool, bias, {}, (T, pool, bias))


# H = 15, f = 72: the last horizon whose four spans fit 64 KB whole (64 704 B, what the plan answers); H = 16: staged in chunks of 15 rows
@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("H", [15, 16])
def test_a_wide_horizon_whole_and_staged_in_chunks(H, cls, gpu_device):
    (hc0, lds0), (hc1, lds1) = _plans(H, 72, 40)
    assert hc0 == hc1 and lds0 == lds1 <= 64 * 1024 and lds0 > 32 * 1024          # the scratch never changes the regime
    assert hc1 == 15, "H = 16 is here for the chunked regime (HC < H), H = 15 for the largest whole one; the plan answers HC = %d" % hc1
    su = Setup(cls, 72, 40, H, seed=H)
    po = Pooler(su, H)
    x = _series(S_REC, N_VERT, 40, 72, H) * 0.25
    for kw in ({}, dict(padding="causal", dilation=2)):
        for pool in (2, 4):
            _assert_bitwise(po, x, pool, True, kw, (kw, pool))


# ---------------------------------------------------------------------------------------------------------------- 2. / 3. oracle, gradients
# (T, H, d, f, g, left, right) of tests/test_series_dilation.py's helpers
ORACLE = [(23, 5, 1, 4, 40, 0, 0), (70, 5, 2, 3, 5, 8, 0), (50, 5, 3, 1, 72, 2, 5)]


@functools.lru_cache(maxsize=None)
def _oracle_case(cls, shape):
    T, H, d, f, g, left, right = shape
    su = Setup(cls, f, g, H, seed=T + d)
    ref = _reference(su, T, H, f, g, d, left, right, np.random.default_rng([T, d, f]))      # series, go, ref_b, ref_0, gs, gW, gb
    return su, Pooler(su, T + d), ref


def _pool64(y, pool):
    """relu + pool in fp64 on a window-major (q, n, g) array"""
    q, n, g = y.shape
    return np.maximum(y.reshape(q, n // pool, pool, g).max(axis=2), 0.0)


def _route(gz, z, idx, pool):
    """the gradient w.r.t. the layer output from gz by the GPU's own choices: to the arg-max member where z > 0; window-major (q, m, g)"""
    q, m, g = gz.shape
    gy = np.zeros((q, m, pool, g))
    np.put_along_axis(gy, idx[:, :, None, :].astype(np.int64), (gz * (z > 0))[:, :, None, :], axis=2)
    return gy.reshape(q, m * pool, g)


def _grads(su, x, run):
    """(z, d series, dW, db) of one forward + backward; run(series tensor) -> (z, gz)"""
    su.layer.zero_grad()
    z, gz = run(x)
    z.backward(gz)
    g = lambda t: None if t is None else t.clone()
    return z.detach(), g(x.grad), g(su.layer.weight.grad), g(su.layer.bias.grad)


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("pool", [2, 4])
@pytest.mark.parametrize("shape", ORACLE, ids=lambda s: "T%d_H%d_d%d_f%d_g%d_l%d_r%d" % s)
def test_values_and_gradients_vs_the_composition_and_the_oracle(shape, pool, cls, gpu_device):
    T, H, d, f, g, left, right = shape
    su, po, (series, go, ref_b, ref_0, _, _, _) = _oracle_case(cls, shape)
    S, n, nwin = S_REC, N_VERT, nwin_of(T, H, d, left, right)
    m = n // pool
    kw = dict(padding=padding_arg(H, d, left, right), dilation=d)
    from test_series_dilation import fold_dilated, windows_dilated
    xw = windows_dilated(series, H, d, left, right).astype(np.float64)
    gz_w = np.random.default_rng([T, pool]).standard_normal((S * nwin, m, g)).astype(np.float32)
    for as_series in (False, True):
        gz = _dev(np.ascontiguousarray(_to_series(gz_w, S, nwin)) if as_series else gz_w)
        res = []
        for fn in (lambda s: po.fused(s, pool, as_series=as_series, **kw), lambda s: po.composition(s, pool, as_series, **kw)):
            x = _dev(series[..., 0] if f == 1 else series).requires_grad_(True)
            res.append(_grads(su, x, lambda s: (fn(s), gz)))
        (z, ds, dW, db), (z_c, ds_c, dW_c, db_c) = res
        assert tuple(z.shape) == ((S, m, nwin, g) if as_series else (S * nwin, m, g))
        # the composition: the same gy through the same kernels
        assert torch.equal(z, z_c) and torch.equal(ds, ds_c) and torch.equal(dW, dW_c) and torch.equal(db, db_c), as_series
        # the oracle: values, then its backward fed with gz routed by the GPU's arg-max and z > 0
        z_w = window_major(z) if as_series else z
        e_out = rel_err(z_w.cpu().numpy(), _pool64(ref_b, pool))
        su.layer.zero_grad()
        xg = _dev(series[..., 0] if f == 1 else series).requires_grad_(True)
        zz = po.fused(xg, pool, as_series=as_series, **kw)
        idx = _saved_idx(zz)
        idx_w = (window_major(idx) if as_series else idx).cpu().numpy()
        gy = _route(gz_w.astype(np.float64), z_w.cpu().numpy(), idx_w, pool)
        gxw, gW = O.layer_backward(su.L, xw, su.W64(), gy, su.mode)
        gs = fold_dilated(gxw, S, T, d, left, right)
        gb = su.bias_grad(gy)
        errs = dict(ds=rel_err(ds.cpu().numpy().reshape(series.shape), gs), dW=rel_err(dW.cpu().numpy(), gW),
                    db=rel_err(db.cpu().numpy().reshape(gb.shape), gb))
        print(cls, shape, pool, "series" if as_series else "window-major", dict(out=e_out, **errs))
        assert e_out <= TOL, e_out
        assert max(errs.values()) <= TOL_GRAD, errs
    # without a bias: values against the oracle's
    z0 = po.fused(_dev(series[..., 0] if f == 1 else series), pool, bias=False, **kw)
    assert rel_err(z0.detach().cpu().numpy(), _pool64(ref_0, pool)) <= TOL


@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_one_sided_backwards(cls, gpu_device):
    shape = ORACLE[0]
    T, H, d, f, g, left, right = shape
    su, po, (series, *_rest) = _oracle_case(cls, shape)
    gz = torch.randn(S_REC * nwin_of(T, H, d, left, right), N_VERT // 4, g, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    full = _grads(su, _dev(series).requires_grad_(True), lambda s: (po.fused(s, 4), gz))
    # a series without grad: dW and db alone
    z, ds, dW, db = _grads(su, _dev(series), lambda s: (po.fused(s, 4), gz))
    assert ds is None and torch.equal(z, full[0]) and torch.equal(dW, full[2]) and torch.equal(db, full[3])
    # a frozen layer: d series alone
    su.layer.requires_grad_(False)
    try:
        z, ds, dW, db = _grads(su, _dev(series).requires_grad_(True), lambda s: (po.fused(s, 4), gz))
    finally:
        su.layer.requires_grad_(True)
    assert dW is None and db is None and torch.equal(z, full[0]) and torch.equal(ds, full[1])


# ---------------------------------------------------------------------------------------------------------------- 4. reordered operand
@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
def test_a_reordered_operand_gives_the_plain_operands_values(as_series, cls, gpu_device):
    su = Setup(cls, 4, 40, H_TAPS, seed=9)
    po = Pooler(su, 9)
    re = su.op.reordered("degree")
    assert re.perm is not None and not su.F.series_pool_is_fused(re) and su.F.series_pool_is_fused(su.op)
    x = _series(S_REC, N_VERT, 40, 4, 9)
    for kw, _ in GEOS:
        for pool in (2, 4):
            res = []
            for op in (None, re):
                def run(s, op=op):
                    z = po.fused(s, pool, op=op, as_series=as_series, **kw)
                    return z, torch.randn(z.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(pool))
                res.append(_grads(su, x.clone().requires_grad_(True), run))
            (z, ds, dW, db), (z_r, ds_r, dW_r, db_r) = res
            assert rel_err(z_r.cpu().numpy(), z.cpu().numpy()) <= TOL, (kw, pool)
            # the arg-max may differ where two members agree to rounding, so the gradients are compared only where the values are bit-equal
            if torch.equal(z, z_r):
                assert max(rel_err(a.cpu().numpy(), b.cpu().numpy()) for a, b in ((ds_r, ds), (dW_r, dW), (db_r, db))) <= TOL_GRAD, (kw, pool)


# ---------------------------------------------------------------------------------------------------------------- 5. streaming
STREAM_CHUNKS = (1, 3, 8, 9, 5, 4, 2)
STREAM = [(3, 1), (3, 2), (5, 2)]           # (H, dilation): C = 2, 4, 8


def test_the_chunk_list_hits_what_it_is_here_for():
    for H, d in STREAM:
        Cr = (H - 1) * d
        heads = [int(h) % Cr for h in np.cumsum((0,) + STREAM_CHUNKS[:-1])]
        assert any(t < Cr for t in STREAM_CHUNKS) or Cr == 2
        assert any(t == Cr for t in STREAM_CHUNKS) and any(t > Cr for t in STREAM_CHUNKS) and any(h != 0 for h in heads)
    Cr = 8
    heads = [int(h) % Cr for h in np.cumsum((0,) + STREAM_CHUNKS[:-1])]
    assert any(0 < t < Cr and h + t > Cr for t, h in zip(STREAM_CHUNKS, heads))          # a short chunk that wraps round the ring's end


def _stream_pool(su, extra, chunk, state, pool, bias=True, **kw):
    import tgcn_amd
    if bias:
        return tgcn_amd.cheb_stream_relu_pool(su.layer, chunk, *extra, pool=pool, state=state, **kw)
    W = su.layer.weight if chunk.dim() == 4 else su.layer.weight.reshape(K_TERMS, su.layer.weight.shape[1], -1)
    return su.F.cheb_time_stream_relu_pool(su.op, chunk, W, None, su.F.BIAS_NONE, su.fmode, pool, state=state, **kw)


def _stream_plain(su, extra, chunk, state, bias=True, **kw):
    if bias:
        return su.layer.forward_stream(chunk, *extra, state=state, **kw)
    W = su.layer.weight if chunk.dim() == 4 else su.layer.weight.reshape(K_TERMS, su.layer.weight.shape[1], -1)
    return su.F.cheb_time_stream(su.op, chunk, W, None, su.F.BIAS_NONE, su.fmode, state=state, **kw)


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("H,d", STREAM, ids=lambda v: str(v))
@pytest.mark.parametrize("f,N", [(4, 40), (3, 5), (1, 72)])
def test_stream_chunks_equal_relu_pool_of_forward_stream_on_twin_states(f, N, H, d, cls, gpu_device):
    su = Setup(cls, f, N, H, seed=f + H + d)
    extra = () if cls == "TGCNCheb_H" else (edge_index_of(f + H + d), None)
    T = sum(STREAM_CHUNKS)
    whole = _series(S_REC, N_VERT, T, f, T + f)
    with torch.no_grad():
        for pool in (2, 4):
            for bias in (True, False):
                fused = plain = cap = alt = None
                t0 = 0
                for i, Tc in enumerate(STREAM_CHUNKS):
                    chunk = whole[:, :, t0:t0 + Tc].contiguous()
                    t0 += Tc
                    z, fused = _stream_pool(su, extra, chunk, fused, pool, bias, dilation=d)
                    out, plain = _stream_plain(su, extra, chunk, plain, bias, dilation=d)
                    z_ref, _ = relu_pool(out, pool)
                    assert tuple(z.shape) == (S_REC, N_VERT // pool, Tc, N) and z.is_contiguous()
                    assert torch.equal(z, z_ref), (pool, bias, i)
                    assert torch.equal(fused.ring, plain.ring) and (fused.head, fused.seen) == (plain.head, plain.seen), (pool, bias, i)
                    # a capturable twin: the position on the device
                    z_c, cap = _stream_pool(su, extra, chunk, cap, pool, bias, dilation=d, capturable=(cap is None))
                    assert torch.equal(z_c, z_ref) and torch.equal(cap.ring, plain.ring), (pool, bias, i)
                    # pooled and unpooled steps alternating on one state
                    if i % 2:
                        o2, alt = _stream_plain(su, extra, chunk, alt, bias, dilation=d)
                        assert torch.equal(o2, out), (pool, bias, i)
                    else:
                        z2, alt = _stream_pool(su, extra, chunk, alt, pool, bias, dilation=d)
                        assert torch.equal(z2, z_ref), (pool, bias, i)
                    assert torch.equal(alt.ring, plain.ring), (pool, bias, i)
                assert cap.capturable and cap.pos.tolist() == [plain.head, plain.seen] and plain.ring.any()


@gpu
def test_one_tap_streams_without_a_ring(gpu_device):
    su = Setup("TGCNCheb_H", 4, 40, 1, seed=2)
    whole = _series(S_REC, N_VERT, 12, 4, 2)
    with torch.no_grad():
        for capturable in (False, True):
            state = plain = None
            for t0, Tc in ((0, 5), (5, 7)):
                z, state = _stream_pool(su, (), whole[:, :, t0:t0 + Tc].contiguous(), state, 4, dilation=3, capturable=capturable)
                out, plain = _stream_plain(su, (), whole[:, :, t0:t0 + Tc].contiguous(), plain, dilation=3)
                assert torch.equal(z, relu_pool(out, 4)[0])
            assert state.ring is None and state.seen == 12


@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_a_two_layer_chain_through_graphed_stream(cls, gpu_device):
    """a pooled 48-vertex layer, then forward_stream on the 12-vertex graph: every replay torch.equal to the eager chain on twin states"""
    import tgcn_amd
    l1, e1 = _layer_on(cls, N_VERT, 4, 24, 3, seed=1)
    l2, e2 = _layer_on(cls, N_VERT // 4, 24, 8, 3, seed=2)

    def chain(capturable):
        def step(chunk, states):
            s1, s2 = states or (None, None)
            z1, s1 = tgcn_amd.cheb_stream_relu_pool(l1, chunk, *e1, pool=4, state=s1, capturable=capturable)
            o2, s2 = l2.forward_stream(z1, *e2, state=s2, dilation=2, capturable=capturable)
            return o2, (s1, s2)
        return step

    Tc, steps = 4, 5
    whole = _series(S_REC, N_VERT, Tc * steps, 4, 7)
    gs = tgcn_amd.GraphedStream(chain(True), whole[:, :, :Tc].contiguous())
    eager = chain(False)
    for rounds in range(2):
        states = None
        with torch.no_grad():
            for i in range(steps):
                chunk = whole[:, :, i * Tc:(i + 1) * Tc].contiguous()
                want, states = eager(chunk, states)
                got = gs(chunk)
                assert tuple(got.shape) == (S_REC, N_VERT // 4, Tc, 8) and torch.equal(got, want), (rounds, i)
        assert all(torch.equal(a.ring, b.ring) for a, b in zip(gs.states, states))
        gs.reset()


# ---------------------------------------------------------------------------------------------------------------- 6. memory
@gpu
def test_the_unpooled_output_is_never_allocated(gpu_device):
    """derived, not measured: stack 2 * 1024 * 128 * 4 floats = 4.2 MB, z 1024/4 * 126 * 64 floats = 8.3 MB, no arg-max under no_grad, the
    fold and workspaces below 1 MB -- about 15 MB with the allocator's rounding, against 33 MB for the (126 * 1024, 64) layer output"""
    import tgcn_amd
    S, n, T, f, N, K, H, pool = 1, 1024, 128, 4, 64, 2, 3, 4
    layer, _ = _layer_on("TGCNCheb_H", n, f, N, H, seed=4, K=K)
    x = _series(S, n, T, f, 4)
    unpooled = S * n * (T - H + 1) * N * 4
    assert unpooled > 33e6
    with torch.no_grad():
        z = tgcn_amd.cheb_series_relu_pool(layer, x, pool=pool)           # builds the operand and the cached workspaces
        del z
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        z = tgcn_amd.cheb_series_relu_pool(layer, x, pool=pool)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    print("peak above the pre-call level: %.1f MB; unpooled output: %.1f MB" % (peak / 1e6, unpooled / 1e6))
    assert tuple(z.shape) == ((T - H + 1) * S, n // pool, N)
    assert peak < unpooled, (peak, unpooled)
