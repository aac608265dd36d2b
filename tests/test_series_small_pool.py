"""relu (+ dropout) + pool in the one-launch series layer (tgcn_amd.cheb_series_relu_pool_fused / F.cheb_time_windows_relu_pool_fused;
csrc/series_small.h small_series_pool_kernel) on the GPU.  The sharp check is bits: z and the gradients w.r.t. series, weight and bias are
torch.equal to the composition of the same commit -- F._relu_pool_view / F._relu_dropout_pool_view of forward_series(..., fused=True) under
the same seed (both routes run the same hop code and the same backward entry on the same stack); it also sidesteps arg-max ties against an
fp64 reference.  Values are checked against the fp64 oracle on materialised windows, then relu, the mask of F.dropout_keep_mask and the max,
within TOL = 1e-5 (tests/test_series_channels.py).  Shapes are the smallest that cross each line of the epilogue: 36 vertices at degree 30
(staged densely: two full vertex tiles and a third holding one pool group), 52 at degree 6 (CSR), 50 at degree 6 with pool = 2 only (the last
accumulator quad holds one whole pair and one pair past n); 1 / 3 / 4 channels, 5 output columns (a partial column tile) and 40 (two column
groups), K = 1 / 2 / 5 in both recurrences, 1 and 3 taps, dilation 1 and 2, no / causal / one-sided padding, both layouts, pool 2 and 4,
p = 0 and 0.3, S = 2 recordings of T = 70 rows.  Each accuracy case asks the plan first and asserts nwin >= 3*tb and nwin % tb != 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cheb_oracle as O
from test_hip_parity import _random_graph
from test_series_channels import TOL, _dev
from test_series_dilation import nwin_of, padding_arg, windows_dilated

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]

S_REC, T_ROWS, SEED = 2, 70, 1234
GRAPHS = {36: 30, 52: 6, 50: 6}     # vertices -> average degree


class Setup:
    """One class on one of the graphs: the layer, its operand, the fp64 forward, the new call and the composition it must equal"""

    def __init__(self, cls, n, f, g, K, H, seed):
        import tgcn_amd
        from tgcn_amd import functional as F
        rng = np.random.default_rng(seed)
        row, col, val = _random_graph(n, GRAPHS[n], rng)
        val = val * (0.4 if GRAPHS[n] < 10 else 0.25)
        torch.manual_seed(seed)
        self.T, self.F, self.n, self.K, self.H, self.f = tgcn_amd, F, n, K, H, f
        if cls == "TGCNCheb_H":
            self.L = O.coo_to_csr(row, col, val, n)
            self.op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val))
            self.layer = layer = tgcn_amd.TGCNCheb_H(self.op, f, g, K, H).cuda()
            self.fmode, self.extra = F.MODE_POWER, ()
            self.forward64 = lambda xw, b: O.tgcn_cheb_h_forward(self.L, xw, self.W64(), b)
        else:
            ei = np.stack([row, col]).astype(np.int64)
            self.layer = layer = tgcn_amd.ChebTimeConv(f, g, K, H).cuda()
            self.fmode = F.MODE_CHEBYSHEV
            eid = _dev(ei)
            self.extra = (eid, None)
            self.op = layer._operand(torch.empty(1, n, 1, device="cuda"), eid, None)
            self.forward64 = lambda xw, b: O.cheb_time_conv_forward(xw, ei, None, self.W64(), b)
        with torch.no_grad():
            layer.bias.uniform_(-0.5, 0.5)       # TGCNCheb_H: per vertex and channel, so it differs inside a pool group

    def W64(self):
        return self.layer.weight.detach().cpu().numpy()

    def weight_for(self, s):
        W = self.layer.weight
        return W if s.dim() == 4 else W.reshape(self.K, W.shape[1], -1)

    def fused(self, s, bias, pool, p, seed, **kw):
        """the new call: the module entry with the layer's bias, the functional entry without one"""
        if bias:
            return self.T.cheb_series_relu_pool_fused(self.layer, s, *self.extra, pool=pool, p=p, seed=seed, **kw)
        return self.F.cheb_time_windows_relu_pool_fused(self.op, s, self.weight_for(s), None, self.F.BIAS_NONE, self.fmode, pool, p=p, seed=seed, **kw)

    def composed(self, s, bias, pool, p, seed, **kw):
        """forward_series(fused=True), then relu (+ dropout) + pool as their own pass"""
        F = self.F
        if bias:
            y = self.layer.forward_series(s, *self.extra, fused=True, **kw)
        else:
            y = F.cheb_time_windows(self.op, s, self.weight_for(s), None, F.BIAS_NONE, self.fmode, fused=True, **kw)
        if p == 0:
            return F._relu_pool_view(y, pool)
        thr, scale = F.dropout_params(p)
        return F._relu_dropout_pool_view(y, pool, F.dropout_seed(seed, y.device), thr, scale)

    def plan(self, N, T, left, right, d):
        rc, tb, dense, lds = self.F._series_small_plan(self.op, self.f, self.H, N, self.K, T, left, right, d, self.fmode)
        assert rc == 0 and lds <= 160 * 1024
        return tb, dense


def _series_in(series):
    """a single channel is given as a 3-D series"""
    return _dev(series[..., 0] if series.shape[3] == 1 else series)


def _run(su, route, series, go, bias, pool, p, **kw):
    """(z, d series, dW, db) of one forward + backward through su.fused or su.composed"""
    su.layer.zero_grad()
    st = _series_in(series).requires_grad_(True)
    z = route(st, bias, pool, p, SEED, **kw)
    z.backward(go)
    db = None if su.layer.bias.grad is None else su.layer.bias.grad.clone()
    return z.detach(), st.grad.clone(), su.layer.weight.grad.clone(), db


def _pooled64(ref, pool, p, nwin, device):
    """relu, the mask, the max of the fp64 window-major layer output ref (S*nwin, n, g)"""
    from tgcn_amd import functional as F
    t = np.maximum(ref, 0.0)
    if p:
        keep = F.dropout_keep_mask(SEED, 0, ref.size, p, device).cpu().numpy().reshape(ref.shape)
        t = t * keep * float(F.dropout_params(p)[1])
    q, n, g = ref.shape
    return t.reshape(q, n // pool, pool, g).max(axis=2)


# (n, f, g, K, H, d, left, right, pool, p): every listed value of every axis, each next to a different neighbour
CASES = [(36, 1, 5, 5, 3, 1, 0, 0, 4, 0.3), (36, 3, 40, 2, 3, 2, 4, 0, 2, 0.0), (36, 4, 40, 5, 3, 1, 1, 2, 4, 0.3), (36, 1, 40, 1, 1, 2, 0, 0, 2, 0.3),
         (52, 1, 40, 5, 3, 2, 1, 2, 4, 0.0), (52, 3, 5, 1, 3, 1, 2, 0, 2, 0.3), (52, 4, 5, 2, 1, 1, 0, 0, 4, 0.0), (52, 4, 40, 5, 3, 2, 0, 0, 4, 0.3),
         (50, 3, 40, 5, 3, 1, 0, 0, 2, 0.3), (50, 1, 5, 2, 3, 2, 1, 2, 2, 0.0)]
CLASSES = ["TGCNCheb_H", "ChebTimeConv"]


def _id(c):
    return "n%d_f%d_g%d_K%d_H%d_d%d_l%d_r%d_pool%d_p%g" % c


def test_the_cases_cover_every_listed_value():
    cols = list(zip(*CASES))
    assert set(cols[0]) == {36, 52, 50} and set(cols[1]) == {1, 3, 4} and set(cols[2]) == {5, 40} and set(cols[3]) == {1, 2, 5}
    assert set(cols[4]) == {1, 3} and set(cols[5]) == {1, 2} and set(cols[8]) == {2, 4} and set(cols[9]) == {0.0, 0.3}
    assert {c[8] for c in CASES if c[0] == 50} == {2}
    for n in (36, 52):          # both pools, with and without a mask, on the dense and on the sparse staging
        assert {c[8] for c in CASES if c[0] == n} == {2, 4} and {c[9] for c in CASES if c[0] == n} == {0.0, 0.3}
    pads = {padding_arg(c[4], c[5], c[6], c[7]) if c[4] > 1 else 0 for c in CASES}
    assert {0, "causal", (1, 2)} <= pads
    assert {(c[2], c[9] > 0) for c in CASES} == {(5, True), (5, False), (40, True), (40, False)}     # N % 4 != 0 and == 0, each with a mask


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bits_of_the_composition_and_values_of_the_oracle(case, cls, gpu_device):
    n, f, g, K, H, d, left, right, pool, p = case
    S, T = S_REC, T_ROWS
    nwin = nwin_of(T, H, d, left, right)
    geo = dict(padding=padding_arg(H, d, left, right) if H > 1 else 0, dilation=d)
    su = Setup(cls, n, f, g, K, H, seed=n + 7 * d + f + K)
    tb, dense = su.plan(g, T, left, right, 1 if H == 1 else d)
    assert dense == (1 if n == 36 else 0)
    assert nwin >= 3 * tb and nwin % tb != 0, (nwin, tb)        # a first, an interior and a ragged last tile
    rng = np.random.default_rng([n, f, g, K, H, d])
    series = rng.standard_normal((S, n, T, f)).astype(np.float32)
    xw = windows_dilated(series, H, d, left, right).astype(np.float64)
    go_wm = torch.randn(S * nwin, n // pool, g, device="cuda")
    go_s = go_wm.view(S, nwin, n // pool, g).permute(0, 2, 1, 3).contiguous()
    for bias in (True, False):
        ref = _pooled64(su.forward64(xw, su.layer.bias.detach().cpu().numpy() if bias else None), pool, p, nwin, "cuda")
        for as_series in (False, True):
            go = go_s if as_series else go_wm
            got = _run(su, su.fused, series, go, bias, pool, p, as_series=as_series, **geo)
            want = _run(su, su.composed, series, go, bias, pool, p, as_series=as_series, **geo)
            z = got[0]
            assert tuple(z.shape) == ((S, n // pool, nwin, g) if as_series else (S * nwin, n // pool, g)) and z.is_contiguous()
            wm = z.permute(0, 2, 1, 3).reshape(S * nwin, n // pool, g) if as_series else z
            err = rel_err(wm.cpu().numpy(), ref)
            print(cls, case, "bias" if bias else "no bias", "series" if as_series else "windows", "TB", tb, "oracle", err)
            for nm, a, b in zip(("z", "d series", "dW", "db"), got, want):
                assert (a is None and b is None) if (nm == "db" and not bias) else torch.equal(a, b), (nm, bias, as_series)
            assert err <= TOL, (bias, as_series)
            if p:
                assert (z == 0).float().mean() > 0.05         # the mask dropped whole groups somewhere


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("n,f,g,pool", [(36, 3, 40, 4), (52, 1, 5, 2)])
def test_a_shifted_series_gives_the_same_bits_across_tile_seams(n, f, g, pool, d, cls, gpu_device):
    """padding=0, p=0: window w of series[:, :, 5:] is window w + 5 of the series; the tiles fall elsewhere, and no sum's order depends on them"""
    su = Setup(cls, n, f, g, 5, 3, seed=n + d)
    tb, _ = su.plan(g, T_ROWS, 0, 0, d)
    assert 5 % tb != 0          # the shift moves every seam
    x = torch.randn(S_REC, n, T_ROWS, f, device="cuda")
    if f == 1:
        x = x[..., 0]
    with torch.no_grad():
        whole = su.fused(x, True, pool, 0.0, None, as_series=True, dilation=d)
        shifted = su.fused(x[:, :, 5:].contiguous(), True, pool, 0.0, None, as_series=True, dilation=d)
    assert shifted.shape[2] == whole.shape[2] - 5 and shifted.shape[1] == n // pool
    assert torch.equal(shifted, whole[:, :, 5:])


@gpu
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("n,f,g,pool", [(36, 3, 40, 4), (52, 4, 5, 2)])
def test_non_finite_values_give_the_bits_of_the_composition(n, f, g, pool, p, gpu_device):
    """one NaN and one +Inf in the series: compared through an int32 view, so that a NaN equals a NaN of the same bits"""
    su = Setup("TGCNCheb_H", n, f, g, 2, 3, seed=n + f)
    x = torch.randn(S_REC, n, T_ROWS, f, device="cuda")
    x[0, 5, 20, 0] = float("nan")
    x[1, n - 2, 41, f - 1] = float("inf")
    with torch.no_grad():
        for as_series in (False, True):
            z = su.fused(x, True, pool, p, SEED, as_series=as_series, padding="causal")
            want = su.composed(x, True, pool, p, SEED, as_series=as_series, padding="causal")
            assert torch.isnan(z).any() and not torch.isnan(z).all()
            assert torch.equal(z.view(torch.int32), want.view(torch.int32)), as_series


@gpu
def test_a_seed_tensor_rewritten_in_place_gives_another_mask(gpu_device):
    su = Setup("ChebTimeConv", 52, 3, 40, 2, 3, seed=4)
    x = torch.randn(S_REC, 52, T_ROWS, 3, device="cuda")
    seed_t = torch.tensor([11], dtype=torch.int64, device="cuda")
    zs = []
    for value in (11, 12):
        seed_t.fill_(value)
        z = su.fused(x, True, 4, 0.3, seed_t)
        assert "ChebSeriesSmallReluPoolFn" in type(z.grad_fn).__name__ and z.grad_fn.seed.data_ptr() == seed_t.data_ptr()
        assert torch.equal(z, su.composed(x, True, 4, 0.3, value)), value
        zs.append(z.detach())
    assert not torch.equal(zs[0], zs[1])


class _Spy:
    """the library with one entry's arguments recorded"""

    def __init__(self, lib, name):
        self._lib, self._name, self.args = lib, name, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != self._name:
            return fn

        def call(*args):
            self.args.append(args)
            return fn(*args)
        return call


@gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["power", "chebyshev"])
@pytest.mark.parametrize("n,f,N,pool,p", [(36, 3, 40, 4, 0.3), (50, 1, 5, 2, 0.0), (52, 4, 40, 2, 0.3)])
def test_the_c_entry_directly(n, f, N, pool, p, mode, gpu_device, monkeypatch):
    """under torch.no_grad() the call passes NULL for idx and for the stack; the entry with both gives the same z, relu_pool's arg-max and
    the stack of the unpooled entry"""
    from tgcn_amd import _lib
    from tgcn_amd import functional as F
    L = _lib.lib()
    su = Setup("TGCNCheb_H", n, f, N, 5, 3, seed=3 * n + f)
    op, K, H, S, T, left, right, d = su.op, 5, 3, S_REC, T_ROWS, 1, 2, 2
    nwin = nwin_of(T, H, d, left, right)
    torch.manual_seed(n + f)
    x, W = torch.randn(S, n, T, f, device="cuda"), torch.randn(K, H, f, N, device="cuda") * 0.3
    bias = torch.randn(N, device="cuda")
    spy = _Spy(L, "tgcn_cheb_series_small_pool_f32")
    monkeypatch.setattr(_lib, "lib", lambda: spy)
    with torch.no_grad():
        z0 = F.cheb_time_windows_relu_pool_fused(op, x, W, bias, F.BIAS_CHANNEL, mode, pool, p=p, seed=SEED, as_series=True, padding=(left, right),
                                                 dilation=d)
    monkeypatch.setattr(_lib, "lib", lambda: L)
    (args,) = spy.args
    assert args[15].value is None and args[17].value is None and args[16] == pool       # idx, stack
    assert (args[21].value is None) == (p == 0)
    # the power-mode call folded the weight: hand the entry the working weight it saw
    Wt = F._working_weight(F._power_fold(mode, W.view(K, H * f, N)), W.view(K, H * f, N))
    thr, scale = F.dropout_params(p)
    seed_t = torch.tensor([SEED], dtype=torch.int64, device="cuda") if p else None
    z1 = torch.full((S, n // pool, nwin, N), float("nan"), device="cuda")
    idx = torch.full((S, n // pool, nwin, N), 255, dtype=torch.uint8, device="cuda")
    stack = torch.full((K, S, n, T * f), float("nan"), device="cuda")
    _lib.check(L.tgcn_cheb_series_small_pool_f32(_lib.stream_ptr(), C.byref(op.struct), mode, S, T, f, H, N, K, _lib.ptr(x), _lib.ptr(Wt), _lib.ptr(bias),
                                                 1, 1, _lib.ptr(z1), _lib.ptr(idx), pool, _lib.ptr(stack), left, right, d, _lib.ptr(seed_t), thr, scale))
    y = torch.empty(S, n, nwin, N, device="cuda")
    stack_y = torch.empty_like(stack)
    _lib.check(L.tgcn_cheb_series_small_f32(_lib.stream_ptr(), C.byref(op.struct), mode, S, T, f, H, N, K, _lib.ptr(x), _lib.ptr(Wt), _lib.ptr(bias), 1, 1,
                                            _lib.ptr(y), _lib.ptr(stack_y), left, right, d))
    torch.cuda.synchronize()
    assert torch.equal(z0, z1) and torch.equal(stack, stack_y) and int(idx.max()) < pool
    # the pass over the stored output: the same z and the same arg-max bytes
    want, widx = torch.empty_like(z1), torch.empty_like(idx)
    y3 = y.view(S, n, nwin * N)
    if p == 0:
        _lib.check(L.tgcn_relu_pool_f32(_lib.stream_ptr(), _lib.ptr(y3), _lib.ptr(want), _lib.ptr(widx), S, n, nwin * N, pool))
    else:
        _lib.check(L.tgcn_relu_dropout_pool_f32(_lib.stream_ptr(), _lib.ptr(y3), _lib.ptr(want), _lib.ptr(widx), S, n, nwin * N, pool, N, _lib.ptr(seed_t),
                                                thr, scale))
    torch.cuda.synchronize()
    assert torch.equal(z1, want) and torch.equal(idx, widx)


@gpu
def test_refused_calls_launch_nothing(gpu_device):
    from tgcn_amd import _lib
    L = _lib.lib()
    su = Setup("TGCNCheb_H", 50, 4, 5, 2, 3, seed=2)
    op, S, T, f, H, N, K = su.op, 1, 12, 4, 3, 5, 2
    x3, W = torch.ones(S, 50, T * f, device="cuda"), torch.zeros(K, H * f, N, device="cuda")
    z, idx = torch.full((S, 25, T - 2, N), float("nan"), device="cuda"), torch.full((S, 25, T - 2, N), 255, dtype=torch.uint8, device="cuda")
    stack = torch.full((K, S, 50, T * f), float("nan"), device="cuda")
    seed_t = torch.tensor([3], dtype=torch.int64, device="cuda")

    def call(pool=2, T=T, left=0, bias_kind=0, series=x3, seed=None, scale=1.0):
        return L.tgcn_cheb_series_small_pool_f32(_lib.stream_ptr(), C.byref(op.struct), 0, S, T, f, H, N, K, _lib.ptr(series), _lib.ptr(W), None, bias_kind,
                                                 1, _lib.ptr(z), _lib.ptr(idx), pool, _lib.ptr(stack), left, 0, 1, _lib.ptr(seed), 0, scale)
    assert call(pool=4) == -1 and call(pool=3) == -1 and call(pool=0) == -1 and call(pool=1) == -1       # 50 % 4 != 0; outside {2, 4}
    assert call(seed=seed_t, scale=0.5) == -1 and call(seed=seed_t, scale=float("inf")) == -1 and call(seed=seed_t, scale=float("nan")) == -1
    assert call(T=2) == -1 and call(left=3) == -1 and call(bias_kind=1) == -1 and call(series=None) == -1
    torch.cuda.synchronize()
    assert torch.isnan(z).all() and torch.isnan(stack).all() and (idx == 255).all()
    assert call() == 0 and call(seed=seed_t, scale=2.0) == 0
    torch.cuda.synchronize()
    assert not z.any() and (idx == 0).all() and (stack[0] == 1).all()          # W = 0: relu(0) = 0, the first member wins
    x = torch.randn(2, 50, 12, 4, device="cuda")
    with torch.no_grad():
        with pytest.raises(_lib.TgcnError, match="multiple of pool"):
            su.T.cheb_series_relu_pool_fused(su.layer, x, pool=4)
        with pytest.raises(_lib.TgcnError, match="reordered"):
            su.F.cheb_time_windows_relu_pool_fused(op.reordered("degree"), x, su.layer.weight, None, su.F.BIAS_NONE, su.fmode, 2)
        assert not su.F.series_pool_fused_supported(op, 4, 3, 5, 2, 12, 0, 1, su.fmode, 4)
        assert su.F.series_pool_fused_supported(op, 4, 3, 5, 2, 12, 0, 1, su.fmode, 2)
        assert not su.F.series_pool_fused_supported(op, 64, 700, 5, 2, 800, 0, 1, su.fmode, 2)
        with pytest.raises(_lib.TgcnError, match="do not fit"):
            su.F.cheb_time_windows_relu_pool_fused(op, torch.randn(1, 50, 800, 64, device="cuda"), torch.randn(2, 700, 64, 5, device="cuda"), None,
                                                   su.F.BIAS_NONE, su.fmode, 2)


@gpu
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_auto_is_one_of_the_two_calls_bit_for_bit(p, gpu_device, monkeypatch):
    """fused="auto" is the one-launch call where F.SERIES_POOL_FUSED_AUTO lists the class, the general pooled call elsewhere"""
    su = Setup("TGCNCheb_H", 52, 3, 40, 5, 3, seed=13)
    F = su.F
    x = torch.randn(S_REC, 52, T_ROWS, 3, device="cuda")
    klass = "pool" if p == 0 else "pool_dropout"
    with torch.no_grad():
        fused = su.fused(x, True, 4, p, SEED, padding="causal")
        if p == 0:
            general = su.T.cheb_series_relu_pool(su.layer, x, pool=4, padding="causal")
        else:
            general = su.T.cheb_series_relu_dropout_pool(su.layer, x, p=p, pool=4, seed=SEED, padding="causal")
        assert torch.equal(su.fused(x, True, 4, p, SEED, padding="causal", fused="auto"), fused if klass in F.SERIES_POOL_FUSED_AUTO else general)
        monkeypatch.setattr(F, "SERIES_POOL_FUSED_AUTO", ("pool", "pool_dropout"))
        assert torch.equal(su.fused(x, True, 4, p, SEED, padding="causal", fused="auto"), fused)
        monkeypatch.setattr(F, "SERIES_POOL_FUSED_AUTO", ())
        assert torch.equal(su.fused(x, True, 4, p, SEED, padding="causal", fused="auto"), general)
    assert rel_err(fused.cpu().numpy(), general.cpu().numpy()) <= TOL      # the two agree to rounding (a hop adds its neighbours in another order)
