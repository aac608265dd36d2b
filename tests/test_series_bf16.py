"""Streaming time windows with bfloat16 parameters: TGCNCheb_H.forward_series / ChebTimeConv.forward_series / F.cheb_time_windows on bf16
layers (ChebSeriesBf16Fn, csrc/windows_bf16.h), forward and the three gradients, by the method of tests/test_bf16_layers.py:

  * the reference is the fp64 oracle on the materialised windows (tests/test_series_conv.py's padded, strided rule) of the bf16-rounded
    series, weight and upstream gradient (the series is given to the layer as bf16: with bf16 parameters it has to be);
  * a numpy emulation rounds at exactly the points DESIGN.md 3.10 "bf16" lists (every hop of the stack, the folded weight, the output, each
    gradient once);
  * the fp64 bound per case and tensor (out, d series, dW, db) is TWICE the emulation's own error against fp64, measured on the CPU
    (TOL64, the measured values in the comments; test_tolerances_are_twice_the_emulations_error recomputes them without a GPU);
  * the GPU must agree with the emulation within EMUL_ULPS = 8 bf16 ulps of the tensor's largest value (sums run in another order, so a
    rounding point may land one ulp away and the hops carry it on: test_bf16_layers' bound and reasoning);
  * the two output layouts of one call are torch.equal.

Every GPU test first requires the new entries and fails without them."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F
from conftest import rel_err
from oracle import cheb_oracle as O
from test_bf16_layers import EMUL_ULPS, _apply, _bias_add, _fold, bf, fp64_reference, golden_graph
from test_hip_parity import _random_graph
from test_series_conv import fold_conv, nwin_of, padding_arg, windows_conv

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]

BF = torch.bfloat16
KB64 = 64 * 1024
OK, UNSUPPORTED = 0, -4
ENTRIES = ("tgcn_cheb_project_series_conv_bf16", "tgcn_cheb_series_conv_backward_bf16", "tgcn_cheb_series_conv_backward_bf16_workspace_bytes",
           "tgcn_series_conv_plan_bf16")


def require_series_bf16_entries():
    import ctypes
    handle = ctypes.CDLL(_lib.LIB_PATH)
    missing = [e for e in ENTRIES if not hasattr(handle, e)]
    assert not missing and all(e in _lib.SIGNATURES for e in ENTRIES) and hasattr(F, "ChebSeriesBf16Fn"), "no bf16 series entries: %s" % missing


# name: (class, n (148: the dti148 golden graph), S, T, H, f, g, K, stride, left, right)  -- what the shape is there for
CASES = {
    "vec8-f8-H15": ("TGCNCheb_H", 148, 2, 40, 15, 8, 16, 3, 1, 0, 0),            # VEC8 rows of one 16-byte group, NT 1, nwin = 26 < 32
    "vec8-f16-H15-g32": ("ChebTimeConv", 148, 1, 50, 15, 16, 32, 4, 1, 0, 0),    # VEC8, NT 2, nwin = 36 (a tail tile of 4), true recurrence
    "f4-g80-even-step": ("TGCNCheb_H", 33, 2, 30, 6, 4, 80, 3, 2, 5, 0),         # narrow reads, NT 4 x 2 column blocks, lst = 2, causal, K*f = 12
    "f3-g40-step3": ("ChebTimeConv", 50, 2, 33, 7, 3, 40, 3, 3, 0, 0),           # narrow reads, column tail (40 of 64), step 3, rows padded 99 -> 104
    "f1-as-series-g20": ("TGCNCheb_H", 19, 2, 20, 5, 1, 20, 3, 1, 0, 0),         # one channel (3-D series, as_series first); g rows of 20: the
                                                                                 # scalar form of the input gradient; 38 wave tiles: 2 idle waves
    "short-recording": ("TGCNCheb_H", 50, 2, 2, 5, 4, 8, 3, 3, 0, 3),            # T + left < min(stride, H): one window, phases without a time row
    "step-over-H-f32": ("ChebTimeConv", 40, 2, 40, 5, 32, 16, 1, 7, 0, 0),       # stride > H >= HC: only the rows read; phases 5, 6 cleared; K = 1
    "pads-f8-K5": ("ChebTimeConv", 45, 2, 24, 6, 8, 16, 5, 2, 2, 3),             # (left, right) with a step, VEC8 with lst = 2, deep recurrence
    "f24-g48-row-wrap": ("TGCNCheb_H", 28, 1, 45, 4, 24, 48, 4, 1, 1, 1),        # VEC8, f/8 odd: k groups that straddle a time row; NT 4 tail
    # regimes (found with tgcn_series_conv_plan_bf16; asserted through it below)
    "fwd-chunked-vec": ("TGCNCheb_H", 19, 1, 50, 20, 96, 8, 2, 2, 0, 3),         # HC = 14 of 20
    "fwd-chunked-narrow": ("TGCNCheb_H", 19, 1, 50, 20, 100, 8, 2, 2, 1, 0),     # f % 8 != 0, HC = 17 of 20
    "fwd-large": ("TGCNCheb_H", 23, 1, 36, 5, 256, 8, 1, 2, 0, 0),
    "igrad-chunked": ("TGCNCheb_H", 23, 1, 36, 9, 8, 224, 2, 2, 1, 0),           # phase 0: 5 weight time rows of 224 channels
    "igrad-large": ("TGCNCheb_H", 23, 1, 36, 9, 8, 256, 2, 2, 0, 1),
}
REGIME = {"fwd-chunked-vec": (0, "lds64-chunked"), "fwd-chunked-narrow": (0, "lds64-chunked"), "fwd-large": (0, "large"),
          "igrad-chunked": (1, "lds64-chunked"), "igrad-large": (1, "large")}
DEGREE = ("vec8-f8-H15", "f3-g40-step3")          # also run on a degree-reordered operand

# fp64 tolerance per case and tensor (out, d series, dW, db) = 2 x the emulation's own rel_err against fp64, measured values in the comments
TOL64 = {
    "vec8-f8-H15": (6.0e-03, 5.6e-03, 5.5e-03, 4.8e-03),  # 2.98e-03 2.80e-03 2.76e-03 2.41e-03
    "vec8-f16-H15-g32": (5.5e-03, 6.5e-03, 6.2e-03, 6.3e-03),  # 2.73e-03 3.25e-03 3.08e-03 3.13e-03
    "f4-g80-even-step": (6.9e-03, 6.1e-03, 5.0e-03, 5.8e-03),  # 3.45e-03 3.07e-03 2.52e-03 2.92e-03
    "f3-g40-step3": (7.1e-03, 4.1e-03, 6.0e-03, 3.7e-03),  # 3.55e-03 2.07e-03 3.02e-03 1.87e-03
    "f1-as-series-g20": (7.4e-03, 8.1e-03, 6.0e-03, 3.5e-03),  # 3.70e-03 4.03e-03 2.99e-03 1.75e-03
    "short-recording": (6.7e-03, 3.8e-03, 7.1e-03, 3.6e-03),  # 3.35e-03 1.92e-03 3.57e-03 1.79e-03
    "step-over-H-f32": (5.5e-03, 4.0e-03, 5.4e-03, 3.6e-03),  # 2.77e-03 2.02e-03 2.72e-03 1.80e-03
    "pads-f8-K5": (5.3e-03, 3.5e-03, 6.2e-03, 6.3e-03),  # 2.64e-03 1.74e-03 3.08e-03 3.15e-03
    "f24-g48-row-wrap": (6.2e-03, 7.0e-03, 6.8e-03, 4.6e-03),  # 3.09e-03 3.48e-03 3.42e-03 2.32e-03
    "fwd-chunked-vec": (3.9e-03, 4.6e-03, 4.6e-03, 4.3e-03),  # 1.95e-03 2.28e-03 2.30e-03 2.17e-03
    "fwd-chunked-narrow": (5.1e-03, 4.3e-03, 6.8e-03, 7.0e-03),  # 2.54e-03 2.16e-03 3.39e-03 3.49e-03
    "fwd-large": (5.1e-03, 4.6e-03, 5.8e-03, 5.7e-03),  # 2.56e-03 2.29e-03 2.91e-03 2.85e-03
    "igrad-chunked": (5.8e-03, 4.7e-03, 6.4e-03, 3.8e-03),  # 2.91e-03 2.33e-03 3.19e-03 1.89e-03
    "igrad-large": (5.4e-03, 5.9e-03, 6.5e-03, 4.2e-03),  # 2.69e-03 2.95e-03 3.26e-03 2.09e-03
}


# ------------------------------------------------------------------------------------------------- cases (CPU) and references
def _graph(n, seed):
    """(scipy CSR L, edge_index) -- the dti148 golden operand, or a random graph with hubs as tests/test_series_conv.py builds them"""
    if n == 148:
        _, L = golden_graph("dti148")
        return L
    row, col, val = _random_graph(n, 6, np.random.default_rng(seed), hubs=((2, min(60, n - 1)),))
    return O.coo_to_csr(row, col, (val * 0.4).astype(np.float32), n)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """the bf16 layer (on the CPU), its graph arguments, L of the oracle, the mode, the fp32 series and upstream gradient (window-major)"""
    cls, n, S, T, H, f, g, K, stride, left, right = CASES[name]
    seed = sum(name.encode())
    L = _graph(n, seed)
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    if cls == "TGCNCheb_H":
        m = tgcn_amd.TGCNCheb_H(torch.as_tensor(L.toarray()), f, g, K, H)
        ei, L_op, mode = None, L, "power"
    else:
        r, c = L.nonzero()
        ei = torch.as_tensor(np.stack([r, c]).astype(np.int64))
        m = tgcn_amd.ChebTimeConv(f, g, K, H)
        row, col, lap = O.edge_laplacian(ei.numpy(), None, n)
        L_op, mode = O.coo_to_csr(row, col, lap, n), "chebyshev"
    with torch.no_grad():
        m.bias.uniform_(-0.5, 0.5)
    nwin = nwin_of(T, H, stride, left, right)
    series = rng.standard_normal((S, n, T, f)).astype(np.float32)
    go = rng.standard_normal((S * nwin, n, g)).astype(np.float32)
    return m.to(BF), ei, L_op, mode, series, go


def _arrays(m, series, go):
    """(series, W (K, H, f, N), bias, g) as fp64 numpy of the bf16 values the layer computes with"""
    W = m.weight.detach().double().numpy()
    b = None if m.bias is None else m.bias.detach().double().numpy()
    return bf(series), W, b, bf(go)


def _win(x3, dims, geom):
    S, n, T, f, H = dims
    nwin = nwin_of(T, H, *geom)
    return windows_conv(x3.reshape(S, n, T, f), H, *geom).reshape(S * nwin, n, H * f)


def _unwin(gxw, dims, geom):
    S, n, T, f, H = dims
    return fold_conv(gxw.reshape(-1, n, H, f), S, T, *geom)


def series_fp64(L, xs, W, b, g, mode, geom):
    """the oracle on the materialised windows, d series folded back onto the series"""
    S, n, T, f = xs.shape
    K, H, _, N = W.shape
    dims = (S, n, T, f, H)
    y, gxw, gW, gb = fp64_reference(L, _win(xs.reshape(S, n, T * f), dims, geom), W.reshape(K, H * f, N), b, g, mode)
    return y, _unwin(gxw, dims, geom), gW.reshape(W.shape), gb


def series_emulate(L, xs, W, b, g, mode, geom):
    """ChebSeriesBf16Fn in fp64 with its rounding points; inputs already bf16 values"""
    S, n, T, f = xs.shape
    K, H, _, N = W.shape
    dims = (S, n, T, f, H)
    L64 = sp.csr_matrix(L, dtype=np.float64)
    LT = L64.T.tocsr()
    mono = mode == "power"
    c = _fold(K) if mono and K > 2 else None
    W3 = W.reshape(K, H * f, N)
    Wt = bf(np.einsum("kj,kcn->jcn", c, W3)) if c is not None else W3        # folded in fp32, rounded once
    terms = [xs.reshape(S, n, T * f)]                                        # the bf16 hops on rows of T*f elements: every hop rounds
    for k in range(1, K):
        if mono or k == 1:
            terms.append(bf(_apply(L64, terms[k - 1])))
        else:
            terms.append(bf(2 * _apply(L64, terms[k - 1]) - terms[k - 2]))
    tw = [_win(t, dims, geom) for t in terms]
    y = bf(_bias_add(sum(np.einsum("qnc,cg->qng", tw[k], Wt[k]) for k in range(K)), b))
    dWt = np.stack([np.einsum("qnc,qng->cg", tw[k], g) for k in range(K)])
    gW = bf(np.einsum("kj,jcn->kcn", c, dWt) if c is not None else dWt).reshape(W.shape)
    gx = np.zeros((S, n, T * f))
    for k in range(K):                                                       # fp32 G, fp32 adjoint hops, one rounding
        P = _unwin(np.einsum("qng,cg->qnc", g, Wt[k]), dims, geom).reshape(S, n, T * f)
        if mono:
            for _ in range(k):
                P = _apply(LT, P)
            gx += P
        else:
            gx += O.stack_chebyshev(LT, P, k + 1)[k]
    gb = None if b is None else bf((g.sum(axis=(0, 1)) if b.size == g.shape[2] else g.sum(axis=0)).reshape(b.shape))
    return y, bf(gx).reshape(xs.shape), gW, gb


@functools.lru_cache(maxsize=None)
def references(name):
    """(fp64 reference, emulation) of a case, computed once and left unchanged"""
    m, ei, L, mode, series, go = make_case(name)
    geom = CASES[name][8:]
    xs, W, b, g = _arrays(m, series, go)
    return series_fp64(L, xs, W, b, g, mode, geom), series_emulate(L, xs, W, b, g, mode, geom)


def _round2(v):
    return float("%.1e" % v)


def test_tolerances_are_twice_the_emulations_error():
    """TOL64 is what its comment says: every row recomputed here on the CPU"""
    assert set(TOL64) == set(CASES)
    for name in CASES:
        ref, emu = references(name)
        assert tuple(_round2(2 * rel_err(e, r)) for e, r in zip(emu, ref)) == TOL64[name], name


# ------------------------------------------------------------------------------------------------- running on the device
def _to_series(a, S, nwin):
    return np.ascontiguousarray(a.reshape((S, nwin) + a.shape[1:]).transpose(0, 2, 1, 3))


class Runner:
    def __init__(self, name, dev, kind=None):
        self.name = name
        cls, n, S, T, H, f, g, K, stride, left, right = CASES[name]
        m, ei, L, mode, series, go = make_case(name)
        import copy
        self.m = m = copy.deepcopy(m).to(dev)
        self.geo = dict(stride=stride, padding=padding_arg(H, left, right))
        self.S, self.nwin = S, nwin_of(T, H, stride, left, right)
        self.series, self.go = series, go
        self.squeeze = f == 1
        if cls == "TGCNCheb_H":
            if kind is None:
                self.call = lambda s, a: m.forward_series(s, as_series=a, **self.geo)
            else:
                op = m._operand(dev).reordered(kind)
                self.call = lambda s, a: F.cheb_time_windows(op, s, m.weight.reshape(K, H, g) if s.dim() == 3 else m.weight, m.bias.reshape(-1),
                                                             F.BIAS_VERTEX_CHANNEL, F.MODE_POWER, as_series=a, **self.geo)
        else:
            eid = ei.to(dev)
            if kind is None:
                self.call = lambda s, a: m.forward_series(s, eid, None, as_series=a, **self.geo)
            else:
                op = m._operand(torch.empty(1, n, 1, device=dev), eid, None).reordered(kind)
                self.call = lambda s, a: F.cheb_time_windows(op, s, m.weight, m.bias, F.BIAS_CHANNEL, F.MODE_CHEBYSHEV, as_series=a, **self.geo)

    def run(self, as_series, series_grad=True):
        """(out, d series, dW, db) as tensors; out and the upstream gradient in the layout asked for"""
        self.m.zero_grad()
        s = torch.as_tensor(self.series[..., 0] if self.squeeze else self.series, device=self.m.weight.device).to(BF).requires_grad_(series_grad)
        out = self.call(s, as_series)
        go = _to_series(self.go, self.S, self.nwin) if as_series else self.go
        out.backward(torch.as_tensor(go, device=out.device).to(BF))
        return out.detach(), s.grad, self.m.weight.grad, self.m.bias.grad if self.m.bias is not None else None


def _compare(name, got, which=(0, 1, 2, 3)):
    """got: (out window-major, d series, dW, db) -> asserts both bounds per tensor"""
    ref, emu = references(name)
    tol = TOL64[name]
    for i, label in enumerate(("out", "ds", "dW", "db")):
        if i not in which or got[i] is None:
            continue
        gv = got[i].detach().double().cpu().numpy().reshape(ref[i].shape)
        scale = np.abs(emu[i]).max()
        d_emu, e64 = float(np.abs(gv - emu[i]).max() / scale), rel_err(gv, ref[i])
        print(name, label, "vs emulation %.2e (bound %.2e)" % (d_emu, EMUL_ULPS * 2.0 ** -8), "vs fp64 %.2e (bound %.1e)" % (e64, tol[i]))
        assert d_emu <= EMUL_ULPS * 2.0 ** -8, (name, label, d_emu)
        assert e64 <= tol[i], (name, label, e64, tol[i])


def _check(name, dev, kind=None):
    cls, n, S, T, H, f, g, K, stride, left, right = CASES[name]
    r = Runner(name, dev, kind)
    nwin = r.nwin
    first = f == 1                       # one channel: as_series first (the window-major call needs a geometry; this case has none)
    out_s, ds_s, dW_s, db_s = r.run(True)
    assert out_s.dtype == BF and tuple(out_s.shape) == (S, n, nwin, g) and out_s.is_contiguous()
    assert ds_s.dtype == BF and dW_s.dtype == BF and db_s.dtype == BF
    wm = out_s.view(S, n, nwin, g).permute(0, 2, 1, 3).reshape(S * nwin, n, g)
    _compare(name, (wm, ds_s, dW_s.clone(), db_s.clone()))
    if first and (stride, left, right) == (1, 0, 0):
        return
    out, ds, dW, db = r.run(False)
    assert out.dtype == BF and tuple(out.shape) == (S * nwin, n, g)
    assert torch.equal(out_s, out.view(S, nwin, n, g).permute(0, 2, 1, 3))
    _compare(name, (out, ds, dW, db))


def plan_bf16(H, f, N, stride, vec=None):
    hc, lds = C.c_int32(-1), C.c_int32(-1)
    rc = _lib.lib().tgcn_series_conv_plan_bf16(H, f, N, int(f % 8 == 0) if vec is None else int(vec), stride, C.byref(hc), C.byref(lds))
    return rc, hc.value, lds.value


def _regime(H, f, N, stride):
    rc, hc, lds = plan_bf16(H, f, N, stride)
    if rc != OK:
        assert rc == UNSUPPORTED, rc
        return "unsupported"
    assert 1 <= hc <= H and 0 < lds, (hc, lds)
    return ("large" if lds > KB64 else "lds64") + ("-whole" if hc == H else "-chunked")


def _regimes(name):
    """(forward, input gradient: phase 0 at step 1 on g as a series of g channels)"""
    cls, n, S, T, H, f, g, K, stride, left, right = CASES[name]
    return _regime(H, f, g, stride), _regime(-(-H // stride), g, K * f, 1)


# ------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", [k for k, v in REGIME.items() if v[1] == "lds64-chunked"])
def test_plan_chunks_these_shapes(name):
    """the 64 KB limit is tried first, so these answers hold with and without a device"""
    direction, want = REGIME[name]
    assert _regimes(name)[direction] == want


@gpu
@pytest.mark.parametrize("name", [k for k in CASES if k not in REGIME])
def test_bf16_series_vs_oracle_and_emulation(name, gpu_device):
    require_series_bf16_entries()
    _check(name, gpu_device)
    if name == "step-over-H-f32":        # time rows 5, 6 (mod 7) lie between the windows: exact zeros, not rounding noise
        r = Runner(name, gpu_device)
        ds = r.run(False)[1]
        assert not ds[:, :, 5::7].any() and not ds[:, :, 6::7].any() and ds[:, :, 4::7].any()


@gpu
@pytest.mark.parametrize("name", list(REGIME))
def test_bf16_series_regimes(name, gpu_device):
    require_series_bf16_entries()
    direction, want = REGIME[name]
    got = _regimes(name)[direction]
    assert got.startswith(want), "%s: the launcher plans %s, this case is here for %s" % (name, got, want)
    _check(name, gpu_device)


@gpu
@pytest.mark.parametrize("name", DEGREE)
def test_bf16_series_on_a_reordered_operand(name, gpu_device):
    require_series_bf16_entries()
    _check(name, gpu_device, "degree")


@gpu
def test_refusal_at_the_device_limit(gpu_device):
    """so many channels that one weight time row fits no LDS: the query says so, the call raises before its hops, the entry launches nothing"""
    require_series_bf16_entries()
    n, S, T, H, g, K, stride = 23, 1, 36, 3, 8, 2, 2
    f = next((c for c in range(8, 16384, 8) if plan_bf16(H, c, g, stride)[0] == UNSUPPORTED), None)
    assert f is not None and plan_bf16(H, f - 8, g, stride)[0] == OK and plan_bf16(H, f - 8, g, stride)[2] > KB64, f
    print("first refused f:", f)
    m = tgcn_amd.TGCNCheb_H(torch.eye(n), f, g, K, H).to(gpu_device).to(BF)
    with pytest.raises(_lib.TgcnError):
        m.forward_series(torch.zeros(S, n, T, f, device=gpu_device, dtype=BF), stride=stride, padding=1)
    assert b"LDS" in _lib.lib().tgcn_last_error()
    out = torch.full((S * 18, n, g), float("nan"), device=gpu_device, dtype=BF)
    stack, W = torch.zeros(K, S, n, T * f, device=gpu_device, dtype=BF), torch.zeros(K, H * f, g, device=gpu_device, dtype=BF)
    rc = _lib.lib().tgcn_cheb_project_series_conv_bf16(_lib.stream_ptr(), S, n, T, f, H, g, K, _lib.ptr(stack), T * f, _lib.ptr(W), None, 0, 0, 0,
                                                       _lib.ptr(out), stride, 1, 1)
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED and torch.isnan(out).all()


# ---------------------------------------------------------------------------------------------------------------- one-sided backwards
ONE_SIDED = "pads-f8-K5"


@gpu
def test_backward_without_the_series_gradient(gpu_device):
    require_series_bf16_entries()
    r = Runner(ONE_SIDED, gpu_device)
    out, ds, dW, db = r.run(False, series_grad=False)
    assert ds is None
    _compare(ONE_SIDED, (out, None, dW, db))


@gpu
def test_backward_with_frozen_parameters(gpu_device):
    require_series_bf16_entries()
    r = Runner(ONE_SIDED, gpu_device)
    r.m.requires_grad_(False)
    out, ds, dW, db = r.run(True)
    assert dW is None and db is None
    _compare(ONE_SIDED, (None, ds, None, None), which=(1,))


@gpu
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
def test_no_bias(as_series, gpu_device):
    require_series_bf16_entries()
    cls, n, S, T, H, f, g, K, stride, left, right = CASES[ONE_SIDED]
    r = Runner(ONE_SIDED, gpu_device)
    m, ei, L, mode, series, go = make_case(ONE_SIDED)
    xs, W, b, gg = _arrays(m, series, go)
    ref = series_fp64(L, xs, W, None, gg, mode, (stride, left, right))
    emu = series_emulate(L, xs, W, None, gg, mode, (stride, left, right))
    op = r.m._operand(torch.empty(1, n, 1, device=gpu_device), ei.to(gpu_device), None)
    r.m.zero_grad()
    s = torch.as_tensor(series, device=gpu_device).to(BF).requires_grad_(True)
    out = F.cheb_time_windows(op, s, r.m.weight, None, F.BIAS_NONE, F.MODE_CHEBYSHEV, as_series=as_series, **r.geo)
    out.backward(torch.as_tensor(_to_series(go, S, r.nwin) if as_series else go, device=gpu_device).to(BF))
    assert r.m.bias.grad is None
    wm = out.detach().permute(0, 2, 1, 3).reshape(S * r.nwin, n, g) if as_series else out.detach()
    tol = TOL64[ONE_SIDED]
    for i, (label, t) in enumerate((("out", wm), ("ds", s.grad), ("dW", r.m.weight.grad))):
        gv = t.double().cpu().numpy().reshape(ref[i].shape)
        scale = np.abs(emu[i]).max()
        assert np.abs(gv - emu[i]).max() <= EMUL_ULPS * 2.0 ** -8 * scale, label
        assert rel_err(gv, ref[i]) <= tol[i], (label, rel_err(gv, ref[i]))


# ---------------------------------------------------------------------------------------------------------------- chain and capture
def _chain(dev):
    n = 148
    L = _graph(n, 0)
    Ld = torch.as_tensor(L.toarray())
    torch.manual_seed(7)
    l1, l2 = tgcn_amd.TGCNCheb_H(Ld, 1, 8, 4, 5), tgcn_amd.TGCNCheb_H(Ld, 8, 16, 3, 4)
    with torch.no_grad():
        l1.bias.uniform_(-0.5, 0.5)
        l2.bias.uniform_(-0.5, 0.5)
    return L, l1.to(BF), l2.to(BF)


def _chain_emulation():
    """l1(as_series, causal) -> relu -> l2(stride 2) emulated on the bf16-rounded series and upstream gradient.  (No fp64 bound here: a hidden
    value that rounding moves across zero switches its relu, which no tolerance on the series' gradient covers; the layers have theirs above.)"""
    n, S, T, H1, H2 = 148, 2, 30, 5, 4
    L, l1, l2 = _chain(None)
    rng = np.random.default_rng(78)
    series = rng.standard_normal((S, n, T)).astype(np.float32)
    nwin2 = nwin_of(T, H2, 2, 0, 0)
    go = rng.standard_normal((S, n, nwin2, 16)).astype(np.float32)
    xs = bf(series)[..., None]
    g2 = bf(np.ascontiguousarray(go.transpose(0, 2, 1, 3)).reshape(S * nwin2, n, 16))
    W1, b1 = l1.weight.detach().double().numpy(), l1.bias.detach().double().numpy()
    W2, b2 = l2.weight.detach().double().numpy(), l2.bias.detach().double().numpy()
    y1 = series_emulate(L, xs, W1, b1, np.zeros((S * T, n, 8)), "power", (1, H1 - 1, 0))[0]
    hid = np.ascontiguousarray(np.maximum(y1, 0).reshape(S, T, n, 8).transpose(0, 2, 1, 3))         # (S, n, T, 8): a series again
    y2, ghid, _, _ = series_emulate(L, hid, W2, b2, g2, "power", (2, 0, 0))
    g1 = np.ascontiguousarray((ghid * (hid > 0)).transpose(0, 2, 1, 3)).reshape(S * T, n, 8)
    gs = series_emulate(L, xs, W1, b1, g1, "power", (1, H1 - 1, 0))[1]
    return series, go, (y2.reshape(S, nwin2, n, 16).transpose(0, 2, 1, 3), gs[..., 0])


@gpu
def test_bf16_chain_vs_emulation(gpu_device):
    """l2.forward_series(relu(l1.forward_series(x, as_series=True, padding="causal")), as_series=True, stride=2), all bf16: the hidden series is
    bf16 and feeds the second layer with no cast"""
    require_series_bf16_entries()
    series, go, emu = _chain_emulation()
    L, l1, l2 = _chain(gpu_device)
    l1, l2 = l1.to(gpu_device), l2.to(gpu_device)
    st = torch.as_tensor(series, device=gpu_device).to(BF).requires_grad_(True)
    h = torch.relu(l1.forward_series(st, as_series=True, padding="causal"))
    assert h.dtype == BF and tuple(h.shape) == (2, 148, 30, 8)
    out = l2.forward_series(h, as_series=True, stride=2)
    assert out.dtype == BF and out.is_contiguous()
    out.backward(torch.as_tensor(go, device=gpu_device).to(BF))
    for i, (label, t) in enumerate((("out", out.detach()), ("ds", st.grad))):
        gv = t.double().cpu().numpy()
        d_emu = float(np.abs(gv - emu[i]).max() / np.abs(emu[i]).max())
        print("chain", label, "vs emulation %.2e" % d_emu)
        assert d_emu <= EMUL_ULPS * 2.0 ** -8, (label, d_emu)


@gpu
def test_bf16_strided_step_is_graph_capturable(gpu_device):
    """forward + backward at stride 3 (three phase launches from a host loop) inside torch.cuda.graph, replayed once: the eager numbers.  The
    launches are sequential on one stream."""
    require_series_bf16_entries()
    n, S, T = 148, 2, 30
    L, l1, l2 = _chain(gpu_device)
    l2 = l2.to(gpu_device)
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((S, n, T, 8), device="cuda", generator=gen).to(BF).requires_grad_(True)
    params = [x, l2.weight, l2.bias]

    def step():
        for p in params:
            p.grad = None
        out = l2.forward_series(x, as_series=True, stride=3, padding=(2, 1))
        out.backward(torch.ones_like(out))
        return out

    eager = [step().detach().clone()] + [p.grad.clone() for p in params]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                             # warm-up on the side stream (schedules, allocator)
    torch.cuda.current_stream().wait_stream(side)
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_static = step()
    graph.replay()
    torch.cuda.synchronize()
    got = [out_static] + [p.grad for p in params]
    assert all(t.dtype == BF for t in got)
    assert all(torch.equal(a, b) for a, b in zip(got, eager))


# ---------------------------------------------------------------------------------------------------------------- the C ABI directly
def _raw_reference(stack, W, bias, g, dims, geom):
    """fp64 sums of the raw entries on given bf16 values: out (window-major), G (K, S, n, T*f), dW"""
    S, n, T, f, H = dims
    K = W.shape[0]
    tw = [_win(stack[k], dims, geom) for k in range(K)]
    out = sum(np.einsum("qnc,cg->qng", tw[k], W[k]) for k in range(K)) + bias
    G = np.stack([_unwin(np.einsum("qng,cg->qnc", g, W[k]), dims, geom).reshape(S, n, T * f) for k in range(K)])
    dW = np.stack([np.einsum("qnc,qng->cg", tw[k], g) for k in range(K)])
    return out, G, dW


@gpu
def test_raw_entries_with_padded_rows_and_null_outputs(gpu_device):
    """the C ABI directly: a stack whose vertex rows carry trailing padding (stack_ld > T*f, filled with NaN: never read), fp32 bias; then the
    backward with G, with dW, and with each null"""
    require_series_bf16_entries()
    Lb = _lib.lib()
    n, S, T, f, H, N, K, stride, left, right = 29, 2, 21, 8, 5, 24, 2, 2, 1, 2
    ld = T * f + 16
    nwin = nwin_of(T, H, stride, left, right)
    dims, geom = (S, n, T, f, H), (stride, left, right)
    rng = np.random.default_rng(3)
    stack = bf(rng.standard_normal((K, S, n, T * f)))
    W, g, bias = bf(rng.standard_normal((K, H * f, N)) * 0.2), bf(rng.standard_normal((S * nwin, n, N))), rng.standard_normal(N).astype(np.float32)
    ref_out, ref_G, ref_dW = _raw_reference(stack, W, bias.astype(np.float64), g, dims, geom)
    st = torch.full((K, S, n, ld), float("nan"), device=gpu_device, dtype=BF)
    st[..., :T * f] = torch.as_tensor(stack, device=gpu_device).to(BF)
    Wd, gd = (torch.as_tensor(a, device=gpu_device).to(BF) for a in (W, g))
    bd = torch.as_tensor(bias, device=gpu_device)
    out = torch.full((S * nwin, n, N), float("nan"), device=gpu_device, dtype=BF)
    head = (_lib.stream_ptr(), S, n, T, f, H, N, K, _lib.ptr(st), ld)
    _lib.check(Lb.tgcn_cheb_project_series_conv_bf16(*head, _lib.ptr(Wd), _lib.ptr(bd), _lib.DTYPE_F32, 1, 0, _lib.ptr(out), stride, left, right))
    # one rounding of an fp32 sum of exact products: half a bf16 ulp of the value, plus the fp32 sum's own error
    o = out.double().cpu().numpy()
    assert np.abs(o - ref_out).max() <= 2.0 ** -8 * np.abs(ref_out).max()
    need = Lb.tgcn_cheb_series_conv_backward_bf16_workspace_bytes(S, n, T, f, H, N, K, stride, left, right)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    tail = (_lib.ptr(ws), need, stride, left, right)

    def backward(want_G, want_dW):
        G = torch.full((K, S, n, T * f), float("nan"), device=gpu_device) if want_G else None
        dW = torch.full((K, H * f, N), float("nan"), device=gpu_device) if want_dW else None
        _lib.check(Lb.tgcn_cheb_series_conv_backward_bf16(*head[:8], _lib.ptr(st) if want_dW else None, ld, _lib.ptr(gd), 0,
                                                          _lib.ptr(Wd) if want_G else None, _lib.ptr(G), _lib.ptr(dW), *tail))
        torch.cuda.synchronize()
        return G, dW

    G, dW = backward(True, True)
    assert rel_err(G.double().cpu().numpy(), ref_G) <= 1e-5 and rel_err(dW.double().cpu().numpy(), ref_dW) <= 1e-5       # fp32 sums of exact products
    G2, none = backward(True, False)
    assert none is None and torch.equal(G2, G)
    none, dW2 = backward(False, True)
    assert none is None and torch.equal(dW2, dW)                # block-order fold: bit-equal across runs
    assert backward(False, False) == (None, None)
    # argument checks of the fp32 entries: null g, a stack_ld below T*f, a host pointer
    assert Lb.tgcn_cheb_series_conv_backward_bf16(*head[:8], _lib.ptr(st), ld, None, 0, _lib.ptr(Wd), None, None, *tail) == -1
    assert Lb.tgcn_cheb_project_series_conv_bf16(*head[:8], _lib.ptr(st), T * f - 1, _lib.ptr(Wd), None, 0, 0, 0, _lib.ptr(out), stride, left, right) == -1
    assert Lb.tgcn_cheb_project_series_conv_bf16(*head, _lib.ptr(Wd), None, 0, 0, 0, None, stride, left, right) == -1
