"""The streaming time-window layers with dilated taps: forward_series / F.cheb_time_windows with `dilation`, against the fp64 oracle run on
the host-materialised dilated windows

    xw[s*nwin + w, i, h, c] = padded_series[s, i, w + h*dilation, c],     nwin = T + left + right - He + 1,  He = (H - 1)*dilation + 1

(the technique of tests/test_series_channels.py: outputs O.tgcn_cheb_h_forward / O.cheb_time_conv_forward, gradients O.layer_backward folded
back onto the series, the padding rows dropped).  The project's bounds of that file: outputs 1e-5, gradients 2e-5 of the tensor's maximum.
Every shape runs for both classes, in both output layouts (torch.equal to each other), with a bias and with bias=None, on a plain and on a
degree-reordered operand.  Then the C ABI directly: the dilated forward is bit-identical, phase by phase, to the plain entry on that phase's
sub-stack, and the `_dilated` entries at dilation 1 are bit-identical to the `_conv` entries."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cheb_oracle as O
from test_hip_parity import _random_graph
from test_series_channels import TOL, TOL_GRAD, _dev, _to_series

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]

N_VERT, S_REC, K_TERMS = 48, 2, 3


def span_of(H, d):
    return (H - 1) * d + 1


def nwin_of(T, H, d, left, right):
    return T + left + right - span_of(H, d) + 1


def windows_dilated(series, H, d, left, right):
    """the windowed batch of the padded, dilated rule, (S*nwin, n, H, f)"""
    S, n, T, f = series.shape
    pad = np.zeros((S, n, T + left + right, f), dtype=series.dtype)
    pad[:, :, left:left + T] = series
    nwin = nwin_of(T, H, d, left, right)
    idx = np.arange(nwin)[:, None] + np.arange(H)[None, :] * d                 # (nwin, H) time rows of the padded series
    return np.ascontiguousarray(pad[:, :, idx].transpose(0, 2, 1, 3, 4)).reshape(S * nwin, n, H, f)


def fold_dilated(gxw, S, T, d, left, right):
    """d series from the gradient of that batch: every tap adds into the padded time row it was read from; the padding rows are dropped"""
    _, n, H, f = gxw.shape
    nwin = nwin_of(T, H, d, left, right)
    gxw = gxw.reshape(S, nwin, n, H, f)
    gs = np.zeros((S, n, T + left + right, f))
    for h in range(H):
        gs[:, :, h * d:h * d + nwin] += gxw[:, :, :, h].transpose(0, 2, 1, 3)
    return gs[:, :, left:left + T]


def padding_arg(H, d, left, right):
    """the spelling a caller would use"""
    if (left, right) == (span_of(H, d) - 1, 0):
        return "causal"
    return left if left == right else (left, right)


def test_window_rule_of_the_helpers():
    """windows_dilated / fold_dilated are adjoint, and dilation 1 is the plain rule"""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 3, 11, 2))
    xw = windows_dilated(x, 3, 4, 2, 5)
    assert xw.shape == (2 * nwin_of(11, 3, 4, 2, 5), 3, 3, 2) and nwin_of(11, 3, 4, 2, 5) == 10
    assert np.array_equal(xw[2, :, 1], x[0, :, 4]) and not xw[0, :, 0].any()        # window 2, tap 1: padded row 6 = row 4; window 0 starts in the padding
    g = rng.standard_normal(xw.shape)
    assert abs((xw * g).sum() - (x * fold_dilated(g, 2, 11, 4, 2, 5)).sum()) < 1e-9
    assert np.array_equal(windows_dilated(x, 3, 1, 0, 0)[1, :, :], x[0, :, 1:4])


class Setup:
    """One class on the 48-vertex graph: the layer, the operand (plain, and degree-reordered on request) and the fp64 references"""

    def __init__(self, cls, f, g, H, seed):
        import tgcn_amd
        from tgcn_amd import functional as F
        n, K = N_VERT, K_TERMS
        rng = np.random.default_rng(seed)
        row, col, val = _random_graph(n, 6, rng, hubs=((2, n - 1),))
        val = val * 0.4
        torch.manual_seed(seed)
        self.cls, self.F = cls, F
        if cls == "TGCNCheb_H":
            self.L = O.coo_to_csr(row, col, val, n)
            self.op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val))
            self.layer = layer = tgcn_amd.TGCNCheb_H(self.op, f, g, K, H).cuda()
            self.mode, self.fmode, self.bias_kind = "power", F.MODE_POWER, F.BIAS_VERTEX_CHANNEL
            self.module = lambda s, **kw: layer.forward_series(s, **kw)
            self.forward64 = lambda xw, b: O.tgcn_cheb_h_forward(self.L, xw, self.W64(), b)
            self.bias_grad = lambda go: go.astype(np.float64).sum(axis=0, keepdims=True)
        else:
            ei = np.stack([row, col]).astype(np.int64)
            r, c, lap = O.edge_laplacian(ei, None, n)
            self.L = O.coo_to_csr(r, c, lap, n)
            self.layer = layer = tgcn_amd.ChebTimeConv(f, g, K, H).cuda()
            self.mode, self.fmode, self.bias_kind = "chebyshev", F.MODE_CHEBYSHEV, F.BIAS_CHANNEL
            eid = _dev(ei)
            self.op = layer._operand(torch.empty(1, n, 1, device="cuda"), eid, None)
            self.module = lambda s, **kw: layer.forward_series(s, eid, None, **kw)
            self.forward64 = lambda xw, b: O.cheb_time_conv_forward(xw, ei, None, self.W64(), b)
            self.bias_grad = lambda go: go.astype(np.float64).sum(axis=(0, 1))
        with torch.no_grad():
            layer.bias.uniform_(-0.5, 0.5)
        self.reordered = None

    def W64(self):
        return self.layer.weight.detach().cpu().numpy()

    def call(self, s, kind, bias, **kw):
        """the streaming call: the module on its own operand with its bias, the functional entry for a reordered operand or no bias"""
        if kind is None and bias:
            return self.module(s, **kw)
        op = self.op
        if kind is not None:
            if self.reordered is None:
                self.reordered = self.op.reordered(kind)
            op = self.reordered
        W = self.layer.weight if s.dim() == 4 else self.layer.weight.reshape(K_TERMS, self.layer.weight.shape[1], -1)
        return self.F.cheb_time_windows(op, s, W, self.layer.bias.reshape(-1) if bias else None, self.bias_kind if bias else self.F.BIAS_NONE,
                                        self.fmode, **kw)


def _run(su, series, go, kind, bias, as_series, geo, need_series=True):
    """(out, d series, dW, db) of one streaming forward + backward; go in the layout of the output"""
    su.layer.zero_grad()
    squeeze = series.shape[3] == 1           # a single channel is given as a 3-D series
    st = _dev(series[..., 0] if squeeze else series).requires_grad_(need_series)
    out = su.call(st, kind, bias, as_series=as_series, **geo)
    out.backward(_dev(go))
    ds = None if st.grad is None else st.grad.cpu().numpy().reshape(series.shape)
    dW = None if su.layer.weight.grad is None else su.layer.weight.grad.cpu().numpy().copy()
    db = None if su.layer.bias.grad is None else su.layer.bias.grad.cpu().numpy().copy()
    return out.detach(), ds, dW, db


def _reference(su, T, H, f, g, d, left, right, rng):
    """series, gradient of the output (window-major) and the fp64 references (out with bias, out without, d series, dW, db), computed once"""
    S, n = S_REC, N_VERT
    nwin = nwin_of(T, H, d, left, right)
    series = rng.standard_normal((S, n, T, f)).astype(np.float32)
    xw = windows_dilated(series, H, d, left, right).astype(np.float64)
    ref_b, ref_0 = su.forward64(xw, su.layer.bias.detach().cpu().numpy()), su.forward64(xw, None)
    go = rng.standard_normal((S * nwin, n, g)).astype(np.float32)
    gxw, gW = O.layer_backward(su.L, xw, su.W64(), go, su.mode)
    return series, go, ref_b, ref_0, fold_dilated(gxw, S, T, d, left, right), gW, su.bias_grad(go)


def _check(cls, shape):
    """every operand kind, with and without the bias, both layouts"""
    T, H, d, f, g, left, right = shape
    S, n = S_REC, N_VERT
    nwin = nwin_of(T, H, d, left, right)
    geo = dict(padding=padding_arg(H, d, left, right), dilation=d)
    su = Setup(cls, f, g, H, seed=T + 7 * d + f)
    series, go, ref_b, ref_0, gs, gW, gb = _reference(su, T, H, f, g, d, left, right, np.random.default_rng([T, d, f, g]))
    go_s = np.ascontiguousarray(_to_series(go, S, nwin))
    for kind in (None, "degree"):
        for bias in (True, False):
            ref = ref_b if bias else ref_0
            out, ds, dW, db = _run(su, series, go, kind, bias, False, geo)
            assert tuple(out.shape) == (S * nwin, n, g)
            errs = dict(out=rel_err(out.cpu().numpy(), ref), ds=rel_err(ds, gs), dW=rel_err(dW, gW))
            out_s, ds_s, dW_s, db_s = _run(su, series, go_s, kind, bias, True, geo)
            assert tuple(out_s.shape) == (S, n, nwin, g) and out_s.is_contiguous()
            assert torch.equal(out_s, out.view(S, nwin, n, g).permute(0, 2, 1, 3)), (kind, bias)
            errs.update(ds_s=rel_err(ds_s, gs), dW_s=rel_err(dW_s, gW))
            if bias:
                errs.update(db=rel_err(db.reshape(gb.shape), gb), db_s=rel_err(db_s.reshape(gb.shape), gb))
            else:
                assert db is None and db_s is None
            print(cls, shape, kind, "bias" if bias else "no bias", errs)
            assert errs.pop("out") <= TOL, (kind, bias)
            assert max(errs.values()) <= TOL_GRAD, (kind, bias, errs)
    return su, series, go, ref_b, gs, gW, gb, geo


CLASSES = ["TGCNCheb_H", "ChebTimeConv"]

# (T, H, d, f, g, left, right)
UNEQUAL = [(50, 5, d, f, g, 0, 0) for d in (3, 7) for f in (1, 3, 4, 8) for g in (5, 40)]     # nwin = 38 / 22: nwin % d != 0, partial tiles
EMPTY = [(20, 3, 9, 4, 8, 0, 0)]                                                              # nwin = 2 < d: phases without a window
TILES = [(150, 3, 2, 4, 8, 0, 0),                                                             # nwin = 146: 73 windows per phase, 2 full tiles + 9
         (69, 3, 2, 4, 8, 0, 0)]                                                              # nwin = 65: 33 and 32 windows, the second phase's
                                                                                              # last tile starts past its last window (a dead wave)
NEGATIVE = [(50, 5, d, f, g, left, right) for d in (3, 7) for f in (1, 3, 4, 8) for g in (5, 40)
            for left, right in (((5 - 1) * d, 0), (2, 5))]                                    # window starts below 0: "causal" and (2, 5)
CHUNKED = [(70, 28, 2, 64, 40, 0, 0)]                                                         # the step-1 plan answers HC < H (asserted below)


def _id(s):
    return "T%d_H%d_d%d_f%d_g%d_l%d_r%d" % s


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", UNEQUAL + EMPTY + TILES + NEGATIVE, ids=_id)
def test_dilated_series_vs_oracle(shape, cls, gpu_device):
    T, H, d, f, g, left, right = shape
    nwin = nwin_of(T, H, d, left, right)
    if shape in UNEQUAL:
        assert nwin % d != 0
    if shape in EMPTY:
        assert d > nwin
    if shape == TILES[0]:
        assert -(-nwin // d) == 73
    if shape == TILES[1]:
        assert -(-nwin // d) == 33 and (nwin - 1) // d == 32
    _check(cls, shape)


def conv_plan(H, f, N, stride=1):
    from tgcn_amd import _lib
    hc, lds = C.c_int32(-1), C.c_int32(-1)
    rc = _lib.lib().tgcn_series_conv_plan(H, f, N, int(f % 4 == 0), stride, C.byref(hc), C.byref(lds))
    return rc, hc.value, lds.value


def test_plan_chunks_the_chunked_shape():
    """the 64 KB limit is tried first, so this answer holds with and without a device; the dilation does not enter the query"""
    T, H, d, f, g, left, right = CHUNKED[0]
    rc, hc, lds = conv_plan(H, f, g)
    assert rc == 0 and 1 <= hc < H and lds <= 64 * 1024, (rc, hc, lds)


@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_dilated_series_with_a_chunked_span(cls, gpu_device):
    T, H, d, f, g, left, right = CHUNKED[0]
    rc, hc, lds = conv_plan(H, f, g)
    assert rc == 0 and hc < H, "this case is here for the chunked regime, the launcher plans HC = %d of %d" % (hc, H)
    _check(cls, CHUNKED[0])


# ---------------------------------------------------------------------------------------------------------------- one-sided backwards
ONE_SIDED = (50, 5, 3, 4, 40, 2, 5)


@functools.lru_cache(maxsize=None)
def _one_sided(cls):
    T, H, d, f, g, left, right = ONE_SIDED
    su = Setup(cls, f, g, H, seed=5)
    return (su, dict(padding=(left, right), dilation=d)) + _reference(su, T, H, f, g, d, left, right, np.random.default_rng(11))


@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_backward_without_the_series_gradient(cls, gpu_device):
    su, geo, series, go, ref_b, ref_0, gs, gW, gb = _one_sided(cls)
    out, ds, dW, db = _run(su, series, go, None, True, False, geo, need_series=False)
    assert ds is None
    errs = dict(out=rel_err(out.cpu().numpy(), ref_b), dW=rel_err(dW, gW), db=rel_err(db.reshape(gb.shape), gb))
    print(errs)
    assert errs["out"] <= TOL and max(errs["dW"], errs["db"]) <= TOL_GRAD, errs


@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_backward_with_frozen_parameters(cls, gpu_device):
    su, geo, series, go, ref_b, ref_0, gs, gW, gb = _one_sided(cls)
    T, H, d, f, g, left, right = ONE_SIDED
    su.layer.requires_grad_(False)
    try:
        out, ds, dW, db = _run(su, series, np.ascontiguousarray(_to_series(go, S_REC, nwin_of(T, H, d, left, right))), None, True, True, geo)
    finally:
        su.layer.requires_grad_(True)
    assert dW is None and db is None
    e = rel_err(ds, gs)
    print(e)
    assert e <= TOL_GRAD, e


# ---------------------------------------------------------------------------------------------------------------- the C ABI directly
@gpu
@pytest.mark.parametrize("f", [4, 3], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("as_series", [0, 1], ids=["window-major", "series"])
def test_dilated_forward_is_the_plain_entry_on_each_phase(f, as_series, gpu_device):
    """dilation 3, no padding: the windows w = rho + v*3 are the plain entry's windows v on the sub-stack of the time rows rho, rho + 3, ... --
    the phase-major tiles make the same products in the same order, so anything but torch.equal is a mistake in the tile decode"""
    from tgcn_amd import _lib
    L = _lib.lib()
    n, S, T, H, N, K, d = 37, 2, 50, 5, 24, 3, 3
    nwin = nwin_of(T, H, d, 0, 0)
    assert nwin == 38
    gen = torch.Generator(device="cuda").manual_seed(f)
    stack = torch.randn((K, S, n, T, f), device="cuda", generator=gen)
    W = torch.randn((K, H * f, N), device="cuda", generator=gen)
    bias = torch.randn((N,), device="cuda", generator=gen)
    out = torch.full((S, n, nwin, N) if as_series else (S * nwin, n, N), float("nan"), device="cuda")
    _lib.check(L.tgcn_cheb_project_series_dilated_f32(_lib.stream_ptr(), S, n, T, f, H, N, K, _lib.ptr(stack), _lib.ptr(W), _lib.ptr(bias), 1, as_series,
                                                      _lib.ptr(out), 1, 0, 0, d))
    assert not torch.isnan(out).any()
    for rho in range(d):
        sub = stack[:, :, :, rho::d].contiguous()
        Tr = sub.shape[3]
        nw = Tr - H + 1
        assert nw == -(-(nwin - rho) // d)
        ref = torch.full((S, n, nw, N) if as_series else (S * nw, n, N), float("nan"), device="cuda")
        _lib.check(L.tgcn_cheb_project_series_f32(_lib.stream_ptr(), S, n, Tr, f, H, N, K, _lib.ptr(sub), _lib.ptr(W), _lib.ptr(bias), 1, as_series,
                                                  _lib.ptr(ref)))
        got = out[:, :, rho::d] if as_series else out.view(S, nwin, n, N)[:, rho::d].reshape(S * nw, n, N)
        assert torch.equal(got, ref), rho


@gpu
@pytest.mark.parametrize("geom", [(1, 0, 0), (2, 1, 2)], ids=["default", "stride2-pads"])
@pytest.mark.parametrize("as_series", [0, 1], ids=["window-major", "series"])
def test_dilated_entries_at_dilation_one_are_the_conv_entries(as_series, geom, gpu_device):
    """fp32 and bf16, forward, G and dW: bit-identical"""
    from tgcn_amd import _lib
    L = _lib.lib()
    n, S, T, f, H, N, K = 37, 2, 40, 8, 6, 32, 3
    stride, left, right = geom
    nwin = (T + left + right - H) // stride + 1
    gen = torch.Generator(device="cuda").manual_seed(n)
    head = (_lib.stream_ptr(), S, n, T, f, H, N, K)
    for dt in (torch.float32, torch.bfloat16):
        bf16 = dt == torch.bfloat16
        stack = torch.randn((K, S, n, T * f), device="cuda", generator=gen).to(dt)
        W = torch.randn((K, H * f, N), device="cuda", generator=gen).to(dt)
        bias = torch.randn((N,), device="cuda", generator=gen).to(dt)
        g = torch.randn((S, n, nwin, N) if as_series else (S * nwin, n, N), device="cuda", generator=gen).to(dt)
        outs = [torch.full_like(g, float("nan")) for _ in range(2)]
        if bf16:
            fwd = (_lib.ptr(stack), T * f, _lib.ptr(W), _lib.ptr(bias), _lib.DTYPE_BF16, 1, as_series)
            _lib.check(L.tgcn_cheb_project_series_conv_bf16(*head, *fwd, _lib.ptr(outs[0]), *geom))
            _lib.check(L.tgcn_cheb_project_series_dilated_bf16(*head, *fwd, _lib.ptr(outs[1]), *geom, 1))
            need = L.tgcn_cheb_series_conv_backward_bf16_workspace_bytes(*head[1:], *geom)
            assert need == L.tgcn_cheb_series_dilated_backward_bf16_workspace_bytes(*head[1:], *geom, 1) > 0
        else:
            fwd = (_lib.ptr(stack), _lib.ptr(W), _lib.ptr(bias), 1, as_series)
            _lib.check(L.tgcn_cheb_project_series_conv_f32(*head, *fwd, _lib.ptr(outs[0]), *geom))
            _lib.check(L.tgcn_cheb_project_series_dilated_f32(*head, *fwd, _lib.ptr(outs[1]), *geom, 1))
            need = L.tgcn_cheb_series_conv_backward_workspace_bytes(*head[1:], *geom)
            assert need == L.tgcn_cheb_series_dilated_backward_workspace_bytes(*head[1:], *geom, 1) > 0
        assert torch.equal(outs[0], outs[1]) and not torch.isnan(outs[0]).any()
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        Gs = [torch.full((K, S, n, T * f), float("nan"), device="cuda") for _ in range(2)]
        dWs = [torch.full((K, H * f, N), float("nan"), device="cuda") for _ in range(2)]
        if bf16:
            bwd = (_lib.ptr(stack), T * f, _lib.ptr(g), as_series, _lib.ptr(W))
            _lib.check(L.tgcn_cheb_series_conv_backward_bf16(*head, *bwd, _lib.ptr(Gs[0]), _lib.ptr(dWs[0]), _lib.ptr(ws), need, *geom))
            _lib.check(L.tgcn_cheb_series_dilated_backward_bf16(*head, *bwd, _lib.ptr(Gs[1]), _lib.ptr(dWs[1]), _lib.ptr(ws), need, *geom, 1))
        else:
            bwd = (_lib.ptr(stack), _lib.ptr(g), as_series, _lib.ptr(W))
            _lib.check(L.tgcn_cheb_series_conv_backward_f32(*head, *bwd, _lib.ptr(Gs[0]), _lib.ptr(dWs[0]), _lib.ptr(ws), need, *geom))
            _lib.check(L.tgcn_cheb_series_dilated_backward_f32(*head, *bwd, _lib.ptr(Gs[1]), _lib.ptr(dWs[1]), _lib.ptr(ws), need, *geom, 1))
        assert torch.equal(Gs[0], Gs[1]) and not torch.isnan(Gs[0]).any(), dt
        assert torch.equal(dWs[0], dWs[1]) and not torch.isnan(dWs[0]).any(), dt


@gpu
@pytest.mark.parametrize("dilation", [2, 2 ** 30, 2 ** 31 - 1])
def test_one_tap_at_any_dilation_is_the_undilated_layer(dilation, gpu_device):
    """H == 1: nothing to dilate and no span to bound the value -- the module's numbers at dilation 1, bit for bit, and the C entry the
    _conv entry's"""
    from tgcn_amd import _lib
    su = Setup("TGCNCheb_H", 4, 8, 1, seed=3)
    x = torch.randn(S_REC, N_VERT, 40, 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    res = []
    for kw in (dict(), dict(dilation=dilation)):
        su.layer.zero_grad()
        xs = x.clone().requires_grad_(True)
        out = su.layer.forward_series(xs, **kw)
        out.square().sum().backward()
        res.append((out.detach(), xs.grad, su.layer.weight.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*res))
    L = _lib.lib()
    n, S, T, f, H, N, K = 11, 1, 30, 4, 1, 8, 2
    gen = torch.Generator(device="cuda").manual_seed(2)
    stack, W = torch.randn(K, S, n, T * f, device="cuda", generator=gen), torch.randn(K, H * f, N, device="cuda", generator=gen)
    outs = [torch.full((S * T, n, N), float("nan"), device="cuda") for _ in range(2)]
    head = (_lib.stream_ptr(), S, n, T, f, H, N, K, _lib.ptr(stack), _lib.ptr(W), None, 0, 0)
    _lib.check(L.tgcn_cheb_project_series_conv_f32(*head, _lib.ptr(outs[0]), 1, 0, 0))
    _lib.check(L.tgcn_cheb_project_series_dilated_f32(*head, _lib.ptr(outs[1]), 1, 0, 0, dilation))
    assert torch.equal(outs[0], outs[1]) and not torch.isnan(outs[0]).any()


@gpu
def test_refused_combinations_launch_nothing(gpu_device):
    """what Python refuses, through the C ABI: an error code, the output untouched"""
    from tgcn_amd import _lib
    L = _lib.lib()
    n, S, T, f, H, N, K = 11, 1, 30, 4, 3, 8, 2
    stack, W = torch.zeros(K, S, n, T * f, device="cuda"), torch.zeros(K, H * f, N, device="cuda")
    out = torch.full((S * T, n, N), float("nan"), device="cuda")
    head = (_lib.stream_ptr(), S, n, T, f, H, N, K, _lib.ptr(stack), _lib.ptr(W), None, 0, 0, _lib.ptr(out))
    assert L.tgcn_cheb_project_series_dilated_f32(*head, 2, 0, 0, 2) == -4             # TGCN_ERR_UNSUPPORTED: a step with a dilation
    assert L.tgcn_cheb_project_series_dilated_f32(*head, 1, 0, 0, 0) == -1             # TGCN_ERR_INVALID
    assert L.tgcn_cheb_project_series_dilated_f32(*head, 1, 5, 0, 2) == -1             # a padding of He
    assert L.tgcn_cheb_project_series_dilated_f32(*head, 1, 0, 0, 15) == -1            # He = 31 > T
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
