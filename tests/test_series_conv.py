"""The streaming time-window layers as a convolution over time: forward_series / F.cheb_time_windows with a window step (`stride`) and zero
padding in time (`padding`), against the fp64 oracle run on the host-materialised windowed batch

    xw[s*nwin + w, i, h, c] = padded_series[s, i, w*stride + h, c],     nwin = (T + left + right - H) // stride + 1

(the `_windows` / `_fold` technique of tests/test_series_channels.py with the padded, strided rule; gradients from O.layer_backward folded back
onto the series, the padding rows dropped).  The project's bounds: outputs 1e-5, gradients 2e-5 of the tensor's maximum (conftest.rel_err)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cheb_oracle as O
from test_hip_parity import _random_graph
from test_series_channels import TOL, TOL_GRAD, _Setup, _dev, _to_series

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]

KB64 = 64 * 1024
OK, UNSUPPORTED = 0, -4       # TGCN_OK, TGCN_ERR_UNSUPPORTED

# (n, S, T, H, f, g, K, stride, left, right)
CASES = [(148, 2, 60, 15, 4, 32, 10, 2, 0, 0),     # aligned rows, HCP window, even step (the bank-rule case), nwin = 23
         (300, 3, 33, 7, 3, 8, 3, 3, 0, 0),        # unaligned f, (T - H) % stride = 2: the last two time rows are in no window
         (784, 1, 40, 12, 8, 15, 5, 1, 11, 0),     # "causal": nwin == T, g not a multiple of 16
         (90, 2, 24, 6, 5, 12, 25, 2, 2, 3),       # deep Chebyshev, both paddings with a step, nwin = 12
         (64, 2, 40, 5, 32, 70, 1, 7, 0, 0),       # step > H (no overlap), K = 1, g > 64
         (100, 1, 150, 9, 4, 16, 3, 2, 0, 0),      # nwin = 71: three wave tiles with a tail of 7, a workgroup with a wave that owns no tile
         (120, 2, 30, 6, 1, 8, 4, 2, 0, 0),        # single channel (run as a 3-D series, window-major first): the MFMA path
         (200, 1, 20, 20, 2, 5, 4, 1, 3, 3)]       # T == H with padding: 7 windows, 6 of them over an edge
NWIN = [23, 9, 40, 12, 6, 71, 13, 7]
CASE_IDS = ["n%d_S%d_T%d_H%d_f%d_g%d_K%d_s%d_l%d_r%d" % c for c in CASES]
DEGREE = {0, 3}               # the cases that also run on a degree-reordered operand


def nwin_of(T, H, stride, left, right):
    return (T + left + right - H) // stride + 1


def windows_conv(series, H, stride, left, right):
    """the windowed batch of the padded, strided rule, (S*nwin, n, H, f)"""
    S, n, T, f = series.shape
    pad = np.zeros((S, n, T + left + right, f), dtype=series.dtype)
    pad[:, :, left:left + T] = series
    nwin = nwin_of(T, H, stride, left, right)
    return np.stack([pad[:, :, w * stride:w * stride + H] for w in range(nwin)], axis=1).reshape(S * nwin, n, H, f)


def fold_conv(gxw, S, T, stride, left, right):
    """d series from the gradient of that batch: every window adds into the padded time rows it was cut from; the padding rows are dropped"""
    _, n, H, f = gxw.shape
    nwin = nwin_of(T, H, stride, left, right)
    gxw = gxw.reshape(S, nwin, n, H, f)
    gs = np.zeros((S, n, T + left + right, f))
    for w in range(nwin):
        gs[:, :, w * stride:w * stride + H] += gxw[:, w]
    return gs[:, :, left:left + T]


def padding_arg(H, left, right):
    """the spelling a caller would use"""
    if (left, right) == (H - 1, 0):
        return "causal"
    return left if left == right else (left, right)


class ConvSetup(_Setup):
    """test_series_channels._Setup with the geometry arguments on its streaming call"""

    def __init__(self, cls, kind, n, f, g, K, H, seed):
        super().__init__(cls, kind, n, f, g, K, H, seed)
        from tgcn_amd import functional as F
        layer = self.layer
        if cls == "TGCNCheb_H":
            self.conv = lambda s, as_series, **geo: layer.forward_series(s, as_series=as_series, **geo)
        else:
            row, col, _ = _random_graph(n, 6, np.random.default_rng(seed), hubs=((2, min(60, n - 1)),))      # _Setup's graph
            eid = _dev(np.stack([row, col]).astype(np.int64))
            if kind is None:
                self.conv = lambda s, as_series, **geo: layer.forward_series(s, eid, None, as_series=as_series, **geo)
            else:
                op = layer._operand(torch.empty(1, n, 1, device="cuda"), eid, None).reordered(kind)
                self.conv = lambda s, as_series, **geo: F.cheb_time_windows(op, s, layer.weight, layer.bias, F.BIAS_CHANNEL, F.MODE_CHEBYSHEV,
                                                                            as_series=as_series, **geo)


def _grads(su, series, go, as_series, geo, squeeze=False):
    """(out, d series, dW, db) of one streaming forward + backward; go in the layout of the output"""
    su.layer.zero_grad()
    st = _dev(series[..., 0] if squeeze else series).requires_grad_(True)
    out = su.conv(st, as_series, **geo)
    out.backward(_dev(go))
    ds = st.grad.cpu().numpy()
    return (out.detach(), ds[..., None] if squeeze else ds, su.layer.weight.grad.cpu().numpy().copy(), su.layer.bias.grad.cpu().numpy().copy())


def _reference(su, shape, rng):
    """series, gradient of the output (window-major) and the fp64 references (out, d series, dW, db)"""
    n, S, T, H, f, g, K, stride, left, right = shape
    nwin = nwin_of(T, H, stride, left, right)
    series = rng.standard_normal((S, n, T, f)).astype(np.float32)
    xw = windows_conv(series, H, stride, left, right).astype(np.float64)
    ref = su.ref_forward(xw)
    go = rng.standard_normal((S * nwin, n, g)).astype(np.float32)
    gxw, gW = O.layer_backward(su.L, xw, su.W64(), go, su.mode)
    return series, go, ref, fold_conv(gxw, S, T, stride, left, right), gW, su.bias_grad(go)


def _check(shape, cls, kind):
    """out / d series / dW / db in both output layouts against the oracle; returns d series of the window-major run"""
    n, S, T, H, f, g, K, stride, left, right = shape
    nwin = nwin_of(T, H, stride, left, right)
    geo = dict(stride=stride, padding=padding_arg(H, left, right))
    su = ConvSetup(cls, kind, n, f, g, K, H, seed=n + T)
    series, go, ref, gs, gW, gb = _reference(su, shape, np.random.default_rng([n, T, f]))
    squeeze = f == 1              # a single channel is given as a 3-D series

    out, ds, dW, db = _grads(su, series, go, False, geo, squeeze)
    errs = dict(out=rel_err(out.cpu().numpy(), ref), ds=rel_err(ds, gs), dW=rel_err(dW, gW), db=rel_err(db.reshape(gb.shape), gb))
    print(shape, cls, kind, "window-major", errs)
    assert tuple(out.shape) == (S * nwin, n, g)
    assert errs["out"] <= TOL, errs
    assert max(errs["ds"], errs["dW"], errs["db"]) <= TOL_GRAD, errs

    out_s, ds_s, dW_s, db_s = _grads(su, series, np.ascontiguousarray(_to_series(go, S, nwin)), True, geo, squeeze)
    assert tuple(out_s.shape) == (S, n, nwin, g) and out_s.is_contiguous()
    assert torch.equal(out_s, out.view(S, nwin, n, g).permute(0, 2, 1, 3))
    errs_s = dict(ds=rel_err(ds_s, gs), dW=rel_err(dW_s, gW), db=rel_err(db_s.reshape(gb.shape), gb))
    print(shape, cls, kind, "series layout", errs_s)
    assert max(errs_s.values()) <= TOL_GRAD, errs_s
    return ds, ds_s


def test_window_counts():
    assert [nwin_of(c[2], c[3], *c[7:]) for c in CASES] == NWIN


@gpu
@pytest.mark.parametrize("cls", ["TGCNCheb_H", "ChebTimeConv"])
@pytest.mark.parametrize("case", range(len(CASES)), ids=CASE_IDS)
def test_series_conv_vs_oracle(case, cls, gpu_device):
    shape = CASES[case]
    ds, ds_s = _check(shape, cls, None)
    if case == 1:             # time rows 31 and 32 lie behind the last window: exact zeros, not rounding noise
        assert not ds[:, :, 31:].any() and not ds_s[:, :, 31:].any()
        assert ds[:, :, 30].any()


# a recording shorter than the window, padded mostly behind: T + left < min(stride, H), so the phases (t + left) % stride >= T + left of the
# input gradient own no time row at all -- what the one window sends there falls into the right padding and must go nowhere
SHORT = [(50, 2, 2, 5, 4, 8, 3, 3, 0, 3), (41, 3, 1, 4, 3, 8, 2, 4, 1, 2), (33, 2, 3, 7, 8, 16, 2, 9, 0, 6)]


@gpu
@pytest.mark.parametrize("cls", ["TGCNCheb_H", "ChebTimeConv"])
@pytest.mark.parametrize("shape", SHORT, ids=["n%d_S%d_T%d_H%d_f%d_g%d_K%d_s%d_l%d_r%d" % c for c in SHORT])
def test_recording_shorter_than_the_window(shape, cls, gpu_device):
    n, S, T, H, f, g, K, stride, left, right = shape
    assert T + left < min(stride, H) and nwin_of(T, H, stride, left, right) == 1
    _check(shape, cls, None)


@gpu
@pytest.mark.parametrize("cls", ["TGCNCheb_H", "ChebTimeConv"])
@pytest.mark.parametrize("case", sorted(DEGREE), ids=[CASE_IDS[c] for c in sorted(DEGREE)])
def test_series_conv_on_a_reordered_operand(case, cls, gpu_device):
    _check(CASES[case], cls, "degree")


# ---------------------------------------------------------------------------------------------------------------- regimes with a step
def conv_plan(H, f, N, stride, vec=None):
    """(rc, hc, lds_bytes) of tgcn_series_conv_plan; vec defaults to what the Python path gives (its tensors are 16-byte aligned)"""
    from tgcn_amd import _lib
    hc, lds = C.c_int32(-1), C.c_int32(-1)
    rc = _lib.lib().tgcn_series_conv_plan(H, f, N, int(f % 4 == 0) if vec is None else int(vec), stride, C.byref(hc), C.byref(lds))
    return rc, hc.value, lds.value


def _regime(H, f, N, stride):
    rc, hc, lds = conv_plan(H, f, N, stride)
    if rc != OK:
        assert rc == UNSUPPORTED, rc
        return "unsupported"
    assert 1 <= hc <= H and 0 < lds, (hc, lds)
    return ("large" if lds > KB64 else "lds64") + ("-whole" if hc == H else "-chunked")


def _regimes(shape):
    """(forward, input gradient): the forward asks with its step, the input gradient -- one step-1 launch per phase over g as a series of
    g channels -- with the weight time rows of phase 0 (include/tgcn_hip.h, tgcn_series_conv_plan)"""
    n, S, T, H, f, g, K, stride, left, right = shape
    return _regime(H, f, g, stride), _regime(-(-H // stride), g, K * f, 1)


# the smallest shapes found with the host-only query that land in the regime ("large": above 64 KB; whole or chunked is the device's answer)
REGIMES = {
    "fwd-chunked-vec": ((19, 1, 50, 20, 48, 8, 2, 2, 0, 3), 0, "lds64-chunked"),           # HC = 18 of 20: overlapping windows, last chunk 2 rows
    "fwd-chunked-no-overlap": ((19, 2, 45, 13, 32, 8, 2, 5, 2, 0), 0, "lds64-chunked"),    # HC = 3 < step 5: only the rows read, last chunk 1 row
    "fwd-chunked-scalar": ((19, 1, 50, 20, 50, 8, 2, 2, 1, 0), 0, "lds64-chunked"),        # f % 4 != 0
    "fwd-large": ((23, 1, 36, 5, 128, 8, 1, 2, 0, 0), 0, "large"),
    "igrad-chunked": ((23, 1, 36, 9, 8, 112, 2, 2, 1, 0), 1, "lds64-chunked"),             # phase 0: 5 weight time rows, HC = 3
    "igrad-large": ((23, 1, 36, 9, 8, 128, 2, 2, 0, 1), 1, "large"),
}


@pytest.mark.parametrize("name", [k for k, v in REGIMES.items() if v[2] == "lds64-chunked"])
def test_plan_chunks_the_horizon_with_a_step(name):
    """the 64 KB limit is tried first, so these answers hold with and without a device"""
    shape, direction, want = REGIMES[name]
    assert _regimes(shape)[direction] == want
    n, S, T, H, f, g, K, stride, left, right = shape
    if direction == 0:        # the same shape at step 1 stages the whole horizon: it is the step that moves it
        assert _regime(H, f, g, 1) == "lds64-whole"


def test_plan_with_step_one_is_the_plan_without():
    from test_series_channels_regimes import series_plan
    for H in (1, 3, 5, 28, 40):
        for f in (1, 3, 8, 64, 66):
            for N in (8, 17, 64):
                assert conv_plan(H, f, N, 1) == series_plan(H, f, N)
    from tgcn_amd import _lib
    hc, lds = C.c_int32(0), C.c_int32(0)
    assert _lib.lib().tgcn_series_conv_plan(4, 8, 8, 1, 0, C.byref(hc), C.byref(lds)) == -1        # TGCN_ERR_INVALID


@gpu
@pytest.mark.parametrize("cls", ["TGCNCheb_H", "ChebTimeConv"])
@pytest.mark.parametrize("name", list(REGIMES))
def test_regimes_with_a_step_vs_oracle(name, cls, gpu_device):
    shape, direction, want = REGIMES[name]
    got = _regimes(shape)[direction]
    assert got.startswith(want), "%s %s: the launcher plans %s, this case is here for %s" % (name, shape, got, want)
    _check(shape, cls, None)


@gpu
def test_refusal_at_the_device_limit(gpu_device):
    """so many channels that one staged chunk of one weight time row fits no LDS: the plan query says so, and the call raises before its hops"""
    from tgcn_amd import _lib
    n, S, T, H, g, K, stride = 23, 1, 36, 3, 8, 2, 2
    f = next((c for c in range(4, 4096, 4) if conv_plan(H, c, g, stride)[0] == UNSUPPORTED), None)
    assert f is not None and conv_plan(H, f - 4, g, stride)[0] == OK, f
    print("first refused f:", f)
    su = ConvSetup("TGCNCheb_H", None, n, f, g, K, H, seed=n)
    st = torch.zeros(S, n, T, f, device="cuda")
    with pytest.raises(_lib.TgcnError):
        su.conv(st, False, stride=stride, padding=1)
    assert b"LDS" in _lib.lib().tgcn_last_error()
    out = torch.full((S * 18, n, g), float("nan"), device="cuda")
    stack, W = torch.zeros(K, S, n, T * f, device="cuda"), torch.zeros(K, H * f, g, device="cuda")
    rc = _lib.lib().tgcn_cheb_project_series_conv_f32(_lib.stream_ptr(), S, n, T, f, H, g, K, _lib.ptr(stack), _lib.ptr(W), None, 0, 0,
                                                      _lib.ptr(out), stride, 1, 1)
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED and torch.isnan(out).all()          # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- the C ABI directly
@gpu
@pytest.mark.parametrize("dims", [(37, 2, 40, 4, 6, 32, 3), (29, 3, 33, 3, 7, 10, 2)], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("as_series", [0, 1], ids=["window-major", "series"])
def test_conv_entries_at_step_one_without_padding_are_the_plain_entries(dims, as_series, gpu_device):
    """stride = 1, pad = 0 through the new entries: bit-identical output, G and dW"""
    from tgcn_amd import _lib
    L = _lib.lib()
    n, S, T, f, H, N, K = dims
    nwin = T - H + 1
    gen = torch.Generator(device="cuda").manual_seed(n)
    stack = torch.randn((K, S, n, T * f), device="cuda", generator=gen)
    W = torch.randn((K, H * f, N), device="cuda", generator=gen)
    bias = torch.randn((N,), device="cuda", generator=gen)
    g = torch.randn((S, n, nwin, N) if as_series else (S * nwin, n, N), device="cuda", generator=gen)
    head = (_lib.stream_ptr(), S, n, T, f, H, N, K)
    outs = [torch.full_like(g, float("nan")) for _ in range(2)]
    _lib.check(L.tgcn_cheb_project_series_f32(*head, _lib.ptr(stack), _lib.ptr(W), _lib.ptr(bias), 1, as_series, _lib.ptr(outs[0])))
    _lib.check(L.tgcn_cheb_project_series_conv_f32(*head, _lib.ptr(stack), _lib.ptr(W), _lib.ptr(bias), 1, as_series, _lib.ptr(outs[1]), 1, 0, 0))
    assert torch.equal(outs[0], outs[1]) and not torch.isnan(outs[0]).any()
    need = L.tgcn_cheb_series_backward_workspace_bytes(S, n, T, f, H, N, K)
    assert need == L.tgcn_cheb_series_conv_backward_workspace_bytes(S, n, T, f, H, N, K, 1, 0, 0) > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    Gs = [torch.full((K, S, n, T * f), float("nan"), device="cuda") for _ in range(2)]
    dWs = [torch.full((K, H * f, N), float("nan"), device="cuda") for _ in range(2)]
    _lib.check(L.tgcn_cheb_series_backward_f32(*head, _lib.ptr(stack), _lib.ptr(g), as_series, _lib.ptr(W), _lib.ptr(Gs[0]), _lib.ptr(dWs[0]),
                                               _lib.ptr(ws), need))
    _lib.check(L.tgcn_cheb_series_conv_backward_f32(*head, _lib.ptr(stack), _lib.ptr(g), as_series, _lib.ptr(W), _lib.ptr(Gs[1]), _lib.ptr(dWs[1]),
                                                    _lib.ptr(ws), need, 1, 0, 0))
    assert torch.equal(Gs[0], Gs[1]) and not torch.isnan(Gs[0]).any()
    assert torch.equal(dWs[0], dWs[1]) and not torch.isnan(dWs[0]).any()


# ---------------------------------------------------------------------------------------------------------------- one-sided backwards
ONE_SIDED = (90, 2, 24, 6, 5, 12, 3, 2, 2, 3)


@pytest.fixture(scope="module")
def one_sided():
    """the layer, inputs and fp64 references of one strided, padded shape, computed once for the tests below (which leave them unchanged)"""
    n, S, T, H, f, g, K, stride, left, right = ONE_SIDED
    su = ConvSetup("TGCNCheb_H", None, n, f, g, K, H, seed=n + T)
    return (su, dict(stride=stride, padding=(left, right))) + _reference(su, ONE_SIDED, np.random.default_rng([n, T, f, 1]))


@gpu
def test_backward_without_the_series_gradient(gpu_device, one_sided):
    su, geo, series, go, ref, gs, gW, gb = one_sided
    su.layer.zero_grad()
    st = _dev(series)
    out = su.conv(st, False, **geo)
    out.backward(_dev(go))
    assert st.grad is None
    errs = dict(out=rel_err(out.detach().cpu().numpy(), ref), dW=rel_err(su.layer.weight.grad.cpu().numpy(), gW),
                db=rel_err(su.layer.bias.grad.cpu().numpy().reshape(gb.shape), gb))
    print(errs)
    assert errs["out"] <= TOL and max(errs["dW"], errs["db"]) <= TOL_GRAD, errs


@gpu
def test_backward_with_frozen_parameters(gpu_device, one_sided):
    su, geo, series, go, ref, gs, gW, gb = one_sided
    n, S, T, H = ONE_SIDED[:4]
    su.layer.zero_grad()
    su.layer.requires_grad_(False)
    try:
        st = _dev(series).requires_grad_(True)
        out = su.conv(st, True, **geo)
        out.backward(_dev(np.ascontiguousarray(_to_series(go, S, nwin_of(T, H, *ONE_SIDED[7:])))))
    finally:
        su.layer.requires_grad_(True)
    assert su.layer.weight.grad is None and su.layer.bias.grad is None
    e = rel_err(st.grad.cpu().numpy(), gs)
    print(e)
    assert e <= TOL_GRAD, e


@gpu
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
def test_no_bias(as_series, gpu_device, one_sided):
    from tgcn_amd import functional as F
    su, geo, series, go, ref, gs, gW, gb = one_sided
    n, S, T, H, f, g, K, stride, left, right = ONE_SIDED
    nwin = nwin_of(T, H, stride, left, right)
    ref0 = O.tgcn_cheb_h_forward(su.L, windows_conv(series, H, stride, left, right).astype(np.float64), su.W64(), None)
    su.layer.zero_grad()
    st = _dev(series).requires_grad_(True)
    out = F.cheb_time_windows(su.layer._operand(st.device), st, su.layer.weight, None, F.BIAS_NONE, F.MODE_POWER, as_series=as_series, **geo)
    out.backward(_dev(np.ascontiguousarray(_to_series(go, S, nwin)) if as_series else go))
    got = out.detach().cpu().numpy()
    errs = dict(out=rel_err(got, _to_series(ref0, S, nwin) if as_series else ref0), ds=rel_err(st.grad.cpu().numpy(), gs),
                dW=rel_err(su.layer.weight.grad.cpu().numpy(), gW))
    print(errs)
    assert su.layer.bias.grad is None
    assert errs["out"] <= TOL and max(errs["ds"], errs["dW"]) <= TOL_GRAD, errs


# ---------------------------------------------------------------------------------------------------------------- chain and capture
def _chain_layers(n, rng):
    import tgcn_amd
    row, col, val = _random_graph(n, 6, rng, hubs=((2, 60),))
    val = val * 0.4
    op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val))
    torch.manual_seed(7)
    return O.coo_to_csr(row, col, val, n), tgcn_amd.TGCNCheb_H(op, 1, 8, 4, 5).cuda(), tgcn_amd.TGCNCheb_H(op, 8, 16, 3, 4).cuda()


@gpu
def test_causal_chain_vs_oracle(gpu_device):
    """l2.forward_series(relu(l1.forward_series(x, as_series=True, padding="causal")), as_series=True, padding="causal", stride=2): the hidden
    series keeps the input's time axis; output and the gradient to x against the oracle composed the same way"""
    n, S, T, H1, H2 = 148, 2, 30, 5, 4
    rng = np.random.default_rng(78)
    L, l1, l2 = _chain_layers(n, rng)
    nwin2 = nwin_of(T, H2, 2, H2 - 1, 0)
    series = rng.standard_normal((S, n, T)).astype(np.float32)
    W1, b1 = l1.weight.detach().cpu().numpy().astype(np.float64), l1.bias.detach().cpu().numpy().astype(np.float64)
    W2, b2 = l2.weight.detach().cpu().numpy().astype(np.float64), l2.bias.detach().cpu().numpy().astype(np.float64)
    L64 = L.astype(np.float64)
    xw1 = windows_conv(series[..., None].astype(np.float64), H1, 1, H1 - 1, 0)                # (S*T, n, H1, 1)
    hid = _to_series(np.maximum(O.tgcn_cheb_h_forward(L64, xw1, W1, b1).astype(np.float64), 0), S, T)      # (S, n, T, 8)
    xw2 = windows_conv(hid, H2, 2, H2 - 1, 0)
    ref = _to_series(O.tgcn_cheb_h_forward(L64, xw2, W2, b2), S, nwin2)                     # (S, n, nwin2, 16)
    go = rng.standard_normal(ref.shape).astype(np.float32)
    gxw2, _ = O.layer_backward(L, xw2, W2, np.ascontiguousarray(go.transpose(0, 2, 1, 3)).reshape(S * nwin2, n, 16), "power")
    ghid = fold_conv(gxw2, S, T, 2, H2 - 1, 0) * (hid > 0)
    gxw1, _ = O.layer_backward(L, xw1, W1, np.ascontiguousarray(ghid.transpose(0, 2, 1, 3)).reshape(S * T, n, 8), "power")
    gs = fold_conv(gxw1, S, T, 1, H1 - 1, 0)[..., 0]

    st = _dev(series).requires_grad_(True)
    h = torch.relu(l1.forward_series(st, as_series=True, padding="causal"))
    assert tuple(h.shape) == (S, n, T, 8)
    out = l2.forward_series(h, as_series=True, padding="causal", stride=2)
    assert tuple(out.shape) == (S, n, nwin2, 16) and out.is_contiguous()
    out.backward(_dev(go))
    errs = dict(out=rel_err(out.detach().cpu().numpy(), ref), ds=rel_err(st.grad.cpu().numpy(), gs))
    print(errs)
    assert errs["out"] <= TOL and errs["ds"] <= TOL_GRAD, errs


@gpu
def test_strided_padded_step_is_graph_capturable(gpu_device):
    """forward + backward at stride 3 (three phase launches from a host loop) with both paddings inside torch.cuda.graph, replayed once:
    the eager numbers.  Nothing in the call synchronises or allocates outside torch."""
    n, S, T = 148, 2, 30
    L, l1, l2 = _chain_layers(n, np.random.default_rng(79))
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((S, n, T, 8), device="cuda", generator=gen).requires_grad_(True)
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
    assert all(torch.equal(a, b) for a, b in zip(got, eager))
