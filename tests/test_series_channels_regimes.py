"""The launch regimes of series_gemm_kernel / series_wgrad_partial_kernel (csrc/windows.h) that tests/test_series_channels.py never reaches:
the horizon staged in chunks (HC < H), dynamic LDS above 64 KB (alone and with chunks), workgroups whose last waves have no tile, one-sided
backwards, bias=None, an unaligned source through the C ABI, the refusal of a time row that fits no LDS, and the 256 MB cap of the weight
gradient's partials.  Same machinery and reference as test_series_channels.py (fp64 oracle on the host-materialised windows, here fed fp64
inputs), same bounds: outputs 1e-5, gradients 2e-5 under conftest.rel_err.

Every case first ASSERTS the regime it is there for, through the library's own answer (tgcn_series_gemm_plan: the NT choice and
series_gemm_lds() the launcher uses) -- nothing here restates the LDS formula, so a change of the launcher that moves a shape back into the
whole-horizon-under-64-KB branch fails the case at its precondition instead of passing it for the wrong reason.  The forward is queried as
(H, f, g), the input gradient -- the same kernel over g as a series of g channels -- as (H, g, K*f)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cheb_oracle as O
from test_hip_parity import _random_graph
from test_series_channels import CASES, TOL, TOL_GRAD, _Setup, _dev, _fold, _grads, _to_series, _windows

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]

KB64 = 64 * 1024
OK, UNSUPPORTED = 0, -4       # TGCN_OK, TGCN_ERR_UNSUPPORTED

# (n, S, T, H, f, g, K) and the regime of (forward, input gradient): LDS class "lds64" / "large" (above 64 KB, the opt-in limit) and
# "whole" (HC == H) / "chunked" (HC < H).  Computed for a 160 KB opt-in limit; what the library answers is what is asserted.
SHAPES = {
    "A": ((37, 1, 40, 28, 2, 64, 2), ("lds64-whole", "lds64-whole")),        # input gradient 64 352 B: just under 64 KB; 1 and 2 live waves in the tail
    "B": ((23, 1, 36, 5, 8, 112, 2), ("lds64-whole", "lds64-chunked")),      # HC = 3 of 5, vector loads, nwin == 32
    "C": ((19, 3, 45, 40, 66, 10, 2), ("lds64-chunked", "lds64-whole")),     # HC = 29 of 40, scalar loads, ragged last k step of a chunk
    "D": ((21, 1, 60, 28, 8, 64, 5), ("lds64-whole", "lds64-chunked")),      # HC = 21 of 28, NT = 4, nwin == 33
    "E": ((23, 1, 36, 5, 128, 8, 1), ("large-whole", "lds64-whole")),        # forward 76 928 B
    "F1": ((23, 1, 36, 5, 8, 128, 2), ("lds64-whole", "large-whole")),       # input gradient 76 928 B ...
    "F2": ((23, 1, 36, 5, 8, 160, 2), ("lds64-whole", "large-whole")),       # ... then 95 360 B on the same kernel instantiation
    "G": ((23, 1, 36, 3, 8, 300, 1), ("lds64-whole", "large-chunked")),      # HC = 2 of 3 above 64 KB
    "H": ((22, 1, 70, 6, 3, 100, 2), ("lds64-whole", "lds64-whole")),        # nwin == 65: three window tiles, the last with one window
}


def series_plan(H, f, N, vec=None):
    """(rc, hc, lds_bytes) of tgcn_series_gemm_plan; vec defaults to what the Python path gives (its tensors are 16-byte aligned)"""
    from tgcn_amd import _lib
    hc, lds = C.c_int32(-1), C.c_int32(-1)
    rc = _lib.lib().tgcn_series_gemm_plan(H, f, N, int(f % 4 == 0) if vec is None else int(vec), C.byref(hc), C.byref(lds))
    return rc, hc.value, lds.value


def _regime(H, f, N, vec=None):
    rc, hc, lds = series_plan(H, f, N, vec)
    if rc != OK:
        assert rc == UNSUPPORTED, rc
        return "unsupported"
    assert 1 <= hc <= H and 0 < lds, (hc, lds)
    return ("large" if lds > KB64 else "lds64") + ("-whole" if hc == H else "-chunked")


def _regimes(shape):
    """(forward, input gradient)"""
    n, S, T, H, f, g, K = shape
    return _regime(H, f, g), _regime(H, g, K * f)


def _tail_tiles(shape):
    """wave tiles of (forward, input gradient) modulo the 4 waves of a workgroup"""
    n, S, T, H, f, g, K = shape
    return (S * n * ((T - H + 1 + 31) // 32)) % 4, (S * n * ((T + 31) // 32)) % 4


# ---------------------------------------------------------------------------------------------------------------- the plan query, no GPU
def test_plan_of_the_existing_cases_is_the_whole_horizon():
    """what this file exists for: all six CASES of test_series_channels.py stage the whole horizon under 64 KB, in both directions"""
    for n, S, T, H, f, g, K in CASES:
        for Hq, fq, Nq in ((H, f, g), (H, g, K * f)):
            rc, hc, lds = series_plan(Hq, fq, Nq)
            assert (rc, hc) == (OK, H) and 0 < lds <= KB64, ((Hq, fq, Nq), rc, hc, lds)


@pytest.mark.parametrize("name,direction", [("B", 1), ("C", 0), ("D", 1)])
def test_plan_chunks_the_horizon(name, direction):
    """B, C, D take chunks that fit 64 KB whatever the device's opt-in limit is (the 64 KB limit is tried first)"""
    n, S, T, H, f, g, K = SHAPES[name][0]
    assert SHAPES[name][1][direction] == "lds64-chunked"
    Hq, fq, Nq = ((H, f, g), (H, g, K * f))[direction]
    rc, hc, lds = series_plan(Hq, fq, Nq)
    assert rc == OK and 1 <= hc < H and 0 < lds <= KB64, (rc, hc, lds)


def test_plan_bounds_and_refusal():
    """1 <= hc <= H and lds within the limit for a sweep of shapes of which one time row fits 64 KB: that limit is tried first, so it is the
    one in force for them on any device.  What needs more (shape E's forward, G's input gradient) is refused without a device, where the
    opt-in limit falls back to 64 KB, and granted above 64 KB with one."""
    from tgcn_amd import _lib
    for H in (1, 3, 5, 28, 40):
        for f in (1, 2, 3, 8, 64, 66, 100):
            for N in (1, 16, 17, 32, 33, 64, 300):
                for vec in ((0, 1) if f % 4 == 0 else (0,)):
                    rc, hc, lds = series_plan(H, f, N, vec)
                    assert rc == OK and 1 <= hc <= H and 0 < lds <= KB64, ((H, f, N, vec), rc, hc, lds)
    for H, f, N in ((5, 128, 8), (3, 300, 8)):
        rc, hc, lds = series_plan(H, f, N)
        assert rc == UNSUPPORTED or (rc == OK and 1 <= hc <= H and lds > KB64), (rc, hc, lds)
        if not torch.cuda.is_available():
            assert rc == UNSUPPORTED and b"LDS" in _lib.lib().tgcn_last_error()
    hc, lds = C.c_int32(0), C.c_int32(0)
    assert _lib.lib().tgcn_series_gemm_plan(0, 8, 8, 1, C.byref(hc), C.byref(lds)) == -1       # TGCN_ERR_INVALID
    assert _lib.lib().tgcn_series_gemm_plan(4, 8, 8, 1, None, C.byref(lds)) == -1


# ---------------------------------------------------------------------------------------------------------------- the regimes on the GPU
def _reference(su, shape, rng):
    """series, gradient of the output and the fp64 references (out, d series, dW, db)"""
    n, S, T, H, f, g, K = shape
    nwin = T - H + 1
    series = rng.standard_normal((S, n, T, f)).astype(np.float32)
    xw = _windows(series, H).astype(np.float64)
    ref = su.ref_forward(xw)
    go = rng.standard_normal((S * nwin, n, g)).astype(np.float32)
    gxw, gW = O.layer_backward(su.L, xw, su.W64(), go, su.mode)
    return series, go, ref, _fold(gxw, S, T), gW, su.bias_grad(go)


def _check(name, cls, kind, shape=None):
    """one row of SHAPES: the preconditions, then out / d series / dW / db in both output layouts against the oracle"""
    shape, want = (SHAPES[name][0], SHAPES[name][1]) if shape is None else (shape, SHAPES[name][1])
    n, S, T, H, f, g, K = shape
    nwin = T - H + 1
    got = _regimes(shape)
    assert got == want, "%s %s: the launcher plans %s, this case is here for %s" % (name, shape, got, want)
    assert all(_tail_tiles(shape)), "%s: a direction fills its last workgroup: %s" % (name, _tail_tiles(shape))
    su = _Setup(cls, kind, n, f, g, K, H, seed=n + T)
    series, go, ref, gs, gW, gb = _reference(su, shape, np.random.default_rng([n, T, f]))

    out, ds, dW, db = _grads(su, series, go, False)
    errs = dict(out=rel_err(out.cpu().numpy(), ref), ds=rel_err(ds, gs), dW=rel_err(dW, gW), db=rel_err(db.reshape(gb.shape), gb))
    print(name, cls, kind, "window-major", errs)
    assert tuple(out.shape) == (S * nwin, n, g)
    assert errs["out"] <= TOL, errs
    assert max(errs["ds"], errs["dW"], errs["db"]) <= TOL_GRAD, errs

    out_s, ds_s, dW_s, db_s = _grads(su, series, np.ascontiguousarray(_to_series(go, S, nwin)), True)
    assert tuple(out_s.shape) == (S, n, nwin, g) and out_s.is_contiguous()
    assert torch.equal(out_s, out.view(S, nwin, n, g).permute(0, 2, 1, 3))
    errs_s = dict(ds=rel_err(ds_s, gs), dW=rel_err(dW_s, gW), db=rel_err(db_s.reshape(gb.shape), gb))
    print(name, cls, kind, "series layout", errs_s)
    assert max(errs_s.values()) <= TOL_GRAD, errs_s


def _same_regime_g(name):
    """the row's shape, with the nearest g (a multiple of 4) whose plan is the row's regime when the device's opt-in limit is not the
    160 KB the table was computed for"""
    (n, S, T, H, f, g, K), want = SHAPES[name]
    for d in sorted(range(-160, 164, 4), key=abs):
        if g + d >= 4 and _regimes((n, S, T, H, f, g + d, K)) == want:
            return (n, S, T, H, f, g + d, K)
    pytest.fail("%s: no g near %d reaches %s on this device" % (name, g, want))


@gpu
@pytest.mark.parametrize("cls", ["TGCNCheb_H", "ChebTimeConv"])
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_chunked_and_tail_regimes_vs_oracle(name, cls, gpu_device):
    _check(name, cls, None)


@gpu
def test_chunked_input_gradient_on_a_reordered_operand(gpu_device):
    _check("D", "TGCNCheb_H", "degree")


@gpu
@pytest.mark.parametrize("kind", [None, "degree"], ids=["plain", "degree"])
def test_large_lds_sizes_ascend_on_one_instantiation(kind, gpu_device):
    """F: the input gradient above 64 KB twice on series_gemm_kernel<1, true>, the second launch larger than the first: the kernel's
    dynamic-LDS attribute has to follow the larger request"""
    f1, f2 = _same_regime_g("F1"), _same_regime_g("F2")
    l1, l2 = series_plan(f1[3], f1[5], f1[6] * f1[4])[2], series_plan(f2[3], f2[5], f2[6] * f2[4])[2]
    assert KB64 < l1 < l2, (l1, l2)
    _check("F1", "ChebTimeConv", kind, f1)
    _check("F2", "ChebTimeConv", kind, f2)


@gpu
def test_large_lds_forward(gpu_device):
    _check("E", "TGCNCheb_H", None)


@gpu
def test_large_lds_chunked_input_gradient(gpu_device):
    _check("G", "ChebTimeConv", None, _same_regime_g("G"))


@gpu
def test_three_window_tiles_scalar_loads(gpu_device):
    _check("H", "TGCNCheb_H", None)


# ---------------------------------------------------------------------------------------------------------------- one-sided backwards
@pytest.fixture(scope="module")
def shape_d():
    """shape D's layer, inputs and fp64 references, computed once for the tests below (which leave them unchanged)"""
    shape = SHAPES["D"][0]
    n, S, T, H, f, g, K = shape
    su = _Setup("TGCNCheb_H", None, n, f, g, K, H, seed=n + T)
    return (su, shape) + _reference(su, shape, np.random.default_rng([n, T, f, 1]))


@gpu
def test_backward_without_the_series_gradient(gpu_device, shape_d):
    """the first layer of a network: G == NULL, the weight gradient alone"""
    su, shape, series, go, ref, gs, gW, gb = shape_d
    assert _regimes(shape) == SHAPES["D"][1]
    su.layer.zero_grad()
    st = _dev(series)
    out = su.stream(st)
    out.backward(_dev(go))
    assert st.grad is None
    errs = dict(out=rel_err(out.detach().cpu().numpy(), ref), dW=rel_err(su.layer.weight.grad.cpu().numpy(), gW),
                db=rel_err(su.layer.bias.grad.cpu().numpy().reshape(gb.shape), gb))
    print(errs)
    assert errs["out"] <= TOL and max(errs["dW"], errs["db"]) <= TOL_GRAD, errs


@gpu
def test_backward_with_frozen_parameters(gpu_device, shape_d):
    """dW == NULL: the input gradient alone"""
    su, shape, series, go, ref, gs, gW, gb = shape_d
    su.layer.zero_grad()
    su.layer.requires_grad_(False)
    try:
        st = _dev(series).requires_grad_(True)
        out = su.stream(st, True)
        out.backward(_dev(np.ascontiguousarray(_to_series(go, shape[1], shape[2] - shape[3] + 1))))
    finally:
        su.layer.requires_grad_(True)
    assert su.layer.weight.grad is None and su.layer.bias.grad is None
    e = rel_err(st.grad.cpu().numpy(), gs)
    print(e)
    assert e <= TOL_GRAD, e


@gpu
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
def test_no_bias(as_series, gpu_device, shape_d):
    """bias=None / BIAS_NONE through the functional entry: the oracle without a bias (the gradients do not depend on it)"""
    from tgcn_amd import functional as F
    su, shape, series, go, ref, gs, gW, gb = shape_d
    n, S, T, H, f, g, K = shape
    nwin = T - H + 1
    ref0 = O.tgcn_cheb_h_forward(su.L, _windows(series, H).astype(np.float64), su.W64(), None)
    su.layer.zero_grad()
    st = _dev(series).requires_grad_(True)
    out = F.cheb_time_windows(su.layer._operand(st.device), st, su.layer.weight, None, F.BIAS_NONE, F.MODE_POWER, as_series=as_series)
    out.backward(_dev(np.ascontiguousarray(_to_series(go, S, nwin)) if as_series else go))
    got = out.detach().cpu().numpy()
    errs = dict(out=rel_err(got, _to_series(ref0, S, nwin) if as_series else ref0), ds=rel_err(st.grad.cpu().numpy(), gs),
                dW=rel_err(su.layer.weight.grad.cpu().numpy(), gW))
    print(errs)
    assert su.layer.bias.grad is None
    assert errs["out"] <= TOL and max(errs["ds"], errs["dW"]) <= TOL_GRAD, errs


# ---------------------------------------------------------------------------------------------------------------- the C ABI directly
@gpu
def test_unaligned_stack_through_the_c_abi(gpu_device):
    """tgcn_cheb_project_series_f32 on a hop stack that starts 4 bytes into a 16-byte-aligned allocation: f = 8 would take 16-byte loads,
    the launcher has to fall back to scalar loads (Python never does this, it aligns its inputs)"""
    from tgcn_amd import _lib
    n, S, T, H, f, N, K = 21, 1, 40, 6, 8, 16, 2
    nwin = T - H + 1
    assert _regime(H, f, N, vec=0) == "lds64-whole" and _regime(H, f, N, vec=1) == "lds64-whole"
    rng = np.random.default_rng(5)
    row, col, val = _random_graph(n, 6, rng, hubs=((2, n - 1),))
    L = O.coo_to_csr(row, col, val * 0.4, n)
    series = rng.standard_normal((S, n, T, f))
    W = rng.standard_normal((K, H, f, N)).astype(np.float32)
    # K = 2: the reference's power stack is (x, L x), no fold of the weight
    stack = O.stack_reference_power(L.astype(np.float64), series.reshape(S, n, T * f), K).astype(np.float32)
    ref = O.tgcn_cheb_h_forward(L, _windows(series, H), W, None)
    buf = torch.empty(stack.size + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    aligned, shifted = buf[:stack.size], buf[1:stack.size + 1]
    assert shifted.data_ptr() % 16 == 4
    Wd = _dev(W)
    outs = []
    for view in (aligned, shifted):
        view.copy_(_dev(stack).reshape(-1))
        out = torch.full((S * nwin, n, N), float("nan"), device="cuda")
        _lib.check(_lib.lib().tgcn_cheb_project_series_f32(_lib.stream_ptr(), S, n, T, f, H, N, K, _lib.ptr(view), _lib.ptr(Wd), None, 0, 0,
                                                           _lib.ptr(out)))
        outs.append(out.cpu().numpy())
    errs = dict(aligned=rel_err(outs[0], ref), shifted=rel_err(outs[1], ref), shifted_vs_aligned=rel_err(outs[1], outs[0]))
    print(errs)
    assert errs["shifted_vs_aligned"] <= 1e-6 and max(errs["aligned"], errs["shifted"]) <= TOL, errs


# ---------------------------------------------------------------------------------------------------------------- the channel limit
@gpu
def test_input_gradient_refuses_too_many_output_channels(gpu_device):
    """Today's behaviour, pinned: with g output channels so many that one time row of g (the input gradient's series) fits no LDS span, the
    forward runs, a backward that needs d series raises TgcnError (TGCN_ERR_UNSUPPORTED, on the host), one that does not backpropagates"""
    from tgcn_amd import _lib
    n, S, T, H, f, K = 23, 1, 36, 3, 8, 1
    g = next((c for c in range(4, 4096, 4) if series_plan(H, c, K * f)[0] == UNSUPPORTED), None)
    assert g is not None and series_plan(H, g - 4, K * f)[0] == OK and series_plan(H, f, g)[0] == OK, g
    print("first refused g:", g)
    shape = (n, S, T, H, f, g, K)
    su = _Setup("TGCNCheb_H", None, n, f, g, K, H, seed=n + T)
    series, go, ref, gs, gW, gb = _reference(su, shape, np.random.default_rng([n, T, g]))
    st = _dev(series).requires_grad_(True)
    out = su.stream(st)
    assert rel_err(out.detach().cpu().numpy(), ref) <= TOL
    with pytest.raises(_lib.TgcnError):
        out.backward(_dev(go))
    su.layer.zero_grad()
    out = su.stream(_dev(series))
    out.backward(_dev(go))
    errs = dict(dW=rel_err(su.layer.weight.grad.cpu().numpy(), gW), db=rel_err(su.layer.bias.grad.cpu().numpy().reshape(gb.shape), gb))
    print(errs)
    assert max(errs.values()) <= TOL_GRAD, errs


# ---------------------------------------------------------------------------------------------------------------- the partials cap
@gpu
def test_weight_gradient_partials_capped_at_256_mb(gpu_device):
    """A 2 MB weight (K, H, f, g) = (4, 16, 32, 256) on 8256 window rows: the rule of at most 1024 row blocks of at least 64 rows would keep
    129 partials, 258 MB; the cap takes larger row blocks.  Asserted through the workspace the library asks for.  References per input
    channel (O.windows_backward: the layer is a sum over its input channels), no windows materialised."""
    import tgcn_amd
    from tgcn_amd import _lib
    n, S, T, H, f, N, K = 64, 1, 144, 16, 32, 256, 4
    M, wbytes = S * n * (T - H + 1), K * H * f * N * 4
    partials = _lib.lib().tgcn_cheb_series_backward_workspace_bytes(S, n, T, f, H, N, K) - wbytes      # wbytes is a multiple of 256
    assert partials % wbytes == 0 and partials <= 256 << 20 < -(-M // 64) * wbytes, (partials, M, wbytes)
    rng = np.random.default_rng(11)
    row, col, val = _random_graph(n, 6, rng, hubs=((2, 40),))
    val = val * 0.4
    L = O.coo_to_csr(row, col, val, n)
    op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val))
    torch.manual_seed(3)
    layer = tgcn_amd.TGCNCheb_H(op, f, N, K, H).cuda()
    series = rng.standard_normal((S, n, T, f)).astype(np.float32)
    go = rng.standard_normal((S * (T - H + 1), n, N)).astype(np.float32)
    st = _dev(series).requires_grad_(True)
    layer.forward_series(st).backward(_dev(go))
    W = layer.weight.detach().cpu().numpy()
    rs, rW = np.zeros((S, n, T, f)), np.zeros((K, H, f, N))
    for c in range(f):
        rs[..., c], rW[:, :, c] = O.windows_backward(L, series[..., c], W[:, :, c], go, "power")
    dW = layer.weight.grad.cpu().numpy()
    errs = dict(ds=rel_err(st.grad.cpu().numpy(), rs), dW=rel_err(dW, rW), dWk=max(rel_err(dW[k], rW[k]) for k in range(K)),
                db=rel_err(layer.bias.grad.cpu().numpy(), go.astype(np.float64).sum(axis=0, keepdims=True)))
    print(errs)
    assert max(errs.values()) <= TOL_GRAD, errs
