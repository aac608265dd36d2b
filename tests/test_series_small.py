"""The one-launch whole-series layer (forward_series / F.cheb_time_windows with fused=True; csrc/series_small.h) on the GPU, against the fp64
oracle on the materialised windows and against the unfused call of the same commit.  Bounds and helpers are those of
tests/test_series_channels.py / tests/test_series_dilation.py: TOL = 1e-5 for an output, TOL_GRAD = 2e-5 of the tensor's maximum for a
gradient.  Shapes are the smallest that cross each line of the kernel: a 37-vertex operand staged densely and a 50-vertex one staged as
CSR (partial vertex tiles in both), 1 / 3 / 4 channels, 5 and 40 output columns (one partial column tile; two column groups), K = 1 / 2 / 5
in both recurrences, 1 and 3 taps, dilation 1 and 2, no / causal / one-sided padding, S = 2 recordings of T = 70 time rows.  Every accuracy
case first asks the plan for TB and asserts nwin >= 3*TB and nwin % TB != 0: a first, an interior and a ragged last tile."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cheb_oracle as O
from test_hip_parity import _random_graph
from test_series_channels import TOL, TOL_GRAD, _dev, _to_series
from test_series_dilation import fold_dilated, nwin_of, padding_arg, windows_dilated

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]

S_REC, T_ROWS = 2, 70
GRAPHS = {37: 60, 50: 6}        # vertices -> average degree: nearly complete (the dense copy is the smaller form) and sparse (the CSR is)


class Setup:
    """One class on one of the two graphs: the layer, its operand and the fp64 references"""

    def __init__(self, cls, n, f, g, K, H, seed):
        import tgcn_amd
        from tgcn_amd import functional as F
        rng = np.random.default_rng(seed)
        row, col, val = _random_graph(n, GRAPHS[n], rng)
        val = val * 0.4
        torch.manual_seed(seed)
        self.cls, self.F, self.n, self.K = cls, F, n, K
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

    def W64(self):
        return self.layer.weight.detach().cpu().numpy()

    def call(self, s, bias, **kw):
        """the module with its bias, the functional entry without one"""
        if bias:
            return self.module(s, **kw)
        W = self.layer.weight if s.dim() == 4 else self.layer.weight.reshape(self.K, self.layer.weight.shape[1], -1)
        return self.F.cheb_time_windows(self.op, s, W, None, self.F.BIAS_NONE, self.fmode, **kw)

    def plan(self, f, H, N, T, left, right, d):
        rc, tb, dense, lds = self.F._series_small_plan(self.op, f, H, N, self.K, T, left, right, d, self.fmode)
        assert rc == 0 and lds <= 160 * 1024
        return tb, dense


def _run(su, series, go, bias, as_series, geo, fused):
    """(out, d series, dW, db) of one forward + backward; go in the layout of the output"""
    su.layer.zero_grad()
    squeeze = series.shape[3] == 1           # a single channel is given as a 3-D series
    st = _dev(series[..., 0] if squeeze else series).requires_grad_(True)
    out = su.call(st, bias, as_series=as_series, fused=fused, **geo)
    out.backward(_dev(go))
    ds = st.grad.cpu().numpy().reshape(series.shape)
    dW = su.layer.weight.grad.cpu().numpy().copy()
    db = None if su.layer.bias.grad is None else su.layer.bias.grad.cpu().numpy().copy()
    return out.detach(), ds, dW, db


# (n, f, g, K, H, d, left, right): every listed value of every axis, each next to a different neighbour
CASES = [(37, 1, 5, 5, 3, 1, 0, 0), (37, 3, 40, 2, 3, 2, 4, 0), (37, 4, 40, 5, 3, 1, 1, 2), (37, 1, 40, 1, 1, 2, 0, 0),
         (50, 1, 40, 5, 3, 2, 1, 2), (50, 3, 5, 1, 3, 1, 2, 0), (50, 4, 5, 2, 1, 1, 0, 0), (50, 4, 40, 5, 3, 2, 0, 0)]
CLASSES = ["TGCNCheb_H", "ChebTimeConv"]


def _id(c):
    return "n%d_f%d_g%d_K%d_H%d_d%d_l%d_r%d" % c


def test_the_cases_cover_every_listed_value():
    cols = list(zip(*CASES))
    assert set(cols[0]) == {37, 50} and set(cols[1]) == {1, 3, 4} and set(cols[2]) == {5, 40} and set(cols[3]) == {1, 2, 5}
    assert set(cols[4]) == {1, 3} and set(cols[5]) == {1, 2}
    pads = {padding_arg(c[4], c[5], c[6], c[7]) if c[4] > 1 else 0 for c in CASES}
    assert {0, "causal", (1, 2)} <= pads


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_fused_series_vs_oracle_and_vs_the_unfused_call(case, cls, gpu_device):
    n, f, g, K, H, d, left, right = case
    S, T = S_REC, T_ROWS
    nwin = nwin_of(T, H, d, left, right)
    geo = dict(padding=padding_arg(H, d, left, right) if H > 1 else 0, dilation=d)
    su = Setup(cls, n, f, g, K, H, seed=n + 7 * d + f + K)
    tb, dense = su.plan(f, H, g, T, left, right, 1 if H == 1 else d)
    assert dense == (1 if n == 37 else 0)
    assert nwin >= 3 * tb and nwin % tb != 0, (nwin, tb)        # a first, an interior and a ragged last tile
    rng = np.random.default_rng([n, f, g, K, H, d])
    series = rng.standard_normal((S, n, T, f)).astype(np.float32)
    xw = windows_dilated(series, H, d, left, right).astype(np.float64)
    go = rng.standard_normal((S * nwin, n, g)).astype(np.float32)
    go_s = np.ascontiguousarray(_to_series(go, S, nwin))
    gxw, gW = O.layer_backward(su.L, xw, su.W64(), go, su.mode)
    gs, gb = fold_dilated(gxw, S, T, d, left, right), su.bias_grad(go)
    for bias in (True, False):
        ref = su.forward64(xw, su.layer.bias.detach().cpu().numpy() if bias else None)
        for as_series in (False, True):
            out, ds, dW, db = _run(su, series, go_s if as_series else go, bias, as_series, geo, True)
            plain = _run(su, series, go_s if as_series else go, bias, as_series, geo, False)[0]
            assert tuple(out.shape) == ((S, n, nwin, g) if as_series else (S * nwin, n, g)) and out.is_contiguous()
            wm = out.permute(0, 2, 1, 3).reshape(S * nwin, n, g) if as_series else out
            errs = dict(out=rel_err(wm.cpu().numpy(), ref), unfused=rel_err(out.cpu().numpy(), plain.cpu().numpy()),
                        ds=rel_err(ds, gs), dW=rel_err(dW, gW))
            if bias:
                errs.update(db=rel_err(db.reshape(gb.shape), gb))
            else:
                assert db is None
            print(cls, case, "bias" if bias else "no bias", "series" if as_series else "windows", "TB", tb, errs)
            assert errs.pop("out") <= TOL and errs.pop("unfused") <= TOL, (bias, as_series)
            assert max(errs.values()) <= TOL_GRAD, (bias, as_series, errs)


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("n,f,g", [(37, 3, 40), (50, 1, 5)])
def test_a_shifted_series_gives_the_same_bits_across_tile_seams(n, f, g, d, cls, gpu_device):
    """padding=0: window w of series[:, :, 5:] is window w + 5 of the series; the tiles fall elsewhere, and no sum's order depends on them"""
    su = Setup(cls, n, f, g, 5, 3, seed=n + d)
    tb, _ = su.plan(f, 3, g, T_ROWS, 0, 0, d)
    assert 5 % tb != 0          # the shift moves every seam
    x = torch.randn(S_REC, n, T_ROWS, f, device="cuda")
    if f == 1:
        x = x[..., 0]
    with torch.no_grad():
        whole = su.module(x, as_series=True, dilation=d, fused=True)
        shifted = su.module(x[:, :, 5:].contiguous(), as_series=True, dilation=d, fused=True)
    assert shifted.shape[2] == whole.shape[2] - 5
    assert torch.equal(shifted, whole[:, :, 5:])


@gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["power", "chebyshev"])
@pytest.mark.parametrize("n,f,N,H,d,left,right", [(37, 3, 40, 3, 2, 1, 2), (50, 1, 5, 3, 1, 0, 0), (50, 4, 40, 1, 1, 0, 0)])
def test_the_c_entry_directly_and_the_stack_it_writes(n, f, N, H, d, left, right, mode, gpu_device):
    from tgcn_amd import _lib
    from tgcn_amd import functional as F
    L = _lib.lib()
    su = Setup("TGCNCheb_H", n, f, N, 5, H, seed=3 * n + f)
    op, K, S, T = su.op, 5, S_REC, T_ROWS
    nwin = nwin_of(T, H, d, left, right)
    rc, tb, _, _ = F._series_small_plan(op, f, H, N, K, T, left, right, d, mode)
    assert rc == 0 and nwin >= 3 * tb and nwin % tb != 0
    torch.manual_seed(n + f)
    x3, W = torch.randn(S, n, T * f, device="cuda"), torch.randn(K, H * f, N, device="cuda") * 0.3
    bias = torch.randn(N, device="cuda")
    # the reference: the hop stack and the _dilated entry
    ref_stack = F._series_stack(op, x3, K, mode)
    ref = torch.empty(S, n, nwin, N, device="cuda")
    _lib.check(L.tgcn_cheb_project_series_dilated_f32(_lib.stream_ptr(), S, n, T, f, H, N, K, _lib.ptr(ref_stack), _lib.ptr(W), _lib.ptr(bias), 1, 1,
                                                      _lib.ptr(ref), 1, left, right, d))

    def entry(stack):
        out = torch.full((S, n, nwin, N), float("nan"), device="cuda")
        _lib.check(L.tgcn_cheb_series_small_f32(_lib.stream_ptr(), C.byref(op.struct), mode, S, T, f, H, N, K, _lib.ptr(x3), _lib.ptr(W),
                                                _lib.ptr(bias), 1, 1, _lib.ptr(out), _lib.ptr(stack), left, right, d))
        torch.cuda.synchronize()
        return out
    out0 = entry(None)
    stack = torch.full((K, S, n, T * f), float("nan"), device="cuda")      # every element is written: none stays NaN
    out1 = entry(stack)
    assert torch.isfinite(out0).all() and torch.isfinite(stack).all()
    assert torch.equal(out0, out1)
    assert rel_err(out0.cpu().numpy(), ref.cpu().numpy()) <= TOL
    assert torch.equal(stack[0], x3)
    for k in range(K):
        assert rel_err(stack[k].cpu().numpy(), ref_stack[k].cpu().numpy()) <= TOL, k
    stack2 = torch.full_like(stack, float("nan"))
    assert torch.equal(entry(stack2), out1) and torch.equal(stack2, stack)


@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_a_training_call_keeps_the_stack_of_the_fused_launch(cls, gpu_device):
    su = Setup(cls, 50, 3, 5, 5, 3, seed=11)
    x = torch.randn(S_REC, 50, T_ROWS, 3, device="cuda")
    out = su.module(x, padding="causal", fused=True)
    assert "ChebSeriesSmallFn" in type(out.grad_fn).__name__          # the fused Function, whose forward hopped nothing on the host side
    stack = out.grad_fn.stack
    assert tuple(stack.shape) == (5, S_REC, 50, T_ROWS * 3)
    ref = su.F._series_stack(su.op, x.view(S_REC, 50, T_ROWS * 3), 5, su.fmode)
    assert rel_err(stack.cpu().numpy(), ref.cpu().numpy()) <= TOL
    with torch.no_grad():
        assert torch.equal(su.module(x, padding="causal", fused=True), out)
    su.layer.weight.requires_grad_(False)
    assert su.module(x.requires_grad_(True), padding="causal", fused=True).grad_fn.stack is None


@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_auto_is_one_of_the_two_calls_bit_for_bit(cls, gpu_device):
    """fused="auto" is the fused call where F.SERIES_FUSED_AUTO lists the class of the call's unfused form, the unfused call elsewhere"""
    su = Setup(cls, 37, 1, 5, 5, 3, seed=13)
    x = torch.randn(S_REC, 37, T_ROWS, device="cuda")
    with torch.no_grad():
        for kw, klass in ((dict(), "windows_f1"), (dict(as_series=True), "series"), (dict(padding="causal"), "series")):
            fused = klass in su.F.SERIES_FUSED_AUTO
            assert torch.equal(su.module(x, fused="auto", **kw), su.module(x, fused=fused, **kw)), kw


@gpu
def test_two_fused_layers_chain_like_the_unfused_ones(gpu_device):
    import tgcn_amd
    su = Setup("TGCNCheb_H", 50, 3, 8, 5, 3, seed=5)
    torch.manual_seed(6)
    l1, l2 = su.layer, tgcn_amd.TGCNCheb_H(su.op, 8, 40, 2, 3).cuda()
    x0 = torch.randn(S_REC, 50, T_ROWS, 3, device="cuda")
    go = torch.randn(S_REC, 50, T_ROWS, 40, device="cuda")
    got = {}
    for fused in (False, True):
        for l in (l1, l2):
            l.zero_grad()
        x = x0.clone().requires_grad_(True)
        h = torch.relu(l1.forward_series(x, as_series=True, padding="causal", fused=fused))
        out = l2.forward_series(h, as_series=True, padding="causal", dilation=2, fused=fused)
        out.backward(go)
        got[fused] = [out.detach()] + [t.grad.clone() for t in (x, l1.weight, l1.bias, l2.weight, l2.bias)]
    names = ["out", "d series", "dW1", "db1", "dW2", "db2"]
    for nm, a, b in zip(names, got[True], got[False]):
        err = rel_err(a.cpu().numpy(), b.cpu().numpy())
        print(nm, err)
        assert err <= (TOL if nm == "out" else TOL_GRAD), nm


@gpu
def test_refused_calls_launch_nothing(gpu_device):
    """through the C ABI: an error code, the output and the stack untouched; through the modules: TgcnError and the same"""
    import tgcn_amd
    from tgcn_amd import _lib
    L = _lib.lib()
    su = Setup("TGCNCheb_H", 50, 4, 5, 2, 3, seed=2)
    op, S, T, f, H, N, K = su.op, 1, 12, 4, 3, 5, 2
    x3, W = torch.ones(S, 50, T * f, device="cuda"), torch.zeros(K, H * f, N, device="cuda")
    out, stack = torch.full((S, 50, T - 2, N), float("nan"), device="cuda"), torch.full((K, S, 50, T * f), float("nan"), device="cuda")

    def call(T=T, H=H, left=0, right=0, d=1, mode=0, bias_kind=0, series=x3):
        return L.tgcn_cheb_series_small_f32(_lib.stream_ptr(), C.byref(op.struct), mode, S, T, f, H, N, K, _lib.ptr(series), _lib.ptr(W), None,
                                            bias_kind, 1, _lib.ptr(out), _lib.ptr(stack), left, right, d)
    assert call(T=2) == -1 and call(left=3) == -1 and call(right=-1) == -1 and call(d=0) == -1 and call(mode=2) == -1 and call(H=0) == -1
    assert call(bias_kind=1) == -1 and call(series=None) == -1
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(stack).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not out.any() and torch.isfinite(stack).all() and (stack[0] == 1).all()          # W = 0
    x = torch.randn(2, 50, 12, 4, device="cuda")
    with torch.no_grad():
        for kw in (dict(stride=2), dict(padding="causal", time_chunk=4), dict(fused="yes")):
            with pytest.raises(_lib.TgcnError):
                su.layer.forward_series(x, **dict(dict(fused=True), **kw))
        with pytest.raises(_lib.TgcnError, match="reordered"):
            su.F.cheb_time_windows(op.reordered("degree"), x, su.layer.weight, None, su.F.BIAS_NONE, su.fmode, fused=True)
        big = tgcn_amd.TGCNCheb_H(op, 64, 5, 2, 700).cuda()          # a 700-tap window of 64 channels: no span fits next to the operand
        assert not su.F.series_fused_supported(op, 64, 700, 5, 2, 800, 0, 1, su.fmode)
        with pytest.raises(_lib.TgcnError, match="do not fit"):
            big.forward_series(torch.randn(1, 50, 800, 64, device="cuda"), fused=True)
