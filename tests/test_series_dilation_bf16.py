"""The streaming time-window layers with dilated taps and bfloat16 parameters (ChebSeriesBf16Fn through the `_dilated_bf16` entries), by the
method of tests/test_series_bf16.py with its two bounds:

  * the GPU agrees with a numpy emulation that rounds at the rounding points of DESIGN.md 3.10 "bf16" within EMUL_ULPS = 8 bf16 ulps of the
    tensor's largest value;
  * against the fp64 oracle on the materialised dilated windows (tests/test_series_dilation.py's rule) of the bf16-rounded series, weight and
    upstream gradient the bound is TWICE the emulation's own error against fp64, per case and tensor, computed here on the CPU;
  * the two output layouts of one call are torch.equal.

Shapes: the unequal-phase, several-tiles and negative-window-start rows of tests/test_series_dilation.py with f in {8, 16} (the 16-byte form)
and f = 3 (the narrow form); both classes, with a bias and without, on a plain and on a degree-reordered operand."""
import copy
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import tgcn_amd
from tgcn_amd import functional as F
from conftest import rel_err
from oracle import cheb_oracle as O
from test_bf16_layers import EMUL_ULPS, _apply, _bias_add, _fold, bf, fp64_reference
from test_series_bf16 import _graph, _to_series
from test_series_dilation import CLASSES, K_TERMS, N_VERT, S_REC, fold_dilated, nwin_of, padding_arg, windows_dilated

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]
BF = torch.bfloat16
ULP_BOUND = EMUL_ULPS * 2.0 ** -8

# (T, H, d, f, g, left, right)
WIDTHS = (8, 16, 3)
UNEQUAL = [(50, 5, d, f, g, 0, 0) for d in (3, 7) for f in WIDTHS for g in (5, 40)]
TILES = [(150, 3, 2, f, 8, 0, 0) for f in WIDTHS]
NEGATIVE = [(50, 5, d, f, g, left, right) for d in (3, 7) for f in WIDTHS for g in (5, 40) for left, right in (((5 - 1) * d, 0), (2, 5))]


def _id(s):
    return "T%d_H%d_d%d_f%d_g%d_l%d_r%d" % s


@functools.lru_cache(maxsize=None)
def make_case(cls, shape):
    """the bf16 layer (on the CPU), its edge list, L of the oracle, the mode, the fp32 series and upstream gradient (window-major)"""
    T, H, d, f, g, left, right = shape
    seed = sum(shape) + len(cls)
    L = _graph(N_VERT, seed)
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    if cls == "TGCNCheb_H":
        m = tgcn_amd.TGCNCheb_H(torch.as_tensor(L.toarray()), f, g, K_TERMS, H)
        ei, L_op, mode = None, L, "power"
    else:
        r, c = L.nonzero()
        ei = torch.as_tensor(np.stack([r, c]).astype(np.int64))
        m = tgcn_amd.ChebTimeConv(f, g, K_TERMS, H)
        row, col, lap = O.edge_laplacian(ei.numpy(), None, N_VERT)
        L_op, mode = O.coo_to_csr(row, col, lap, N_VERT), "chebyshev"
    with torch.no_grad():
        m.bias.uniform_(-0.5, 0.5)
    series = rng.standard_normal((S_REC, N_VERT, T, f)).astype(np.float32)
    go = rng.standard_normal((S_REC * nwin_of(T, H, d, left, right), N_VERT, g)).astype(np.float32)
    return m.to(BF), ei, L_op, mode, series, go


def _win(x3, dims, geom):
    S, n, T, f, H = dims
    return windows_dilated(x3.reshape(S, n, T, f), H, *geom).reshape(-1, n, H * f)


def _unwin(gxw, dims, geom):
    S, n, T, f, H = dims
    return fold_dilated(gxw.reshape(-1, n, H, f), S, T, *geom)


def series_fp64(L, xs, W, b, g, mode, geom):
    """the oracle on the materialised dilated windows, d series folded back onto the series; geom = (dilation, left, right)"""
    S, n, T, f = xs.shape
    K, H, _, N = W.shape
    dims = (S, n, T, f, H)
    y, gxw, gW, gb = fp64_reference(L, _win(xs.reshape(S, n, T * f), dims, geom), W.reshape(K, H * f, N), b, g, mode)
    return y, _unwin(gxw, dims, geom), gW.reshape(W.shape), gb


def series_emulate(L, xs, W, b, g, mode, geom):
    """ChebSeriesBf16Fn in fp64 with its rounding points (tests/test_series_bf16.py's emulation on the dilated window rule); inputs already
    bf16 values"""
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
def references(cls, shape, bias):
    """(fp64 reference, emulation) of a case with or without its bias, computed once and left unchanged"""
    m, ei, L, mode, series, go = make_case(cls, shape)
    T, H, d, f, g, left, right = shape
    W = m.weight.detach().double().numpy()
    b = m.bias.detach().double().numpy() if bias else None
    xs, gg = bf(series), bf(go)
    geom = (d, left, right)
    return series_fp64(L, xs, W, b, gg, mode, geom), series_emulate(L, xs, W, b, gg, mode, geom)


def test_emulation_is_close_to_fp64_on_a_dilated_case():
    """the two references agree to bf16 precision (a few rounding points of 2^-9 each), so the bounds below are bf16-sized, not loose"""
    ref, emu = references("TGCNCheb_H", UNEQUAL[0], True)
    for e, r in zip(emu, ref):
        assert 0 < rel_err(e, r) < 2.0 ** -6


class Runner:
    def __init__(self, cls, shape, dev):
        T, H, d, f, g, left, right = shape
        m, ei, L, mode, series, go = make_case(cls, shape)
        self.m = m = copy.deepcopy(m).to(dev)
        self.geo = dict(padding=padding_arg(H, d, left, right), dilation=d)
        self.nwin, self.series, self.go = nwin_of(T, H, d, left, right), series, go
        if cls == "TGCNCheb_H":
            self.op = m._operand(dev)
            self.module = lambda s, a: m.forward_series(s, as_series=a, **self.geo)
            self.fargs = lambda bias: (m.weight, m.bias.reshape(-1) if bias else None, F.BIAS_VERTEX_CHANNEL if bias else F.BIAS_NONE, F.MODE_POWER)
        else:
            eid = ei.to(dev)
            self.op = m._operand(torch.empty(1, N_VERT, 1, device=dev), eid, None)
            self.module = lambda s, a: m.forward_series(s, eid, None, as_series=a, **self.geo)
            self.fargs = lambda bias: (m.weight, m.bias if bias else None, F.BIAS_CHANNEL if bias else F.BIAS_NONE, F.MODE_CHEBYSHEV)
        self.ops = {None: self.op}

    def run(self, kind, bias, as_series, series_grad=True):
        """(out, d series, dW, db) as tensors; out and the upstream gradient in the layout asked for"""
        self.m.zero_grad()
        s = torch.as_tensor(self.series, device=self.m.weight.device).to(BF).requires_grad_(series_grad)
        if kind is None and bias:
            out = self.module(s, as_series)
        else:
            if kind not in self.ops:
                self.ops[kind] = self.op.reordered(kind)
            out = F.cheb_time_windows(self.ops[kind], s, *self.fargs(bias), as_series=as_series, **self.geo)
        go = _to_series(self.go, S_REC, self.nwin) if as_series else self.go
        out.backward(torch.as_tensor(go, device=out.device).to(BF))
        return out.detach(), s.grad, self.m.weight.grad, self.m.bias.grad


def _compare(cls, shape, bias, got, label_prefix=""):
    """got: (out window-major, d series, dW, db) -> both bounds per tensor"""
    ref, emu = references(cls, shape, bias)
    for i, label in enumerate(("out", "ds", "dW", "db")):
        if got[i] is None:
            continue
        gv = got[i].detach().double().cpu().numpy().reshape(ref[i].shape)
        tol = 2 * rel_err(emu[i], ref[i])                  # twice the emulation's own error against fp64
        d_emu, e64 = float(np.abs(gv - emu[i]).max() / np.abs(emu[i]).max()), rel_err(gv, ref[i])
        print(cls, shape, label_prefix, label, "vs emulation %.2e (bound %.2e)" % (d_emu, ULP_BOUND), "vs fp64 %.2e (bound %.2e)" % (e64, tol))
        assert d_emu <= ULP_BOUND, (label_prefix, label, d_emu)
        assert e64 <= tol, (label_prefix, label, e64, tol)


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", UNEQUAL + TILES + NEGATIVE, ids=_id)
def test_dilated_bf16_series_vs_oracle_and_emulation(shape, cls, gpu_device):
    T, H, d, f, g, left, right = shape
    S, n = S_REC, N_VERT
    r = Runner(cls, shape, gpu_device)
    nwin = r.nwin
    for kind in (None, "degree"):
        for bias in (True, False):
            out_s, ds_s, dW_s, db_s = r.run(kind, bias, True)
            assert out_s.dtype == BF and tuple(out_s.shape) == (S, n, nwin, g) and out_s.is_contiguous()
            assert ds_s.dtype == BF and dW_s.dtype == BF and (db_s is None) == (not bias)
            wm = out_s.permute(0, 2, 1, 3).reshape(S * nwin, n, g)
            _compare(cls, shape, bias, (wm, ds_s, dW_s.clone(), None if db_s is None else db_s.clone()), "%s series" % kind)
            out, ds, dW, db = r.run(kind, bias, False)
            assert out.dtype == BF and tuple(out.shape) == (S * nwin, n, g)
            assert torch.equal(out_s, out.view(S, nwin, n, g).permute(0, 2, 1, 3))
            _compare(cls, shape, bias, (out, ds, dW, db), "%s window-major" % kind)


ONE_SIDED = (50, 5, 3, 8, 40, 2, 5)


@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_one_sided_backwards(cls, gpu_device):
    r = Runner(cls, ONE_SIDED, gpu_device)
    out, ds, dW, db = r.run(None, True, False, series_grad=False)
    assert ds is None
    _compare(cls, ONE_SIDED, True, (out, None, dW, db), "no series gradient")
    r.m.requires_grad_(False)
    out, ds, dW, db = r.run(None, True, True)
    assert dW is None and db is None
    _compare(cls, ONE_SIDED, True, (None, ds, None, None), "frozen parameters")
