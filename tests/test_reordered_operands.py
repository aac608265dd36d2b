"""GraphOperand.reordered(kind) against the fp64 oracle on the caller's ORIGINAL operand, in both recurrences, on every layer path.

A reordered operand works in its own vertex labels; the layer functions relabel x and a per-vertex bias on the way in and the result on
the way out, so that a caller never sees the permutation.  Data that is already in the operand's labels must not be relabelled a second
time on the way through (cheb_stack's _operand_labels): every case here compares with the oracle evaluated on the unpermuted L, whose
values are random per entry, so that L and L^T differ and neither a wrong transpose nor a wrong relabelling can cancel out.  The plain
operand runs in the same parametrisation as the control."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cheb_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]
TOL = 1e-5           # outputs and stacks
GTOL = 2e-5          # gradients
KINDS = [None, "rcm", "hub_first"]
MODES = [0, 1]       # functional.MODE_POWER, functional.MODE_CHEBYSHEV
MODE_NAME = {0: "power", 1: "chebyshev"}


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _sym_graph(n, avg, rng):
    m = n * avg // 2
    u, v = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = u != v
    u, v = u[keep], v[keep]
    row, col = np.concatenate([u, v]), np.concatenate([v, u])
    key = np.unique(row.astype(np.int64) * n + col)
    return key // n, key % n


@functools.lru_cache(maxsize=None)
def _graph(n, isolated=0.0):
    """(row, col, val) of an n-vertex graph with a symmetric pattern and random, non-symmetric values; a share `isolated` of the
    vertices, scattered over the labels, has no entry at all (the compact plans' left-out vertices)"""
    rng = np.random.default_rng(n)
    n_core = n - int(n * isolated)
    row, col = _sym_graph(n_core, 8, rng)
    if n_core < n:
        lab = rng.permutation(n)[:n_core]
        row, col = lab[row], lab[col]
    val = (rng.standard_normal(row.shape[0]) / 4).astype(np.float32)
    return row, col, val


@functools.lru_cache(maxsize=None)
def _operand(n, isolated, kind):
    """(operand, L in fp64): the operand in the caller's labels (kind None) or reordered; L is always the caller's"""
    import tgcn_amd
    row, col, val = _graph(n, isolated)
    op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val))
    if kind is not None:
        op = op.reordered(kind)
        assert op.perm is not None and not bool((op.perm == torch.arange(n, device=op.perm.device)).all())
    return op, O.coo_to_csr(row, col, val, n).astype(np.float64)


def _stack(L, x, K, mode):
    return (O.stack_reference_power if mode == 0 else O.stack_chebyshev)(L, np.asarray(x, np.float64), K)


def _forward64(L, x, W, b, mode):
    """sum_k T_k(L) x W_k + b in fp64; x (q, n, C), W (K, C, N), b (N,) or (n, N)"""
    out = np.einsum("kqnc,kcg->qng", _stack(L, x, W.shape[0], mode), W.astype(np.float64), optimize=True)
    return out + b.astype(np.float64)


def _bias_grad64(g, b):
    g = np.asarray(g, np.float64)
    return g.sum(axis=(0, 1)) if b.ndim == 1 else g.sum(axis=0)


def _leaves(*arrays):
    return [_dev(a).requires_grad_(True) for a in arrays]


def _check_grads(leaves, want):
    for name, t, w in zip(("dx", "dW", "db"), leaves, want):
        e = rel_err(t.grad.cpu().numpy(), w)
        assert e <= GTOL, (name, e)


# ------------------------------------------------------------------------------------------------ cheb_layer on every layer path
# id: (n, isolated share, q, C, N, K, path kind, row layout, keep-basis bytes (None: the default))
LAYER_CASES = {
    "small": (300, 0.0, 2, 8, 8, 4, "small", 0, None),
    "project_first": (3000, 0.0, 2, 64, 16, 3, "project_first", 0, None),
    "hops_layout0": (3000, 0.0, 2, 32, 24, 4, "hops", 0, None),
    "hops_layout1": (3000, 0.0, 3, 8, 12, 4, "hops", 1, None),
    "hops_layout0_over_keep": (3000, 0.0, 2, 32, 24, 4, "hops", 0, 0),
    "hops_layout1_over_keep": (3000, 0.0, 3, 8, 12, 4, "hops", 1, 0),
    "compact": (70000, 0.2, 1, 8, 8, 3, "compact", 0, None),
    "compact_over_keep": (70000, 0.2, 1, 8, 8, 3, "compact", 0, 0),
}


@pytest.mark.parametrize("bias_kind", [1, 2], ids=["bias_channel", "bias_vertex"])
@pytest.mark.parametrize("kind", KINDS, ids=["plain", "rcm", "hub_first"])
@pytest.mark.parametrize("mode", MODES, ids=["power", "chebyshev"])
@pytest.mark.parametrize("case", list(LAYER_CASES))
def test_layer_on_reordered_operand_vs_oracle(case, mode, kind, bias_kind, gpu_device, monkeypatch):
    """cheb_layer: training output, dx / dW / db for a random output gradient, and the inference output under no_grad, against the
    fp64 oracle on the caller's L -- on the layer path each case names (asserted, so that a threshold change cannot move a case off it)"""
    from tgcn_amd import functional as F
    n, isolated, q, C, N, K, path_kind, layout, keep = LAYER_CASES[case]
    if keep is not None:
        monkeypatch.setattr(F, "KEEP_BASIS_BYTES", keep)
    op, L = _operand(n, isolated, kind)
    path = F._layer_path(op, q, n, C, N, K, mode)
    assert path.kind == path_kind and (path_kind != "hops" or path.layout == layout), path
    rng = np.random.default_rng([list(LAYER_CASES).index(case), mode, bias_kind])
    x = rng.standard_normal((q, n, C)).astype(np.float32)
    W = (rng.standard_normal((K, C, N)) / np.sqrt(K * C)).astype(np.float32)
    b = rng.standard_normal((N,) if bias_kind == F.BIAS_CHANNEL else (n, N)).astype(np.float32)
    want = _forward64(L, x, W, b, mode)
    leaves = _leaves(x, W, b)
    out = F.cheb_layer(op, *leaves, bias_kind, mode)
    e = rel_err(out.detach().cpu().numpy(), want)
    assert e <= TOL, ("out", e)
    g = rng.standard_normal(want.shape).astype(np.float32)
    out.backward(_dev(g))
    gx, gW = O.layer_backward(L, x, W, g, MODE_NAME[mode])
    _check_grads(leaves, (gx, gW, _bias_grad64(g, b)))
    with torch.no_grad():
        out = F.cheb_layer(op, _dev(x), _dev(W), _dev(b), bias_kind, mode)
    e = rel_err(out.cpu().numpy(), want)
    assert e <= TOL, ("inference out", e)


def test_learnable_values_on_reordered_operand_are_refused(gpu_device):
    """learnable operand values are packed in the operand's CSR order, which a reordered operand does not share with the caller"""
    from tgcn_amd import _lib, functional as F
    op, _ = _operand(300, 0.0, "rcm")
    x, W, b = torch.randn(2, 300, 8, device="cuda"), torch.randn(3, 8, 8, device="cuda"), torch.randn(8, device="cuda")
    values = torch.randn(op.nnz, device="cuda", requires_grad=True)
    with pytest.raises(_lib.TgcnError):
        F.cheb_layer(op, x, W, b, F.BIAS_CHANNEL, F.MODE_CHEBYSHEV, values=values)


# ------------------------------------------------------------------------------------------------ cheb_relu_pool
def _relu_pool64(y, pool, gz):
    """z = max over `pool` consecutive vertices of relu(y) and the gradient it sends back to y"""
    q, n, N = y.shape
    r = np.maximum(y, 0).reshape(q, n // pool, pool, N)
    arg = r.argmax(axis=2)
    z = np.take_along_axis(r, arg[:, :, None], axis=2)[:, :, 0]
    gy = np.zeros_like(r)
    np.put_along_axis(gy, arg[:, :, None], np.where(z > 0, gz, 0)[:, :, None], axis=2)
    return z, gy.reshape(q, n, N)


@pytest.mark.parametrize("pool", [2, 4])
@pytest.mark.parametrize("kind", KINDS, ids=["plain", "rcm", "hub_first"])
@pytest.mark.parametrize("mode", MODES, ids=["power", "chebyshev"])
@pytest.mark.parametrize("case", ["small", "hops_layout0"])
def test_relu_pool_on_reordered_operand_vs_oracle(case, mode, kind, pool, gpu_device):
    """cheb_relu_pool: pooling groups consecutive vertices of the CALLER's labels (the reordered path relabels the layer output back
    before the pool pass, the plain one fuses it), forward and gradients against the oracle"""
    from tgcn_amd import functional as F
    n, isolated, q, C, N, K, path_kind, _, _ = LAYER_CASES[case]
    op, L = _operand(n, isolated, kind)
    assert F._layer_path(op, q, n, C, N, K, mode).kind == path_kind
    rng = np.random.default_rng([list(LAYER_CASES).index(case), mode, pool])
    x = rng.standard_normal((q, n, C)).astype(np.float32)
    W = (rng.standard_normal((K, C, N)) / np.sqrt(K * C)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    y = _forward64(L, x, W, b, mode)
    gz = rng.standard_normal((q, n // pool, N)).astype(np.float32)
    want, gy = _relu_pool64(y, pool, gz)
    leaves = _leaves(x, W, b)
    z = F.cheb_relu_pool(op, *leaves, F.BIAS_CHANNEL, mode, pool)
    e = rel_err(z.detach().cpu().numpy(), want)
    assert e <= TOL, ("z", e)
    z.backward(_dev(gz))
    gx, gW = O.layer_backward(L, x, W, gy, MODE_NAME[mode])
    _check_grads(leaves, (gx, gW, _bias_grad64(gy, b)))


# ------------------------------------------------------------------------------------------------ cheb_time_windows
def _windows(series, H):
    """the windowed batch x[s*(T-H+1) + w, i, h] = series[s, i, w + h]"""
    S, n, T = series.shape
    nwin = T - H + 1
    return np.stack([series[:, :, w:w + H] for w in range(nwin)], axis=1).reshape(S * nwin, n, H)


def _unwindow_grad(gxw, S, T):
    """d series from the gradient of the windowed batch: every window adds into the columns it was cut from"""
    _, n, H = gxw.shape
    nwin = T - H + 1
    gxw = gxw.reshape(S, nwin, n, H)
    gs = np.zeros((S, n, T))
    for w in range(nwin):
        gs[:, :, w:w + H] += gxw[:, w]
    return gs


@pytest.mark.parametrize("bias_kind", [1, 2], ids=["bias_channel", "bias_vertex"])
@pytest.mark.parametrize("kind", KINDS, ids=["plain", "rcm", "hub_first"])
@pytest.mark.parametrize("mode", MODES, ids=["power", "chebyshev"])
@pytest.mark.parametrize("T,H,K", [(22, 15, 4), (24, 6, 3)], ids=["T22_H15_K4", "T24_H6_K3"])
def test_time_windows_on_reordered_operand_vs_oracle(T, H, K, mode, kind, bias_kind, gpu_device):
    """cheb_time_windows: output, d series, dW and db against the oracle's layer on the windowed batch"""
    from tgcn_amd import functional as F
    n, S, N = 1500, 2, 8
    op, L = _operand(n, 0.0, kind)
    rng = np.random.default_rng([T, mode, bias_kind])
    series = rng.standard_normal((S, n, T)).astype(np.float32)
    W = (rng.standard_normal((K, H, N)) / np.sqrt(K * H)).astype(np.float32)
    b = rng.standard_normal((N,) if bias_kind == F.BIAS_CHANNEL else (n, N)).astype(np.float32)
    xw = _windows(series, H)
    want = _forward64(L, xw, W, b, mode)
    leaves = _leaves(series, W, b)
    out = F.cheb_time_windows(op, *leaves, bias_kind, mode)
    e = rel_err(out.detach().cpu().numpy(), want)
    assert e <= TOL, ("out", e)
    g = rng.standard_normal(want.shape).astype(np.float32)
    out.backward(_dev(g))
    gxw, gW = O.layer_backward(L, xw, W, g, MODE_NAME[mode])
    _check_grads(leaves, (_unwindow_grad(gxw, S, T), gW, _bias_grad64(g, b)))


# ------------------------------------------------------------------------------------------------ cheb_stack
@pytest.mark.parametrize("kind", KINDS, ids=["plain", "rcm", "hub_first"])
@pytest.mark.parametrize("mode", MODES, ids=["power", "chebyshev"])
def test_stack_on_reordered_operand_vs_oracle(mode, kind, gpu_device):
    """cheb_stack called with data in the caller's labels (the nn modules' _chebyshev / _time_chebyshev, numpy_api) relabels in and out"""
    from tgcn_amd import functional as F
    n, q, C, K = 3000, 2, 8, 5
    op, L = _operand(n, 0.0, kind)
    x = np.random.default_rng(mode).standard_normal((q, n, C)).astype(np.float32)
    st = F.cheb_stack(op, _dev(x), K, mode)
    e = rel_err(st.cpu().numpy(), _stack(L, x, K, mode))
    assert e <= TOL, ("stack", e)
