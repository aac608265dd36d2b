"""Module backward at the baseline configurations' own training shapes (BASELINE.json configs 2-5; config 5 at 1/10 scale) and at the HCP
pipeline's shapes: x.grad, weight.grad and bias.grad against the fp64 references O.layer_backward_gside / O.windows_backward, which run the
hops on g (N columns) and so finish in seconds where O.layer_backward would take the K(K+1)/2 wide hops.  Every case asserts the layer path
it reaches (functional._layer_path) and whether the training forward kept the basis the weight gradient contracts with."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_err
from oracle import cheb_oracle as O

pytestmark = pytest.mark.gpu
TOL_GRAD = 2e-5
THREADS = 16          # host threads of the fp64 references' hops


def _host_L(op):
    import scipy.sparse as sp
    row, col, val = op.coo()
    return sp.csr_matrix((val.double().cpu().numpy(), (row.cpu().numpy(), col.cpu().numpy())), shape=(op.n, op.n))


class _PathRecorder:
    """Wraps functional.layer_backward: the LayerPath of each backward call and the basis its forward kept."""

    def __init__(self, monkeypatch):
        from tgcn_amd import functional as F
        self.calls = []
        real = F.layer_backward

        def spy(op, mode, fold, x3, W, g, bias_kind, bias_shape, needs, basis=None):
            K, Crow, N = W.shape
            path = F._layer_path(op, x3.shape[0], x3.shape[1], Crow, N, K, mode)
            self.calls.append((path.kind, basis))
            return real(op, mode, fold, x3, W, g, bias_kind, bias_shape, needs, basis=basis)
        monkeypatch.setattr(F, "layer_backward", spy)

    def only(self):
        assert len(self.calls) == 1, self.calls
        return self.calls[0]


def _check_grads(xg, Wg, bg, ref_x, ref_W, ref_b):
    assert rel_err(xg.cpu().numpy(), ref_x) <= TOL_GRAD
    Wg = Wg.cpu().numpy().reshape(ref_W.shape)
    assert rel_err(Wg, ref_W) <= TOL_GRAD
    for k in range(ref_W.shape[0]):               # each Chebyshev term on its own scale
        assert rel_err(Wg[k], ref_W[k]) <= TOL_GRAD, k
    assert rel_err(bg.cpu().numpy().reshape(ref_b.shape), ref_b) <= TOL_GRAD


def _mnist_grid(device):
    from tgcn_amd.graph import GraphOperand
    z = np.load(os.path.join(GOLDEN, "GCNCheb_grid784_q3_f1_g8_K5_x2d.npz"))
    n = int(z["n"])
    rowptr = torch.as_tensor(z["rowptr"])
    row = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
    return GraphOperand.from_coo(n, row.to(device), torch.as_tensor(z["col"]).long().to(device), torch.as_tensor(z["val"]).to(device))


def _module_case(layer, op, x, monkeypatch):
    """forward + backward of a dense-L module with a seeded g -> (recorded (kind, basis), g)"""
    rec = _PathRecorder(monkeypatch)
    xt = x.clone().requires_grad_(True)
    out = layer(xt)
    gen = torch.Generator(device="cuda").manual_seed(5)
    go = torch.randn(out.shape, device="cuda", generator=gen)
    out.backward(go)
    return rec.only(), xt.grad, go


@pytest.mark.parametrize("f", [1, 64])
def test_cfg2_mnist_gcncheb_backward(f, gpu_device, monkeypatch):
    """configs[1]: GCNCheb(L, f, 64, 5) on the 784-vertex MNIST grid, batch 128."""
    import tgcn_amd
    op = _mnist_grid(gpu_device)
    torch.manual_seed(1)
    layer = tgcn_amd.GCNCheb(op, f, 64, 5).cuda()
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((128, 784) if f == 1 else (128, 784, f), device="cuda", generator=gen)
    (kind, basis), xg, go = _module_case(layer, op, x, monkeypatch)
    assert kind == "small" and basis is None
    x4 = x.reshape(128, 784, f).cpu().numpy()
    rx, rW = O.layer_backward_gside(_host_L(op), x4, layer.weight.detach().cpu().numpy(), go.cpu().numpy(), "power")
    _check_grads(xg, layer.weight.grad, layer.bias.grad, rx.reshape(x.shape), rW,
                 go.double().sum(dim=(0, 1)).cpu().numpy().reshape(layer.bias.shape))


def test_cfg3_mnist_temporal_backward(gpu_device, monkeypatch):
    """configs[2]: TGCNCheb_H(L, 1, 64, 5, 28) on the MNIST grid, batch 64."""
    import tgcn_amd
    op = _mnist_grid(gpu_device)
    torch.manual_seed(1)
    layer = tgcn_amd.TGCNCheb_H(op, 1, 64, 5, 28).cuda()
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((64, 784, 28), device="cuda", generator=gen)
    (kind, basis), xg, go = _module_case(layer, op, x, monkeypatch)
    assert kind == "small" and basis is None
    rx, rW = O.layer_backward_gside(_host_L(op), x.cpu().numpy()[..., None], layer.weight.detach().cpu().numpy(), go.cpu().numpy(), "power")
    _check_grads(xg, layer.weight.grad, layer.bias.grad, rx[..., 0], rW, go.double().sum(dim=0, keepdim=True).cpu().numpy())


def test_cfg4_hcp_mesh_T1200_backward(gpu_device, monkeypatch):
    """configs[3]: TGCNCheb_H(L, 1, 32, 5, 1200), q = 1 on the 90 k-vertex sheet mesh: project-first, so the training forward keeps no
    basis and the backward recomputes the 2.16 GB monomial basis; dW with Kc = 1200 over ~940 row-block partials, dx through G = g W^T
    and 4 adjoint hops on 1200-wide rows."""
    import tgcn_amd
    from tools import synth
    n, row, col, val = synth.sheet_mesh(300, device=gpu_device)
    op = tgcn_amd.GraphOperand.from_coo(n, row, col, val, gpu_device)
    torch.manual_seed(1)
    layer = tgcn_amd.TGCNCheb_H(op, 1, 32, 5, 1200).cuda()
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((1, n, 1200), device="cuda", generator=gen)
    (kind, basis), xg, go = _module_case(layer, op, x, monkeypatch)
    assert kind == "project_first" and basis is None
    rx, rW = O.layer_backward_gside(_host_L(op), x.cpu().numpy()[..., None], layer.weight.detach().cpu().numpy(), go.cpu().numpy(), "power",
                                    threads=THREADS)
    _check_grads(xg, layer.weight.grad, layer.bias.grad, rx[..., 0], rW, go.double().sum(dim=0, keepdim=True).cpu().numpy())


@pytest.fixture(scope="module")
def rmat_1m(gpu_device):
    """configs[4] at 1/10 scale, as tests/test_baseline_configs.py::test_cfg5_reduced_rmat_tgcncheb: R-MAT 1 M vertices / 16 M entries,
    random labels, and its fp64 CSR on the host."""
    import tgcn_amd
    from tools import synth
    n, nnz = 1_000_000, 16_000_000
    _, row, col, val = synth.rmat(n, nnz, seed=12345, labeling="random", device=gpu_device)
    op = tgcn_amd.GraphOperand.from_coo(n, row, col, val, gpu_device)
    del row, col, val
    assert op.nnz == nnz
    return op, _host_L(op)


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("mode", [0, 1])
def test_cfg5_reduced_compact_backward(mode, keep, rmat_1m, monkeypatch):
    """The compact path in both recursions (mode 0: TGCNCheb(L, 64, 64, 5); mode 1: the functional layer, no module gives it on this
    operand), with the basis kept by the forward and recomputed by the backward: q is picked from the plan's n_c on either side of
    KEEP_BASIS_BYTES.  Mode 1 contracts compact_wgrad's S_out = S_all - dW[0] into every even term."""
    import tgcn_amd
    from tgcn_amd import functional as F
    op, L = rmat_1m
    K, C, N = 5, 64, 64
    plan = F.compact_plan_for(op, mode, K, 1, op.n, C, N)
    assert plan is not None and plan.n_empty > 0
    per_q = K * (plan.n_c + 1) * C * 4
    q_keep = F.KEEP_BASIS_BYTES // per_q
    assert 1 <= q_keep <= 8, (plan.n_c, q_keep)
    q = q_keep if keep else q_keep + 1
    assert F.choose_layout(q, op.n, C) == 0 and F.compact_plan_for(op, mode, K, q, op.n, C, N) is plan
    rec = _PathRecorder(monkeypatch)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((q, op.n, C), device="cuda", generator=gen).requires_grad_(True)
    torch.manual_seed(1)
    if mode == 0:
        layer = tgcn_amd.TGCNCheb(op, C, N, K).cuda()
        W, b = layer.weight, layer.bias
        out = layer(x)
    else:
        W = (torch.randn((K, C, N), device="cuda", generator=gen) / np.sqrt(K * C)).requires_grad_(True)
        b = torch.randn(N, device="cuda", generator=gen).requires_grad_(True)
        out = F.cheb_layer(op, x, W, b, F.BIAS_CHANNEL, mode)
    go = torch.randn(out.shape, device="cuda", generator=gen)
    out.backward(go)
    del out
    kind, basis = rec.only()
    assert kind == "compact"
    assert (basis is not None and basis.plan is plan) if keep else basis is None
    gx, gW, gb = x.grad, W.grad, b.grad
    x = x.detach()
    rx, rW = O.layer_backward_gside(L, x.cpu().numpy(), W.detach().cpu().numpy(), go.cpu().numpy(), "power" if mode == 0 else "chebyshev",
                                    threads=THREADS)
    ref_b = go.double().sum(dim=0, keepdim=True) if mode == 0 else go.double().sum(dim=(0, 1))
    _check_grads(gx, gW, gb, rx, rW, ref_b.cpu().numpy())


def test_true_recurrence_hcp_shape_backward(gpu_device, monkeypatch):
    """ChebTimeConv(1, 32, K=25, H=15), q = 4 on a 60 k-vertex sheet mesh (the pygeo HCP shape): hops-then-projection on the padded
    16-wide rows, basis kept by the forward, 24 Clenshaw hops on L^T."""
    import tgcn_amd
    from tools import synth
    n, row, col, _ = synth.sheet_mesh(245, device=gpu_device)
    assert 59_000 <= n <= 61_000
    ei = torch.stack([row, col])
    torch.manual_seed(1)
    layer = tgcn_amd.ChebTimeConv(1, 32, K=25, H=15).cuda()
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((4, n, 15), device="cuda", generator=gen).requires_grad_(True)
    rec = _PathRecorder(monkeypatch)
    out = layer(x, ei)
    go = torch.randn(out.shape, device="cuda", generator=gen)
    out.backward(go)
    kind, basis = rec.only()
    assert kind == "hops" and basis is not None and basis.plan is None
    r, c, lap = O.edge_laplacian(ei.cpu().numpy(), None, n, np.float64)
    L = O.coo_to_csr(r, c, lap, n)
    rx, rW = O.layer_backward_gside(L, x.detach().cpu().numpy()[..., None], layer.weight.detach().cpu().numpy(), go.cpu().numpy(), "chebyshev",
                                    threads=THREADS)
    _check_grads(x.grad, layer.weight.grad, layer.bias.grad, rx[..., 0], rW, go.double().sum(dim=(0, 1)).cpu().numpy())


def test_streaming_windows_backward_past_the_chunk_cap(gpu_device):
    """TGCNCheb_H(L, 1, 32, 5, 15).forward_series on one 75-step recording of the 90 k-vertex mesh: 61 windows x 90 k vertices = 5.49 M
    rows, past the 256-chunk cap of the windows weight gradient (each lane sums ~5400 products)."""
    import tgcn_amd
    from tgcn_amd import _lib
    from tools import synth
    n, row, col, val = synth.sheet_mesh(300, device=gpu_device)
    op = tgcn_amd.GraphOperand.from_coo(n, row, col, val, gpu_device)
    S, T, H, K, N = 1, 75, 15, 5, 32
    nwin = T - H + 1
    assert S * nwin * n > 256 * 16384
    assert _lib.lib().tgcn_cheb_windows_wgrad_workspace_bytes(S, n, T, H, N, K) == 256 * K * H * N * 4
    torch.manual_seed(1)
    layer = tgcn_amd.TGCNCheb_H(op, 1, N, K, H).cuda()
    gen = torch.Generator(device="cuda").manual_seed(0)
    series = torch.randn((S, n, T), device="cuda", generator=gen).requires_grad_(True)
    out = layer.forward_series(series)
    go = torch.randn(out.shape, device="cuda", generator=gen)
    out.backward(go)
    del out
    rs, rW = O.windows_backward(_host_L(op), series.detach().cpu().numpy(), layer.weight.detach().reshape(K, H, N).cpu().numpy(),
                                go.cpu().numpy(), "power", threads=THREADS)
    ref_b = go.double().view(S * nwin, n, N).sum(dim=0, keepdim=True).cpu().numpy()
    _check_grads(series.grad, layer.weight.grad, layer.bias.grad, rs, rW, ref_b)
