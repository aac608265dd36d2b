"""The five layer classes with bfloat16 parameters (model.to(torch.bfloat16)) on the golden graphs, on each of the small / project-first /
hops paths: forward and the three gradients against the fp64 oracle on the bf16-rounded x, W and upstream gradient, and against a numpy
emulation that rounds at exactly the points DESIGN.md "bf16 layers" lists.

Tolerances: the fp64 bound of every fixture is twice the emulation's own measured error against fp64 (TOL64, the measured values in the
comments); the GPU must agree with the emulation to a few bf16 ulps of the tensor's largest value (EMUL_ULPS, a rough bound: sums run in
another order, so a rounding point may land one ulp away and the hops carry it on).

Every test first checks that the library has the bf16 entries and FAILS without them (a bf16 layer on a library without them would run
fp32 kernels over bf16 buffers)."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import tgcn_amd
from tgcn_amd import functional as F
from conftest import GOLDEN, rel_err
from oracle import cheb_oracle as O
from test_bf16_kernels import require_bf16_entries

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EMUL_ULPS = 8


def bf(a):
    """round to bf16, to nearest even (what every rounding point of the layer does)"""
    return torch.from_numpy(np.asarray(a, np.float64)).to(BF).double().numpy()


# ------------------------------------------------------------------------------------------------- graphs and fixtures
def golden_graph(name):
    """(n, scipy CSR L-hat) of a committed golden graph"""
    if name == "pad48":
        z = np.load("%s/graph_chebyshev3d_pad48_K4.npz" % GOLDEN)
        n, rp, col, val = int(z["n"]), z["rowptr"], z["col"], z["val"]
    else:
        lm = {"grid784": "lmax2", "dti148": "lmax2", "rmat1024": "lmax1p5"}[name]
        z = np.load("%s/operand_%s_%s.npz" % (GOLDEN, name, lm))
        n, rp, col, val = int(z["n"]), z["L_rowptr"], z["L_col"], z["L_val"]
    return n, sp.csr_matrix((val.astype(np.float32), col, rp), shape=(n, n))


def empty_rows_graph():
    """an R-MAT-like graph with a third of its rows empty (isolated sources) and a hub row"""
    rng = np.random.default_rng(11)
    n = 600
    row = rng.integers(0, n, 5000)
    row = row[row % 3 != 0]
    row = np.concatenate([row, np.full(700, 4)])
    col = rng.integers(0, n, row.size)
    val = (rng.standard_normal(row.size) * 0.12).astype(np.float32)
    val[row == 4] /= 10
    L = sp.coo_matrix((val, (row, col)), shape=(n, n)).tocsr()
    return n, L


DENSE = ("TGCNCheb", "TGCNCheb_H", "GCNCheb")
# id: (class, graph, q, C, N, K, expected path); C is f for the plain classes, H * f (f = C / H, H = 16) for the time classes
FIXTURES = {
    "TGCNCheb-grid784-small": ("TGCNCheb", "grid784", 2, 16, 16, 5, "small"),
    "TGCNCheb-grid784-pf": ("TGCNCheb", "grid784", 2, 256, 32, 5, "project_first"),
    "TGCNCheb-grid784-hops": ("TGCNCheb", "grid784", 2, 256, 160, 5, "hops"),
    "TGCNCheb_H-dti148-small": ("TGCNCheb_H", "dti148", 3, 16, 8, 4, "small"),
    "TGCNCheb_H-dti148-pf": ("TGCNCheb_H", "dti148", 3, 256, 32, 5, "project_first"),
    "TGCNCheb_H-rmat1024-hops": ("TGCNCheb_H", "rmat1024", 2, 256, 144, 4, "hops"),
    "GCNCheb-rmat1024-small": ("GCNCheb", "rmat1024", 2, 16, 16, 3, "small"),
    "GCNCheb-pad48-pf": ("GCNCheb", "pad48", 4, 256, 64, 3, "project_first"),
    "GCNCheb-empty-rows-hops": ("GCNCheb", "empty", 2, 256, 256, 5, "hops"),
    "ChebConv-pad48-small": ("ChebConv", "pad48", 3, 16, 8, 4, "small"),
    "ChebConv-dti148-pf": ("ChebConv", "dti148", 2, 256, 48, 5, "project_first"),
    "ChebConv-rmat1024-hops-K25": ("ChebConv", "rmat1024", 2, 256, 160, 25, "hops"),
    "ChebTimeConv-grid784-small": ("ChebTimeConv", "grid784", 2, 16, 16, 5, "small"),
    "ChebTimeConv-rmat1024-pf": ("ChebTimeConv", "rmat1024", 2, 256, 16, 25, "project_first"),
    "ChebTimeConv-empty-rows-hops": ("ChebTimeConv", "empty", 2, 256, 176, 3, "hops"),
}
H = 16

# fp64 tolerance per fixture and tensor (y, gx, gW, gb) = 2 x the emulation's own rel_err against fp64, measured values in the comments
TOL64 = {
    "TGCNCheb-grid784-small": (4.1e-03, 6.3e-03, 4.0e-03, 5.3e-03),  # 2.06e-03 3.14e-03 2.00e-03 2.67e-03
    "TGCNCheb-grid784-pf": (5.7e-03, 7.4e-03, 6.4e-03, 5.1e-03),  # 2.87e-03 3.71e-03 3.20e-03 2.54e-03
    "TGCNCheb-grid784-hops": (7.2e-03, 6.9e-03, 5.6e-03, 5.0e-03),  # 3.61e-03 3.46e-03 2.82e-03 2.50e-03
    "TGCNCheb_H-dti148-small": (4.7e-03, 5.3e-03, 4.0e-03, 5.4e-03),  # 2.35e-03 2.67e-03 2.02e-03 2.68e-03
    "TGCNCheb_H-dti148-pf": (5.4e-03, 8.1e-03, 6.4e-03, 4.9e-03),  # 2.70e-03 4.07e-03 3.19e-03 2.44e-03
    "TGCNCheb_H-rmat1024-hops": (7.5e-03, 5.7e-03, 5.0e-03, 4.5e-03),  # 3.77e-03 2.87e-03 2.50e-03 2.25e-03
    "GCNCheb-rmat1024-small": (4.9e-03, 3.7e-03, 6.1e-03, 3.8e-03),  # 2.46e-03 1.84e-03 3.05e-03 1.92e-03
    "GCNCheb-pad48-pf": (5.1e-03, 6.4e-03, 5.1e-03, 6.3e-03),  # 2.54e-03 3.19e-03 2.56e-03 3.14e-03
    "GCNCheb-empty-rows-hops": (6.5e-03, 6.3e-03, 6.2e-03, 4.2e-03),  # 3.27e-03 3.15e-03 3.11e-03 2.12e-03
    "ChebConv-pad48-small": (3.9e-03, 5.9e-03, 3.4e-03, 4.9e-03),  # 1.95e-03 2.96e-03 1.72e-03 2.46e-03
    "ChebConv-dti148-pf": (7.0e-03, 4.0e-03, 6.1e-03, 5.7e-03),  # 3.52e-03 1.99e-03 3.03e-03 2.83e-03
    "ChebConv-rmat1024-hops-K25": (1.4e-02, 4.6e-03, 1.1e-02, 3.8e-03),  # 7.16e-03 2.31e-03 5.25e-03 1.92e-03
    "ChebTimeConv-grid784-small": (3.4e-03, 4.0e-03, 4.9e-03, 5.5e-03),  # 1.70e-03 2.00e-03 2.46e-03 2.75e-03
    "ChebTimeConv-rmat1024-pf": (4.1e-03, 5.9e-03, 1.1e-02, 4.6e-03),  # 2.03e-03 2.94e-03 5.40e-03 2.31e-03
    "ChebTimeConv-empty-rows-hops": (5.7e-03, 4.1e-03, 7.2e-03, 4.8e-03),  # 2.83e-03 2.06e-03 3.62e-03 2.41e-03
}


def make_case(name, dev):
    cls, graph, q, C, N, K, path = FIXTURES[name]
    n, L = empty_rows_graph() if graph == "empty" else golden_graph(graph)
    seed = sum(name.encode())
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    timed = cls in ("TGCNCheb_H", "ChebTimeConv")
    f = C // H if timed else C
    if cls in DENSE:
        Ld = torch.as_tensor(L.toarray())
        args = {"TGCNCheb": (Ld, f, N, K), "TGCNCheb_H": (Ld, f, N, K, H), "GCNCheb": (Ld, f, N, K)}[cls]
        m = getattr(tgcn_amd, cls)(*args)
        graph_args, L_op, mode = (), L, "power"
    else:
        r, c = L.nonzero()
        ei = torch.as_tensor(np.stack([r, c]).astype(np.int64))
        m = getattr(tgcn_amd, cls)(*((f, N, K, H) if timed else (f, N, K)))
        row, col, lap = O.edge_laplacian(ei.numpy(), None, n)
        L_op = O.coo_to_csr(row, col, lap, n)
        graph_args, mode = (ei.to(dev),), "chebyshev"
    with torch.no_grad():
        if m.bias is not None:
            m.bias.uniform_(-0.5, 0.5)
    x = rng.standard_normal((q, n, H, f) if timed else (q, n, f)).astype(np.float32)
    go = rng.standard_normal((q, n, N)).astype(np.float32)
    return m.to(dev), torch.as_tensor(x, device=dev), graph_args, L_op, mode, path, torch.as_tensor(go, device=dev)


# ------------------------------------------------------------------------------------------------- references
def _apply(L, X):
    q, n, C = X.shape
    return (L @ X.transpose(1, 0, 2).reshape(n, q * C)).reshape(n, q, C).transpose(1, 0, 2)


def _fold(K):
    c = np.zeros((K, K))
    for k in range(K):
        c[k, k] = 1.0 if k < 2 else 2.0
        if k >= 2:
            c[k] -= c[k - 2]
    return c


def _bias_add(y, b):
    return y if b is None else y + b.reshape((1,) + b.shape[-2:] if b.ndim == 3 else (1, 1, -1))


def fp64_reference(L, x3, W, b, g, mode):
    """the oracle's forward and layer_backward in fp64 on the given (already bf16-rounded) values; x3 (q, n, C), W (K, C, N)"""
    K = W.shape[0]
    L64 = sp.csr_matrix(L, dtype=np.float64)
    stack = (O.stack_reference_power if mode == "power" else O.stack_chebyshev)(L64, x3, K)
    y = _bias_add(np.einsum("kqnc,kcg->qng", stack, W), b)
    gx, gW = O.layer_backward(L64, x3, W, g, mode)
    gb = None if b is None else (g.sum(axis=(0, 1)) if b.size == g.shape[2] else g.sum(axis=0)).reshape(b.shape)
    return y, gx, gW, gb


def emulate(path, L, x3, W, b, g, mode):
    """The bf16 layer in fp64 with the rounding points of each path (DESIGN.md "bf16 layers"); inputs already bf16 values."""
    K = W.shape[0]
    L64 = sp.csr_matrix(L, dtype=np.float64)
    LT = L64.T.tocsr()
    if path == "small":                                     # fp32 one-launch kernels on the upcast operands: only the outputs round
        y, gx, gW, gb = fp64_reference(L, x3, W, b, g, mode)
        return bf(y), bf(gx), bf(gW), None if gb is None else bf(gb)
    c = _fold(K) if mode == "power" and K > 2 else None
    Wt = bf(np.einsum("kj,kcn->jcn", c, W)) if c is not None else W       # the fold runs in fp32 and is rounded once
    mono = mode == "power"
    # the basis the bf16 hops produce (every hop rounds) -- the hops path's forward, and the weight gradient of both general paths
    terms = [x3]
    for k in range(1, K):
        if mono or k == 1:
            terms.append(bf(_apply(L64, terms[k - 1])))
        else:
            terms.append(bf(2 * _apply(L64, terms[k - 1]) - terms[k - 2]))
    if path == "project_first":                             # fp32 Z and fp32 hops: one rounding at the output
        exact = [x3]
        for k in range(1, K):
            exact.append(_apply(L64, exact[k - 1]) if (mono or k == 1) else 2 * _apply(L64, exact[k - 1]) - exact[k - 2])
        y = bf(_bias_add(sum(np.einsum("qnc,cg->qng", exact[k], Wt[k]) for k in range(K)), b))
    else:
        y = bf(_bias_add(sum(np.einsum("qnc,cg->qng", terms[k], Wt[k]) for k in range(K)), b))
    dWt = np.stack([np.einsum("qnc,qng->cg", terms[k], g) for k in range(K)])
    gW = bf(np.einsum("kj,jcn->kcn", c, dWt) if c is not None else dWt)
    G = [np.einsum("qng,cg->qnc", g, Wt[k]) for k in range(K)]          # fp32 projection, fp32 adjoint hops
    gx = np.zeros_like(x3)
    for k in range(K):
        P = G[k]
        if mono:
            for _ in range(k):
                P = _apply(LT, P)
            gx += P
        else:
            gx += O.stack_chebyshev(LT, G[k], k + 1)[k]
    gb = None if b is None else bf((g.sum(axis=(0, 1)) if b.size == g.shape[2] else g.sum(axis=0)).reshape(b.shape))
    return y, bf(gx), gW, gb


def case_arrays(m, x, go):
    """(x3, W (K, C, N), bias, g) as fp64 numpy of the bf16 values the layer computes with"""
    K = m.weight.shape[0]
    W = m.weight.detach().double().cpu().numpy().reshape(K, -1, m.weight.shape[-1])
    b = None if m.bias is None else m.bias.detach().double().cpu().numpy()
    q, n = x.shape[:2]
    return bf(x.double().cpu().numpy().reshape(q, n, -1)), W, b, bf(go.double().cpu().numpy())


def run_bf16(m, x, graph_args, go):
    xb = x.clone().requires_grad_(True)
    out = m(xb, *graph_args)
    out.backward(go.to(BF))
    return out, xb.grad, m.weight.grad, None if m.bias is None else m.bias.grad


# ------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", list(FIXTURES))
def test_bf16_layer_forward_and_gradients(gpu_device, name):
    require_bf16_entries()
    m32, x, graph_args, L, mode, path, go = make_case(name, gpu_device)
    m = copy.deepcopy(m32).to(BF)
    q, n = x.shape[:2]
    K, N = m.weight.shape[0], m.weight.shape[-1]
    C = m.weight.numel() // (K * N)
    op = m._operand(gpu_device) if FIXTURES[name][0] in DENSE else m._operand(x, *graph_args, None)
    assert F._layer_path(op, q, n, C, N, K, F.MODE_POWER if mode == "power" else F.MODE_CHEBYSHEV, compact=False).kind == path
    out, gx, gW, gb = run_bf16(m, x, graph_args, go)
    assert out.dtype == BF and gx.dtype == torch.float32 and gW.dtype == BF and (gb is None or gb.dtype == BF)
    x3, W, b, g = case_arrays(m, x, go)
    ref = fp64_reference(L, x3, W, b, g, mode)
    emu = emulate(path, L, x3, W, b, g, mode)
    got = [out, gx, gW.reshape(K, C, N), gb]
    tol = TOL64[name]
    for i, label in enumerate(("y", "gx", "gW", "gb")):
        if ref[i] is None:
            continue
        gv = got[i].detach().double().cpu().numpy().reshape(ref[i].shape)
        scale = np.abs(emu[i]).max()
        assert np.abs(gv - emu[i]).max() <= EMUL_ULPS * 2.0 ** -8 * scale, (label, float(np.abs(gv - emu[i]).max() / scale))
        assert rel_err(gv, ref[i]) <= tol[i], (label, rel_err(gv, ref[i]), tol[i])


def test_bf16_input_gradient_follows_the_input_dtype(gpu_device):
    """x.grad has x's dtype (autograd casts the bf16 gradient of the cast); with a bf16 input it is bf16"""
    require_bf16_entries()
    m32, x, graph_args, L, mode, path, go = make_case("TGCNCheb-grid784-hops", gpu_device)
    m = copy.deepcopy(m32).to(BF)
    xb = x.to(BF).requires_grad_(True)
    m(xb).backward(go.to(BF))
    assert xb.grad.dtype == BF


def test_fp32_model_is_bitwise_unchanged_and_bf16_is_deterministic(gpu_device):
    require_bf16_entries()
    for name in ("TGCNCheb-grid784-small", "TGCNCheb-grid784-pf", "TGCNCheb-grid784-hops", "ChebConv-rmat1024-hops-K25"):
        m32, x, graph_args, L, mode, path, go = make_case(name, gpu_device)
        before = m32(x, *graph_args).detach().clone()          # evaluated before any bf16 call on this model
        m = copy.deepcopy(m32).to(BF)
        y1 = m(x, *graph_args)
        y2 = m(x, *graph_args)
        assert torch.equal(y1, y2), name
        assert torch.equal(m32(x, *graph_args), before), name
        assert m32.weight.dtype == torch.float32


def test_reference_style_network_trains_in_bf16(gpu_device):
    """a network written like the reference's HCP model (TGCNCheb_H -> relu -> gcn_pool_4 -> flatten -> Linear), .to(bfloat16), trains"""
    require_bf16_entries()
    n, L = golden_graph("dti148")
    n4 = n - n % 4
    Ld = torch.as_tensor(L.toarray()[:n4, :n4])

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = tgcn_amd.TGCNCheb_H(Ld, 1, 16, 5, 15)
            self.fc1 = torch.nn.Linear(n4 // 4 * 16, 6)

        def forward(self, x):
            x = tgcn_amd.gcn_pool_4(torch.relu(self.conv1(x)))
            return self.fc1(x.reshape(x.shape[0], -1))

    torch.manual_seed(0)
    net = Net().to(gpu_device).to(BF)
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    x = torch.randn(8, n4, 15, device=gpu_device)
    target = torch.randint(0, 6, (8,), device=gpu_device)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(net(x).float(), target)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        assert net.conv1.weight.grad.dtype == BF
    assert all(np.isfinite(losses)), losses
