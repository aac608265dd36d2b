"""bfloat16 reference-power layers on compact hop tensors (DESIGN.md 3.9 "compacted"): the row-mapped bf16 projection
(tgcn_cheb_project_mapped_bf16) against tgcn_cheb_project_bf16 on explicitly gathered rows, the bf16 row gather (tgcn_pack_rows_bf16) against
index_select, and F.cheb_layer / TGCNCheb with bf16 parameters compacted against the same call with F.COMPACT_BF16 = False.

Bounds.  Forward, x.grad and bias.grad: torch.equal -- a kept row's hops sum the same entries in the same order on the compact operand, a
projection row's sums do not depend on its tile row, and the input / bias gradients run the same code.  weight.grad: EMUL_ULPS = 8 bf16 ulps
of the tensor's largest value (tests/test_bf16_layers.py's rule): the row blocks of the two-stage reduction fold in another order.  Against
fp64 (oracle.cheb_oracle on the bf16-rounded x, W and g): the compacted layer's rel_err is at most twice the uncompacted layer's own, measured
in the same test.

Every test first checks that the library has the two entries and FAILS without them."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F
from conftest import rel_err
from oracle import cheb_oracle as O
from test_bf16_layers import EMUL_ULPS
from test_compact_wave import _rmat_like

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
ENTRIES = ("tgcn_cheb_project_mapped_bf16", "tgcn_pack_rows_bf16")
SENTINEL = 7.0


def require_entries():
    handle = _lib.lib()
    missing = [e for e in ENTRIES if not hasattr(handle, e)]
    assert not missing, "libtgcn_hip has no %s" % missing


# ------------------------------------------------------------------------------------------------- the mapped projection
@pytest.mark.parametrize("N", [8, 48, 80])
@pytest.mark.parametrize("Kc", [8, 20, 64], ids=["Kc8-zero-tail", "Kc20-element-form", "Kc64-full-steps"])
def test_mapped_projection_equals_projection_of_gathered_rows(Kc, N, gpu_device):
    require_entries()
    dev = gpu_device
    n_v = 300
    g = torch.Generator().manual_seed(Kc * 100 + N)
    for M in (5, 130):
        rows = torch.randperm(n_v, generator=g)[:M].sort().values
        rowmap = rows.to(torch.int32).to(dev)
        rows_d = rows.to(dev)
        for nterms, mapped in ((1, 0b1), (3, 0b001), (3, 0b101)):
            W = (torch.randn(nterms, Kc, N, generator=g) / (nterms * Kc) ** 0.5).to(BF).to(dev)
            for nb in (1, 3):
                # mapped terms have a row per vertex, the others a row per tile row (and one more, as the compact buffers do)
                nrows = [n_v if (mapped >> t) & 1 else M + 1 for t in range(nterms)]
                terms = [torch.randn(nb, nrows[t], Kc, generator=g).to(BF).to(dev) for t in range(nterms)]
                gathered = [[(terms[t][b][rows_d] if (mapped >> t) & 1 else terms[t][b][:M]).contiguous() for t in range(nterms)] for b in range(nb)]
                for bias_kind in (F.BIAS_NONE, F.BIAS_CHANNEL, F.BIAS_VERTEX_CHANNEL):
                    for bdt in ((torch.float32,) if bias_kind == F.BIAS_NONE else (torch.float32, BF)):
                        bias = None
                        if bias_kind:
                            bias = torch.randn((N,) if bias_kind == F.BIAS_CHANNEL else (n_v, N), generator=g).to(bdt).to(dev)
                        bias_g = bias[rows_d].contiguous() if bias_kind == F.BIAS_VERTEX_CHANNEL else bias
                        for odt in (BF, torch.float32):
                            out = torch.full((nb, n_v, N), SENTINEL, dtype=odt, device=dev)
                            F.project_mapped_bf16(terms, [nrows[t] * Kc for t in range(nterms)], W.view(nterms * Kc, N), bias, bias_kind, n_v, rowmap,
                                                  mapped, nb, out)
                            what = (M, nterms, mapped, nb, bias_kind, bdt, odt)
                            untouched = torch.ones(n_v, dtype=torch.bool, device=dev)
                            untouched[rows_d] = False
                            assert bool((out[:, untouched] == SENTINEL).all()), what
                            for b in range(nb):
                                ref = F.cheb_project_bf16(gathered[b], W, bias_g, bias_kind, M, out_dtype=odt)
                                assert ref.dtype == odt and torch.equal(out[b][rows_d], ref), what


def test_mapped_projection_refuses_bad_arguments(gpu_device):
    require_entries()
    dev = gpu_device
    L = _lib.lib()
    import ctypes as C
    x = torch.randn(2, 16, 8, device=dev).to(BF)
    W = torch.randn(8, 8, device=dev).to(BF)
    out = torch.full((2, 16, 8), SENTINEL, dtype=BF, device=dev)
    rowmap = torch.arange(4, dtype=torch.int32, device=dev)
    a, lda, a_bs = (C.c_void_p * 1)(x.data_ptr()), (C.c_int64 * 1)(8), (C.c_int64 * 1)(16 * 8)

    def call(rm, nbatch, bs):
        return L.tgcn_cheb_project_mapped_bf16(_lib.stream_ptr(), 4, 8, 8, 1, a, lda, _lib.ptr(W), None, 0, 0, 16, rm, 1, nbatch, bs, 16 * 8,
                                               _lib.ptr(out), 8, 1)
    assert call(None, 1, a_bs) != 0 and call(_lib.ptr(rowmap), 0, a_bs) != 0 and call(_lib.ptr(rowmap), 2, None) != 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call(_lib.ptr(rowmap), 2, a_bs) == 0
    assert torch.equal(out[:, :4], F.cheb_project_bf16([x.view(32, 8)], W.view(1, 8, 8), None, 0, 32).view(2, 16, 8)[:, :4])
    assert bool((out[:, 4:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------- the row gather
@pytest.mark.parametrize("C_row", [1, 20, 64])
def test_pack_rows_bf16_equals_index_select(C_row, gpu_device):
    require_entries()
    dev = gpu_device
    g = torch.Generator().manual_seed(C_row)
    n_src, n_out = 500, 333
    idx = torch.randint(0, n_src, (n_out,), generator=g).to(dev)
    flat = torch.randn(n_src * (C_row + 8) + 16, generator=g).to(BF).to(dev)
    views = {
        "contiguous": flat[: n_src * C_row].view(n_src, C_row),
        "base-off-16-bytes": flat[4: 4 + n_src * C_row].view(n_src, C_row),            # 8 bytes into a 16-byte unit
        "strided": flat[: n_src * (C_row + 8)].view(n_src, C_row + 8)[:, :C_row],     # ld_src = C + 8
    }
    assert views["base-off-16-bytes"].data_ptr() % 16 == 8
    for name, src in views.items():
        out = torch.full((n_out + 1, C_row), SENTINEL, dtype=BF, device=dev)
        F.pack_rows_bf16(src, idx, out[:n_out])
        assert torch.equal(out[:n_out], src.index_select(0, idx)), name
        assert bool((out[n_out] == SENTINEL).all()), name
    # an output that starts off a 16-byte boundary
    buf = torch.full((n_out * C_row + 8,), SENTINEL, dtype=BF, device=dev)
    out = buf[4: 4 + n_out * C_row].view(n_out, C_row)
    F.pack_rows_bf16(views["contiguous"], idx, out)
    assert torch.equal(out, views["contiguous"].index_select(0, idx)) and bool((buf[:4] == SENTINEL).all()) and bool((buf[-4:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------- the layer
def _fp64_layer(L, x3, W, b, g):
    """the reference-power layer and its gradients in fp64 (oracle.cheb_oracle) on bf16-rounded values"""
    K = W.shape[0]
    L64 = sp.csr_matrix(L, dtype=np.float64)
    stack = O.stack_reference_power(L64, x3, K)
    q, n, Cr = x3.shape
    y = sum(stack[k].reshape(q * n, Cr) @ W[k] for k in range(K)).reshape(q, n, -1)
    if b is not None:
        y = y + b.reshape((1, 1, -1) if b.ndim == 1 else (1,) + b.shape)
    gx, gW = O.layer_backward_gside(L64, x3, W, g, "power")
    gb = None if b is None else (g.sum(axis=(0, 1)) if b.ndim == 1 else g.sum(axis=0))
    return y, gx, gW, gb


def _run_layer(op, x, W, bias, bias_kind, go):
    xb = x.clone().requires_grad_(True)
    Wb = W.clone().requires_grad_(True)
    bb = None if bias is None else bias.clone().requires_grad_(True)
    out = F.cheb_layer(op, xb, Wb, bb, bias_kind, F.MODE_POWER)
    out.backward(go)
    return out.detach(), xb.grad, Wb.grad, None if bb is None else bb.grad


@pytest.mark.parametrize("symmetric", [True, False], ids=["symmetric", "entries-into-empty-rows"])
# (1, 24, 8, 2, 0): 2 N <= C, the project-first path -- the switch must change nothing there; the other two shapes run compacted
@pytest.mark.parametrize("q,C_row,N,K,bias_kind", [(3, 64, 64, 5, 2), (2, 32, 48, 3, 1), (1, 24, 8, 2, 0)])
def test_compacted_bf16_layer_equals_uncompacted(q, C_row, N, K, bias_kind, symmetric, gpu_device, monkeypatch):
    from tgcn_amd import graph
    require_entries()
    dev = gpu_device
    monkeypatch.setattr(graph, "COMPACT_MIN_ROWS", 1)
    n = 40000
    rng = np.random.default_rng(q * 100 + C_row + K)
    row, col, val = _rmat_like(n, 50000, rng, symmetric)
    as_dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    op = graph.GraphOperand.from_coo(n, as_dev(row), as_dev(col), as_dev(val))
    plan = op.compact_plan()
    assert plan is not None and plan.n_c + plan.n_empty == n and plan.n_empty > n / 8
    deg = np.bincount(row, minlength=n)
    if not symmetric:
        assert (deg[col] == 0).any()          # entries that point at vertices without a compact row: they gather the zero row
    assert deg.max() > 64                     # a hub row: the long-row fold
    x = as_dev(rng.standard_normal((q, n, C_row)).astype(np.float32)).to(BF)
    W = as_dev((rng.standard_normal((K, C_row, N)) / np.sqrt(K * C_row)).astype(np.float32)).to(BF)
    bias = None if bias_kind == 0 else as_dev(rng.standard_normal((N,) if bias_kind == 1 else (n, N)).astype(np.float32)).to(BF)
    go = as_dev(rng.standard_normal((q, n, N)).astype(np.float32)).to(BF)

    monkeypatch.setattr(F, "COMPACT_BF16", False)
    plain = _run_layer(op, x, W, bias, bias_kind, go)
    monkeypatch.setattr(F, "COMPACT_BF16", True)
    comp = _run_layer(op, x, W, bias, bias_kind, go)
    assert comp[0].dtype == BF and comp[2].dtype == BF
    assert torch.equal(comp[0], plain[0]), "forward"
    assert torch.equal(comp[1], plain[1]), "x.grad"
    if bias is not None:
        assert torch.equal(comp[3], plain[3]), "bias.grad"
    scale = float(plain[2].float().abs().max())
    dw = float((comp[2].float() - plain[2].float()).abs().max())
    assert dw <= EMUL_ULPS * 2.0 ** -8 * scale, ("weight.grad", dw / scale)

    # over the keep limit the backward recomputes the compact terms: the same gradients
    with monkeypatch.context() as m:
        m.setattr(F, "KEEP_BASIS_BYTES", 0)
        again = _run_layer(op, x, W, bias, bias_kind, go)
    assert torch.equal(again[0], comp[0]) and torch.equal(again[2], comp[2])

    # the inference forward in its automatic passes, and forced into passes of two samples (q = 3: two and one)
    with torch.no_grad():
        one = F.cheb_layer(op, x, W, bias, bias_kind, F.MODE_POWER)
        assert torch.equal(one, plain[0])
        if q > 1 and F._layer_path(op, q, n, C_row, N, K, F.MODE_POWER, compact=False).kind == "hops":
            key = ("bf16", K, C_row, q)
            assert plan.q_chunk_cache.get(key) == q
            per_q = (K - 1) * (plan.n_c + 1) * C_row * 2
            most = max(1, q - 1)
            with monkeypatch.context() as m:
                m.setattr(torch.cuda, "mem_get_info", lambda d=None: (int((most + 0.5) * per_q / F.COMPACT_WS_FRACTION), 1 << 40))
                plan.q_chunk_cache.clear()
                two = F.cheb_layer(op, x, W, bias, bias_kind, F.MODE_POWER)
                assert plan.q_chunk_cache[key] < q
            plan.q_chunk_cache.clear()
            assert torch.equal(two, one), "passes"

    # against fp64 on the bf16-rounded operands: no worse than twice the uncompacted layer's own error
    L = sp.coo_matrix((val.astype(np.float64), (row, col)), shape=(n, n)).tocsr()
    b64 = None if bias is None else bias.double().cpu().numpy()
    ref = _fp64_layer(L, x.double().cpu().numpy(), W.double().cpu().numpy(), b64, go.double().cpu().numpy())
    for i, label in enumerate(("y", "gx", "gW", "gb")):
        if ref[i] is None:
            continue
        ec = rel_err(comp[i].double().cpu().numpy().reshape(ref[i].shape), ref[i])
        ep = rel_err(plain[i].double().cpu().numpy().reshape(ref[i].shape), ref[i])
        print("%s: rel_err compacted %.3e uncompacted %.3e" % (label, ec, ep))
        assert ec <= 2 * ep, "%s: compacted %.3e, uncompacted %.3e" % (label, ec, ep)


def test_tgcncheb_module_on_a_scipy_operand(gpu_device, monkeypatch):
    from tgcn_amd import graph
    require_entries()
    monkeypatch.setattr(graph, "COMPACT_MIN_ROWS", 1)
    n = 40000
    rng = np.random.default_rng(5)
    row, col, val = _rmat_like(n, 50000, rng, True)
    L = sp.coo_matrix((val, (row, col)), shape=(n, n)).tocsr()
    torch.manual_seed(0)
    m = tgcn_amd.TGCNCheb(L, 32, 32, 3).to(gpu_device).to(BF)
    with torch.no_grad():
        m.bias.uniform_(-0.5, 0.5)
    x = torch.randn(2, n, 32, device=gpu_device)
    op = m._operand(gpu_device)
    assert op.compact_plan() is not None and F.compact_plan_for(op, F.MODE_POWER, 3, 2, n, 32) is not None
    outs = {}
    for switch in (True, False):
        monkeypatch.setattr(F, "COMPACT_BF16", switch)
        with torch.no_grad():
            outs[switch] = m(x)
    assert outs[True].dtype == BF and torch.equal(outs[True], outs[False])
    assert bool(torch.isfinite(outs[True].float()).all()) and float(outs[True].float().abs().max()) > 0
