"""The bf16 entries of the library against fp64 on the same bf16 values: tgcn_csr_hop_bf16 / tgcn_csr_hop2_bf16 (every element within one
bf16 ulp of the fp64 product rounded to bf16), tgcn_cheb_project_bf16 in its fp32-output mode (1e-5 of fp64) and tgcn_cheb_wgrad_bf16 (1e-5
of fp64, bitwise equal across two runs).

Every test first checks that the library has the bf16 entries and FAILS without them: on a library that lacks them a bf16 buffer would be
handed to an fp32 kernel, which reads past its end."""
import numpy as np
import pytest
import torch

from tgcn_amd import _lib
from tgcn_amd import functional as F
from tgcn_amd.graph import GraphOperand

pytestmark = pytest.mark.gpu

BF16_ENTRIES = ("tgcn_csr_hop_bf16", "tgcn_csr_hop2_bf16", "tgcn_cheb_project_bf16", "tgcn_cheb_wgrad_bf16")


def require_bf16_entries():
    handle = _lib.lib()
    missing = [e for e in BF16_ENTRIES if not hasattr(handle, e)]
    assert not missing, "libtgcn_hip has no bf16 entries %s" % missing


def _bf(a, dev):
    return torch.as_tensor(np.asarray(a, np.float32)).to(dev).to(torch.bfloat16)


def _np(t):
    return t.detach().double().cpu().numpy()


def _ulp_bf16(v):
    """one bf16 ulp at |v| (8 significant bits)"""
    a = np.maximum(np.abs(v), np.finfo(np.float32).tiny)
    return np.exp2(np.floor(np.log2(a)) - 7)


def _round_bf16(a):
    return torch.from_numpy(np.asarray(a, np.float64)).to(torch.bfloat16).double().numpy()


def _graph(n, rng, dev):
    """random rows of 0..12 entries, every 7th row empty, and two hub rows long enough for the fix-up path (rows above row_thresh)"""
    deg = rng.integers(0, 13, n)
    deg[::7] = 0
    deg[5] = deg[n // 2] = 6000
    row = np.repeat(np.arange(n), deg)
    col = rng.integers(0, n, row.size)
    val = (rng.standard_normal(row.size) / 4).astype(np.float32)
    val[row == 5] /= 40
    val[row == n // 2] /= 40
    import scipy.sparse as sp
    L = sp.coo_matrix((val.astype(np.float64), (row, col)), shape=(n, n)).tocsr()
    op = GraphOperand.from_coo(n, torch.as_tensor(row, device=dev), torch.as_tensor(col, device=dev), torch.as_tensor(val, device=dev), dev)
    return L, op


def _apply(L, X):
    q, n, C = X.shape
    return (L @ X.transpose(1, 0, 2).reshape(n, q * C)).reshape(n, q, C).transpose(1, 0, 2)


@pytest.mark.parametrize("C", [8, 16, 24, 64, 128, 1024])
@pytest.mark.parametrize("form", ["plain", "alpha_beta", "clenshaw", "strided"])
def test_hop_bf16_within_one_ulp_of_fp64(gpu_device, C, form):
    require_bf16_entries()
    rng = np.random.default_rng(C + len(form))
    n, nb = 1500, 3
    L, op = _graph(n, rng, gpu_device)
    x = _bf(rng.standard_normal((nb, n, C)), gpu_device)
    z = _bf(rng.standard_normal((nb, n, C)), gpu_device)
    z2 = _bf(rng.standard_normal((nb, n, C)), gpu_device)
    y_out = None
    if form == "strided":
        # batch and row strides beyond the row (a 16-byte aligned pitch keeps the 8-element lanes; C + 4 takes the scalar form)
        pitch = C + (8 if C % 16 == 0 else 4)
        xs = torch.zeros((nb, n + 1, pitch), dtype=torch.bfloat16, device=gpu_device)
        xs[:, :n, :C] = x
        x = xs[:, :n, :C]
        ys = torch.zeros((nb, n + 1, pitch), dtype=torch.bfloat16, device=gpu_device)
        y_out = ys[:, :n, :C]
    if form == "plain" or form == "strided":
        y = F.csr_hop_bf16(op, x, out=y_out)
        ref = _apply(L, _np(x))
    elif form == "alpha_beta":
        y = F.csr_hop_bf16(op, x, z=z, alpha=2.0, beta=-1.0)
        ref = 2.0 * _apply(L, _np(x)) - _np(z)
    else:
        y = F.csr_hop_bf16(op, x, z=z, alpha=2.0, beta=-1.0, z2=z2, gamma=1.0)
        ref = 2.0 * _apply(L, _np(x)) - _np(z) + _np(z2)
    sched = F.schedule_for_bf16(op, C, F._aligned16_bf16(C, x, y))
    assert sched.struct.nlong > 0, "the graph must reach the fix-up path"
    torch.cuda.synchronize()
    got = _np(y)
    ref_b = _round_bf16(ref)
    # one ulp of the rounded value; near zero the fp32 sum of many terms may differ from fp64 by its own rounding of the addends' scale
    tol = _ulp_bf16(ref_b) + 2.0 ** -20 * np.abs(ref).max()
    bad = np.abs(got - ref_b) > tol
    assert not bad.any(), (int(bad.sum()), float(np.abs(got - ref_b).max()))
    if form == "alpha_beta":            # empty rows: y = -z exactly
        assert np.array_equal(got[:, ::7], -_np(z)[:, ::7])


def _proj_ref(terms, W, bias, kind, n_vertices, interleave=1):
    M = terms[0].shape[0]
    out = sum(t.astype(np.float64) @ W[i].astype(np.float64) for i, t in enumerate(terms))
    if interleave > 1:
        m = np.arange(M)
        orow = (m % interleave) * n_vertices + m // interleave
        res = np.empty_like(out)
        res[orow] = out
        out = res
    if kind == F.BIAS_CHANNEL:
        out = out + bias.reshape(1, -1)
    elif kind == F.BIAS_VERTEX_CHANNEL:
        out = out + np.tile(bias.reshape(n_vertices, -1), (M // n_vertices, 1))
    return out


@pytest.mark.parametrize("T,Kc,N", [(1, 64, 48), (3, 20, 16), (5, 24, 100), (33, 8, 32), (2, 1200, 160)])
@pytest.mark.parametrize("bias", ["none", "channel_f32", "vertex_bf16", "channel_bf16"])
@pytest.mark.parametrize("interleave", [1, 3])
def test_project_bf16_fp32_output_matches_fp64(gpu_device, T, Kc, N, bias, interleave):
    require_bf16_entries()
    rng = np.random.default_rng(T * 1000 + Kc + N)
    n_v = 97
    M = n_v * 3
    terms = [_bf(rng.standard_normal((M, Kc)), gpu_device) for _ in range(T)]
    W = _bf(rng.standard_normal((T, Kc, N)) / np.sqrt(T * Kc), gpu_device)
    kind, b = F.BIAS_NONE, None
    if bias != "none":
        kind = F.BIAS_CHANNEL if bias.startswith("channel") else F.BIAS_VERTEX_CHANNEL
        shape = (N,) if kind == F.BIAS_CHANNEL else (n_v, N)
        b = torch.as_tensor(rng.standard_normal(shape).astype(np.float32), device=gpu_device)
        if bias.endswith("bf16"):
            b = b.to(torch.bfloat16)
    out = F.cheb_project_bf16(terms, W, b, kind, n_v, out_dtype=torch.float32, interleave=interleave)
    assert out.dtype == torch.float32
    ref = _proj_ref([_np(t) for t in terms], _np(W), None if b is None else _np(b), kind, n_v, interleave)
    err = np.abs(_np(out) - ref).max() / np.abs(ref).max()
    assert err <= 1e-5, err            # T = 33: two launches, the second accumulates into the fp32 output


def test_project_bf16_rounds_its_bf16_output_once(gpu_device):
    require_bf16_entries()
    rng = np.random.default_rng(3)
    terms = [_bf(rng.standard_normal((500, 40)), gpu_device) for _ in range(3)]
    W = _bf(rng.standard_normal((3, 40, 24)) / 10, gpu_device)
    b = _bf(rng.standard_normal(24), gpu_device)
    o32 = F.cheb_project_bf16(terms, W, b, F.BIAS_CHANNEL, 500, out_dtype=torch.float32)
    o16 = F.cheb_project_bf16(terms, W, b, F.BIAS_CHANNEL, 500)
    assert o16.dtype == torch.bfloat16
    assert torch.equal(o16, o32.to(torch.bfloat16))


@pytest.mark.parametrize("T,M,Kc,N", [(1, 64, 16, 16), (5, 3000, 64, 64), (7, 1001, 20, 70), (3, 50000, 15, 32)])
def test_wgrad_bf16_matches_fp64_and_is_deterministic(gpu_device, T, M, Kc, N):
    require_bf16_entries()
    rng = np.random.default_rng(M + Kc)
    terms = [_bf(rng.standard_normal((M, Kc)), gpu_device) for _ in range(T)]
    g = _bf(rng.standard_normal((M, N)), gpu_device)
    dW = F.cheb_wgrad_bf16(terms, g)
    dW2 = F.cheb_wgrad_bf16(terms, g)
    assert dW.dtype == torch.float32 and tuple(dW.shape) == (T, Kc, N)
    assert torch.equal(dW, dW2)
    ref = np.stack([_np(t).T @ _np(g) for t in terms])
    err = np.abs(_np(dW) - ref).max() / np.abs(ref).max()
    assert err <= 1e-5, err
