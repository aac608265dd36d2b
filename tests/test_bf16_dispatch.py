"""CPU test of the launches of a layer call with bfloat16 parameters (the recorder technique of tests/test_layer_dispatch.py): bf16 weights
launch only the _bf16 entries, or _f32 entries on fp32 buffers where the bf16 path runs in fp32 (the small path on the upcast operands, the
project-first recursion on the fp32 projection, the adjoint hops, the fp32 fold and re-layout of the weight).  Parameters of any other dtype,
a weight and a bias of two dtypes, and the parts of the API the bf16 path leaves out raise TgcnError with nothing launched."""
import contextlib

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F

from test_layer_dispatch import N_V, _op, _small, recorder  # noqa: F401  (the recorder fixture)

BF = torch.bfloat16
F32_ON_FP32 = {"cheb_forward_small", "cheb_basis_small", "cheb_wgrad", "csr_hop2", "fold_weight", "weight_layout", "cheb_project",
               "pack_rows"}


def _run(kind, q, C, N, K, mode, small, train, recorder, bias_kind=F.BIAS_CHANNEL, wdt=BF, bdt=BF):
    rec = recorder(_small(small))
    op = _op(kind)
    torch.manual_seed(0)
    x = torch.randn(q, N_V, C)
    W = torch.randn(K, C, N).to(wdt)
    bias = (torch.randn(N_V, N) if bias_kind == F.BIAS_VERTEX_CHANNEL else torch.randn(N)).to(bdt)
    for t in (x, W, bias):
        t.requires_grad_(train)
    with (contextlib.nullcontext() if train else torch.no_grad()):
        out = F.cheb_layer(op, x, W, bias, bias_kind, mode)
    if train:
        out.backward(torch.ones_like(out))
        assert W.grad.dtype == wdt and bias.grad.dtype == bdt
    return rec.calls, out


def _entries(calls):
    return [c.split()[0] for c in calls]


CASES = {
    # id: (operand, q, C, N, K, mode, small tiles, expected path)
    "small-power": ("plain", 2, 8, 8, 5, 0, [("cheb_forward_small", 8), ("cheb_basis_small", 8), ("cheb_forward_small", 8)], "small"),
    "pf-cheb": ("plain", 2, 64, 16, 3, 1, [], "project_first"),
    "pf-power": ("plain", 2, 64, 16, 5, 0, [], "project_first"),
    "hops-power": ("plain", 2, 32, 32, 5, 0, [], "hops"),
    "hops-cheb-compactable": ("compact", 2, 32, 32, 3, 1, [], "hops"),
    "hops-reordered": ("reordered", 2, 32, 32, 3, 1, [], "hops"),
}


@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("name", list(CASES))
def test_bf16_layer_launches_bf16_entries(name, train, recorder):
    kind, q, C, N, K, mode, small, path = CASES[name]
    calls, out = _run(kind, q, C, N, K, mode, small, train, recorder)
    assert out.dtype == BF and tuple(out.shape) == (q, N_V, N)
    ent = _entries(calls)
    assert ent, "nothing launched"
    for e in ent:
        assert e.endswith("_bf16") or e in F32_ON_FP32, e
    bf16 = [e for e in ent if e.endswith("_bf16")]
    if path == "small":
        assert not bf16 and ent[0] == "cheb_forward_small"
    elif path == "project_first":
        # one bf16 projection (fp32 Z), the fp32 recursion on it, no bf16 hop in the forward
        fwd = ent[: ent.index("cheb_project_bf16") + K]
        assert fwd.count("cheb_project_bf16") == 1 and "csr_hop2_bf16" not in fwd
        if train:
            assert "cheb_wgrad_bf16" in ent and "cheb_wgrad" not in ent
    else:
        assert ent.count("csr_hop2_bf16") >= K - 1 and "cheb_project_bf16" in ent and "cheb_compact_layer" not in ent
        assert "cheb_forward" not in ent and "cheb_forward_pf" not in ent
        if train:
            assert "cheb_wgrad_bf16" in ent and "cheb_wgrad" not in ent
            assert ent.count("csr_hop2_bf16") == K - 1          # the forward's basis is kept for the weight gradient


def test_bf16_hops_recompute_the_basis_over_the_keep_limit(recorder, monkeypatch):
    monkeypatch.setattr(F, "KEEP_BASIS_BYTES", 0)
    calls, _ = _run("plain", 2, 32, 32, 5, 0, [], True, recorder)
    assert _entries(calls).count("csr_hop2_bf16") == 2 * 4


def test_fp32_launches_are_unchanged_by_the_guard(recorder):
    """the fp32 path through the new dtype guard: the same sequence tests/test_layer_dispatch.py pins"""
    from test_layer_dispatch import EXPECTED
    calls, out = _run("plain", 2, 64, 16, 3, 1, [], True, recorder, wdt=torch.float32, bdt=torch.float32)
    assert out.dtype == torch.float32
    assert calls == EXPECTED["project-first-K3-cheb/training"]


@pytest.mark.parametrize("wdt,bdt", [(torch.float16, torch.float16), (torch.float64, torch.float64), (BF, torch.float32),
                                     (torch.float32, BF), (torch.float32, torch.float64)])
def test_other_parameter_dtypes_raise_before_any_launch(wdt, bdt, recorder):
    with pytest.raises(_lib.TgcnError):
        _run("plain", 2, 32, 32, 3, 0, [], False, recorder, wdt=wdt, bdt=bdt)
    assert _lib.lib().calls == []


@pytest.mark.parametrize("cls", ["TGCNCheb", "TGCNCheb_H", "GCNCheb", "ChebConv", "ChebTimeConv"])
@pytest.mark.parametrize("dt", [torch.float16, torch.float64])
def test_modules_refuse_other_dtypes_before_building_the_operand(cls, dt, recorder):
    rec = recorder({})
    L = torch.eye(8)
    m = {"TGCNCheb": lambda: tgcn_amd.TGCNCheb(L, 2, 3, 3), "TGCNCheb_H": lambda: tgcn_amd.TGCNCheb_H(L, 2, 3, 3, 4),
         "GCNCheb": lambda: tgcn_amd.GCNCheb(L, 2, 3, 3), "ChebConv": lambda: tgcn_amd.ChebConv(2, 3, 3),
         "ChebTimeConv": lambda: tgcn_amd.ChebTimeConv(2, 3, 3, 4)}[cls]().to(dt)
    x = torch.randn(2, 8, 4, 2) if cls.endswith("_H") or cls == "ChebTimeConv" else torch.randn(2, 8, 2)
    graph = (torch.tensor([[0, 1], [1, 0]]),) if cls.startswith("Cheb") else ()
    with pytest.raises(_lib.TgcnError):
        m(x, *graph)
    assert rec.calls == []


def test_out_of_scope_entries_raise_with_bf16(recorder):
    rec = recorder({})
    L = torch.eye(8)
    h = tgcn_amd.TGCNCheb_H(L, 1, 3, 3, 4).to(BF)
    with pytest.raises(_lib.TgcnError):
        h.forward_series(torch.randn(2, 8, 10))
    with pytest.raises(_lib.TgcnError):
        tgcn_amd.nn.cheb_relu_pool(tgcn_amd.TGCNCheb(L, 2, 3, 3).to(BF), torch.randn(2, 8, 2))
    op = _op("plain")
    with pytest.raises(_lib.TgcnError):
        F.cheb_relu_pool(op, torch.randn(2, N_V, 8), torch.randn(3, 8, 8).to(BF), None, F.BIAS_NONE, 0, 4)
    conv = tgcn_amd.ChebConv(2, 3, 3).to(BF)
    ew = torch.ones(2, requires_grad=True)
    with pytest.raises(_lib.TgcnError):
        conv(torch.randn(2, 8, 2), torch.tensor([[0, 1], [1, 0]]), ew)
    with pytest.raises(_lib.TgcnError):
        F.cheb_layer(op, torch.randn(2, N_V, 8), torch.randn(3, 8, 8).to(BF), None, F.BIAS_NONE, 1, values=torch.randn(op.nnz))
    assert rec.calls == []


def test_sharded_modules_refuse_bf16(recorder):
    from tgcn_amd import dist
    rec = recorder({})
    m = dist.ShardedGCNCheb(torch.eye(8), 2, 3, 3).to(BF)
    with pytest.raises(_lib.TgcnError):
        m(torch.randn(2, 8, 2))
    with pytest.raises(_lib.TgcnError):
        m.shard("cpu")
    assert rec.calls == []
