"""CPU test of the launches of a bfloat16 reference-power layer on an operand with a compact plan (the recorder of
tests/test_layer_dispatch.py): K-1 bf16 hops on the compact operands and two row-mapped bf16 projections (kept rows, left-out rows) instead of
full-size hops and tgcn_cheb_project_bf16; the weight gradient from the compact terms and the gathered kept rows of g; the passes of a forward
that does not fit the workspace share; and everything that must NOT change: mode 1, the switches off, the input gradient's launches."""
import contextlib
import os

import torch

from tgcn_amd import _lib
from tgcn_amd import functional as F

from test_layer_dispatch import N_V, _op, _small, recorder  # noqa: F401  (the recorder fixture)

BF = torch.bfloat16
Q, C_ROW, N_OUT, K = 2, 32, 32, 5          # the shape of test_bf16_dispatch's "hops-power"
N_C, N_EMPTY = 40, 24                      # _op("compact")'s "rows" plan


def _run(recorder, kind, train, mode=0, K=K, bias_kind=F.BIAS_CHANNEL):
    rec = recorder(_small([]))
    op = _op(kind)
    torch.manual_seed(0)
    x = torch.randn(Q, N_V, C_ROW)
    W = torch.randn(K, C_ROW, N_OUT).to(BF)
    bias = (torch.randn(N_V, N_OUT) if bias_kind == F.BIAS_VERTEX_CHANNEL else torch.randn(N_OUT)).to(BF)
    for t in (x, W, bias):
        t.requires_grad_(train)
    with (contextlib.nullcontext() if train else torch.no_grad()):
        out = F.cheb_layer(op, x, W, bias, bias_kind, mode)
    assert out.dtype == BF and tuple(out.shape) == (Q, N_V, N_OUT)
    if train:
        out.backward(torch.ones_like(out))
        assert W.grad.dtype == BF and tuple(W.grad.shape) == (K, C_ROW, N_OUT) and x.grad.shape == x.shape
    return rec.calls


def _entries(calls):
    return [c.split()[0] for c in calls]


def _args(call):
    return call.split()[1:]


def _dx(calls):
    """the launches of the input gradient: everything after the transposed fold of the weight gradient"""
    last = max(i for i, c in enumerate(calls) if c.startswith("fold_weight ") and c.split()[-1] == "1")
    return calls[last + 1:]


def test_inference_runs_compact_hops_and_two_mapped_projections(recorder, monkeypatch):
    monkeypatch.setattr(F, "COMPACT_BF16", True)
    calls = _run(recorder, "compact", False)
    ent = _entries(calls)
    assert ent == ["fold_weight"] + ["csr_hop2_bf16"] * (K - 1) + ["cheb_project_mapped_bf16"] * 2
    proj = [c for c in calls if c.startswith("cheb_project_mapped_bf16 ")]
    # scalars: M Kc N nterms bias_kind bias_dtype n_vertices mapped_terms nbatch out_bs ldo out_dtype
    assert _args(proj[0]) == [str(v) for v in (N_C, C_ROW, N_OUT, K, 1, 1, N_V, 1, Q, N_V * N_OUT, N_OUT, 1)]
    assert _args(proj[1]) == [str(v) for v in (N_EMPTY, C_ROW, N_OUT, 1, 1, 1, N_V, 1, Q, N_V * N_OUT, N_OUT, 1)]
    for e in ("cheb_project_bf16", "cheb_compact_layer", "csr_hop2", "csr_hop", "cheb_project", "cheb_project_mapped"):
        assert e not in ent, e
    # every hop carries all samples of the one pass
    assert all(_args(c)[0] == str(Q) for c in calls if c.startswith("csr_hop2_bf16 "))


def test_training_keeps_the_compact_basis(recorder, monkeypatch):
    monkeypatch.setattr(F, "COMPACT_BF16", True)
    calls = _run(recorder, "compact", True)
    ent = _entries(calls)
    assert ent.count("csr_hop2_bf16") == K - 1
    assert ent.count("cheb_project_mapped_bf16") == 2 and "cheb_project_bf16" in ent      # (the latter: G = g W^T of the input gradient)
    assert ent.count("pack_rows_bf16") == Q and ent.count("cheb_wgrad_bf16") == 2 and "cheb_wgrad" not in ent
    wg = [c for c in calls if c.startswith("cheb_wgrad_bf16 ")]
    assert _args(wg[0])[:4] == [str(Q * N_V), str(C_ROW), str(N_OUT), "1"]                     # x^T g over every vertex
    assert _args(wg[1])[:4] == [str(Q * (N_C + 1)), str(C_ROW), str(N_OUT), str(K - 1)]       # compact terms against the gathered rows of g
    pk = [c for c in calls if c.startswith("pack_rows_bf16 ")]
    assert all(_args(c) == [str(N_OUT), str(N_C), str(N_OUT)] for c in pk)
    assert "cheb_compact_layer" not in ent and "pack_rows" not in ent
    # the input gradient is untouched: the launches of today's hops path
    monkeypatch.setattr(F, "COMPACT_BF16", False)
    plain = _run(recorder, "compact", True)
    assert _dx(calls) == _dx(plain) and len(_dx(plain)) == 3 + K - 1
    assert _entries(_dx(plain)) == ["fold_weight", "weight_layout", "cheb_project_bf16"] + ["csr_hop2"] * (K - 1)
    assert _dx(calls) == _dx(_run(recorder, "plain", True))


def test_over_the_keep_limit_the_compact_hops_run_again(recorder, monkeypatch):
    monkeypatch.setattr(F, "COMPACT_BF16", True)
    monkeypatch.setattr(F, "KEEP_BASIS_BYTES", 0)
    ent = _entries(_run(recorder, "compact", True))
    assert ent.count("csr_hop2_bf16") == 2 * (K - 1)
    assert ent.count("cheb_project_mapped_bf16") == 2 and ent.count("cheb_wgrad_bf16") == 2 and ent.count("pack_rows_bf16") == Q


def test_switches_off_give_the_uncompacted_sequence(recorder, monkeypatch):
    monkeypatch.setattr(F, "COMPACT_BF16", True)
    for train in (False, True):
        want = _run(recorder, "plain", train)           # test_bf16_dispatch's "hops-power": an operand without a plan
        assert "cheb_project_bf16" in _entries(want) and "cheb_project_mapped_bf16" not in _entries(want)
        for switch in ("COMPACT", "COMPACT_BF16"):
            with monkeypatch.context() as m:
                m.setattr(F, switch, False)
                assert _run(recorder, "compact", train) == want, (switch, train)


def test_chebyshev_recurrence_is_not_compacted(recorder, monkeypatch):
    monkeypatch.setattr(F, "COMPACT_BF16", True)
    for train in (False, True):
        got = _run(recorder, "compact", train, mode=1, K=3)
        assert got == _run(recorder, "plain", train, mode=1, K=3)
        assert "cheb_project_mapped_bf16" not in _entries(got) and _entries(got).count("csr_hop2_bf16") == 2


def test_a_small_budget_runs_two_passes(recorder, monkeypatch):
    monkeypatch.setattr(F, "COMPACT_BF16", True)
    rec_factory = recorder

    def small_budget(small):
        rec = rec_factory(small)
        # one sample's K-1 compact terms, and a half: one sample per pass
        per_q = (K - 1) * (N_C + 1) * C_ROW * 2
        monkeypatch.setattr(torch.cuda, "mem_get_info", lambda d=None: (int(1.5 * per_q / F.COMPACT_WS_FRACTION), 1 << 35))
        return rec
    calls = _run(small_budget, "compact", False, bias_kind=F.BIAS_VERTEX_CHANNEL)
    ent = _entries(calls)
    one_pass = ["csr_hop2_bf16"] * (K - 1) + ["cheb_project_mapped_bf16"] * 2
    assert ent == ["fold_weight"] + one_pass * 2
    assert all(_args(c)[0] == "1" for c in calls if c.startswith("csr_hop2_bf16 "))                  # nb
    assert all(_args(c)[8] == "1" for c in calls if c.startswith("cheb_project_mapped_bf16 "))       # nbatch
    # the choice is cached on the plan under a key of its own: no second query, no collision with the fp32 layer's (K, C, q)
    op = _op("compact")
    plan = op.plans["rows"]
    F._compact_q_chunk_bf16(plan, Q, K, C_ROW, torch.device("cpu"))
    assert list(plan.q_chunk_cache) == [("bf16", K, C_ROW, Q)]
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda d=None: (_ for _ in ()).throw(AssertionError("asked twice")))
    assert F._compact_q_chunk_bf16(plan, Q, K, C_ROW, torch.device("cpu")) == 1


def test_entries_and_abi():
    names = ("tgcn_cheb_project_mapped_bf16", "tgcn_pack_rows_bf16")
    header = open(os.path.join(_lib.INCLUDE, "tgcn_hip.h")).read()
    L = _lib.lib()
    for nm in names:
        assert nm in _lib.SIGNATURES, nm
        assert ("int %s(" % nm) in header, nm
        assert hasattr(L, nm), nm
    assert L.tgcn_abi_version() == 8 == _lib.ABI_VERSION and "#define TGCN_ABI_VERSION 8" in header
    assert F.COMPACT_BF16 in (True, False)
