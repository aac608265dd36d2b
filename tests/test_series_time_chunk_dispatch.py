"""CPU test of the launches of forward_series / F.cheb_time_windows with time_chunk=, by the recorder technique of tests/test_layer_dispatch.py.
Without the keyword, or with time_chunk=None, a call makes exactly the calls it makes today.  A chunked forward asks the step-1 plan once and
first, then per chunk runs K - 1 hops on rows of Tc*f floats and ONE tgcn_cheb_project_series_stream_at_f32 call with the chunk's place in the
whole output and a head that follows (head + Tc) mod C; the backward walks the chunks in the same order: the hops again, ONE
tgcn_cheb_series_chunk_backward_f32 call with the chunk's place in the whole gradient and the same heads, the adjoint hops.  The one-sided
backwards pass null pointers and skip what they do not need; every refusal raises TgcnError with nothing launched and no operand built."""
import ctypes
import os

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F
from tgcn_amd.graph import GraphOperand

from test_layer_dispatch import N_V, _Op, _op, recorder  # noqa: F401  (the recorder fixture)

AT, CB, HOP = "cheb_project_series_stream_at", "cheb_series_chunk_backward", "csr_hop2"
# positions of the pointer arguments of tgcn_cheb_series_chunk_backward_f32 (the stream, position 0, is null in the recorder's world)
P_STACK, P_RING, P_G, P_W, P_GOUT, P_DW, P_WS = 8, 9, 12, 16, 17, 18, 19


def _entries(calls):
    return [c.split()[0] for c in calls]


def _stub_operands(monkeypatch):
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda *a, **k: _Op(N_V, 256)))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: _Op(N_V, 256)))


def _no_operands(monkeypatch):
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda *a, **k: pytest.fail("operand built")))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: pytest.fail("operand built")))


def _chunks(T, Tc):
    return [(t0, min(Tc, T - t0)) for t0 in range(0, T, Tc)]


def test_without_the_keyword_the_calls_are_todays(recorder, monkeypatch):
    """both classes, a default and a causal dilated geometry: time_chunk=None is the call without the keyword, forward and backward"""
    rec = recorder({})
    _stub_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    for layer, extra in ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3), ()), (tgcn_amd.ChebTimeConv(4, 8, 3, 3), (ei,))):
        for geo in (dict(), dict(padding="causal", as_series=True, dilation=2)):
            lists = []
            for kw in (dict(), dict(time_chunk=None)):
                torch.manual_seed(1)
                series = torch.randn(2, N_V, 12, 4, requires_grad=True)
                del rec.calls[:]
                out = layer.forward_series(series, *extra, **geo, **kw)
                out.backward(torch.ones_like(out))
                lists.append(list(rec.calls))
            assert lists[0] == lists[1] and lists[0], geo
            assert not any(e in (AT, CB) for e in _entries(lists[0]))
    # and the functional entry
    W = torch.randn(3, 3, 4, 8)
    lists = []
    for kw in (dict(), dict(time_chunk=None)):
        del rec.calls[:]
        F.cheb_time_windows(_op("plain"), torch.randn(2, N_V, 12, 4), W, None, F.BIAS_NONE, 1, padding="causal", dilation=2, **kw)
        lists.append(list(rec.calls))
    assert lists[0] == lists[1] and lists[0]


@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
@pytest.mark.parametrize("mode", [0, 1], ids=["power", "chebyshev"])
def test_a_chunked_call_logs_plan_hops_and_one_entry_per_chunk_in_both_directions(mode, as_series, recorder):
    rec = recorder({})
    S, T, f, H, N, K, d, Tc = 2, 23, 4, 4, 8, 3, 2, 5
    Cr = (H - 1) * d
    op = _op("plain")
    torch.manual_seed(0)
    series = torch.randn(S, N_V, T, f, requires_grad=True)
    W, bias = torch.randn(K, H, f, N, requires_grad=True), torch.randn(N, requires_grad=True)
    out = F.cheb_time_windows(op, series, W, bias, F.BIAS_CHANNEL, mode, as_series=as_series, padding="causal", dilation=d, time_chunk=Tc)
    assert tuple(out.shape) == ((S, N_V, T, N) if as_series else (S * T, N_V, N)) and out.is_contiguous() and out.requires_grad
    calls, ent = list(rec.calls), _entries(rec.calls)
    # the step-1 plan first and once: H f N vec 1
    assert calls[0] == "series_conv_plan %d %d %d 1 1" % (H, f, N) and ent.count("series_conv_plan") == 1
    assert ent.count("fold_weight") == (1 if mode == 0 else 0) and ent.index(AT) > (1 if mode == 0 else 0)
    assert set(ent) <= {"series_conv_plan", "fold_weight", HOP, AT}, ent
    # per chunk: K - 1 hops on rows of Tc*f, then the _at entry
    per_chunk = [c for c in calls if c.split()[0] in (HOP, AT)]
    head, i = 0, 0
    for t0, tc in _chunks(T, Tc):
        hops, at = per_chunk[i:i + K - 1], per_chunk[i + K - 1]
        i += K
        assert all(c.split()[:3] == [HOP, str(S), str(tc * f)] for c in hops), (t0, hops)
        # S n Tc f H N K bias_kind out_T out_t0 out_as_series ring_ld head dilation
        assert at == "%s %d %d %d %d %d %d %d 1 %d %d %d %d %d %d" % (AT, S, N_V, tc, f, H, N, K, T, t0, int(as_series), Cr * f, head, d), (t0, at)
        head = (head + tc) % Cr
    assert i == len(per_chunk) and _chunks(T, Tc)[-1] == (20, 3)        # a short tail

    del rec.calls[:], rec.nulls[:]
    out.backward(torch.ones_like(out))
    calls, ent = list(rec.calls), _entries(rec.calls)
    assert set(ent) <= {"fold_weight", HOP, CB}, ent
    assert ent.count("fold_weight") == (1 if mode == 0 else 0) and (mode == 1 or ent[-1] == "fold_weight")      # the sum un-folded once, last
    per_chunk = [(c, nl) for c, nl in zip(calls, rec.nulls) if c.split()[0] in (HOP, CB)]
    head, i = 0, 0
    for t0, tc in _chunks(T, Tc):
        rehops, (cb, nulls), adj = per_chunk[i:i + K - 1], per_chunk[i + K - 1], per_chunk[i + K:i + 2 * K - 1]
        i += 2 * K - 1
        assert all(c.split()[:3] == [HOP, str(S), str(tc * f)] for c, _ in rehops + adj), t0
        # S n Tc f H N K ring_ld head g_T g_t0 g_as_series workspace_bytes dilation
        assert cb == "%s %d %d %d %d %d %d %d %d %d %d %d %d 1024 %d" % (CB, S, N_V, tc, f, H, N, K, Cr * f, head, T, t0, int(as_series), d), (t0, cb)
        assert not set(nulls) & {P_STACK, P_RING, P_G, P_W, P_GOUT, P_DW, P_WS}, nulls
        head = (head + tc) % Cr
    assert i == len(per_chunk)
    assert tuple(series.grad.shape) == (S, N_V, T, f) and tuple(W.grad.shape) == (K, H, f, N) and tuple(bias.grad.shape) == (N,)


def test_one_chunk_and_three_dimensional_series_on_both_classes(recorder, monkeypatch):
    """Tc >= T is one chunk on the chunked path; a single channel runs the general kernels with f = 1, never the scalar-load form; one tap
    keeps no ring: a null ring, ring_ld 0 and head 0"""
    rec = recorder({})
    _stub_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    T = 12
    for H, d in ((3, 2), (1, 5)):
        Cr = (H - 1) * (d if H > 1 else 1)
        for layer, extra in ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), 1, 8, 3, H), ()), (tgcn_amd.ChebTimeConv(1, 8, 3, H), (ei,))):
            for Tc in (T, 64):
                del rec.calls[:], rec.nulls[:]
                series = torch.randn(2, N_V, T, requires_grad=True)
                out = layer.forward_series(series, *extra, padding="causal", dilation=d, time_chunk=Tc)
                assert tuple(out.shape) == (2 * T, N_V, 8)
                ent = _entries(rec.calls)
                assert ent.count(AT) == 1 and "cheb_project_windows" not in ent and not any("series_conv" in e and e != "series_conv_plan" for e in ent)
                at = rec.calls[ent.index(AT)].split()
                assert at[1:8] == [str(v) for v in (2, N_V, T, 1, H, 8, 3)] and at[9:] == [str(v) for v in (T, 0, 0, Cr, 0, d if H > 1 else 1)]
                ring_null = 16 in rec.nulls[ent.index(AT)]
                assert ring_null == (H == 1)
                del rec.calls[:], rec.nulls[:]
                out.backward(torch.ones_like(out))
                ent = _entries(rec.calls)
                assert ent.count(CB) == 1
                cb = rec.calls[ent.index(CB)].split()
                assert cb[3] == str(T) and cb[8:13] == [str(v) for v in (Cr, 0, T, 0, 0)]
                assert (P_RING in rec.nulls[ent.index(CB)]) == (H == 1)
                assert tuple(series.grad.shape) == (2, N_V, T)


def test_the_one_sided_backwards_pass_null_pointers_and_skip_their_hops(recorder):
    rec = recorder({})
    S, T, f, H, N, K, d, Tc = 2, 11, 4, 3, 8, 3, 1, 4
    op = _op("plain")
    nchunks = len(_chunks(T, Tc))
    # a frozen weight: no second hop pass, no ring, no dW -- G and the adjoint hops only
    series, W = torch.randn(S, N_V, T, f, requires_grad=True), torch.randn(K, H, f, N)
    out = F.cheb_time_windows(op, series, W, None, F.BIAS_NONE, 1, as_series=True, padding="causal", dilation=d, time_chunk=Tc)
    del rec.calls[:], rec.nulls[:]
    out.backward(torch.ones_like(out))
    ent = _entries(rec.calls)
    assert ent.count(CB) == nchunks and ent.count(HOP) == nchunks * (K - 1) and set(ent) == {HOP, CB}
    for c, nulls in zip(rec.calls, rec.nulls):
        if c.split()[0] == CB:
            assert {P_STACK, P_RING, P_DW} <= set(nulls) and not set(nulls) & {P_G, P_W, P_GOUT, P_WS}
            assert c.split()[8:10] == ["0", "0"]                         # no ring: ring_ld and head unused
    assert ent[0] == CB                                                  # nothing is hopped before the first chunk's G
    # a series without grad: no G, no adjoint hops -- the hops again, the ring and dW
    series, W = torch.randn(S, N_V, T, f), torch.randn(K, H, f, N, requires_grad=True)
    out = F.cheb_time_windows(op, series, W, None, F.BIAS_NONE, 1, as_series=False, padding="causal", dilation=d, time_chunk=Tc)
    del rec.calls[:], rec.nulls[:]
    out.backward(torch.ones_like(out))
    ent = _entries(rec.calls)
    assert ent.count(CB) == nchunks and ent.count(HOP) == nchunks * (K - 1) and set(ent) == {HOP, CB}
    heads = []
    for c, nulls in zip(rec.calls, rec.nulls):
        if c.split()[0] == CB:
            assert {P_W, P_GOUT} <= set(nulls) and not set(nulls) & {P_STACK, P_RING, P_G, P_DW, P_WS}
            heads.append(int(c.split()[9]))
    assert heads == [0, 0, 0] and ent[-1] == CB                          # C = 2, chunks of 4: the head returns to 0; no hop after the last dW
    # only the bias trains: no library call at all in the backward
    series, W, bias = torch.randn(S, N_V, T, f), torch.randn(K, H, f, N), torch.randn(N, requires_grad=True)
    out = F.cheb_time_windows(op, series, W, bias, F.BIAS_CHANNEL, 1, as_series=True, padding="causal", time_chunk=Tc)
    del rec.calls[:]
    out.backward(torch.ones_like(out))
    assert rec.calls == [] and tuple(bias.grad.shape) == (N,)


def test_a_reordered_operand_relabels_once_on_the_way_in_and_out(recorder):
    rec = recorder({})
    op = _op("reordered")
    series = torch.randn(2, N_V, 9, 4, requires_grad=True)
    out = F.cheb_time_windows(op, series, torch.randn(3, 3, 4, 8), None, F.BIAS_NONE, 1, as_series=True, padding="causal", time_chunk=4)
    ent = _entries(rec.calls)
    assert ent.count("pack_rows") == 2 and ent[0] == "pack_rows" and ent[-1] == "pack_rows" and ent.count(AT) == 3
    del rec.calls[:]
    out.backward(torch.ones_like(out))
    ent = _entries(rec.calls)
    assert ent.count("pack_rows") == 2 and ent[0] == "pack_rows" and ent[-1] == "pack_rows" and ent.count(CB) == 3


def test_every_refusal_comes_before_anything_is_built_or_launched(recorder, monkeypatch):
    rec = recorder({})
    _no_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    h, c = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3), tgcn_amd.ChebTimeConv(4, 8, 3, 3)
    series = torch.randn(2, N_V, 12, 4)
    op = _op("plain")

    def calls(**kw):
        return (lambda: h.forward_series(series, **kw), lambda: c.forward_series(series, ei, **kw),
                lambda: F.cheb_time_windows(op, series, h.weight, None, F.BIAS_NONE, 0, **kw))

    for bad in (0, -1, 2.0, True, "4", (4,)):
        for call in calls(padding="causal", time_chunk=bad):
            with pytest.raises(_lib.TgcnError, match="time_chunk is None or an integer >= 1"):
                call()
    for pad in (0, 1, (2, 0), (2, 1)):          # (2, 0) is the causal geometry spelt as a pair: the chunked path takes the word only
        for call in calls(padding=pad, time_chunk=4):
            with pytest.raises(_lib.TgcnError, match='padding="causal" only'):
                call()
    for call in calls(time_chunk=4):            # the default padding
        with pytest.raises(_lib.TgcnError, match='padding="causal" only'):
            call()
    for call in calls(padding="causal", stride=2, time_chunk=4):
        with pytest.raises(_lib.TgcnError, match="stride=1 only"):
            call()
    BF = torch.bfloat16
    hb, cb = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3).to(BF), tgcn_amd.ChebTimeConv(4, 8, 3, 3).to(BF)
    for call in (lambda: hb.forward_series(series.to(BF), padding="causal", time_chunk=4),
                 lambda: cb.forward_series(series.to(BF), ei, padding="causal", time_chunk=4),
                 lambda: F.cheb_time_windows(op, series.to(BF), hb.weight, None, F.BIAS_NONE, 0, padding="causal", time_chunk=4)):
        with pytest.raises(_lib.TgcnError, match="float32 only"):
            call()
    with pytest.raises(_lib.TgcnError, match="learnable edge weights"):
        c.forward_series(series, ei, torch.ones(2, requires_grad=True), padding="causal", time_chunk=4)
    # the refusals that were there before stay: a dilation with a step, a dilation that is no integer, streaming in grad mode
    with pytest.raises(_lib.TgcnError, match="not supported"):
        h.forward_series(series, padding="causal", stride=2, dilation=2, time_chunk=4)
    with pytest.raises(_lib.TgcnError, match="dilation is an integer >= 1"):
        h.forward_series(series, padding="causal", dilation=0, time_chunk=4)
    with pytest.raises(_lib.TgcnError, match=r"torch\.no_grad\(\)"):
        h.forward_stream(series)
    assert rec.calls == []


def test_the_new_entries_are_declared_everywhere():
    """the header, the ctypes table and the library agree on the entries; ABI 8; the scalar rules refuse before any pointer is read"""
    names = ["tgcn_cheb_project_series_stream_at_f32", "tgcn_cheb_series_chunk_backward_f32", "tgcn_cheb_series_chunk_backward_workspace_bytes"]
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "tgcn_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert nm in _lib.SIGNATURES and hasattr(handle, nm) and (" " + nm + "(") in header, nm
    L = _lib.lib()
    assert L.tgcn_abi_version() == 8 == _lib.ABI_VERSION
    INVALID = -1
    one = ctypes.c_void_p(16)       # a non-null pointer that the refused calls never read

    # S n Tc f H N K = 2 48 5 4 3 8 3, dilation 4: C = 8, ring_ld >= 32
    def at(Tc=5, H=3, out_T=23, out_t0=0, ring_ld=32, head=0, dil=4):
        return L.tgcn_cheb_project_series_stream_at_f32(None, 2, 48, Tc, 4, H, 8, 3, one, one, None, 0, one, out_T, out_t0, 1, one, ring_ld, head, dil)

    def cb(Tc=5, H=3, g_T=23, g_t0=0, ring_ld=32, head=0, dil=4, G=one, dW=one, stack=one, ring=one, W=one):
        return L.tgcn_cheb_series_chunk_backward_f32(None, 2, 48, Tc, 4, H, 8, 3, stack, ring, ring_ld, head, one, g_T, g_t0, 1, W, G, dW, one, 1 << 30, dil)

    for entry in (at, cb):
        assert entry(head=8) == INVALID and entry(head=-1) == INVALID and entry(ring_ld=31) == INVALID
        assert entry(Tc=0) == INVALID and entry(dil=0) == INVALID and entry(dil=2 ** 30) == INVALID and entry(H=0) == INVALID
    assert at(out_t0=19) == INVALID and at(out_t0=-1) == INVALID and at(out_T=0) == INVALID and at(out_T=4) == INVALID
    assert cb(g_t0=19) == INVALID and cb(g_t0=-1) == INVALID and cb(g_T=0) == INVALID
    assert cb(G=None, dW=None) == INVALID                               # nothing asked for
    assert cb(W=None) == INVALID and cb(stack=None) == INVALID          # G needs W, dW the stack
    assert cb(ring=None) == INVALID                                     # ... and, with more than one tap, the ring
    assert cb(G=None, dW=None, H=1) == INVALID
    need = L.tgcn_cheb_series_chunk_backward_workspace_bytes
    assert need(2, 48, 5, 4, 3, 8, 3, 4) >= 3 * 3 * 4 * 8 * 4 and need(2, 48, 0, 4, 3, 8, 3, 4) == 0 and need(2, 48, 5, 4, 3, 8, 3, 0) == 0
    assert need(2, 48, 5, 4, 1, 8, 3, 7) > 0                            # one tap: any dilation >= 1 is dilation 1
