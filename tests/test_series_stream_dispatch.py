"""CPU test of the launches of the streaming-state calls (forward_stream / F.cheb_time_stream), by the recorder technique of
tests/test_layer_dispatch.py: a call asks the step-1 plan once and first, runs K - 1 hops on the chunk's rows and launches the stream entry
with the ring's scalars; head follows (head + Tc) mod C over a sequence of chunks and seen adds up; state.reset() returns both to 0; a
one-tap layer keeps no ring and launches the _conv entry; every refusal raises TgcnError with nothing launched and no operand built; and the
existing streaming calls make exactly the calls they made before, whether a stream call came first or not."""
import ctypes
import os

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F
from tgcn_amd.graph import GraphOperand

from test_layer_dispatch import N_V, T_WIN, _Op, _op, recorder  # noqa: F401  (the recorder fixture)

BF = torch.bfloat16


def _entries(calls):
    return [c.split()[0] for c in calls]


def _stub_operands(monkeypatch):
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda *a, **k: _Op(N_V, 256)))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: _Op(N_V, 256)))


def _no_operands(monkeypatch):
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda *a, **k: pytest.fail("operand built")))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: pytest.fail("operand built")))


def _stream(rec, op, chunk, W, bias, mode, state, dilation):
    del rec.calls[:]
    with torch.no_grad():
        out, state = F.cheb_time_stream(op, chunk, W, bias, F.BIAS_NONE if bias is None else F.BIAS_CHANNEL, mode, state, dilation)
    return out, state, list(rec.calls)


@pytest.mark.parametrize("mode", [0, 1], ids=["power", "chebyshev"])
@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
def test_a_stream_call_logs_plan_hops_and_the_stream_entry(dt, mode, recorder):
    rec = recorder({})
    S, f, H, N, K, d = 3, 8, 3, 8, 3, 4
    Cr = (H - 1) * d
    bf16 = dt == BF
    torch.manual_seed(0)
    W, bias, op = torch.randn(K, H, f, N).to(dt), torch.randn(N).to(dt), _op("plain")
    state, head, seen = None, 0, 0
    for i, Tc in enumerate([1, 1, 3, 8, 9, 40, 5]):
        out, state, calls = _stream(rec, op, torch.randn(S, N_V, Tc, f).to(dt), W, bias, mode, state, d)
        assert tuple(out.shape) == (S, N_V, Tc, N) and out.dtype == dt and out.is_contiguous()
        ent = _entries(calls)
        plan, hop, entry = (("series_conv_plan_bf16", "csr_hop2_bf16", "cheb_project_series_stream_bf16") if bf16
                            else ("series_conv_plan", "csr_hop2", "cheb_project_series_stream"))
        # the step-1 plan first and once: H f N vec 1
        assert calls[0] == "%s %d %d %d 1 1" % (plan, H, f, N) and ent.count(plan) == 1
        # K - 1 hops on rows of Tc*f elements (f = 8: no trailing padding in bf16 either), all before the entry
        hops = [c for c in calls if c.split()[0] == hop]
        assert len(hops) == K - 1 and all(c.split()[1:3] == [str(S), str(Tc * f)] for c in hops)
        assert ent.index(entry) == len(ent) - 1 and ent.count(entry) == 1
        # scalars: S n Tc f H N K [stack_ld bias_dtype] bias_kind ring_ld head dilation
        mid = "%d 1 1" % (Tc * f) if bf16 else "1"
        assert calls[-1] == "%s %d %d %d %d %d %d %d %s %d %d %d" % (entry, S, N_V, Tc, f, H, N, K, mid, Cr * f, head, d)
        # the weight is folded to the kernels' basis on every call, as forward_series does: the state keeps nothing of the weight
        assert ent.count("fold_weight") == (1 if mode == 0 else 0)
        assert set(ent) <= {plan, hop, entry, "fold_weight"}, ent
        head, seen = (head + Tc) % Cr, seen + Tc
        assert (state.head, state.seen, state.dilation, state.C) == (head, seen, d, Cr)
    assert isinstance(state, F.SeriesStreamState) and tuple(state.ring.shape) == (K, S, N_V, Cr * f) and state.ring.dtype == dt
    assert (state.S, state.n, state.f, state.K, state.H, state.dtype, state.op) == (S, N_V, f, K, H, dt, op)
    assert head != 0 and state.reset() is state and (state.head, state.seen) == (0, 0) and not state.ring.any()
    out, state2, calls = _stream(rec, op, torch.randn(S, N_V, 2, f).to(dt), W, bias, mode, state, d)
    assert state2 is state and calls[-1].split()[-2:] == ["0", str(d)] and (state.head, state.seen) == (2, 2)


def test_bf16_rows_that_are_no_multiple_of_eight_are_padded_by_trailing_elements(recorder):
    rec = recorder({})
    out, state, calls = _stream(rec, _op("plain"), torch.randn(2, N_V, 3, 4).to(BF), torch.randn(3, 2, 4, 8).to(BF), None, 1, None, 1)
    # Tc*f = 12 -> rows of 16 elements (stack_ld), a time row stays 4 contiguous elements; f % 8 != 0: the narrow plan
    assert calls[0] == "series_conv_plan_bf16 2 4 8 0 1"
    assert [c.split()[1:3] for c in calls if c.startswith("csr_hop2_bf16 ")] == [["2", "16"]] * 2
    assert calls[-1] == "cheb_project_series_stream_bf16 2 %d 3 4 2 8 3 16 1 0 4 0 1" % N_V


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
def test_both_classes_and_three_dimensional_chunks(dt, recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    sfx = "_bf16" if dt == BF else ""
    for f in (1, 4):
        for layer, extra in ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), f, 8, 3, 3).to(dt), ()), (tgcn_amd.ChebTimeConv(f, 8, 3, 3).to(dt), (ei,))):
            state, head = None, 0
            for Tc in (5, 2, 7):
                chunk = torch.randn(2, N_V, Tc, f).to(dt)
                if f == 1:
                    chunk = chunk[..., 0]       # (S, n, Tc): the single channel
                del rec.calls[:]
                with torch.no_grad():
                    out, state = layer.forward_stream(chunk, *extra, state=state, dilation=2)
                assert tuple(out.shape) == (2, N_V, Tc, 8) and out.dtype == dt
                ent = _entries(rec.calls)
                # a single channel runs the general kernels: the stream entry with f = 1, never the scalar-load form
                assert ent.count("cheb_project_series_stream" + sfx) == 1 and "cheb_project_windows" not in ent
                sc = rec.calls[-1].split()
                assert sc[1:8] == [str(v) for v in (2, N_V, Tc, f, 3, 8, 3)] and sc[-3:] == [str(4 * f), str(head), "2"]
                head = (head + Tc) % 4
            assert state.seen == 14 and state.head == head


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
def test_a_reordered_operand_relabels_the_chunk_in_and_the_output_out(dt, recorder):
    rec = recorder({})
    op = _op("reordered")
    out, state, calls = _stream(rec, op, torch.randn(2, N_V, 5, 4).to(dt), torch.randn(3, 3, 4, 8).to(dt), torch.randn(8).to(dt), 1, None, 1)
    ent = _entries(calls)
    assert ent.count("pack_rows") == 2 and ent[0] == "pack_rows" and ent[-1] == "pack_rows"          # (a per-channel bias has no vertex axis)
    assert out.dtype == dt and tuple(out.shape) == (2, N_V, 5, 8) and state.op is op


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
def test_one_tap_keeps_no_ring_and_launches_the_conv_entry(dt, recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    sfx = "_bf16" if dt == BF else ""
    layer = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 8, 8, 3, 1).to(dt)
    state = None
    for Tc, dil in ((4, 1), (1, 7), (9, 2 ** 30)):          # one tap has nothing to dilate: any dilation >= 1 is dilation 1
        del rec.calls[:]
        with torch.no_grad():
            out, state = layer.forward_stream(torch.randn(2, N_V, Tc, 8).to(dt), state=state, dilation=dil)
        ent = _entries(rec.calls)
        assert not any("stream" in e for e in ent) and ent.count("cheb_project_series_conv" + sfx) == 1
        # the _conv entry on the chunk: as_series = 1, stride 1, no pads
        assert rec.calls[-1].split()[-4:] == ["1", "1", "0", "0"] and rec.calls[-1].split()[1:4] == ["2", str(N_V), str(Tc)]
        assert tuple(out.shape) == (2, N_V, Tc, 8)
    assert state.ring is None and (state.C, state.head, state.seen, state.dilation) == (0, 0, 14, 1)
    assert state.reset().seen == 0


def test_every_refusal_comes_before_anything_is_built_or_launched(recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    h, c = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3), tgcn_amd.ChebTimeConv(4, 8, 3, 3)
    h2 = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3)
    chunk = torch.randn(2, N_V, 5, 4)
    with torch.no_grad():           # states to offer to the wrong calls, and every operand cached
        _, s_h = h.forward_stream(chunk, dilation=2)
        _, s_c = c.forward_stream(chunk, ei, dilation=2)
        _, s_h2 = h2.forward_stream(chunk, dilation=2)
        _, s_bf = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3).to(BF).forward_stream(chunk.to(BF), dilation=2)
    before = (s_h.head, s_h.seen, s_h.ring.clone())
    del rec.calls[:]
    _no_operands(monkeypatch)
    NOGRAD, MADE = r"torch\.no_grad\(\)", "the state was made for"
    # grad mode with a parameter (or the chunk) that requires grad
    for call in (lambda: h.forward_stream(chunk), lambda: c.forward_stream(chunk, ei), lambda: h.forward_stream(chunk, state=s_h, dilation=2)):
        with pytest.raises(_lib.TgcnError, match=NOGRAD):
            call()
    h.requires_grad_(False)
    with pytest.raises(_lib.TgcnError, match=NOGRAD):
        h.forward_stream(chunk.clone().requires_grad_(True))
    h.requires_grad_(True)
    with pytest.raises(_lib.TgcnError, match=NOGRAD):
        F.cheb_time_stream(_op("plain"), chunk, torch.randn(3, 3, 4, 8, requires_grad=True), None, F.BIAS_NONE, 0)
    with torch.no_grad():
        # a state of another dilation, shape (S, n, f, K, H), dtype or operand
        with pytest.raises(_lib.TgcnError, match=MADE + " dilation 2"):
            h.forward_stream(chunk, state=s_h, dilation=3)
        with pytest.raises(_lib.TgcnError, match=MADE + r" \(S, n, f, K, H\)"):
            h.forward_stream(torch.randn(3, N_V, 5, 4), state=s_h, dilation=2)
        with pytest.raises(_lib.TgcnError, match=MADE + r" \(S, n, f, K, H\)"):
            tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 4).forward_stream(chunk, state=s_h, dilation=2)
        with pytest.raises(_lib.TgcnError, match=MADE + " dtype"):
            h.forward_stream(chunk, state=s_bf, dilation=2)
        with pytest.raises(_lib.TgcnError, match=MADE + " another operand"):
            h.forward_stream(chunk, state=s_h2, dilation=2)
        with pytest.raises(_lib.TgcnError, match=MADE + " another operand"):
            c.forward_stream(chunk, ei, state=s_h, dilation=2)
        with pytest.raises(_lib.TgcnError, match=MADE + " another operand"):
            F.cheb_time_stream(_op("plain"), chunk, h.weight, None, F.BIAS_NONE, 0, s_c, 2)
        # a graph the layer holds no operand for (another edge list, or one its cache has evicted): refused by a look into the cache
        with pytest.raises(_lib.TgcnError, match=MADE + " another operand"):
            c.forward_stream(chunk, torch.tensor([[0, 2], [2, 0]]), state=s_c, dilation=2)
        with pytest.raises(_lib.TgcnError, match=MADE + " another operand"):
            tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3).forward_stream(chunk, state=s_h, dilation=2)
        with pytest.raises(_lib.TgcnError, match="SeriesStreamState or None"):
            h.forward_stream(chunk, state=s_h.ring, dilation=2)
        # an fp32 chunk with bf16 parameters
        with pytest.raises(_lib.TgcnError, match="cast it once"):
            tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3).to(BF).forward_stream(chunk)
        with pytest.raises(_lib.TgcnError, match="cast it once"):
            tgcn_amd.ChebTimeConv(4, 8, 3, 3).to(BF).forward_stream(chunk, ei)
        # a learnable edge weight
        with pytest.raises(_lib.TgcnError, match="learnable edge weights"):
            c.forward_stream(chunk, ei, torch.ones(2, requires_grad=True))
        # dilations that are no integer >= 1, an empty chunk, the wrong channel count, mixed parameter dtypes
        for bad in (0, -1, 2.0, True, None):
            with pytest.raises(_lib.TgcnError, match="dilation is an integer >= 1"):
                h.forward_stream(chunk, dilation=bad)
            with pytest.raises(_lib.TgcnError, match="dilation is an integer >= 1"):
                c.forward_stream(chunk, ei, dilation=bad)
            with pytest.raises(_lib.TgcnError, match="dilation is an integer >= 1"):
                F.cheb_time_stream(_op("plain"), chunk, h.weight, None, F.BIAS_NONE, 0, None, bad)
        with pytest.raises(_lib.TgcnError, match="at least one time row"):
            h.forward_stream(chunk[:, :, :0])
        with pytest.raises(_lib.TgcnError, match="channel"):
            h.forward_stream(torch.randn(2, N_V, 5, 3))
        with pytest.raises(_lib.TgcnError, match="channel"):
            c.forward_stream(torch.randn(2, N_V, 5), ei)
    assert rec.calls == []
    # a refused call leaves the state it was offered as it was
    assert (s_h.head, s_h.seen) == before[:2] and torch.equal(s_h.ring, before[2])


def test_the_existing_streaming_calls_make_the_calls_they_made(recorder, monkeypatch):
    """one default call, one causal call and one dilated call, in both dtypes and on both classes: the same launch lists before and after
    stream calls on the same modules"""
    rec = recorder({})
    _stub_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])

    def lists():
        got = []
        for dt in (torch.float32, BF):
            torch.manual_seed(3)
            series = torch.randn(2, N_V, T_WIN, 4).to(dt)
            for layer, extra in ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3).to(dt), ()), (tgcn_amd.ChebTimeConv(4, 8, 3, 3).to(dt), (ei,))):
                if lists.stream_first:
                    with torch.no_grad():
                        _, st = layer.forward_stream(series[:, :, :5], *extra, dilation=2)
                        layer.forward_stream(series[:, :, 5:], *extra, state=st, dilation=2)
                for geo in (dict(), dict(padding="causal", as_series=True), dict(padding="causal", as_series=True, dilation=2)):
                    del rec.calls[:]
                    out = layer.forward_series(series, *extra, **geo)
                    out.backward(torch.ones_like(out))
                    got.append(list(rec.calls))
                del rec.calls[:]
                F.cheb_time_windows(_op("plain"), series, layer.weight, None, F.BIAS_NONE, 1, dilation=2)
                got.append(list(rec.calls))
        return got

    lists.stream_first = False
    plain = lists()
    lists.stream_first = True
    after = lists()
    assert plain == after and all(plain) and not any("stream" in c for calls in plain for c in calls)


def test_the_stream_entries_are_declared_everywhere():
    """the header, the ctypes table and the library agree on the two entries; ABI 8; the host checks that run before any launch"""
    names = ["tgcn_cheb_project_series_stream_f32", "tgcn_cheb_project_series_stream_bf16"]
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "tgcn_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert nm in _lib.SIGNATURES and hasattr(handle, nm) and (" " + nm + "(") in header, nm
    L = _lib.lib()
    assert L.tgcn_abi_version() == 8 == _lib.ABI_VERSION
    # null pointers are never reached: the scalar rules refuse first.  S n Tc f H N K = 2 48 5 4 3 8 3, dilation 4: C = 8, ring_ld >= 32
    INVALID = -1
    one = ctypes.c_void_p(16)       # a non-null pointer that the refused calls never read

    def f32(Tc=5, H=3, ring_ld=32, head=0, dil=4):
        return L.tgcn_cheb_project_series_stream_f32(None, 2, 48, Tc, 4, H, 8, 3, one, one, None, 0, one, one, ring_ld, head, dil)

    def b16(Tc=5, H=3, ring_ld=32, head=0, dil=4):
        return L.tgcn_cheb_project_series_stream_bf16(None, 2, 48, Tc, 4, H, 8, 3, one, Tc * 4, one, None, 0, 0, one, one, ring_ld, head, dil)

    for entry in (f32, b16):
        assert entry(head=8) == INVALID and entry(head=-1) == INVALID           # head outside [0, C)
        assert entry(Tc=0) == INVALID and entry(dil=0) == INVALID and entry(dil=-3) == INVALID
        assert entry(ring_ld=31) == INVALID                                     # the ring's rows hold C*f elements
        assert entry(H=1, head=0, ring_ld=0) == INVALID                         # one tap keeps no ring: C = 0, no head is inside [0, 0)
        assert entry(dil=2 ** 30) == INVALID
