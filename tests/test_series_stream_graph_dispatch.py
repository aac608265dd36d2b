"""CPU test of the launches of the capturable streaming calls (forward_stream / F.cheb_time_stream with capturable=True), by the recorder
technique of tests/test_layer_dispatch.py: a capturable call asks the step-1 plan, runs K - 1 hops and launches the _pos entry with the
host-head entry's scalars minus the head (the position is a device pointer, which the recorder does not log); a one-tap layer launches the
_conv entry and then series_stream_advance; default calls log what tests/test_series_stream_dispatch.py expects of them, before and after a
capturable call; the new refusals -- capturable=True next to a host-head state, a host-head state while the stream is capturing -- raise
TgcnError with nothing logged and no operand built; and the three new entries are declared in the header, the ctypes table and the library."""
import ctypes
import os

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F

from test_layer_dispatch import N_V, _op, recorder  # noqa: F401  (the recorder fixture)
from test_series_stream_dispatch import BF, _entries, _no_operands, _stream, _stub_operands

CHUNKS = [1, 1, 3, 8, 9, 40, 5]


def _stream_cap(rec, op, chunk, W, bias, mode, state, dilation, capturable=True):
    del rec.calls[:]
    with torch.no_grad():
        out, state = F.cheb_time_stream(op, chunk, W, bias, F.BIAS_NONE if bias is None else F.BIAS_CHANNEL, mode, state, dilation,
                                        capturable=capturable)
    return out, state, list(rec.calls)


@pytest.mark.parametrize("mode", [0, 1], ids=["power", "chebyshev"])
@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
def test_a_capturable_call_logs_plan_hops_and_the_pos_entry(dt, mode, recorder):
    rec = recorder({})
    S, f, H, N, K, d = 3, 8, 3, 8, 3, 4
    Cr = (H - 1) * d
    bf16 = dt == BF
    torch.manual_seed(0)
    W, bias, op = torch.randn(K, H, f, N).to(dt), torch.randn(N).to(dt), _op("plain")
    cap = host = None
    for Tc in CHUNKS:
        chunk = torch.randn(S, N_V, Tc, f).to(dt)
        out, cap, calls = _stream_cap(rec, op, chunk, W, bias, mode, cap, d, capturable=(cap is None))      # afterwards the state's kind rules
        _, host, host_calls = _stream(rec, op, chunk, W, bias, mode, host, d)
        assert tuple(out.shape) == (S, N_V, Tc, N) and out.dtype == dt and out.is_contiguous()
        ent = _entries(calls)
        plan, hop, entry = (("series_conv_plan_bf16", "csr_hop2_bf16", "cheb_project_series_stream_pos_bf16") if bf16
                            else ("series_conv_plan", "csr_hop2", "cheb_project_series_stream_pos"))
        assert calls[0] == "%s %d %d %d 1 1" % (plan, H, f, N) and ent.count(plan) == 1
        hops = [c for c in calls if c.split()[0] == hop]
        assert len(hops) == K - 1 and all(c.split()[1:3] == [str(S), str(Tc * f)] for c in hops)
        assert ent.index(entry) == len(ent) - 1 and ent.count(entry) == 1
        # scalars: S n Tc f H N K [stack_ld bias_dtype] bias_kind ring_ld dilation -- the host-head entry's without the head
        mid = "%d 1 1" % (Tc * f) if bf16 else "1"
        assert calls[-1] == "%s %d %d %d %d %d %d %d %s %d %d" % (entry, S, N_V, Tc, f, H, N, K, mid, Cr * f, d)
        hs = host_calls[-1].split()
        assert hs[0] == entry.replace("_pos", "") and hs[1:-2] + hs[-1:] == calls[-1].split()[1:]
        # everything before the entry is the host-head call's
        assert calls[:-1] == host_calls[:-1]
        assert set(ent) <= {plan, hop, entry, "fold_weight"}, ent
    assert cap.capturable and cap.pos.dtype == torch.int64 and tuple(cap.pos.shape) == (2,) and cap.pos.device == cap.ring.device
    assert tuple(cap.ring.shape) == (K, S, N_V, Cr * f) and cap.ring.dtype == dt and (cap.C, cap.dilation) == (Cr, d)
    # the host does not move a capturable state (the recorder launches nothing, so pos is still zero); head and seen read pos
    assert (cap.head, cap.seen) == (0, 0) and (host.head, host.seen) == (sum(CHUNKS) % Cr, sum(CHUNKS))
    cap.pos.copy_(torch.tensor([5, 77]))
    assert (cap.head, cap.seen) == (5, 77)
    cap.ring.fill_(1)
    assert cap.reset() is cap and (cap.head, cap.seen) == (0, 0) and not cap.ring.any() and not cap.pos.any()
    assert not host.capturable and host.pos is None


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
def test_both_classes_pass_the_flag_on(dt, recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    sfx = "_bf16" if dt == BF else ""
    for f in (1, 4):
        for layer, extra in ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), f, 8, 3, 3).to(dt), ()), (tgcn_amd.ChebTimeConv(f, 8, 3, 3).to(dt), (ei,))):
            state = None
            for Tc in (5, 2, 7):
                chunk = torch.randn(2, N_V, Tc, f).to(dt)
                if f == 1:
                    chunk = chunk[..., 0]
                del rec.calls[:]
                with torch.no_grad():
                    out, state = layer.forward_stream(chunk, *extra, state=state, dilation=2, capturable=True)
                ent = _entries(rec.calls)
                assert ent.count("cheb_project_series_stream_pos" + sfx) == 1 and ent[-1] == "cheb_project_series_stream_pos" + sfx
                assert "cheb_project_series_stream" + sfx not in ent and "series_stream_advance" not in ent
                sc = rec.calls[-1].split()
                assert sc[1:8] == [str(v) for v in (2, N_V, Tc, f, 3, 8, 3)] and sc[-2:] == [str(4 * f), "2"]
                assert state.capturable and tuple(out.shape) == (2, N_V, Tc, 8) and out.dtype == dt


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
def test_one_tap_launches_the_conv_entry_then_the_advance(dt, recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    sfx = "_bf16" if dt == BF else ""
    layer = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 8, 8, 3, 1).to(dt)
    state = None
    for Tc, dil in ((4, 1), (1, 7), (9, 2 ** 30)):
        del rec.calls[:]
        with torch.no_grad():
            out, state = layer.forward_stream(torch.randn(2, N_V, Tc, 8).to(dt), state=state, dilation=dil, capturable=True)
        ent = _entries(rec.calls)
        assert ent[-2:] == ["cheb_project_series_conv" + sfx, "series_stream_advance"] and ent.count("series_stream_advance") == 1
        assert not any("project_series_stream" in e for e in ent)
        assert rec.calls[-2].split()[-4:] == ["1", "1", "0", "0"] and rec.calls[-2].split()[1:4] == ["2", str(N_V), str(Tc)]
        assert rec.calls[-1] == "series_stream_advance %d 0" % Tc           # Tc, C = 0: head stays 0, seen counts
        assert tuple(out.shape) == (2, N_V, Tc, 8)
    assert state.capturable and state.ring is None and state.C == 0 and tuple(state.pos.shape) == (2,)


def test_default_calls_log_what_they_logged_before_and_after_a_capturable_call(recorder):
    """the launch list tests/test_series_stream_dispatch.py pins for a host-head call, chunk by chunk, on fresh states -- once before any
    capturable call, once after capturable calls on the same operand"""
    rec = recorder({})
    S, f, H, N, K, d = 3, 8, 3, 8, 3, 4
    Cr = (H - 1) * d
    torch.manual_seed(0)
    op = _op("plain")

    def default_lists(dt, mode):
        W, bias = torch.randn(K, H, f, N).to(dt), torch.randn(N).to(dt)
        state, head, got = None, 0, []
        bf16 = dt == BF
        plan, hop, entry = (("series_conv_plan_bf16", "csr_hop2_bf16", "cheb_project_series_stream_bf16") if bf16
                            else ("series_conv_plan", "csr_hop2", "cheb_project_series_stream"))
        for Tc in CHUNKS:
            _, state, calls = _stream(rec, op, torch.randn(S, N_V, Tc, f).to(dt), W, bias, mode, state, d)
            ent = _entries(calls)
            assert calls[0] == "%s %d %d %d 1 1" % (plan, H, f, N) and ent.count(plan) == 1
            assert len([c for c in calls if c.split()[0] == hop]) == K - 1
            mid = "%d 1 1" % (Tc * f) if bf16 else "1"
            assert calls[-1] == "%s %d %d %d %d %d %d %d %s %d %d %d" % (entry, S, N_V, Tc, f, H, N, K, mid, Cr * f, head, d)
            assert set(ent) <= {plan, hop, entry, "fold_weight"} and ent.count("fold_weight") == (1 if mode == 0 else 0)
            head = (head + Tc) % Cr
            assert (state.head, state.seen) == (head, sum(CHUNKS[:len(got) + 1])) and not state.capturable and state.pos is None
            got.append(calls)
        return got

    cases = [(dt, mode) for dt in (torch.float32, BF) for mode in (0, 1)]
    before = [default_lists(dt, mode) for dt, mode in cases]
    for dt, mode in cases:
        st = None
        for Tc in (3, 9):
            _, st, _ = _stream_cap(rec, op, torch.randn(S, N_V, Tc, f).to(dt), torch.randn(K, H, f, N).to(dt), None, mode, st, d)
    after = [default_lists(dt, mode) for dt, mode in cases]
    assert before == after and not any("_pos" in c or "advance" in c for lists in before for calls in lists for c in calls)


def test_the_new_refusals_come_before_anything_is_built_or_launched(recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    h, c = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3), tgcn_amd.ChebTimeConv(4, 8, 3, 3)
    one = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 1)
    chunk = torch.randn(2, N_V, 5, 4)
    with torch.no_grad():           # host-head and capturable states, and every operand cached
        _, s_h = h.forward_stream(chunk, dilation=2)
        _, s_c = c.forward_stream(chunk, ei, dilation=2)
        _, s_one = one.forward_stream(chunk)
        _, s_hc = h.forward_stream(chunk, dilation=2, capturable=True)
        _, s_cc = c.forward_stream(chunk, ei, dilation=2, capturable=True)
    op = s_h.op
    before = (s_h.head, s_h.seen, s_h.ring.clone())
    del rec.calls[:]
    _no_operands(monkeypatch)
    HOST, CAP = "keeps its head on the host", r"capturable=True"
    with torch.no_grad():
        # capturable=True next to a state that keeps its head on the host
        with pytest.raises(_lib.TgcnError, match=HOST):
            h.forward_stream(chunk, state=s_h, dilation=2, capturable=True)
        with pytest.raises(_lib.TgcnError, match=HOST):
            c.forward_stream(chunk, ei, state=s_c, dilation=2, capturable=True)
        with pytest.raises(_lib.TgcnError, match=HOST):
            F.cheb_time_stream(op, chunk, h.weight, None, F.BIAS_NONE, 0, s_h, 2, capturable=True)
        assert rec.calls == []
        # a host-head state with a ring while the stream is capturing: given, or about to be made
        monkeypatch.setattr(F, "stream_is_capturing", lambda: True)
        for call in (lambda: h.forward_stream(chunk, state=s_h, dilation=2), lambda: c.forward_stream(chunk, ei, state=s_c, dilation=2),
                     lambda: h.forward_stream(chunk, dilation=2), lambda: c.forward_stream(chunk, ei),
                     lambda: F.cheb_time_stream(op, chunk, h.weight, None, F.BIAS_NONE, 0, s_h, 2),
                     lambda: F.cheb_time_stream(op, chunk, h.weight, None, F.BIAS_NONE, 0)):
            with pytest.raises(_lib.TgcnError, match=CAP):
                call()
        assert rec.calls == []
        assert (s_h.head, s_h.seen) == before[:2] and torch.equal(s_h.ring, before[2])
    # what is NOT refused while capturing: capturable states, and a one-tap layer, which keeps no ring (C == 0) -- operands come from the cache
    _stub_operands(monkeypatch)
    with torch.no_grad():
        h.forward_stream(chunk, state=s_hc, dilation=2)
        c.forward_stream(chunk, ei, state=s_cc, dilation=2)
        one.forward_stream(chunk, state=s_one)
        h.forward_stream(chunk, dilation=2, capturable=True)
    assert [e for e in _entries(rec.calls) if "stream" in e] == ["cheb_project_series_stream_pos"] * 2 + ["cheb_project_series_stream_pos"]
    # eager calls are unaffected
    monkeypatch.setattr(F, "stream_is_capturing", lambda: False)
    del rec.calls[:]
    with torch.no_grad():
        h.forward_stream(chunk, state=s_h, dilation=2)
    assert _entries(rec.calls)[-1] == "cheb_project_series_stream"


def test_the_capturing_predicate_is_false_without_a_device():
    """no device is initialised in a CPU run: the predicate answers False without touching one"""
    if not torch.cuda.is_initialized():
        assert F.stream_is_capturing() is False


def test_the_pos_entries_are_declared_everywhere():
    """the header, the ctypes table and the library agree on the three entries; ABI 8; the host checks that run before any launch"""
    names = ["tgcn_cheb_project_series_stream_pos_f32", "tgcn_cheb_project_series_stream_pos_bf16", "tgcn_series_stream_advance"]
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "tgcn_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert nm in _lib.SIGNATURES and hasattr(handle, nm) and (" " + nm + "(") in header, nm
    L = _lib.lib()
    assert L.tgcn_abi_version() == 8 == _lib.ABI_VERSION
    # null pointers are never reached: the scalar rules refuse first.  S n Tc f H N K = 2 48 5 4 3 8 3, dilation 4: C = 8, ring_ld >= 32
    INVALID = -1
    one = ctypes.c_void_p(16)       # a non-null pointer that the refused calls never read

    def f32(Tc=5, H=3, ring_ld=32, pos=one, dil=4, f=4):
        return L.tgcn_cheb_project_series_stream_pos_f32(None, 2, 48, Tc, f, H, 8, 3, one, one, None, 0, one, one, ring_ld, pos, dil)

    def b16(Tc=5, H=3, ring_ld=32, pos=one, dil=4, f=4):
        return L.tgcn_cheb_project_series_stream_pos_bf16(None, 2, 48, Tc, f, H, 8, 3, one, Tc * f, one, None, 0, 0, one, one, ring_ld, pos, dil)

    for entry in (f32, b16):
        # a time row that fits no LDS span: the plan refuses (TGCN_ERR_UNSUPPORTED) before anything is launched
        assert entry(f=4096, ring_ld=8 * 4096) == -4 and b"do not fit the LDS span" in L.tgcn_last_error()
        assert entry(pos=None) == INVALID                                       # a null position
        assert entry(Tc=0) == INVALID and entry(dil=0) == INVALID and entry(dil=-3) == INVALID
        assert entry(ring_ld=31) == INVALID
        assert entry(H=1, ring_ld=0) == INVALID                                 # one tap keeps no ring: the _conv entry and the advance
        assert entry(dil=2 ** 30) == INVALID
    assert L.tgcn_series_stream_advance(None, None, 1, 2) == INVALID
    assert L.tgcn_series_stream_advance(None, one, 0, 2) == INVALID and L.tgcn_series_stream_advance(None, one, 1, -1) == INVALID
