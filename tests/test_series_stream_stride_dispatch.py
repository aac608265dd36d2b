"""CPU test of the launches of a streaming call with a window step (forward_stream / F.cheb_time_stream, stride=s), by the recorder of
tests/test_layer_dispatch.py: without `stride`, or at stride=1, a call logs exactly what it logs without the keyword (host-head and
capturable states, fp32 and bf16, H > 1 and H = 1); at stride=3 the plan query carries the step and ONE call of the _stream_strided entry
follows the hops, with (head | pos, stride, win_off) as computed from seen -- no _conv entry, no other stream entry, also for a chunk in which
no window ends; every refusal raises TgcnError with nothing logged; m and off over the chunk lists of tests/test_series_stream_stride.py
equal a brute-force count; the header, the ctypes table and the library agree on the two entries at ABI 8."""
import ctypes
import os

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F

from test_layer_dispatch import N_V, _op, recorder  # noqa: F401  (the recorder fixture)
from test_series_stream_dispatch import _entries, _no_operands, _stub_operands
from test_series_stream_stride import LISTS

BF = torch.bfloat16
NAMES = ["tgcn_cheb_project_series_stream_strided_f32", "tgcn_cheb_project_series_stream_strided_bf16"]


def brute_force(seen, Tc, s):
    """(m, off): the windows j (ending at absolute row j*s) that end inside [seen, seen + Tc), and the chunk row of the first"""
    ends = [t - seen for t in range(seen, seen + Tc) if t % s == 0]
    return len(ends), (ends[0] if ends else next(t for t in range(seen, seen + s) if t % s == 0) - seen)


@pytest.mark.parametrize("case", LISTS, ids=lambda c: "H%d_s%d" % c[:2])
def test_m_and_off_are_a_brute_force_count(case):
    H, s, chunks = case
    seen = total = 0
    for Tc in chunks:
        m, off = F.stream_windows(seen, Tc, s)
        assert (m, off) == brute_force(seen, Tc, s) and 0 <= off < s
        assert m == -(-(seen + Tc) // s) - -(-seen // s) and off == (-seen) % s
        assert m == ((Tc - off - 1) // s + 1 if off < Tc else 0)                 # the entry's own count from (Tc, stride, win_off)
        seen, total = seen + Tc, total + m
    assert total == (seen - 1) // s + 1 == F.series_geometry(seen, H, s, "causal")[3]


def _call(rec, layer, extra, chunk, state, **kw):
    del rec.calls[:], rec.nulls[:]
    with torch.no_grad():
        out, state = layer.forward_stream(chunk, *extra, state=state, **kw)
    return out, state, list(rec.calls)


def _layers(dt, f, H):
    ei = torch.tensor([[0, 1], [1, 0]])
    return ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), f, 8, 3, H).to(dt), ()), (tgcn_amd.ChebTimeConv(f, 8, 3, H).to(dt), (ei,)))


@pytest.mark.parametrize("capturable", [False, True], ids=["host-head", "capturable"])
@pytest.mark.parametrize("H", [3, 1])
@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
def test_stride_one_and_no_stride_log_the_same_calls(dt, H, capturable, recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    for layer, extra in _layers(dt, 4, H):
        lists = []
        for kw in (dict(), dict(stride=1)):
            state, got = None, []
            for Tc in (5, 2, 7):
                torch.manual_seed(Tc)
                out, state, calls = _call(rec, layer, extra, torch.randn(2, N_V, Tc, 4).to(dt), state, capturable=capturable, **kw)
                assert tuple(out.shape) == (2, N_V, Tc, 8) and state.stride == 1
                got.append((calls, list(rec.nulls)))
            lists.append(got)
        assert lists[0] == lists[1] and all(c for c, _ in lists[0])
        ent = [e for calls, _ in lists[0] for e in _entries(calls)]
        assert not any("strided" in e for e in ent)
        sfx = "_bf16" if dt == BF else ""
        want = "cheb_project_series_conv" if H == 1 else ("cheb_project_series_stream_pos" if capturable else "cheb_project_series_stream")
        assert ent.count(want + sfx) == 3


@pytest.mark.parametrize("H", [3, 1])
@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
def test_stride_three_logs_the_plan_with_the_step_and_one_strided_entry(dt, H, recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    S, f, N, K, s = 2, 8, 8, 3, 3
    Cr = H - 1
    bf16 = dt == BF
    plan, hop, entry = (("series_conv_plan_bf16", "csr_hop2_bf16", "cheb_project_series_stream_strided_bf16") if bf16
                        else ("series_conv_plan", "csr_hop2", "cheb_project_series_stream_strided"))
    for layer, extra in _layers(dt, f, H):
        state, head, seen = None, 0, 0
        for Tc in (1, 1, 5, 2, 1, 9):                  # seen = 1 and 8: chunks of one row in which no window ends
            out, state, calls = _call(rec, layer, extra, torch.randn(S, N_V, Tc, f).to(dt), state, stride=s)
            m, off = brute_force(seen, Tc, s)
            assert tuple(out.shape) == (S, N_V, m, N) and out.dtype == dt and out.is_contiguous()
            ent = _entries(calls)
            assert calls[0] == "%s %d %d %d 1 %d" % (plan, H, f, N, s) and ent.count(plan) == 1            # H f N vec step
            hops = [c for c in calls if c.split()[0] == hop]
            assert len(hops) == K - 1 and all(c.split()[1:3] == [str(S), str(Tc * f)] for c in hops)
            assert ent.index(entry) == len(ent) - 1 and ent.count(entry) == 1
            # scalars: S n Tc f H N K [stack_ld bias_dtype] bias_kind ring_ld head stride win_off
            sc = calls[-1].split()
            assert sc[:8] == [entry] + [str(v) for v in (S, N_V, Tc, f, H, N, K)] and sc[-4:] == [str(v) for v in (Cr * f, head, s, off)]
            assert len(sc) == (15 if bf16 else 13) and (not bf16 or sc[8:10] == [str(Tc * f), "1"])
            assert not any(("stream" in e and e != entry) or "series_conv" in e.replace("series_conv_plan", "") for e in ent), ent
            # pointers: out is null exactly when no window ends inside the chunk, the ring when H = 1, pos always (a host-head state)
            types = _lib.SIGNATURES["tgcn_" + entry + ("" if bf16 else "_f32")][1]
            ptrs = [i for i, t in enumerate(types) if t is ctypes.c_void_p]
            out_i, ring_i, pos_i = ptrs[-3:]
            nulls = rec.nulls[-1]
            assert (out_i in nulls) == (m == 0) and (ring_i in nulls) == (H == 1) and pos_i in nulls
            seen += Tc
            head = seen % Cr if Cr else 0
            assert (state.head, state.seen, state.stride) == (head, seen, s)
        assert any(brute_force(t, 1, s)[0] == 0 for t in (1, 8))


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
def test_a_capturable_state_passes_the_device_position(dt, recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    s, f, H = 2, 8, 3
    entry = "cheb_project_series_stream_strided" + ("_bf16" if dt == BF else "")
    for layer, extra in _layers(dt, f, H):
        state = None
        for _ in range(2):
            out, state, calls = _call(rec, layer, extra, torch.randn(2, N_V, 6, f).to(dt), state, stride=s, capturable=True)
            assert tuple(out.shape) == (2, N_V, 3, 8) and state.capturable and state.stride == s
            ent = _entries(calls)
            assert ent.count(entry) == 1 and ent[-1] == entry and "series_stream_advance" not in ent      # the entry moves the position
            assert calls[-1].split()[-4:] == [str((H - 1) * f), "0", str(s), "0"]                       # ring_ld, head (unused), stride, win_off
            types = _lib.SIGNATURES["tgcn_" + entry + ("" if dt == BF else "_f32")][1]
            pos_i = [i for i, t in enumerate(types) if t is ctypes.c_void_p][-1]
            assert pos_i not in rec.nulls[-1]


def test_every_refusal_of_the_step_comes_before_anything_is_built_or_launched(recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    h, c = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3), tgcn_amd.ChebTimeConv(4, 8, 3, 3)
    chunk = torch.randn(2, N_V, 6, 4)
    with torch.no_grad():
        _, s1 = h.forward_stream(chunk)
        _, s2 = h.forward_stream(chunk, stride=2)
        _, s2c = h.forward_stream(chunk, stride=2, capturable=True)
        _, c2 = c.forward_stream(chunk, ei, stride=2)
    before = (s2.head, s2.seen, s2.ring.clone())
    del rec.calls[:]
    _no_operands(monkeypatch)
    with torch.no_grad():
        for bad in (0, -1, 2.0, True, None, "2"):
            for call in (lambda: h.forward_stream(chunk, stride=bad), lambda: c.forward_stream(chunk, ei, stride=bad),
                         lambda: F.cheb_time_stream(_op("plain"), chunk, h.weight, None, F.BIAS_NONE, 0, stride=bad),
                         lambda: F.stream_precheck(chunk, h.weight, None, None, 1, stride=bad)):
                with pytest.raises(_lib.TgcnError, match="stride is an integer >= 1"):
                    call()
        for call in (lambda: h.forward_stream(chunk, dilation=2, stride=2), lambda: c.forward_stream(chunk, ei, dilation=2, stride=2),
                     lambda: F.cheb_time_stream(_op("plain"), chunk, h.weight, None, F.BIAS_NONE, 0, None, 2, stride=2)):
            with pytest.raises(_lib.TgcnError, match="together with stride"):
                call()
        for call in (lambda: h.forward_stream(chunk, fused=True, stride=2), lambda: c.forward_stream(chunk, ei, fused=True, stride=2),
                     lambda: h.forward_stream(chunk, state=s2, fused=True, stride=2)):
            with pytest.raises(_lib.TgcnError, match="fused=True has no window step"):
                call()
        # a state of another stride, either way round
        with pytest.raises(_lib.TgcnError, match="the state was made for stride 2, the call has 1"):
            h.forward_stream(chunk, state=s2)
        with pytest.raises(_lib.TgcnError, match="the state was made for stride 2, the call has 3"):
            h.forward_stream(chunk, state=s2, stride=3)
        with pytest.raises(_lib.TgcnError, match="the state was made for stride 1, the call has 2"):
            h.forward_stream(chunk, state=s1, stride=2)
        with pytest.raises(_lib.TgcnError, match="the state was made for stride 2, the call has 4"):
            c.forward_stream(chunk, ei, state=c2, stride=4)
        # a capturable state takes chunks of whole steps only: with a state, and when the call would make one
        for call in (lambda: h.forward_stream(chunk[:, :, :5], state=s2c, stride=2),
                     lambda: h.forward_stream(chunk[:, :, :1], state=s2c, stride=2),
                     lambda: h.forward_stream(chunk[:, :, :5], stride=2, capturable=True),
                     lambda: c.forward_stream(chunk, ei, stride=4, capturable=True)):
            with pytest.raises(_lib.TgcnError, match="chunks of whole steps"):
                call()
        # what forward_stream refused without the keyword stays refused with it
        with pytest.raises(_lib.TgcnError, match="at least one time row"):
            h.forward_stream(chunk[:, :, :0], stride=2)
        with pytest.raises(_lib.TgcnError, match="capturable=True with a state that keeps its head on the host"):
            h.forward_stream(chunk, state=s2, stride=2, capturable=True)
    with pytest.raises(_lib.TgcnError, match=r"torch\.no_grad\(\)"):
        h.forward_stream(chunk, stride=2)
    assert rec.calls == []
    assert (s2.head, s2.seen) == before[:2] and torch.equal(s2.ring, before[2])
    assert s2.mismatch(torch.float32, 2, N_V, 4, 3, 3, 1) == "stride 2, the call has 1" and s2.mismatch(torch.float32, 2, N_V, 4, 3, 3, 1, 2) is None


def test_fused_auto_takes_the_unfused_path_at_a_step(recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    monkeypatch.setattr(F, "STREAM_FUSED_AUTO_MAX_TC", 64)
    h = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3)
    out, state, calls = _call(rec, h, (), torch.randn(2, N_V, 6, 4), None, fused="auto", stride=2)
    ent = _entries(calls)
    assert ent[-1] == "cheb_project_series_stream_strided" and not any("stream_small" in e for e in ent) and tuple(out.shape) == (2, N_V, 3, 8)


def test_positional_calls_keep_their_meaning():
    import inspect
    assert list(inspect.signature(tgcn_amd.TGCNCheb_H.forward_stream).parameters)[1:] == ["chunk", "state", "dilation", "capturable", "fused", "stride"]
    assert list(inspect.signature(tgcn_amd.ChebTimeConv.forward_stream).parameters)[1:] == ["chunk", "edge_index", "edge_weight", "state", "dilation",
                                                                                            "capturable", "fused", "stride"]
    assert list(inspect.signature(F.cheb_time_stream).parameters)[-4:] == ["dilation", "capturable", "fused", "stride"]
    assert list(inspect.signature(F.stream_precheck).parameters)[-3:] == ["capturable", "fused", "stride"]
    assert list(inspect.signature(F.SeriesStreamState.__init__).parameters)[-2:] == ["capturable", "stride"]
    assert list(inspect.signature(F.SeriesStreamState.mismatch).parameters)[-2:] == ["dilation", "stride"]
    for fn in (tgcn_amd.TGCNCheb_H.forward_stream, tgcn_amd.ChebTimeConv.forward_stream, F.cheb_time_stream):
        assert inspect.signature(fn).parameters["stride"].default == 1 and "(-seen) mod s" in fn.__doc__ and "skips its later" in fn.__doc__


def test_the_strided_stream_entries_are_declared_everywhere():
    """the header, the ctypes table and the library agree on the two entries; ABI 8; the host checks that run before any launch"""
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "tgcn_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for nm in NAMES:
        assert nm in _lib.SIGNATURES and hasattr(handle, nm) and (" " + nm + "(") in header, nm
    L = _lib.lib()
    assert L.tgcn_abi_version() == 8 == _lib.ABI_VERSION
    INVALID = -1
    one = ctypes.c_void_p(16)       # a non-null pointer that the refused calls never read

    # S n Tc f H N K = 2 48 5 4 3 8 3: C = 2, ring_ld >= 8
    def f32(Tc=5, H=3, ring_ld=8, head=0, pos=None, stride=2, off=0, ring=one):
        return L.tgcn_cheb_project_series_stream_strided_f32(None, 2, 48, Tc, 4, H, 8, 3, one, one, None, 0, one, ring, ring_ld, head, pos, stride, off)

    def b16(Tc=5, H=3, ring_ld=8, head=0, pos=None, stride=2, off=0, ring=one):
        return L.tgcn_cheb_project_series_stream_strided_bf16(None, 2, 48, Tc, 4, H, 8, 3, one, Tc * 4, one, None, 0, 0, one, ring, ring_ld, head, pos,
                                                              stride, off)

    for entry in (f32, b16):
        assert entry(stride=0) == INVALID and entry(stride=-2) == INVALID
        assert entry(off=2) == INVALID and entry(off=-1) == INVALID and entry(stride=1, off=1) == INVALID      # win_off outside [0, stride)
        assert entry(head=2) == INVALID and entry(head=-1) == INVALID            # the host's head outside [0, C)
        assert entry(Tc=0) == INVALID and entry(ring_ld=7) == INVALID and entry(ring=None) == INVALID
        assert entry(H=0) == INVALID
