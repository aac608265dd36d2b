"""CPU test of the launches of the one-launch streaming step (forward_stream / F.cheb_time_stream with fused=...), by the recorder technique
of tests/test_layer_dispatch.py.  fused=True asks tgcn_cheb_stream_small_plan once and first, folds the weight at most once and launches
tgcn_cheb_stream_small_f32 last -- or, for a capturable state, followed by series_stream_advance -- with the ring's scalars: head follows
(head + Tc) mod C over a chunk sequence that wraps, seen adds up, pos is null for a host-head state and a pointer for a capturable one.
fused="auto" above the threshold, or with a plan that refuses, makes exactly the calls of fused=False.  Every refusal raises TgcnError with
nothing launched, and without an operand where none is needed.  Fused and unfused calls alternate on one state.  The two entries are in the
header, the ctypes table and the library at ABI 8, and small_stream_kernel's instantiations use no scratch and spill nothing."""
import ctypes
import os
import sys

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F

from test_layer_dispatch import N_V, _Op, _op, _Recorder, recorder  # noqa: F401  (the recorder fixture)
from test_series_stream_dispatch import BF, _entries, _no_operands, _stream, _stub_operands

CHUNKS = [1, 1, 3, 8, 9, 40, 5]
PLAN, ENTRY, ADVANCE = "cheb_stream_small_plan", "cheb_stream_small", "series_stream_advance"
POS_ARG = 17        # position of `pos` among tgcn_cheb_stream_small_f32's arguments


def _fused(rec, op, chunk, W, bias, mode, state, dilation, fused=True, capturable=False):
    del rec.calls[:], rec.nulls[:]
    with torch.no_grad():
        out, state = F.cheb_time_stream(op, chunk, W, bias, F.BIAS_NONE if bias is None else F.BIAS_CHANNEL, mode, state, dilation,
                                        capturable=capturable, fused=fused)
    return out, state, list(rec.calls)


@pytest.mark.parametrize("capturable", [False, True], ids=["host-head", "capturable"])
@pytest.mark.parametrize("mode,K", [(0, 3), (1, 3), (0, 2)], ids=["power", "chebyshev", "power-K2"])
def test_a_fused_call_logs_the_plan_at_most_one_fold_and_the_fused_entry(mode, K, capturable, recorder):
    rec = recorder({})
    S, f, H, N, d = 3, 8, 3, 8, 4
    Cr = (H - 1) * d
    torch.manual_seed(0)
    W, bias, op = torch.randn(K, H, f, N), torch.randn(N), _op("plain")
    state, head, seen = None, 0, 0
    wrapped = False
    for Tc in CHUNKS:
        out, state, calls = _fused(rec, op, torch.randn(S, N_V, Tc, f), W, bias, mode, state, d, capturable=capturable and state is None)
        assert tuple(out.shape) == (S, N_V, Tc, N) and out.dtype == torch.float32 and out.is_contiguous()
        ent = _entries(calls)
        # the plan once and first: n nnz mode f H N K Tc dilation
        assert calls[0] == "%s %d %d %d %d %d %d %d %d %d" % (PLAN, N_V, op.nnz, mode, f, H, N, K, Tc, d) and ent.count(PLAN) == 1
        # the fold in power mode with K > 2 only, between the plan and the entry
        folds = 1 if (mode == 0 and K > 2) else 0
        assert ent.count("fold_weight") == folds
        tail = [ENTRY, ADVANCE] if capturable else [ENTRY]
        assert ent == [PLAN] + ["fold_weight"] * folds + tail, ent
        # scalars of the entry: mode S Tc f H N K bias_kind ring_ld head dilation (a capturable state passes head 0 and a pointer)
        ei = ent.index(ENTRY)
        assert calls[ei] == "%s %d %d %d %d %d %d %d 1 %d %d %d" % (ENTRY, mode, S, Tc, f, H, N, K, Cr * f, 0 if capturable else head, d)
        assert (POS_ARG in rec.nulls[ei]) == (not capturable)
        if capturable:
            assert calls[-1] == "%s %d %d" % (ADVANCE, Tc, Cr)
        wrapped = wrapped or (Tc < Cr and head + Tc > Cr)
        head, seen = (head + Tc) % Cr, seen + Tc
        if not capturable:
            assert (state.head, state.seen) == (head, seen)
        assert not any(e.startswith("csr_hop") or e.startswith("series_conv_plan") or "project_series_stream" in e for e in ent)
    assert wrapped and isinstance(state, F.SeriesStreamState) and state.capturable == capturable and state.C == Cr
    assert tuple(state.ring.shape) == (K, S, N_V, Cr * f) and state.ring.dtype == torch.float32
    if capturable:      # the host does not move a capturable state; the recorder launched nothing, so pos is still zero
        assert (state.head, state.seen) == (0, 0) and state.pos is not None
    else:
        assert state.pos is None and state.reset() is state and (state.head, state.seen) == (0, 0)


def test_both_classes_pass_the_keyword_on_and_a_reordered_operand_relabels_once(recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    for f in (1, 4):
        for layer, extra, mode in ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), f, 8, 3, 3), (), 0), (tgcn_amd.ChebTimeConv(f, 8, 3, 3), (ei,), 1)):
            state, head = None, 0
            for Tc in (5, 2, 7):
                chunk = torch.randn(2, N_V, Tc, f)
                if f == 1:
                    chunk = chunk[..., 0]
                del rec.calls[:]
                with torch.no_grad():
                    out, state = layer.forward_stream(chunk, *extra, state=state, dilation=2, fused=True)
                ent = _entries(rec.calls)
                assert ent[0] == PLAN and ent[-1] == ENTRY and ent.count(ENTRY) == 1 and tuple(out.shape) == (2, N_V, Tc, 8)
                sc = rec.calls[-1].split()
                assert sc[1:8] == [str(v) for v in (mode, 2, Tc, f, 3, 8, 3)] and sc[-3:] == [str(4 * f), str(head), "2"]
                head = (head + Tc) % 4
            assert (state.head, state.seen) == (head, 14)
    out, state, calls = _fused(rec, _op("reordered"), torch.randn(2, N_V, 5, 4), torch.randn(3, 3, 4, 8), torch.randn(8), 1, None, 1)
    ent = _entries(calls)
    # the plan first, then the chunk relabelled in, the entry, the output relabelled out
    assert ent == [PLAN, "pack_rows", ENTRY, "pack_rows"], ent


class _RefusingRecorder(_Recorder):
    """the recorder with a plan that answers TGCN_ERR_UNSUPPORTED; the refused query is counted, not logged as a launch"""

    def __init__(self, small):
        super().__init__(small)
        self.plans = 0

    def __getattr__(self, name):
        if name == "tgcn_cheb_stream_small_plan":
            def plan(*args):
                self.plans += 1
                return -4
            return plan
        if name == "tgcn_last_error":
            return lambda: b"stream_small_plan: does not fit"
        return super().__getattr__(name)


@pytest.fixture
def refusing(recorder, monkeypatch):
    def make():
        recorder({})
        rec = _RefusingRecorder({})
        monkeypatch.setattr(_lib, "lib", lambda: rec)
        return rec
    return make


def _lists(rec, fused, chunks, dt=torch.float32, capturable=False):
    torch.manual_seed(1)
    W, bias, op = torch.randn(3, 3, 4, 8).to(dt), torch.randn(8).to(dt), _op("plain")
    state, got = None, []
    for Tc in chunks:
        _, state, calls = _fused(rec, op, torch.randn(2, N_V, Tc, 4).to(dt), W, bias, 0, state, 2, fused=fused, capturable=capturable and state is None)
        got.append(calls)
    return got, state


def test_auto_above_the_threshold_makes_the_calls_of_the_default(recorder, monkeypatch):
    rec = recorder({})
    monkeypatch.setattr(F, "STREAM_FUSED_AUTO_MAX_TC", 4)
    above, s_auto = _lists(rec, "auto", (5, 9, 40))
    plain, s_plain = _lists(rec, False, (5, 9, 40))
    assert above == plain and all(PLAN not in _entries(c) and ENTRY not in _entries(c) for c in above)
    assert (s_auto.head, s_auto.seen) == (s_plain.head, s_plain.seen)
    # at and below it the step is fused (the plan of the recorder accepts)
    below, _ = _lists(rec, "auto", (1, 4))
    assert all(_entries(c) == [PLAN, "fold_weight", ENTRY] for c in below)
    # bf16 parameters and a one-tap layer take the default route under "auto", whatever the threshold
    bf, _ = _lists(rec, "auto", (2, 3), dt=BF)
    bf_plain, _ = _lists(rec, False, (2, 3), dt=BF)
    assert bf == bf_plain and all(PLAN not in _entries(c) for c in bf)
    _, _, one_tap = _fused(rec, _op("plain"), torch.randn(2, N_V, 3, 4), torch.randn(3, 1, 4, 8), None, 0, None, 1, fused="auto")
    assert "cheb_project_series_conv" in _entries(one_tap) and PLAN not in _entries(one_tap)
    # the constant that ships: what the measured table gave (DESIGN.md 3.10 "One launch per step")
    monkeypatch.undo()
    assert isinstance(F.STREAM_FUSED_AUTO_MAX_TC, int) and F.STREAM_FUSED_AUTO_MAX_TC >= 0


def test_auto_with_a_plan_that_refuses_makes_the_calls_of_the_default(recorder, refusing, monkeypatch):
    monkeypatch.setattr(F, "STREAM_FUSED_AUTO_MAX_TC", 64)
    plain, s_plain = _lists(recorder({}), False, (1, 5, 9))
    rec = refusing()
    auto, s_auto = _lists(rec, "auto", (1, 5, 9))
    assert auto == plain and rec.plans == 3
    assert (s_auto.head, s_auto.seen) == (s_plain.head, s_plain.seen) == (3, 15)
    assert not F.stream_fused_supported(_op("plain"), 4, 3, 8, 3, 5, 2, 0) and rec.plans == 4


def test_every_fused_refusal_comes_before_anything_is_built_or_launched(recorder, refusing, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    chunk = torch.randn(2, N_V, 5, 4)
    h, c = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3), tgcn_amd.ChebTimeConv(4, 8, 3, 3)
    with torch.no_grad():
        _, s_h = h.forward_stream(chunk, dilation=2, fused=True)
    before = (s_h.head, s_h.seen, s_h.ring.clone())
    del rec.calls[:]
    _no_operands(monkeypatch)
    with torch.no_grad():
        # bfloat16 parameters, a one-tap layer, a value that is no choice: no operand is needed, none is built
        for layer, extra in ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3).to(BF), ()), (tgcn_amd.ChebTimeConv(4, 8, 3, 3).to(BF), (ei,))):
            with pytest.raises(_lib.TgcnError, match="float32 only"):
                layer.forward_stream(chunk.to(BF), *extra, fused=True)
        for layer, extra in ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 1), ()), (tgcn_amd.ChebTimeConv(4, 8, 3, 1), (ei,))):
            with pytest.raises(_lib.TgcnError, match="one-tap"):
                layer.forward_stream(chunk, *extra, fused=True)
        for bad in (1, 0, None, "yes", "AUTO"):
            with pytest.raises(_lib.TgcnError, match="fused is False, True"):
                h.forward_stream(chunk, fused=bad)
            with pytest.raises(_lib.TgcnError, match="fused is False, True"):
                c.forward_stream(chunk, ei, fused=bad)
        with pytest.raises(_lib.TgcnError, match="float32 only"):
            F.cheb_time_stream(_op("plain"), chunk.to(BF), torch.randn(3, 3, 4, 8).to(BF), None, F.BIAS_NONE, 0, fused=True)
        with pytest.raises(_lib.TgcnError, match="one-tap"):
            F.cheb_time_stream(_op("plain"), chunk, torch.randn(3, 1, 4, 8), None, F.BIAS_NONE, 0, fused=True)
        # a non-square operand: refused on the operand's shape, before the plan is asked
        with pytest.raises(_lib.TgcnError, match="square operand"):
            F.cheb_time_stream(_Op(N_V, 256, n_cols=N_V + 1), chunk, torch.randn(3, 3, 4, 8), None, F.BIAS_NONE, 0, fused=True)
        assert not F.stream_fused_supported(_Op(N_V, 256, n_cols=N_V + 1), 4, 3, 8, 3, 5, 1, 0)
        assert not F.stream_fused_supported(_op("plain"), 4, 1, 8, 3, 5, 1, 0)
    assert rec.calls == []
    # a plan that refuses: the query is asked, nothing is launched, no state is made and the offered one is left alone
    rrec = refusing()
    with torch.no_grad():
        with pytest.raises(_lib.TgcnError, match="do not fit the one-launch step"):
            F.cheb_time_stream(_op("plain"), chunk, torch.randn(3, 3, 4, 8), None, F.BIAS_NONE, 0, fused=True)
        with pytest.raises(_lib.TgcnError, match="do not fit the one-launch step"):
            F.cheb_time_stream(s_h.op, chunk, h.weight, None, F.BIAS_NONE, 0, s_h, 2, fused=True)
    assert rrec.calls == [] and rrec.plans == 2
    assert (s_h.head, s_h.seen) == before[:2] and torch.equal(s_h.ring, before[2])


def test_fused_and_unfused_calls_alternate_on_one_state(recorder):
    rec = recorder({})
    torch.manual_seed(2)
    W, op, d, H = torch.randn(3, 3, 4, 8), _op("plain"), 4, 3
    Cr = (H - 1) * d
    state, head, seen = None, 0, 0
    for i, Tc in enumerate(CHUNKS):
        fused = i % 2 == 0
        _, state, calls = _fused(rec, op, torch.randn(2, N_V, Tc, 4), W, None, 1, state, d, fused=fused)
        ent = _entries(calls)
        assert (ent[-1] == ENTRY and PLAN in ent) if fused else (ent[-1] == "cheb_project_series_stream" and PLAN not in ent)
        assert calls[-1].split()[-2:] == [str(head), str(d)]        # both entries end on head and dilation
        head, seen = (head + Tc) % Cr, seen + Tc
        assert (state.head, state.seen) == (head, seen)
    # and the default route is untouched by the keyword's presence: the same list with and without it
    a, _ = _lists(rec, False, (3, 8))
    b = []
    st = None
    torch.manual_seed(1)
    W2, bias2 = torch.randn(3, 3, 4, 8), torch.randn(8)
    for Tc in (3, 8):
        _, st, calls = _stream(rec, op, torch.randn(2, N_V, Tc, 4), W2, bias2, 0, st, 2)
        b.append(calls)
    assert a == b


def test_the_fused_entries_are_declared_everywhere():
    names = ["tgcn_cheb_stream_small_plan", "tgcn_cheb_stream_small_f32"]
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "tgcn_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert nm in _lib.SIGNATURES and hasattr(handle, nm) and (" " + nm + "(") in header, nm
    L = _lib.lib()
    assert L.tgcn_abi_version() == 8 == _lib.ABI_VERSION and "#define TGCN_ABI_VERSION 8" in header
    # the plan is a host query: it answers without a device.  n nnz mode f H N K Tc dilation
    tb, dense, lds = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)

    def plan(n=48, nnz=300, mode=0, f=4, H=3, N=8, K=3, Tc=70, d=1):
        return L.tgcn_cheb_stream_small_plan(n, nnz, mode, f, H, N, K, Tc, d, ctypes.byref(tb), ctypes.byref(dense), ctypes.byref(lds))
    assert plan() == 0 and 1 <= tb.value <= 70 and dense.value == 0 and 0 < lds.value <= 160 * 1024
    assert plan(n=1025) == -4 and plan(n=1024, nnz=8000, f=64, mode=1) == -4          # too many vertices; buffers past the LDS at tb = 1
    assert plan(n=148, nnz=148 * 147, f=32, N=64, K=10, H=5, Tc=1) == 0 and dense.value == 1 and tb.value == 1      # the DTI parcels: dense only
    assert plan(n=784, nnz=784 * 9, f=1, N=32, K=10, H=5, Tc=8) == 0 and dense.value == 0                           # the 28 x 28 grid: sparse only
    assert plan(f=0) == -1 and plan(Tc=0) == -1 and plan(d=0) == -1 and plan(mode=2) == -1
    one = ctypes.c_void_p(16)       # a non-null pointer that the refused calls never read
    A = _lib.CsrStruct(48, 300, 16, 16, None)

    def entry(Tc=5, H=3, ring_ld=32, head=0, dil=4, pos=None):
        return L.tgcn_cheb_stream_small_f32(None, ctypes.byref(A), 0, 2, Tc, 4, H, 8, 3, one, one, None, 0, one, one, ring_ld, head, pos, dil)
    assert entry(head=8) == -1 and entry(head=-1) == -1 and entry(Tc=0) == -1 and entry(dil=0) == -1 and entry(ring_ld=31) == -1
    assert entry(H=1, ring_ld=0) == -1
    A.n = 1025
    assert entry() == -4


def test_small_stream_kernel_uses_no_scratch_and_spills_nothing():
    sys.path.insert(0, os.path.join(os.path.dirname(_lib.__file__), "..", "tools"))
    try:
        from kernel_resources import demangle, kernel_resources
    finally:
        sys.path.pop(0)
    res = kernel_resources(_lib.LIB_PATH)
    names = sorted(res)
    mine = [nm for nm, pretty in zip(names, demangle(names)) if "small_stream_kernel" in pretty]
    assert len(mine) == 12, mine        # the dense and the sparse carve-up x 1 / 2 / 4 column tiles per wave x the two recurrences
    for nm in mine:
        r = res[nm]
        print(nm, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (nm, r)
        assert r.get("uses_dynamic_stack") in (None, 0, "false") and r.get("max_flat_workgroup_size") == 1024
