"""CPU test of the launches of the one-launch whole-series layer (forward_series / F.cheb_time_windows with fused=...), by the recorder
technique of tests/test_series_stream_fused_dispatch.py.  Without the keyword and with fused=False a call logs exactly what it logged
before the keyword existed.  fused=True asks tgcn_cheb_series_small_plan once and first, folds the weight at most once and launches
tgcn_cheb_series_small_f32 -- no hop, no project_series entry -- with a stack pointer only when the weight trains; its backward is the
existing series backward entry of the geometry.  Every refusal raises TgcnError with nothing launched, and without an operand where none
is needed; fused="auto" makes the default's calls on each of them.  The two entries are in the header, the ctypes table and the library at
ABI 8, the plan answers as a host query, and small_series_kernel's instantiations use no scratch and spill nothing."""
import contextlib
import ctypes
import os
import sys

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F

from test_layer_dispatch import N_V, _Op, _op, _Recorder, recorder  # noqa: F401  (the recorder fixture)
from test_series_stream_dispatch import BF, _entries, _no_operands, _stub_operands

PLAN, ENTRY = "cheb_series_small_plan", "cheb_series_small"
STACK_ARG = 15      # position of `stack` among tgcn_cheb_series_small_f32's arguments
T = 20
GEOMETRIES = {"default": dict(), "conv": dict(stride=2, padding=(1, 2)), "causal": dict(padding="causal"), "dilated": dict(padding=(1, 3), dilation=2)}
EI = torch.tensor([[0, 1], [1, 0]])


def _layers(f, K=3, H=3, N=8):
    return ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), f, N, K, H), (), 0), (tgcn_amd.ChebTimeConv(f, N, K, H), (EI,), 1))


def _series(f, S=2):
    torch.manual_seed(3)
    x = torch.randn(S, N_V, T, f)
    return x[..., 0] if f == 1 else x


def _module_call(rec, layer, extra, series, train, **kw):
    """the calls one forward_series (and its backward when train) logs"""
    del rec.calls[:], rec.nulls[:]
    series = series.clone().requires_grad_(train)
    with (contextlib.nullcontext() if train else torch.no_grad()):
        out = layer.forward_series(series, *extra, **kw)
    if train:
        out.backward(torch.ones_like(out))
    return out, list(rec.calls)


@pytest.mark.parametrize("train", [False, True], ids=["no-grad", "train"])
@pytest.mark.parametrize("geometry", ["default", "conv", "dilated"])
@pytest.mark.parametrize("f", [1, 4])
def test_the_default_launch_list_is_unchanged(f, geometry, train, recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    for layer, extra, _ in _layers(f):
        for as_series in (False, True):
            kw = dict(GEOMETRIES[geometry], as_series=as_series)
            _, omitted = _module_call(rec, layer, extra, _series(f), train, **kw)
            _, off = _module_call(rec, layer, extra, _series(f), train, fused=False, **kw)
            assert omitted and omitted == off
            assert PLAN not in _entries(omitted) and ENTRY not in _entries(omitted)
            # "auto" outside the measured rule is that call too, launch for launch, and asks no plan
            measured = f == 1 and not as_series and geometry == "default"
            with monkeypatch.context() as m:
                if measured:
                    m.setattr(F, "SERIES_FUSED_AUTO", ())
                assert _module_call(rec, layer, extra, _series(f), train, fused="auto", **kw)[1] == omitted
    # and through the functional entry
    op, W, x = _op("plain"), torch.randn(3, 3, 4, 8), torch.randn(2, N_V, T, 4)
    lists = []
    for kw in (dict(), dict(fused=False)):
        del rec.calls[:]
        with torch.no_grad():
            F.cheb_time_windows(op, x, W, None, F.BIAS_NONE, 1, **dict(GEOMETRIES[geometry], **kw))
        lists.append(list(rec.calls))
    assert lists[0] == lists[1] and lists[0]


BACKWARD = {"default": "cheb_series_backward", "causal": "cheb_series_conv_backward", "dilated": "cheb_series_dilated_backward"}


@pytest.mark.parametrize("geometry", ["default", "causal", "dilated"])
@pytest.mark.parametrize("f", [1, 4])
def test_a_fused_call_logs_the_plan_at_most_one_fold_and_the_fused_entry(f, geometry, recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    geo = GEOMETRIES[geometry]
    K, H, N, S = 3, 3, 8, 2
    _, left, right, nwin = F.series_geometry(T, H, 1, geo.get("padding", 0), dilation=geo.get("dilation", 1))
    d = geo.get("dilation", 1)
    for layer, extra, mode in _layers(f, K, H, N):
        folds = 1 if mode == 0 else 0          # power mode with K > 2
        bias_kind = 2 if mode == 0 else 1
        for as_series in (False, True):
            kw = dict(geo, as_series=as_series, fused=True)
            want = "%s %d %d %d %d %d %d %d %d %d %d %d %d" % (ENTRY, mode, S, T, f, H, N, K, bias_kind, int(as_series), left, right, d)
            shape = (S, N_V, nwin, N) if as_series else (S * nwin, N_V, N)
            # no grad: the plan first, the fold, the entry; no stack
            out, calls = _module_call(rec, layer, extra, _series(f), False, **kw)
            assert tuple(out.shape) == shape and out.dtype == torch.float32 and out.is_contiguous()
            assert calls[0] == "%s %d %d %d %d %d %d %d %d %d %d %d" % (PLAN, N_V, 256, mode, f, H, N, K, T, left, right, d)
            assert _entries(calls) == [PLAN] + ["fold_weight"] * folds + [ENTRY] and calls[-1] == want
            assert STACK_ARG in rec.nulls[-1]
            # training: a stack, then the existing backward entry of the geometry and the adjoint hops
            out, calls = _module_call(rec, layer, extra, _series(f), True, **kw)
            ent = _entries(calls)
            i = ent.index(ENTRY)
            assert ent[:i + 1] == [PLAN] + ["fold_weight"] * folds + [ENTRY] and calls[i] == want and STACK_ARG not in rec.nulls[i]
            assert ent.count(BACKWARD[geometry]) == 1 and ent.index(BACKWARD[geometry]) > i
            assert not any(e.startswith("cheb_project_series") or e == "series_conv_plan" for e in ent)
            assert not any(e.startswith("csr_hop") for e in ent[:ent.index(BACKWARD[geometry])])       # the forward hops nothing
            assert sum(e.startswith("csr_hop") for e in ent) == K - 1                                   # the adjoint hops of d series
            # a frozen weight: no stack, and the backward entry still gives d series
            layer.weight.requires_grad_(False)
            out, calls = _module_call(rec, layer, extra, _series(f), True, **kw)
            layer.weight.requires_grad_(True)
            ent = _entries(calls)
            assert STACK_ARG in rec.nulls[ent.index(ENTRY)] and ent.count(BACKWARD[geometry]) == 1


class _RefusingRecorder(_Recorder):
    """the recorder with a plan that answers TGCN_ERR_UNSUPPORTED; the refused query is counted, not logged as a launch"""

    def __init__(self, small):
        super().__init__(small)
        self.plans = 0

    def __getattr__(self, name):
        if name == "tgcn_cheb_series_small_plan":
            def plan(*args):
                self.plans += 1
                return -4
            return plan
        if name == "tgcn_last_error":
            return lambda: b"series_small_plan: does not fit"
        return super().__getattr__(name)


def _functional(rec, op, series, W, fused, **kw):
    del rec.calls[:]
    with torch.no_grad():
        F.cheb_time_windows(op, series, W, None, F.BIAS_NONE, 1, fused=fused, **kw)
    return list(rec.calls)


def test_every_fused_refusal_comes_before_anything_is_built_or_launched(recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    x = _series(4)
    layers = _layers(4)
    for layer, extra, _ in layers:          # every operand cached, so that "auto" below builds none either
        _module_call(rec, layer, extra, x, False)
    bf_layers = [(l.to(BF), e, m) for l, e, m in _layers(4)]
    for layer, extra, _ in bf_layers:
        _module_call(rec, layer, extra, x.to(BF), False)
    default = {}
    for tag, kw in (("stride", dict(stride=2)), ("chunk", dict(padding="causal", time_chunk=4))):
        default[tag] = [_module_call(rec, layer, extra, x, False, **kw)[1] for layer, extra, _ in layers]
    default["bf16"] = [_module_call(rec, layer, extra, x.to(BF), False)[1] for layer, extra, _ in bf_layers]
    del rec.calls[:]
    _no_operands(monkeypatch)
    with torch.no_grad():
        for i, (layer, extra, _) in enumerate(layers):
            with pytest.raises(_lib.TgcnError, match="stride=1"):
                layer.forward_series(x, *extra, stride=2, fused=True)
            with pytest.raises(_lib.TgcnError, match="time chunks"):
                layer.forward_series(x, *extra, padding="causal", time_chunk=4, fused=True)
            for bad in ("yes", 1, 0, None, "AUTO"):
                with pytest.raises(_lib.TgcnError, match="fused is False, True"):
                    layer.forward_series(x, *extra, fused=bad)
        for layer, extra, _ in bf_layers:
            with pytest.raises(_lib.TgcnError, match="float32 only"):
                layer.forward_series(x.to(BF), *extra, fused=True)
        W = torch.randn(3, 3, 4, 8)
        with pytest.raises(_lib.TgcnError, match="float32 only"):
            F.cheb_time_windows(_op("plain"), x.to(BF), W.to(BF), None, F.BIAS_NONE, 0, fused=True)
        with pytest.raises(_lib.TgcnError, match="stride=1"):
            F.cheb_time_windows(_op("plain"), x, W, None, F.BIAS_NONE, 0, stride=2, fused=True)
        with pytest.raises(_lib.TgcnError, match="time chunks"):
            F.cheb_time_windows(_op("plain"), x, W, None, F.BIAS_NONE, 0, padding="causal", time_chunk=4, fused=True)
        with pytest.raises(_lib.TgcnError, match="fused is False, True"):
            F.cheb_time_windows(_op("plain"), x, W, None, F.BIAS_NONE, 0, fused="yes")
        # the operand's own rules: refused on its shape and labels, before the plan is asked
        with pytest.raises(_lib.TgcnError, match="square operand"):
            F.cheb_time_windows(_Op(N_V, 256, n_cols=N_V + 1), x, W, None, F.BIAS_NONE, 0, fused=True)
        with pytest.raises(_lib.TgcnError, match="reordered operand"):
            F.cheb_time_windows(_op("reordered"), x, W, None, F.BIAS_NONE, 0, fused=True)
        assert not F.series_fused_supported(_Op(N_V, 256, n_cols=N_V + 1), 4, 3, 8, 3, T, 0, 1, 0)
        assert not F.series_fused_supported(_op("reordered"), 4, 3, 8, 3, T, 0, 1, 0)
        assert not F.series_fused_supported(_op("plain"), 4, 3, 8, 3, T, 3, 1, 0)       # a pad above H - 1: no query either
        assert rec.calls == []
        # "auto" on each of them makes the default's calls (the operands are cached: none is built)
        for i, (layer, extra, _) in enumerate(layers):
            assert _module_call(rec, layer, extra, x, False, stride=2, fused="auto")[1] == default["stride"][i]
            assert _module_call(rec, layer, extra, x, False, padding="causal", time_chunk=4, fused="auto")[1] == default["chunk"][i]
        for i, (layer, extra, _) in enumerate(bf_layers):
            assert _module_call(rec, layer, extra, x.to(BF), False, fused="auto")[1] == default["bf16"][i]
    monkeypatch.setattr(F, "SERIES_FUSED_AUTO", ("windows_f1", "series"))      # inside the rule, so that the operand's rules decide
    auto = _functional(rec, _op("reordered"), x, W, "auto")
    assert auto == _functional(rec, _op("reordered"), x, W, False) and PLAN not in _entries(auto) and ENTRY not in _entries(auto)
    for fused in (False, "auto"):       # a rectangular operand takes no series at all: "auto" ends where the default ends, the plan unasked
        with pytest.raises(AssertionError):
            _functional(rec, _Op(N_V, 256, n_cols=N_V + 1), x, W, fused)
        assert PLAN not in _entries(rec.calls) and ENTRY not in _entries(rec.calls)
    # a plan that refuses: the query is asked, nothing is launched; "auto" inside the measured rule then makes the default's calls
    plain = _functional(rec, _op("plain"), x, W, False)
    rrec = _RefusingRecorder({})
    monkeypatch.setattr(_lib, "lib", lambda: rrec)
    with torch.no_grad():
        with pytest.raises(_lib.TgcnError, match="do not fit the one-launch layer"):
            F.cheb_time_windows(_op("plain"), x, W, None, F.BIAS_NONE, 1, fused=True)
    assert rrec.calls == [] and rrec.plans == 1
    assert not F.series_fused_supported(_op("plain"), 4, 3, 8, 3, T, 0, 1, 0) and rrec.plans == 2
    monkeypatch.setattr(F, "SERIES_FUSED_AUTO", ("windows_f1", "series"))
    assert _functional(rrec, _op("plain"), x, W, "auto") == plain and rrec.plans == 3
    # ... and with a plan that accepts, "auto" inside the rule fuses; outside it (the constant that ships may be "never") it does not ask
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    assert _entries(_functional(rec, _op("plain"), x, W, "auto")) == [PLAN, ENTRY]
    monkeypatch.setattr(F, "SERIES_FUSED_AUTO", ())
    assert _functional(rec, _op("plain"), x, W, "auto") == plain


def test_the_shipped_auto_rule_fuses_the_measured_class_only(recorder, monkeypatch):
    """F.SERIES_FUSED_AUTO names classes of the call's unfused form: "windows_f1" (a single channel, window-major, default geometry: the
    scalar-load form) and "series" (everything else).  What ships is what profiles/r21_series_small.json gave"""
    assert isinstance(F.SERIES_FUSED_AUTO, tuple) and set(F.SERIES_FUSED_AUTO) <= {"windows_f1", "series"}
    rec = recorder({})
    _stub_operands(monkeypatch)
    for layer, extra, mode in _layers(1):
        for kw, cls in ((dict(), "windows_f1"), (dict(as_series=True), "series"), (dict(padding="causal"), "series"), (dict(dilation=2), "series")):
            _, auto = _module_call(rec, layer, extra, _series(1), False, fused="auto", **kw)
            _, on = _module_call(rec, layer, extra, _series(1), False, fused=True, **kw)
            _, off = _module_call(rec, layer, extra, _series(1), False, **kw)
            assert auto == (on if cls in F.SERIES_FUSED_AUTO else off), (kw, cls)
    for layer, extra, mode in _layers(4):
        _, auto = _module_call(rec, layer, extra, _series(4), False, fused="auto")
        assert auto == _module_call(rec, layer, extra, _series(4), False, fused=("series" in F.SERIES_FUSED_AUTO))[1]


def test_the_fused_entries_are_declared_everywhere():
    names = ["tgcn_cheb_series_small_plan", "tgcn_cheb_series_small_f32"]
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "tgcn_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert nm in _lib.SIGNATURES and hasattr(handle, nm) and (" " + nm + "(") in header, nm
    L = _lib.lib()
    assert L.tgcn_abi_version() == 8 == _lib.ABI_VERSION and "#define TGCN_ABI_VERSION 8" in header


def test_the_plan_answers_as_a_host_query():
    L = _lib.lib()
    tb, dense, lds = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)

    def plan(n=48, nnz=300, mode=0, f=4, H=3, N=8, K=3, T=70, left=0, right=0, d=1, res=True):
        return L.tgcn_cheb_series_small_plan(n, nnz, mode, f, H, N, K, T, left, right, d, ctypes.byref(tb) if res else None, ctypes.byref(dense),
                                             ctypes.byref(lds))
    assert plan() == 0 and 1 <= tb.value <= 68 and dense.value == 0 and 0 < lds.value <= 160 * 1024
    # the HCP layer: 148 parcels, dense only, the contiguous span leaves room for a tile next to the operand
    assert plan(n=148, nnz=148 * 147, f=1, H=15, N=32, K=10, T=284) == 0 and dense.value == 1 and tb.value >= 1 and lds.value <= 160 * 1024
    assert plan(n=148, nnz=148 * 147, f=1, H=15, N=32, K=10, T=284, mode=1) == 0 and dense.value == 1
    # the 28 x 28 grid with a 28-tap window: sparse only, one buffer in mode 0
    assert plan(n=784, nnz=784 + 4 * 27 * 28, f=1, H=28, N=64, K=5, T=128) == 0 and dense.value == 0 and tb.value >= 1
    assert lds.value <= 160 * 1024
    assert plan(n=1025) == -4 and plan(nnz=(1 << 20) + 1) == -4 and plan(N=1025) == -4
    assert plan(n=1024, nnz=8000, f=64, mode=1) == -4          # the span buffers past the LDS at tb = 1
    assert plan(f=0) == -1 and plan(n=0) == -1 and plan(H=0) == -1 and plan(N=0) == -1 and plan(K=0) == -1 and plan(T=0) == -1 and plan(d=0) == -1
    assert plan(T=2) == -1 and plan(T=4, d=2) == -1 and plan(T=2, left=1) == 0          # fewer rows than one window; the pad counts
    assert plan(left=3) == -1 and plan(right=3) == -1 and plan(left=-1) == -1 and plan(left=4, d=2) == 0 and plan(left=5, d=2) == -1
    assert plan(mode=2) == -1 and plan(res=False) == -1
    one = ctypes.c_void_p(16)       # a non-null pointer that the refused calls never read
    A = _lib.CsrStruct(48, 300, 16, 16, None)

    def entry(series=one, W=one, out=one, A_=A, S=2, bias_kind=0, left=0, T_=20):
        return L.tgcn_cheb_series_small_f32(None, ctypes.byref(A_) if A_ is not None else None, 0, S, T_, 4, 3, 8, 3, series, W, None, bias_kind, 1,
                                            out, None, left, 0, 1)
    assert entry(series=None) == -1 and entry(W=None) == -1 and entry(out=None) == -1 and entry(A_=None) == -1
    assert entry(S=0) == -1 and entry(bias_kind=1) == -1 and entry(bias_kind=3) == -1 and entry(left=3) == -1 and entry(T_=2) == -1
    A.n = 1025
    assert entry() == -4


def test_small_series_kernel_uses_no_scratch_and_spills_nothing():
    sys.path.insert(0, os.path.join(os.path.dirname(_lib.__file__), "..", "tools"))
    try:
        from kernel_resources import demangle, kernel_resources
    finally:
        sys.path.pop(0)
    res = kernel_resources(_lib.LIB_PATH)
    names = sorted(res)
    mine = [nm for nm, pretty in zip(names, demangle(names)) if "small_series_kernel" in pretty]
    assert len(mine) == 12, mine        # the dense and the sparse carve-up x 1 / 2 / 4 column tiles per wave x the two recurrences
    for nm in mine:
        r = res[nm]
        print(nm, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (nm, r)
        assert r.get("uses_dynamic_stack") in (None, 0, "false") and r.get("max_flat_workgroup_size") == 1024
