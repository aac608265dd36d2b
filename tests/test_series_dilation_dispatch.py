"""CPU test of the launches of the streaming time-window entries with dilated taps (the recorder technique of tests/test_layer_dispatch.py):
dilation=1, however it is spelled, makes exactly the calls of a call without the argument; dilation > 1 asks the step-1 plan first and once,
then launches the `_dilated` entries with the scalars that were passed -- a single-channel window-major series included, in fp32 and bf16;
the geometry rules run on the span He = (H - 1) * dilation + 1; every invalid value raises TgcnError with nothing launched and no operand
built."""
import contextlib

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F
from tgcn_amd.graph import GraphOperand

from test_layer_dispatch import N_V, T_WIN, _Op, _op, recorder  # noqa: F401  (the recorder fixture)
from test_series_conv_dispatch import GEOMETRIES

BF = torch.bfloat16


def _entries(calls):
    return [c.split()[0] for c in calls]


def _call(rec, series, W, mode, train, as_series=False, **geo):
    """the calls one F.cheb_time_windows (and its backward when train) logs"""
    del rec.calls[:]
    torch.manual_seed(1)
    series, W = series.clone(), W.clone()
    bias = torch.randn(W.shape[-1]).to(W.dtype)
    for t in (series, W, bias):
        t.requires_grad_(train)
    with (contextlib.nullcontext() if train else torch.no_grad()):
        out = F.cheb_time_windows(_op("plain"), series, W, bias, F.BIAS_CHANNEL, mode, as_series=as_series, **geo)
    if train:
        out.backward(torch.ones_like(out))
        assert all(t.grad is not None and t.grad.shape == t.shape for t in (series, W, bias))
    return out, list(rec.calls)


# the default geometry and every geometry of tests/test_series_conv_dispatch.py
ALL_GEOMETRIES = [dict()] + [dict(stride=g[0][0], padding=g[0][1]) for g in GEOMETRIES]


@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
@pytest.mark.parametrize("f", [1, 4])
@pytest.mark.parametrize("geo", ALL_GEOMETRIES, ids=[str(tuple(g.values())) for g in ALL_GEOMETRIES])
def test_dilation_one_spelled_out_makes_the_same_calls(geo, f, as_series, train, recorder):
    rec = recorder({})
    torch.manual_seed(0)
    series, W = (torch.randn(2, N_V, T_WIN), torch.randn(3, 6, 8)) if f == 1 else (torch.randn(2, N_V, T_WIN, f), torch.randn(3, 6, f, 8))
    out, plain = _call(rec, series, W, 0, train, as_series, **geo)
    assert plain and not any("_dilated" in c for c in plain)
    out2, calls = _call(rec, series, W, 0, train, as_series, dilation=1, **geo)
    assert calls == plain and out2.shape == out.shape
    if not geo:       # the three spellings of the default geometry with the dilation next to them
        for g in (dict(stride=1, padding=0), dict(padding=(0, 0)), dict(stride=1, padding=[0, 0])):
            out2, calls = _call(rec, series, W, 0, train, as_series, dilation=1, **g)
            assert calls == plain and out2.shape == out.shape, g


def test_dilation_one_on_the_modules_and_in_bf16_makes_the_same_calls(recorder, monkeypatch):
    rec = recorder({})
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda *a, **k: _Op(N_V, 256)))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: _Op(N_V, 256)))
    for dt in (torch.float32, BF):
        series = torch.randn(2, N_V, T_WIN, 4).to(dt)
        for layer, extra in ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 6).to(dt), ()),
                             (tgcn_amd.ChebTimeConv(4, 8, 3, 6).to(dt), (torch.tensor([[0, 1], [1, 0]]),))):
            for geo in (dict(), dict(stride=2, padding="causal"), dict(as_series=True, padding=(1, 2))):
                del rec.calls[:]
                a = layer.forward_series(series, *extra, **geo)
                plain = list(rec.calls)
                del rec.calls[:]
                b = layer.forward_series(series, *extra, dilation=1, **geo)
                assert plain and list(rec.calls) == plain and a.shape == b.shape and not any("_dilated" in c for c in plain)


# (padding, (left, right)) at H = 3, dilation = 3: He = 7
DILATED = [(0, (0, 0)), ("causal", (6, 0)), ((2, 5), (2, 5)), (6, (6, 6))]


@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
@pytest.mark.parametrize("mode", [0, 1], ids=["power", "chebyshev"])
@pytest.mark.parametrize("padding,pads", DILATED, ids=[str(d[0]) for d in DILATED])
def test_dilation_three_launches_the_dilated_entries(padding, pads, mode, as_series, train, recorder):
    rec = recorder({})
    S, T, H, f, N, K, d = 3, T_WIN, 3, 4, 8, 3, 3
    left, right = pads
    nwin = T + left + right - ((H - 1) * d + 1) + 1
    torch.manual_seed(0)
    out, calls = _call(rec, torch.randn(S, N_V, T, f), torch.randn(K, H, f, N), mode, train, as_series, padding=padding, dilation=d)
    assert tuple(out.shape) == ((S, N_V, nwin, N) if as_series else (S * nwin, N_V, N))
    ent = _entries(calls)
    allowed = {"series_conv_plan", "cheb_project_series_dilated", "cheb_series_dilated_backward", "csr_hop2", "fold_weight"}
    assert set(ent) <= allowed, ent
    # the regime query comes first (host only, before the hops) and once, at step 1 whatever the dilation: H f N vec 1
    assert calls[0] == "series_conv_plan %d %d %d 1 1" % (H, f, N) and ent.count("series_conv_plan") == 1
    # scalars of the entry: S n T f H N K bias_kind as_series stride pad_left pad_right dilation
    assert [c for c in calls if c.startswith("cheb_project_series_dilated ")] == [
        "cheb_project_series_dilated %d %d %d %d %d %d %d 1 %d 1 %d %d %d" % (S, N_V, T, f, H, N, K, int(as_series), left, right, d)]
    back = [c for c in calls if c.startswith("cheb_series_dilated_backward ")]
    assert back == (["cheb_series_dilated_backward %d %d %d %d %d %d %d %d 1024 1 %d %d %d" % (S, N_V, T, f, H, N, K, int(as_series), left, right, d)]
                    if train else [])
    # the hops do not depend on the dilation: K - 1 per direction on rows of T*f floats
    hops = [c for c in calls if c.startswith("csr_hop2 ")]
    assert len(hops) == (K - 1) * (2 if train else 1) and all(c.split()[1:3] == [str(S), str(T * f)] for c in hops)
    # order: plan, the forward's hops, the forward entry; the backward entry before the adjoint hops
    i_fwd = ent.index("cheb_project_series_dilated")
    assert ent[:i_fwd].count("csr_hop2") == K - 1
    if train:
        assert "csr_hop2" not in ent[i_fwd + 1:ent.index("cheb_series_dilated_backward")]
    assert ("fold_weight" in ent) == (mode == 0)


@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("four_d", [False, True], ids=["3d", "4d_f1"])
def test_single_channel_window_major_takes_the_dilated_entries(four_d, train, recorder):
    """f == 1 with as_series=False is the scalar-load form only at the default geometry and dilation 1"""
    rec = recorder({})
    torch.manual_seed(0)
    x, W = torch.randn(2, N_V, T_WIN), torch.randn(3, 4, 8)
    if four_d:
        x, W = x.unsqueeze(3), W.unsqueeze(2)
    out, calls = _call(rec, x, W, 0, train, dilation=2)          # He = 7: 6 windows
    assert tuple(out.shape) == (2 * 6, N_V, 8)
    ent = _entries(calls)
    assert not {"cheb_project_windows", "cheb_windows_backward", "cheb_project_series", "cheb_project_series_conv"} & set(ent)
    assert ent.count("cheb_project_series_dilated") == 1 and ent.count("cheb_series_dilated_backward") == (1 if train else 0)
    assert "cheb_project_series_dilated 2 %d %d 1 4 8 3 1 0 1 0 0 2" % (N_V, T_WIN) in calls


@pytest.mark.parametrize("four_d", [False, True], ids=["3d", "4d_f1"])
def test_single_channel_window_major_takes_the_dilated_entries_in_bf16(four_d, recorder):
    """check_series_bf16 lets a dilation pass as it lets a stride or a padding pass"""
    rec = recorder({})
    torch.manual_seed(0)
    x, W = torch.randn(2, N_V, T_WIN).to(BF), torch.randn(3, 4, 8).to(BF)
    if four_d:
        x, W = x.unsqueeze(3), W.unsqueeze(2)
    out, calls = _call(rec, x, W, 0, True, dilation=2)
    assert out.dtype == BF and tuple(out.shape) == (2 * 6, N_V, 8)
    ent = _entries(calls)
    # the forward's plan and the input gradient's (all H weight time rows of N channels, K*f columns), both at step 1, before the hops
    assert calls[:2] == ["series_conv_plan_bf16 4 1 8 0 1", "series_conv_plan_bf16 4 8 3 1 1"] and ent.count("series_conv_plan_bf16") == 2
    # stack_ld = 16: rows of T*f = 12 elements padded up to a multiple of 8
    assert "cheb_project_series_dilated_bf16 2 %d %d 1 4 8 3 16 1 1 0 1 0 0 2" % (N_V, T_WIN) in calls
    assert "cheb_series_dilated_backward_bf16 2 %d %d 1 4 8 3 16 0 1024 1 0 0 2" % (N_V, T_WIN) in calls
    assert ent.count("cheb_project_series_dilated_bf16") == 1 and ent.count("cheb_series_dilated_backward_bf16") == 1
    assert not any("_series" in e and not e.endswith("_bf16") for e in ent)
    # the default geometry at dilation 1 stays refused
    with pytest.raises(_lib.TgcnError, match="as_series=True"):
        F.cheb_time_windows(_op("plain"), x, W, None, F.BIAS_NONE, 0, dilation=1)


def test_series_geometry_values():
    assert F.series_geometry(50, 5, dilation=3) == (1, 0, 0, 38)
    assert F.series_geometry(50, 5, 1, "causal", dilation=3) == (1, 12, 0, 50)
    assert F.series_geometry(20, 3, dilation=9) == (1, 0, 0, 2)
    with pytest.raises(_lib.TgcnError):
        F.series_geometry(12, 5, dilation=3)
    # the return value stays the 4-tuple; the padding rules run on He = 13
    assert F.series_geometry(50, 5, 1, (12, 12), dilation=3) == (1, 12, 12, 62)
    assert F.series_geometry(12, 5, 1, 1, dilation=3) == (1, 1, 1, 2)
    assert F.series_geometry(50, 5, 2, 4) == (2, 4, 4, 27)


# H = 3 taps on 8 time steps; dilation 2: He = 5.  Each case with the rule that has to refuse it (a part of its message)
PAD, INT, STEP, SHORT = r"padding \(\d+, \d+\) outside", "dilation is an integer >= 1", "together with stride", "fewer than one window"
BAD = [(dict(dilation=2, padding=5), PAD), (dict(dilation=2, padding=(5, 0)), PAD), (dict(dilation=2, padding=(0, 5)), PAD),
       (dict(dilation=0), INT), (dict(dilation=-1), INT), (dict(dilation=True), INT), (dict(dilation=2.0), INT), (dict(dilation="2"), INT),
       (dict(dilation=None), INT), (dict(stride=2, dilation=2), STEP), (dict(stride=3, dilation=2, padding=4), STEP),
       (dict(dilation=5), SHORT), (dict(dilation=4, padding=(0, 0)), SHORT)]


@pytest.mark.parametrize("geo,rule", BAD, ids=[str(b[0]) for b in BAD])
def test_invalid_dilation_raises_before_anything_is_built_or_launched(geo, rule, recorder, monkeypatch):
    """a padding of He, dilations that are no integer >= 1, a dilation with a window step, a span longer than the series -- each refused by its
    own rule"""
    rec = recorder({})
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda L, device: pytest.fail("operand built")))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: pytest.fail("operand built")))
    ei = torch.tensor([[0, 1], [1, 0]])
    h = tgcn_amd.TGCNCheb_H(torch.eye(8), 4, 3, 3, 3)
    c = tgcn_amd.ChebTimeConv(4, 3, 3, 3)
    for dt in (torch.float32, BF):
        series = torch.randn(2, 8, 8, 4).to(dt)
        for as_series in (False, True):
            with pytest.raises(_lib.TgcnError, match=rule):
                h.to(dt).forward_series(series, as_series=as_series, **geo)
            with pytest.raises(_lib.TgcnError, match=rule):
                c.to(dt).forward_series(series, ei, as_series=as_series, **geo)
            with pytest.raises(_lib.TgcnError, match=rule):
                F.cheb_time_windows(_op("plain"), torch.randn(2, N_V, 8, 4).to(dt), torch.randn(3, 3, 4, 8).to(dt), None, F.BIAS_NONE, 0,
                                    as_series=as_series, **geo)
    with pytest.raises(_lib.TgcnError, match=rule):
        F.series_geometry(8, 3, geo.get("stride", 1), geo.get("padding", 0), dilation=geo["dilation"])
    assert rec.calls == []


HUGE = [2, 2 ** 26, 2 ** 30, 2 ** 31 - 1]


@pytest.mark.parametrize("dilation", HUGE)
@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
def test_one_tap_has_nothing_to_dilate(dt, dilation, recorder, monkeypatch):
    """H == 1: the span is 1 whatever the dilation, so nothing bounds the value -- the call is the call at dilation 1, nothing dilated is
    launched, and the C entries' host checks agree (their workspace query answers as the _conv query; no value reaches a kernel's 32-bit window
    arithmetic)"""
    rec = recorder({})
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda *a, **k: _Op(N_V, 256)))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: _Op(N_V, 256)))
    assert F.series_geometry(50, 1, dilation=dilation) == (1, 0, 0, 50) and F.series_dilation(1, dilation) == 1 and F.series_dilation(2, 7) == 7
    series = torch.randn(2, N_V, T_WIN, 4).to(dt)
    for layer, extra in ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 1).to(dt), ()),
                         (tgcn_amd.ChebTimeConv(4, 8, 3, 1).to(dt), (torch.tensor([[0, 1], [1, 0]]),))):
        for kw in (dict(), dict(as_series=True)):
            del rec.calls[:]
            a = layer.forward_series(series, *extra, **kw)
            plain = list(rec.calls)
            del rec.calls[:]
            b = layer.forward_series(series, *extra, dilation=dilation, **kw)
            assert plain and list(rec.calls) == plain and a.shape == b.shape and not any("_dilated" in c for c in plain)
        with pytest.raises(_lib.TgcnError, match="together with stride"):          # a step stays refused at any dilation > 1
            layer.forward_series(series, *extra, stride=2, dilation=dilation)


@pytest.mark.parametrize("dilation", HUGE)
def test_one_tap_through_the_c_entries_host_checks(dilation):
    """the real library, host only: the workspace queries of the _dilated entries at H == 1 answer as the _conv queries (the entries take the
    same branch), and with a step they refuse"""
    L = _lib.lib()
    dims = (2, 48, 50, 4, 1, 8, 3)
    for q, conv in ((L.tgcn_cheb_series_dilated_backward_workspace_bytes, L.tgcn_cheb_series_conv_backward_workspace_bytes),
                    (L.tgcn_cheb_series_dilated_backward_bf16_workspace_bytes, L.tgcn_cheb_series_conv_backward_bf16_workspace_bytes)):
        assert q(*dims, 1, 0, 0, dilation) == conv(*dims, 1, 0, 0) > 0
        assert q(*dims, 2, 0, 0, dilation) == 0 and q(*dims, 1, 1, 0, dilation) == 0          # a step; a padding of He = 1


def test_a_padding_of_one_less_than_the_span_runs(recorder, monkeypatch):
    rec = recorder({})
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda *a, **k: _Op(N_V, 256)))
    h = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 3, 3, 3)
    assert tuple(h.forward_series(torch.randn(2, N_V, 10, 4), padding=4, dilation=2).shape) == (2 * 14, N_V, 3)
    assert tuple(h.forward_series(torch.randn(2, N_V, 10, 4), padding="causal", dilation=2, as_series=True).shape) == (2, N_V, 10, 3)
    assert tuple(h.forward_series(torch.randn(2, N_V, 1, 4), padding="causal", dilation=4, as_series=True).shape) == (2, N_V, 1, 3)
    assert _entries(rec.calls).count("cheb_project_series_dilated") == 3


def test_learnable_edge_weights_and_other_series_dtypes_stay_refused(recorder, monkeypatch):
    rec = recorder({})
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda L, device: pytest.fail("operand built")))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: pytest.fail("operand built")))
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(_lib.TgcnError):
        tgcn_amd.ChebTimeConv(4, 3, 3, 3).forward_series(torch.randn(2, 8, 10, 4), ei, torch.ones(2, requires_grad=True), dilation=2)
    with pytest.raises(_lib.TgcnError, match="cast it once"):
        tgcn_amd.TGCNCheb_H(torch.eye(8), 4, 3, 3, 3).to(BF).forward_series(torch.randn(2, 8, 10, 4), as_series=True, dilation=2)
    with pytest.raises(_lib.TgcnError, match="cast it once"):
        tgcn_amd.ChebTimeConv(4, 3, 3, 3).to(BF).forward_series(torch.randn(2, 8, 10, 4), ei, dilation=2)
    assert rec.calls == []


def test_the_new_entries_are_declared_everywhere():
    """the header, the ctypes table and the library agree on the six entries"""
    import ctypes
    import os
    names = ["tgcn_cheb_project_series_dilated_f32", "tgcn_cheb_series_dilated_backward_workspace_bytes", "tgcn_cheb_series_dilated_backward_f32",
             "tgcn_cheb_project_series_dilated_bf16", "tgcn_cheb_series_dilated_backward_bf16_workspace_bytes",
             "tgcn_cheb_series_dilated_backward_bf16"]
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "tgcn_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert nm in _lib.SIGNATURES and hasattr(handle, nm) and (" " + nm + "(") in header, nm
    # host-only argument checks of the workspace query: the _conv answer at dilation 1, 0 for what Python refuses
    L = _lib.lib()
    q, conv = L.tgcn_cheb_series_dilated_backward_workspace_bytes, L.tgcn_cheb_series_conv_backward_workspace_bytes
    assert q(2, 48, 50, 4, 5, 8, 3, 2, 1, 2, 1) == conv(2, 48, 50, 4, 5, 8, 3, 2, 1, 2) > 0
    assert q(2, 48, 50, 4, 5, 8, 3, 1, 12, 0, 3) > 0
    assert q(2, 48, 50, 4, 5, 8, 3, 1, 13, 0, 3) == 0 and q(2, 48, 50, 4, 5, 8, 3, 2, 0, 0, 3) == 0 and q(2, 48, 50, 4, 5, 8, 3, 1, 0, 0, 0) == 0
    assert q(2, 48, 12, 4, 5, 8, 3, 1, 0, 0, 3) == 0
