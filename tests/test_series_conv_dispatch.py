"""CPU test of the launches of the streaming time-window entries with a window step and zero padding (the recorder technique of
tests/test_layer_dispatch.py): the default geometry, however it is spelled, makes exactly the calls of a call without the arguments; any
other geometry launches the `_conv` entries with the scalars that were passed, a single-channel window-major series included; every invalid
value raises TgcnError with nothing launched and no operand built."""
import contextlib

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F
from tgcn_amd.graph import GraphOperand

from test_layer_dispatch import N_V, T_WIN, _Op, _op, recorder  # noqa: F401  (the recorder fixture)


def _entries(calls):
    return [c.split()[0] for c in calls]


def _call(rec, series, W, mode, train, as_series=False, **geo):
    """the calls one F.cheb_time_windows (and its backward when train) logs"""
    del rec.calls[:]
    torch.manual_seed(1)
    series, W = series.clone(), W.clone()
    bias = torch.randn(W.shape[-1])
    for t in (series, W, bias):
        t.requires_grad_(train)
    with (contextlib.nullcontext() if train else torch.no_grad()):
        out = F.cheb_time_windows(_op("plain"), series, W, bias, F.BIAS_CHANNEL, mode, as_series=as_series, **geo)
    if train:
        out.backward(torch.ones_like(out))
        assert all(t.grad is not None and t.grad.shape == t.shape for t in (series, W, bias))
    return out, list(rec.calls)


@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
@pytest.mark.parametrize("f", [1, 4])
def test_default_geometry_spelled_out_makes_the_same_calls(f, as_series, train, recorder):
    rec = recorder({})
    torch.manual_seed(0)
    series, W = (torch.randn(2, N_V, T_WIN), torch.randn(3, 6, 8)) if f == 1 else (torch.randn(2, N_V, T_WIN, f), torch.randn(3, 6, f, 8))
    out, plain = _call(rec, series, W, 0, train, as_series)
    assert plain and not any("_conv" in c for c in plain)
    for geo in (dict(stride=1, padding=0), dict(padding=(0, 0)), dict(stride=1, padding=[0, 0])):
        out2, calls = _call(rec, series, W, 0, train, as_series, **geo)
        assert calls == plain and out2.shape == out.shape, geo


# (stride, padding) -> (left, right)
GEOMETRIES = [((2, 0), (0, 0)), ((1, 2), (2, 2)), ((3, (1, 4)), (1, 4)), ((2, "causal"), (5, 0)), ((1, "causal"), (5, 0)), ((40, 5), (5, 5))]


@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
@pytest.mark.parametrize("mode", [0, 1], ids=["power", "chebyshev"])
@pytest.mark.parametrize("geo,pads", GEOMETRIES, ids=[str(g[0]) for g in GEOMETRIES])
def test_other_geometries_launch_the_conv_entries(geo, pads, mode, as_series, train, recorder):
    rec = recorder({})
    S, T, H, f, N, K = 3, T_WIN, 6, 4, 8, 3
    (stride, padding), (left, right) = geo, pads
    nwin = (T + left + right - H) // stride + 1
    torch.manual_seed(0)
    out, calls = _call(rec, torch.randn(S, N_V, T, f), torch.randn(K, H, f, N), mode, train, as_series, stride=stride, padding=padding)
    assert tuple(out.shape) == ((S, N_V, nwin, N) if as_series else (S * nwin, N_V, N))
    ent = _entries(calls)
    allowed = {"series_conv_plan", "cheb_project_series_conv", "cheb_series_conv_backward", "csr_hop2", "fold_weight"}
    assert set(ent) <= allowed, ent
    # the regime query comes first (host only, before the hops): H f N vec stride
    assert calls[0] == "series_conv_plan %d %d %d 1 %d" % (H, f, N, stride) and ent.count("series_conv_plan") == 1
    # scalars of the entry: S n T f H N K bias_kind as_series stride pad_left pad_right
    assert [c for c in calls if c.startswith("cheb_project_series_conv ")] == ["cheb_project_series_conv %d %d %d %d %d %d %d 1 %d %d %d %d"
                                                                              % (S, N_V, T, f, H, N, K, int(as_series), stride, left, right)]
    back = [c for c in calls if c.startswith("cheb_series_conv_backward ")]
    assert back == (["cheb_series_conv_backward %d %d %d %d %d %d %d %d 1024 %d %d %d" % (S, N_V, T, f, H, N, K, int(as_series), stride, left, right)]
                    if train else [])
    # the hops do not depend on the geometry: once per direction on rows of T*f floats
    hops = [c for c in calls if c.startswith("csr_hop2 ")]
    assert len(hops) == (K - 1) * (2 if train else 1) and all(c.split()[1:3] == [str(S), str(T * f)] for c in hops)
    assert ("fold_weight" in ent) == (mode == 0)


@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("four_d", [False, True], ids=["3d", "4d_f1"])
def test_single_channel_window_major_takes_the_mfma_entries(four_d, train, recorder):
    """f == 1 with as_series=False is the scalar-load form only at the default geometry"""
    rec = recorder({})
    torch.manual_seed(0)
    x, W = torch.randn(2, N_V, T_WIN), torch.randn(3, 6, 8)
    if four_d:
        x, W = x.unsqueeze(3), W.unsqueeze(2)
    out, calls = _call(rec, x, W, 0, train, stride=2)
    assert tuple(out.shape) == (2 * 4, N_V, 8)
    ent = _entries(calls)
    assert "cheb_project_windows" not in ent and "cheb_windows_backward" not in ent and "cheb_project_series" not in ent
    assert ent.count("cheb_project_series_conv") == 1 and ent.count("cheb_series_conv_backward") == (1 if train else 0)
    assert "cheb_project_series_conv 2 %d %d 1 6 8 3 1 0 2 0 0" % (N_V, T_WIN) in calls


# positions of the nullable pointers in tgcn_cheb_series_conv_backward_f32(stream, S, n, T, f, H, N, K, stack, g, g_as_series, W, G, dW, ws, ...)
_STACK, _G, _DW = 8, 12, 13


@pytest.mark.parametrize("need_series,need_params", [(True, True), (False, True), (True, False), (False, False)],
                         ids=["both", "first-layer", "frozen", "nothing"])
def test_one_sided_backwards_pass_null_pointers(need_series, need_params, recorder):
    rec = recorder({})
    S, T, H, f, N, K = 2, T_WIN, 5, 4, 8, 3
    torch.manual_seed(0)
    series = torch.randn(S, N_V, T, f, requires_grad=need_series)
    W, bias = torch.randn(K, H, f, N, requires_grad=need_params), torch.randn(N, requires_grad=need_params)
    out = F.cheb_time_windows(_op("plain"), series, W, bias, F.BIAS_CHANNEL, 0, stride=2, padding=(1, 2))
    if out.requires_grad:
        out.backward(torch.ones_like(out))
    back = [i for i, c in enumerate(rec.calls) if c.startswith("cheb_series_conv_backward ")]
    assert len(back) == (1 if need_series or need_params else 0)
    for i in back:
        nulls = set(rec.nulls[i]) - {0}            # the recorder's stream is null
        assert nulls == ({_G} if not need_series else set()) | ({_STACK, _DW} if not need_params else set()), nulls


BAD = [dict(stride=0), dict(stride=-1), dict(stride=1.5), dict(stride=True), dict(stride="2"), dict(stride=None),
       dict(padding=-1), dict(padding=5), dict(padding=(0, 5)), dict(padding=(5, 0)), dict(padding=(-1, 0)), dict(padding=(0, -1)),
       dict(padding=1.0), dict(padding=(1.0, 0)), dict(padding=(1, 2, 3)), dict(padding=(1,)), dict(padding="same"), dict(padding=None),
       dict(padding=True)]


@pytest.mark.parametrize("geo", BAD, ids=[str(b) for b in BAD])
def test_invalid_geometry_raises_before_anything_is_built_or_launched(geo, recorder, monkeypatch):
    """H = 5: pads above 4, negative pads, steps below 1, non-integers and unknown strings"""
    rec = recorder({})
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda L, device: pytest.fail("operand built")))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: pytest.fail("operand built")))
    ei = torch.tensor([[0, 1], [1, 0]])
    h = tgcn_amd.TGCNCheb_H(torch.eye(8), 4, 3, 3, 5)
    c = tgcn_amd.ChebTimeConv(4, 3, 3, 5)
    series = torch.randn(2, 8, 10, 4)
    for as_series in (False, True):
        with pytest.raises(_lib.TgcnError):
            h.forward_series(series, as_series=as_series, **geo)
        with pytest.raises(_lib.TgcnError):
            c.forward_series(series, ei, as_series=as_series, **geo)
        with pytest.raises(_lib.TgcnError):
            F.cheb_time_windows(_op("plain"), torch.randn(2, N_V, 10, 4), torch.randn(3, 5, 4, 8), None, F.BIAS_NONE, 0, as_series=as_series, **geo)
    assert rec.calls == []


def test_padded_series_shorter_than_a_window_raises(recorder, monkeypatch):
    """Tp = T + left + right < H; a series shorter than H is fine once its padding makes up for it"""
    rec = recorder({})
    h = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 3, 3, 5)
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda L, device: pytest.fail("operand built")))
    for T, padding in ((4, 0), (2, 1), (2, (2, 0)), (1, (1, 2))):
        with pytest.raises(_lib.TgcnError):
            h.forward_series(torch.randn(2, N_V, T, 4), padding=padding)
    assert rec.calls == []
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda L, device: _Op(N_V, 256)))
    assert tuple(h.forward_series(torch.randn(2, N_V, 2, 4), padding=(2, 1)).shape) == (2 * 1, N_V, 3)
    assert tuple(h.forward_series(torch.randn(2, N_V, 1, 4), padding="causal", as_series=True).shape) == (2, N_V, 1, 3)


def test_bf16_and_learnable_edge_weights_still_raise(recorder, monkeypatch):
    rec = recorder({})
    op = _op("plain")
    geo = dict(stride=2, padding="causal")
    with pytest.raises(_lib.TgcnError):
        F.cheb_time_windows(op, torch.randn(2, N_V, T_WIN, 4), torch.randn(3, 6, 4, 8).to(torch.bfloat16), None, F.BIAS_NONE, 0, **geo)
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda L, device: pytest.fail("operand built")))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: pytest.fail("operand built")))
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(_lib.TgcnError):
        tgcn_amd.TGCNCheb_H(torch.eye(8), 4, 3, 3, 4).to(torch.bfloat16).forward_series(torch.randn(2, 8, 10, 4), as_series=True, **geo)
    with pytest.raises(_lib.TgcnError):
        tgcn_amd.ChebTimeConv(4, 3, 3, 4).to(torch.bfloat16).forward_series(torch.randn(2, 8, 10, 4), ei, **geo)
    with pytest.raises(_lib.TgcnError):
        tgcn_amd.ChebTimeConv(4, 3, 3, 5).forward_series(torch.randn(2, 8, 10, 4), ei, torch.ones(2, requires_grad=True), **geo)
    assert rec.calls == []


# (padding spelling, stride) -> nwin for T = 12, H = 6
SPELLINGS = [(0, 1, 7), (0, 5, 2), (2, 1, 11), (2, 3, 4), ((0, 3), 2, 5), ((5, 0), 1, 12), ("causal", 1, 12), ("causal", 4, 3), ((5, 5), 1, 17),
             ([1, 0], 7, 2)]


@pytest.mark.parametrize("cls", ["TGCNCheb_H", "ChebTimeConv"])
@pytest.mark.parametrize("padding,stride,nwin", SPELLINGS, ids=["%s-s%d" % (s[0], s[1]) for s in SPELLINGS])
def test_output_shapes_of_every_padding_spelling(padding, stride, nwin, cls, recorder, monkeypatch):
    recorder({})
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda *a, **k: _Op(N_V, 256)))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: _Op(N_V, 256)))
    assert F.series_geometry(T_WIN, 6, stride, padding)[3] == nwin
    if cls == "TGCNCheb_H":
        layer, extra = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 6), ()
    else:
        layer, extra = tgcn_amd.ChebTimeConv(4, 8, 3, 6), (torch.tensor([[0, 1], [1, 0]]),)
    series = torch.randn(3, N_V, T_WIN, 4)
    assert tuple(layer.forward_series(series, *extra, stride=stride, padding=padding).shape) == (3 * nwin, N_V, 8)
    assert tuple(layer.forward_series(series, *extra, as_series=True, stride=stride, padding=padding).shape) == (3, N_V, nwin, 8)
