"""CPU test of the launches of the streaming time-window entries on multi-channel series (the recorder technique of
tests/test_layer_dispatch.py): a (S, n, T, f) series with f > 1, or any series with as_series=True, launches the series entries -- ONE
projection for all recordings, one backward call in training; a single-channel series with as_series=False keeps the launches that
test_layer_dispatch.EXPECTED pins; what the entries refuse raises TgcnError with nothing launched."""
import contextlib

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F
from tgcn_amd.graph import GraphOperand

from test_layer_dispatch import EXPECTED, N_V, T_WIN, _Op, _op, recorder  # noqa: F401  (the recorder fixture)


def _entries(calls):
    return [c.split()[0] for c in calls]


def _windows_call(series, W, mode, train, op_kind="plain", as_series=False, bias_kind=F.BIAS_CHANNEL):
    op = _op(op_kind)
    bias = torch.randn(W.shape[-1])
    leaves = [series, W, bias]
    for t in leaves:
        t.requires_grad_(train)
    with (contextlib.nullcontext() if train else torch.no_grad()):
        out = F.cheb_time_windows(op, series, W, bias, bias_kind, mode, as_series=as_series)
    if train:
        out.backward(torch.ones_like(out))
        assert all(t.grad is not None and t.grad.shape == t.shape for t in leaves)
    return out


@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
@pytest.mark.parametrize("mode", [0, 1], ids=["power", "chebyshev"])
def test_multi_channel_series_launches_the_series_entries_once(mode, as_series, train, recorder):
    rec = recorder({})
    S, T, H, f, N, K = 3, T_WIN, 6, 4, 8, 3
    torch.manual_seed(0)
    out = _windows_call(torch.randn(S, N_V, T, f), torch.randn(K, H, f, N), mode, train, as_series=as_series)
    nwin = T - H + 1
    assert tuple(out.shape) == ((S, N_V, nwin, N) if as_series else (S * nwin, N_V, N))
    ent = _entries(rec.calls)
    # scalars of the entry: S n T f H N K bias_kind as_series
    assert [c for c in rec.calls if c.startswith("cheb_project_series ")] == ["cheb_project_series %d %d %d %d %d %d %d 1 %d"
                                                                             % (S, N_V, T, f, H, N, K, int(as_series))]
    assert "cheb_project_windows" not in ent and "cheb_windows_backward" not in ent and "cheb_project" not in ent
    # the hops run once per call in each direction, on rows of T*f floats for all S recordings
    hops = [c for c in rec.calls if c.startswith("csr_hop2 ")]
    assert len(hops) == (K - 1) * (2 if train else 1) and all(c.split()[1:3] == [str(S), str(T * f)] for c in hops)
    back = [c for c in rec.calls if c.startswith("cheb_series_backward ")]
    assert back == (["cheb_series_backward %d %d %d %d %d %d %d %d 1024" % (S, N_V, T, f, H, N, K, int(as_series))] if train else [])


# positions of the nullable pointers in tgcn_cheb_series_backward_f32(stream, S, n, T, f, H, N, K, stack, g, g_as_series, W, G, dW, ws, bytes)
_STACK, _G, _DW = 8, 12, 13


@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
@pytest.mark.parametrize("need_series,need_params", [(True, True), (False, True), (True, False), (False, False)],
                         ids=["both", "first-layer", "frozen", "nothing"])
def test_one_sided_backwards_pass_null_pointers(need_series, need_params, as_series, recorder):
    """G is null when the series needs no gradient, dW (and the hop stack it contracts) when the parameters are frozen; when nothing needs
    a gradient there is no backward call at all"""
    rec = recorder({})
    S, T, H, f, N, K = 2, T_WIN, 5, 4, 8, 3
    torch.manual_seed(0)
    series = torch.randn(S, N_V, T, f, requires_grad=need_series)
    W, bias = torch.randn(K, H, f, N, requires_grad=need_params), torch.randn(N, requires_grad=need_params)
    out = F.cheb_time_windows(_op("plain"), series, W, bias, F.BIAS_CHANNEL, 0, as_series=as_series)
    assert out.requires_grad == (need_series or need_params)
    if out.requires_grad:
        out.backward(torch.ones_like(out))
    assert (series.grad is not None) == need_series and (W.grad is not None) == need_params and (bias.grad is not None) == need_params
    back = [i for i, c in enumerate(rec.calls) if c.startswith("cheb_series_backward ")]
    assert len(back) == (1 if need_series or need_params else 0)
    for i in back:
        assert rec.calls[i] == "cheb_series_backward %d %d %d %d %d %d %d %d 1024" % (S, N_V, T, f, H, N, K, int(as_series))
        nulls = set(rec.nulls[i]) - {0}            # the recorder's stream is null
        assert nulls == ({_G} if not need_series else set()) | ({_STACK, _DW} if not need_params else set()), nulls
    # the adjoint hops run only for a series that needs its gradient
    assert len([c for c in rec.calls if c.startswith("csr_hop2 ")]) == (K - 1) * (2 if need_series else 1)


@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
def test_single_channel_in_the_series_layout_launches_the_series_entries(train, recorder):
    rec = recorder({})
    torch.manual_seed(0)
    out = _windows_call(torch.randn(2, N_V, T_WIN), torch.randn(3, 6, 8), 0, train, as_series=True)
    assert tuple(out.shape) == (2, N_V, T_WIN - 6 + 1, 8)
    ent = _entries(rec.calls)
    assert ent.count("cheb_project_series") == 1 and ent.count("cheb_series_backward") == (1 if train else 0)
    assert "cheb_project_windows" not in ent


@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("four_d", [False, True], ids=["3d", "4d_f1"])
@pytest.mark.parametrize("name", ["windows-power-K3", "windows-cheb-K4-reordered-relabel-once", "windows-K1"])
def test_single_channel_series_keeps_its_launches(name, four_d, train, recorder):
    """(S, n, T) and (S, n, T, 1) with as_series=False: exactly the sequence test_layer_dispatch pins for the windows entry"""
    from test_layer_dispatch import CASES
    _, kind, q, H, N, K, mode, _, _ = CASES[name]
    rec = recorder({})
    torch.manual_seed(0)
    x, W = torch.randn(q, N_V, T_WIN), torch.randn(K, H, N)
    if four_d:
        x, W = x.unsqueeze(3), W.unsqueeze(2)
    out = _windows_call(x, W, mode, train, op_kind=kind)
    assert tuple(out.shape) == (q * (T_WIN - H + 1), N_V, N)
    assert rec.calls == EXPECTED["%s/%s" % (name, "training" if train else "inference")]


def test_bf16_weights_raise_with_nothing_launched(recorder, monkeypatch):
    rec = recorder({})
    op = _op("plain")
    with pytest.raises(_lib.TgcnError):
        F.cheb_time_windows(op, torch.randn(2, N_V, T_WIN, 4), torch.randn(3, 6, 4, 8).to(torch.bfloat16), None, F.BIAS_NONE, 0)
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda L, device: pytest.fail("operand built")))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: pytest.fail("operand built")))
    h = tgcn_amd.TGCNCheb_H(torch.eye(8), 4, 3, 3, 4).to(torch.bfloat16)
    with pytest.raises(_lib.TgcnError):
        h.forward_series(torch.randn(2, 8, 10, 4), as_series=True)
    c = tgcn_amd.ChebTimeConv(4, 3, 3, 4).to(torch.bfloat16)
    with pytest.raises(_lib.TgcnError):
        c.forward_series(torch.randn(2, 8, 10, 4), torch.tensor([[0, 1], [1, 0]]))
    assert rec.calls == []


def test_bad_shapes_and_learnable_edge_weights_raise_before_any_launch(recorder, monkeypatch):
    rec = recorder({})
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda L, device: pytest.fail("operand built")))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: pytest.fail("operand built")))
    ei = torch.tensor([[0, 1], [1, 0]])
    h = tgcn_amd.TGCNCheb_H(torch.eye(8), 4, 3, 3, 5)
    c = tgcn_amd.ChebTimeConv(4, 3, 3, 5)
    for series in (torch.randn(2, 8, 10, 3),       # f != in_channels
                   torch.randn(2, 8, 10),          # a single-channel series for a 4-channel layer
                   torch.randn(2, 8, 4, 4),        # T < H
                   torch.randn(2, 8)):
        with pytest.raises(_lib.TgcnError):
            h.forward_series(series)
        with pytest.raises(_lib.TgcnError):
            c.forward_series(series, ei)
    with pytest.raises(_lib.TgcnError):
        c.forward_series(torch.randn(2, 8, 10, 4), ei, torch.ones(2, requires_grad=True))
    op = _op("plain")
    with pytest.raises(_lib.TgcnError):             # functional entry: the weight's channels against the series'
        F.cheb_time_windows(op, torch.randn(2, N_V, T_WIN, 4), torch.randn(3, 6, 2, 8), None, F.BIAS_NONE, 0)
    with pytest.raises(_lib.TgcnError):
        F.cheb_time_windows(op, torch.randn(2, N_V, 5, 4), torch.randn(3, 6, 4, 8), None, F.BIAS_NONE, 0)
    assert rec.calls == []


@pytest.mark.parametrize("cls", ["TGCNCheb_H", "ChebTimeConv"])
def test_modules_build_their_operand_once_and_launch_the_series_entries(cls, recorder, monkeypatch):
    rec = recorder({})
    built = []

    def build(*a, **k):
        built.append(1)
        return _Op(N_V, 256)
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(build))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(build))
    ei = torch.tensor([[0, 1], [1, 0]])
    ew = torch.ones(2)
    if cls == "TGCNCheb_H":
        layer, extra = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 6), ()
    else:
        layer, extra = tgcn_amd.ChebTimeConv(4, 8, 3, 6), (ei, ew)
    series = torch.randn(3, N_V, T_WIN, 4, requires_grad=True)
    out = layer.forward_series(series, *extra)
    assert tuple(out.shape) == (3 * (T_WIN - 6 + 1), N_V, 8)
    out.backward(torch.ones_like(out))
    out2 = layer.forward_series(series, *extra, as_series=True)
    assert tuple(out2.shape) == (3, N_V, T_WIN - 6 + 1, 8)
    assert built == [1]
    ent = _entries(rec.calls)
    assert ent.count("cheb_project_series") == 2 and ent.count("cheb_series_backward") == 1
    assert layer.weight.grad.shape == layer.weight.shape and layer.bias.grad.shape == layer.bias.shape and series.grad.shape == series.shape
    mode, bias_kind = (0, F.BIAS_VERTEX_CHANNEL) if cls == "TGCNCheb_H" else (1, F.BIAS_CHANNEL)
    assert "cheb_project_series 3 %d %d 4 6 8 3 %d 0" % (N_V, T_WIN, bias_kind) in rec.calls
    assert ("fold_weight" in ent) == (mode == 0)
