"""CPU test of the launches of the streaming time-window entries with bfloat16 parameters (the recorder technique of
tests/test_layer_dispatch.py): a bf16 TGCNCheb_H / ChebTimeConv streams through the bf16 hops and the `_bf16` series entries only, the
adjoint hops and the weight fold run in fp32, no fp32 series entry is launched; the one call left out (single channel, window-major,
default geometry: the scalar-load form) and a series that is not bfloat16 itself raise with nothing launched; a shape the plan refuses raises before any hop.  The plan query
itself (host only, real library): bf16 spans hold the horizon in fewer bytes than the fp32 ones."""
import ctypes as C

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F
from tgcn_amd.graph import GraphOperand

from test_layer_dispatch import N_V, T_WIN, _Op, _op, recorder  # noqa: F401  (the recorder fixture)

BF = torch.bfloat16
KB64 = 64 * 1024
# fp32 entries the bf16 path launches on fp32 buffers: the adjoint hops on the fp32 G, the fold of the weight and of its gradient
F32_ON_FP32 = {"csr_hop2", "fold_weight"}


def _entries(calls):
    return [c.split()[0] for c in calls]


def _layer(cls, f, N, K, H, monkeypatch):
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda *a, **k: _Op(N_V, 256)))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: _Op(N_V, 256)))
    if cls == "TGCNCheb_H":
        return tgcn_amd.TGCNCheb_H(torch.eye(N_V), f, N, K, H).to(BF), ()
    return tgcn_amd.ChebTimeConv(f, N, K, H).to(BF), (torch.tensor([[0, 1], [1, 0]]),)


GEOMETRIES = [(dict(), (1, 0, 0)), (dict(stride=2, padding="causal"), (2, 5, 0))]


@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
@pytest.mark.parametrize("geo,geom", GEOMETRIES, ids=["default", "stride2-causal"])
@pytest.mark.parametrize("cls", ["TGCNCheb_H", "ChebTimeConv"])
def test_bf16_series_launches_the_bf16_entries(cls, geo, geom, as_series, recorder, monkeypatch):
    rec = recorder({})
    S, T, H, f, N, K = 2, T_WIN, 6, 4, 8, 3
    stride, left, right = geom
    nwin = (T + left + right - H) // stride + 1
    layer, extra = _layer(cls, f, N, K, H, monkeypatch)
    torch.manual_seed(0)
    series = torch.randn(S, N_V, T, f).to(BF).requires_grad_(True)
    out = layer.forward_series(series, *extra, as_series=as_series, **geo)
    assert out.dtype == BF and tuple(out.shape) == ((S, N_V, nwin, N) if as_series else (S * nwin, N_V, N))
    fwd = list(rec.calls)
    ent = _entries(fwd)
    # the regime query comes first (host only, before the hops): H f N vec stride -- f = 4 is the narrow-read form
    # then the input gradient's (the series needs one): ceil(H / stride) weight time rows of N channels, K*f columns, step 1
    assert fwd[0] == "series_conv_plan_bf16 %d %d %d 0 %d" % (H, f, N, stride)
    assert fwd[1] == "series_conv_plan_bf16 %d %d %d 1 1" % (-(-H // stride), N, K * f) and ent.count("series_conv_plan_bf16") == 2
    assert set(ent) <= {"series_conv_plan_bf16", "csr_hop2_bf16", "cheb_project_series_conv_bf16", "fold_weight"}, ent
    assert ent.count("csr_hop2_bf16") >= K - 1
    # scalars of the entry: S n T f H N K stack_ld bias_dtype bias_kind (per vertex and channel in TGCNCheb_H) as_series stride pad_left pad_right
    assert [c for c in fwd if c.startswith("cheb_project_series_conv_bf16 ")] == [
        "cheb_project_series_conv_bf16 %d %d %d %d %d %d %d %d 1 %d %d %d %d %d" % (S, N_V, T, f, H, N, K, T * f, 2 if cls == "TGCNCheb_H" else 1, int(as_series),
                                                                                  stride, left, right)]
    del rec.calls[:]
    out.backward(torch.ones_like(out))
    back = list(rec.calls)
    bent = _entries(back)
    assert [c for c in back if c.startswith("cheb_series_conv_backward_bf16 ")] == [
        "cheb_series_conv_backward_bf16 %d %d %d %d %d %d %d %d %d 1024 %d %d %d" % (S, N_V, T, f, H, N, K, T * f, int(as_series), stride, left, right)]
    assert set(bent) <= {"cheb_series_conv_backward_bf16"} | F32_ON_FP32, bent
    assert bent.count("csr_hop2") == K - 1                      # the fp32 adjoint hops on rows of T*f floats
    assert all(c.split()[1:3] == [str(S), str(T * f)] for c in back if c.startswith("csr_hop2 "))
    assert not any("_series" in e and not e.endswith("_bf16") for e in ent + bent)
    assert series.grad.dtype == BF and layer.weight.grad.dtype == BF and layer.bias.grad.dtype == BF
    assert series.grad.shape == series.shape and layer.weight.grad.shape == layer.weight.shape


def test_rows_are_padded_by_trailing_elements_only(recorder):
    """T*f = 36: the hop rows and stack_ld are 40 elements, the channel count of the projection stays 3"""
    rec = recorder({})
    S, T, H, f, N, K = 2, 12, 5, 3, 8, 3
    out = F.cheb_time_windows(_op("plain"), torch.randn(S, N_V, T, f).to(BF), torch.randn(K, H, f, N).to(BF), None, F.BIAS_NONE, 1)
    assert out.dtype == BF
    hops = [c for c in rec.calls if c.startswith("csr_hop2_bf16 ")]
    assert len(hops) == K - 1 and all(c.split()[1:3] == [str(S), "40"] for c in hops)
    assert "cheb_project_series_conv_bf16 %d %d %d %d %d %d %d 40 1 0 0 1 0 0" % (S, N_V, T, f, H, N, K) in rec.calls


@pytest.mark.parametrize("four_d", [False, True], ids=["3d", "4d_f1"])
def test_single_channel_runs_as_a_series_or_with_a_geometry(four_d, recorder):
    rec = recorder({})
    x, W = torch.randn(2, N_V, T_WIN).to(BF), torch.randn(3, 6, 8).to(BF)
    if four_d:
        x, W = x.unsqueeze(3), W.unsqueeze(2)
    bias = torch.randn(8).to(BF)
    out = F.cheb_time_windows(_op("plain"), x, W, bias, F.BIAS_CHANNEL, 0, as_series=True)
    assert out.dtype == BF and tuple(out.shape) == (2, N_V, T_WIN - 5, 8)
    out = F.cheb_time_windows(_op("plain"), x, W, bias, F.BIAS_CHANNEL, 0, stride=2)
    assert out.dtype == BF and tuple(out.shape) == (2 * 4, N_V, 8)
    ent = _entries(rec.calls)
    assert ent.count("cheb_project_series_conv_bf16") == 2 and "cheb_project_windows" not in ent and "cheb_project_series_conv" not in ent


def test_single_channel_window_major_default_geometry_raises_with_nothing_launched(recorder, monkeypatch):
    rec = recorder({})
    x, W = torch.randn(2, N_V, T_WIN).to(BF), torch.randn(3, 6, 8).to(BF)
    for xx, ww in ((x, W), (x.unsqueeze(3), W.unsqueeze(2))):
        for geo in (dict(), dict(stride=1, padding=0), dict(padding=(0, 0))):
            with pytest.raises(_lib.TgcnError, match="as_series=True or any stride / padding"):
                F.cheb_time_windows(_op("plain"), xx, ww, None, F.BIAS_NONE, 0, **geo)
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda L, device: pytest.fail("operand built")))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: pytest.fail("operand built")))
    with pytest.raises(_lib.TgcnError, match="as_series=True"):
        tgcn_amd.TGCNCheb_H(torch.eye(8), 1, 3, 3, 4).to(BF).forward_series(torch.randn(2, 8, 10).to(BF))
    with pytest.raises(_lib.TgcnError, match="as_series=True"):
        tgcn_amd.ChebTimeConv(1, 3, 3, 4).to(BF).forward_series(torch.randn(2, 8, 10).to(BF), torch.tensor([[0, 1], [1, 0]]))
    assert rec.calls == []


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.float64])
def test_a_series_of_another_dtype_raises_with_nothing_launched(dt, recorder, monkeypatch):
    """bf16 parameters take a bf16 series: the recording is cast once by its owner (series.to(torch.bfloat16)), any other dtype is refused
    before an operand is built -- in both layouts and with a geometry"""
    rec = recorder({})
    for geo in (dict(), dict(as_series=True), dict(stride=2, padding="causal")):
        with pytest.raises(_lib.TgcnError, match="cast it once"):
            F.cheb_time_windows(_op("plain"), torch.randn(2, N_V, T_WIN, 4).to(dt), torch.randn(3, 6, 4, 8).to(BF), None, F.BIAS_NONE, 0, **geo)
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda L, device: pytest.fail("operand built")))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: pytest.fail("operand built")))
    with pytest.raises(_lib.TgcnError, match="cast it once"):
        tgcn_amd.TGCNCheb_H(torch.eye(8), 4, 3, 3, 4).to(BF).forward_series(torch.randn(2, 8, 10, 4).to(dt), as_series=True)
    with pytest.raises(_lib.TgcnError, match="cast it once"):
        tgcn_amd.ChebTimeConv(4, 3, 3, 4).to(BF).forward_series(torch.randn(2, 8, 10, 4).to(dt), torch.tensor([[0, 1], [1, 0]]))
    assert rec.calls == []


def test_learnable_edge_weights_stay_refused_with_bf16(recorder, monkeypatch):
    rec = recorder({})
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: pytest.fail("operand built")))
    with pytest.raises(_lib.TgcnError):
        tgcn_amd.ChebTimeConv(4, 3, 3, 4).to(BF).forward_series(torch.randn(2, 8, 10, 4), torch.tensor([[0, 1], [1, 0]]),
                                                                torch.ones(2, requires_grad=True), as_series=True)
    assert rec.calls == []


def test_a_shape_the_plan_refuses_raises_before_any_hop(recorder, monkeypatch):
    rec = recorder({})
    real = rec.__getattr__

    def refuse(*a):
        rec.calls.append("series_conv_plan_bf16")
        return -4                                   # TGCN_ERR_UNSUPPORTED
    monkeypatch.setattr(type(rec), "__getattr__", lambda self, name: refuse if name == "tgcn_series_conv_plan_bf16" else
                        ((lambda: b"refused") if name == "tgcn_last_error" else real(name)))
    with pytest.raises(_lib.TgcnError):
        F.cheb_time_windows(_op("plain"), torch.randn(2, N_V, T_WIN, 8).to(BF), torch.randn(3, 6, 8, 8).to(BF), None, F.BIAS_NONE, 0, stride=2)
    assert rec.calls == ["series_conv_plan_bf16"]
    # the input gradient's span refused (the second query): also before any hop
    del rec.calls[:]
    answers = iter([0, -4])

    def refuse_second(*a):
        rec.calls.append("series_conv_plan_bf16")
        return next(answers)
    monkeypatch.setattr(type(rec), "__getattr__", lambda self, name: refuse_second if name == "tgcn_series_conv_plan_bf16" else
                        ((lambda: b"refused") if name == "tgcn_last_error" else real(name)))
    with pytest.raises(_lib.TgcnError):
        F.cheb_time_windows(_op("plain"), torch.randn(2, N_V, T_WIN, 8).to(BF).requires_grad_(True), torch.randn(3, 6, 8, 8).to(BF), None,
                            F.BIAS_NONE, 0, stride=2)
    assert rec.calls == ["series_conv_plan_bf16"] * 2


def test_fp32_calls_are_unchanged(recorder):
    """fp32 parameters through the new routing: the entries tests/test_series_conv_dispatch.py pins, no bf16 entry"""
    rec = recorder({})
    out = F.cheb_time_windows(_op("plain"), torch.randn(2, N_V, T_WIN, 4), torch.randn(3, 6, 4, 8), None, F.BIAS_NONE, 0, stride=2)
    out2 = F.cheb_time_windows(_op("plain"), torch.randn(2, N_V, T_WIN, 4), torch.randn(3, 6, 4, 8), None, F.BIAS_NONE, 0)
    assert out.dtype == out2.dtype == torch.float32
    assert sorted(set(_entries(rec.calls))) == ["cheb_project_series", "cheb_project_series_conv", "csr_hop2", "fold_weight", "series_conv_plan"]
    assert not any(e.endswith("_bf16") for e in _entries(rec.calls))


# ---------------------------------------------------------------------------------------------------------------- the plan query (host only)
def _plan(name, H, f, N, vec, stride):
    hc, lds = C.c_int32(-1), C.c_int32(-1)
    rc = getattr(_lib.lib(), name)(H, f, N, vec, stride, C.byref(hc), C.byref(lds))
    return rc, hc.value, lds.value


def _regime(rc, hc, lds, H):
    if rc != 0:
        assert rc == -4, rc
        return "unsupported"
    assert 1 <= hc <= H and lds > 0
    return ("large" if lds > KB64 else "lds64") + ("-whole" if hc == H else "-chunked")


def test_bf16_plan_holds_more_of_the_horizon_than_the_fp32_plan():
    """the chunked shapes of tests/test_series_conv.py's REGIMES: on bf16 span bytes the same (H, f) answers a larger HC or leaves the
    chunked regime.  The 64 KB limit is tried first, so these answers hold with and without a device."""
    from test_series_conv import REGIMES
    seen = 0
    for name, (shape, direction, want) in REGIMES.items():
        if want != "lds64-chunked":
            continue
        n, S, T, H, f, g, K, stride, left, right = shape
        q = (H, f, g, stride) if direction == 0 else (-(-H // stride), g, K * f, 1)
        rc32, hc32, lds32 = _plan("tgcn_series_conv_plan", q[0], q[1], q[2], int(q[1] % 4 == 0), q[3])
        rcb, hcb, ldsb = _plan("tgcn_series_conv_plan_bf16", q[0], q[1], q[2], int(q[1] % 8 == 0), q[3])
        assert _regime(rc32, hc32, lds32, q[0]) == "lds64-chunked", name
        assert rcb == 0 and ldsb <= KB64 and hcb > hc32, (name, hcb, hc32)
        print(name, "fp32 HC", hc32, "bf16 HC", hcb, _regime(rcb, hcb, ldsb, q[0]))
        seen += 1
    assert seen == 4


def test_bf16_plan_arguments_and_span_bytes():
    L = _lib.lib()
    hc, lds = C.c_int32(0), C.c_int32(0)
    assert L.tgcn_series_conv_plan_bf16(0, 8, 8, 1, 1, C.byref(hc), C.byref(lds)) == -1        # TGCN_ERR_INVALID
    assert L.tgcn_series_conv_plan_bf16(4, 8, 8, 1, 0, C.byref(hc), C.byref(lds)) == -1
    assert L.tgcn_series_conv_plan_bf16(4, 8, 8, 1, 1, None, C.byref(lds)) == -1
    # weight tile: NT*16 columns of 72 bf16; four spans of (31 * lst + hc) rows.  f = 8: unpadded rows of 8 elements
    assert _plan("tgcn_series_conv_plan_bf16", 15, 8, 16, 1, 1) == (0, 15, (16 * 72 + 4 * 46 * 8) * 2)
    # f = 32, odd lst: rows of 6 slots (48 elements); lst = 2: 5 slots (40 elements)
    assert _plan("tgcn_series_conv_plan_bf16", 5, 32, 64, 1, 1) == (0, 5, (64 * 72 + 4 * 36 * 48) * 2)
    assert _plan("tgcn_series_conv_plan_bf16", 5, 32, 64, 1, 2) == (0, 5, (64 * 72 + 4 * 67 * 40) * 2)
    # f = 16, odd lst: no padding.  The narrow-read form (vec = 0, or f % 8 != 0): the plain element sequence, rounded up to 8 elements
    assert _plan("tgcn_series_conv_plan_bf16", 5, 16, 32, 1, 3) == (0, 5, (32 * 72 + 4 * 98 * 16) * 2)
    assert _plan("tgcn_series_conv_plan_bf16", 5, 3, 8, 0, 1) == (0, 5, (16 * 72 + 4 * 112) * 2)
    assert _plan("tgcn_series_conv_plan_bf16", 5, 3, 8, 1, 1) == _plan("tgcn_series_conv_plan_bf16", 5, 3, 8, 0, 1)
