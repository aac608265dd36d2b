"""CPU test of the launches of the streaming time-window layers with the relu + pool epilogue (cheb_series_relu_pool /
cheb_stream_relu_pool, F.cheb_time_windows_relu_pool / F.cheb_time_stream_relu_pool), by the recorder technique of
tests/test_layer_dispatch.py: a fused call asks the pool plan first, runs K - 1 hops and launches exactly one pooled entry, with a null idx
under no_grad; its backward launches relu_pool_bwd and then what ChebSeriesFn's backward launches; a reordered operand launches the unpooled
entry and relu_pool; the stream call launches the _stream_pool entry with the host's head or a non-null pos; every refusal raises TgcnError
with nothing logged and no operand built; forward_series / forward_stream log what they logged before; the three entries are declared in the
header, the ctypes table and the library, and their scalar rules answer TGCN_ERR_INVALID before a pointer is read."""
import contextlib
import ctypes
import os

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F

from test_layer_dispatch import N_V, T_WIN, _op, recorder  # noqa: F401  (the recorder fixture)
from test_series_stream_dispatch import BF, _entries, _no_operands, _stream, _stub_operands

POOL_ENTRY, STREAM_ENTRY = "cheb_project_series_pool", "cheb_project_series_stream_pool"
IDX_ARG = _lib.SIGNATURES["tgcn_cheb_project_series_pool_f32"][1].index(ctypes.c_void_p, 13) + 1          # z at 13, idx behind it
POS_ARG = 17                                                                                             # of the _stream_pool entry


def test_argument_positions():
    sig = _lib.SIGNATURES["tgcn_cheb_project_series_pool_f32"][1]
    assert IDX_ARG == 14 and sig[13] is ctypes.c_void_p and sig[14] is ctypes.c_void_p and sig[15] is ctypes.c_int32
    sig = _lib.SIGNATURES["tgcn_cheb_project_series_stream_pool_f32"][1]
    assert sig[POS_ARG] is ctypes.c_void_p and sig[POS_ARG - 1] is ctypes.c_int32 and sig[POS_ARG + 1] is ctypes.c_int32 and len(sig) == 19


def _call(rec, op, series, W, mode, train, pool, bias_kind=F.BIAS_CHANNEL, **kw):
    """the calls one F.cheb_time_windows_relu_pool (and its backward when train) logs"""
    del rec.calls[:], rec.nulls[:]
    torch.manual_seed(1)
    series, W = series.clone(), W.clone()
    bias = torch.randn(W.shape[-1]) if bias_kind == F.BIAS_CHANNEL else torch.randn(N_V * W.shape[-1])
    for t in (series, W, bias):
        t.requires_grad_(train)
    with (contextlib.nullcontext() if train else torch.no_grad()):
        z = F.cheb_time_windows_relu_pool(op, series, W, bias, bias_kind, mode, pool, **kw)
    n_fwd = len(rec.calls)
    if train:
        z.backward(torch.ones_like(z))
        assert all(t.grad is not None and t.grad.shape == t.shape for t in (series, W, bias))
    return z, list(rec.calls), list(rec.nulls), n_fwd


# (kwargs, (stride, left, right, dilation), backward entry and its geometry scalars) at H = 3
GEOS = [(dict(), (1, 0, 0, 1), "cheb_series_backward", ""),
        (dict(stride=2, padding=1), (2, 1, 1, 1), "cheb_series_conv_backward", " 2 1 1"),
        (dict(padding="causal", dilation=2), (1, 4, 0, 2), "cheb_series_dilated_backward", " 1 4 0 2")]


@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
@pytest.mark.parametrize("mode", [0, 1], ids=["power", "chebyshev"])
@pytest.mark.parametrize("f", [1, 4])
@pytest.mark.parametrize("pool", [2, 4])
@pytest.mark.parametrize("geo", GEOS, ids=["default", "stride2-pad1", "causal-dil2"])
def test_a_fused_call_logs_plan_hops_and_one_pooled_entry(geo, pool, f, mode, as_series, train, recorder):
    rec = recorder({})
    kw, (stride, left, right, dil), bwd_entry, bwd_geo = geo
    S, T, H, N, K = 2, T_WIN, 3, 8, 3
    nwin = (T + left + right - (H - 1) * dil - 1) // stride + 1
    torch.manual_seed(0)
    series, W = (torch.randn(S, N_V, T), torch.randn(K, H, N)) if f == 1 else (torch.randn(S, N_V, T, f), torch.randn(K, H, f, N))
    z, calls, nulls, n_fwd = _call(rec, _op("plain"), series, W, mode, train, pool, as_series=as_series, **kw)
    assert tuple(z.shape) == ((S, N_V // pool, nwin, N) if as_series else (S * nwin, N_V // pool, N)) and z.is_contiguous()
    ent = _entries(calls)
    # the plan first and once, with the step and the pool: H f N vec stride pool
    assert calls[0] == "series_pool_plan %d %d %d %d %d %d" % (H, f, N, int(f % 4 == 0), stride, pool) and ent.count("series_pool_plan") == 1
    assert "series_conv_plan" not in ent
    # K - 1 hops on rows of T*f floats, then exactly one pooled entry: S n T f H N K bias_kind as_series pool stride left right dilation
    i_fwd = ent.index(POOL_ENTRY)
    assert ent.count(POOL_ENTRY) == 1 and i_fwd == n_fwd - 1
    hops = [c for c in calls[:i_fwd] if c.startswith("csr_hop2 ")]
    assert len(hops) == K - 1 and all(c.split()[1:3] == [str(S), str(T * f)] for c in hops)
    assert calls[i_fwd] == "%s %d %d %d %d %d %d %d 1 %d %d %d %d %d %d" % (POOL_ENTRY, S, N_V, T, f, H, N, K, int(as_series), pool, stride, left, right,
                                                                          dil)
    assert set(ent[:n_fwd]) <= {"series_pool_plan", "csr_hop2", "fold_weight", POOL_ENTRY}, ent
    # no unpooled projection, no scalar-load form, no separate pool pass
    assert not {"cheb_project_series", "cheb_project_series_conv", "cheb_project_series_dilated", "cheb_project_windows", "relu_pool"} & set(ent)
    # idx: null under no_grad, stored when something trains
    assert (IDX_ARG in nulls[i_fwd]) == (not train)
    back = calls[n_fwd:]
    if not train:
        assert back == []
        return
    # the backward: relu_pool_bwd on the forward's layout, then ChebSeriesFn's backward entry with its geometry, then the adjoint hops
    q, fN = (S, nwin * N) if as_series else (S * nwin, N)
    assert back[0] == "relu_pool_bwd %d %d %d %d" % (q, N_V, fN, pool)
    assert back[1] == "%s %d %d %d %d %d %d %d %d 1024%s" % (bwd_entry, S, N_V, T, f, H, N, K, int(as_series), bwd_geo)
    assert _entries(back).count("csr_hop2") == K - 1 and _entries(back).count("relu_pool_bwd") == 1
    assert set(_entries(back)) <= {"relu_pool_bwd", bwd_entry, "csr_hop2", "fold_weight"}, back


@pytest.mark.parametrize("geo", GEOS, ids=["default", "stride2-pad1", "causal-dil2"])
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
def test_the_backward_after_the_pool_gradient_is_the_unpooled_backward(geo, as_series, recorder):
    """behind relu_pool_bwd the fused backward logs, call for call, what the backward of F.cheb_time_windows logs"""
    rec = recorder({})
    kw = geo[0]
    torch.manual_seed(0)
    series, W = torch.randn(2, N_V, T_WIN, 4), torch.randn(3, 3, 4, 8)
    _, calls, _, n_fwd = _call(rec, _op("plain"), series, W, 0, True, 4, as_series=as_series, **kw)
    del rec.calls[:]
    s, w, b = series.clone().requires_grad_(), W.clone().requires_grad_(), torch.randn(8, requires_grad=True)
    out = F.cheb_time_windows(_op("plain"), s, w, b, F.BIAS_CHANNEL, 0, as_series=as_series, **kw)
    n_plain = len(rec.calls)
    out.backward(torch.ones_like(out))
    assert calls[n_fwd + 1:] == rec.calls[n_plain:] and calls[n_fwd].startswith("relu_pool_bwd ")


@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("f", [1, 4])
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
def test_a_reordered_operand_logs_the_unpooled_entry_and_relu_pool(as_series, f, train, recorder):
    rec = recorder({})
    S, T, H, N, K, pool = 2, T_WIN, 3, 8, 3, 4
    nwin = T - H + 1
    torch.manual_seed(0)
    series, W = (torch.randn(S, N_V, T), torch.randn(K, H, N)) if f == 1 else (torch.randn(S, N_V, T, f), torch.randn(K, H, f, N))
    assert not F.series_pool_is_fused(_op("reordered"), pool) and F.series_pool_is_fused(_op("plain"), pool)
    z, calls, _, n_fwd = _call(rec, _op("reordered"), series, W, 1, train, pool, as_series=as_series)
    assert tuple(z.shape) == ((S, N_V // pool, nwin, N) if as_series else (S * nwin, N_V // pool, N))
    ent = _entries(calls)
    assert not any("pool_plan" in e or e in (POOL_ENTRY, STREAM_ENTRY) for e in ent)
    # the MFMA entry also for one channel in the window-major layout, then the pool pass on the layer's layout
    assert ent.count("cheb_project_series") == 1 and "cheb_project_windows" not in ent
    assert "cheb_project_series %d %d %d %d %d %d %d 1 %d" % (S, N_V, T, f, H, N, K, int(as_series)) in calls
    q, fN = (S, nwin * N) if as_series else (S * nwin, N)
    assert [c for c in calls if c.startswith("relu_pool ")] == ["relu_pool %d %d %d %d" % (q, N_V, fN, pool)]
    assert ent.index("cheb_project_series") < ent.index("relu_pool") and ent.index("relu_pool") < n_fwd
    assert [c for c in calls if c.startswith("relu_pool_bwd ")] == (["relu_pool_bwd %d %d %d %d" % (q, N_V, fN, pool)] if train else [])
    if train:
        assert ent.index("relu_pool_bwd") < ent.index("cheb_series_backward")


CHUNKS = [1, 1, 3, 8, 9, 40, 5]


def _stream_pool(rec, op, chunk, W, bias, mode, state, dilation, pool, capturable=False):
    del rec.calls[:], rec.nulls[:]
    with torch.no_grad():
        z, state = F.cheb_time_stream_relu_pool(op, chunk, W, bias, F.BIAS_NONE if bias is None else F.BIAS_CHANNEL, mode, pool, state=state,
                                                dilation=dilation, capturable=capturable)
    return z, state, list(rec.calls), list(rec.nulls)


@pytest.mark.parametrize("mode", [0, 1], ids=["power", "chebyshev"])
@pytest.mark.parametrize("d", [1, 4])
@pytest.mark.parametrize("pool", [2, 4])
def test_a_stream_call_logs_the_stream_pool_entry_and_the_head_follows(pool, d, mode, recorder):
    rec = recorder({})
    S, f, H, N, K = 3, 8, 3, 8, 3
    Cr = (H - 1) * d
    torch.manual_seed(0)
    W, bias, op = torch.randn(K, H, f, N), torch.randn(N), _op("plain")
    host = cap = plain = None
    head = 0
    for Tc in CHUNKS:
        chunk = torch.randn(S, N_V, Tc, f)
        z, host, calls, nulls = _stream_pool(rec, op, chunk, W, bias, mode, host, d, pool)
        assert tuple(z.shape) == (S, N_V // pool, Tc, N) and z.is_contiguous() and z.dtype == torch.float32
        ent = _entries(calls)
        assert calls[0] == "series_pool_plan %d %d %d 1 1 %d" % (H, f, N, pool) and ent.count("series_pool_plan") == 1
        hops = [c for c in calls if c.startswith("csr_hop2 ")]
        assert len(hops) == K - 1 and all(c.split()[1:3] == [str(S), str(Tc * f)] for c in hops)
        assert ent[-1] == STREAM_ENTRY and ent.count(STREAM_ENTRY) == 1 and set(ent) <= {"series_pool_plan", "csr_hop2", "fold_weight", STREAM_ENTRY}
        # scalars: S n Tc f H N K bias_kind pool ring_ld head dilation; the head follows (head + Tc) mod C; pos is null
        assert calls[-1] == "%s %d %d %d %d %d %d %d 1 %d %d %d %d" % (STREAM_ENTRY, S, N_V, Tc, f, H, N, K, pool, Cr * f, head, d)
        assert POS_ARG in nulls[-1]
        head = (head + Tc) % Cr
        assert host.head == head
        # the unpooled call on a twin state: the same calls but the plan and the entry, the same head
        _, plain, plain_calls = _stream(rec, op, chunk, W, bias, mode, plain, d)
        assert calls[1:-1] == plain_calls[1:-1] and plain.head == host.head and plain.seen == host.seen
        # a capturable twin passes a non-null pos and a head of 0
        z2, cap, ccalls, cnulls = _stream_pool(rec, op, chunk, W, bias, mode, cap, d, pool, capturable=(cap is None))
        assert ccalls[:-1] == calls[:-1]
        assert ccalls[-1] == "%s %d %d %d %d %d %d %d 1 %d %d 0 %d" % (STREAM_ENTRY, S, N_V, Tc, f, H, N, K, pool, Cr * f, d)
        assert POS_ARG not in cnulls[-1] and "series_stream_advance" not in _entries(ccalls)
    assert cap.capturable and not host.capturable and host.seen == sum(CHUNKS)
    assert isinstance(host, F.SeriesStreamState) and tuple(host.ring.shape) == (K, S, N_V, Cr * f)


def test_pooled_and_unpooled_steps_alternate_on_one_state(recorder):
    rec = recorder({})
    torch.manual_seed(0)
    W, op = torch.randn(3, 3, 4, 8), _op("plain")
    state, head = None, 0
    for i, Tc in enumerate(CHUNKS):
        chunk = torch.randn(2, N_V, Tc, 4)
        if i % 2:
            _, state, calls = _stream(rec, op, chunk, W, None, 0, state, 2)
            assert calls[-1].split()[0] == "cheb_project_series_stream" and calls[-1].split()[-2] == str(head)
        else:
            _, state, calls, _ = _stream_pool(rec, op, chunk, W, None, 0, state, 2, 4)
            assert calls[-1].split()[0] == STREAM_ENTRY and calls[-1].split()[-2] == str(head)
        head = (head + Tc) % 4
        assert state.head == head


def test_one_tap_stream_launches_the_pooled_entry_on_the_chunk(recorder):
    rec = recorder({})
    W, op = torch.randn(3, 1, 4, 8), _op("plain")
    for capturable in (False, True):
        state = None
        for Tc in (4, 1):
            z, state, calls, nulls = _stream_pool(rec, op, torch.randn(2, N_V, Tc, 4), W, None, 1, state, 7, 2, capturable=capturable)
            ent = _entries(calls)
            assert STREAM_ENTRY not in ent and ent.count(POOL_ENTRY) == 1 and tuple(z.shape) == (2, N_V // 2, Tc, 8)
            i = ent.index(POOL_ENTRY)
            assert calls[i] == "%s 2 %d %d 4 1 8 3 0 1 2 1 0 0 1" % (POOL_ENTRY, N_V, Tc) and IDX_ARG in nulls[i]
            assert ent[i + 1:] == (["series_stream_advance"] if capturable else [])
        assert state.ring is None and state.C == 0


def test_a_reordered_operand_streams_unfused(recorder):
    rec = recorder({})
    z, state, calls, _ = _stream_pool(rec, _op("reordered"), torch.randn(2, N_V, 5, 4), torch.randn(3, 3, 4, 8), None, 1, None, 1, 4)
    ent = _entries(calls)
    assert tuple(z.shape) == (2, N_V // 4, 5, 8) and STREAM_ENTRY not in ent and "series_pool_plan" not in ent
    assert ent.count("cheb_project_series_stream") == 1 and calls[-1] == "relu_pool 2 %d %d 4" % (N_V, 5 * 8)


def test_the_modules_pass_everything_on(recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    assert tgcn_amd.cheb_series_relu_pool is tgcn_amd.nn.cheb_series_relu_pool and tgcn_amd.cheb_stream_relu_pool is tgcn_amd.nn.cheb_stream_relu_pool
    for f in (1, 4):
        for layer, extra, kind in ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), f, 8, 3, 3), (), 2), (tgcn_amd.ChebTimeConv(f, 8, 3, 3), (ei,), 1),
                                   (tgcn_amd.ChebTimeConv(f, 8, 3, 3, bias=False), (ei, torch.ones(2)), 0)):
            series = torch.randn(2, N_V, T_WIN, f)
            if f == 1:
                series = series[..., 0]
            del rec.calls[:]
            with torch.no_grad():
                z = tgcn_amd.cheb_series_relu_pool(layer, series, *extra, as_series=True, padding="causal", dilation=2)      # pool=4 is the default
            assert tuple(z.shape) == (2, N_V // 4, T_WIN, 8)
            assert rec.calls[0] == "series_pool_plan 3 %d 8 %d 1 4" % (f, int(f == 4))
            assert rec.calls[-1] == "%s 2 %d %d %d 3 8 3 %d 1 4 1 4 0 2" % (POOL_ENTRY, N_V, T_WIN, f, kind)
            del rec.calls[:]
            z = tgcn_amd.cheb_series_relu_pool(layer, series, *extra, pool=2, stride=3)
            assert tuple(z.shape) == (2 * 4, N_V // 2, 8) and rec.calls[-1].split()[-5:] == ["2", "3", "0", "0", "1"]
            z.sum().backward()
            assert _entries(rec.calls).count("relu_pool_bwd") == 1 and layer.weight.grad is not None
            state = None
            for Tc, head in ((5, 0), (2, 1), (7, 3)):
                del rec.calls[:]
                with torch.no_grad():
                    z, state = tgcn_amd.cheb_stream_relu_pool(layer, series[:, :, :Tc], *extra, state=state, dilation=2)
                assert tuple(z.shape) == (2, N_V // 4, Tc, 8) and isinstance(state, F.SeriesStreamState)
                assert rec.calls[-1] == "%s 2 %d %d %d 3 8 3 %d 4 %d %d 2" % (STREAM_ENTRY, N_V, Tc, f, kind, 4 * f, head)
            # the same state continues through forward_stream
            del rec.calls[:]
            with torch.no_grad():
                out, state2 = layer.forward_stream(series[:, :, :3], *extra, state=state, dilation=2)
            assert state2 is state and rec.calls[-1].split()[0] == "cheb_project_series_stream" and rec.calls[-1].split()[-2] == "2"


def test_refusals_launch_nothing_and_build_no_operand(recorder, monkeypatch):
    rec = recorder({})
    _no_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    h, c = tgcn_amd.TGCNCheb_H(torch.eye(8), 4, 3, 3, 3), tgcn_amd.ChebTimeConv(4, 3, 3, 3)
    x = torch.randn(2, 8, 10, 4)
    both = ((h, ()), (c, (ei,)))
    sr, st = tgcn_amd.cheb_series_relu_pool, tgcn_amd.cheb_stream_relu_pool
    for layer, extra in both:
        for pool in (0, 1, 3, 8, 2.0, True, None, "4"):
            with pytest.raises(_lib.TgcnError, match="pool is 2 or 4"):
                sr(layer, x, *extra, pool=pool)
            with pytest.raises(_lib.TgcnError, match="pool is 2 or 4"), torch.no_grad():
                st(layer, x, *extra, pool=pool)
        # 10 vertices at pool 4 (and 9 at pool 2)
        for xs, pool in ((torch.randn(2, 10, 10, 4), 4), (torch.randn(2, 9, 10, 4), 2)):
            with pytest.raises(_lib.TgcnError, match="not a multiple of pool"):
                sr(layer, xs, *extra, pool=pool)
            with pytest.raises(_lib.TgcnError, match="not a multiple of pool"), torch.no_grad():
                st(layer, xs, *extra, pool=pool)
        # every refusal forward_series makes for the same arguments
        for kw, rule in ((dict(stride=2, dilation=2), "together with stride"), (dict(padding=3), r"padding \(\d+, \d+\) outside"),
                         (dict(dilation=0), "dilation is an integer >= 1"), (dict(dilation=5), "fewer than one window"), (dict(stride=0), "stride is an integer")):
            with pytest.raises(_lib.TgcnError, match=rule):
                sr(layer, x, *extra, **kw)
        with pytest.raises(_lib.TgcnError, match="channel"):
            sr(layer, torch.randn(2, 8, 10, 3), *extra)
        with pytest.raises(_lib.TgcnError, match=r"\(S, n, T\) or \(S, n, T, f\)"):
            sr(layer, torch.randn(2, 8), *extra)
        # ... and forward_stream: grad mode, an empty chunk, a foreign state, a state made for a window step
        with pytest.raises(_lib.TgcnError, match="no backward"):
            st(layer, x, *extra)
        with pytest.raises(_lib.TgcnError, match="at least one time row"), torch.no_grad():
            st(layer, x[:, :, :0], *extra)
        with pytest.raises(_lib.TgcnError, match="dilation is an integer"), torch.no_grad():
            st(layer, x, *extra, dilation=0)
        for bad_state, rule in ((F.SeriesStreamState(_op("plain"), torch.float32, 2, 8, 4, 3, 3, 1, "cpu", stride=2), "stride 2"),
                                (F.SeriesStreamState(_op("plain"), torch.float32, 2, 8, 4, 3, 3, 2, "cpu"), "dilation 2"),
                                (F.SeriesStreamState(_op("plain"), torch.float32, 2, 8, 4, 3, 3, 1, "cpu"), "another operand"), (object(), "SeriesStreamState")):
            with pytest.raises(_lib.TgcnError, match=rule), torch.no_grad():
                st(layer, x, *extra, state=bad_state)
        with pytest.raises(_lib.TgcnError, match="capturable=True with a state"), torch.no_grad():
            st(layer, x, *extra, state=F.SeriesStreamState(_op("plain"), torch.float32, 2, 8, 4, 3, 3, 1, "cpu"), capturable=True)
        # no time_chunk, fused or stream stride keyword
        for fn, kw in ((sr, dict(time_chunk=4)), (st, dict(fused=True)), (st, dict(stride=2)), (sr, dict(fused=True))):
            with pytest.raises(TypeError):
                fn(layer, x, *extra, **kw)
    # bf16 parameters: cheb_relu_pool's wording
    for layer, extra in ((tgcn_amd.TGCNCheb_H(torch.eye(8), 4, 3, 3, 3).to(BF), ()), (tgcn_amd.ChebTimeConv(4, 3, 3, 3).to(BF), (ei,))):
        for fn in (sr, st):
            with pytest.raises(_lib.TgcnError, match=r"bfloat16 parameters are not supported \(run the layer, then gcn_pool / gcn_pool_4\)"), torch.no_grad():
                fn(layer, x.to(BF), *extra)
    for fn, args in ((F.cheb_time_windows_relu_pool, (_op("plain"), torch.randn(2, N_V, 10, 4).to(BF), torch.randn(3, 3, 4, 8).to(BF), None, 0, 0, 4)),
                     (F.cheb_time_stream_relu_pool, (_op("plain"), torch.randn(2, N_V, 10, 4).to(BF), torch.randn(3, 3, 4, 8).to(BF), None, 0, 0, 4))):
        with pytest.raises(_lib.TgcnError, match=r"bfloat16 parameters are not supported \(run the layer, then gcn_pool / gcn_pool_4\)"), torch.no_grad():
            fn(*args)
    # a learnable edge weight, another layer class, graph arguments that do not fit the class
    for fn in (sr, st):
        with pytest.raises(_lib.TgcnError, match="learnable edge weights"):
            fn(c, x, ei, torch.ones(2, requires_grad=True))
        with pytest.raises(_lib.TgcnError, match="TGCNCheb_H or a ChebTimeConv"):
            fn(tgcn_amd.GCNCheb(torch.eye(8), 4, 3, 3), x)
        with pytest.raises(_lib.TgcnError, match="takes"):
            fn(h, x, ei)
        with pytest.raises(_lib.TgcnError, match="takes"):
            fn(c, x)
    # the functional entries on their own
    op = _op("plain")
    with pytest.raises(_lib.TgcnError, match="pool is 2 or 4"):
        F.cheb_time_windows_relu_pool(op, torch.randn(2, N_V, 10, 4), torch.randn(3, 3, 4, 8), None, 0, 0, 3)
    with pytest.raises(_lib.TgcnError, match="not a multiple of pool"):
        F.cheb_time_windows_relu_pool(_op("plain"), torch.randn(2, 6, 10, 4), torch.randn(3, 3, 4, 8), None, 0, 0, 4)
    with pytest.raises(_lib.TgcnError, match="takes a"):
        F.cheb_time_windows_relu_pool(op, torch.randn(2, N_V, 10, 4), torch.randn(3, 3, 8), None, 0, 0, 4)
    with pytest.raises(_lib.TgcnError, match="not a multiple of pool"), torch.no_grad():
        F.cheb_time_stream_relu_pool(op, torch.randn(2, 6, 10, 4), torch.randn(3, 3, 4, 8), None, 0, 0, 4)
    assert rec.calls == []


# what forward_series / forward_stream logged before this file existed: one list per call, pinned
PINNED = {
    "h-series-default": ['fold_weight 3 96 0', 'csr_hop2 2 48 1 0 0 1024', 'csr_hop2 2 48 1 0 0 1024', 'cheb_project_series 2 64 12 4 3 8 3 2 0'],
    "h-series-causal-dil2-as-series": ['series_conv_plan 3 4 8 1 1', 'fold_weight 3 96 0', 'csr_hop2 2 48 1 0 0 1024', 'csr_hop2 2 48 1 0 0 1024',
                                       'cheb_project_series_dilated 2 64 12 4 3 8 3 2 1 1 4 0 2'],
    "c-series-stride2": ['series_conv_plan 3 4 8 1 2', 'csr_hop2 2 48 1 0 0 1024', 'csr_hop2 2 48 2 -1 0 1024',
                         'cheb_project_series_conv 2 64 12 4 3 8 3 1 0 2 0 0'],
    "h-single-channel-window-major": ['fold_weight 3 24 0', 'csr_hop2 2 12 1 0 0 1024', 'csr_hop2 2 12 1 0 0 1024',
                                      'cheb_project_windows 64 12 3 8 3 2', 'cheb_project_windows 64 12 3 8 3 2'],
    "h-stream": ['series_conv_plan 3 4 8 1 1', 'fold_weight 3 96 0', 'csr_hop2 2 20 1 0 0 1024', 'csr_hop2 2 20 1 0 0 1024',
                 'cheb_project_series_stream 2 64 5 4 3 8 3 2 16 0 2'],
    "c-stream-capturable": ['series_conv_plan 3 4 8 1 1', 'csr_hop2 2 20 1 0 0 1024', 'csr_hop2 2 20 2 -1 0 1024',
                            'cheb_project_series_stream_pos 2 64 5 4 3 8 3 1 8 1'],
}


def _pinned_calls(rec, monkeypatch):
    _stub_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    torch.manual_seed(0)
    h, c, h1 = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3), tgcn_amd.ChebTimeConv(4, 8, 3, 3), tgcn_amd.TGCNCheb_H(torch.eye(N_V), 1, 8, 3, 3)
    x = torch.randn(2, N_V, T_WIN, 4)
    got = {}
    with torch.no_grad():
        for name, fn in (("h-series-default", lambda: h.forward_series(x)),
                         ("h-series-causal-dil2-as-series", lambda: h.forward_series(x, as_series=True, padding="causal", dilation=2)),
                         ("c-series-stride2", lambda: c.forward_series(x, ei, stride=2)),
                         ("h-single-channel-window-major", lambda: h1.forward_series(x[..., 0])),
                         ("h-stream", lambda: h.forward_stream(x[:, :, :5], dilation=2)),
                         ("c-stream-capturable", lambda: c.forward_stream(x[:, :, :5], ei, capturable=True))):
            del rec.calls[:]
            fn()
            got[name] = list(rec.calls)
    return got


def test_forward_series_and_forward_stream_log_what_they_logged(recorder, monkeypatch):
    rec = recorder({})
    assert _pinned_calls(rec, monkeypatch) == PINNED


def test_the_new_entries_are_declared_everywhere():
    """the header, the ctypes table and the library agree on the three entries; the ABI is still 8"""
    names = ["tgcn_series_pool_plan", "tgcn_cheb_project_series_pool_f32", "tgcn_cheb_project_series_stream_pool_f32"]
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "tgcn_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert nm in _lib.SIGNATURES and hasattr(handle, nm) and (" " + nm + "(") in header, nm
    assert _lib.ABI_VERSION == 8 and _lib.lib().tgcn_abi_version() == 8 and "#define TGCN_ABI_VERSION 8" in header


def _plan(H, f, N, stride, pool, conv=False):
    L = _lib.lib()
    hc, lds = ctypes.c_int32(-1), ctypes.c_int32(-1)
    if conv:
        rc = L.tgcn_series_conv_plan(H, f, N, int(f % 4 == 0), stride, ctypes.byref(hc), ctypes.byref(lds))
    else:
        rc = L.tgcn_series_pool_plan(H, f, N, int(f % 4 == 0), stride, pool, ctypes.byref(hc), ctypes.byref(lds))
    return rc, hc.value, lds.value


def test_the_pool_plan_keeps_the_regime_and_takes_the_larger_lds():
    """host only (the 64 KB limit is tried first, so the answers hold with and without a device)"""
    for H, f, N, stride in ((1, 1, 40, 1), (3, 4, 5, 1), (3, 4, 40, 2), (5, 3, 72, 1), (15, 72, 40, 1), (16, 72, 40, 1), (6, 64, 24, 1)):
        rc0, hc0, lds0 = _plan(H, f, N, stride, 0, conv=True)
        scratch = 4 * 32 * (16 if N <= 16 else (32 if N <= 32 else 64)) * 4
        for pool in (2, 4):
            rc, hc, lds = _plan(H, f, N, stride, pool)
            assert (rc, hc) == (rc0, hc0) == (0, hc) and lds == max(lds0, scratch), (H, f, N, stride, pool)
    # one tap of one channel into 40 columns: the GEMM needs about 11 KB, the scratch 32 KB
    assert _plan(1, 1, 40, 1, 0, conv=True)[2] < 12 * 1024 and _plan(1, 1, 40, 1, 4)[2] == 32 * 1024
    # H = 15, f = 72 is the last horizon whose four spans and weight tile fit 64 KB whole (64 704 B); H = 16 is staged in chunks of 15
    assert _plan(15, 72, 40, 1, 4)[1:] == (15, 64704) and _plan(16, 72, 40, 1, 4)[1] == 15
    for pool in (0, 1, 3, 8, -2):
        assert _plan(3, 4, 8, 1, pool)[0] == -1
    assert _plan(0, 4, 8, 1, 4)[0] == -1 and _plan(3, 4, 8, 0, 4)[0] == -1
    L = _lib.lib()
    assert L.tgcn_series_pool_plan(3, 4, 8, 1, 1, 4, None, None) == -1


def test_the_scalar_rules_answer_invalid_before_a_pointer_is_read():
    """never-read pointers: every call below must return before it touches one (TGCN_ERR_INVALID = -1, TGCN_ERR_UNSUPPORTED = -4)"""
    L = _lib.lib()
    bad = ctypes.c_void_p(16)

    def pool_entry(S=2, n=48, T=20, f=4, H=3, N=8, K=3, bias=None, bias_kind=0, as_series=0, z=bad, pool=4, stride=1, left=0, right=0, dil=1,
                   stack=bad, W=bad):
        return L.tgcn_cheb_project_series_pool_f32(None, S, n, T, f, H, N, K, stack, W, bias, bias_kind, as_series, z, None, pool, stride, left, right, dil)

    for pool in (0, 1, 3, 8, -4):
        assert pool_entry(pool=pool) == -1
    assert pool_entry(n=50, pool=4) == -1 and pool_entry(n=49, pool=2) == -1 and pool_entry(n=0) == -1
    assert pool_entry(stack=None) == -1 and pool_entry(W=None) == -1 and pool_entry(z=None) == -1
    assert pool_entry(bias_kind=1) == -1 and pool_entry(bias_kind=3) == -1
    # the _conv / _dilated entries' geometry rules
    assert pool_entry(left=3) == -1 and pool_entry(right=3) == -1 and pool_entry(stride=0) == -1 and pool_entry(T=2) == -1
    assert pool_entry(dil=0) == -1 and pool_entry(dil=10) == -1 and pool_entry(dil=2, left=5) == -1
    assert pool_entry(stride=2, dil=2) == -4
    assert pool_entry(S=0) == -1 and pool_entry(K=0) == -1 and pool_entry(f=0) == -1 and pool_entry(N=0) == -1

    def stream_entry(S=2, n=48, Tc=5, f=4, H=3, N=8, K=3, bias=None, bias_kind=0, z=bad, pool=4, ring=bad, ring_ld=8, head=0, pos=None, dil=1,
                     stack=bad, W=bad):
        return L.tgcn_cheb_project_series_stream_pool_f32(None, S, n, Tc, f, H, N, K, stack, W, bias, bias_kind, z, pool, ring, ring_ld, head, pos, dil)

    for pool in (0, 1, 3, 8):
        assert stream_entry(pool=pool) == -1
    assert stream_entry(n=50) == -1 and stream_entry(n=49, pool=2) == -1
    assert stream_entry(stack=None) == -1 and stream_entry(W=None) == -1 and stream_entry(z=None) == -1 and stream_entry(ring=None) == -1
    # the ring / head / geometry rules of the stream entries
    assert stream_entry(head=2) == -1 and stream_entry(head=-1) == -1 and stream_entry(ring_ld=7) == -1 and stream_entry(Tc=0) == -1
    assert stream_entry(dil=0) == -1 and stream_entry(dil=2, ring_ld=8) == -1 and stream_entry(bias_kind=2) == -1
    assert stream_entry(H=1, dil=0) == -1 and stream_entry(H=1, stack=None) == -1 and stream_entry(H=1, pool=3) == -1
