"""CPU test of the launches of the relu + dropout + pool calls (cheb_series_relu_dropout_pool / cheb_relu_dropout_pool,
F.cheb_time_windows_relu_dropout_pool), by the recorder of tests/test_layer_dispatch.py: a fused call asks the pool plan once, runs K - 1
hops and launches exactly one cheb_project_series_pool_dropout carrying thr and scale and a non-null seed, with a null idx under no_grad
and no relu_pool or unpooled entry; its backward is relu_pool_bwd and then what the unpooled backward logs; a reordered operand logs the
unpooled entry, then relu_dropout_pool; p = 0 and training=False log exactly cheb_series_relu_pool's calls; every refusal raises with
nothing logged and no operand built; the three entries are in the header, the ctypes table and the library at ABI 8, and their scalar
rules answer TGCN_ERR_INVALID before a pointer is read."""
import contextlib
import ctypes
import os

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F

from test_dropout_mask import scale_of, thr_of
from test_layer_dispatch import N_V, T_WIN, _op, recorder  # noqa: F401  (the recorder fixture)
from test_series_stream_dispatch import BF, _entries, _no_operands, _stub_operands

ENTRY, POOL_ENTRY, PASS = "cheb_project_series_pool_dropout", "cheb_project_series_pool", "relu_dropout_pool"
SIG = _lib.SIGNATURES["tgcn_cheb_project_series_pool_dropout_f32"][1]
IDX_ARG, SEED_ARG = 14, 20


def test_the_entry_takes_the_pooled_entrys_arguments_then_seed_thr_scale():
    pooled = _lib.SIGNATURES["tgcn_cheb_project_series_pool_f32"][1]
    assert SIG[:len(pooled)] == pooled and SIG[len(pooled):] == [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float]
    assert SIG[IDX_ARG] is ctypes.c_void_p and SIG[IDX_ARG - 1] is ctypes.c_void_p and SIG[SEED_ARG] is ctypes.c_void_p and len(SIG) == 23
    assert _lib.SIGNATURES["tgcn_relu_dropout_pool_f32"][1] == _lib.SIGNATURES["tgcn_relu_pool_f32"][1] + [ctypes.c_int32, ctypes.c_void_p,
                                                                                                          ctypes.c_uint32, ctypes.c_float]


def _tail(p):
    """the scalars the mask adds to a logged call"""
    return "%d %g" % (thr_of(p), scale_of(p))


def _call(rec, op, series, W, mode, train, pool, p, seed, bias_kind=F.BIAS_CHANNEL, **kw):
    del rec.calls[:], rec.nulls[:]
    torch.manual_seed(1)
    series, W = series.clone(), W.clone()
    bias = torch.randn(W.shape[-1]) if bias_kind == F.BIAS_CHANNEL else torch.randn(N_V * W.shape[-1])
    for t in (series, W, bias):
        t.requires_grad_(train)
    with (contextlib.nullcontext() if train else torch.no_grad()):
        z = F.cheb_time_windows_relu_dropout_pool(op, series, W, bias, bias_kind, mode, pool, p, seed, **kw)
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
@pytest.mark.parametrize("pool,p,seed", [(2, 0.1, None), (4, 0.5, 12345), (4, 0.1, "tensor")])
@pytest.mark.parametrize("geo", GEOS, ids=["default", "stride2-pad1", "causal-dil2"])
def test_a_fused_call_logs_plan_hops_and_one_dropout_entry(geo, pool, p, seed, f, mode, as_series, train, recorder):
    rec = recorder({})
    kw, (stride, left, right, dil), bwd_entry, bwd_geo = geo
    S, T, H, N, K = 2, T_WIN, 3, 8, 3
    nwin = (T + left + right - (H - 1) * dil - 1) // stride + 1
    torch.manual_seed(0)
    series, W = (torch.randn(S, N_V, T), torch.randn(K, H, N)) if f == 1 else (torch.randn(S, N_V, T, f), torch.randn(K, H, f, N))
    seed = torch.tensor([7]) if seed == "tensor" else seed
    z, calls, nulls, n_fwd = _call(rec, _op("plain"), series, W, mode, train, pool, p, seed, as_series=as_series, **kw)
    assert tuple(z.shape) == ((S, N_V // pool, nwin, N) if as_series else (S * nwin, N_V // pool, N)) and z.is_contiguous()
    ent = _entries(calls)
    # the pool plan first and once, unchanged: H f N vec stride pool
    assert calls[0] == "series_pool_plan %d %d %d %d %d %d" % (H, f, N, int(f % 4 == 0), stride, pool) and ent.count("series_pool_plan") == 1
    # K - 1 hops, then exactly one dropout entry: the pooled entry's scalars, then thr and scale
    i_fwd = ent.index(ENTRY)
    assert ent.count(ENTRY) == 1 and i_fwd == n_fwd - 1
    hops = [c for c in calls[:i_fwd] if c.startswith("csr_hop2 ")]
    assert len(hops) == K - 1 and all(c.split()[1:3] == [str(S), str(T * f)] for c in hops)
    assert calls[i_fwd] == "%s %d %d %d %d %d %d %d 1 %d %d %d %d %d %d %s" % (ENTRY, S, N_V, T, f, H, N, K, int(as_series), pool, stride, left, right,
                                                                             dil, _tail(p))
    assert set(ent[:n_fwd]) <= {"series_pool_plan", "csr_hop2", "fold_weight", ENTRY}, ent
    # no undropped pooled entry, no unpooled projection, no separate pass
    assert not {POOL_ENTRY, "cheb_project_series", "cheb_project_series_conv", "cheb_project_series_dilated", "cheb_project_windows", "relu_pool",
                PASS, "series_conv_plan"} & set(ent)
    # the seed is never null; idx is null under no_grad and stored when something trains
    assert SEED_ARG not in nulls[i_fwd] and (IDX_ARG in nulls[i_fwd]) == (not train)
    back = calls[n_fwd:]
    if not train:
        assert back == []
        return
    # the backward: relu_pool_bwd on the forward's layout (on gz * scale), then ChebSeriesFn's backward entry, then the adjoint hops
    q, fN = (S, nwin * N) if as_series else (S * nwin, N)
    assert back[0] == "relu_pool_bwd %d %d %d %d" % (q, N_V, fN, pool)
    assert back[1] == "%s %d %d %d %d %d %d %d %d 1024%s" % (bwd_entry, S, N_V, T, f, H, N, K, int(as_series), bwd_geo)
    assert _entries(back).count("csr_hop2") == K - 1 and set(_entries(back)) <= {"relu_pool_bwd", bwd_entry, "csr_hop2", "fold_weight"}, back


@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("f", [1, 4])
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
def test_a_reordered_operand_logs_the_unpooled_entry_then_relu_dropout_pool(as_series, f, train, recorder):
    rec = recorder({})
    S, T, H, N, K, pool, p = 2, T_WIN, 3, 8, 3, 4, 0.1
    nwin = T - H + 1
    torch.manual_seed(0)
    series, W = (torch.randn(S, N_V, T), torch.randn(K, H, N)) if f == 1 else (torch.randn(S, N_V, T, f), torch.randn(K, H, f, N))
    z, calls, nulls, n_fwd = _call(rec, _op("reordered"), series, W, 1, train, pool, p, None, as_series=as_series)
    assert tuple(z.shape) == ((S, N_V // pool, nwin, N) if as_series else (S * nwin, N_V // pool, N))
    ent = _entries(calls)
    assert not any("pool_plan" in e or e in (ENTRY, POOL_ENTRY, "relu_pool") for e in ent)
    assert ent.count("cheb_project_series") == 1 and "cheb_project_series %d %d %d %d %d %d %d 1 %d" % (S, N_V, T, f, H, N, K, int(as_series)) in calls
    # one pass on the layer's layout: q n f pool N thr scale -- the window count rides in f / N
    q, fN = (S, nwin * N) if as_series else (S * nwin, N)
    assert [c for c in calls if c.startswith(PASS + " ")] == ["%s %d %d %d %d %d %s" % (PASS, q, N_V, fN, pool, N, _tail(p))]
    i = ent.index(PASS)
    assert ent.index("cheb_project_series") < i < n_fwd and 9 not in nulls[i]          # the seed of the pass
    assert [c for c in calls if c.startswith("relu_pool_bwd ")] == (["relu_pool_bwd %d %d %d %d" % (q, N_V, fN, pool)] if train else [])


def test_p_zero_and_eval_log_exactly_the_undropped_calls(recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    assert tgcn_amd.cheb_series_relu_dropout_pool is tgcn_amd.nn.cheb_series_relu_dropout_pool
    assert tgcn_amd.cheb_relu_dropout_pool is tgcn_amd.nn.cheb_relu_dropout_pool
    for layer, extra, kind in ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3), (), 2), (tgcn_amd.ChebTimeConv(4, 8, 3, 3), (ei,), 1)):
        series = torch.randn(2, N_V, T_WIN, 4)
        for kw in (dict(), dict(as_series=True, padding="causal", dilation=2, pool=2)):
            del rec.calls[:]
            with torch.no_grad():
                tgcn_amd.cheb_series_relu_pool(layer, series, *extra, **kw)
            want = list(rec.calls)
            assert POOL_ENTRY in _entries(want)
            for off in (dict(training=False), dict(p=0), dict(p=0.0, seed=5), dict(training=False, p=0.9, seed=torch.tensor([3]))):
                del rec.calls[:]
                with torch.no_grad():
                    tgcn_amd.cheb_series_relu_dropout_pool(layer, series, *extra, **off, **kw)
                assert rec.calls == want, (off, kw)
            # switched on, the module passes everything on: pool = 4 and p = 0.5 are the defaults
            del rec.calls[:]
            with torch.no_grad():
                z = tgcn_amd.cheb_series_relu_dropout_pool(layer, series, *extra, **kw)
            pool = kw.get("pool", 4)
            geo = "1 %d 1 4 0 2" % pool if kw else "0 4 1 0 0 1"
            assert rec.calls[-1] == "%s 2 %d %d 4 3 8 3 %d %s %s" % (ENTRY, N_V, T_WIN, kind, geo, _tail(0.5))
            assert [c.replace(ENTRY, POOL_ENTRY) for c in rec.calls[:-1]] == want[:-1]
        z = tgcn_amd.cheb_series_relu_dropout_pool(layer, series, *extra, p=0.1, seed=9)
        z.sum().backward()
        assert _entries(rec.calls).count("relu_pool_bwd") == 1 and layer.weight.grad is not None
    # the batch layers: the layer's own calls, then one pass; off, cheb_relu_pool's calls
    g = tgcn_amd.GCNCheb(torch.eye(N_V), 4, 8, 3)
    x = torch.randn(3, N_V, 4)
    del rec.calls[:]
    with torch.no_grad():
        g(x)
    layer_calls = list(rec.calls)
    del rec.calls[:]
    with torch.no_grad():
        z = tgcn_amd.cheb_relu_dropout_pool(g, x, p=0.1, pool=2)
    assert tuple(z.shape) == (3, N_V // 2, 8) and rec.calls == layer_calls + ["%s 3 %d 8 2 8 %s" % (PASS, N_V, _tail(0.1))]
    del rec.calls[:]
    with torch.no_grad():
        tgcn_amd.cheb_relu_pool(g, x, pool=2)
    want = list(rec.calls)
    for off in (dict(training=False), dict(p=0)):
        del rec.calls[:]
        with torch.no_grad():
            tgcn_amd.cheb_relu_dropout_pool(g, x, pool=2, **off)
        assert rec.calls == want


def test_refusals_launch_nothing_and_build_no_operand(recorder, monkeypatch):
    rec = recorder({})
    _no_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    h, c = tgcn_amd.TGCNCheb_H(torch.eye(8), 4, 3, 3, 3), tgcn_amd.ChebTimeConv(4, 3, 3, 3)
    x = torch.randn(2, 8, 10, 4)
    sd = tgcn_amd.cheb_series_relu_dropout_pool
    for layer, extra in ((h, ()), (c, (ei,))):
        for p in (-0.1, 1, 1.0, 2, float("nan"), None, "0.5", True):
            for training in (True, False):
                with pytest.raises(_lib.TgcnError, match=r"p is a real number in \[0, 1\)"):
                    sd(layer, x, *extra, p=p, training=training)
        for seed in (-1, 2 ** 62, 0.5, "1", True):
            with pytest.raises(_lib.TgcnError, match="seed is None, an integer"):
                sd(layer, x, *extra, seed=seed)
        for seed in (torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(1), torch.zeros(1, dtype=torch.int64, device="meta")):
            with pytest.raises(_lib.TgcnError, match="one int64 element"):
                sd(layer, x, *extra, seed=seed)
        # everything cheb_series_relu_pool refuses, switched on and off
        for training in (True, False):
            for pool in (0, 1, 3, 8, 2.0, True, None, "4"):
                with pytest.raises(_lib.TgcnError, match="pool is 2 or 4"):
                    sd(layer, x, *extra, pool=pool, training=training)
            with pytest.raises(_lib.TgcnError, match="not a multiple of pool"):
                sd(layer, torch.randn(2, 10, 10, 4), *extra, training=training)
            for kw, rule in ((dict(stride=2, dilation=2), "together with stride"), (dict(padding=3), r"padding \(\d+, \d+\) outside"),
                             (dict(dilation=0), "dilation is an integer >= 1"), (dict(dilation=5), "fewer than one window"), (dict(stride=0), "stride is an integer")):
                with pytest.raises(_lib.TgcnError, match=rule):
                    sd(layer, x, *extra, training=training, **kw)
            with pytest.raises(_lib.TgcnError, match="channel"):
                sd(layer, torch.randn(2, 8, 10, 3), *extra, training=training)
            with pytest.raises(_lib.TgcnError, match=r"\(S, n, T\) or \(S, n, T, f\)"):
                sd(layer, torch.randn(2, 8), *extra, training=training)
        for kw in (dict(time_chunk=4), dict(fused=True)):
            with pytest.raises(TypeError):
                sd(layer, x, *extra, **kw)
    # bf16 parameters: cheb_series_relu_pool's wording
    for layer, extra in ((tgcn_amd.TGCNCheb_H(torch.eye(8), 4, 3, 3, 3).to(BF), ()), (tgcn_amd.ChebTimeConv(4, 3, 3, 3).to(BF), (ei,))):
        with pytest.raises(_lib.TgcnError, match=r"bfloat16 parameters are not supported \(run the layer, then gcn_pool / gcn_pool_4\)"):
            sd(layer, x.to(BF), *extra)
    with pytest.raises(_lib.TgcnError, match=r"bfloat16 parameters are not supported \(run the layer, then gcn_pool / gcn_pool_4\)"):
        F.cheb_time_windows_relu_dropout_pool(_op("plain"), torch.randn(2, N_V, 10, 4).to(BF), torch.randn(3, 3, 4, 8).to(BF), None, 0, 0, 4, 0.5, 1)
    with pytest.raises(_lib.TgcnError, match=r"bfloat16 parameters are not supported \(run the layer, then gcn_pool / gcn_pool_4\)"):
        tgcn_amd.cheb_relu_dropout_pool(tgcn_amd.GCNCheb(torch.eye(8), 4, 3, 3).to(BF), torch.randn(2, 8, 4).to(BF))
    with pytest.raises(_lib.TgcnError, match="learnable edge weights"):
        sd(c, x, ei, torch.ones(2, requires_grad=True))
    with pytest.raises(_lib.TgcnError, match="TGCNCheb_H or a ChebTimeConv"):
        sd(tgcn_amd.GCNCheb(torch.eye(8), 4, 3, 3), x)
    with pytest.raises(_lib.TgcnError, match="takes"):
        sd(h, x, ei)
    # the functional entries on their own
    op = _op("plain")
    args = (torch.randn(2, N_V, 10, 4), torch.randn(3, 3, 4, 8), None, 0, 0)
    with pytest.raises(_lib.TgcnError, match="pool is 2 or 4"):
        F.cheb_time_windows_relu_dropout_pool(op, *args, 3, 0.5, 1)
    with pytest.raises(_lib.TgcnError, match=r"p is a real number in \[0, 1\)"):
        F.cheb_time_windows_relu_dropout_pool(op, *args, 4, 1.0, 1)
    with pytest.raises(_lib.TgcnError, match="seed is None, an integer"):
        F.cheb_time_windows_relu_dropout_pool(op, *args, 4, 0.5, -3)
    with pytest.raises(_lib.TgcnError, match="takes a"):
        F.cheb_time_windows_relu_dropout_pool(op, torch.randn(2, N_V, 10, 4), torch.randn(3, 3, 8), None, 0, 0, 4, 0.5, 1)
    for bad in (dict(p=1.0), dict(seed=2 ** 62), dict(pool=3)):
        with pytest.raises(_lib.TgcnError):
            tgcn_amd.cheb_relu_dropout_pool(tgcn_amd.GCNCheb(torch.eye(8), 4, 3, 3), torch.randn(2, 8, 4), **bad)
    with pytest.raises(_lib.TgcnError, match=r"p is a real number in \[0, 1\)"):
        F.dropout_keep_mask(1, 0, 4, 1.5, "cpu")
    with pytest.raises(_lib.TgcnError, match="e0 >= 0 and count >= 1"):
        F.dropout_keep_mask(1, -1, 4, 0.5, "cpu")
    assert rec.calls == []


def test_the_new_entries_are_declared_everywhere():
    """the header, the ctypes table and the library agree on the three entries; the ABI is still 8"""
    names = ["tgcn_cheb_project_series_pool_dropout_f32", "tgcn_relu_dropout_pool_f32", "tgcn_dropout_keep_u8"]
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "tgcn_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert nm in _lib.SIGNATURES and hasattr(handle, nm) and (" " + nm + "(") in header, nm
    assert _lib.ABI_VERSION == 8 and _lib.lib().tgcn_abi_version() == 8 and "#define TGCN_ABI_VERSION 8" in header


def test_the_scalar_rules_answer_invalid_before_a_pointer_is_read():
    """never-read pointers: every call below must return before it touches one (TGCN_ERR_INVALID = -1, TGCN_ERR_UNSUPPORTED = -4)"""
    L = _lib.lib()
    bad = ctypes.c_void_p(16)

    def entry(S=2, n=48, T=20, f=4, H=3, N=8, K=3, bias=None, bias_kind=0, as_series=0, z=bad, pool=4, stride=1, left=0, right=0, dil=1,
              stack=bad, W=bad, seed=bad, thr=1 << 31, scale=2.0):
        return L.tgcn_cheb_project_series_pool_dropout_f32(None, S, n, T, f, H, N, K, stack, W, bias, bias_kind, as_series, z, None, pool, stride, left,
                                                           right, dil, seed, thr, scale)

    # the mask's own rules
    assert entry(seed=None) == -1
    for scale in (0.5, 0.0, -2.0, float("nan"), float("inf"), 0.99999994):
        assert entry(scale=scale) == -1, scale
    # everything the pooled entry refuses, with its codes
    for pool in (0, 1, 3, 8, -4):
        assert entry(pool=pool) == -1
    assert entry(n=50, pool=4) == -1 and entry(n=49, pool=2) == -1 and entry(n=0) == -1
    assert entry(stack=None) == -1 and entry(W=None) == -1 and entry(z=None) == -1
    assert entry(bias_kind=1) == -1 and entry(bias_kind=3) == -1
    assert entry(left=3) == -1 and entry(right=3) == -1 and entry(stride=0) == -1 and entry(T=2) == -1
    assert entry(dil=0) == -1 and entry(dil=10) == -1 and entry(dil=2, left=5) == -1
    assert entry(stride=2, dil=2) == -4
    assert entry(S=0) == -1 and entry(K=0) == -1 and entry(f=0) == -1 and entry(N=0) == -1

    def one_pass(y=bad, out=bad, q=3, n=48, f=16, pool=4, N=8, seed=bad, thr=5, scale=2.0):
        return L.tgcn_relu_dropout_pool_f32(None, y, out, None, q, n, f, pool, N, seed, thr, scale)

    assert one_pass(f=12) == -1 and one_pass(N=0) == -1 and one_pass(f=0) == -1          # f % N != 0
    assert one_pass(seed=None) == -1 and one_pass(scale=0.5) == -1 and one_pass(scale=float("nan")) == -1
    assert one_pass(y=None) == -1 and one_pass(out=None) == -1 and one_pass(q=0) == -1 and one_pass(n=50) == -1 and one_pass(pool=0) == -1

    def keep(seed=bad, e0=0, count=4, out=bad):
        return L.tgcn_dropout_keep_u8(None, seed, e0, count, 7, out)

    assert keep(seed=None) == -1 and keep(out=None) == -1 and keep(e0=-1) == -1 and keep(count=0) == -1 and keep(e0=2 ** 63 - 2, count=4) == -1
