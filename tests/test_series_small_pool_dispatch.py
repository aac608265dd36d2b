"""CPU test of the launches of relu (+ dropout) + pool in the one-launch series layer (tgcn_amd.cheb_series_relu_pool_fused /
F.cheb_time_windows_relu_pool_fused), by the recorder technique of tests/test_series_small_dispatch.py.  A fused call asks
tgcn_cheb_series_small_plan once and first, folds the weight at most once and launches tgcn_cheb_series_small_pool_f32 -- no hop, no
project_series entry, no relu_pool pass -- with an idx pointer only where something needs a gradient, a stack pointer only when the weight
trains and a seed pointer only with a mask; its backward is tgcn_relu_pool_bwd_f32, then the existing series backward entry of the geometry.
Every refusal raises TgcnError with nothing launched, and without an operand where none is needed; fused="auto" outside the measured rule
logs exactly what cheb_series_relu_pool / cheb_series_relu_dropout_pool log.  The entry is in the header, the ctypes table and the library at
ABI 8, refuses bad scalars before it reads a pointer, and small_series_pool_kernel's instantiations use no scratch and spill nothing."""
import contextlib
import ctypes
import inspect
import os
import sys

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F

from test_layer_dispatch import N_V, _Op, _op, _Recorder, recorder  # noqa: F401  (the recorder fixture)
from test_series_stream_dispatch import BF, _entries, _no_operands, _stub_operands

PLAN, ENTRY = "cheb_series_small_plan", "cheb_series_small_pool"
# positions of the pointers among tgcn_cheb_series_small_pool_f32's arguments
IDX_ARG, STACK_ARG, SEED_ARG = 15, 17, 21
T = 20
GEOMETRIES = {"default": dict(), "causal": dict(padding="causal"), "dilated": dict(padding=(1, 3), dilation=2)}
BACKWARD = {"default": "cheb_series_backward", "causal": "cheb_series_conv_backward", "dilated": "cheb_series_dilated_backward"}
EI = torch.tensor([[0, 1], [1, 0]])


def _layers(f, K=3, H=3, N=8):
    return ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), f, N, K, H), (), 0), (tgcn_amd.ChebTimeConv(f, N, K, H), (EI,), 1))


def _series(f, S=2):
    torch.manual_seed(3)
    x = torch.randn(S, N_V, T, f)
    return x[..., 0] if f == 1 else x


def _call(rec, fn, layer, extra, series, train, **kw):
    """the calls one pooled call (and its backward when train) logs"""
    del rec.calls[:], rec.nulls[:]
    series = series.clone().requires_grad_(train)
    with (contextlib.nullcontext() if train else torch.no_grad()):
        z = fn(layer, series, *extra, **kw)
    if train:
        z.backward(torch.ones_like(z))
    return z, list(rec.calls)


def test_the_signatures_are_the_documented_ones():
    sig = inspect.signature(tgcn_amd.cheb_series_relu_pool_fused)
    kw = {k: v.default for k, v in sig.parameters.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert kw == dict(pool=4, p=0.0, training=True, seed=None, as_series=False, padding=0, dilation=1, fused=True)
    sig = inspect.signature(F.cheb_time_windows_relu_pool_fused)
    assert list(sig.parameters) == ["op", "series", "weight", "bias", "bias_kind", "mode", "pool", "p", "seed", "as_series", "padding", "dilation", "fused"]
    assert "stride" not in sig.parameters and "time_chunk" not in sig.parameters
    assert [sig.parameters[k].default for k in ("p", "seed", "as_series", "padding", "dilation", "fused")] == [0.0, None, False, 0, 1, True]
    assert list(inspect.signature(F.series_pool_fused_supported).parameters) == ["op", "f", "H", "N", "K", "T", "padding", "dilation", "mode", "pool"]
    assert isinstance(F.SERIES_POOL_FUSED_AUTO, tuple) and set(F.SERIES_POOL_FUSED_AUTO) <= {"pool", "pool_dropout"}


@pytest.mark.parametrize("p", [0.0, 0.5], ids=["no-mask", "dropout"])
@pytest.mark.parametrize("geometry", ["default", "causal", "dilated"])
@pytest.mark.parametrize("f", [1, 4])
def test_a_fused_call_logs_the_plan_at_most_one_fold_and_the_pooled_entry(f, geometry, p, recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    geo = GEOMETRIES[geometry]
    K, H, N, S, pool = 3, 3, 8, 2, 4
    _, left, right, nwin = F.series_geometry(T, H, 1, geo.get("padding", 0), dilation=geo.get("dilation", 1))
    d = geo.get("dilation", 1)
    thr, scale = F.dropout_params(p)
    fn = tgcn_amd.cheb_series_relu_pool_fused
    for layer, extra, mode in _layers(f, K, H, N):
        folds = 1 if mode == 0 else 0          # power mode with K > 2
        bias_kind = 2 if mode == 0 else 1
        for as_series in (False, True):
            kw = dict(geo, as_series=as_series, pool=pool, p=p, seed=7)
            # the scalars in the entry's order: mode S T f H N K bias_kind as_series pool left right dilation thr scale
            want = "%s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %g" % (ENTRY, mode, S, T, f, H, N, K, bias_kind, int(as_series), pool, left, right, d,
                                                                          thr if p else 0, scale if p else 1.0)
            shape = (S, N_V // pool, nwin, N) if as_series else (S * nwin, N_V // pool, N)
            # no grad: the plan first, the fold, the entry; no idx, no stack
            z, calls = _call(rec, fn, layer, extra, _series(f), False, **kw)
            assert tuple(z.shape) == shape and z.dtype == torch.float32 and z.is_contiguous()
            assert calls[0] == "%s %d %d %d %d %d %d %d %d %d %d %d" % (PLAN, N_V, 256, mode, f, H, N, K, T, left, right, d)
            assert _entries(calls) == [PLAN] + ["fold_weight"] * folds + [ENTRY] and calls[-1] == want
            assert IDX_ARG in rec.nulls[-1] and STACK_ARG in rec.nulls[-1] and (SEED_ARG in rec.nulls[-1]) == (p == 0)
            # training=False drops the mask
            z, calls = _call(rec, fn, layer, extra, _series(f), False, training=False, **kw)
            assert calls[-1].split()[-2:] == ["0", "1"] and SEED_ARG in rec.nulls[-1]
            # training: idx and a stack, then relu_pool_bwd, the existing backward entry of the geometry and the adjoint hops
            z, calls = _call(rec, fn, layer, extra, _series(f), True, **kw)
            ent = _entries(calls)
            i = ent.index(ENTRY)
            assert ent[:i + 1] == [PLAN] + ["fold_weight"] * folds + [ENTRY] and calls[i] == want
            assert IDX_ARG not in rec.nulls[i] and STACK_ARG not in rec.nulls[i]
            assert ent.count("relu_pool_bwd") == 1 and ent.count(BACKWARD[geometry]) == 1 and i < ent.index("relu_pool_bwd") < ent.index(BACKWARD[geometry])
            assert not any(e.startswith("cheb_project_series") or e in ("series_conv_plan", "series_pool_plan", "cheb_series_small", "relu_pool",
                                                                        "relu_dropout_pool") for e in ent)
            assert not any(e.startswith("csr_hop") for e in ent[:ent.index(BACKWARD[geometry])])       # the forward hops nothing
            assert sum(e.startswith("csr_hop") for e in ent) == K - 1                                   # the adjoint hops of d series
            # a frozen weight: idx but no stack
            layer.weight.requires_grad_(False)
            z, calls = _call(rec, fn, layer, extra, _series(f), True, **kw)
            layer.weight.requires_grad_(True)
            j = _entries(calls).index(ENTRY)
            assert STACK_ARG in rec.nulls[j] and IDX_ARG not in rec.nulls[j]
            if p:
                assert z.grad_fn.seed.dtype == torch.int64 and int(z.grad_fn.seed) == 7
    # the functional entry without a bias, a 3-D series with a 3-D weight
    del rec.calls[:]
    with torch.no_grad():
        F.cheb_time_windows_relu_pool_fused(_op("plain"), torch.randn(2, N_V, T), torch.randn(K, H, N), None, F.BIAS_NONE, 1, 2, p=p, seed=3, **geo)
    assert _entries(rec.calls) == [PLAN, ENTRY]
    assert rec.calls[-1].split()[1:14] == [str(v) for v in (1, 2, T, 1, H, N, K, 0, 0, 2, left, right, d)]


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


def _functional(rec, op, series, W, fused, p=0.0, pool=4, **kw):
    del rec.calls[:]
    with torch.no_grad():
        F.cheb_time_windows_relu_pool_fused(op, series, W, None, F.BIAS_NONE, 1, pool, p=p, seed=5, fused=fused, **kw)
    return list(rec.calls)


def _general(rec, op, series, W, p=0.0, pool=4, **kw):
    del rec.calls[:]
    with torch.no_grad():
        if p == 0:
            F.cheb_time_windows_relu_pool(op, series, W, None, F.BIAS_NONE, 1, pool, **kw)
        else:
            F.cheb_time_windows_relu_dropout_pool(op, series, W, None, F.BIAS_NONE, 1, pool, p, 5, **kw)
    return list(rec.calls)


def test_every_refusal_comes_before_anything_is_built_or_launched(recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    x = _series(4)
    layers = _layers(4)
    fn = tgcn_amd.cheb_series_relu_pool_fused
    bf_layers = [(l.to(BF), e, m) for l, e, m in _layers(4)]
    del rec.calls[:]
    _no_operands(monkeypatch)
    W = torch.randn(3, 3, 4, 8)
    with torch.no_grad():
        for layer, extra, _ in layers:
            for bad in ("yes", 1, 0, None, False, "AUTO"):
                with pytest.raises(_lib.TgcnError, match="fused is True or"):
                    fn(layer, x, *extra, fused=bad)
            for kw, match in ((dict(pool=3), "pool is 2 or 4"), (dict(pool=True), "pool is 2 or 4"), (dict(p=1.0), r"p is a real number in \[0, 1\)"),
                              (dict(p=-0.1), "p is a real number"), (dict(p=0.5, seed=-1), "seed is None"), (dict(p=0.5, seed=2 ** 62), "seed is None"),
                              (dict(seed=torch.zeros(2, dtype=torch.int64)), "seed tensor"), (dict(padding=3), "padding"), (dict(dilation=0), "dilation"),
                              (dict(padding="same"), "padding")):
                with pytest.raises(_lib.TgcnError, match=match):
                    fn(layer, x, *extra, **kw)
            with pytest.raises(_lib.TgcnError, match="multiple of pool"):
                fn(layer, torch.randn(2, 62, T, 4), *extra, pool=4)
            with pytest.raises(_lib.TgcnError, match="channel"):
                fn(layer, torch.randn(2, N_V, T, 3), *extra)
            with pytest.raises(TypeError):
                fn(layer, x, *extra, stride=2)
            with pytest.raises(TypeError):
                fn(layer, x, *extra, time_chunk=4)
        for layer, extra, _ in bf_layers:
            for fused in (True, "auto"):
                with pytest.raises(_lib.TgcnError, match="bfloat16"):
                    fn(layer, x.to(BF), *extra, fused=fused)
        with pytest.raises(_lib.TgcnError, match="learnable edge weights"):
            fn(layers[1][0], x, EI, torch.ones(2, requires_grad=True))
        with pytest.raises(_lib.TgcnError, match="TGCNCheb_H or a ChebTimeConv"):
            fn(tgcn_amd.GCNCheb(torch.eye(N_V), 4, 8, 3), x)
        # the functional entry: the same, then the operand's own rules -- refused on its shape and labels, before the plan is asked
        with pytest.raises(_lib.TgcnError, match="float32 only"):
            F.cheb_time_windows_relu_pool_fused(_op("plain"), x.to(BF), W.to(BF), None, F.BIAS_NONE, 0, 4)
        with pytest.raises(_lib.TgcnError, match="pool is 2 or 4"):
            F.cheb_time_windows_relu_pool_fused(_op("plain"), x, W, None, F.BIAS_NONE, 0, 8)
        with pytest.raises(_lib.TgcnError, match="p is a real number"):
            F.cheb_time_windows_relu_pool_fused(_op("plain"), x, W, None, F.BIAS_NONE, 0, 4, p=1.5)
        with pytest.raises(_lib.TgcnError, match="seed is None"):
            F.cheb_time_windows_relu_pool_fused(_op("plain"), x, W, None, F.BIAS_NONE, 0, 4, p=0.5, seed=-3)
        with pytest.raises(_lib.TgcnError, match="padding"):
            F.cheb_time_windows_relu_pool_fused(_op("plain"), x, W, None, F.BIAS_NONE, 0, 4, padding=(0, 3))
        with pytest.raises(_lib.TgcnError, match="fused is True or"):
            F.cheb_time_windows_relu_pool_fused(_op("plain"), x, W, None, F.BIAS_NONE, 0, 4, fused=False)
        with pytest.raises(_lib.TgcnError, match="square operand"):
            F.cheb_time_windows_relu_pool_fused(_Op(N_V, 256, n_cols=N_V + 1), x, W, None, F.BIAS_NONE, 0, 4)
        with pytest.raises(_lib.TgcnError, match="reordered operand"):
            F.cheb_time_windows_relu_pool_fused(_op("reordered"), x, W, None, F.BIAS_NONE, 0, 4)
        assert not F.series_pool_fused_supported(_Op(N_V, 256, n_cols=N_V + 1), 4, 3, 8, 3, T, 0, 1, 0, 4)
        assert not F.series_pool_fused_supported(_op("reordered"), 4, 3, 8, 3, T, 0, 1, 0, 4)
        assert not F.series_pool_fused_supported(_op("plain"), 4, 3, 8, 3, T, 3, 1, 0, 4)       # a pad above H - 1: no query either
        assert not F.series_pool_fused_supported(_op("plain"), 4, 3, 8, 3, T, 0, 1, 0, 3)       # the pool rule: no query
        assert not F.series_pool_fused_supported(_Op(62, 256), 4, 3, 8, 3, T, 0, 1, 0, 4)
        assert rec.calls == []
        assert F.series_pool_fused_supported(_op("plain"), 4, 3, 8, 3, T, 0, 1, 0, 4) and _entries(rec.calls) == [PLAN]
    # a plan that refuses: the query is asked, nothing is launched; "auto" inside the rule then makes the general call's launches
    plain = _general(rec, _op("plain"), x, W)
    rrec = _RefusingRecorder({})
    monkeypatch.setattr(_lib, "lib", lambda: rrec)
    with torch.no_grad():
        with pytest.raises(_lib.TgcnError, match="do not fit the one-launch layer"):
            F.cheb_time_windows_relu_pool_fused(_op("plain"), x, W, None, F.BIAS_NONE, 1, 4)
    assert rrec.calls == [] and rrec.plans == 1
    assert not F.series_pool_fused_supported(_op("plain"), 4, 3, 8, 3, T, 0, 1, 0, 4) and rrec.plans == 2
    monkeypatch.setattr(F, "SERIES_POOL_FUSED_AUTO", ("pool", "pool_dropout"))
    assert _functional(rrec, _op("plain"), x, W, "auto") == plain and rrec.plans == 3


@pytest.mark.parametrize("p", [0.0, 0.5], ids=["no-mask", "dropout"])
def test_auto_outside_the_rule_logs_the_general_pooled_call(p, recorder, monkeypatch):
    rec = recorder({})
    _stub_operands(monkeypatch)
    klass = "pool" if p == 0 else "pool_dropout"
    other = "pool_dropout" if p == 0 else "pool"
    monkeypatch.setattr(F, "SERIES_POOL_FUSED_AUTO", (other,))          # this call's class is not listed
    for f in (1, 4):
        for layer, extra, _ in _layers(f):
            for geometry in GEOMETRIES:
                for train in (False, True):
                    kw = dict(GEOMETRIES[geometry], pool=2, as_series=True)
                    if p == 0:
                        _, want = _call(rec, tgcn_amd.cheb_series_relu_pool, layer, extra, _series(f), train, **kw)
                    else:
                        _, want = _call(rec, tgcn_amd.cheb_series_relu_dropout_pool, layer, extra, _series(f), train, p=p, seed=9, **kw)
                    _, auto = _call(rec, tgcn_amd.cheb_series_relu_pool_fused, layer, extra, _series(f), train, p=p, seed=9, fused="auto", **kw)
                    assert want and auto == want and PLAN not in _entries(auto) and ENTRY not in _entries(auto)
    # through the functional entry: outside the rule, a reordered operand inside it, and inside the rule
    x, W = _series(4), torch.randn(3, 3, 4, 8)
    plain = _general(rec, _op("plain"), x, W, p=p)
    assert _functional(rec, _op("plain"), x, W, "auto", p=p) == plain
    monkeypatch.setattr(F, "SERIES_POOL_FUSED_AUTO", (klass,))
    assert _entries(_functional(rec, _op("plain"), x, W, "auto", p=p)) == [PLAN, ENTRY]
    assert _functional(rec, _op("plain"), x, W, "auto", p=p) == _functional(rec, _op("plain"), x, W, True, p=p)
    reordered = _general(rec, _op("reordered"), x, W, p=p)
    auto = _functional(rec, _op("reordered"), x, W, "auto", p=p)
    assert auto == reordered and PLAN not in _entries(auto) and ENTRY not in _entries(auto)
    monkeypatch.setattr(F, "SERIES_POOL_FUSED_AUTO", ())
    assert _functional(rec, _op("plain"), x, W, "auto", p=p) == plain


def test_the_shipped_auto_rule_is_what_the_profile_gave():
    """F.SERIES_POOL_FUSED_AUTO lists a class only where profiles/r24_series_small_pool.json has the new call below both comparators by more
    than the largest spread, on every measured operand, forward and forward + backward"""
    import json
    path = os.path.join(os.path.dirname(_lib.__file__), "..", "profiles", "r24_series_small_pool.json")
    prof = json.load(open(path))
    assert tuple(prof["auto"]["classes"]) == F.SERIES_POOL_FUSED_AUTO
    for klass in ("pool", "pool_dropout"):
        rows = [r for r in prof["rows"] if r["class"] == klass and r["label"] == "this"]
        assert rows, klass
        wins = all(r["fused"]["median_ms"] + max(r[c]["spread_ms"] for c in ("fused", "general", "composed")) < min(r["general"]["median_ms"],
                                                                                                                  r["composed"]["median_ms"]) for r in rows)
        assert wins == (klass in F.SERIES_POOL_FUSED_AUTO), klass


def test_the_pooled_entry_is_declared_everywhere_and_refuses_before_it_reads():
    nm = "tgcn_cheb_series_small_pool_f32"
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "tgcn_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert nm in _lib.SIGNATURES and hasattr(handle, nm) and (" " + nm + "(") in header
    assert len(_lib.SIGNATURES[nm][1]) == 24
    L = _lib.lib()
    assert L.tgcn_abi_version() == 8 == _lib.ABI_VERSION and "#define TGCN_ABI_VERSION 8" in header
    one = ctypes.c_void_p(16)       # a non-null pointer that the refused calls never read
    A = _lib.CsrStruct(48, 300, 16, 16, None)

    def entry(series=one, W=one, z=one, A_=A, S=2, bias_kind=0, left=0, T_=20, pool=4, seed=None, scale=1.0, idx=one, stack=one):
        return L.tgcn_cheb_series_small_pool_f32(None, ctypes.byref(A_) if A_ is not None else None, 0, S, T_, 4, 3, 8, 3, series, W, None, bias_kind, 1, z,
                                                 idx, pool, stack, left, 0, 1, seed, 0, scale)
    # the unpooled entry's own codes
    assert entry(series=None) == -1 and entry(W=None) == -1 and entry(z=None) == -1 and entry(A_=None) == -1
    assert entry(S=0) == -1 and entry(bias_kind=1) == -1 and entry(bias_kind=3) == -1 and entry(left=3) == -1 and entry(T_=2) == -1
    # the pool's: outside {2, 4}, not dividing n, and a scale that dropout_scale_ok refuses next to a seed
    assert entry(pool=0) == -1 and entry(pool=1) == -1 and entry(pool=3) == -1 and entry(pool=8) == -1 and entry(pool=-4) == -1
    A.n = 50
    assert entry(pool=4) == -1
    A.n = 48
    for bad in (0.5, 0.0, -2.0, float("inf"), float("nan")):
        assert entry(seed=one, scale=bad) == -1, bad
    assert b"scale" in L.tgcn_last_error()
    A.n = 1025
    assert entry() == -4 and entry(pool=3) == -4          # the plan's code comes first


def test_small_series_pool_kernel_uses_no_scratch_and_spills_nothing():
    sys.path.insert(0, os.path.join(os.path.dirname(_lib.__file__), "..", "tools"))
    try:
        from kernel_resources import demangle, kernel_resources
    finally:
        sys.path.pop(0)
    res = kernel_resources(_lib.LIB_PATH)
    names = sorted(res)
    mine = [nm for nm, pretty in zip(names, demangle(names)) if "small_series_pool_kernel" in pretty]
    # the dense and the sparse carve-up x 1 / 2 / 4 column tiles per wave x the two recurrences x pool 2 / 4 x without / with dropout
    assert len(mine) == 48, mine
    for nm in mine:
        r = res[nm]
        print(nm, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (nm, r)
        assert r.get("uses_dynamic_stack") in (None, 0, "false") and r.get("max_flat_workgroup_size") == 1024
