"""CPU test of the launches of cheb_series_relu_pool_chunked / F.cheb_time_windows_relu_pool_chunked (DESIGN.md 3.10 "Time chunks through the
pooled epilogue"), by the recorder technique of tests/test_layer_dispatch.py.  The forward asks tgcn_series_pool_plan once and first, then per
chunk runs K - 1 hops on rows of Tc*f floats and ONE tgcn_cheb_project_series_stream_pool_at_f32 call with the chunk's place in the whole z, a
head that follows (head + Tc) mod C, and a null seed iff p == 0 or not training.  The backward walks the chunks in the same order: ONE
tgcn_relu_pool_bwd_rows_f32 call on rows = min(Tc + C, T - t0) time rows, the hops again, ONE tgcn_cheb_series_chunk_backward_f32 call on the
slab (g_T = rows, g_t0 = 0), the adjoint hops.  The one-sided backwards pass null pointers; every refusal raises TgcnError with nothing
launched and no operand built; the existing pooled calls still reject the keyword."""
import ctypes
import os

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F
from tgcn_amd.graph import GraphOperand

from test_layer_dispatch import N_V, _Op, _op, recorder  # noqa: F401  (the recorder fixture)

PLAN, AT, ROWS, CB, HOP = "series_pool_plan", "cheb_project_series_stream_pool_at", "relu_pool_bwd_rows", "cheb_series_chunk_backward", "csr_hop2"
# positions of the pointer arguments (the stream, position 0, is null in the recorder's world)
A_STACK, A_W, A_BIAS, A_Z, A_IDX, A_RING, A_SEED = 8, 9, 10, 12, 13, 18, 22                  # tgcn_cheb_project_series_stream_pool_at_f32
R_GZ, R_Z, R_IDX, R_GY = 1, 2, 3, 4                                                          # tgcn_relu_pool_bwd_rows_f32
P_STACK, P_RING, P_G, P_W, P_GOUT, P_DW, P_WS = 8, 9, 12, 16, 17, 18, 19                     # tgcn_cheb_series_chunk_backward_f32
SEED = (0x2468ACE << 32) | 0x13579BDF


def _entries(calls):
    return [c.split()[0] for c in calls]


def _stub_operands(monkeypatch):
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda *a, **k: _Op(N_V, 256)))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: _Op(N_V, 256)))


def _no_operands(monkeypatch):
    monkeypatch.setattr(GraphOperand, "from_any", staticmethod(lambda *a, **k: pytest.fail("operand built")))
    monkeypatch.setattr(GraphOperand, "from_edge_index", staticmethod(lambda *a, **k: pytest.fail("operand built")))


def _chunks(T, Tc):
    return [(t0, min(Tc, T - t0)) for t0 in range(0, T, Tc)]


@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
@pytest.mark.parametrize("mode", [0, 1], ids=["power", "chebyshev"])
@pytest.mark.parametrize("p", [0.0, 0.3], ids=["no-mask", "p0.3"])
def test_plan_then_hops_and_one_entry_per_chunk_in_both_directions(p, mode, as_series, recorder):
    rec = recorder({})
    S, T, f, H, N, K, d, Tc, pool = 2, 23, 4, 4, 8, 3, 2, 5, 4
    Cr = (H - 1) * d
    op = _op("plain")
    torch.manual_seed(0)
    series = torch.randn(S, N_V, T, f, requires_grad=True)
    W, bias = torch.randn(K, H, f, N, requires_grad=True), torch.randn(N, requires_grad=True)
    z = F.cheb_time_windows_relu_pool_chunked(op, series, W, bias, F.BIAS_CHANNEL, mode, pool, Tc, p=p, seed=SEED, as_series=as_series, dilation=d)
    assert tuple(z.shape) == ((S, N_V // pool, T, N) if as_series else (S * T, N_V // pool, N)) and z.is_contiguous() and z.requires_grad
    calls, ent = list(rec.calls), _entries(rec.calls)
    # the pooled step-1 plan first and once: H f N vec 1 pool
    assert calls[0] == "%s %d %d %d 1 1 %d" % (PLAN, H, f, N, pool) and ent.count(PLAN) == 1
    assert ent.count("fold_weight") == (1 if mode == 0 else 0) and set(ent) <= {PLAN, "fold_weight", HOP, AT}, ent
    thr, scale = F.dropout_params(p) if p else (0, 1.0)
    per_chunk = [(c, nl) for c, nl in zip(calls, rec.nulls) if c.split()[0] in (HOP, AT)]
    head, i = 0, 0
    for t0, tc in _chunks(T, Tc):
        hops, (at, nulls) = per_chunk[i:i + K - 1], per_chunk[i + K - 1]
        i += K
        assert all(c.split()[:3] == [HOP, str(S), str(tc * f)] for c, _ in hops), (t0, hops)
        # S n Tc f H N K bias_kind pool out_T out_t0 out_as_series ring_ld head dilation thr scale
        assert at == "%s %d %d %d %d %d %d %d 1 %d %d %d %d %d %d %d %d %g" % (AT, S, N_V, tc, f, H, N, K, pool, T, t0, int(as_series), Cr * f, head, d,
                                                                                thr, scale), (t0, at)
        assert (A_SEED in nulls) == (p == 0) and not set(nulls) & {A_STACK, A_W, A_BIAS, A_Z, A_IDX, A_RING}, nulls
        head = (head + tc) % Cr
    assert i == len(per_chunk) and _chunks(T, Tc)[-1] == (20, 3)        # a short tail

    del rec.calls[:], rec.nulls[:]
    z.backward(torch.ones_like(z))
    calls, ent = list(rec.calls), _entries(rec.calls)
    assert set(ent) <= {"fold_weight", HOP, ROWS, CB}, ent
    assert ent.count("fold_weight") == (1 if mode == 0 else 0) and (mode == 1 or ent[-1] == "fold_weight")      # the sum un-folded once, last
    per_chunk = [(c, nl) for c, nl in zip(calls, rec.nulls) if c.split()[0] in (HOP, ROWS, CB)]
    head, i = 0, 0
    for t0, tc in _chunks(T, Tc):
        rows = min(tc + Cr, T - t0)
        (rw, rnulls), rehops, (cb, nulls), adj = per_chunk[i], per_chunk[i + 1:i + K], per_chunk[i + K], per_chunk[i + K + 1:i + 2 * K]
        i += 2 * K
        # S n out_T t0 rows N pool as_series scale
        assert rw == "%s %d %d %d %d %d %d %d %d %g" % (ROWS, S, N_V, T, t0, rows, N, pool, int(as_series), scale), (t0, rw)
        assert not set(rnulls) & {R_GZ, R_Z, R_IDX, R_GY}
        assert all(c.split()[:3] == [HOP, str(S), str(tc * f)] for c, _ in rehops + adj), t0
        # S n Tc f H N K ring_ld head g_T g_t0 g_as_series workspace_bytes dilation: the slab is the whole gradient the entry sees
        assert cb == "%s %d %d %d %d %d %d %d %d %d %d 0 %d 1024 %d" % (CB, S, N_V, tc, f, H, N, K, Cr * f, head, rows, int(as_series), d), (t0, cb)
        assert not set(nulls) & {P_STACK, P_RING, P_G, P_W, P_GOUT, P_DW, P_WS}, nulls
        head = (head + tc) % Cr
    assert i == len(per_chunk)
    assert [min(tc + Cr, T - t0) for t0, tc in _chunks(T, Tc)] == [11, 11, 11, 8, 3]        # the halo, clipped at the recording's end
    assert tuple(series.grad.shape) == (S, N_V, T, f) and tuple(W.grad.shape) == (K, H, f, N) and tuple(bias.grad.shape) == (N,)


def test_both_classes_three_dimensional_series_one_tap_and_the_training_switch(recorder, monkeypatch):
    """the module-level call on both classes: a single channel as a 3-D series runs with f = 1; Tc >= T is one chunk; one tap keeps no ring (a
    null ring, ring_ld 0, head 0, dilation 1); training=False passes a null seed whatever p; no grad mode stores no arg-max"""
    rec = recorder({})
    _stub_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    T = 12
    for H, d in ((3, 2), (1, 5)):
        Cr = (H - 1) * (d if H > 1 else 1)
        for layer, extra in ((tgcn_amd.TGCNCheb_H(torch.eye(N_V), 1, 8, 3, H), ()), (tgcn_amd.ChebTimeConv(1, 8, 3, H), (ei,))):
            for Tc, training in ((T, True), (64, False)):
                del rec.calls[:], rec.nulls[:]
                series = torch.randn(2, N_V, T, requires_grad=True)
                z = tgcn_amd.cheb_series_relu_pool_chunked(layer, series, *extra, time_chunk=Tc, pool=2, p=0.5, training=training, seed=7, dilation=d)
                assert tuple(z.shape) == (2 * T, N_V // 2, 8)
                ent = _entries(rec.calls)
                assert ent[0] == PLAN and ent.count(AT) == 1 and not any(e.startswith("cheb_project_series") and e != AT for e in ent)
                at, nulls = rec.calls[ent.index(AT)].split(), rec.nulls[ent.index(AT)]
                assert at[1:8] == [str(v) for v in (2, N_V, T, 1, H, 8, 3)] and at[9:16] == [str(v) for v in (2, T, 0, 0, Cr, 0, d if H > 1 else 1)]
                assert (A_RING in nulls) == (H == 1) and (A_SEED in nulls) == (not training) and A_IDX not in nulls
                assert at[16:] == (["2147483648", "2"] if training else ["0", "1"])
                del rec.calls[:], rec.nulls[:]
                z.backward(torch.ones_like(z))
                ent = _entries(rec.calls)
                assert ent.count(ROWS) == 1 and ent.count(CB) == 1
                rw, cb = rec.calls[ent.index(ROWS)].split(), rec.calls[ent.index(CB)].split()
                assert rw[1:] == [str(v) for v in (2, N_V, T, 0, T, 8, 2, 0)] + ["2" if training else "1"]
                assert cb[3] == str(T) and cb[8:13] == [str(v) for v in (Cr, 0, T, 0, 0)]
                assert (P_RING in rec.nulls[ent.index(CB)]) == (H == 1)
                assert tuple(series.grad.shape) == (2, N_V, T)
            del rec.calls[:], rec.nulls[:]
            with torch.no_grad():
                tgcn_amd.cheb_series_relu_pool_chunked(layer, torch.randn(2, N_V, T), *extra, time_chunk=5, p=0.5, seed=7, dilation=d)
            at_nulls = [nl for c, nl in zip(rec.calls, rec.nulls) if c.split()[0] == AT]
            assert len(at_nulls) == 3 and all(A_IDX in nl for nl in at_nulls)


def test_the_one_sided_backwards_pass_null_pointers_and_skip_their_hops(recorder):
    rec = recorder({})
    S, T, f, H, N, K, d, Tc, pool = 2, 11, 4, 3, 8, 3, 1, 4, 2
    op = _op("plain")
    nchunks = len(_chunks(T, Tc))
    # a frozen weight: no second hop pass, no ring, no dW -- the slab, G and the adjoint hops only
    series, W = torch.randn(S, N_V, T, f, requires_grad=True), torch.randn(K, H, f, N)
    z = F.cheb_time_windows_relu_pool_chunked(op, series, W, None, F.BIAS_NONE, 1, pool, Tc, as_series=True, dilation=d)
    del rec.calls[:], rec.nulls[:]
    z.backward(torch.ones_like(z))
    ent = _entries(rec.calls)
    assert ent.count(ROWS) == nchunks and ent.count(CB) == nchunks and ent.count(HOP) == nchunks * (K - 1) and set(ent) == {HOP, ROWS, CB}
    for c, nulls in zip(rec.calls, rec.nulls):
        if c.split()[0] == CB:
            assert {P_STACK, P_RING, P_DW} <= set(nulls) and not set(nulls) & {P_G, P_W, P_GOUT, P_WS}
            assert c.split()[8:10] == ["0", "0"]                         # no ring: ring_ld and head unused
    assert ent[:2] == [ROWS, CB]                                         # nothing is hopped before the first chunk's G
    # a series without grad: no G, no adjoint hops -- the slab, the hops again, the ring and dW
    series, W = torch.randn(S, N_V, T, f), torch.randn(K, H, f, N, requires_grad=True)
    z = F.cheb_time_windows_relu_pool_chunked(op, series, W, None, F.BIAS_NONE, 1, pool, Tc, as_series=False, dilation=d)
    del rec.calls[:], rec.nulls[:]
    z.backward(torch.ones_like(z))
    ent = _entries(rec.calls)
    assert ent.count(ROWS) == nchunks and ent.count(CB) == nchunks and ent.count(HOP) == nchunks * (K - 1) and set(ent) == {HOP, ROWS, CB}
    heads = []
    for c, nulls in zip(rec.calls, rec.nulls):
        if c.split()[0] == CB:
            assert {P_W, P_GOUT} <= set(nulls) and not set(nulls) & {P_STACK, P_RING, P_G, P_DW, P_WS}
            heads.append(int(c.split()[9]))
    assert heads == [0, 0, 0] and ent[-1] == CB                          # C = 2, chunks of 4: the head returns to 0; no hop after the last dW
    # only the bias trains: the slabs and nothing else
    series, W, bias = torch.randn(S, N_V, T, f), torch.randn(K, H, f, N), torch.randn(N, requires_grad=True)
    z = F.cheb_time_windows_relu_pool_chunked(op, series, W, bias, F.BIAS_CHANNEL, 1, pool, Tc, as_series=True)
    del rec.calls[:]
    z.backward(torch.ones_like(z))
    assert _entries(rec.calls) == [ROWS] * nchunks and tuple(bias.grad.shape) == (N,)


def test_a_reordered_operand_runs_the_chunked_layer_then_the_pool_pass(recorder):
    rec = recorder({})
    op = _op("reordered")
    assert not F.series_pool_is_fused(op)
    for p, tail in ((0.0, "relu_pool"), (0.5, "relu_dropout_pool")):
        del rec.calls[:]
        series = torch.randn(2, N_V, 9, 4, requires_grad=True)
        z = F.cheb_time_windows_relu_pool_chunked(op, series, torch.randn(3, 3, 4, 8), None, F.BIAS_NONE, 1, 4, 4, p=p, seed=3, as_series=True)
        ent = _entries(rec.calls)
        assert tuple(z.shape) == (2, N_V // 4, 9, 8)
        assert ent.count("cheb_project_series_stream_at") == 3 and ent.count(AT) == 0 and ent[-1] == tail and ent.count("pack_rows") == 2


def test_every_refusal_comes_before_anything_is_built_or_launched(recorder, monkeypatch):
    rec = recorder({})
    _no_operands(monkeypatch)
    ei = torch.tensor([[0, 1], [1, 0]])
    h, c = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3), tgcn_amd.ChebTimeConv(4, 8, 3, 3)
    series = torch.randn(2, N_V, 12, 4)
    op = _op("plain")

    def calls(time_chunk=4, pool=4, **kw):
        return (lambda: tgcn_amd.cheb_series_relu_pool_chunked(h, series, time_chunk=time_chunk, pool=pool, **kw),
                lambda: tgcn_amd.cheb_series_relu_pool_chunked(c, series, ei, time_chunk=time_chunk, pool=pool, **kw),
                lambda: F.cheb_time_windows_relu_pool_chunked(op, series, h.weight, None, F.BIAS_NONE, 0, pool, time_chunk,
                                                              **{k: v for k, v in kw.items() if k != "training"}))

    for bad in (0, -1, 2.0, True, "4", (4,), None):
        for call in calls(time_chunk=bad):
            with pytest.raises(_lib.TgcnError, match="time_chunk is (None or )?an integer >= 1"):
                call()
    for bad in (3, 1, 8, 0, 2.0, True):
        for call in calls(pool=bad):
            with pytest.raises(_lib.TgcnError, match="pool is 2 or 4"):
                call()
    for call in (lambda: tgcn_amd.cheb_series_relu_pool_chunked(tgcn_amd.TGCNCheb_H(torch.eye(6), 4, 8, 3, 3), torch.randn(2, 6, 12, 4), time_chunk=4),
                 lambda: F.cheb_time_windows_relu_pool_chunked(op, torch.randn(2, 6, 12, 4), h.weight, None, F.BIAS_NONE, 0, 4, 4)):
        with pytest.raises(_lib.TgcnError, match="not a multiple of pool"):
            call()
    for bad in (-0.1, 1, 1.5, float("nan"), None, "0.5", True):
        for call in calls(p=bad):
            with pytest.raises(_lib.TgcnError, match=r"p is a real number in \[0, 1\)"):
                call()
    for bad in (-1, 2 ** 62, 1.5, "7", True):
        for call in calls(p=0.5, seed=bad):
            with pytest.raises(_lib.TgcnError, match="seed is None, an integer"):
                call()
    for call in calls(p=0.5, seed=torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(_lib.TgcnError, match="one int64 element"):
            call()
    BF = torch.bfloat16
    hb, cb = tgcn_amd.TGCNCheb_H(torch.eye(N_V), 4, 8, 3, 3).to(BF), tgcn_amd.ChebTimeConv(4, 8, 3, 3).to(BF)
    for call in (lambda: tgcn_amd.cheb_series_relu_pool_chunked(hb, series.to(BF), time_chunk=4),
                 lambda: tgcn_amd.cheb_series_relu_pool_chunked(cb, series.to(BF), ei, time_chunk=4),
                 lambda: F.cheb_time_windows_relu_pool_chunked(op, series.to(BF), hb.weight, None, F.BIAS_NONE, 0, 4, 4)):
        with pytest.raises(_lib.TgcnError, match="bfloat16 parameters are not supported"):
            call()
    with pytest.raises(_lib.TgcnError, match="learnable edge weights"):
        tgcn_amd.cheb_series_relu_pool_chunked(c, series, ei, torch.ones(2, requires_grad=True), time_chunk=4)
    with pytest.raises(_lib.TgcnError, match="dilation is an integer >= 1"):
        tgcn_amd.cheb_series_relu_pool_chunked(h, series, time_chunk=4, dilation=0)
    with pytest.raises(_lib.TgcnError, match="the layer is a TGCNCheb_H or a ChebTimeConv"):
        tgcn_amd.cheb_series_relu_pool_chunked(tgcn_amd.GCNCheb(torch.eye(N_V), 4, 8, 3), series, time_chunk=4)
    # the geometry is the causal layer at step 1: no stride and no padding keyword; time_chunk is required
    for kw in (dict(stride=2), dict(padding="causal"), dict()):
        with pytest.raises(TypeError):
            tgcn_amd.cheb_series_relu_pool_chunked(h, series, **dict(dict(time_chunk=4) if kw else {}, **kw))
    # and the existing pooled calls keep their signatures
    for fn in (tgcn_amd.cheb_series_relu_pool, tgcn_amd.cheb_series_relu_dropout_pool):
        with pytest.raises(TypeError):
            fn(h, series, padding="causal", time_chunk=4)
    assert rec.calls == []


def test_the_new_entries_are_declared_everywhere():
    """the header, the ctypes table and the library agree on the two entries; ABI 8; the scalar rules refuse before any pointer is read"""
    names = ["tgcn_cheb_project_series_stream_pool_at_f32", "tgcn_relu_pool_bwd_rows_f32"]
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "tgcn_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert nm in _lib.SIGNATURES and hasattr(handle, nm) and (" " + nm + "(") in header, nm
    assert hasattr(tgcn_amd, "cheb_series_relu_pool_chunked") and hasattr(F, "cheb_time_windows_relu_pool_chunked")
    assert hasattr(F, "ChebSeriesChunkReluPoolFn")
    L = _lib.lib()
    assert L.tgcn_abi_version() == 8 == _lib.ABI_VERSION
    INVALID, UNSUPPORTED = -1, -4
    one = ctypes.c_void_p(16)       # a non-null pointer that the refused calls never read

    # S n Tc f H N K = 2 48 5 4 3 8 3, dilation 4: C = 8, ring_ld >= 32
    def at(n=48, Tc=5, f=4, H=3, pool=4, out_T=23, out_t0=0, ring=one, ring_ld=32, head=0, dil=4, seed=one, scale=2.0, z=one, stack=one, W=one):
        return L.tgcn_cheb_project_series_stream_pool_at_f32(None, 2, n, Tc, f, H, 8, 3, stack, W, None, 0, z, one, pool, out_T, out_t0, 1, ring, ring_ld,
                                                             head, dil, seed, 1 << 31, scale)

    assert at(head=8) == INVALID and at(head=-1) == INVALID and at(ring_ld=31) == INVALID and at(ring=None) == INVALID
    assert at(Tc=0) == INVALID and at(dil=0) == INVALID and at(dil=2 ** 30) == INVALID and at(H=0) == INVALID
    assert at(out_t0=19) == INVALID and at(out_t0=-1) == INVALID and at(out_T=0) == INVALID and at(out_T=4) == INVALID
    assert at(pool=3) == INVALID and at(pool=0) == INVALID and at(pool=8) == INVALID and at(n=50) == INVALID       # 50 % 4 != 0
    assert at(scale=0.5) == INVALID and at(scale=float("inf")) == INVALID and at(scale=float("nan")) == INVALID
    assert at(z=None) == INVALID and at(stack=None) == INVALID and at(W=None) == INVALID
    assert at(f=40000, ring_ld=320000) == UNSUPPORTED                                  # the plan refuses: the span does not fit the LDS
    assert at(seed=None, f=40000, ring_ld=320000) == UNSUPPORTED and at(seed=None, head=8) == INVALID and at(seed=None, pool=3) == INVALID

    def rows(S=2, n=48, out_T=23, t0=3, nrows=7, N=8, pool=4, scale=1.0, gz=one, z=one, idx=one, gy=one):
        return L.tgcn_relu_pool_bwd_rows_f32(None, gz, z, idx, gy, S, n, out_T, t0, nrows, N, pool, 1, scale)

    assert rows(S=0) == INVALID and rows(n=0) == INVALID and rows(N=0) == INVALID and rows(out_T=0) == INVALID
    assert rows(t0=-1) == INVALID and rows(nrows=0) == INVALID and rows(t0=17) == INVALID and rows(t0=23, nrows=1) == INVALID
    assert rows(pool=0) == INVALID and rows(pool=5) == INVALID and rows(pool=256, n=512) == INVALID
    assert rows(scale=float("nan")) == INVALID and rows(scale=float("inf")) == INVALID
    assert rows(gz=None) == INVALID and rows(z=None) == INVALID and rows(idx=None) == INVALID and rows(gy=None) == INVALID
