"""forward_series / F.cheb_time_windows with time_chunk=: the causal layer walked Tc time rows at a time through the streaming ring in both
directions (DESIGN.md 3.10 "Time chunks").  Output and all three gradients against the fp64 oracle on the materialised causal dilated windows
of the WHOLE series (the helpers and the project's bounds of tests/test_series_dilation.py: output 1e-5, gradients 2e-5 of the tensor's
maximum) and against the unchunked call at the same arguments, in both layouts; the two C entries against the entries they are built from,
bit for bit where the sums are the same sums; the one-sided backwards, two identical runs, a two-layer chain, and the capability itself:
the peak memory of a training step, which no longer holds anything of the hop stack's size."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cheb_oracle as O
from test_hip_parity import _random_graph
from test_series_channels import TOL, TOL_GRAD, _dev, _to_series
import test_series_dilation as D

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]

S_REC, T_ROWS, K_TERMS = 2, 23, D.K_TERMS
GRAPHS = {"dense37": (37, 12), "sparse50": (50, 2)}        # vertices, average degree: partial tiles of 32 windows x vertices either way
GEOMS = [(4, 2), (3, 1), (1, 1)]                           # (H, dilation): C = 6, 2 and no ring at all


def chunk_lengths(H, d):
    """below, at and above the ring length (the ring wraps), a short tail (16 of 23) and one chunk (64 >= T)"""
    Cr = (H - 1) * d
    return sorted({tc for tc in (1, Cr, Cr + 1, 16, 64) if tc >= 1})


class Setup(D.Setup):
    """test_series_dilation.Setup on a graph of this file (its W64 and call are inherited)"""

    def __init__(self, cls, graph, f, g, H, seed):
        import tgcn_amd
        from tgcn_amd import functional as F
        n, deg = GRAPHS[graph]
        K = K_TERMS
        rng = np.random.default_rng(seed)
        row, col, val = _random_graph(n, deg, rng)
        val = val * 0.4
        torch.manual_seed(seed)
        self.cls, self.F, self.n = cls, F, n
        if cls == "TGCNCheb_H":
            self.L = O.coo_to_csr(row, col, val, n)
            self.op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val))
            self.layer = layer = tgcn_amd.TGCNCheb_H(self.op, f, g, K, H).cuda()
            self.mode, self.fmode, self.bias_kind = "power", F.MODE_POWER, F.BIAS_VERTEX_CHANNEL
            self.module = lambda s, **kw: layer.forward_series(s, **kw)
            self.forward64 = lambda xw, b: O.tgcn_cheb_h_forward(self.L, xw, self.W64(), b)
            self.bias_grad = lambda go: go.astype(np.float64).sum(axis=0, keepdims=True)
        else:
            ei = np.stack([row, col]).astype(np.int64)
            r, c, lap = O.edge_laplacian(ei, None, n)
            self.L = O.coo_to_csr(r, c, lap, n)
            self.layer = layer = tgcn_amd.ChebTimeConv(f, g, K, H).cuda()
            self.mode, self.fmode, self.bias_kind = "chebyshev", F.MODE_CHEBYSHEV, F.BIAS_CHANNEL
            eid = _dev(ei)
            self.op = layer._operand(torch.empty(1, n, 1, device="cuda"), eid, None)
            self.module = lambda s, **kw: layer.forward_series(s, eid, None, **kw)
            self.forward64 = lambda xw, b: O.cheb_time_conv_forward(xw, ei, None, self.W64(), b)
            self.bias_grad = lambda go: go.astype(np.float64).sum(axis=(0, 1))
        with torch.no_grad():
            layer.bias.uniform_(-0.5, 0.5)
        self.reordered = None


def _reference(su, S, T, H, f, g, d, rng):
    """series, output gradient (window-major) and the fp64 references of the causal layer on the whole series, computed once"""
    left = (H - 1) * d
    series = rng.standard_normal((S, su.n, T, f)).astype(np.float32)
    xw = D.windows_dilated(series, H, d, left, 0).astype(np.float64)
    assert xw.shape[0] == S * T                                  # causal: a window for every time row
    ref_b, ref_0 = su.forward64(xw, su.layer.bias.detach().cpu().numpy()), su.forward64(xw, None)
    go = rng.standard_normal((S * T, su.n, g)).astype(np.float32)
    gxw, gW = O.layer_backward(su.L, xw, su.W64(), go, su.mode)
    return series, go, ref_b, ref_0, D.fold_dilated(gxw, S, T, d, left, 0), gW, su.bias_grad(go)


def _errs(res, base, ref, gs, gW, gb, bias):
    """errors of one run (out, ds, dW, db) against the oracle and, under the same bounds, against the unchunked run `base`"""
    out, ds, dW, db = res
    e = dict(out=rel_err(out.cpu().numpy(), ref), ds=rel_err(ds, gs), dW=rel_err(dW, gW),
             out_u=rel_err(out.cpu().numpy(), base[0].cpu().numpy()), ds_u=rel_err(ds, base[1]), dW_u=rel_err(dW, base[2]))
    if bias:
        e.update(db=rel_err(db.reshape(gb.shape), gb), db_u=rel_err(db, base[3]))
    else:
        assert db is None
    return e


def _check(cls, graph, H, d, f, g, S=S_REC, T=T_ROWS, chunks=None, kinds=(None, "degree"), biases=(True, False), seed=None):
    su = Setup(cls, graph, f, g, H, seed=H + 7 * d + f if seed is None else seed)
    n = su.n
    series, go, ref_b, ref_0, gs, gW, gb = _reference(su, S, T, H, f, g, d, np.random.default_rng([T, H, d, f, g]))
    go_s = np.ascontiguousarray(_to_series(go, S, T))
    geo = dict(padding="causal", dilation=d)
    for kind in kinds:
        for bias in biases:
            ref = ref_b if bias else ref_0
            base = {lay: D._run(su, series, go_s if lay else go, kind, bias, lay, geo) for lay in (False, True)}
            for tc in (chunk_lengths(H, d) if chunks is None else chunks):
                res = {lay: D._run(su, series, go_s if lay else go, kind, bias, lay, dict(geo, time_chunk=tc)) for lay in (False, True)}
                assert tuple(res[False][0].shape) == (S * T, n, g) and tuple(res[True][0].shape) == (S, n, T, g) and res[True][0].is_contiguous()
                # the two layouts hold the same numbers: the kernel only addresses its output differently
                assert torch.equal(res[True][0], res[False][0].view(S, T, n, g).permute(0, 2, 1, 3)), (kind, bias, tc)
                for lay in (False, True):
                    e = _errs(res[lay], base[lay], _to_series(ref, S, T) if lay else ref, gs, gW, gb, bias)
                    print(cls, graph, (H, d, f, g), kind, "bias" if bias else "no bias", "Tc", tc, "series" if lay else "windows", e)
                    assert max(e.pop("out"), e.pop("out_u")) <= TOL, (kind, bias, tc, lay)
                    assert max(e.values()) <= TOL_GRAD, (kind, bias, tc, lay, e)
    return su


@gpu
@pytest.mark.parametrize("cls", D.CLASSES)
@pytest.mark.parametrize("graph", sorted(GRAPHS))
@pytest.mark.parametrize("g", [5, 40])
@pytest.mark.parametrize("f", [4, 3, 1], ids=["f4", "f3", "single-channel"])
@pytest.mark.parametrize("H,d", GEOMS, ids=["H4_d2", "H3_d1", "H1"])
def test_time_chunks_vs_oracle_and_the_unchunked_call(H, d, f, g, graph, cls, gpu_device):
    """bias and none, plain and degree-reordered operand, both layouts, every chunk length of chunk_lengths; f = 1 is given as a 3-D series"""
    assert chunk_lengths(4, 2) == [1, 6, 7, 16, 64] and chunk_lengths(3, 1) == [1, 2, 3, 16, 64] and chunk_lengths(1, 1) == [1, 16, 64]
    _check(cls, graph, H, d, f, g)


@gpu
@pytest.mark.parametrize("cls", D.CLASSES)
def test_time_chunks_with_a_chunked_span(cls, gpu_device):
    """the shape of test_dilated_series_with_a_chunked_span: the step-1 plan stages HC < H weight time rows at a time, in the forward and
    in the GEMM over g (one recording, to keep the oracle's windows small); chunks below and above C = 54"""
    T, H, d, f, g, left, right = D.CHUNKED[0]
    rc, hc, lds = D.conv_plan(H, f, g)
    assert rc == 0 and hc < H
    _check(cls, "sparse50", H, d, f, g, S=1, T=T, chunks=(16, 60), kinds=(None,), biases=(True,))


# ---------------------------------------------------------------------------------------------------------------- one-sided, repeatable
ONE = (4, 2, 4, 40)        # H, d, f, g


@functools.lru_cache(maxsize=None)
def _one(cls):
    H, d, f, g = ONE
    su = Setup(cls, "sparse50", f, g, H, seed=5)
    return (su,) + _reference(su, S_REC, T_ROWS, H, f, g, d, np.random.default_rng(11))


@gpu
@pytest.mark.parametrize("cls", D.CLASSES)
def test_backward_without_the_series_gradient(cls, gpu_device):
    su, series, go, ref_b, ref_0, gs, gW, gb = _one(cls)
    out, ds, dW, db = D._run(su, series, go, None, True, False, dict(padding="causal", dilation=ONE[1], time_chunk=7), need_series=False)
    assert ds is None
    errs = dict(out=rel_err(out.cpu().numpy(), ref_b), dW=rel_err(dW, gW), db=rel_err(db.reshape(gb.shape), gb))
    print(errs)
    assert errs["out"] <= TOL and max(errs["dW"], errs["db"]) <= TOL_GRAD, errs


@gpu
@pytest.mark.parametrize("cls", D.CLASSES)
def test_backward_with_frozen_parameters(cls, gpu_device):
    su, series, go, ref_b, ref_0, gs, gW, gb = _one(cls)
    su.layer.requires_grad_(False)
    try:
        out, ds, dW, db = D._run(su, series, np.ascontiguousarray(_to_series(go, S_REC, T_ROWS)), None, True, True,
                                 dict(padding="causal", dilation=ONE[1], time_chunk=7))
    finally:
        su.layer.requires_grad_(True)
    assert dW is None and db is None
    e = rel_err(ds, gs)
    print(e)
    assert e <= TOL_GRAD, e


@gpu
@pytest.mark.parametrize("cls", D.CLASSES)
def test_two_identical_runs_are_bit_identical(cls, gpu_device):
    su, series, go = _one(cls)[:3]
    runs = [D._run(su, series, go, None, True, False, dict(padding="causal", dilation=ONE[1], time_chunk=6)) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert a is not None and np.array_equal(a, b)


@gpu
@pytest.mark.parametrize("cls", D.CLASSES)
def test_a_two_layer_causal_chain_trains_through_both_layers(cls, gpu_device):
    """dilations 1 and 2 with a relu between, time_chunk on both layers: every gradient matches the unchunked chain within the bounds"""
    H, f, g1, g2 = 3, 4, 8, 5
    l1, l2 = Setup(cls, "sparse50", f, g1, H, seed=21), Setup(cls, "sparse50", g1, g2, H, seed=21)        # the same graph (same seed)
    gen = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randn(S_REC, l1.n, T_ROWS, f, device="cuda", generator=gen)
    go = torch.randn(S_REC, l1.n, T_ROWS, g2, device="cuda", generator=gen)
    res = []
    for kw in (dict(), dict(time_chunk=5)):
        l1.layer.zero_grad(), l2.layer.zero_grad()
        xs = x.clone().requires_grad_(True)
        h = torch.relu(l1.module(xs, as_series=True, padding="causal", dilation=1, **kw))
        out = l2.module(h, as_series=True, padding="causal", dilation=2, **({"time_chunk": 4} if kw else {}))
        out.backward(go)
        res.append([out.detach().cpu().numpy(), xs.grad.cpu().numpy()] + [p.grad.cpu().numpy().copy() for lay in (l1, l2)
                                                                          for p in (lay.layer.weight, lay.layer.bias)])
    errs = [rel_err(a, b) for a, b in zip(res[1], res[0])]
    print(errs)
    assert errs[0] <= TOL and max(errs[1:]) <= TOL_GRAD, errs


# ---------------------------------------------------------------------------------------------------------------- the C ABI directly
@gpu
@pytest.mark.parametrize("f", [4, 3], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("H,d", [(4, 2), (3, 1)], ids=["H4_d2", "H3_d1"])
def test_the_at_entry_is_the_stream_entry_in_place(H, d, f, gpu_device):
    """on one stack and ring: its rows torch.equal to tgcn_cheb_project_series_stream_f32's in both layouts, the other rows untouched, and
    the same ring afterwards; one tap (a null ring) against the _conv entry"""
    from tgcn_amd import _lib
    L = _lib.lib()
    n, S, Tc, N, K, T, t0 = 37, 2, 7, 24, 3, 23, 11
    Cr = (H - 1) * d
    gen = torch.Generator(device="cuda").manual_seed(H * 10 + f)
    stack = torch.randn((K, S, n, Tc * f), device="cuda", generator=gen)
    W, bias = torch.randn((K, H * f, N), device="cuda", generator=gen), torch.randn((N,), device="cuda", generator=gen)
    ring0, head = torch.randn((K, S, n, Cr * f), device="cuda", generator=gen), Cr - 1
    args = (_lib.stream_ptr(), S, n, Tc, f, H, N, K, _lib.ptr(stack), _lib.ptr(W), _lib.ptr(bias), 1)
    ref, ring_ref = torch.full((S, n, Tc, N), float("nan"), device="cuda"), ring0.clone()
    _lib.check(L.tgcn_cheb_project_series_stream_f32(*args, _lib.ptr(ref), _lib.ptr(ring_ref), Cr * f, head, d))
    assert not torch.isnan(ref).any() and not torch.equal(ring_ref, ring0)
    for as_series in (1, 0):
        out, ring = torch.full((S, n, T, N) if as_series else (S * T, n, N), float("nan"), device="cuda"), ring0.clone()
        _lib.check(L.tgcn_cheb_project_series_stream_at_f32(*args, _lib.ptr(out), T, t0, as_series, _lib.ptr(ring), Cr * f, head, d))
        rows = out if as_series else out.view(S, T, n, N).permute(0, 2, 1, 3)
        assert torch.equal(rows[:, :, t0:t0 + Tc], ref), as_series
        assert torch.isnan(rows[:, :, :t0]).all() and torch.isnan(rows[:, :, t0 + Tc:]).all()
        assert torch.equal(ring, ring_ref)
    # one tap: no ring, the _conv entry's rows
    W1 = torch.randn((K, f, N), device="cuda", generator=gen)
    ref = torch.full((S, n, Tc, N), float("nan"), device="cuda")
    _lib.check(L.tgcn_cheb_project_series_conv_f32(_lib.stream_ptr(), S, n, Tc, f, 1, N, K, _lib.ptr(stack), _lib.ptr(W1), _lib.ptr(bias), 1, 1,
                                                   _lib.ptr(ref), 1, 0, 0))
    out = torch.full((S * T, n, N), float("nan"), device="cuda")
    _lib.check(L.tgcn_cheb_project_series_stream_at_f32(_lib.stream_ptr(), S, n, Tc, f, 1, N, K, _lib.ptr(stack), _lib.ptr(W1), _lib.ptr(bias), 1,
                                                        _lib.ptr(out), T, t0, 0, None, 0, 0, 1))
    assert torch.equal(out.view(S, T, n, N).permute(0, 2, 1, 3)[:, :, t0:t0 + Tc], ref) and torch.isnan(out.view(S, T, n, N)[:, :t0]).all()


@gpu
@pytest.mark.parametrize("as_series", [0, 1], ids=["window-major", "series"])
@pytest.mark.parametrize("f,N", [(4, 24), (3, 5)], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("H,d", [(4, 2), (3, 1), (1, 1)], ids=["H4_d2", "H3_d1", "H1"])
def test_the_chunk_entry_against_the_whole_series_backward(H, d, f, N, as_series, gpu_device):
    """G of every chunk torch.equal to its rows of tgcn_cheb_series_dilated_backward_f32's G on the whole g (the same GEMM over the same rows
    of g); dW summed over the chunks within 2e-5 of the whole-series dW (other partial sums); the ring the entry leaves is the stream
    entry's.  Chunk lists below, at and above the ring length."""
    from tgcn_amd import _lib
    L = _lib.lib()
    n, S, K, T = 37, 2, 3, 23
    Cr = (H - 1) * d
    gen = torch.Generator(device="cuda").manual_seed(H * 100 + f + as_series)
    stack = torch.randn((K, S, n, T, f), device="cuda", generator=gen)
    W = torch.randn((K, H * f, N), device="cuda", generator=gen)
    g = torch.randn((S, n, T, N) if as_series else (S * T, n, N), device="cuda", generator=gen)
    head = (_lib.stream_ptr(), S, n, T, f, H, N, K)
    need = L.tgcn_cheb_series_dilated_backward_workspace_bytes(*head[1:], 1, Cr, 0, d)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    G_ref, dW_ref = torch.full((K, S, n, T, f), float("nan"), device="cuda"), torch.full((K, H * f, N), float("nan"), device="cuda")
    _lib.check(L.tgcn_cheb_series_dilated_backward_f32(*head, _lib.ptr(stack), _lib.ptr(g), as_series, _lib.ptr(W), _lib.ptr(G_ref), _lib.ptr(dW_ref),
                                                       _lib.ptr(ws), need, 1, Cr, 0, d))
    assert not torch.isnan(G_ref).any() and not torch.isnan(dW_ref).any()
    for lens in ([1] * T, [Cr + 1] * (T // (Cr + 1)) + ([T % (Cr + 1)] if T % (Cr + 1) else []), [7, 16], [16, 7], [T]):
        assert sum(lens) == T
        ring = torch.zeros((K, S, n, Cr * f), device="cuda") if Cr else None
        hd, t0, dW = 0, 0, None
        for tc in lens:
            st = stack[:, :, :, t0:t0 + tc].contiguous().view(K, S, n, tc * f)
            G = torch.full((K, S, n, tc, f), float("nan"), device="cuda")
            dWc = torch.full((K, H * f, N), float("nan"), device="cuda")
            need = L.tgcn_cheb_series_chunk_backward_workspace_bytes(S, n, tc, f, H, N, K, d)
            assert need > 0
            wsc = torch.empty(need, dtype=torch.uint8, device="cuda")
            _lib.check(L.tgcn_cheb_series_chunk_backward_f32(_lib.stream_ptr(), S, n, tc, f, H, N, K, _lib.ptr(st), _lib.ptr(ring), Cr * f, hd,
                                                             _lib.ptr(g), T, t0, as_series, _lib.ptr(W), _lib.ptr(G), _lib.ptr(dWc), _lib.ptr(wsc),
                                                             need, d))
            assert torch.equal(G, G_ref[:, :, :, t0:t0 + tc]), (lens, t0)
            assert not torch.isnan(dWc).any()
            dW = dWc if dW is None else dW + dWc
            t0 += tc
            if Cr:
                hd = (hd + tc) % Cr
                # the ring holds the last C rows seen, slot j the row whose index is j (mod C)
                for j in range(max(0, t0 - Cr), t0):
                    assert torch.equal(ring[..., (j % Cr) * f:(j % Cr + 1) * f], stack[:, :, :, j]), (lens, t0, j)
        e = rel_err(dW.cpu().numpy(), dW_ref.cpu().numpy())
        print((H, d, f, N, as_series), lens, "dW", e)
        assert e <= TOL_GRAD, (lens, e)
    # the one-sided forms: G alone needs neither stack nor ring
    G = torch.full((K, S, n, 5, f), float("nan"), device="cuda")
    need = L.tgcn_cheb_series_chunk_backward_workspace_bytes(S, n, 5, f, H, N, K, d)
    wsc = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(L.tgcn_cheb_series_chunk_backward_f32(_lib.stream_ptr(), S, n, 5, f, H, N, K, None, None, 0, 0, _lib.ptr(g), T, 9, as_series,
                                                     _lib.ptr(W), _lib.ptr(G), None, _lib.ptr(wsc), need, d))
    assert torch.equal(G, G_ref[:, :, :, 9:14])


@gpu
def test_refused_calls_launch_nothing(gpu_device):
    """an error code through the C ABI, the outputs untouched"""
    from tgcn_amd import _lib
    L = _lib.lib()
    n, S, T, Tc, f, H, N, K, d = 11, 1, 30, 6, 4, 3, 8, 2, 2
    stack, W = torch.zeros(K, S, n, Tc * f, device="cuda"), torch.zeros(K, H * f, N, device="cuda")
    ring, g = torch.zeros(K, S, n, 4 * f, device="cuda"), torch.zeros(S, n, T, N, device="cuda")
    out = torch.full((S, n, T, N), float("nan"), device="cuda")
    G, dW = torch.full((K, S, n, Tc * f), float("nan"), device="cuda"), torch.full((K, H * f, N), float("nan"), device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    at = lambda out_t0, head: L.tgcn_cheb_project_series_stream_at_f32(_lib.stream_ptr(), S, n, Tc, f, H, N, K, _lib.ptr(stack), _lib.ptr(W), None, 0,
                                                                       _lib.ptr(out), T, out_t0, 1, _lib.ptr(ring), 4 * f, head, d)
    cb = lambda g_t0, head, nbytes: L.tgcn_cheb_series_chunk_backward_f32(_lib.stream_ptr(), S, n, Tc, f, H, N, K, _lib.ptr(stack), _lib.ptr(ring),
                                                                          4 * f, head, _lib.ptr(g), T, g_t0, 1, _lib.ptr(W), _lib.ptr(G),
                                                                          _lib.ptr(dW), _lib.ptr(ws), nbytes, d)
    assert at(25, 0) == -1 and at(0, 4) == -1                            # TGCN_ERR_INVALID: the chunk leaves the output; head outside [0, C)
    assert cb(25, 0, ws.numel()) == -1 and cb(0, 4, ws.numel()) == -1
    assert cb(0, 0, 16) == -3                                            # TGCN_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(G).all() and torch.isnan(dW).all() and not ring.any()


# ---------------------------------------------------------------------------------------------------------------- the capability: peak memory
@gpu
def test_a_chunked_training_step_holds_less_than_half_the_memory(gpu_device):
    """n = 4096 (sparse), S = 1, T = 512, f = N = 4, K = 8, H = 3, d = 1, forward + backward with all three gradients.  With X the bytes of
    the series, the unchunked step holds at least the hop stack and G, 2 K X = 16 X.  The chunked step (time_chunk = 32) holds the series'
    gradient, the output and its gradient -- 3 X at f = N above a baseline that already counts the series -- two chunk tensors of
    K X / 16 = X / 2 each, a ring of K X 2 / 512 and chunk-sized workspaces of the hops: 4 to 5 X, so well below half of 16 X + 3 X.  The
    condition is derived, not measured."""
    import tgcn_amd
    n, S, T, f, N, K, H = 4096, 1, 512, 4, 4, 8, 3
    rng = np.random.default_rng(0)
    row, col, val = _random_graph(n, 4, rng)
    op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val * 0.2))
    layer = tgcn_amd.TGCNCheb_H(op, f, N, K, H).cuda()
    x = torch.randn(S, n, T, f, device="cuda", requires_grad=True)

    def step(**kw):
        layer.zero_grad(set_to_none=True)
        x.grad = None
        out = layer.forward_series(x, as_series=True, padding="causal", **kw)
        out.backward(torch.ones_like(out))
        assert x.grad is not None and layer.weight.grad is not None and layer.bias.grad is not None
        del out

    peaks = {}
    for name, kw in (("whole", dict()), ("chunked", dict(time_chunk=32))):
        step(**kw)                                                       # warm-up: the operand's schedules and transpose are built and cached
        layer.zero_grad(set_to_none=True)
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(**kw)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
    X = x.numel() * 4
    print({k: v / X for k, v in peaks.items()}, "in units of the series' bytes")
    assert peaks["whole"] >= 16 * X
    assert peaks["chunked"] < peaks["whole"] / 2, peaks
