"""The one-launch streaming step (forward_stream / F.cheb_time_stream with fused=True, tgcn_cheb_stream_small_f32): hops, projection and ring
update of a chunk out of LDS, one workgroup per recording.  The outputs of the chunks, concatenated along time, are compared with the fp64
oracle on the materialised causal dilated windows of the WHOLE series under the bound of tests/test_series_stream.py, TOL = 1e-5 of the
tensor's maximum (the general path measures <= 1.4e-6 under it; the fused kernel makes the same kind of sums) -- the chunk lists of that
file on the 48-vertex graph (the sparse carve-up, more than one sub-chunk for the chunk of 70), both classes, f in {4, 3, one channel as a
3-D chunk}, g in {5, 40}, a plain and a degree-reordered operand, with and without a bias.  Then what that graph cannot show: partial
16-row tiles (a dense operand of 37 vertices, a sparse one of 50), K in {1, 2, 5} in both recurrences, fused and unfused calls alternating
on one state, reset(), host-head against capturable twins, a two-layer fused chain through GraphedStream, and the C ABI directly against
the existing pipeline (hop stack + tgcn_cheb_project_series_stream_f32) in output and ring, with the refusals launching nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cheb_oracle as O
from test_hip_parity import _random_graph
from test_series_channels import TOL, _dev
from test_series_dilation import CLASSES, K_TERMS, N_VERT, S_REC, Setup
from test_series_stream import SPARSE_RING, UNDILATED, WRAP, Streamer, causal_reference

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]


def plan_of(op, mode, f, H, N, K, Tc, d):
    """tgcn_cheb_stream_small_plan on the operand -> (rc, tb, dense, lds_bytes)"""
    from tgcn_amd import _lib
    tb, dense, lds = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = _lib.lib().tgcn_cheb_stream_small_plan(op.n, op.nnz, mode, f, H, N, K, Tc, d, C.byref(tb), C.byref(dense), C.byref(lds))
    return rc, tb.value, dense.value, lds.value


class FusedStreamer(Streamer):
    """Streamer with the keyword: `fused` is one value for every chunk, or a tuple that the chunks walk round"""

    def __init__(self, su, seed, fused=True, capturable=False):
        if getattr(su, "edge_index", None) is None:
            super().__init__(su, seed)
        else:               # an operand of this file: the layer's own edge list
            self.su, self.extra = su, (() if su.cls == "TGCNCheb_H" else (su.edge_index, None))
        self.fused, self.capturable, self.calls = fused, capturable, 0

    def step(self, chunk, state, kind, bias, d):
        su = self.su
        fused = self.fused[self.calls % len(self.fused)] if isinstance(self.fused, tuple) else self.fused
        self.calls += 1
        if kind is None and bias:
            return su.layer.forward_stream(chunk, *self.extra, state=state, dilation=d, capturable=self.capturable, fused=fused)
        op = su.op
        if kind is not None:
            if su.reordered is None:
                su.reordered = su.op.reordered(kind)
            op = su.reordered
        W = su.layer.weight if chunk.dim() == 4 else su.layer.weight.reshape(su.layer.weight.shape[0], su.layer.weight.shape[1], -1)
        return su.F.cheb_time_stream(op, chunk, W, su.layer.bias.reshape(-1) if bias else None, su.bias_kind if bias else su.F.BIAS_NONE,
                                     su.fmode, state, d, capturable=self.capturable, fused=fused)


def _check_fused(cls, H, d, chunks, f, g, three_d=False):
    T = sum(chunks)
    seed = T + 7 * d + f
    su = Setup(cls, f, g, H, seed=seed)
    st = FusedStreamer(su, seed)
    # the 48-vertex graph takes the sparse carve-up, and the longest chunk more than one sub-chunk
    rc, tb, dense, lds = plan_of(su.op, su.fmode, f, H, g, K_TERMS, max(chunks), d)
    assert rc == 0 and dense == 0 and 0 < lds <= 160 * 1024, (rc, tb, dense, lds)
    if max(chunks) == 70:
        assert tb < 70, tb
    series = np.random.default_rng([T, d, f, g]).standard_normal((S_REC, N_VERT, T, f)).astype(np.float32)
    dev = _dev(series[..., 0] if three_d else series)
    refs = {bias: causal_reference(su, series, H, d, bias) for bias in (True, False)}
    for kind in (None, "degree"):
        for bias in (True, False):
            out, state = st.feed(dev, chunks, kind, bias, d)
            e = rel_err(out.cpu().numpy(), refs[bias])
            print(cls, (H, d, chunks, f, g), kind, "bias" if bias else "no bias", "tb %d" % tb, "%.2e" % e)
            assert e <= TOL, (kind, bias, e)


def _id(c):
    return "H%d_d%d" % c[:2]


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("g", [5, 40])
@pytest.mark.parametrize("f", [4, 3, "3d"])
@pytest.mark.parametrize("case", [WRAP, UNDILATED, SPARSE_RING], ids=_id)
def test_fused_chunked_stream_vs_oracle(case, f, g, cls, gpu_device):
    H, d, chunks = case
    if f == "3d":
        _check_fused(cls, H, d, chunks, 1, g, three_d=True)
    else:
        _check_fused(cls, H, d, chunks, f, g)


# ------------------------------------------------------------------------------------------- operands of this file: partial 16-row tiles
class SmallSetup:
    """Setup's interface (layer, operand, fp64 reference) on a graph of this file: "dense37" stores three quarters of its off-diagonal
    entries (37 vertices: the last 16-row tile holds 5), "sparse50" about six per row (50 vertices: the last tile holds 2); K terms"""

    def __init__(self, cls, graph, f, g, K, H, seed):
        import tgcn_amd
        from tgcn_amd import functional as F
        rng = np.random.default_rng(seed)
        if graph == "dense37":
            n = 37
            pairs = np.array([(i, j) for i in range(n) for j in range(n) if i != j])
            pairs = pairs[rng.permutation(len(pairs))[:len(pairs) * 3 // 4]]
            row, col = pairs[:, 0].copy(), pairs[:, 1].copy()
            val = (rng.standard_normal(row.shape[0]) / np.sqrt(n)).astype(np.float32)
        else:
            n = 50
            row, col, val = _random_graph(n, 6, rng)
        val = val * 0.4
        torch.manual_seed(seed)
        self.cls, self.F, self.n, self.K, self.reordered = cls, F, n, K, None
        if cls == "TGCNCheb_H":
            self.L = O.coo_to_csr(row, col, val, n)
            self.op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val))
            self.layer = tgcn_amd.TGCNCheb_H(self.op, f, g, K, H).cuda()
            self.fmode, self.bias_kind, self.edge_index = F.MODE_POWER, F.BIAS_VERTEX_CHANNEL, False
            self.forward64 = lambda xw, b: O.tgcn_cheb_h_forward(self.L, xw, self.W64(), b)
        else:
            ei = np.stack([row, col]).astype(np.int64)
            self.layer = tgcn_amd.ChebTimeConv(f, g, K, H).cuda()
            self.fmode, self.bias_kind, self.edge_index = F.MODE_CHEBYSHEV, F.BIAS_CHANNEL, _dev(ei)
            self.op = self.layer._operand(torch.empty(1, n, 1, device="cuda"), self.edge_index, None)
            self.forward64 = lambda xw, b: O.cheb_time_conv_forward(xw, ei, None, self.W64(), b)
        with torch.no_grad():
            self.layer.bias.uniform_(-0.5, 0.5)

    def W64(self):
        return self.layer.weight.detach().cpu().numpy()


def _check_small(cls, graph, f, g, K, case, want_dense):
    H, d, chunks = case
    T = sum(chunks)
    su = SmallSetup(cls, graph, f, g, K, H, seed=T + K + f)
    st = FusedStreamer(su, None)
    rc, tb, dense, lds = plan_of(su.op, su.fmode, f, H, g, K, max(chunks), d)
    assert rc == 0 and dense == want_dense, (rc, tb, dense, lds, su.op.n, su.op.nnz)
    if want_dense:
        assert 2 * su.op.nnz > su.n * su.n
    series = np.random.default_rng([T, K, f, g]).standard_normal((S_REC, su.n, T, f)).astype(np.float32)
    dev = _dev(series)
    for kind in (None, "degree"):
        for bias in (True, False):
            ref = causal_reference(su, series, H, d, bias)
            out, state = st.feed(dev, chunks, kind, bias, d)
            e = rel_err(out.cpu().numpy(), ref)
            print(cls, graph, (f, g, K), case, kind, "bias" if bias else "no bias", "tb %d" % tb, "%.2e" % e)
            assert e <= TOL, (kind, bias, e)


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("graph,want_dense", [("dense37", 1), ("sparse50", 0)])
def test_partial_row_tiles_in_both_carve_ups(graph, want_dense, cls, gpu_device):
    """n = 37 and n = 50: a last tile of 5 and of 2 vertices; g = 20: a last column tile of 4; the chunk list wraps round the ring"""
    _check_small(cls, graph, 3, 20, 3, WRAP, want_dense)


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("K", [1, 2, 5])
def test_no_hop_no_recurrence_and_the_buffers_going_round(K, cls, gpu_device):
    """K = 1: the projection of the chunk alone; K = 2: one hop, no recurrence; K = 5: the three buffers of the Chebyshev mode go round
    more than once (and the fold of the power mode has something to fold)"""
    _check_small(cls, "sparse50", 4, 8, K, WRAP, 0)


# ------------------------------------------------------------------------------------------------------- one state, both routes
@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_fused_and_unfused_chunks_alternate_on_one_state(cls, gpu_device):
    H, d, chunks = WRAP
    su = Setup(cls, 4, 8, H, seed=11)
    series = np.random.default_rng(11).standard_normal((S_REC, N_VERT, sum(chunks), 4)).astype(np.float32)
    dev = _dev(series)
    ref = causal_reference(su, series, H, d, True)
    for kind in (None, "degree"):
        mixed, s_mixed = FusedStreamer(su, 11, fused=(True, False)).feed(dev, chunks, kind, True, d)
        e = rel_err(mixed.cpu().numpy(), ref)
        print(cls, kind, "alternating %.2e" % e)
        assert e <= TOL, (kind, e)
        other, s_other = FusedStreamer(su, 11, fused=(False, True)).feed(dev, chunks, kind, True, d)
        assert rel_err(other.cpu().numpy(), ref) <= TOL
        # the ring an all-fused recording leaves is the ring an all-unfused one leaves (the hops add in another order: not bit for bit)
        _, s_f = FusedStreamer(su, 11, fused=True).feed(dev, chunks, kind, True, d)
        _, s_u = FusedStreamer(su, 11, fused=False).feed(dev, chunks, kind, True, d)
        assert (s_f.head, s_f.seen) == (s_u.head, s_u.seen) == (s_mixed.head, s_mixed.seen) and s_f.head != 0
        er = float((s_f.ring - s_u.ring).abs().max() / s_u.ring.abs().max())
        print(cls, kind, "ring %.2e" % er)
        assert er <= 1e-5, er
        assert float((s_mixed.ring - s_u.ring).abs().max() / s_u.ring.abs().max()) <= 1e-5


@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_reset_starts_the_same_fused_recording_again(cls, gpu_device):
    H, d, chunks = WRAP
    su = Setup(cls, 4, 8, H, seed=9)
    st = FusedStreamer(su, 9)
    series = torch.randn(S_REC, N_VERT, sum(chunks), 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    first, state = st.feed(series, chunks, None, True, d)
    ring = state.ring.clone()
    assert state.head != 0 and state.reset() is state and (state.head, state.seen) == (0, 0) and not state.ring.any()
    again, state2 = st.feed(series, chunks, None, True, d, state=state)
    assert state2 is state and torch.equal(first, again) and torch.equal(ring, state.ring)


# ---------------------------------------------------------------------------------------------------------------------- capturable
@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_host_head_and_capturable_twins_are_equal_chunk_by_chunk(cls, gpu_device):
    """both fused: only the source of the head differs"""
    H, d, chunks = WRAP
    su = Setup(cls, 3, 8, H, seed=5)
    host, cap = FusedStreamer(su, 5), FusedStreamer(su, 5, capturable=True)
    series = torch.randn(S_REC, N_VERT, sum(chunks), 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
    s_h = s_c = None
    t = 0
    with torch.no_grad():
        for Tc in chunks:
            o_h, s_h = host.step(series[:, :, t:t + Tc], s_h, None, True, d)
            o_c, s_c = cap.step(series[:, :, t:t + Tc], s_c, None, True, d)
            cap.capturable = False          # afterwards the state's kind rules
            t += Tc
            assert torch.equal(o_h, o_c), Tc
            assert s_c.capturable and not s_h.capturable and (s_c.head, s_c.seen) == (s_h.head, s_h.seen) == (t % s_h.C, t)
    assert torch.equal(s_h.ring, s_c.ring)


@gpu
def test_a_fused_two_layer_chain_through_graphed_stream(gpu_device):
    """1 -> 8 -> relu -> 8 -> 5 with dilations 1 and 2: every replay torch.equal to the eager fused chain, the whole within TOL of the chain
    through forward_series"""
    import tgcn_amd
    n, S, H, K, TC = N_VERT, S_REC, 3, K_TERMS, 3
    rng = np.random.default_rng(23)
    row, col, val = _random_graph(n, 6, rng, hubs=((2, n - 1),))
    op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val * 0.4))
    torch.manual_seed(23)
    l1, l2 = tgcn_amd.TGCNCheb_H(op, 1, 8, K, H).cuda(), tgcn_amd.TGCNCheb_H(op, 8, 5, K, H).cuda()
    T = 7 * TC
    x = torch.randn(S, n, T, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))

    def chain(capturable):
        def step(chunk, states):
            s1, s2 = states or (None, None)
            o1, s1 = l1.forward_stream(chunk, state=s1, capturable=capturable, fused=True)
            o2, s2 = l2.forward_stream(torch.relu(o1), state=s2, dilation=2, capturable=capturable, fused=True)
            return o2, (s1, s2)
        return step

    chunks = [x[:, :, t:t + TC].contiguous() for t in range(0, T, TC)]
    with torch.no_grad():
        whole = l2.forward_series(torch.relu(l1.forward_series(x, as_series=True, padding="causal")), as_series=True, padding="causal", dilation=2)
        eager, states = [], None
        for c in chunks:
            o, states = chain(False)(c, states)
            eager.append(o)
    gs = tgcn_amd.GraphedStream(chain(True), chunks[0])
    for i, c in enumerate(chunks):
        assert torch.equal(gs(c), eager[i]), i          # the second replay is where a captured host head would go stale
    s1, s2 = gs.states
    assert (s1.seen, s2.seen, s1.head, s2.head) == (T, T, T % 2, T % 4)
    e = rel_err(torch.cat(eager, dim=2).cpu().numpy(), whole.cpu().numpy())
    print("fused two-layer chain %.2e" % e)
    assert e <= TOL, e


# ---------------------------------------------------------------------------------------------------------------- the C ABI directly
@gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["monomial", "chebyshev"])
@pytest.mark.parametrize("f,d", [(4, 1), (3, 3)])
def test_fused_entry_against_the_hop_stack_and_the_stream_entry(f, d, mode, gpu_device):
    """the same chunk and ring through both: outputs and rings afterwards within 1e-5 of their maxima (another sum order in the hops, so not
    bit for bit); with the head on the device the fused entry gives exactly what it gives with the host's head"""
    import tgcn_amd
    from tgcn_amd import _lib
    from tgcn_amd import functional as F
    L = _lib.lib()
    n, S, H, N, K = 50, 2, 4, 24, 4
    Cr = (H - 1) * d
    rng = np.random.default_rng(31 + f)
    row, col, val = _random_graph(n, 6, rng)
    op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val * 0.4))
    gen = torch.Generator(device="cuda").manual_seed(f + 10 * d)
    W = torch.randn((K, H * f, N), device="cuda", generator=gen)
    bias = torch.randn((N,), device="cuda", generator=gen)
    ring0 = torch.randn((K, S, n, Cr * f), device="cuda", generator=gen)
    for head, Tc in ((0, 5), (Cr - 1, 2), (1, 40), (Cr // 2, Cr)):
        chunk = torch.randn((S, n, Tc * f), device="cuda", generator=gen)
        stack = F._monomial_stack(op, chunk, K) if mode == 0 else F.cheb_stack(op, chunk, K, F.MODE_CHEBYSHEV, _operand_labels=True)
        ring_a, ring_b, ring_c = ring0.clone(), ring0.clone(), ring0.clone()
        out_a = torch.full((S, n, Tc, N), float("nan"), device="cuda")
        out_b, out_c = out_a.clone(), out_a.clone()
        _lib.check(L.tgcn_cheb_project_series_stream_f32(_lib.stream_ptr(), S, n, Tc, f, H, N, K, _lib.ptr(stack), _lib.ptr(W), _lib.ptr(bias), 1,
                                                         _lib.ptr(out_a), _lib.ptr(ring_a), Cr * f, head, d))
        _lib.check(L.tgcn_cheb_stream_small_f32(_lib.stream_ptr(), C.byref(op.struct), mode, S, Tc, f, H, N, K, _lib.ptr(chunk), _lib.ptr(W),
                                                _lib.ptr(bias), 1, _lib.ptr(out_b), _lib.ptr(ring_b), Cr * f, head, None, d))
        pos = torch.tensor([head, 100], dtype=torch.int64, device="cuda")
        _lib.check(L.tgcn_cheb_stream_small_f32(_lib.stream_ptr(), C.byref(op.struct), mode, S, Tc, f, H, N, K, _lib.ptr(chunk), _lib.ptr(W),
                                                _lib.ptr(bias), 1, _lib.ptr(out_c), _lib.ptr(ring_c), Cr * f, 0, _lib.ptr(pos), d))
        assert not torch.isnan(out_b).any()
        eo = float((out_a - out_b).abs().max() / out_a.abs().max())
        er = float((ring_a - ring_b).abs().max() / ring_a.abs().max())
        print((f, d, mode, head, Tc), "out %.2e ring %.2e" % (eo, er))
        assert eo <= 1e-5 and er <= 1e-5, (head, Tc, eo, er)
        assert torch.equal(out_b, out_c) and torch.equal(ring_b, ring_c) and pos.tolist() == [head, 100]        # pos is never written


@gpu
def test_refused_fused_calls_launch_nothing(gpu_device):
    import tgcn_amd
    from tgcn_amd import _lib
    L = _lib.lib()
    S, Tc, f, H, N, K, d = 1, 6, 4, 3, 8, 2, 2
    Cr = (H - 1) * d

    def operand(n):
        idx = torch.arange(n, device="cuda")
        return tgcn_amd.GraphOperand.from_coo(n, idx, (idx + 1) % n, torch.full((n,), 0.5, device="cuda"))

    for n, kw, want in ((11, dict(head=Cr), -1), (11, dict(head=-1), -1), (11, dict(Tc=0), -1), (11, dict(d=0), -1), (11, dict(ring_ld=Cr * f - 1), -1),
                        (11, dict(H=1, ring_ld=0), -1), (1025, dict(), -4)):
        op = operand(n)
        chunk, W = torch.ones(S, n, Tc * f, device="cuda"), torch.zeros(K, H * f, N, device="cuda")
        out, ring = torch.full((S, n, Tc, N), float("nan"), device="cuda"), torch.full((K, S, n, Cr * f), float("nan"), device="cuda")

        def call(Tc=Tc, H=H, ring_ld=Cr * f, head=0, d=d):
            return L.tgcn_cheb_stream_small_f32(_lib.stream_ptr(), C.byref(op.struct), 0, S, Tc, f, H, N, K, _lib.ptr(chunk), _lib.ptr(W), None, 0,
                                                _lib.ptr(out), _lib.ptr(ring), ring_ld, head, None, d)
        assert call(**kw) == want, (n, kw)
        torch.cuda.synchronize()
        assert torch.isnan(out).all() and torch.isnan(ring).all(), (n, kw)
        if n == 1025:
            assert plan_of(op, 0, f, H, N, K, Tc, d)[0] == -4
            continue
        ring.zero_()                                                          # (a NaN in the ring would be read: it is the past)
        assert call() == 0
        torch.cuda.synchronize()
        assert not out.any() and (ring[0] == 1).all() and (ring[1] == 0.5).all()      # W = 0; Tc >= C: every slot written, term 1 = A . 1
