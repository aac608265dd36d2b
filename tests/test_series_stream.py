"""Streaming state: forward_stream / F.cheb_time_stream feed a series chunk after chunk through a causal time layer that keeps the last
C = (H - 1)*dilation time rows of its hop stack in a ring.  The outputs of the chunks, concatenated along time, are compared with the fp64
oracle on the materialised causal dilated windows of the WHOLE series (tests/test_series_dilation.py's rule and output bound, 1e-5 of the
tensor's maximum) -- both classes, with and without a bias, on a plain and on a degree-reordered operand.

The chunk lists hit each way the ring can go wrong: chunks shorter than the ring with wrap-around, as long as it, longer; a chunk of two
32-window tiles with unequal phases; a non-zero head at every kind of chunk; the undilated kernel with three tiles per vertex and a tail
wave; a ring that is still mostly zeros with empty phases (q >= Tc) and negative window starts; one tap (no ring); the chunked-span regime.
Then a two-layer chain against the same chain through forward_series, a second pass after state.reset(), and the C ABI directly: the stream
entry is bit-identical to the windows [t0, t0 + Tc) of the _dilated entry on the whole stack, and leaves the ring a fresh fill would."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from test_hip_parity import _random_graph
from test_series_channels import TOL, _dev
from test_series_dilation import CHUNKED, CLASSES, K_TERMS, N_VERT, S_REC, Setup, conv_plan, windows_dilated

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]

# (H, dilation, chunk sizes)
WRAP = (3, 4, (1, 1, 3, 8, 9, 40, 5))      # C = 8
UNDILATED = (5, 1, (2, 70, 1, 33))         # C = 4
SPARSE_RING = (5, 7, (3, 3, 50))           # C = 28
ONE_TAP = (1, 3, (4, 1, 9))                # no ring
LISTS = [WRAP, UNDILATED, SPARSE_RING, ONE_TAP]


def test_the_chunk_lists_hit_what_they_are_here_for():
    H, d, chunks = WRAP
    Cr = (H - 1) * d
    heads = [int(h) % Cr for h in np.cumsum((0,) + chunks[:-1])]
    kinds = {"below": [t < Cr for t in chunks], "equal": [t == Cr for t in chunks], "above": [t > Cr for t in chunks]}
    assert all(any(h != 0 for k, h in zip(kinds[name], heads) if k) for name in kinds)        # every kind of chunk, each at a non-zero head
    assert any(t < Cr and h + t > Cr for t, h in zip(chunks, heads))                          # a short chunk that wraps round the ring's end
    assert any(t > 32 for t in chunks) and any(t > d and t % d for t in chunks)               # more than one tile's windows; unequal phases
    H, d, chunks = UNDILATED
    assert d == 1 and -(-max(chunks) // 32) == 3 and max(chunks) % 32                         # three tiles per vertex, the last one partial
    H, d, chunks = SPARSE_RING
    assert chunks[0] < d and sum(chunks[:2]) < (H - 1) * d                                    # phases q >= Tc; a ring that is mostly zeros
    assert ONE_TAP[0] == 1 and ONE_TAP[1] > 1


def edge_index_of(seed):
    """the edge list Setup draws for ChebTimeConv (its first use of the seed)"""
    row, col, _ = _random_graph(N_VERT, 6, np.random.default_rng(seed), hubs=((2, N_VERT - 1),))
    return _dev(np.stack([row, col]).astype(np.int64))


class Streamer:
    """forward_stream on the layer's own operand with its bias; F.cheb_time_stream for a reordered operand or no bias (Setup.call's split)"""

    def __init__(self, su, seed):
        self.su = su
        self.extra = () if su.cls == "TGCNCheb_H" else (edge_index_of(seed), None)
        if self.extra:      # the module's operand for this edge list is the one Setup holds: the same graph
            op = su.layer._operand(torch.empty(1, N_VERT, 1, device="cuda"), self.extra[0], None)
            assert torch.equal(op.rowptr, su.op.rowptr)

    def step(self, chunk, state, kind, bias, d):
        su = self.su
        if kind is None and bias:
            return su.layer.forward_stream(chunk, *self.extra, state=state, dilation=d)
        op = su.op
        if kind is not None:
            if su.reordered is None:
                su.reordered = su.op.reordered(kind)
            op = su.reordered
        W = su.layer.weight if chunk.dim() == 4 else su.layer.weight.reshape(K_TERMS, su.layer.weight.shape[1], -1)
        return su.F.cheb_time_stream(op, chunk, W, su.layer.bias.reshape(-1) if bias else None, su.bias_kind if bias else su.F.BIAS_NONE,
                                     su.fmode, state, d)

    def feed(self, series, chunks, kind, bias, d, state=None):
        """the whole series chunk by chunk -> (outputs concatenated along time, state)"""
        outs, t = [], 0
        with torch.no_grad():
            for Tc in chunks:
                out, state = self.step(series[:, :, t:t + Tc], state, kind, bias, d)
                g = out.shape[-1]
                assert tuple(out.shape) == (series.shape[0], series.shape[1], Tc, g) and out.is_contiguous() and out.dtype == series.dtype
                t += Tc
                assert state.seen == t and state.head == (t % state.C if state.C else 0)
                outs.append(out)
        assert t == series.shape[2]
        return torch.cat(outs, dim=2), state


def causal_reference(su, series, H, d, bias):
    """fp64 oracle on the materialised causal dilated windows of the whole series, as a series (S, n, T, g)"""
    S, n, T, f = series.shape
    xw = windows_dilated(series, H, d, (H - 1) * d, 0).astype(np.float64)
    ref = su.forward64(xw, su.layer.bias.detach().cpu().numpy() if bias else None)
    return ref.reshape(S, T, n, -1).transpose(0, 2, 1, 3)


def _check(cls, H, d, chunks, f, g, three_d=False):
    T = sum(chunks)
    seed = T + 7 * d + f
    su = Setup(cls, f, g, H, seed=seed)
    st = Streamer(su, seed)
    series = np.random.default_rng([T, d, f, g]).standard_normal((S_REC, N_VERT, T, f)).astype(np.float32)
    dev = _dev(series[..., 0] if three_d else series)
    refs = {bias: causal_reference(su, series, H, d, bias) for bias in (True, False)}
    for kind in (None, "degree"):
        for bias in (True, False):
            out, state = st.feed(dev, chunks, kind, bias, d)
            e = rel_err(out.cpu().numpy(), refs[bias])
            print(cls, (H, d, chunks, f, g), kind, "bias" if bias else "no bias", "%.2e" % e)
            assert e <= TOL, (kind, bias, e)
    return su, st, dev


def _id(c):
    return "H%d_d%d" % c[:2]


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("g", [5, 40])
@pytest.mark.parametrize("f", [4, 3, "3d"])
@pytest.mark.parametrize("case", LISTS, ids=_id)
def test_chunked_stream_vs_oracle(case, f, g, cls, gpu_device):
    H, d, chunks = case
    if f == "3d":
        _check(cls, H, d, chunks, 1, g, three_d=True)
    else:
        _check(cls, H, d, chunks, f, g)


@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_chunked_stream_with_a_chunked_span(cls, gpu_device):
    T, H, d, f, g, left, right = CHUNKED[0]
    rc, hc, lds = conv_plan(H, f, g)
    assert rc == 0 and hc < H, "this case is here for the chunked regime, the launcher plans HC = %d of %d" % (hc, H)
    _check(cls, H, d, (30, T - 30), f, g)


@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_reset_starts_the_same_recording_again(cls, gpu_device):
    H, d, chunks = WRAP
    su = Setup(cls, 4, 8, H, seed=9)
    st = Streamer(su, 9)
    series = torch.randn(S_REC, N_VERT, sum(chunks), 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    for kind in (None, "degree"):
        first, state = st.feed(series, chunks, kind, True, d)
        ring = state.ring.clone()
        assert state.head != 0 and state.reset() is state and (state.head, state.seen) == (0, 0) and not state.ring.any()
        again, state2 = st.feed(series, chunks, kind, True, d, state=state)
        assert state2 is state and torch.equal(first, again) and torch.equal(ring, state.ring)
        # and a fresh state is a reset one
        fresh, _ = st.feed(series, chunks, kind, True, d)
        assert torch.equal(first, fresh)


@gpu
def test_two_layer_chain_equals_the_chain_through_forward_series(gpu_device):
    """1 -> 8 -> relu -> 8 -> 5 with dilations 1 and 2, one state per layer; the reference is the same chain on the whole series"""
    import tgcn_amd
    n, S, H, K = N_VERT, S_REC, 3, K_TERMS
    chunks = (1, 5, 3, 40, 2, 33, 4)
    T = sum(chunks)
    rng = np.random.default_rng(21)
    row, col, val = _random_graph(n, 6, rng, hubs=((2, n - 1),))
    op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val * 0.4))
    torch.manual_seed(21)
    l1, l2 = tgcn_amd.TGCNCheb_H(op, 1, 8, K, H).cuda(), tgcn_amd.TGCNCheb_H(op, 8, 5, K, H).cuda()
    x = torch.randn(S, n, T, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    with torch.no_grad():
        whole = l2.forward_series(torch.relu(l1.forward_series(x, as_series=True, padding="causal")), as_series=True, padding="causal", dilation=2)
        s1 = s2 = None
        outs, t = [], 0
        for Tc in chunks:
            o1, s1 = l1.forward_stream(x[:, :, t:t + Tc], s1)
            o2, s2 = l2.forward_stream(torch.relu(o1), s2, dilation=2)
            outs.append(o2)
            t += Tc
    got = torch.cat(outs, dim=2)
    assert tuple(got.shape) == tuple(whole.shape) == (S, n, T, 5) and (s1.seen, s2.seen, s1.C, s2.C) == (T, T, 2, 4)
    e = rel_err(got.cpu().numpy(), whole.cpu().numpy())
    print("two-layer chain %.2e" % e)
    assert e <= TOL, e


@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_a_weight_that_changes_between_chunks_is_the_weight_of_the_chunk(cls, gpu_device):
    """the ring holds hop tensors, nothing of the weight: every chunk is projected with the weight of ITS call -- a temporary that is freed
    after the call (the next one may get its address), then one written through .data -- and equals those rows of the whole-series call with
    that weight"""
    H, d, chunks = 3, 2, (5, 9, 1, 20)
    su = Setup(cls, 4, 8, H, seed=13)
    F = su.F
    series = torch.randn(S_REC, N_VERT, sum(chunks), 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    W0 = su.layer.weight.detach().clone()
    state, t = None, 0
    with torch.no_grad():
        for i, Tc in enumerate(chunks):
            if i % 2 == 0:
                W = (W0 * (1.0 + i)).clone()            # a temporary per call
            else:
                W = W0.clone()
                W.data.mul_(-0.5 * i)                   # written through .data: the version counter does not move
            out, state = F.cheb_time_stream(su.op, series[:, :, t:t + Tc], W, None, F.BIAS_NONE, su.fmode, state, d)
            whole = F.cheb_time_windows(su.op, series, W, None, F.BIAS_NONE, su.fmode, as_series=True, padding="causal", dilation=d)
            e = rel_err(out.cpu().numpy(), whole[:, :, t:t + Tc].cpu().numpy())
            print(cls, i, "%.2e" % e)
            assert e <= TOL, (i, e)
            del W
            t += Tc


# ---------------------------------------------------------------------------------------------------------------- the C ABI directly
def ring_of(stack5, t0, Cr, ring_ld, fill):
    """the ring (K, S, n, ring_ld) that holds the time rows [t0 - Cr, t0) of stack5 (K, S, n, T, f) at the slots of the map -- row a at slot
    a mod Cr, zeros where a < 0; the elements past Cr*f keep `fill`"""
    K, S, n, T, f = stack5.shape
    ring = torch.full((K, S, n, ring_ld), fill, dtype=stack5.dtype, device=stack5.device)
    ring[..., :Cr * f] = 0
    for a in range(max(0, t0 - Cr), t0):
        ring[..., (a % Cr) * f:(a % Cr + 1) * f] = stack5[:, :, :, a]
    return ring


def stream_entry_bit_identity(dt, f, d, pad_ring=False, odd_ring=False):
    """one random stack; for (t0, Tc) pairs whose heads differ (one of them wraps): the stream entry on rows [t0, t0 + Tc) with the ring of the
    rows before them equals windows [t0, t0 + Tc) of the _dilated entry on the whole stack at pads (C, 0), and leaves the ring of t0 + Tc"""
    from tgcn_amd import _lib
    L = _lib.lib()
    bf16 = dt == torch.bfloat16
    n, S, T, H, N, K = 37, 2, 80, 4, 24, 3
    Cr = (H - 1) * d
    ring_ld = Cr * f if not pad_ring else (Cr * f + 8) // 8 * 8
    if odd_ring:        # f allows 16-byte accesses, the ring's rows do not: the entry stages and copies narrow
        assert f % (8 if bf16 else 4) == 0
        ring_ld = Cr * f + 1
    gen = torch.Generator(device="cuda").manual_seed(f + 10 * d)
    stack = torch.randn((K, S, n, T, f), device="cuda", generator=gen).to(dt)
    W = torch.randn((K, H * f, N), device="cuda", generator=gen).to(dt)
    bias = torch.randn((N,), device="cuda", generator=gen).to(dt)
    whole = torch.full((S, n, T, N), float("nan"), device="cuda", dtype=dt)
    head = (_lib.stream_ptr(), S, n, T, f, H, N, K, _lib.ptr(stack))
    if bf16:
        _lib.check(L.tgcn_cheb_project_series_dilated_bf16(*head, T * f, _lib.ptr(W), _lib.ptr(bias), _lib.DTYPE_BF16, 1, 1, _lib.ptr(whole), 1, Cr, 0, d))
    else:
        _lib.check(L.tgcn_cheb_project_series_dilated_f32(*head, _lib.ptr(W), _lib.ptr(bias), 1, 1, _lib.ptr(whole), 1, Cr, 0, d))
    assert not torch.isnan(whole).any()
    pairs = [(0, 5), (2, 40), (5, 1), (8, 2), (7, 20), (31, 49), (70, Cr), (77, 3)]
    assert len({t0 % Cr for t0, _ in pairs}) >= min(Cr, 3) and any(0 < Tc < Cr and t0 % Cr + Tc > Cr for t0, Tc in pairs)
    for t0, Tc in pairs:
        chunk = stack[:, :, :, t0:t0 + Tc].contiguous()
        ring = ring_of(stack, t0, Cr, ring_ld, 7.0)
        out = torch.full((S, n, Tc, N), float("nan"), device="cuda", dtype=dt)
        args = (_lib.stream_ptr(), S, n, Tc, f, H, N, K, _lib.ptr(chunk))
        tail = (_lib.ptr(out), _lib.ptr(ring), ring_ld, t0 % Cr, d)
        if bf16:
            _lib.check(L.tgcn_cheb_project_series_stream_bf16(*args, Tc * f, _lib.ptr(W), _lib.ptr(bias), _lib.DTYPE_BF16, 1, *tail))
        else:
            _lib.check(L.tgcn_cheb_project_series_stream_f32(*args, _lib.ptr(W), _lib.ptr(bias), 1, *tail))
        assert torch.equal(out, whole[:, :, t0:t0 + Tc]), (t0, Tc)
        assert torch.equal(ring, ring_of(stack, t0 + Tc, Cr, ring_ld, 7.0)), (t0, Tc)


@gpu
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("f", [4, 3], ids=["aligned", "unaligned"])
def test_stream_entry_is_the_dilated_entry_on_the_whole_stack(f, d, gpu_device):
    stream_entry_bit_identity(torch.float32, f, d)


@gpu
@pytest.mark.parametrize("d", [1, 3])
def test_stream_entry_with_a_ring_that_rules_out_16_byte_accesses(d, gpu_device):
    """f = 4 on ring rows of C*f + 1 floats: the stack would take the 16-byte form, the ring cannot -- the narrow staging and the element-wise
    ring update, the same numbers"""
    stream_entry_bit_identity(torch.float32, 4, d, odd_ring=True)


@gpu
def test_refused_calls_launch_nothing(gpu_device):
    """through the C ABI: an error code, the output and the ring untouched"""
    from tgcn_amd import _lib
    L = _lib.lib()
    n, S, Tc, f, H, N, K, d = 11, 1, 6, 4, 3, 8, 2, 2
    Cr = (H - 1) * d
    stack, W = torch.ones(K, S, n, Tc * f, device="cuda"), torch.zeros(K, H * f, N, device="cuda")
    out, ring = torch.full((S, n, Tc, N), float("nan"), device="cuda"), torch.full((K, S, n, Cr * f), float("nan"), device="cuda")

    def call(Tc=Tc, H=H, ring_ld=Cr * f, head=0, d=d):
        return L.tgcn_cheb_project_series_stream_f32(_lib.stream_ptr(), S, n, Tc, f, H, N, K, _lib.ptr(stack), _lib.ptr(W), None, 0, _lib.ptr(out),
                                                     _lib.ptr(ring), ring_ld, head, d)
    assert call(head=Cr) == -1 and call(head=-1) == -1 and call(Tc=0) == -1 and call(d=0) == -1 and call(ring_ld=Cr * f - 1) == -1
    assert call(H=1, ring_ld=0) == -1
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(ring).all()
    ring.zero_()                                                              # (a NaN in the ring would be read: it is the past)
    assert call() == 0
    torch.cuda.synchronize()
    assert not out.any() and (ring == 1).all()                                # W = 0; Tc >= C: every slot written from the stack
