"""Streaming state with a window step: forward_stream / F.cheb_time_stream(..., stride=s) return, chunk after chunk, the rows of
forward_series(whole, as_series=True, padding="causal", stride=s) whose window ends inside the chunk.

The non-empty chunk outputs, concatenated along time, are compared with the fp64 oracle on the materialised causal strided windows of the
WHOLE series (tests/test_series_conv.py's windows_conv at pads (H-1, 0); the output bound of tests/test_series_channels.py, 1e-5 of the
tensor's maximum) -- both classes, with a bias and without, on a plain and on a degree-reordered operand.  The chunk lists hit each way the
step can go wrong on a ring: both phases of an even step at non-zero heads, chunks in which no window ends, more than one tile of windows, a
step that is no smaller than the window (no two windows share a staged row), a step above the chunk length, one tap (no ring).
Then the C ABI directly: the _stream_strided entry is bit-identical to the rows of the _conv entry on the whole stack and leaves the ring the
step-1 stream entry leaves; at stride 1 it IS the stream entry, with the host's head or the device's position; refusals launch nothing.
Then chains: two layers of step 2 against the same chain through forward_series, a second pass after reset(), and the chain captured into
a hipGraph by GraphedStream."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from test_series_channels import TOL, _dev
from test_series_conv import windows_conv
from test_series_dilation import CLASSES, K_TERMS, N_VERT, S_REC, Setup, conv_plan
from test_hip_parity import _random_graph
from test_series_stream import Streamer

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]

# (H, step, chunk sizes)
WRAP = (5, 2, (1, 1, 3, 4, 8, 9, 70, 5, 1))     # C = 4
NO_OVERLAP = (3, 5, (2, 2, 7, 1, 12, 4))        # C = 2
STEP_OVER_CHUNK = (3, 7, (2, 2, 2, 2, 9))       # C = 2
WIDE = (4, 3, (100, 2, 33))                     # C = 3
ONE_TAP = (1, 3, (4, 1, 9))                     # no ring
LISTS = [WRAP, NO_OVERLAP, STEP_OVER_CHUNK, WIDE, ONE_TAP]
CHUNKED = (20, 48, 8, 2)                        # (H, f, N, step): the plan answers HC < H (tests/test_series_conv.py, "fwd-chunked-vec")
ENTRIES = ("tgcn_cheb_project_series_stream_strided_f32", "tgcn_cheb_project_series_stream_strided_bf16")


def require_entries():
    """every GPU test starts here: the library has the two entries"""
    from tgcn_amd import _lib
    L = _lib.lib()
    for nm in ENTRIES:
        assert nm in _lib.SIGNATURES and hasattr(L, nm), nm
    return L


def windows_of(seen, Tc, s):
    """(m, off) by counting: the windows (ending at absolute rows j*s) that end inside the chunk, the chunk row of the first"""
    ends = [t - seen for t in range(seen, seen + Tc) if t % s == 0]
    return len(ends), (ends[0] if ends else (-seen) % s)


def walk(chunks, s):
    """[(seen, Tc, m, off)] of a chunk list"""
    out, seen = [], 0
    for Tc in chunks:
        out.append((seen, Tc) + windows_of(seen, Tc, s))
        seen += Tc
    return out


def test_the_chunk_lists_hit_what_they_are_here_for():
    H, s, chunks = WRAP
    Cr, w = H - 1, walk(chunks, s)
    for kind in (lambda t: t < Cr, lambda t: t == Cr, lambda t: t > Cr):                    # shorter than, equal to, longer than the ring ...
        assert any(kind(Tc) and seen % Cr != 0 for seen, Tc, m, off in w)                   # ... each at a non-zero head
    assert {off for seen, Tc, m, off in w} == {0, 1}                                       # both phases
    assert sum(1 for seen, Tc, m, off in w if m == 0) == 2                                 # two chunks in which no window ends
    assert any(m == 35 for seen, Tc, m, off in w)                                          # two tiles of windows, the second partial
    assert any(Tc < Cr and seen % Cr + Tc > Cr for seen, Tc, m, off in w)                  # a short chunk that wraps round the ring's end
    H, s, chunks = NO_OVERLAP
    assert s >= H and {off for seen, Tc, m, off in walk(chunks, s)} >= {0, 1, 3, 4}
    H, s, chunks = STEP_OVER_CHUNK
    w = walk(chunks, s)
    assert s > max(chunks[:-1]) and any(a[2] == 0 and b[2] == 0 for a, b in zip(w, w[1:])) and any(m == 1 and Tc < s for seen, Tc, m, off in w)
    H, s, chunks = WIDE
    w = walk(chunks, s)
    assert w[0][2] == 34 and w[1][2] == 0 and w[1][0] % (H - 1) == 1                       # 34 windows; an empty chunk at head 1
    assert ONE_TAP[0] == 1 and ONE_TAP[1] > 1
    for H, s, chunks in LISTS:
        T = sum(chunks)
        assert sum(m for seen, Tc, m, off in walk(chunks, s)) == (T - 1) // s + 1


def test_the_plan_chunks_the_chunked_shape():
    H, f, N, s = CHUNKED
    rc, hc, lds = conv_plan(H, f, N, s)
    assert rc == 0 and hc < H, "this shape is here for the chunked regime, the launcher plans HC = %d of %d" % (hc, H)


class StrideStreamer(Streamer):
    """tests/test_series_stream.py's Streamer with the step"""

    def step(self, chunk, state, kind, bias, s):
        su = self.su
        if kind is None and bias:
            return su.layer.forward_stream(chunk, *self.extra, state=state, stride=s)
        op = su.op
        if kind is not None:
            if su.reordered is None:
                su.reordered = su.op.reordered(kind)
            op = su.reordered
        W = su.layer.weight if chunk.dim() == 4 else su.layer.weight.reshape(K_TERMS, su.layer.weight.shape[1], -1)
        return su.F.cheb_time_stream(op, chunk, W, su.layer.bias.reshape(-1) if bias else None, su.bias_kind if bias else su.F.BIAS_NONE,
                                     su.fmode, state, stride=s)

    def feed(self, series, chunks, kind, bias, s, state=None):
        """the whole series chunk by chunk -> (the non-empty outputs concatenated along time, state)"""
        outs, t = [], 0
        with torch.no_grad():
            for Tc in chunks:
                m, off = windows_of(t, Tc, s)
                out, state = self.step(series[:, :, t:t + Tc], state, kind, bias, s)
                assert tuple(out.shape) == (series.shape[0], series.shape[1], m, out.shape[-1]) and out.is_contiguous() and out.dtype == series.dtype
                t += Tc
                assert state.seen == t and state.head == (t % state.C if state.C else 0) and state.stride == s
                if m:
                    outs.append(out)
        assert t == series.shape[2]
        return torch.cat(outs, dim=2), state


def strided_reference(su, series, H, s, bias):
    """fp64 oracle on the materialised causal strided windows of the whole series, as a series (S, n, nwin, g)"""
    S, n, T, f = series.shape
    xw = windows_conv(series, H, s, H - 1, 0).astype(np.float64)
    ref = su.forward64(xw, su.layer.bias.detach().cpu().numpy() if bias else None)
    return ref.reshape(S, (T - 1) // s + 1, n, -1).transpose(0, 2, 1, 3)


def _check(cls, H, s, chunks, f, g, three_d=False):
    T = sum(chunks)
    seed = T + 7 * s + f
    su = Setup(cls, f, g, H, seed=seed)
    st = StrideStreamer(su, seed)
    series = np.random.default_rng([T, s, f, g]).standard_normal((S_REC, N_VERT, T, f)).astype(np.float32)
    dev = _dev(series[..., 0] if three_d else series)
    refs = {bias: strided_reference(su, series, H, s, bias) for bias in (True, False)}
    for kind in (None, "degree"):
        for bias in (True, False):
            out, state = st.feed(dev, chunks, kind, bias, s)
            assert tuple(out.shape) == refs[bias].shape
            e = rel_err(out.cpu().numpy(), refs[bias])
            print(cls, (H, s, chunks, f, g), kind, "bias" if bias else "no bias", "%.2e" % e)
            assert e <= TOL, (kind, bias, e)


def _id(c):
    return "H%d_s%d" % c[:2]


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("g", [5, 32])
@pytest.mark.parametrize("f", [4, 3, "3d"])
@pytest.mark.parametrize("case", LISTS, ids=_id)
def test_strided_stream_vs_oracle(case, f, g, cls, gpu_device):
    require_entries()
    H, s, chunks = case
    if f == "3d":
        _check(cls, H, s, chunks, 1, g, three_d=True)
    else:
        _check(cls, H, s, chunks, f, g)


@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_strided_stream_with_a_chunked_span(cls, gpu_device):
    require_entries()
    H, f, N, s = CHUNKED
    assert conv_plan(H, f, N, s)[1] < H
    _check(cls, H, s, (7, 30, 1, 12), f, N)


@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_reset_starts_the_same_recording_again(cls, gpu_device):
    require_entries()
    H, s, chunks = WRAP
    su = Setup(cls, 4, 8, H, seed=9)
    st = StrideStreamer(su, 9)
    series = torch.randn(S_REC, N_VERT, sum(chunks), 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    for kind in (None, "degree"):
        first, state = st.feed(series, chunks, kind, True, s)
        ring = state.ring.clone()
        assert state.head != 0 and state.reset() is state and (state.head, state.seen, state.stride) == (0, 0, s) and not state.ring.any()
        again, state2 = st.feed(series, chunks, kind, True, s, state=state)
        assert state2 is state and torch.equal(first, again) and torch.equal(ring, state.ring)


# ---------------------------------------------------------------------------------------------------------------- the C ABI directly
class Abi:
    """one random stack (K, S, n, T, f) with weight and bias; the entries of a dtype on its chunks.  bf16: stack rows padded to stack_ld"""

    def __init__(self, dt, f, H, T, ring_pad=0, stack_pad=0, N=24):
        from tgcn_amd import _lib
        self._lib, self.L = _lib, require_entries()
        self.dt, self.f, self.H, self.T, self.bf16 = dt, f, H, T, dt == torch.bfloat16
        self.n, self.S, self.N, self.K = 37, 2, N, 3
        self.Cr = H - 1
        self.ring_ld = self.Cr * f + ring_pad
        self.stack_pad = stack_pad
        gen = torch.Generator(device="cuda").manual_seed(f + 10 * H + T)
        self.stack = torch.randn((self.K, self.S, self.n, T, f), device="cuda", generator=gen).to(dt)
        self.W = torch.randn((self.K, H * f, self.N), device="cuda", generator=gen).to(dt)
        self.bias = torch.randn((self.N,), device="cuda", generator=gen).to(dt)

    def ring(self):
        return torch.zeros((self.K, self.S, self.n, self.ring_ld), device="cuda", dtype=self.dt) if self.Cr else None

    def rows(self, t0, Tc):
        """(the chunk's stack as the entries read it, its row leading dimension)"""
        flat = self.stack[:, :, :, t0:t0 + Tc].reshape(self.K, self.S, self.n, Tc * self.f)
        if self.stack_pad:
            flat = torch.nn.functional.pad(flat, (0, self.stack_pad), value=3.0)
        return flat.contiguous(), Tc * self.f + self.stack_pad

    def _args(self, rows, ld, T):
        _lib = self._lib
        head = (_lib.stream_ptr(), self.S, self.n, T, self.f, self.H, self.N, self.K, _lib.ptr(rows))
        mid = (ld, _lib.ptr(self.W), _lib.ptr(self.bias), _lib.DTYPE_BF16, 1) if self.bf16 else (_lib.ptr(self.W), _lib.ptr(self.bias), 1)
        return head + mid

    def whole(self, s):
        """the _conv entry on the whole stack at pads (H-1, 0), as_series = 1, step s -> (S, n, nwin, N)"""
        _lib = self._lib
        nwin = (self.T - 1) // s + 1
        out = torch.full((self.S, self.n, nwin, self.N), float("nan"), device="cuda", dtype=self.dt)
        rows, ld = self.rows(0, self.T)
        entry = self.L.tgcn_cheb_project_series_conv_bf16 if self.bf16 else self.L.tgcn_cheb_project_series_conv_f32
        _lib.check(entry(*self._args(rows, ld, self.T), 1, _lib.ptr(out), s, self.Cr, 0))
        assert not torch.isnan(out).any()
        return out

    def strided(self, t0, Tc, ring, head, pos, s, off, check=True):
        """the _stream_strided entry on rows [t0, t0 + Tc) -> (rc, out (S, n, m, N))"""
        _lib = self._lib
        m = (Tc - off - 1) // s + 1 if off < Tc else 0
        out = torch.full((self.S, self.n, m, self.N), float("nan"), device="cuda", dtype=self.dt)
        rows, ld = self.rows(t0, Tc)
        entry = self.L.tgcn_cheb_project_series_stream_strided_bf16 if self.bf16 else self.L.tgcn_cheb_project_series_stream_strided_f32
        rc = entry(*self._args(rows, ld, Tc), _lib.ptr(out) if m else None, _lib.ptr(ring), self.ring_ld, head, _lib.ptr(pos), s, off)
        if check:
            _lib.check(rc)
        return rc, out

    def stream(self, t0, Tc, ring, head):
        """the step-1 stream entry on the same rows -> out (S, n, Tc, N)"""
        _lib = self._lib
        out = torch.full((self.S, self.n, Tc, self.N), float("nan"), device="cuda", dtype=self.dt)
        rows, ld = self.rows(t0, Tc)
        entry = self.L.tgcn_cheb_project_series_stream_bf16 if self.bf16 else self.L.tgcn_cheb_project_series_stream_f32
        _lib.check(entry(*self._args(rows, ld, Tc), _lib.ptr(out), _lib.ptr(ring), self.ring_ld, head, 1))
        return out


def strided_entry_bit_identity(dt, f, case, ring_pad=0, stack_pad=0):
    """over a chunk list: the entry's rows equal the _conv entry's on the whole stack, and its ring the step-1 stream entry's on a twin"""
    H, s, chunks = case
    a = Abi(dt, f, H, sum(chunks), ring_pad, stack_pad)
    whole = a.whole(s)
    ring, twin = a.ring(), a.ring()
    for seen, Tc, m, off in walk(chunks, s):
        head = seen % a.Cr if a.Cr else 0
        rc, out = a.strided(seen, Tc, ring, head, None, s, off)
        j0 = -(-seen // s)
        assert tuple(out.shape) == (a.S, a.n, m, a.N) and torch.equal(out, whole[:, :, j0:j0 + m]), (seen, Tc, m, off)
        if a.Cr:
            a.stream(seen, Tc, twin, head)
            assert torch.equal(ring, twin), (seen, Tc)
    if a.Cr:
        assert ring[..., :a.Cr * f].any() and (not ring_pad or not ring[..., a.Cr * f:].any())      # the padding of a ring row is never written


@gpu
@pytest.mark.parametrize("f", [4, 3], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("case", LISTS, ids=_id)
def test_strided_entry_is_the_conv_entry_on_the_whole_stack(case, f, gpu_device):
    strided_entry_bit_identity(torch.float32, f, case)


@gpu
@pytest.mark.parametrize("case", [WRAP, NO_OVERLAP], ids=_id)
def test_strided_entry_with_a_ring_that_rules_out_16_byte_accesses(case, gpu_device):
    """f = 4 on ring rows of C*f + 1 floats: the stack would take the 16-byte form, the ring cannot -- narrow staging, the same numbers"""
    strided_entry_bit_identity(torch.float32, 4, case, ring_pad=1)


def step_one_equivalence(dt, f, stack_pad=0):
    """stride 1, win_off 0: the stream entry's output and ring; with pos, the host-head form on twin rings and pos = {seen mod C, seen}"""
    H, chunks = 4, (1, 2, 5, 40, 3)
    a = Abi(dt, f, H, sum(chunks), 0, stack_pad)
    rings = [a.ring() for _ in range(3)]
    pos = torch.zeros(2, dtype=torch.int64, device="cuda")
    seen = 0
    for Tc in chunks:
        head = seen % a.Cr
        want = a.stream(seen, Tc, rings[0], head)
        _, host = a.strided(seen, Tc, rings[1], head, None, 1, 0)
        _, dev = a.strided(seen, Tc, rings[2], 0, pos, 1, 0)
        seen += Tc
        assert not torch.isnan(want).any() and torch.equal(want, host) and torch.equal(want, dev), Tc
        assert torch.equal(rings[0], rings[1]) and torch.equal(rings[0], rings[2]) and pos.tolist() == [seen % a.Cr, seen], Tc
    # and with a step: the device position against the host's head on twin rings
    s = 2
    rings = [a.ring() for _ in range(2)]
    pos.zero_()
    for seen, Tc, m, off in walk((4, 2, 6, 10, 20, 9), s):
        _, host = a.strided(seen, Tc, rings[0], seen % a.Cr, None, s, off)
        _, dev = a.strided(seen, Tc, rings[1], 0, pos, s, off)
        assert torch.equal(host, dev) and torch.equal(rings[0], rings[1]) and pos.tolist() == [(seen + Tc) % a.Cr, seen + Tc], (seen, Tc)


@gpu
@pytest.mark.parametrize("f", [4, 3], ids=["aligned", "unaligned"])
def test_strided_entry_at_step_one_is_the_stream_entry(f, gpu_device):
    step_one_equivalence(torch.float32, f)


@gpu
def test_refused_calls_launch_nothing(gpu_device):
    """through the C ABI: an error code, the sentinel-filled output and the ring untouched"""
    from tgcn_amd import _lib
    L = require_entries()
    INVALID, UNSUPPORTED = -1, -4
    n, S, Tc, f, H, N, K = 11, 1, 6, 4, 3, 8, 2
    Cr = H - 1
    stack, W = torch.ones(K, S, n, Tc * f, device="cuda"), torch.zeros(K, H * f, N, device="cuda")
    out, ring = torch.full((S, n, Tc, N), float("nan"), device="cuda"), torch.full((K, S, n, Cr * f), float("nan"), device="cuda")
    pos = torch.tensor([1, 5], dtype=torch.int64, device="cuda")

    def call(Tc=Tc, H=H, ring_ld=Cr * f, head=0, pos=None, stride=2, off=0, bias_kind=0, ring=ring):
        return L.tgcn_cheb_project_series_stream_strided_f32(_lib.stream_ptr(), S, n, Tc, f, H, N, K, _lib.ptr(stack), _lib.ptr(W), None, bias_kind,
                                                             _lib.ptr(out), _lib.ptr(ring), ring_ld, head, _lib.ptr(pos), stride, off)
    assert call(stride=0) == INVALID and call(stride=-1) == INVALID
    assert call(off=2) == INVALID and call(off=-1) == INVALID and call(stride=1, off=1) == INVALID
    assert call(head=Cr) == INVALID and call(head=-1) == INVALID and call(Tc=0) == INVALID and call(ring_ld=Cr * f - 1) == INVALID
    assert call(ring=None) == INVALID and call(bias_kind=1) == INVALID and call(H=0) == INVALID
    assert call(pos=pos, ring_ld=Cr * f - 1) == INVALID and call(pos=pos, off=2) == INVALID
    # the plan refuses: so many channels that one weight time row fits no LDS (the query says so first)
    fbig = next((c for c in range(4, 4096, 4) if conv_plan(H, c, N, 2)[0] == UNSUPPORTED), None)
    assert fbig is not None
    bstack, bW = torch.ones(K, S, n, Tc * fbig, device="cuda"), torch.zeros(K, H * fbig, N, device="cuda")
    bring = torch.full((K, S, n, Cr * fbig), float("nan"), device="cuda")
    for p in (None, pos):
        rc = L.tgcn_cheb_project_series_stream_strided_f32(_lib.stream_ptr(), S, n, Tc, fbig, H, N, K, _lib.ptr(bstack), _lib.ptr(bW), None, 0,
                                                           _lib.ptr(out), _lib.ptr(bring), Cr * fbig, 0, _lib.ptr(p), 2, 0)
        assert rc == UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(ring).all() and torch.isnan(bring).all() and pos.tolist() == [1, 5]
    ring.zero_()                                                              # (a NaN in the ring would be read: it is the past)
    assert call() == 0
    torch.cuda.synchronize()
    flat, m = out.reshape(-1), 3                                              # W = 0: (S, n, m, N) zeros at the front of the buffer; Tc >= C
    assert not flat[:S * n * m * N].any() and torch.isnan(flat[S * n * m * N:]).all() and (ring == 1).all()


# ---------------------------------------------------------------------------------------------------------------- chains
class Chain:
    """4 -> 8 -> relu -> 8 -> 5 channels, three taps and step 2 in both layers, TGCNCheb_H with its per-vertex bias, one state per layer"""

    def __init__(self):
        import tgcn_amd
        n, H, K = N_VERT, 3, K_TERMS
        rng = np.random.default_rng(21)
        row, col, val = _random_graph(n, 6, rng, hubs=((2, n - 1),))
        op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val * 0.4))
        torch.manual_seed(21)
        self.l1, self.l2 = tgcn_amd.TGCNCheb_H(op, 4, 8, K, H).cuda(), tgcn_amd.TGCNCheb_H(op, 8, 5, K, H).cuda()

    def whole(self, x):
        with torch.no_grad():
            h = torch.relu(self.l1.forward_series(x, as_series=True, padding="causal", stride=2))
            return self.l2.forward_series(h, as_series=True, padding="causal", stride=2)

    def step(self, capturable):
        def step(chunk, states):
            s1, s2 = states or (None, None)
            o1, s1 = self.l1.forward_stream(chunk, state=s1, capturable=capturable, stride=2)
            if o1.shape[2] == 0:            # no window of the first layer ends inside the chunk: the second layer has nothing to read
                return None, (s1, s2)
            o2, s2 = self.l2.forward_stream(torch.relu(o1), state=s2, capturable=capturable, stride=2)
            return o2, (s1, s2)
        return step

    def eager(self, x, chunks, states=None):
        outs, t, step = [], 0, self.step(False)
        with torch.no_grad():
            for Tc in chunks:
                o, states = step(x[:, :, t:t + Tc], states)
                outs.append(o)
                t += Tc
        return outs, states


@gpu
def test_two_layer_chain_equals_the_chain_through_forward_series(gpu_device):
    require_entries()
    ch = Chain()
    chunks = (1, 5, 3, 1, 40, 2, 33, 1, 1, 4)
    T = sum(chunks)
    x = torch.randn(S_REC, N_VERT, T, 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    whole = ch.whole(x)
    outs, (s1, s2) = ch.eager(x, chunks)
    assert any(o is None for o in outs) and any(o is not None and o.shape[2] == 0 for o in outs)       # both layers meet a chunk without a window
    got = torch.cat([o for o in outs if o is not None], dim=2)
    n1 = (T - 1) // 2 + 1
    assert tuple(got.shape) == tuple(whole.shape) == (S_REC, N_VERT, (n1 - 1) // 2 + 1, 5) and (s1.seen, s2.seen, s1.C, s2.C) == (T, n1, 2, 2)
    print("two-layer chain of steps: rel err %.2e, %d of %d elements differ" % (rel_err(got.cpu().numpy(), whole.cpu().numpy()),
                                                                               int((got != whole).sum()), got.numel()))
    assert torch.equal(got, whole)
    # another recording on the same states
    rings = (s1.ring.clone(), s2.ring.clone())
    for st in (s1, s2):
        assert st.reset() is st and (st.head, st.seen) == (0, 0) and not st.ring.any()
    again, (t1, t2) = ch.eager(x, chunks, (s1, s2))
    assert t1 is s1 and t2 is s2 and torch.equal(torch.cat([o for o in again if o is not None], dim=2), got)
    assert torch.equal(s1.ring, rings[0]) and torch.equal(s2.ring, rings[1])


@gpu
def test_a_captured_chain_of_steps_replays_the_recording(gpu_device):
    """capturable states take chunks of whole steps: Tc = 4 gives 2 rows to the second layer and 1 row out, on every replay"""
    import tgcn_amd
    require_entries()
    ch = Chain()
    TC, T = 4, 24
    x = torch.randn(S_REC, N_VERT, T, 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    chunks = [x[:, :, t:t + TC].contiguous() for t in range(0, T, TC)]
    eager, states = ch.eager(x, (TC,) * (T // TC))
    gs = tgcn_amd.GraphedStream(ch.step(True), chunks[0])
    s1, s2 = gs.states
    assert s1.capturable and s2.capturable and (s1.stride, s2.stride, s1.seen, s2.seen) == (2, 2, 0, 0)
    first = []
    for i, c in enumerate(chunks):
        out = gs(c)
        assert tuple(out.shape) == (S_REC, N_VERT, 1, 5) and torch.equal(out, eager[i]), i
        first.append(out.clone())
    assert (s1.seen, s2.seen, s1.head, s2.head) == (T, T // 2, T % 2, (T // 2) % 2)
    assert torch.equal(s1.ring, states[0].ring) and torch.equal(s2.ring, states[1].ring)
    assert torch.equal(torch.cat(first, dim=2), ch.whole(x))
    assert gs.reset() is gs and (s1.seen, s2.seen) == (0, 0) and not s1.ring.any() and not s2.ring.any()
    for i, c in enumerate(chunks):
        assert torch.equal(gs(c), first[i]), i
