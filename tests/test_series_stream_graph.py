"""Streaming state with the ring's position on the device (capturable=True) and a streaming step captured into a hipGraph (GraphedStream).

  1. through the C ABI: the _pos entries against the host-head entries on twin rings over a list of chunks -- outputs and rings torch.equal
     after every call, pos equal to the host's (head, seen);
  2. the defensive read: a pos[0] outside [0, C) is read as head 0 (valid memory only: the kernels clamp before they address the ring);
  3. the modules, eager: capturable=True chunk by chunk is torch.equal to capturable=False, both classes, with a bias and without, plain and
     degree-reordered operands, fp32 and bf16;
  4. captured: a two-layer chain through GraphedStream, every replay torch.equal to eager forward_stream on twin host-head states, the whole
     within tests/test_series_dilation.py's 1e-5 of the fp64 oracle on the materialised causal windows of the whole series (bf16: the
     8-ulp / twice-own-error rule of tests/test_series_stream_bf16.py), a second pass after reset() torch.equal to the first; the same with
     a one-tap first layer;
  5. a host-head state inside torch.cuda.graph raises TgcnError and leaves its ring as it was."""
import numpy as np
import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F
from conftest import rel_err
from oracle import cheb_oracle as O
from test_bf16_layers import EMUL_ULPS, bf
from test_series_bf16 import _graph
from test_series_channels import TOL
from test_series_dilation import CLASSES, K_TERMS, N_VERT, S_REC, Setup, windows_dilated
from test_series_dilation_bf16 import series_emulate, series_fp64
from test_series_stream import edge_index_of

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]
BF = torch.bfloat16
ULP_BOUND = EMUL_ULPS * 2.0 ** -8

ABI_CHUNKS = (1, 1, 3, 8, 9, 5)
ABI_SHAPES = [(3, 1), (3, 4), (5, 3)]       # (H, dilation): C = 2, 8, 12


def test_the_abi_chunk_list_hits_what_it_is_here_for():
    seen = set()
    for H, d in ABI_SHAPES:
        Cr = (H - 1) * d
        heads = [int(h) % Cr for h in np.cumsum((0,) + ABI_CHUNKS[:-1])]
        assert any(h != 0 for h in heads)
        seen |= {"below" for t in ABI_CHUNKS if t < Cr} | {"equal" for t in ABI_CHUNKS if t == Cr} | {"above" for t in ABI_CHUNKS if t > Cr}
        if Cr > 2:
            assert any(0 < t < Cr and h + t > Cr for t, h in zip(ABI_CHUNKS, heads))      # a short chunk that wraps round the ring's end
    assert seen == {"below", "equal", "above"}
    assert any(t < d for t in ABI_CHUNKS for H, d in ABI_SHAPES[2:])                   # nwin < dilation: phases without a window


class Abi:
    """one weight and bias; host(...) and pos(...) launch the two entries of a dtype on a chunk's stack"""

    def __init__(self, dt, f, H, d):
        self.dt, self.f, self.H, self.d, self.bf16 = dt, f, H, d, dt == BF
        self.n, self.S, self.N, self.K = N_VERT, S_REC, 24, K_TERMS
        self.Cr = (H - 1) * d
        self.gen = torch.Generator(device="cuda").manual_seed(f + 10 * d + H)
        self.W = self.rand(self.K, H * f, self.N)
        self.bias = self.rand(self.N)
        self.L = _lib.lib()

    def rand(self, *shape):
        return torch.randn(shape, device="cuda", generator=self.gen).to(self.dt)

    def ring(self):
        return torch.zeros((self.K, self.S, self.n, self.Cr * self.f), device="cuda", dtype=self.dt)

    def call(self, stack, ring, where):
        """where: the host's head (int) or the pos tensor"""
        Tc = stack.shape[3]
        out = torch.full((self.S, self.n, Tc, self.N), float("nan"), device="cuda", dtype=self.dt)
        head = (_lib.stream_ptr(), self.S, self.n, Tc, self.f, self.H, self.N, self.K, _lib.ptr(stack))
        on_device = isinstance(where, torch.Tensor)
        tail = (_lib.ptr(out), _lib.ptr(ring), ring.shape[-1], _lib.ptr(where) if on_device else where, self.d)
        if self.bf16:
            entry = self.L.tgcn_cheb_project_series_stream_pos_bf16 if on_device else self.L.tgcn_cheb_project_series_stream_bf16
            _lib.check(entry(*head, Tc * self.f, _lib.ptr(self.W), _lib.ptr(self.bias), _lib.DTYPE_BF16, 1, *tail))
        else:
            entry = self.L.tgcn_cheb_project_series_stream_pos_f32 if on_device else self.L.tgcn_cheb_project_series_stream_f32
            _lib.check(entry(*head, _lib.ptr(self.W), _lib.ptr(self.bias), 1, *tail))
        return out


ABI_WIDTHS = [(torch.float32, 4), (torch.float32, 3), (BF, 8), (BF, 5)]


@gpu
@pytest.mark.parametrize("H,d", ABI_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("dt,f", ABI_WIDTHS, ids=["fp32-f4", "fp32-f3", "bf16-f8", "bf16-f5"])
def test_pos_entries_equal_the_host_head_entries_on_twin_rings(dt, f, H, d, gpu_device):
    a = Abi(dt, f, H, d)
    ring_h, ring_p = a.ring(), a.ring()
    pos = torch.zeros(2, dtype=torch.int64, device="cuda")
    head = seen = 0
    for Tc in ABI_CHUNKS:
        stack = a.rand(a.K, a.S, a.n, Tc, f)
        out_h = a.call(stack, ring_h, head)
        out_p = a.call(stack, ring_p, pos)
        head, seen = (head + Tc) % a.Cr, seen + Tc
        assert not torch.isnan(out_h).any() and torch.equal(out_h, out_p), (Tc, head)
        assert torch.equal(ring_h, ring_p), (Tc, head)
        assert pos.tolist() == [head, seen]
    assert ring_h.any() and head != 0


@gpu
@pytest.mark.parametrize("dt,f", ABI_WIDTHS, ids=["fp32-f4", "fp32-f3", "bf16-f8", "bf16-f5"])
def test_a_position_outside_the_ring_is_read_as_head_zero(dt, f, gpu_device):
    """The kernels use pos[0] only if 0 <= pos[0] < C and take 0 otherwise (windows.h: series_ring_head), before any ring address is formed:
    with pos[0] = C, -1 and 2^40 the call returns what the host-head entry returns at head = 0, the ring update writes the slots of head 0,
    and the advance continues from 0.  Every access stays inside the ring: nothing here provokes a fault."""
    H, d = 3, 4
    a = Abi(dt, f, H, d)
    past = a.rand(a.K, a.S, a.n, a.Cr * f)               # a ring that is not zero, so that a wrong head would show
    for Tc in (3, 9):
        stack = a.rand(a.K, a.S, a.n, Tc, f)
        ring_h = past.clone()
        want = a.call(stack, ring_h, 0)
        for bad in (a.Cr, -1, 2 ** 40):
            ring_p = past.clone()
            pos = torch.tensor([bad, 7], dtype=torch.int64, device="cuda")
            got = a.call(stack, ring_p, pos)
            assert torch.equal(got, want) and torch.equal(ring_p, ring_h), (Tc, bad)
            assert pos.tolist() == [Tc % a.Cr, 7 + Tc], (Tc, bad)


@gpu
def test_the_advance_alone_counts_seen_and_refusals_launch_nothing(gpu_device):
    L = _lib.lib()
    pos = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    _lib.check(L.tgcn_series_stream_advance(_lib.stream_ptr(), _lib.ptr(pos), 5, 0))          # a one-tap layer: no ring, head stays 0
    assert pos.tolist() == [0, 9]
    _lib.check(L.tgcn_series_stream_advance(_lib.stream_ptr(), _lib.ptr(pos), 5, 3))
    assert pos.tolist() == [2, 14]
    a = Abi(torch.float32, 4, 3, 2)
    stack, ring = a.rand(a.K, a.S, a.n, 6, 4), torch.full((a.K, a.S, a.n, a.Cr * 4), float("nan"), device="cuda")
    out = torch.full((a.S, a.n, 6, a.N), float("nan"), device="cuda")

    def call(Tc=6, H=3, ring_ld=a.Cr * 4, where=pos, dil=2):
        return L.tgcn_cheb_project_series_stream_pos_f32(_lib.stream_ptr(), a.S, a.n, Tc, 4, H, a.N, a.K, _lib.ptr(stack), _lib.ptr(a.W), None, 0,
                                                         _lib.ptr(out), _lib.ptr(ring), ring_ld, _lib.ptr(where), dil)
    assert call(where=None) == -1 and call(Tc=0) == -1 and call(dil=0) == -1 and call(ring_ld=a.Cr * 4 - 1) == -1 and call(H=1, ring_ld=0) == -1
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(ring).all() and pos.tolist() == [2, 14]


# ------------------------------------------------------------------------------------------------------------- the modules, eager
@gpu
@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cls", CLASSES)
def test_capturable_states_give_what_host_head_states_give(cls, dt, gpu_device):
    import copy
    H, d, chunks = 3, 2, (1, 3, 5, 4, 2, 9)
    f, g = (8 if dt == BF else 4), 8
    su = Setup(cls, f, g, H, seed=17)
    layer = copy.deepcopy(su.layer).to(dt)
    extra = () if cls == "TGCNCheb_H" else (edge_index_of(17), None)
    series = torch.randn(S_REC, N_VERT, sum(chunks), f, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8)).to(dt)
    ops = {None: layer._operand(series.device) if cls == "TGCNCheb_H" else layer._operand(series, extra[0], None)}
    ops["degree"] = ops[None].reordered("degree")

    def step(chunk, state, kind, bias, capturable):
        if kind is None and bias:
            return layer.forward_stream(chunk, *extra, state=state, dilation=d, capturable=capturable)
        return F.cheb_time_stream(ops[kind], chunk, layer.weight, layer.bias.reshape(-1) if bias else None, su.bias_kind if bias else F.BIAS_NONE,
                                  su.fmode, state, d, capturable=capturable)

    with torch.no_grad():
        for kind in (None, "degree"):
            for bias in (True, False):
                host = dev = None
                t = 0
                for Tc in chunks:
                    chunk = series[:, :, t:t + Tc]
                    o_h, host = step(chunk, host, kind, bias, False)
                    o_d, dev = step(chunk, dev, kind, bias, dev is None)        # afterwards the state's kind rules
                    t += Tc
                    assert o_d.dtype == dt and torch.equal(o_h, o_d), (kind, bias, t)
                assert dev.capturable and not host.capturable and torch.equal(host.ring, dev.ring)
                assert (dev.head, dev.seen) == (host.head, host.seen) == (t % dev.C, t)
                assert dev.reset() is dev and (dev.head, dev.seen) == (0, 0) and not dev.ring.any()


# --------------------------------------------------------------------------------------------------------------------- captured
TC, NCHUNK = 3, 7


class Chain:
    """1 -> 8 -> relu -> 8 channels, H1 taps at dilation 1 then 3 taps at dilation 2, TGCNCheb_H with its per-vertex bias, on one graph"""

    def __init__(self, dt, H1):
        self.dt, self.H1 = dt, H1
        self.L = _graph(N_VERT, 31)
        torch.manual_seed(31 + H1)
        dense = torch.as_tensor(self.L.toarray(), dtype=torch.float32)
        self.l1, self.l2 = tgcn_amd.TGCNCheb_H(dense, 1, 8, K_TERMS, H1), tgcn_amd.TGCNCheb_H(dense, 8, 8, K_TERMS, 3)
        with torch.no_grad():
            for m in (self.l1, self.l2):
                m.bias.uniform_(-0.5, 0.5)
        self.l1, self.l2 = self.l1.to(dt).cuda(), self.l2.to(dt).cuda()
        self.x = np.random.default_rng(5).standard_normal((S_REC, N_VERT, TC * NCHUNK, 1)).astype(np.float32)

    def step(self, capturable):
        def step(chunk, states):
            s1, s2 = states or (None, None)
            o1, s1 = self.l1.forward_stream(chunk, state=s1, capturable=capturable)
            o2, s2 = self.l2.forward_stream(torch.relu(o1), state=s2, dilation=2, capturable=capturable)
            return o2, (s1, s2)
        return step

    def references(self):
        """(fp64 oracle, emulation or None) of the chain on the whole series, as series (S, n, T, 8)"""
        S, n, T = S_REC, N_VERT, TC * NCHUNK
        geo = ((1, self.H1 - 1, 0), (2, 4, 0))           # (dilation, left, right) of the two causal layers
        zeros = np.zeros((S * T, n, 8))

        def to_series(y):
            return y.reshape(S, T, n, -1).transpose(0, 2, 1, 3)
        if self.dt != BF:
            h = self.x.astype(np.float64)
            for m, (d, left, _) in zip((self.l1, self.l2), geo):
                xw = windows_dilated(h, m.weight.shape[1], d, left, 0)
                h = to_series(O.tgcn_cheb_h_forward(self.L, xw, m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()))
                if m is self.l1:
                    h = np.maximum(h, 0)
            return h, None
        ref, emu = bf(self.x), bf(self.x)
        for m, g3 in zip((self.l1, self.l2), geo):
            W, b = m.weight.detach().double().cpu().numpy(), m.bias.detach().double().cpu().numpy()
            ref = to_series(series_fp64(self.L, np.ascontiguousarray(ref), W, b, zeros, "power", g3)[0])
            emu = to_series(series_emulate(self.L, np.ascontiguousarray(emu), W, b, zeros, "power", g3)[0])
            if m is self.l1:
                ref, emu = np.maximum(ref, 0), np.maximum(emu, 0)
        return ref, emu


@gpu
@pytest.mark.parametrize("H1", [3, 1], ids=["H3-then-H3", "one-tap-then-H3"])
@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
def test_a_captured_chain_replays_the_recording(dt, H1, gpu_device):
    ch = Chain(dt, H1)
    x = torch.as_tensor(ch.x, device="cuda").to(dt)
    chunks = [x[:, :, i * TC:(i + 1) * TC].contiguous() for i in range(NCHUNK)]
    eager, states = [], None
    with torch.no_grad():
        for c in chunks:
            o, states = ch.step(False)(c, states)
            eager.append(o)
    gs = tgcn_amd.GraphedStream(ch.step(True), chunks[0])
    s1, s2 = gs.states
    assert (s1.C, s2.C) == ((H1 - 1), 4) and s1.capturable and s2.capturable and (s1.seen, s2.seen, s1.head, s2.head) == (0, 0, 0, 0)
    heads = set()
    first = []
    for i, c in enumerate(chunks):
        out = gs(c)
        assert torch.equal(out, eager[i]), i          # the second replay is where a captured host head goes stale
        first.append(out.clone())
        heads.add(s2.head)
    assert heads == {0, 1, 2, 3}                       # every slot, and round the ring's end
    assert (s1.seen, s2.seen) == (TC * NCHUNK, TC * NCHUNK) == (21, 21) and s2.head == 21 % 4 and s1.head == (21 % 2 if H1 > 1 else 0)
    assert torch.equal(s2.ring, states[1].ring) and (H1 == 1 or torch.equal(s1.ring, states[0].ring))
    got = torch.cat(first, dim=2).double().cpu().numpy()
    ref, emu = ch.references()
    if dt == BF:
        tol = 2 * rel_err(emu, ref)
        d_emu, e64 = float(np.abs(got - emu).max() / np.abs(emu).max()), rel_err(got, ref)
        print("captured chain bf16 H1=%d: vs emulation %.2e (bound %.2e), vs fp64 %.2e (bound %.2e)" % (H1, d_emu, ULP_BOUND, e64, tol))
        assert d_emu <= ULP_BOUND and e64 <= tol, (d_emu, e64, tol)
    else:
        e = rel_err(got, ref)
        print("captured chain fp32 H1=%d: %.2e (bound %.0e)" % (H1, e, TOL))
        assert e <= TOL, e
    # another recording: reset, the same chunks, the same numbers
    assert gs.reset() is gs and (s1.seen, s2.seen, s2.head) == (0, 0, 0) and not s2.ring.any()
    for i, c in enumerate(chunks):
        assert torch.equal(gs(c), first[i]), i
    # one graph per chunk shape and dtype
    with pytest.raises(_lib.TgcnError, match="one graph per chunk shape"):
        gs(x[:, :, :TC + 1].contiguous())
    with pytest.raises(_lib.TgcnError, match="one graph per chunk shape"):
        gs(chunks[0].to(torch.float64))
    assert s2.seen == 21


@gpu
def test_graphed_stream_refuses_a_chain_of_host_head_states_before_capture(gpu_device):
    ch = Chain(torch.float32, 3)
    chunk = torch.as_tensor(ch.x[:, :, :TC], device="cuda")
    with pytest.raises(_lib.TgcnError, match="capturable=True"):
        tgcn_amd.GraphedStream(ch.step(False), chunk)
    assert not torch.cuda.is_current_stream_capturing()
    with pytest.raises(_lib.TgcnError, match="warmup"):
        tgcn_amd.GraphedStream(ch.step(True), chunk, warmup=0)
    with pytest.raises(_lib.TgcnError, match="returns"):
        tgcn_amd.GraphedStream(lambda c, s: (c, None), chunk)


@gpu
def test_a_host_head_state_is_refused_while_the_stream_is_capturing(gpu_device):
    ch = Chain(torch.float32, 3)
    chunk = torch.as_tensor(ch.x[:, :, :TC], device="cuda")
    with torch.no_grad():
        _, state = ch.l1.forward_stream(chunk)                     # eager: builds the operand and a host-head state with a ring
        _, state = ch.l1.forward_stream(chunk, state=state)
    ring, where = state.ring.clone(), (state.head, state.seen)
    assert ring.any()
    probe = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        probe.add_(1)                                              # the captured graph is not empty
        with pytest.raises(_lib.TgcnError, match="capturable=True"):
            ch.l1.forward_stream(chunk, state=state)
        with pytest.raises(_lib.TgcnError, match="capturable=True"):
            ch.l1.forward_stream(chunk)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(state.ring, ring) and (state.head, state.seen) == where and probe.tolist() == [1.0] * 4
    with torch.no_grad():                                          # eager calls go on as before
        _, state = ch.l1.forward_stream(chunk, state=state)
    assert state.seen == where[1] + TC
