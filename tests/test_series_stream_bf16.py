"""Streaming state with bfloat16 parameters: the chunked causal layer (bf16 chunk, ring, stack and output, fp32 sums) by the method and the
two bounds of tests/test_series_dilation_bf16.py, on the WHOLE series --

  * within EMUL_ULPS bf16 ulps of the tensor's largest value of the numpy emulation that rounds at the rounding points of DESIGN.md 3.10
    "bf16" (it rounds per element, so cutting the series into chunks does not change it);
  * against the fp64 oracle on the materialised causal dilated windows within TWICE the emulation's own error, computed per case on the CPU.

The first two chunk lists of tests/test_series_stream.py with f in {8, 16} (the 16-byte staging) and f = 3 (the narrow one); both classes,
with a bias and without, on a plain and on a degree-reordered operand.  Then the C ABI: the bf16 stream entry is bit-identical to the
_dilated_bf16 entry on the whole stack, with ring rows of exactly C*f elements and padded to a multiple of 8."""
import copy
import functools

import numpy as np
import pytest
import torch

from tgcn_amd import functional as F
from conftest import rel_err
from test_bf16_layers import EMUL_ULPS, bf
from test_series_dilation import CLASSES, N_VERT, S_REC
from test_series_dilation_bf16 import make_case, series_emulate, series_fp64
from test_series_stream import UNDILATED, WRAP, stream_entry_bit_identity

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]
BF = torch.bfloat16
ULP_BOUND = EMUL_ULPS * 2.0 ** -8


def shape_of(case, f, g):
    """make_case's (T, H, d, f, g, left, right) of a chunk list: the whole series with the causal padding"""
    H, d, chunks = case
    return (sum(chunks), H, d, f, g, (H - 1) * d, 0)


@functools.lru_cache(maxsize=None)
def references(cls, shape, bias):
    """(fp64 reference, emulation) of the whole series' output, window-major, computed once and left unchanged"""
    m, ei, L, mode, series, go = make_case(cls, shape)
    T, H, d, f, g, left, right = shape
    W = m.weight.detach().double().numpy()
    b = m.bias.detach().double().numpy() if bias else None
    xs, gg = bf(series), bf(go)
    return series_fp64(L, xs, W, b, gg, mode, (d, left, right))[0], series_emulate(L, xs, W, b, gg, mode, (d, left, right))[0]


class Streamer:
    def __init__(self, cls, shape, dev):
        m, ei, L, mode, series, go = make_case(cls, shape)
        self.m = m = copy.deepcopy(m).to(dev)
        self.d = shape[2]
        self.series = torch.as_tensor(series, device=dev).to(BF)
        if cls == "TGCNCheb_H":
            self.op, self.extra = m._operand(dev), ()
            self.fargs = lambda bias: (m.weight, m.bias.reshape(-1) if bias else None, F.BIAS_VERTEX_CHANNEL if bias else F.BIAS_NONE, F.MODE_POWER)
        else:
            eid = ei.to(dev)
            self.op, self.extra = m._operand(torch.empty(1, N_VERT, 1, device=dev), eid, None), (eid, None)
            self.fargs = lambda bias: (m.weight, m.bias if bias else None, F.BIAS_CHANNEL if bias else F.BIAS_NONE, F.MODE_CHEBYSHEV)
        self.ops = {None: self.op}

    def feed(self, chunks, kind, bias):
        """the whole series chunk by chunk -> the outputs concatenated along time, window-major (S*T, n, g)"""
        state, outs, t = None, [], 0
        with torch.no_grad():
            for Tc in chunks:
                chunk = self.series[:, :, t:t + Tc]
                if kind is None and bias:
                    out, state = self.m.forward_stream(chunk, *self.extra, state=state, dilation=self.d)
                else:
                    if kind not in self.ops:
                        self.ops[kind] = self.op.reordered(kind)
                    out, state = F.cheb_time_stream(self.ops[kind], chunk, *self.fargs(bias), state, self.d)
                assert out.dtype == BF and tuple(out.shape) == (S_REC, N_VERT, Tc, out.shape[-1]) and out.is_contiguous()
                assert state.dtype == BF and (state.ring is None or state.ring.dtype == BF)
                outs.append(out)
                t += Tc
        out = torch.cat(outs, dim=2)
        return out.permute(0, 2, 1, 3).reshape(S_REC * t, N_VERT, -1)


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("g", [5, 40])
@pytest.mark.parametrize("f", [8, 16, 3])
@pytest.mark.parametrize("case", [WRAP, UNDILATED], ids=lambda c: "H%d_d%d" % c[:2])
def test_chunked_bf16_stream_vs_oracle_and_emulation(case, f, g, cls, gpu_device):
    shape = shape_of(case, f, g)
    st = Streamer(cls, shape, gpu_device)
    for kind in (None, "degree"):
        for bias in (True, False):
            ref, emu = references(cls, shape, bias)
            gv = st.feed(case[2], kind, bias).double().cpu().numpy()
            tol = 2 * rel_err(emu, ref)                        # twice the emulation's own error against fp64
            d_emu, e64 = float(np.abs(gv - emu).max() / np.abs(emu).max()), rel_err(gv, ref)
            print(cls, shape, kind, "bias" if bias else "no bias", "vs emulation %.2e (bound %.2e)" % (d_emu, ULP_BOUND),
                  "vs fp64 %.2e (bound %.2e)" % (e64, tol))
            assert d_emu <= ULP_BOUND, (kind, bias, d_emu)
            assert e64 <= tol, (kind, bias, e64, tol)


@gpu
@pytest.mark.parametrize("pad_ring", [False, True], ids=["ring_ld=C*f", "ring_ld-padded"])
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("f", [8, 3], ids=["vec8", "narrow"])
def test_bf16_stream_entry_is_the_dilated_entry_on_the_whole_stack(f, d, pad_ring, gpu_device):
    stream_entry_bit_identity(BF, f, d, pad_ring)


@gpu
@pytest.mark.parametrize("d", [1, 3])
def test_bf16_stream_entry_with_a_ring_that_rules_out_16_byte_accesses(d, gpu_device):
    """f = 8 on ring rows of C*f + 1 elements: narrow staging and an element-wise ring update, bit-identical all the same"""
    stream_entry_bit_identity(BF, 8, d, odd_ring=True)
