"""Streaming state with a window step and bfloat16 parameters: the chunk lists of tests/test_series_stream_stride.py through the bf16 layers
(bf16 chunk, ring, stack and output, fp32 sums) by the two rules of tests/test_series_stream_bf16.py on the WHOLE series --

  * within EMUL_ULPS bf16 ulps of the tensor's largest value of the numpy emulation that rounds at the rounding points of DESIGN.md 3.10
    "bf16".  The emulation rounds per element and window j of the causal series at step s is window j*s at step 1, so the reference is
    every s-th row of that file's step-1 references;
  * against the fp64 oracle within TWICE the emulation's own error, computed per case on the CPU.

f = 8 (the 16-byte staging) and f = 3 (the narrow one), both classes, with a bias and without, on a plain and on a degree-reordered operand.
Then the C ABI: the bf16 _stream_strided entry is bit-identical to the rows of the _conv_bf16 entry on the whole stack -- also with stack
rows padded to a leading dimension and ring rows padded -- and at stride 1 it is the bf16 stream entry."""
import numpy as np
import pytest
import torch

from tgcn_amd import functional as F
from conftest import rel_err
from test_series_dilation import CLASSES, N_VERT, S_REC
from test_series_stream_bf16 import ULP_BOUND, Streamer, references
from test_series_stream_stride import LISTS, NO_OVERLAP, WRAP, _id, require_entries, step_one_equivalence, strided_entry_bit_identity, windows_of

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]
BF = torch.bfloat16


def shape_of(case, f, g):
    """make_case's (T, H, d, f, g, left, right) of a chunk list: the whole series at step 1 with the causal padding"""
    H, s, chunks = case
    return (sum(chunks), H, 1, f, g, H - 1, 0)


def every(ref, T, s):
    """the windows j*s of a window-major step-1 reference (S*T, n, g) -> (S*nwin, n, g)"""
    return np.ascontiguousarray(ref.reshape(S_REC, T, N_VERT, -1)[:, ::s]).reshape(-1, N_VERT, ref.shape[-1])


class StrideStreamer(Streamer):
    def feed(self, chunks, kind, bias, s):
        """the whole series chunk by chunk -> the non-empty outputs concatenated along time, window-major (S*nwin, n, g)"""
        state, outs, t = None, [], 0
        with torch.no_grad():
            for Tc in chunks:
                chunk = self.series[:, :, t:t + Tc]
                m, off = windows_of(t, Tc, s)
                if kind is None and bias:
                    out, state = self.m.forward_stream(chunk, *self.extra, state=state, stride=s)
                else:
                    if kind not in self.ops:
                        self.ops[kind] = self.op.reordered(kind)
                    out, state = F.cheb_time_stream(self.ops[kind], chunk, *self.fargs(bias), state, stride=s)
                assert out.dtype == BF and tuple(out.shape) == (S_REC, N_VERT, m, out.shape[-1]) and out.is_contiguous()
                assert state.dtype == BF and (state.ring is None or state.ring.dtype == BF)
                t += Tc
                assert state.seen == t and state.head == (t % state.C if state.C else 0) and state.stride == s
                if m:
                    outs.append(out)
        out = torch.cat(outs, dim=2)
        return out.permute(0, 2, 1, 3).reshape(S_REC * out.shape[2], N_VERT, -1)


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("f", [8, 3])
@pytest.mark.parametrize("case", LISTS, ids=_id)
def test_strided_bf16_stream_vs_oracle_and_emulation(case, f, cls, gpu_device):
    require_entries()
    g = 8
    H, s, chunks = case
    T = sum(chunks)
    shape = shape_of(case, f, g)
    st = StrideStreamer(cls, shape, gpu_device)
    for kind in (None, "degree"):
        for bias in (True, False):
            ref, emu = (every(a, T, s) for a in references(cls, shape, bias))
            gv = st.feed(chunks, kind, bias, s).double().cpu().numpy()
            assert gv.shape == emu.shape
            tol = 2 * rel_err(emu, ref)                        # twice the emulation's own error against fp64
            d_emu, e64 = float(np.abs(gv - emu).max() / np.abs(emu).max()), rel_err(gv, ref)
            print(cls, (H, s, chunks, f, g), kind, "bias" if bias else "no bias", "vs emulation %.2e (bound %.2e)" % (d_emu, ULP_BOUND),
                  "vs fp64 %.2e (bound %.2e)" % (e64, tol))
            assert d_emu <= ULP_BOUND, (kind, bias, d_emu)
            assert e64 <= tol, (kind, bias, e64, tol)


@gpu
@pytest.mark.parametrize("f", [8, 3], ids=["vec8", "narrow"])
@pytest.mark.parametrize("case", LISTS, ids=_id)
def test_bf16_strided_entry_is_the_conv_entry_on_the_whole_stack(case, f, gpu_device):
    strided_entry_bit_identity(BF, f, case)


@gpu
@pytest.mark.parametrize("ring_pad,stack_pad", [(0, 8), (8, 8), (1, 0), (0, 5)], ids=["stack_ld-padded", "both-padded", "odd-ring", "odd-stack_ld"])
@pytest.mark.parametrize("case", [WRAP, NO_OVERLAP], ids=_id)
def test_bf16_strided_entry_with_padded_rows(case, ring_pad, stack_pad, gpu_device):
    """f = 8: leading dimensions that keep the 16-byte form (multiples of 8) and that rule it out (narrow staging, element-wise ring update)"""
    strided_entry_bit_identity(BF, 8, case, ring_pad=ring_pad, stack_pad=stack_pad)


@gpu
@pytest.mark.parametrize("f", [8, 3], ids=["vec8", "narrow"])
def test_bf16_strided_entry_at_step_one_is_the_stream_entry(f, gpu_device):
    step_one_equivalence(BF, f)
