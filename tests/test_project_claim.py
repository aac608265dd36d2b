"""project_x3_claim_kernel (csrc/project.h): the co-schedulable form of the streaming bf16x3 projection -- 256-thread workgroups on a capped
grid whose waves claim their 16-row tiles from a counter in device memory -- against project_x3_stream_kernel (1024-thread workgroups, tiles
dealt round robin), through tgcn_cheb_project_stream_f32.  A tile's arithmetic does not depend on the wave that computes it, so the two must
agree BIT FOR BIT: on row counts around one tile and one workgroup, on a capped grid whose waves claim several tiles while others find
none, for 1 and 5 terms, 1 ... 3 samples per tile (odd unit counts hand the prefetched unit over between the two register buffers), rows of
32 and 64 floats, every column-tile instantiation (N = 16 / 32 / 64), with and without a row map, and the three bias kinds."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 63, 64, 65)
CAP = 2
CAPPED_ROWS = 64 * CAP + 1          # 9 tiles for the 8 waves of two workgroups


def _project(L, _lib, terms, term_bs, W, bias, bias_kind, n_vertices, rowmap, nbatch, out, counter):
    T, Kc, N = W.shape
    M = terms[-1].shape[1] if rowmap is None else int(rowmap.numel())
    a = (C.c_void_p * T)(*[t.data_ptr() for t in terms])
    lda = (C.c_int64 * T)(*[Kc] * T)
    a_bs = (C.c_int64 * T)(*term_bs)
    _lib.check(L.tgcn_cheb_project_stream_f32(_lib.stream_ptr(), M, Kc, N, T, a, lda, _lib.ptr(W), _lib.ptr(bias), bias_kind, n_vertices,
                                              _lib.ptr(rowmap), 1 if rowmap is not None else 0, nbatch, a_bs, n_vertices * N, _lib.ptr(out), N,
                                              _lib.ptr(counter)))


@pytest.mark.parametrize("Kc", [32, 64])
@pytest.mark.parametrize("N", [16, 32, 64])
@pytest.mark.parametrize("T", [1, 5])
def test_claiming_form_is_bitwise_the_static_form(Kc, N, T, gpu_device):
    from tgcn_amd import _lib
    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(Kc * 1000 + N * 10 + T)
    NB, MMAX = 3, CAPPED_ROWS
    nv = 2 * MMAX + 5
    x = torch.randn((NB, nv, Kc), device="cuda", generator=g)
    W = torch.randn((T, Kc, N), device="cuda", generator=g) / (T * Kc) ** 0.5
    bias_c, bias_v = torch.randn(N, device="cuda", generator=g), torch.randn((nv, N), device="cuda", generator=g)
    counter = torch.full((1,), 12345, dtype=torch.int32, device="cuda")          # the call zeroes it
    checked = 0
    for M in ROWS + (CAPPED_ROWS,):
        _lib.check(L.tgcn_set_tuning(b"x3_stream_cap", CAP if M == CAPPED_ROWS else 0))
        rest = [torch.randn((NB, M, Kc), device="cuda", generator=g) for _ in range(T - 1)]
        perm = torch.randperm(nv, device="cuda", generator=g)[:M].sort().values.to(torch.int32)
        for mapped in (True, False):
            # mapped: term 0 and the output live in the caller's nv rows; unmapped: every operand has M rows per sample
            rows_per_sample = nv if mapped else M
            first = x if mapped else x[:, :M].contiguous()
            terms = [first] + rest
            term_bs = [rows_per_sample * Kc] + [M * Kc] * (T - 1)
            for nbatch in (1, 2, 3):
                for bias_kind, bias in ((0, None), (1, bias_c), (2, bias_v[:rows_per_sample].contiguous())):
                    outs = []
                    for cnt in (None, counter):
                        out = torch.full((nbatch, rows_per_sample, N), float("nan"), device="cuda")
                        _project(L, _lib, terms, term_bs, W, bias, bias_kind, rows_per_sample, perm if mapped else None, nbatch, out, cnt)
                        outs.append(out)
                    written = outs[0][:, perm.long()] if mapped else outs[0]
                    assert not torch.isnan(written).any()
                    # bitwise, rows outside the map (still NaN in both) included
                    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), (M, mapped, nbatch, bias_kind)
                    checked += 1
        if M == CAPPED_ROWS:
            # every wave that started claimed up to two tiles beyond the last one it found; nothing else moves the counter
            tiles = (M + 15) // 16
            assert tiles <= int(counter.item()) <= tiles + 2 * 4 * CAP
    assert checked == 8 * 2 * 3 * 3


def test_stream_entry_refuses_shapes_without_the_kernel(gpu_device):
    from tgcn_amd import _lib
    L = _lib.lib()
    x, W, out = torch.randn(64, 48, device="cuda"), torch.randn(1, 48, 64, device="cuda"), torch.empty(64, 64, device="cuda")
    a, lda, bs = (C.c_void_p * 1)(x.data_ptr()), (C.c_int64 * 1)(48), (C.c_int64 * 1)(0)
    rc = L.tgcn_cheb_project_stream_f32(_lib.stream_ptr(), 64, 48, 64, 1, a, lda, _lib.ptr(W), None, 0, 64, None, 0, 1, bs, 64 * 64, _lib.ptr(out), 64, None)
    assert rc != 0 and b"streaming" in L.tgcn_last_error()
