"""The two weight-gradient entry points of libtgcn_hip.so against chunked fp64 numpy at the shapes where their reductions change form:
tgcn_cheb_wgrad_f32 (row blocks of wgrad_rows_per_block rows, at most 1024 partials, 32 terms per call) and tgcn_cheb_windows_backward_f32
(chunks of 16384 window rows, capped at 256, plus the input-gradient taps).  Each term is checked against its own largest element, so a
small term cannot hide behind a large one; the workspace is filled with NaN before every call and a second call must give the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cheb_oracle as O

pytestmark = pytest.mark.gpu
TOL_WGRAD = 1e-5
TOL_WINDOWS = 2e-5
ERR_INVALID, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -3, -4
HOST_CHUNK_FLOATS = 1 << 25           # rows moved to the host per chunk of the fp64 reference: (Kc + N) * rows <= 32 M floats


def _rows_per_block(M):
    """wgrad_rows_per_block in tgcn_hip.hip: at most 1024 row blocks of at least 64 rows, a multiple of 16."""
    rpb = max((M + 1023) // 1024, 64)
    return (rpb + 15) // 16 * 16


def _fill(kind, shape, gen, scale=1.0):
    x = torch.randn(shape, device="cuda", generator=gen)
    if kind == "relu":                # positive mean far above the spread: long same-sign accumulation chains
        x = 4.0 + 0.25 * x
    return x * scale if scale != 1.0 else x


def _wgrad_ref(terms, g):
    """dW[t] = terms[t]^T g in fp64 on the host, rows in chunks (A and G cast per chunk)."""
    M, Kc = terms[0].shape
    N = g.shape[1]
    ref = np.zeros((len(terms), Kc, N))
    step = max(1, HOST_CHUNK_FLOATS // (Kc + N))
    for m0 in range(0, M, step):
        gc = g[m0:m0 + step].double().cpu().numpy()
        for t, a in enumerate(terms):
            ref[t] += a[m0:m0 + step].double().cpu().numpy().T @ gc
    return ref


def _wgrad_raw(terms, g, ws):
    """tgcn_cheb_wgrad_f32 through ctypes on the caller's workspace -> (rc, dW)"""
    from tgcn_amd import _lib
    L = _lib.lib()
    M, Kc = terms[0].shape
    N = g.shape[1]
    nt = len(terms)
    dW = torch.full((nt, Kc, N), float("nan"), device="cuda")
    a = (C.c_void_p * nt)(*[t.data_ptr() for t in terms])
    lda = (C.c_int64 * nt)(*[t.stride(0) for t in terms])
    rc = L.tgcn_cheb_wgrad_f32(_lib.stream_ptr(), M, Kc, N, nt, a, lda, _lib.ptr(g), g.stride(0), _lib.ptr(dW), _lib.ptr(ws), ws.numel() * 4)
    torch.cuda.synchronize()
    return rc, dW


def _nan_workspace(nbytes):
    return torch.full(((max(nbytes, 16) + 3) // 4,), float("nan"), device="cuda")


def _make_terms(M, Kc, N, nt, kind, strided, seed):
    """nt (M, Kc) terms and G (M, N): contiguous, or views into wider rows (lda > Kc at an odd column offset, ldg > N)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    scales = np.logspace(-3, 3, nt) if kind == "scaled" else np.ones(nt)
    if strided:
        width = Kc + 3
        base = _fill(kind, (M, nt * width + 1), gen)
        terms = []
        for t in range(nt):
            view = base[:, 1 + t * width:1 + t * width + Kc]
            view.mul_(float(scales[t]))
            terms.append(view)
        gb = _fill(kind, (M, N + 5), gen)
        g = gb[:, 2:2 + N]
        assert all(t.stride(0) > Kc for t in terms) and g.stride(0) > N
    else:
        terms = [_fill(kind, (M, Kc), gen, float(scales[t])) for t in range(nt)]
        g = _fill(kind, (M, N), gen)
    return terms, g


def _assert_per_term(got, ref, tol, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    for t in range(ref.shape[0]):
        assert np.isfinite(got[t]).all(), (what, t)
        err = rel_err(got[t], ref[t])
        assert err <= tol, (what, t, err)


M_BIG = 4_200_017
WGRAD_CASES = [
    # M, Kc, N, nterms, data kind, strided
    (1, 1, 1, 1, "zero", False),
    (3, 17, 65, 5, "zero", True),
    (63, 15, 63, 6, "relu", False),
    (64, 16, 64, 32, "scaled", True),
    (65, 17, 129, 5, "zero", False),
    (65, 1, 1, 33, "scaled", False),
    (1000, 1201, 1, 1, "relu", False),
    (65536, 16, 64, 6, "relu", False),
    (65537, 15, 65, 5, "scaled", True),
    (65537, 1200, 32, 5, "zero", False),
    (90000, 1201, 33, 1, "zero", True),
    (M_BIG, 17, 65, 6, "zero", False),
    (M_BIG, 16, 64, 1, "relu", True),
    (M_BIG, 15, 63, 5, "scaled", True),
]


@pytest.mark.parametrize("M,Kc,N,nt,kind,strided", WGRAD_CASES)
def test_wgrad_entry_vs_fp64(M, Kc, N, nt, kind, strided, gpu_device):
    """tgcn_cheb_wgrad_f32 through F.cheb_wgrad and bare ctypes: every term against its own max, NaN workspace, the same bits twice."""
    from tgcn_amd import _lib
    from tgcn_amd import functional as F
    if M == M_BIG:
        rpb = _rows_per_block(M)
        assert M % rpb != 0 and (M + rpb - 1) // rpb > 1000          # a ragged last block, near the 1024-partial cap
    terms, g = _make_terms(M, Kc, N, nt, kind, strided, seed=M + 7 * Kc + N + nt)
    ref = _wgrad_ref(terms, g)
    dW = F.cheb_wgrad(terms, g)
    _assert_per_term(dW, ref, TOL_WGRAD, "cheb_wgrad")
    if nt > 32:                                   # the entry point takes 32 terms: F.cheb_wgrad split it
        return
    L = _lib.lib()
    ws = _nan_workspace(L.tgcn_cheb_wgrad_workspace_bytes(M, Kc, N, nt))
    rc, d1 = _wgrad_raw(terms, g, ws)
    assert rc == 0, L.tgcn_last_error()
    _assert_per_term(d1, ref, TOL_WGRAD, "ctypes")
    ws.fill_(float("nan"))
    rc, d2 = _wgrad_raw(terms, g, ws)
    assert rc == 0
    assert torch.equal(d1, d2) and torch.equal(d1, dW)                 # fixed reduction order, whatever the workspace held


def test_wgrad_entry_error_codes(gpu_device):
    """nterms > 32, a workspace one float short, M <= 0: refused before anything is launched, dW untouched."""
    from tgcn_amd import _lib
    L = _lib.lib()
    M, Kc, N = 300, 16, 8
    terms, g = _make_terms(M, Kc, N, 33, "zero", False, seed=3)
    need = L.tgcn_cheb_wgrad_workspace_bytes(M, Kc, N, 32)
    ws = _nan_workspace(L.tgcn_cheb_wgrad_workspace_bytes(M, Kc, N, 33))
    rc, dW = _wgrad_raw(terms, g, ws)
    assert rc == ERR_UNSUPPORTED and torch.isnan(dW).all()
    short = _nan_workspace(need)
    rc, dW = _wgrad_raw(terms[:32], g, short[:(need - 4) // 4])
    assert rc == ERR_WORKSPACE and torch.isnan(dW).all()
    rc, dW = _wgrad_raw([t[:0] for t in terms[:2]], g[:0], ws)
    assert rc == ERR_INVALID and torch.isnan(dW).all()
    assert L.tgcn_cheb_wgrad_workspace_bytes(0, Kc, N, 1) == 0
    rc, dW = _wgrad_raw(terms[:32], g, short)
    assert rc == 0                                                     # the queried size is enough


def _windows_raw(stack, g, W, want_G, want_dW, ws):
    from tgcn_amd import _lib
    L = _lib.lib()
    K, S, n, T = stack.shape
    H = W.shape[0] // K
    N = W.shape[1]
    G = torch.full((K, S, n, T), float("nan"), device="cuda") if want_G else None
    dW = torch.full((K, H, N), float("nan"), device="cuda") if want_dW else None
    rc = L.tgcn_cheb_windows_backward_f32(_lib.stream_ptr(), S, n, T, H, N, K, _lib.ptr(stack), _lib.ptr(g), _lib.ptr(W), _lib.ptr(G),
                                          _lib.ptr(dW), _lib.ptr(ws), ws.numel() * 4)
    torch.cuda.synchronize()
    assert rc == 0, L.tgcn_last_error()
    return G, dW


WINDOWS_CASES = [
    # S, n, T, H, N, K
    (1, 100, 9, 1, 64, 3),              # H = 1
    (3, 70, 12, 12, 65, 4),             # H = T: one window per recording
    (1, 64, 40, 15, 1, 25),             # K * H = 375
    (2, 33, 20, 5, 130, 2),
    (1, 1024, 19, 4, 64, 3),            # M = S * (T-H+1) * n = 16384: one chunk
    (1, 16385, 3, 3, 64, 2),            # M = 16385: a second chunk of one row
    (3, 997, 30, 7, 65, 3),
    (1, 90000, 75, 15, 32, 2),          # M = 5.49 M: the 256-chunk cap, ~5400-long chains per lane
]


@pytest.mark.parametrize("which", ["dgrad", "wgrad", "both"])
@pytest.mark.parametrize("S,n,T,H,N,K", WINDOWS_CASES)
def test_windows_backward_entry_vs_fp64(S, n, T, H, N, K, which, gpu_device):
    """tgcn_cheb_windows_backward_f32 against O.windows_projection_backward on a random stack: G = per-term input gradients (dW null),
    dW alone (G null) or both, every term k against its own max, NaN-filled workspace and outputs, the same bits twice."""
    from tgcn_amd import _lib
    L = _lib.lib()
    nwin = T - H + 1
    gen = torch.Generator(device="cuda").manual_seed(S * 7 + n + T * 3 + H + N + K)
    stack = torch.randn((K, S, n, T), device="cuda", generator=gen)
    g = torch.randn((S * nwin, n, N), device="cuda", generator=gen)
    W = torch.randn((K * H, N), device="cuda", generator=gen)
    want_G, want_dW = which in ("dgrad", "both"), which in ("wgrad", "both")
    ws = _nan_workspace(L.tgcn_cheb_windows_wgrad_workspace_bytes(S, n, T, H, N, K))
    G1, dW1 = _windows_raw(stack, g, W, want_G, want_dW, ws)
    ref_dW, ref_G = O.windows_projection_backward(stack.cpu().numpy(), g.cpu().numpy(), W.view(K, H, N).cpu().numpy())
    if want_G:
        _assert_per_term(G1, ref_G, TOL_WINDOWS, "G")
    if want_dW:
        _assert_per_term(dW1, ref_dW, TOL_WINDOWS, "dW")
    ws.fill_(float("nan"))
    G2, dW2 = _windows_raw(stack, g, W, want_G, want_dW, ws)
    for a, b in ((G1, G2), (dW1, dW2)):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
