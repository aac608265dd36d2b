"""Host side of the hot path: thin wrappers over the C ABI + the autograd function of the fused layer.

Every product, sum and axpy of the forward runs in libtgcn_hip.so (include/tgcn_hip.h); torch supplies device
memory, the stream and autograd bookkeeping.  There is no CPU fallback.
"""
import ctypes as C
import dataclasses
import functools
import math
import numbers
import struct
import threading

import torch

from . import _lib

SMALL_PATH = True   # developer switch (tools/): route small graphs through the general multi-launch path instead
MODE_POWER = 0      # dense-L classes: Xt[k] = 2 L^k x - Xt[k-2]  (tgcn/nn/gcn.py:75-78,150-153,233-236)
MODE_CHEBYSHEV = 1  # edge-list classes: Tx_k = 2 L Tx_{k-1} - Tx_{k-2}  (gcn.py:427-432,524-528)
BIAS_NONE, BIAS_CHANNEL, BIAS_VERTEX_CHANNEL = 0, 1, 2


def _cuda_device_of(a):
    """device of a CUDA tensor / GraphOperand / CompactPlan argument (or of the first element of a list of them), else None"""
    if isinstance(a, torch.Tensor):
        return a.device if a.is_cuda else None
    if isinstance(a, (list, tuple)):
        return _cuda_device_of(a[0]) if a else None
    d = getattr(a, "device", None)
    return d if isinstance(d, torch.device) and d.type == "cuda" else None


def _on_device(fn):
    """Every entry that calls the library runs with the device of its DATA current, on that device's current stream -- the reference's
    torch ops follow the tensor's device (tgcn/nn/gcn.py:141,147: `model.to('cuda:1')(x.to('cuda:1'))` works whatever device is
    current, and nn.DataParallel's replicas rely on it, examples/pytorch_based/pytorch_hcp_tgcn.py:270-273), while a raw launch goes
    to the calling thread's current device.  Arguments on two different devices are refused here (the kernels would dereference a
    foreign pointer); the C ABI checks the same against hipGetDevice (common.h: check_pointer_device)."""
    @functools.wraps(fn)
    def on_device(*args, **kw):
        dev = None
        for a in args:
            d = _cuda_device_of(a)
            if d is None:
                continue
            if dev is None:
                dev = d
            elif d != dev:
                raise _lib.TgcnError("tgcn_amd.%s: arguments on two devices (%s and %s) -- move the input, the parameters and the operand to one device"
                                     % (fn.__name__, dev, d))
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kw)
        with torch.cuda.device(dev):
            return fn(*args, **kw)
    return on_device


def _dense(t):
    """(nb, rows, C) view with a contiguous last dim -> tgcn_dense (strides in floats)."""
    assert t.dim() == 3 and t.dtype == torch.float32 and (t.shape[2] == 1 or t.stride(2) == 1), (t.shape, t.stride())
    return _lib.DenseStruct(t.data_ptr(), int(t.stride(0)), int(t.stride(1)))


def _aligned16(C_row, *tensors):
    ok = C_row % 4 == 0
    for t in tensors:
        if t is not None:
            ok = ok and t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 and t.stride(1) % 4 == 0
    return ok


def _aligned_input(x3):
    """x3, copied when a batch slice data[i:i+bs] of odd-width rows starts off a 16-byte boundary: the drivers want 16 bytes"""
    return x3.clone() if x3.data_ptr() % 16 else x3


def _workspace(nbytes, device, floor=256):
    return torch.empty(max(nbytes, floor), dtype=torch.uint8, device=device)


def weight_layout(W_kcn, kind):
    """Re-layouts of a (K, C, N) layer weight in libtgcn_hip.so (tgcn_weight_layout_f32): kind 0 -> (C, K*N) column blocks W_0 | ... | W_{K-1}
    (project-first form); kind 1 -> (K, N, C), W_k^T (the input gradient as a layer on (L^T, g, W^T)); kind 2 -> (N, K*C) (G = g W^T for all
    terms in one projection)."""
    _lib.require_device(W_kcn)
    K, Cc, N = W_kcn.shape
    W = W_kcn.contiguous()
    out = torch.empty({0: (Cc, K * N), 1: (K, N, Cc), 2: (N, K * Cc)}[kind], dtype=torch.float32, device=W.device)
    with torch.cuda.device(W.device):
        _lib.check(_lib.lib().tgcn_weight_layout_f32(_lib.stream_ptr(), K, Cc, N, _lib.ptr(W), _lib.ptr(out), kind))
    return out


class RowPermFn(torch.autograd.Function):
    """out[b, i] = x[b, perm[i]] for a (nb, rows, C) tensor -- the relabelling a GraphOperand.reordered() operand needs on the way in (perm)
    and out (inv_perm) -- as a differentiable op on tgcn_pack_rows_f32: the backward is the same kernel with the inverse permutation."""

    @staticmethod
    def forward(ctx, x3, perm, inv):
        ctx.perm, ctx.inv = perm, inv
        return _permute_rows(x3, perm)

    @staticmethod
    def backward(ctx, g):
        return _permute_rows(g, ctx.inv), None, None


def _permute_rows(x3, perm):
    _lib.require_device(x3, perm)
    x3 = x3.float().contiguous()
    out = torch.empty_like(x3)
    nb, rows, Cw = x3.shape
    with torch.cuda.device(x3.device):
        if nb > 1 and nb * rows <= (1 << 22):
            # many small samples (the reference's batches of 64 ... 512 on coarsened graphs): ONE launch over all of them -- the row index of
            # sample b is b * rows + perm (integer plumbing on nb * rows elements)
            idx = (torch.arange(nb, device=x3.device, dtype=torch.int64).unsqueeze(1) * rows + perm.unsqueeze(0)).reshape(-1)
            pack_rows(x3.view(nb * rows, Cw), idx, out.view(nb * rows, Cw))
        else:
            for b in range(nb):
                pack_rows(x3[b], perm, out[b])
    return out


def relabel_rows(t, perm, inv, dim=1):
    """t with its axis `dim` (the vertex axis) permuted: t.index_select(dim, perm), differentiable, through the library's row-packing kernel"""
    sh = t.shape
    lead = 1
    for d in sh[:dim]:
        lead *= d
    t3 = t.reshape(lead, sh[dim], -1)
    return RowPermFn.apply(t3, perm, inv).reshape(sh)


# ----------------------------------------------------------------------------------------- single ops
@_on_device
def csr_hop(op, x, z=None, alpha=1.0, beta=0.0, want_p=False, out=None, p_out=None, z2=None, gamma=0.0):
    """One hop:  S = L x;  y = alpha*S + beta*z (+ gamma*z2);  optionally also S.  x: (nb, op.n_cols, C); y, z, z2, S:
    (nb, op.n, C); any of them may be a strided view as long as the last dim is contiguous.  Returns y (and S when want_p).
    Low-level: rows are in the OPERAND's labels -- for a GraphOperand.reordered() operand the caller relabels (x[:, op.perm] in,
    y[:, op.inv_perm] out), as cheb_layer / cheb_stack / cheb_time_windows / cheb_relu_pool do."""
    _lib.require_device(x, z, z2)
    L = _lib.lib()
    assert x.dim() == 3 and x.dtype == torch.float32 and x.shape[1] == op.n_cols, (x.shape, op.n_cols)
    nb, _, Crow = x.shape
    y = torch.empty((nb, op.n, Crow), dtype=torch.float32, device=x.device) if out is None else out
    p = (torch.empty((nb, op.n, Crow), dtype=torch.float32, device=x.device) if p_out is None else p_out) if want_p else None
    for t in (y, z, p, z2):
        assert t is None or tuple(t.shape) == (nb, op.n, Crow), (t.shape, (nb, op.n, Crow))
    al = _aligned16(Crow, x, z, y, p, z2)
    sched = op.schedule_for(Crow, al)
    # the batch rides on grid.y (x column chunks of wide rows): slice batches beyond its 65535 limit
    nb_max = 65535 // max(1, -(-Crow // (256 if al else 64)))
    if nb > nb_max:
        for b0 in range(0, nb, nb_max):
            sl = slice(b0, min(nb, b0 + nb_max))
            csr_hop(op, x[sl], None if z is None else z[sl], alpha, beta, want_p, y[sl], None if p is None else p[sl],
                    None if z2 is None else z2[sl], gamma)
        return (y, p) if want_p else y
    ws = _workspace(L.tgcn_csr_hop_workspace_bytes(C.byref(sched.struct), nb, Crow, 1 if al else 0), x.device, floor=16)
    X, Y = _dense(x), _dense(y)
    Z = _dense(z) if z is not None else None
    P = _dense(p) if p is not None else None
    Z2 = _dense(z2) if z2 is not None else None
    _lib.check(L.tgcn_csr_hop2_f32(_lib.stream_ptr(), C.byref(op.struct), C.byref(sched.struct), nb, Crow, C.byref(X),
                                   C.byref(Z) if Z is not None else None, float(alpha), float(beta),
                                   C.byref(Z2) if Z2 is not None else None, float(gamma), C.byref(Y),
                                   C.byref(P) if P is not None else None, _lib.ptr(ws), ws.numel()))
    return (y, p) if want_p else y


@_on_device
def cheb_project(terms, W, bias, bias_kind, n_vertices, interleave=1, out=None):
    """out[r(m)] = sum_t terms[t][m, :] @ W[t] + bias; terms: list of (M, Kc) contiguous; W: (T, Kc, N)."""
    _lib.require_device(W, *terms)
    L = _lib.lib()
    T = len(terms)
    M, Kc = terms[0].shape
    N = W.shape[-1]
    W = W.reshape(T * Kc, N).contiguous()
    rows_out = M
    if out is None:
        out = torch.empty((rows_out, N), dtype=torch.float32, device=W.device)
    b = bias.contiguous() if bias is not None else None
    for t0 in range(0, T, 32):
        nt = min(32, T - t0)
        last = t0 + nt >= T
        a = (C.c_void_p * nt)(*[terms[t0 + i].data_ptr() for i in range(nt)])
        lda = (C.c_int64 * nt)(*[terms[t0 + i].stride(0) for i in range(nt)])
        _lib.check(L.tgcn_cheb_project_f32(_lib.stream_ptr(), M, Kc, N, nt, a, lda, _lib.ptr(W[t0 * Kc:]),
                                           _lib.ptr(b) if last else None, bias_kind if last else 0, n_vertices,
                                           interleave, 1 if t0 > 0 else 0, _lib.ptr(out), N))
    return out


@_on_device
def project_first(x3, Wcat, bias, bias_kind, K, N, rowmap=None):
    """Z = x . [W_0 | ... | W_{K-1}] with the bias on the first N columns (Z_0): the first step of the project-first form as its own call
    (tgcn_cheb_project_first_f32) for callers that run the recursion themselves -- the vertex-sharded layer exchanges cut rows between its
    hops.  x3: (q, rows, C); Wcat: (C, K*N) (weight_layout kind 0); bias read at the OUTPUT row; rowmap (int32[rows], nullable): output row of
    input row m.  -> (q, rows, K*N)"""
    _lib.require_device(x3, Wcat, bias, rowmap)
    q, rows, Crow = x3.shape
    assert x3.is_contiguous() and Wcat.is_contiguous() and tuple(Wcat.shape) == (Crow, K * N) and (rowmap is None or (rowmap.dtype == torch.int32 and rowmap.numel() == rows))
    x3 = _aligned_input(x3)
    Z = torch.empty((q, rows, K * N), dtype=torch.float32, device=x3.device)
    b = bias.contiguous() if bias is not None else None
    _lib.check(_lib.lib().tgcn_cheb_project_first_f32(_lib.stream_ptr(), q, rows, Crow, K, N, _lib.ptr(x3), _lib.ptr(Wcat), _lib.ptr(b),
                                                      bias_kind if b is not None else BIAS_NONE, _lib.ptr(rowmap), _lib.ptr(Z)))
    return Z


@_on_device
def csr_sddmm(op, rows3, cols3, alpha=1.0, out=None, accumulate=False):
    """dval[e] (+)= alpha * sum_b sum_c rows3[b, row(e), c] * cols3[b, col(e), c] over the stored entries of `op`, in CSR order -> (nnz,).
    The gradient of S = L X w.r.t. the values of L is csr_sddmm(op, dS, X) (tgcn_csr_sddmm_f32)."""
    _lib.require_device(rows3, cols3, out)
    nb, _, Crow = rows3.shape
    assert rows3.shape[1] == op.n and cols3.shape[1] == op.n_cols and cols3.shape[0] == nb and cols3.shape[2] == Crow
    if out is None:
        out = torch.zeros(max(op.nnz, 1), dtype=torch.float32, device=rows3.device)[: op.nnz]
        accumulate = False
    R, Cc = _dense(rows3), _dense(cols3)
    _lib.check(_lib.lib().tgcn_csr_sddmm_f32(_lib.stream_ptr(), C.byref(op.struct), op.n_cols, nb, Crow, C.byref(R), C.byref(Cc), float(alpha),
                                             _lib.ptr(out), 1 if accumulate else 0))
    return out


def _values_guard(op, epoch, values_csr):
    """Learnable values are packed IN PLACE into one operand per pattern (GraphOperand.update_values), and a backward reads the operand's
    CURRENT values (hops on op.transpose(), the recomputed basis).  When the same pattern has been packed with OTHER values between a forward
    and its backward -- two spmm calls with one index and two weight tensors, one ChebConv called twice with computed edge_weights -- the
    operand no longer holds what this backward differentiates: re-pack the values the forward ran with (saved in ctx), and drop the stamp of
    the last packing so that the next forward packs its own weight again.  torch's in-place version check cannot see this (the packed
    entries are not a tensor of the graph); the old per-weight cache key was correct by construction, this keeps the per-pattern operand
    correct too."""
    if values_csr is None or op.values_epoch == epoch:
        return
    with op._lock:
        if op.values_epoch != epoch:
            op.update_values(values_csr)
            op._packed_stamp = None
            op._packed_alias = None


class SpmmFn(torch.autograd.Function):
    """out = L matrix3 (one hop) as a differentiable op: d matrix = L^T g (the hop on the cached transposed operand), d values = the sampled
    product <g[row(e)], matrix[col(e)]> in CSR order (csr_sddmm) -- the reference's spmm* are differentiable in both (gcn.py:296-308)."""

    @staticmethod
    @_on_device
    def forward(ctx, matrix3, values_csr, op):
        ctx.op = op
        ctx.values_epoch = op.values_epoch
        ctx.save_for_backward(matrix3, None if values_csr is None else values_csr.detach())
        return csr_hop(op, matrix3)

    @staticmethod
    @_on_device
    def backward(ctx, g):
        matrix3, vals = ctx.saved_tensors
        _values_guard(ctx.op, ctx.values_epoch, vals)
        g = g.contiguous()
        gm = csr_hop(ctx.op.transpose(), g) if ctx.needs_input_grad[0] else None
        gv = csr_sddmm(ctx.op, g, matrix3) if ctx.needs_input_grad[1] else None
        return gm, gv, None


@_on_device
def chebyshev_values_grad(op, x3, W_kcn, g, basis=None):
    """d loss / d values (CSR order) of the true-recurrence layer out = sum_k T_k W_k, T_1 = L x, T_k = 2 L T_{k-1} - T_{k-2} (ChebConv /
    ChebTimeConv: lap_e = -deg^-1/2[row] w_e deg^-1/2[col] is differentiable in w_e in the reference, tgcn/nn/gcn.py:413,510).
    With G_k = g W_k^T and the Clenshaw adjoints b_{K-1} = G_{K-1}, b_k = G_k + 2 L^T b_{k+1} - b_{k+2}:
        dL = b_1 T_0^T + 2 sum_{k>=2} b_k T_{k-1}^T   sampled on the stored pattern (csr_sddmm).  Hops, projection and SDDMM in libtgcn_hip.so.
    basis: the (q, n, C) terms T_0 .. T_{K-1} when the forward kept them (ChebLayerFn: forward_keeping_basis) -- otherwise T_0 .. T_{K-2} are
    recomputed here.  Every adjoint is consumed by its sampled product as soon as it exists and only the two the recurrence still needs stay
    alive (the K-1 adjoints used to be held until the SDDMM loop)."""
    K, Crow, N = W_kcn.shape
    q, n, _ = x3.shape
    dval = torch.zeros(max(op.nnz, 1), dtype=torch.float32, device=x3.device)[: op.nnz]
    if K < 2 or op.nnz == 0:
        return dval
    if basis is not None:
        T = basis
    else:
        T = cheb_stack(op, x3.contiguous(), K - 1, MODE_CHEBYSHEV) if K > 2 else x3.contiguous().unsqueeze(0)      # T_0 .. T_{K-2}
    g = g.contiguous()
    Wcat = weight_layout(W_kcn, 2).view(1, N, K * Crow)
    Gall = cheb_project([g.reshape(q * n, N)], Wcat, None, BIAS_NONE, n).view(q, n, K * Crow)
    G = lambda k: Gall[:, :, k * Crow:(k + 1) * Crow]
    opT = op.transpose()
    b1, b2 = G(K - 1), None                     # b_k, b_{k+1} as the loop walks k = K-1 .. 1
    first = True
    for k in range(K - 1, 0, -1):
        if k < K - 1:
            b1, b2 = csr_hop(opT, b1, z=b2, alpha=2.0, beta=-1.0, z2=G(k), gamma=1.0), b1
        csr_sddmm(op, b1, T[k - 1], alpha=1.0 if k == 1 else 2.0, out=dval, accumulate=not first)
        first = False
    return dval


def _adjoint_hops(opT, G, mode):
    """sum_k T_k(L^T) G[k] for the K per-term input gradients G (a list or a (K, ...) tensor of (q, n, C) terms): Horner for MODE_POWER
    (b = G_j + L^T b), Clenshaw for MODE_CHEBYSHEV (b_{K-1} = G_{K-1}, b_k = G_k + 2 L^T b_{k+1} - b_{k+2}, result G_0 + L^T b_1 - b_2); one
    hop launch per step.  K = 1: G[0] itself."""
    K = len(G)
    if K == 1:
        return G[0]
    if mode == MODE_POWER:
        b = G[K - 1]
        for j in range(K - 2, -1, -1):
            b = csr_hop(opT, b, z=G[j], alpha=1.0, beta=1.0)
        return b
    b1, b2 = G[K - 1], None
    for k in range(K - 2, 0, -1):
        b1, b2 = csr_hop(opT, b1, z=b2, alpha=2.0, beta=-1.0, z2=G[k], gamma=1.0), b1
    return csr_hop(opT, b1, z=b2, alpha=1.0, beta=-1.0, z2=G[0], gamma=1.0)


def _bias_grad(g3, bias_kind, bias_shape, needed):
    """gradient of a per-channel / per-(vertex, channel) bias from the (samples, n, N) output gradient (torch reductions), or None when
    there is no bias or it needs none"""
    if bias_shape is None or not needed:
        return None
    return (g3.sum(dim=(0, 1)) if bias_kind == BIAS_CHANNEL else g3.sum(dim=0)).reshape(bias_shape)


@_on_device
def _windows_forward(op, x3, W, bias, bias_kind, mode):
    """x3 (S, n, T) fp32 contiguous, W (K, H, N) in the WORKING basis (folded for MODE_POWER) -> (out, stack (K, S, n, T))"""
    L = _lib.lib()
    S, n, T = x3.shape
    K, H, N = W.shape
    nwin = T - H + 1
    # x3 is in the operand's labels already (cheb_time_windows relabelled it): cheb_stack must not relabel it again
    stack = _series_stack(op, x3, K, mode)   # (K, S, n, T)
    out = torch.empty((S * nwin, n, N), dtype=torch.float32, device=x3.device)
    W2 = W.reshape(K * H, N).contiguous()
    b = bias.contiguous() if bias is not None else None
    assert K <= 32, "more than 32 hops: chunk the projection"
    for s in range(S):
        ptrs = (C.c_void_p * K)(*[stack[k, s].data_ptr() for k in range(K)])
        _lib.check(L.tgcn_cheb_project_windows_f32(_lib.stream_ptr(), n, T, H, N, K, ptrs, _lib.ptr(W2), _lib.ptr(b), bias_kind,
                                                   _lib.ptr(out[s * nwin:])))
    return out, stack


class ChebWindowsFn(torch.autograd.Function):
    """Streaming time-window layer with its backward: the hops run once on the T columns of every recording in both directions.
    d series = sum_k T_k(L^T) G_k with G_k the per-term input gradients of the window projection (tgcn_cheb_windows_backward_f32),
    folded by Horner (mode 0) / Clenshaw (mode 1) hops on L^T (_adjoint_hops, as in layer_backward); dW from the same entry point."""

    @staticmethod
    @_on_device
    def forward(ctx, series, weight_khg, bias, op, mode, bias_kind):
        x3 = series.float().contiguous()
        W = weight_khg.float().contiguous()
        fold = _power_fold(mode, W)
        Wt = _working_weight(fold, W)
        out, stack = _windows_forward(op, x3, Wt, bias, bias_kind, mode)
        ctx.save_for_backward(x3, Wt)
        ctx.stack = stack if ctx.needs_input_grad[1] else None       # the basis the weight gradient contracts with g
        ctx.op, ctx.mode, ctx.fold, ctx.bias_kind = op, mode, fold, bias_kind
        ctx.bias_shape = None if bias is None else bias.shape
        return out

    @staticmethod
    @_on_device
    def backward(ctx, g):
        x3, Wt = ctx.saved_tensors
        S, n, T = x3.shape
        K, H, N = Wt.shape
        nwin = T - H + 1
        L = _lib.lib()
        g = g.contiguous()
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        G = torch.empty((K, S, n, T), dtype=torch.float32, device=g.device) if need_x else None
        dW = torch.empty((K, H, N), dtype=torch.float32, device=g.device) if need_w else None
        ws = _workspace(L.tgcn_cheb_windows_wgrad_workspace_bytes(S, n, T, H, N, K), g.device, floor=16)
        _lib.check(L.tgcn_cheb_windows_backward_f32(_lib.stream_ptr(), S, n, T, H, N, K, _lib.ptr(ctx.stack), _lib.ptr(g),
                                                    _lib.ptr(Wt.reshape(K * H, N)), _lib.ptr(G), _lib.ptr(dW), _lib.ptr(ws), ws.numel()))
        ctx.stack = None
        gx = _adjoint_hops(ctx.op.transpose(), G, ctx.mode) if need_x else None
        if need_w and ctx.fold is not None:
            dW = fold_weight(ctx.fold, dW, transpose=True)
        gb = _bias_grad(g.view(S * nwin, n, N), ctx.bias_kind, ctx.bias_shape, ctx.needs_input_grad[2])
        return gx, dW, gb, None, None, None


def series_geometry(T, H, stride=1, padding=0, who="cheb_time_windows", dilation=1):
    """(stride, left, right, nwin) of a streaming call on T time steps with windows of H: padding an int p = (p, p), a pair (left, right) or
    "causal" = (H-1, 0), 0 <= left, right <= H-1 (every window touches a real row); nwin = (T + left + right - H) // stride + 1.
    dilation (an integer >= 1) puts the H taps that many time rows apart: the window then spans He = (H-1)*dilation + 1 rows and He takes H's
    place in all of the above; dilation > 1 runs at stride 1 only.  (H == 1: He == 1, the undilated window -- series_dilation.)
    TgcnError for anything else -- checked before an operand is built or anything launches."""
    def integer(v):
        return isinstance(v, numbers.Integral) and not isinstance(v, bool)
    if not integer(dilation) or dilation < 1:
        raise _lib.TgcnError("%s: dilation is an integer >= 1, got %r" % (who, dilation))
    taps, H = H, (H - 1) * int(dilation) + 1      # from here on H is the span He
    if isinstance(padding, str):
        if padding != "causal":
            raise _lib.TgcnError('%s: padding is an int, a pair (left, right) or "causal", got %r' % (who, padding))
        left, right = H - 1, 0
    elif integer(padding):
        left = right = int(padding)
    elif isinstance(padding, (tuple, list)) and len(padding) == 2 and all(integer(v) for v in padding):
        left, right = int(padding[0]), int(padding[1])
    else:
        raise _lib.TgcnError('%s: padding is an int, a pair (left, right) or "causal", got %r' % (who, padding))
    if not integer(stride) or stride < 1:
        raise _lib.TgcnError("%s: stride is an integer >= 1, got %r" % (who, stride))
    if dilation > 1 and stride > 1:
        raise _lib.TgcnError("%s: dilation=%d together with stride=%d is not supported (a dilated window runs at stride 1)" % (who, dilation, stride))
    if not (0 <= left <= H - 1 and 0 <= right <= H - 1):
        raise _lib.TgcnError("%s: padding (%d, %d) outside 0 .. %s - 1 = %d" % (who, left, right, "H" if dilation == 1 else "(H - 1) * dilation + 1", H - 1))
    if T + left + right < H:
        raise _lib.TgcnError("%s: %d time steps with padding (%d, %d) are fewer than one window of %d%s"
                             % (who, T, left, right, H, "" if dilation == 1 else " (%d taps, dilation %d)" % (taps, dilation)))
    return int(stride), left, right, (T + left + right - H) // int(stride) + 1


def series_dilation(H, dilation):
    """the dilation a call with H taps runs at, after series_geometry has checked it: one tap has nothing to dilate, so H == 1 runs as
    dilation 1 (the same windows, the same calls) whatever the value -- no dilation that a span does not bound reaches a kernel"""
    return 1 if H == 1 else int(dilation)


def _geom4(geom):
    """(stride, left, right, dilation) of a geom given with or without its dilation"""
    return (tuple(geom) + (1,))[:4]


def _series_stack(op, x3, K, mode):
    """the K hop tensors of a series' rows in the operand's labels: the monomial stack (power mode) or the Chebyshev recurrence"""
    return _monomial_stack(op, x3, K) if mode == MODE_POWER else cheb_stack(op, x3, K, MODE_CHEBYSHEV, _operand_labels=True)


def _series_bias_grad(g, as_series, bias_kind, bias_shape):
    """the bias gradient of a time-window layer from its fp32 output gradient g: (S, n, nwin, N) as a series, else (S*nwin, n, N)"""
    if as_series:
        return (g.sum(dim=(0, 1, 2)) if bias_kind == BIAS_CHANNEL else g.sum(dim=(0, 2))).reshape(bias_shape)
    return _bias_grad(g, bias_kind, bias_shape, True)


def _bf16_row_ld(Tf):
    """elements between the vertex rows of a bf16 hop stack (the trailing-element row padding): T*f rounded up to whole 16-byte units, so
    that every row starts aligned; rows of fewer than 7 elements stay packed"""
    return Tf if (Tf % 8 == 0 or Tf < 7) else Tf + (-Tf) % 8


def _series_stack_bf16(op, rows, K, mode):
    """the bf16 hop stack of a (S, n, T*f) block of bf16 rows in the operand's labels -> (stack (K, S, n, ld), ld): the rows padded with
    trailing zeros to ld elements (_bf16_row_ld), then one bf16 hop per term written into its slice (_basis_bf16)"""
    S, n, Tf = rows.shape
    ld = _bf16_row_ld(Tf)
    if ld != Tf:
        rows = torch.nn.functional.pad(rows, (0, ld - Tf))
    stack = torch.empty((K, S, n, ld), dtype=BF16, device=rows.device)
    _basis_bf16(op, rows, K, mode, out=stack)
    return stack, ld


def check_series_bf16(f, as_series, geom, series_dtype):
    """what a streaming call with bfloat16 parameters needs, checked before an operand is built: not the scalar-load form (ChebWindowsFn: one
    channel, window-major, default geometry), and a series that is bfloat16 already -- a streaming chain is bf16 from end to end (an
    as_series=True output feeds the next layer as it is), so the recording is cast once by its owner, not once per call here; a series of
    another dtype with bf16 parameters is refused like a weight and a bias of two dtypes (param_dtype)."""
    if f == 1 and not as_series and _geom4(geom) == (1, 0, 0, 1):
        raise _lib.TgcnError("forward_series / cheb_time_windows: bfloat16 parameters are not supported on a single-channel series with "
                             "as_series=False at stride=1, padding=0, dilation=1 (the scalar-load form); as_series=True or any stride / padding "
                             "/ dilation runs")
    if series_dtype != BF16:
        raise _lib.TgcnError("forward_series / cheb_time_windows: the parameters are bfloat16 but the series is %s -- cast it once "
                             "(series.to(torch.bfloat16))" % series_dtype)


def _series_operands(series, weight_khfg, bias, mode):
    """what every float32 series Function launches with -> (series, fold, working weight, bias): the fp32 contiguous series (S, n, T, f), the
    fold of the (K, H*f, N) weight view (_power_fold: None outside power mode with K > 2), that view in the kernels' basis (_working_weight:
    at most one tgcn_fold_weight_f32) and the contiguous bias.  The bias goes through .float() at every site (the one-launch Functions did,
    the others called .contiguous() alone): param_dtype has refused a bias of another dtype than the weight's, so on these float32 paths it
    returns the tensor itself and launches nothing"""
    K, H, f, N = weight_khfg.shape
    W = weight_khfg.float().contiguous().view(K, H * f, N)
    fold = power_fold_matrix(K, W.device) if (mode == MODE_POWER and K > 2) else None       # _power_fold and _working_weight, without their calls
    return series.float().contiguous(), fold, W if fold is None else fold_weight(fold, W), None if bias is None else bias.float().contiguous()


def _series_ctx(ctx, op, mode, fold, bias, bias_kind, as_series, dims, geom=None, pooled=None, bf16=None):
    """The fields a float32 series Function leaves for its backward, in one call per forward (these calls run at 0.3 ms, where a Python
    call counts); dims starts (S, n, T, f, H, N, K).
    geom = (stride, left, right, dilation) of a Function with a whole hop stack: ctx.geom is the backward's record of it -- the arguments
    that follow the common ones in the entries of that geometry, which also names them (_series_backward): () the default geometry's,
    (stride, left, right) the _conv entries', all four the _dilated ones'.
    pooled = (Wt, z, idx, pool, nwin, drop) of a pooled one (_series_pool_backward): saved in that order, the pool, the window count, and
    the mask's seed tensor and scale (None, None without one).
    bf16 = (ld, (series dtype, weight dtype, bias dtype)) of ChebSeriesBf16Fn -- the stack's row distance and what the gradients are cast
    to; None marks a float32 Function for _series_backward."""
    ctx.op, ctx.mode, ctx.fold, ctx.bias_kind, ctx.as_series, ctx.dims, ctx.bf16 = op, mode, fold, bias_kind, as_series, dims, bf16
    ctx.bias_shape = None if bias is None else bias.shape
    if geom is not None:
        ctx.geom = geom if geom[3] > 1 else (geom[:3] if geom[:3] != (1, 0, 0) else ())
    if pooled is not None:
        Wt, z, idx, ctx.pool, ctx.nwin, drop = pooled
        ctx.save_for_backward(Wt, z, idx)
        ctx.seed, ctx.scale = (None, None) if drop is None else (drop[0], drop[2])


def _series_dW(ctx, dW):
    """the (K, H*f, N) weight gradient of the working weight -> the caller's (K, H, f, N): un-folded (once: a chunked walk passes its sum)"""
    S, n, T, f, H, N, K = ctx.dims[:7]
    if ctx.fold is not None:
        dW = fold_weight(ctx.fold, dW, transpose=True)
    return dW.view(K, H, f, N)


class ChebSeriesFn(torch.autograd.Function):
    """Streaming time-window layer on a multi-channel series (S, n, T, f), weight (K, H, f, N): the hops run once on rows of T*f floats in
    both directions, the window projection and its two gradients are the sliding-window MFMA kernels of csrc/windows.h
    (tgcn_cheb_project_series_f32 / tgcn_cheb_series_backward_f32), one launch each for all S recordings.  as_series picks the output
    layout, (S*nwin, n, N) or (S, n, nwin, N); the backward reads its gradient in that layout in place.
    geom = (stride, left, right[, dilation]): a window step, zero padding and tap distance in time.  (1, 0, 0) calls the entries above; anything
    else their _conv forms (the hops do not depend on it), after asking tgcn_series_conv_plan whether the forward's span fits -- before the hops
    run.  dilation > 1 (at stride 1) calls the _dilated entries, planned as step 1: their span does not grow with the dilation."""

    @staticmethod
    @_on_device
    def forward(ctx, series, weight_khfg, bias, op, mode, bias_kind, as_series, geom=(1, 0, 0)):
        L = _lib.lib()
        S, n, T, f = series.shape
        K, H, _, N = weight_khfg.shape
        stride, left, right, dil = _geom4(geom)
        nwin = (T + left + right - (H - 1) * dil - 1) // stride + 1
        if dil > 1 or (stride, left, right) != (1, 0, 0):
            hc, lds = C.c_int32(0), C.c_int32(0)
            _lib.check(L.tgcn_series_conv_plan(H, f, N, int(f % 4 == 0), stride, C.byref(hc), C.byref(lds)))
        x, fold, Wt, b = _series_operands(series, weight_khfg, bias, mode)
        _series_ctx(ctx, op, mode, fold, bias, bias_kind, as_series, (S, n, T, f, H, N, K), (stride, left, right, dil))
        x3 = _aligned_input(x.view(S, n, T * f))
        # the series is in the operand's labels already (cheb_time_windows relabelled it)
        stack = _series_stack(op, x3, K, mode)   # (K, S, n, T*f)
        out = torch.empty((S, n, nwin, N) if as_series else (S * nwin, n, N), dtype=torch.float32, device=x3.device)
        entry = (L.tgcn_cheb_project_series_dilated_f32 if dil > 1 else L.tgcn_cheb_project_series_conv_f32 if ctx.geom
                 else L.tgcn_cheb_project_series_f32)
        _lib.check(entry(_lib.stream_ptr(), S, n, T, f, H, N, K, _lib.ptr(stack), _lib.ptr(Wt), _lib.ptr(b), bias_kind, 1 if as_series else 0,
                         _lib.ptr(out), *ctx.geom))
        ctx.save_for_backward(Wt)
        ctx.stack = stack if ctx.needs_input_grad[1] else None       # the basis the weight gradient contracts with g
        return out

    @staticmethod
    @_on_device
    def backward(ctx, g):
        return _series_backward(ctx, ctx.saved_tensors[0], g) + (None,) * 5


def _series_backward(ctx, Wt, g):
    """(d series, dW, d bias) of ChebSeriesFn from the gradient g of its output in the forward's layout -- the body every series Function
    with a whole hop stack shares; reads ctx.stack and _series_ctx's fields, ctx.geom among them, of the forward.
    ctx.bf16 (ChebSeriesBf16Fn) picks the _bf16 workspace queries and entries, which take the stack's ld behind the stack and a bf16 g, and
    casts the three results to the forward's dtypes; G, dW, the adjoint hops, the un-fold and the bias sum are fp32 either way."""
    S, n, T, f, H, N, K = ctx.dims
    L = _lib.lib()
    g = _aligned_input((g.float() if ctx.bf16 is None else g.to(BF16)).contiguous())
    need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    gx = dW = None
    if need_x or need_w:
        G = torch.empty((K, S, n, T * f), dtype=torch.float32, device=g.device) if need_x else None
        dW = torch.empty((K, H * f, N), dtype=torch.float32, device=g.device) if need_w else None
        if ctx.bf16 is None:
            stack = (_lib.ptr(ctx.stack),)
            query, entry = ((L.tgcn_cheb_series_dilated_backward_workspace_bytes, L.tgcn_cheb_series_dilated_backward_f32) if len(ctx.geom) == 4 else
                            (L.tgcn_cheb_series_conv_backward_workspace_bytes, L.tgcn_cheb_series_conv_backward_f32) if ctx.geom else
                            (L.tgcn_cheb_series_backward_workspace_bytes, L.tgcn_cheb_series_backward_f32))
        else:       # (no default-geometry entry: ctx.geom is never ())
            stack = (_lib.ptr(ctx.stack), ctx.bf16[0])
            query, entry = ((L.tgcn_cheb_series_dilated_backward_bf16_workspace_bytes, L.tgcn_cheb_series_dilated_backward_bf16)
                            if len(ctx.geom) == 4 else (L.tgcn_cheb_series_conv_backward_bf16_workspace_bytes, L.tgcn_cheb_series_conv_backward_bf16))
        ws = _workspace(query(S, n, T, f, H, N, K, *ctx.geom), g.device, floor=16)
        _lib.check(entry(_lib.stream_ptr(), S, n, T, f, H, N, K, *stack, _lib.ptr(g), 1 if ctx.as_series else 0, _lib.ptr(Wt),
                         _lib.ptr(G), _lib.ptr(dW), _lib.ptr(ws), ws.numel(), *ctx.geom))
        ctx.stack = None
        if need_x:
            gx = _adjoint_hops(ctx.op.transpose(), G, ctx.mode).reshape(S, n, T, f)
        if need_w:
            dW = _series_dW(ctx, dW)
    gb = None
    if ctx.bias_shape is not None and ctx.needs_input_grad[2]:
        gb = _series_bias_grad(g if ctx.bf16 is None else g.float(), ctx.as_series, ctx.bias_kind, ctx.bias_shape)
    if ctx.bf16 is not None:        # rounded once each: bf16, or fp32 for a series behind a reordered operand's relabelling
        gx, dW, gb = (None if t is None else t.to(dt) for t, dt in zip((gx, dW, gb), ctx.bf16[1]))
    return gx, dW, gb


def check_pool(pool, n, who):
    """what the relu + pool epilogue of the streaming layers asks: pool 2 or 4 consecutive vertices, dividing the graph"""
    if not isinstance(pool, numbers.Integral) or isinstance(pool, bool) or pool not in (2, 4):
        raise _lib.TgcnError("%s: pool is 2 or 4, got %r" % (who, pool))
    if n % pool:
        raise _lib.TgcnError("%s: %d vertices are not a multiple of pool = %d" % (who, n, pool))
    return int(pool)


def series_pool_is_fused(op, pool=4, stream=False):
    """True where cheb_time_windows_relu_pool / cheb_time_stream_relu_pool (stream=True) run relu + pool inside the projection's epilogue
    (ChebSeriesReluPoolFn, tgcn_cheb_project_series_stream_pool_f32), False where they run the unfused composition -- the layer, then
    tgcn_relu_pool_f32 on a view of its output.  The two are bit-identical, so this is a question of speed and memory only.
    A reordered operand is never fused: pool groups are consecutive vertices of the CALLER's labels, scattered rows of the operand's.
    Nothing else is excluded: profiles/r18_series_relu_pool.json (DESIGN.md 3.10 "relu + pool epilogue") has the fused call at 0.99 of the
    composition's forward at 32 -> 64 on the 148-parcel graph (4.525 against 4.591 ms, spreads 0.015 / 0.035; a tie in training), 0.80 / 0.92 on
    the 90 k mesh at 4 -> 32 and 0.48 at 1 -> 32 -- no measured shape class where it is slower by more than the spread.  pool = 2 and the
    stream call are not measured."""
    return op.perm is None


class ChebSeriesReluPoolFn(torch.autograd.Function):
    """z = max over `pool` consecutive vertices of relu(ChebSeriesFn's output), the max taken in the projection's epilogue
    (tgcn_cheb_project_series_pool_f32, csrc/windows.h POOLED): the (S, n, nwin, N) layer output is never allocated, in the forward or --
    beyond the gradient w.r.t. it, which the layer's backward reads -- in the backward.  z is (S*nwin, n/pool, N) or, as_series,
    (S, n/pool, nwin, N), bit-identical to tgcn_relu_pool_f32 on the unfused output.  Asks tgcn_series_pool_plan before the hops.
    need_idx (the caller's: grad mode and a leaf that requires grad) stores the arg-max bytes; the backward routes gz through them
    (tgcn_relu_pool_bwd_f32 on the forward's layout: q = S*nwin, f = N window-major, q = S, f = nwin*N as a series) and runs ChebSeriesFn's
    backward body on the result.  Saves z, idx, the working weight, and the stack only if the weight trains.
    drop = (seed tensor, thr, scale) puts dropout between relu and the pool (tgcn_cheb_project_series_pool_dropout_f32, csrc/windows.h DROP):
    z = the max of relu(y) * m, m = scale where dropout.h's mask keeps the element and 0 elsewhere, bit-identical to
    tgcn_relu_dropout_pool_f32 on the unfused output; neither y nor a mask is ever allocated.  The backward needs no mask: z > 0 implies
    the arg-max was kept, so gy[arg-max] = z > 0 ? gz * scale : 0 -- gz * scale (fp32), then the backward without one.  ctx.seed is the
    seed's tensor (z.grad_fn.seed: what a captured step with seed=None drew).
    One channel runs the MFMA kernels in every geometry: where forward_series itself runs the scalar-load form (ChebWindowsFn: one channel,
    window-major, default geometry) the bits are those of forward_series(..., as_series=True), permuted."""

    @staticmethod
    @_on_device
    def forward(ctx, series, weight_khfg, bias, op, mode, bias_kind, as_series, geom, pool, need_idx, drop=None):
        L = _lib.lib()
        S, n, T, f = series.shape
        K, H, _, N = weight_khfg.shape
        stride, left, right, dil = geom       # (the entries pass all four)
        nwin = (T + left + right - (H - 1) * dil - 1) // stride + 1
        hc, lds = C.c_int32(0), C.c_int32(0)
        _lib.check(L.tgcn_series_pool_plan(H, f, N, int(f % 4 == 0), stride, pool, C.byref(hc), C.byref(lds)))
        x, fold, Wt, b = _series_operands(series, weight_khfg, bias, mode)
        x3 = _aligned_input(x.view(S, n, T * f))
        stack = _series_stack(op, x3, K, mode)   # (K, S, n, T*f)
        shape = (S, n // pool, nwin, N) if as_series else (S * nwin, n // pool, N)
        z = torch.empty(shape, dtype=torch.float32, device=x3.device)
        idx = torch.empty(shape, dtype=torch.uint8, device=x3.device) if need_idx else None
        args = (_lib.stream_ptr(), S, n, T, f, H, N, K, _lib.ptr(stack), _lib.ptr(Wt), _lib.ptr(b), bias_kind, 1 if as_series else 0, _lib.ptr(z),
                _lib.ptr(idx), pool, stride, left, right, dil)
        if drop is None:
            _lib.check(L.tgcn_cheb_project_series_pool_f32(*args))
        else:
            _lib.check(L.tgcn_cheb_project_series_pool_dropout_f32(*args, _lib.ptr(drop[0]), drop[1], drop[2]))
        ctx.stack = stack if ctx.needs_input_grad[1] else None
        _series_ctx(ctx, op, mode, fold, bias, bias_kind, as_series, (S, n, T, f, H, N, K), (stride, left, right, dil),
                    (Wt, z, idx, pool, nwin, drop))
        return z

    @staticmethod
    @_on_device
    def backward(ctx, gz):
        who = "cheb_time_windows_relu_pool" if ctx.scale is None else "cheb_time_windows_relu_dropout_pool"
        return _series_pool_backward(ctx, gz, who) + (None,) * 8


def _series_pool_backward(ctx, gz, who):
    """(d series, dW, d bias) behind a pooled forward: gz (times the mask's scale) to the arg-max vertex where z > 0, then ChebSeriesFn's
    backward body; who names the public entry in the refusal of a forward that kept no arg-max"""
    Wt, z, idx = ctx.saved_tensors
    S, n, T, f, H, N, K = ctx.dims
    if idx is None:
        raise _lib.TgcnError("%s: the forward ran without grad mode and kept no arg-max" % who)
    if ctx.scale is not None:
        gz = gz.float() * ctx.scale
    gy = torch.empty((S, n, ctx.nwin, N) if ctx.as_series else (S * ctx.nwin, n, N), dtype=torch.float32, device=gz.device)
    q, fN = (S, ctx.nwin * N) if ctx.as_series else (S * ctx.nwin, N)
    _lib.check(_lib.lib().tgcn_relu_pool_bwd_f32(_lib.stream_ptr(), _lib.ptr(gz.float().contiguous()), _lib.ptr(z), _lib.ptr(idx), _lib.ptr(gy),
                                                 q, n, fN, ctx.pool))
    return _series_backward(ctx, Wt, gy)


def _relu_pool_view(y, pool):
    """relu + pool as its own pass (ReluPoolFn) over the vertex axis (dim 1) of a layer output in either layout: (q, n, N) as it is,
    (S, n, nwin, N) through its (S, n, nwin*N) view"""
    if y.dim() == 3:
        return ReluPoolFn.apply(y, pool)
    S, n, nwin, N = y.shape
    return ReluPoolFn.apply(y.reshape(S, n, nwin * N), pool).view(S, n // pool, nwin, N)


def cheb_time_windows_relu_pool(op, series, weight, bias, bias_kind, mode, pool, as_series=False, stride=1, padding=0, dilation=1):
    """gcn_pool_4(relu(cheb_time_windows(...))) (pool=4; pool=2: gcn_pool) with relu and the max over `pool` consecutive vertices in the
    projection's epilogue: series (S, n, T) with weight (K, H, N), or (S, n, T, f) with (K, H, f, N) -> z (S*nwin, n/pool, N) or,
    as_series=True, (S, n/pool, nwin, N) -- a series on the coarsened graph.  The layer's full output is never allocated; values and every
    gradient are bit-identical to the hand-written composition.  as_series, stride, padding, dilation: cheb_time_windows'.
    A single-channel series runs the MFMA kernels (ChebSeriesFn's) in every geometry -- the scalar-load form has no pooled epilogue.
    A reordered operand runs the unfused composition (series_pool_is_fused): the layer, relabelled back, then tgcn_relu_pool_f32 on a view.
    Dropout between relu and pool, as the reference's training script has it, is cheb_time_windows_relu_dropout_pool (below): the same
    epilogue with a counter-based mask, so the full output stays unallocated in training too.
    TgcnError before anything is built or launched: bfloat16 parameters, pool outside {2, 4}, n % pool != 0, and every refusal
    cheb_time_windows makes for the same arguments.  There is no time_chunk: the causal layer in time chunks through this epilogue is
    cheb_time_windows_relu_pool_chunked."""
    return _series_relu_pool("cheb_time_windows_relu_pool", op, series, weight, bias, bias_kind, mode, pool, as_series, stride, padding, dilation)


def _series_relu_pool(who, op, series, weight, bias, bias_kind, mode, pool, as_series, stride, padding, dilation, seed=None, thr=None, scale=None):
    """cheb_time_windows_relu_pool (thr None: no mask) and, behind its own checks of p and the seed, cheb_time_windows_relu_dropout_pool:
    seed is the caller's (None, an integer or a tensor) -- the seed tensor of drop = (seed tensor, thr, scale) is made here, once the
    arguments are accepted"""
    if param_dtype(weight, bias, who) == BF16:
        raise _lib.TgcnError(_POOL_F32_ONLY % who)
    pool, geom = _series_pool_checks(who, series, weight, pool, stride, padding, dilation)
    series, weight, need_idx = _series_pool_tensors(series, weight, bias)
    drop = None if thr is None else (dropout_seed(seed, series.device, who), thr, scale)
    if not series_pool_is_fused(op, pool):
        return _series_pool_unfused(op, lambda s, b: ChebSeriesFn.apply(s, weight, b, op, mode, bias_kind, bool(as_series), geom), series, bias,
                                    bias_kind, pool, drop)
    return ChebSeriesReluPoolFn.apply(series, weight, bias, op, mode, bias_kind, bool(as_series), geom, pool, need_idx, drop)


def _series_shape_check(who, series, weight):
    """the ranks and channels of a whole-series call -> f"""
    if series.dim() not in (3, 4) or weight.dim() != series.dim():
        raise _lib.TgcnError("%s: a (S, n, T) series takes a (K, H, N) weight and a (S, n, T, f) series a (K, H, f, N) weight "
                             "(got %s and %s)" % (who, tuple(series.shape), tuple(weight.shape)))
    f = series.shape[3] if series.dim() == 4 else 1
    if series.dim() == 4 and weight.shape[2] != f:
        raise _lib.TgcnError("%s: the series has %d channels, the weight %d" % (who, f, weight.shape[2]))
    return f


_POOL_F32_ONLY = "%s: bfloat16 parameters are not supported (run the layer, then gcn_pool / gcn_pool_4)"     # the pooled entries' refusal


def _series_pool_checks(who, series, weight, pool, stride, padding, dilation):
    """what the four pooled entries ask of their arguments behind the parameters' dtype (_POOL_F32_ONLY; the one-launch entry has its own
    rule), in this order, before anything is built or launched: ranks and channels, the pool, the geometry
    -> (pool, (stride, left, right, dilation))"""
    _series_shape_check(who, series, weight)
    pool = check_pool(pool, series.shape[1], who)
    H = weight.shape[1]
    return pool, series_geometry(series.shape[2], H, stride, padding, who, dilation)[:3] + (series_dilation(H, dilation),)


def _series_pool_tensors(series, weight, bias):
    """the accepted tensors of a pooled entry -> (series, weight) on the device and 4-D, and need_idx: grad mode and a leaf that trains"""
    _lib.require_device(series, weight, bias)
    need_idx = torch.is_grad_enabled() and (series.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad))
    if series.dim() == 3:
        series, weight = series.unsqueeze(3), weight.unsqueeze(2)
    return series, weight, need_idx


def _in_operand_labels(op, layer, series, bias, bias_kind):
    """layer(series, bias) -> out around a reordered operand: the rows of the series and of a per-vertex bias to the operand's labels, the
    output's back to the caller's (the vertex axis is dim 1 in every layout); a plain operand calls the layer as it is"""
    series, bias = _to_operand_labels(op, series, bias, bias_kind)
    out = layer(series, bias)
    return out if op.perm is None else relabel_rows(out, op.inv_perm, op.perm)


def _series_pool_unfused(op, layer, series, bias, bias_kind, pool, drop):
    """what a pooled entry runs where series_pool_is_fused says no: the unpooled layer in the operand's labels, relabelled back, then relu
    (+ dropout, drop = (seed tensor, thr, scale)) + pool as one pass on a view"""
    y = _in_operand_labels(op, layer, series, bias, bias_kind)
    return _relu_pool_view(y, pool) if drop is None else _relu_dropout_pool_view(y, pool, *drop)


# ---- dropout between relu and the pool ("dropout in the relu + pool epilogue")
def _f32(v):
    """v rounded to float32, as a Python float"""
    return struct.unpack("f", struct.pack("f", v))[0]


def dropout_params(p, who="dropout"):
    """(thr, scale) of the mask for a drop probability p, a real number in [0, 1): element e is kept iff its Philox word is >= thr =
    min(floor(p * 2^32 + 0.5), 2^32 - 1), and a kept value is multiplied by scale = float32(1) / (float32(1) - float32(p)) -- the float32
    operations, carried out in double precision and rounded once each (a difference of two float32 is exact there, and a quotient of two
    float32 rounds to float32 the same way from 53 bits as from the exact value)."""
    if not isinstance(p, numbers.Real) or isinstance(p, bool) or not 0.0 <= p < 1.0 or _f32(p) >= 1.0:      # float32(p) == 1: no finite scale
        raise _lib.TgcnError("%s: p is a real number in [0, 1) (in float32), got %r" % (who, p))
    p = float(p)
    thr = min(int(math.floor(p * 4294967296.0 + 0.5)), 4294967295)
    return thr, _f32(1.0 / _f32(1.0 - _f32(p)))


def dropout_seed(seed, device, who="dropout", draw=True):
    """the mask's seed as the kernels read it -- a one-element int64 tensor on `device` holding 0 <= seed < 2^62: None draws one there with
    torch.randint (it follows torch.manual_seed and is legal inside a hipGraph capture; draw=False only checks and returns None), an int is
    copied there, a tensor is checked (int64, one element, on the device; its VALUE is the caller's to keep in range -- reading it would
    synchronise) and used as it is.  TgcnError for anything else."""
    if seed is None:
        return torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=device) if draw else None
    if isinstance(seed, torch.Tensor):
        if seed.dtype != torch.int64 or seed.numel() != 1 or seed.device != torch.device(device):
            raise _lib.TgcnError("%s: a seed tensor is one int64 element on the input's device %s, got %s %s on %s"
                                 % (who, device, tuple(seed.shape), seed.dtype, seed.device))
        return seed.reshape(1) if draw else None
    if not isinstance(seed, numbers.Integral) or isinstance(seed, bool) or not 0 <= seed < 2 ** 62:
        raise _lib.TgcnError("%s: seed is None, an integer in [0, 2^62) or a one-element int64 tensor, got %r" % (who, seed))
    return torch.tensor([int(seed)], dtype=torch.int64, device=device) if draw else None


@_on_device
def _dropout_keep(seed_t, e0, count, thr):
    out = torch.empty(count, dtype=torch.uint8, device=seed_t.device)
    _lib.check(_lib.lib().tgcn_dropout_keep_u8(_lib.stream_ptr(), _lib.ptr(seed_t), e0, count, thr, _lib.ptr(out)))
    return out.bool()


def dropout_keep_mask(seed, e0, count, p, device):
    """bool tensor of `count` elements on `device`: True where the elements e0 .. e0 + count - 1 are kept at drop probability p under `seed`
    (tgcn_dropout_keep_u8) -- the mask cheb_series_relu_dropout_pool and cheb_relu_dropout_pool apply, by element index in the caller's
    vertex labels: ((s * nwin + w) * n + v) * N + c for the streaming layers, (q * n + v) * N + c for the batch layers."""
    who = "dropout_keep_mask"
    thr, _ = dropout_params(p, who)
    if not all(isinstance(v, numbers.Integral) and not isinstance(v, bool) for v in (e0, count)) or e0 < 0 or count < 1 or e0 + count > 2 ** 63 - 1:
        raise _lib.TgcnError("%s: e0 >= 0 and count >= 1 are integers below 2^63, got %r and %r" % (who, e0, count))
    seed_t = dropout_seed(seed, torch.device(device), who)
    _lib.require_device(seed_t)
    return _dropout_keep(seed_t, int(e0), int(count), thr)


class ReluDropoutPoolFn(torch.autograd.Function):
    """z = max over `pool` consecutive vertices of relu(y) * mask as its own pass (tgcn_relu_dropout_pool_f32 / tgcn_relu_pool_bwd_f32 on
    gz * scale): y (q, n, f) with f = nw * N columns per vertex, column cc = window cc / N, channel cc % N."""

    @staticmethod
    @_on_device
    def forward(ctx, y, pool, N, seed_t, thr, scale):
        _lib.require_device(y, seed_t)
        y = y.float().contiguous()
        q, n, f = y.shape
        assert n % pool == 0 and f % N == 0, "pooling needs n divisible by the pool size and whole windows of N columns"
        z = torch.empty((q, n // pool, f), dtype=torch.float32, device=y.device)
        idx = torch.empty((q, n // pool, f), dtype=torch.uint8, device=y.device)
        _lib.check(_lib.lib().tgcn_relu_dropout_pool_f32(_lib.stream_ptr(), _lib.ptr(y), _lib.ptr(z), _lib.ptr(idx), q, n, f, pool, N,
                                                         _lib.ptr(seed_t), thr, scale))
        ctx.save_for_backward(z, idx)
        ctx.shape, ctx.pool, ctx.scale = (q, n, f), pool, scale
        return z

    @staticmethod
    @_on_device
    def backward(ctx, gz):
        z, idx = ctx.saved_tensors
        q, n, f = ctx.shape
        gy = torch.empty((q, n, f), dtype=torch.float32, device=gz.device)
        _lib.check(_lib.lib().tgcn_relu_pool_bwd_f32(_lib.stream_ptr(), _lib.ptr((gz.float() * ctx.scale).contiguous()), _lib.ptr(z), _lib.ptr(idx),
                                                     _lib.ptr(gy), q, n, f, ctx.pool))
        return gy, None, None, None, None, None


def _relu_dropout_pool_view(y, pool, seed_t, thr, scale):
    """_relu_pool_view with the mask: (q, n, N) as it is, (S, n, nwin, N) through its (S, n, nwin*N) view -- one element index for both"""
    if y.dim() == 3:
        return ReluDropoutPoolFn.apply(y, pool, y.shape[2], seed_t, thr, scale)
    S, n, nwin, N = y.shape
    return ReluDropoutPoolFn.apply(y.reshape(S, n, nwin * N), pool, N, seed_t, thr, scale).view(S, n // pool, nwin, N)


@_on_device
def cheb_time_windows_relu_dropout_pool(op, series, weight, bias, bias_kind, mode, pool, p, seed, as_series=False, stride=1, padding=0, dilation=1):
    """gcn_pool_4(dropout(relu(cheb_time_windows(...)), p)) -- the reference's training pattern -- with relu, the dropout and the max over
    `pool` consecutive vertices in the projection's epilogue: cheb_time_windows_relu_pool's arguments, shapes and refusals, then
    p, a real number in [0, 1), and seed: None (drawn on the series' device with torch.randint: follows torch.manual_seed, legal in a
    capture), an integer in [0, 2^62) or a one-element int64 tensor on the series' device (read by the kernel: rewrite it between the
    replays of a captured step).  The mask is a pure function of (seed, element index in the caller's vertex labels) -- dropout_keep_mask
    reproduces it -- so nothing of the full output's size is allocated, no mask is stored, and both layouts and a reordered operand drop the
    same elements; values and gradients are bit-identical to ReluPoolFn on relu(y) * mask.  p == 0 is cheb_time_windows_relu_pool itself.
    A reordered operand runs the layer, relabels back, then tgcn_relu_dropout_pool_f32 on a view."""
    who = "cheb_time_windows_relu_dropout_pool"
    thr, scale = dropout_params(p, who)
    dropout_seed(seed, series.device, who, draw=False)
    if p == 0:
        return cheb_time_windows_relu_pool(op, series, weight, bias, bias_kind, mode, pool, as_series=as_series, stride=stride, padding=padding,
                                           dilation=dilation)
    return _series_relu_pool(who, op, series, weight, bias, bias_kind, mode, pool, as_series, stride, padding, dilation, seed, thr, scale)


def check_time_chunk(time_chunk, stride, padding, bf16, who="cheb_time_windows"):
    """what time_chunk= asks of a streaming call, checked before an operand is built: None (no chunks: today's call) or an integer >= 1,
    padding="causal" (the zero ring is that padding), stride=1 and float32 parameters.  -> the chunk length or None"""
    if time_chunk is None:
        return None
    if not isinstance(time_chunk, numbers.Integral) or isinstance(time_chunk, bool) or time_chunk < 1:
        raise _lib.TgcnError("%s: time_chunk is None or an integer >= 1, got %r" % (who, time_chunk))
    if not (isinstance(padding, str) and padding == "causal"):
        raise _lib.TgcnError('%s: time_chunk runs with padding="causal" only (the chunks pass through the streaming ring), got padding=%r'
                             % (who, padding))
    if not isinstance(stride, numbers.Integral) or isinstance(stride, bool) or stride != 1:
        raise _lib.TgcnError("%s: time_chunk runs at stride=1 only, got stride=%r" % (who, stride))
    if bf16:
        raise _lib.TgcnError("%s: time_chunk runs in float32 only -- the parameters are bfloat16" % who)
    return int(time_chunk)


@_on_device
def _chunk_stack(op, x, t0, tc, K, mode):
    """the hop stack (K, S, n, tc*f) of time rows [t0, t0 + tc) of a contiguous series (S, n, T, f) in the operand's labels: K - 1 hops on rows
    of tc*f floats, as _stream_chunk's"""
    S, n, _, f = x.shape
    x3 = x[:, :, t0:t0 + tc].reshape(S, n, tc * f)       # a view (time and channel merge); the stack's term 0 is the contiguous copy
    return _series_stack(op, x3, K, mode)


class ChebSeriesChunkFn(torch.autograd.Function):
    """ChebSeriesFn on a causal series at stride 1, time_chunk rows at a time (DESIGN.md 3.10 "Time chunks"): checkpointing in time on the
    streaming ring.  Same output and the exact gradients, but nothing of the hop stack's size (K, S, n, T*f) is held in either direction:
    the forward keeps the relabelled series and the working weight, not the stack.
    forward: the step-1 plan once, a zero ring (SeriesStreamState, host head: the causal padding), then per chunk the K - 1 hops on rows of
    Tc*f floats and tgcn_cheb_project_series_stream_at_f32, which projects the chunk through the ring into rows [t0, t0 + Tc) of the whole
    output (either layout) and updates the ring.
    backward: a second pass in forward time order from a zero ring.  Per chunk the hops again (the same values, so the same ring) if the
    weight needs a gradient, one tgcn_cheb_series_chunk_backward_f32 call -- the chunk's G (K, S, n, Tc*f) from g rows [t0, t0 + Tc + C)
    read in place, and / or the dW of the windows that end in the chunk from the ring and the chunk's stack, then the ring update -- and
    _adjoint_hops on G into d series[:, :, t0:t0 + Tc].  dW is summed over the chunks in fp32 in chunk order (a re-run is bit-identical)
    and un-folded once.  A frozen weight: no second hop pass and no ring; a series without grad: no G and no adjoint hops."""

    @staticmethod
    @_on_device
    def forward(ctx, series, weight_khfg, bias, op, mode, bias_kind, as_series, dil, time_chunk):
        L = _lib.lib()
        S, n, T, f = series.shape
        K, H, _, N = weight_khfg.shape
        hc, lds = C.c_int32(0), C.c_int32(0)
        _lib.check(L.tgcn_series_conv_plan(H, f, N, int(f % 4 == 0), 1, C.byref(hc), C.byref(lds)))
        x, fold, Wt, b = _series_operands(series, weight_khfg, bias, mode)
        state = SeriesStreamState(op, torch.float32, S, n, f, K, H, dil, x.device)
        out = torch.empty((S, n, T, N) if as_series else (S * T, n, N), dtype=torch.float32, device=x.device)
        for t0, tc in _time_chunks(T, time_chunk):
            stack = _chunk_stack(op, x, t0, tc, K, mode)
            _lib.check(L.tgcn_cheb_project_series_stream_at_f32(_lib.stream_ptr(), S, n, tc, f, H, N, K, _lib.ptr(stack), _lib.ptr(Wt), _lib.ptr(b),
                                                                bias_kind, _lib.ptr(out), T, t0, 1 if as_series else 0, _lib.ptr(state.ring),
                                                                state.ring_ld, state.head, dil))
            state.advance(tc)
            stack = None        # released before the next chunk's is allocated: one chunk tensor at a time
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, Wt)
        _series_ctx(ctx, op, mode, fold, bias, bias_kind, as_series, (S, n, T, f, H, N, K, dil, time_chunk))
        return out

    @staticmethod
    @_on_device
    def backward(ctx, g):
        x, Wt = ctx.saved_tensors
        T, time_chunk = ctx.dims[2], ctx.dims[8]
        g = _aligned_input(g.float().contiguous())
        gx = dW = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            opT, state, gx = _chunk_backward_start(ctx, g.device)
            for t0, tc in _time_chunks(T, time_chunk):
                dW = _chunk_backward_step(ctx, x, Wt, opT, state, g, T, t0, t0, tc, gx, dW)     # g rows [t0, t0 + tc + C) read in place
            if dW is not None:
                dW = _series_dW(ctx, dW)
        gb = None
        if ctx.bias_shape is not None and ctx.needs_input_grad[2]:
            gb = _series_bias_grad(g, ctx.as_series, ctx.bias_kind, ctx.bias_shape)
        return gx, dW, gb, None, None, None, None, None, None


def _time_chunks(T, time_chunk):
    """(t0, tc) of the chunks a walk over T time rows takes, in time order: time_chunk rows each, the last one what is left"""
    return ((t0, min(time_chunk, T - t0)) for t0 in range(0, T, time_chunk))


def _chunk_backward_start(ctx, device):
    """what a backward walk carries from chunk to chunk -> (the transposed operand, a zero ring, d series): the first and the last only
    when the series needs a gradient, the ring only when the weight does (its dW reads the forward's ring)"""
    S, n, T, f, H, N, K, dil, _ = ctx.dims
    need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    return (ctx.op.transpose() if need_x else None,
            SeriesStreamState(ctx.op, torch.float32, S, n, f, K, H, dil, device) if need_w else None,
            torch.empty((S, n, T, f), dtype=torch.float32, device=device) if need_x else None)


def _chunk_backward_step(ctx, x, Wt, opT, state, g, g_T, g_t0, t0, tc, gx, dW):
    """One chunk of a backward walk, rows [t0, t0 + tc) of the series x: the hops again if the weight trains (state is not None), one
    tgcn_cheb_series_chunk_backward_f32 call on the output gradient g of g_T time rows with the chunk's first at row g_t0, the ring's
    advance, and the adjoint hops into gx[:, :, t0:t0 + tc] if the series needs a gradient (opT is not None).  -> dW plus the chunk's, summed
    in fp32 in chunk order.  The chunk's stack, G, dWc and workspace are this call's locals: none outlives its chunk."""
    S, n, T, f, H, N, K, dil, _ = ctx.dims
    L = _lib.lib()
    need_x, need_w = opT is not None, state is not None
    stack = _chunk_stack(ctx.op, x, t0, tc, K, ctx.mode) if need_w else None
    G = torch.empty((K, S, n, tc * f), dtype=torch.float32, device=g.device) if need_x else None
    dWc = torch.empty((K, H * f, N), dtype=torch.float32, device=g.device) if need_w else None
    ws = _workspace(L.tgcn_cheb_series_chunk_backward_workspace_bytes(S, n, tc, f, H, N, K, dil), g.device, floor=16)
    _lib.check(L.tgcn_cheb_series_chunk_backward_f32(_lib.stream_ptr(), S, n, tc, f, H, N, K, _lib.ptr(stack),
                                                     _lib.ptr(state.ring) if need_w else None, state.ring_ld if need_w else 0,
                                                     state.head if need_w else 0, _lib.ptr(g), g_T, g_t0, 1 if ctx.as_series else 0,
                                                     _lib.ptr(Wt) if need_x else None, _lib.ptr(G), _lib.ptr(dWc), _lib.ptr(ws), ws.numel(), dil))
    if need_w:
        state.advance(tc)
        dW = dWc if dW is None else dW.add_(dWc)
    if need_x:
        gx[:, :, t0:t0 + tc] = _adjoint_hops(opT, G, ctx.mode).view(S, n, tc, f)
    return dW


class ChebSeriesChunkReluPoolFn(torch.autograd.Function):
    """ChebSeriesChunkFn's walk with relu, dropout and the vertex max-pool in the projection's epilogue (DESIGN.md 3.10 "Time chunks through
    the pooled epilogue"): z = max over `pool` consecutive vertices of relu(y) * mask of the causal layer at step 1, time_chunk rows at a time
    in both directions.  Neither the hop stack (K, S, n, T*f) nor the layer's output (S, n, T, N) nor that output's gradient is ever
    allocated: the step holds z, idx and chunk-sized buffers.
    forward: tgcn_series_pool_plan once, a zero ring, then per chunk the K - 1 hops and tgcn_cheb_project_series_stream_pool_at_f32, which
    writes the chunk's pooled rows (and arg-max bytes, need_idx) into rows [t0, t0 + Tc) of the whole z and updates the ring.  seed_t None:
    no mask.  The mask's element index is taken at the absolute window, so the chunking does not change which elements drop.
    backward, per chunk in forward time order, C = (H-1)*dilation: ONE slab of rows = min(Tc + C, T - t0) time rows of the output gradient
    (tgcn_relu_pool_bwd_rows_f32: gz * scale to the arg-max vertex where z > 0), the hops again if the weight trains, one
    tgcn_cheb_series_chunk_backward_f32 call on the slab (g_T = rows, g_t0 = 0: the same launch over the same rows as ChebSeriesChunkFn's on
    the whole gradient), the ring's advance, the adjoint hops into d series[:, :, t0:t0 + Tc].  dW is summed in chunk order and un-folded
    once.  The bias gradient is summed per chunk from slab rows [0, Tc) only -- the C halo rows are the next chunk's first rows and are
    counted there.  The one-sided forms skip what ChebSeriesChunkFn's skip.  Saves the series (only if the weight trains), the working
    weight, z and idx."""

    @staticmethod
    @_on_device
    def forward(ctx, series, weight_khfg, bias, op, mode, bias_kind, as_series, dil, time_chunk, pool, need_idx, seed_t, thr, scale):
        L = _lib.lib()
        S, n, T, f = series.shape
        K, H, _, N = weight_khfg.shape
        hc, lds = C.c_int32(0), C.c_int32(0)
        _lib.check(L.tgcn_series_pool_plan(H, f, N, int(f % 4 == 0), 1, pool, C.byref(hc), C.byref(lds)))
        x, fold, Wt, b = _series_operands(series, weight_khfg, bias, mode)
        state = SeriesStreamState(op, torch.float32, S, n, f, K, H, dil, x.device)
        shape = (S, n // pool, T, N) if as_series else (S * T, n // pool, N)
        z = torch.empty(shape, dtype=torch.float32, device=x.device)
        idx = torch.empty(shape, dtype=torch.uint8, device=x.device) if need_idx else None
        for t0, tc in _time_chunks(T, time_chunk):
            stack = _chunk_stack(op, x, t0, tc, K, mode)
            _lib.check(L.tgcn_cheb_project_series_stream_pool_at_f32(_lib.stream_ptr(), S, n, tc, f, H, N, K, _lib.ptr(stack), _lib.ptr(Wt), _lib.ptr(b),
                                                                     bias_kind, _lib.ptr(z), _lib.ptr(idx), pool, T, t0, 1 if as_series else 0,
                                                                     _lib.ptr(state.ring), state.ring_ld, state.head, dil, _lib.ptr(seed_t), thr, scale))
            state.advance(tc)
            stack = None        # released before the next chunk's is allocated: one chunk tensor at a time
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, Wt, z, idx)
        ctx.pool, ctx.scale, ctx.seed = pool, scale, seed_t
        _series_ctx(ctx, op, mode, fold, bias, bias_kind, as_series, (S, n, T, f, H, N, K, dil, time_chunk))
        return z

    @staticmethod
    @_on_device
    def backward(ctx, gz):
        x, Wt, z, idx = ctx.saved_tensors
        S, n, T, f, H, N, K, dil, time_chunk = ctx.dims
        if idx is None:
            raise _lib.TgcnError("cheb_time_windows_relu_pool_chunked: the forward ran without grad mode and kept no arg-max")
        L = _lib.lib()
        gz = gz.float().contiguous()
        need_b = ctx.bias_shape is not None and ctx.needs_input_grad[2]
        Cr = (H - 1) * dil
        dW = gb = None
        opT, state, gx = _chunk_backward_start(ctx, gz.device)
        for t0, tc in _time_chunks(T, time_chunk):
            rows = min(tc + Cr, T - t0)
            slab = torch.empty((S, n, rows, N) if ctx.as_series else (S * rows, n, N), dtype=torch.float32, device=gz.device)
            _lib.check(L.tgcn_relu_pool_bwd_rows_f32(_lib.stream_ptr(), _lib.ptr(gz), _lib.ptr(z), _lib.ptr(idx), _lib.ptr(slab), S, n, T, t0, rows, N,
                                                     ctx.pool, 1 if ctx.as_series else 0, ctx.scale))
            if opT is not None or state is not None:
                dW = _chunk_backward_step(ctx, x, Wt, opT, state, slab, rows, 0, t0, tc, gx, dW)      # the slab is the whole gradient it reads
            if need_b:      # rows [0, tc) only: the halo rows are the next chunk's own
                own = slab[:, :, :tc] if ctx.as_series else slab.view(S, rows, n, N)[:, :tc]
                if ctx.bias_kind == BIAS_CHANNEL:
                    part = own.sum(dim=(0, 1, 2))
                else:
                    part = own.sum(dim=(0, 2)) if ctx.as_series else own.sum(dim=(0, 1))
                gb = part if gb is None else gb.add_(part)
            slab = own = None      # released before the next chunk's is allocated: one slab at a time (own is a view of it)
        if dW is not None:
            dW = _series_dW(ctx, dW)
        if gb is not None:
            gb = gb.reshape(ctx.bias_shape)
        return (gx, dW, gb) + (None,) * 11


@_on_device
def cheb_time_windows_relu_pool_chunked(op, series, weight, bias, bias_kind, mode, pool, time_chunk, p=0.0, seed=None, as_series=False, dilation=1):
    """gcn_pool_4(dropout(relu(cheb_time_windows(..., padding="causal", dilation=dilation, time_chunk=time_chunk)), p)) with relu, the dropout
    and the max over `pool` consecutive vertices in the projection's epilogue AND the walk in time chunks (ChebSeriesChunkReluPoolFn): the
    two memory features of the streaming layers in one call.  series (S, n, T) with weight (K, H, N), or (S, n, T, f) with (K, H, f, N)
    -> z (S*T, n/pool, N) or, as_series=True, (S, n/pool, T, N).  The geometry is always the causal layer at step 1 -- what the streaming
    ring implements -- so there is no stride and no padding.  Nothing of the size of the hop stack, of the layer's output or of that
    output's gradient is allocated in either direction; the price is time_chunk's own (a second hop pass when the weight trains, and
    (H-1)*dilation re-routed gradient rows per chunk).
    p == 0: relu + pool without a mask.  Otherwise the mask, its seed and its element index are cheb_time_windows_relu_dropout_pool's with
    nwin = T, e = ((s*T + t)*n + v)*N + c in the caller's vertex labels: dropout_keep_mask reproduces it, and the chunk length does not
    change which elements drop.  z, d series and dW are bit-identical to the composition at the same time_chunk; d bias is summed chunk by
    chunk and agrees to rounding.
    A reordered operand (series_pool_is_fused(op) False) runs cheb_time_windows(time_chunk=...), relabels back, then the relu (+ dropout) +
    pool pass: the same values and the same mask, but the layer's output is allocated -- the memory saving is absent there.
    TgcnError before an operand is built: bfloat16 parameters, a bad pool, p, seed or time_chunk, n % pool != 0."""
    who = "cheb_time_windows_relu_pool_chunked"
    thr, scale = dropout_params(p, who)
    dropout_seed(seed, series.device, who, draw=False)
    if param_dtype(weight, bias, who) == BF16:
        raise _lib.TgcnError(_POOL_F32_ONLY % who)
    if time_chunk is None:
        raise _lib.TgcnError("%s: time_chunk is None or an integer >= 1, got None -- without chunks this is cheb_time_windows_relu_pool / "
                             "cheb_time_windows_relu_dropout_pool" % who)
    time_chunk = check_time_chunk(time_chunk, 1, "causal", False, who)
    pool, geom = _series_pool_checks(who, series, weight, pool, 1, "causal", dilation)
    series, weight, need_idx = _series_pool_tensors(series, weight, bias)
    seed_t = dropout_seed(seed, series.device, who) if p != 0 else None       # (p == 0: thr = 0 and scale = 1 already)
    if not series_pool_is_fused(op, pool):
        return _series_pool_unfused(op, lambda s, b: ChebSeriesChunkFn.apply(s, weight, b, op, mode, bias_kind, bool(as_series), geom[3], time_chunk),
                                    series, bias, bias_kind, pool, None if seed_t is None else (seed_t, thr, scale))
    return ChebSeriesChunkReluPoolFn.apply(series, weight, bias, op, mode, bias_kind, bool(as_series), geom[3], time_chunk, pool, need_idx, seed_t,
                                           thr, scale)


# fused="auto" fuses the shape classes listed here.  A call's class is what its UNFUSED form would be: "windows_f1" -- a single channel,
# window-major, stride 1, no padding, dilation 1: the scalar-load form (ChebWindowsFn) -- or "series", every other call (the MFMA series
# kernels, ChebSeriesFn).  Set from profiles/r21_series_small.json (DESIGN.md 3.10 "One launch per series"): a class is listed only where the
# fused median lies below the unfused median of the same commit by more than the larger of the two spreads.  "windows_f1" does on both
# measured operands, forward and forward + backward (148 parcels: 0.498 against 0.572 ms and 1.01 against 15.0 ms; the 28 x 28 grid: 0.456
# against 0.495 ms and 1.86 against 35.0 ms; spreads under 0.02 ms but the last, 0.45); "series" does not (148 parcels as a series: 0.497
# against 0.273 ms).  () would be "never".
SERIES_FUSED_AUTO = ("windows_f1",)


def check_series_fused(fused, stride, time_chunk, bf16, who="cheb_time_windows"):
    """what fused= asks of a whole-series call that needs no operand, checked before one is built: False, True or "auto"; fused=True runs in
    float32 at stride=1 without time_chunk.  -> fused"""
    if fused is not False and fused is not True and not (isinstance(fused, str) and fused == "auto"):
        raise _lib.TgcnError("%s: fused is False, True or \"auto\", got %r" % (who, fused))
    if fused is True:
        if bf16:
            raise _lib.TgcnError("%s: fused=True runs in float32 only -- the parameters are bfloat16 (fused=False or \"auto\")" % who)
        if not isinstance(stride, numbers.Integral) or isinstance(stride, bool) or stride != 1:
            raise _lib.TgcnError("%s: fused=True has no window step -- the one-launch layer runs at stride=1, got stride=%r (fused=False or "
                                 "\"auto\")" % (who, stride))
        if time_chunk is not None:
            raise _lib.TgcnError("%s: fused=True does not walk time chunks (time_chunk=%r): a workgroup keeps its span in LDS and nothing of "
                                 "the stack's size exists unless the weight trains (fused=False or \"auto\")" % (who, time_chunk))
    return fused


def _series_small_plan(op, f, H, N, K, T, left, right, dilation, mode):
    """tgcn_cheb_series_small_plan on a square operand -> (rc, tb, dense, lds_bytes)"""
    tb, dense, lds = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = _lib.lib().tgcn_cheb_series_small_plan(op.n, op.nnz, int(mode), int(f), int(H), int(N), int(K), int(T), int(left), int(right),
                                                int(dilation), C.byref(tb), C.byref(dense), C.byref(lds))
    return rc, tb.value, dense.value, lds.value


def series_fused_supported(op, f, H, N, K, T, padding, dilation, mode):
    """True where cheb_time_windows(..., fused=True) runs a float32 series of T time rows on this operand at stride 1: a square operand in
    its own labels (op.perm is None), a legal padding / dilation and a plan that accepts (tgcn_cheb_series_small_plan: operand and span
    buffers in one workgroup's LDS).  A host query: nothing launches."""
    if op.n_cols != op.n or op.perm is not None or min(f, H, N, K, T) < 1:
        return False
    try:
        _, left, right, _ = series_geometry(T, H, 1, padding, "series_fused_supported", dilation)
    except _lib.TgcnError:
        return False
    return _series_small_plan(op, f, H, N, K, T, left, right, series_dilation(H, dilation), mode)[0] == 0


def _series_fused_auto(f, as_series, geom):
    """the measured rule of fused="auto": the class of the call's unfused form is listed in SERIES_FUSED_AUTO"""
    return ("windows_f1" if (f == 1 and not as_series and tuple(geom) == (1, 0, 0, 1)) else "series") in SERIES_FUSED_AUTO


def _series_fused_route(op, fused, bf16, time_chunk, geom, as_series, f, H, N, K, T, mode):
    """whether a call with fused=True / "auto" takes the one-launch layer.  True: TgcnError for an operand or a plan that cannot; "auto":
    False for those, for what check_series_fused refuses and outside the measured rule (asked first: no query is made for a class that never
    fuses)"""
    stride, left, right, dil = geom
    if fused is True:
        if op.n_cols != op.n:
            raise _lib.TgcnError("cheb_time_windows: fused=True needs a square operand, got %d x %d" % (op.n, op.n_cols))
        if op.perm is not None:
            raise _lib.TgcnError("cheb_time_windows: fused=True runs in the operand's own labels -- a reordered operand is not supported "
                                 "(fused=False or \"auto\")")
        if _series_small_plan(op, f, H, N, K, T, left, right, dil, mode)[0] != 0:
            raise _lib.TgcnError("cheb_time_windows: fused=True, but n = %d, nnz = %d, f = %d, H = %d, N = %d do not fit the one-launch layer "
                                 "(series_fused_supported; fused=False or \"auto\")" % (op.n, op.nnz, f, H, N))
        return True
    return (not bf16 and time_chunk is None and stride == 1 and op.n_cols == op.n and op.perm is None and _series_fused_auto(f, as_series, geom)
            and _series_small_plan(op, f, H, N, K, T, left, right, dil, mode)[0] == 0)


class ChebSeriesSmallFn(torch.autograd.Function):
    """ChebSeriesFn at stride 1 on an operand that fits in LDS, the forward in ONE launch (tgcn_cheb_series_small_f32, csrc/series_small.h;
    DESIGN.md 3.10 "One launch per series"): the fold in power mode with K > 2, then the fused entry on the series itself -- hops, window
    projection and bias of a tile of windows per workgroup.  The hop stack (K, S, n, T*f) is allocated and written by that launch only when
    the weight needs a gradient (need_stack, the caller's look at grad mode); otherwise nothing of size K*T exists.  The backward is ChebSeriesFn's (_series_backward: the existing
    backward entry of the geometry on the fused forward's stack, _adjoint_hops for the input gradient).  geom = (1, left, right, dilation)."""

    @staticmethod
    @_on_device
    def forward(ctx, series, weight_khfg, bias, op, mode, bias_kind, as_series, geom, need_stack):
        L = _lib.lib()
        S, n, T, f = series.shape
        K, H, _, N = weight_khfg.shape
        _, left, right, dil = geom
        nwin = T + left + right - (H - 1) * dil
        x, fold, Wt, b = _series_operands(series, weight_khfg, bias, mode)
        out = torch.empty((S, n, nwin, N) if as_series else (S * nwin, n, N), dtype=torch.float32, device=x.device)
        stack = torch.empty((K, S, n, T * f), dtype=torch.float32, device=x.device) if need_stack else None
        _lib.check(L.tgcn_cheb_series_small_f32(_lib.stream_ptr(), C.byref(op.struct), int(mode), S, T, f, H, N, K, _lib.ptr(x), _lib.ptr(Wt),
                                                _lib.ptr(b), bias_kind, 1 if as_series else 0, _lib.ptr(out), _lib.ptr(stack), left, right, dil))
        ctx.save_for_backward(Wt)
        ctx.stack = stack
        _series_ctx(ctx, op, mode, fold, bias, bias_kind, as_series, (S, n, T, f, H, N, K), (1, left, right, dil))
        return out

    @staticmethod
    @_on_device
    def backward(ctx, g):
        return _series_backward(ctx, ctx.saved_tensors[0], g) + (None,) * 6


def cheb_time_windows(op, series, weight, bias, bias_kind, mode=MODE_POWER, as_series=False, stride=1, padding=0, dilation=1, time_chunk=None,
                      fused=False):
    """Streaming form of TGCNCheb_H / ChebTimeConv on sliding windows: series (S, n, T) raw recordings with weight (K, H, N), or
    (S, n, T, f) with weight (K, H, f, N), in the reference basis.  Returns (S * (T-H+1), n, N), identical to running the layer on the
    windowed batch x[s*(T-H+1) + w, i, h, c] = series[s, i, w + h, c] (load/data_hcp.py:146-152), but the K-1 hops run once on the T time
    rows of each recording -- in the backward too, so the windows it replaces can be trained through.
    as_series=True returns the same numbers as (S, n, T-H+1, N), contiguous: itself a series, which the next time layer streams over.
    A single-channel series with as_series=False takes the scalar-load form (ChebWindowsFn, one projection launch per recording); every
    other call the sliding-window MFMA kernels (ChebSeriesFn, one launch for all recordings).
    stride, padding: the layer as a convolution over time.  padding = p, (left, right) or "causal" (= (H-1, 0)) puts that many zero time rows
    (at most H-1 each) around every recording, stride keeps every stride-th window: nwin = (T + left + right - H) // stride + 1 windows,
    xw[s*nwin + w, i, h, c] = padded_series[s, i, w*stride + h, c], out (S*nwin, n, N) or (S, n, nwin, N).  The hops do not depend on either;
    the projection and its gradients shrink with the stride.  Anything but stride=1, padding=0 runs the MFMA kernels, f == 1 included.
    dilation: the H taps of a window lie that many time rows apart, xw[s*nwin + w, i, h, c] = padded_series[s, i, w*stride + h*dilation, c];
    the window spans He = (H-1)*dilation + 1 rows, and He replaces H in the padding rules ("causal" = (He-1, 0)) and in nwin.  dilation > 1
    runs at stride 1 only (TgcnError otherwise) through the _dilated entries, f == 1 included; a chain with dilations 1, 2, 4, ... sees
    exponentially many time steps with a few taps per layer.  A one-tap layer (H == 1) has nothing to dilate and makes the calls of dilation 1.
    bfloat16 parameters take ChebSeriesBf16Fn (bf16 series, stack and output, fp32 sums) for every call but the scalar-load form; that one, and
    a series that is not bfloat16 itself, raise TgcnError before anything is built (check_series_bf16).
    time_chunk=Tc (an integer >= 1; None: everything above, call for call) returns the same tensor with the same autograd behaviour, but walks
    the recording Tc time rows at a time through the streaming ring in both directions (ChebSeriesChunkFn; the last chunk is shorter, Tc >= T
    is one chunk): nothing of size K*T is allocated in the forward or the backward, at the price of a third hop pass when the weight trains.
    It runs the causal layer at step 1 -- padding="causal", stride=1, any dilation, float32 parameters, either layout, a single channel on
    the general kernels -- and anything else raises TgcnError before an operand is built (check_time_chunk).  The causal result holds a row
    for every time step; the windows that lie wholly inside the recording (padding=0) are out[:, :, He-1:] of it.
    fused=True runs the forward of a layer in ONE launch on an operand that fits in LDS (ChebSeriesSmallFn, tgcn_cheb_series_small_f32:
    hops, window projection and bias per tile of windows; the stack for the backward is written by the same launch, and only when the weight
    trains): float32 parameters, stride=1, no time_chunk, any legal padding and dilation, either layout, a single channel included.  It
    raises TgcnError before anything launches for bfloat16 parameters, stride > 1, a time_chunk, a non-square or reordered operand and a
    plan that refuses (series_fused_supported tells).  fused="auto" fuses where all of that holds and SERIES_FUSED_AUTO says it pays, and
    is the fused=False call everywhere else.  Fused and unfused results agree to rounding (a hop adds its neighbours in another order)."""
    bf16 = param_dtype(weight, bias, "cheb_time_windows") == BF16
    fused = check_series_fused(fused, stride, time_chunk, bf16)
    time_chunk = check_time_chunk(time_chunk, stride, padding, bf16)
    f = _series_shape_check("cheb_time_windows", series, weight)
    geom = series_geometry(series.shape[2], weight.shape[1], stride, padding, dilation=dilation)[:3] + (series_dilation(weight.shape[1], dilation),)
    if bf16:
        check_series_bf16(f, as_series, geom, series.dtype)
    if fused is not False:
        fused = _series_fused_route(op, fused, bf16, time_chunk, geom, bool(as_series), f, weight.shape[1], weight.shape[-1], weight.shape[0], series.shape[2], mode)
    _lib.require_device(series, weight, bias)
    if not (fused or bf16) and time_chunk is None and f == 1 and not as_series and geom == (1, 0, 0, 1):      # the scalar-load form, on 3-D tensors
        if series.dim() == 4:
            series, weight = series.reshape(series.shape[:3]), weight.reshape(weight.shape[0], weight.shape[1], weight.shape[3])
        return _in_operand_labels(op, lambda s, b: ChebWindowsFn.apply(s, weight, b, op, mode, bias_kind), series, bias, bias_kind)
    if series.dim() == 3:
        series, weight = series.unsqueeze(3), weight.unsqueeze(2)
    if fused:
        need_stack = torch.is_grad_enabled() and weight.requires_grad       # the only reader of the stack is the weight gradient
        return ChebSeriesSmallFn.apply(series, weight, bias, op, mode, bias_kind, bool(as_series), geom, need_stack)
    if bf16:
        layer = lambda s, b: ChebSeriesBf16Fn.apply(s, weight, b, op, mode, bias_kind, bool(as_series), geom)
    elif time_chunk is not None:
        layer = lambda s, b: ChebSeriesChunkFn.apply(s, weight, b, op, mode, bias_kind, bool(as_series), geom[3], time_chunk)
    else:
        layer = lambda s, b: ChebSeriesFn.apply(s, weight, b, op, mode, bias_kind, bool(as_series), geom)
    out = _in_operand_labels(op, layer, series, bias, bias_kind)
    return out.to(BF16) if bf16 and op.perm is not None else out      # (the relabelling kernel is fp32: bf16 values pass through it exactly)


# ---- relu (+ dropout) + pool in the one-launch series layer ("relu + pool in the one-launch series layer")
# fused="auto" of cheb_time_windows_relu_pool_fused takes the one-launch form for the classes listed here: "pool" -- a call without a mask
# (p == 0) -- and "pool_dropout".  Set from profiles/r24_series_small_pool.json by SERIES_FUSED_AUTO's rule: a class is listed only where
# the new call's median lies below BOTH comparators' -- the general pooled epilogue and forward_series(fused=True) followed by the relu
# (+ dropout) + pool pass -- by more than the largest of the spreads, on both measured operands, forward and forward + backward.
# () is "never": "auto" is then cheb_time_windows_relu_pool / cheb_time_windows_relu_dropout_pool everywhere.
SERIES_POOL_FUSED_AUTO = ()


def series_pool_fused_supported(op, f, H, N, K, T, padding, dilation, mode, pool):
    """True where cheb_time_windows_relu_pool_fused(..., fused=True) runs: series_fused_supported's rules plus the pool's -- 2 or 4
    consecutive vertices, dividing the graph.  A host query: nothing launches."""
    try:
        check_pool(pool, op.n, "series_pool_fused_supported")
    except _lib.TgcnError:
        return False
    return series_fused_supported(op, f, H, N, K, T, padding, dilation, mode)


class ChebSeriesSmallReluPoolFn(torch.autograd.Function):
    """z = max over `pool` consecutive vertices of relu(ChebSeriesSmallFn's output) -- with drop = (seed tensor, thr, scale), of
    relu(y) * mask -- taken in the registers of the one-launch layer's epilogue (tgcn_cheb_series_small_pool_f32, csrc/series_small.h
    small_series_pool_kernel): the fold in power mode with K > 2, then ONE launch; the (S, n, nwin, N) output is never allocated.  z is
    (S*nwin, n/pool, N) or, as_series, (S, n/pool, nwin, N), bit-identical to _relu_pool_view / _relu_dropout_pool_view of
    ChebSeriesSmallFn's output.  The hop stack is written by that launch only when the weight trains (need_stack), the arg-max bytes only
    with need_idx (the caller's looks at grad mode).  The backward is _series_pool_backward: gz (times scale with dropout) through
    tgcn_relu_pool_bwd_f32, then ChebSeriesFn's backward body on the stack the launch wrote.  ctx.seed is the seed's tensor.
    geom = (1, left, right, dilation)."""

    @staticmethod
    @_on_device
    def forward(ctx, series, weight_khfg, bias, op, mode, bias_kind, as_series, geom, pool, need_idx, need_stack, drop):
        L = _lib.lib()
        S, n, T, f = series.shape
        K, H, _, N = weight_khfg.shape
        _, left, right, dil = geom
        nwin = T + left + right - (H - 1) * dil
        x, fold, Wt, b = _series_operands(series, weight_khfg, bias, mode)
        shape = (S, n // pool, nwin, N) if as_series else (S * nwin, n // pool, N)
        z = torch.empty(shape, dtype=torch.float32, device=x.device)
        idx = torch.empty(shape, dtype=torch.uint8, device=x.device) if need_idx else None
        stack = torch.empty((K, S, n, T * f), dtype=torch.float32, device=x.device) if need_stack else None
        seed_t, thr, scale = drop if drop is not None else (None, 0, 1.0)
        _lib.check(L.tgcn_cheb_series_small_pool_f32(_lib.stream_ptr(), C.byref(op.struct), int(mode), S, T, f, H, N, K, _lib.ptr(x), _lib.ptr(Wt),
                                                     _lib.ptr(b), bias_kind, 1 if as_series else 0, _lib.ptr(z), _lib.ptr(idx), pool,
                                                     _lib.ptr(stack), left, right, dil, _lib.ptr(seed_t), thr, scale))
        ctx.stack = stack
        _series_ctx(ctx, op, mode, fold, bias, bias_kind, as_series, (S, n, T, f, H, N, K), (1, left, right, dil), (Wt, z, idx, pool, nwin, drop))
        return z

    @staticmethod
    @_on_device
    def backward(ctx, gz):
        return _series_pool_backward(ctx, gz, "cheb_time_windows_relu_pool_fused") + (None,) * 9


@_on_device
def cheb_time_windows_relu_pool_fused(op, series, weight, bias, bias_kind, mode, pool, p=0.0, seed=None, as_series=False, padding=0, dilation=1,
                                      fused=True):
    """gcn_pool_4(dropout(relu(cheb_time_windows(..., fused=True)), p)) (pool=4; pool=2: gcn_pool) in ONE launch on an operand that fits in
    LDS: the hops, the window projection, the bias, relu, the dropout and the max over `pool` consecutive vertices
    (ChebSeriesSmallReluPoolFn).  series (S, n, T) with weight (K, H, N), or (S, n, T, f) with (K, H, f, N) -> z (S*nwin, n/pool, N) or,
    as_series=True, (S, n/pool, nwin, N).  The layer's full output is never allocated; z and every gradient are bit-identical to
    _relu_pool_view / _relu_dropout_pool_view of cheb_time_windows(..., fused=True) under the same seed.  p == 0 runs the form without a
    mask; otherwise p, seed and the element index are cheb_time_windows_relu_dropout_pool's (dropout_keep_mask reproduces the mask).
    There is no stride and no time_chunk: the one-launch layer has neither.
    fused=True raises TgcnError before an operand is touched or anything launches: bfloat16 parameters, a non-square or reordered
    operand, a plan that refuses (series_pool_fused_supported tells), and everything check_pool, dropout_params, dropout_seed and
    series_geometry refuse.  fused="auto" runs the one-launch form where it can and where SERIES_POOL_FUSED_AUTO lists the call's class
    ("pool" at p == 0, else "pool_dropout"); everywhere else it is cheb_time_windows_relu_pool / cheb_time_windows_relu_dropout_pool with
    the same arguments."""
    who = "cheb_time_windows_relu_pool_fused"
    if fused is not True and not (isinstance(fused, str) and fused == "auto"):
        raise _lib.TgcnError("%s: fused is True or \"auto\", got %r" % (who, fused))
    thr, scale = dropout_params(p, who)
    dropout_seed(seed, series.device, who, draw=False)
    bf16 = param_dtype(weight, bias, who) == BF16
    if bf16 and fused is True:
        raise _lib.TgcnError("%s: fused=True runs in float32 only -- the parameters are bfloat16" % who)
    run = not bf16
    if run:
        pool, geom = _series_pool_checks(who, series, weight, pool, 1, padding, dilation)
        f, K, H, N, T = series.shape[3] if series.dim() == 4 else 1, weight.shape[0], weight.shape[1], weight.shape[-1], series.shape[2]
        if fused is True:
            if op.n_cols != op.n:
                raise _lib.TgcnError("%s: fused=True needs a square operand, got %d x %d" % (who, op.n, op.n_cols))
            if op.perm is not None:
                raise _lib.TgcnError("%s: fused=True runs in the operand's own labels -- a reordered operand is not supported (fused=\"auto\")" % who)
            if _series_small_plan(op, f, H, N, K, T, geom[1], geom[2], geom[3], mode)[0] != 0:
                raise _lib.TgcnError("%s: fused=True, but n = %d, nnz = %d, f = %d, H = %d, N = %d do not fit the one-launch layer "
                                     "(series_pool_fused_supported; fused=\"auto\")" % (who, op.n, op.nnz, f, H, N))
        else:       # the measured rule first: no query is made for a class that never fuses
            run = (("pool" if p == 0 else "pool_dropout") in SERIES_POOL_FUSED_AUTO and op.n_cols == op.n and op.perm is None
                   and _series_small_plan(op, f, H, N, K, T, geom[1], geom[2], geom[3], mode)[0] == 0)
    if not run:
        if p == 0:
            return cheb_time_windows_relu_pool(op, series, weight, bias, bias_kind, mode, pool, as_series=as_series, padding=padding,
                                               dilation=dilation)
        return cheb_time_windows_relu_dropout_pool(op, series, weight, bias, bias_kind, mode, pool, p, seed, as_series=as_series, padding=padding,
                                                   dilation=dilation)
    series, weight, need_idx = _series_pool_tensors(series, weight, bias)
    drop = None if p == 0 else (dropout_seed(seed, series.device, who), thr, scale)
    return ChebSeriesSmallReluPoolFn.apply(series, weight, bias, op, mode, bias_kind, bool(as_series), geom, pool, need_idx,
                                           torch.is_grad_enabled() and weight.requires_grad, drop)


@_on_device
def cheb_wgrad(terms, g2d):
    """dW[t] = terms[t]^T @ g2d  ->  (T, Kc, N); terms: list of (M, Kc) views with contiguous rows, g2d: (M, N)."""
    _lib.require_device(g2d, *terms)
    L = _lib.lib()
    T = len(terms)
    M, Kc = terms[0].shape
    N = g2d.shape[1]
    dW = torch.empty((T, Kc, N), dtype=torch.float32, device=g2d.device)
    for t0 in range(0, T, 32):
        nt = min(32, T - t0)
        ws = _workspace(L.tgcn_cheb_wgrad_workspace_bytes(M, Kc, N, nt), g2d.device, floor=16)
        a = (C.c_void_p * nt)(*[terms[t0 + i].data_ptr() for i in range(nt)])
        lda = (C.c_int64 * nt)(*[terms[t0 + i].stride(0) for i in range(nt)])
        _lib.check(L.tgcn_cheb_wgrad_f32(_lib.stream_ptr(), M, Kc, N, nt, a, lda, _lib.ptr(g2d), g2d.stride(0),
                                         _lib.ptr(dW[t0:]), _lib.ptr(ws), ws.numel()))
    return dW


def choose_layout(q, n, C_row):
    """layout 1 (re-lay x to one long row per vertex) when per-sample rows are short: gathers then move
    q*C contiguous floats per neighbour instead of C."""
    return 1 if (C_row < 32 and q > 1) else 0


def choose_q_chunk(q, n, C_row):
    """Samples per pass on layout 0: operands that overflow the caches anyway go one sample at a time, so a
    pass's gather working set is one (n, C) slab (and the hop workspace stays small)."""
    per_q = n * C_row * 4
    return int(max(1, min(q, (64 << 20) // max(per_q, 1))))


def _hops_setup(op, q, Crow, layout, q_chunk):
    """(layout, q_chunk, schedule) of the hops-then-projection drivers: the row layout and samples per pass default to choose_layout /
    choose_q_chunk; layout 1 hops one (vertex, q*C) row per vertex"""
    layout = choose_layout(q, op.n, Crow) if layout is None else layout
    q_chunk = choose_q_chunk(q, op.n, Crow) if q_chunk is None else q_chunk
    hop_C = q * Crow if layout == 1 else Crow
    return layout, q_chunk, op.schedule_for(hop_C, hop_C % 4 == 0)


@_on_device
def cheb_forward_raw(op, x3, Wt, bias, bias_kind, mode, K, layout=None, q_chunk=None):
    """Fused layer forward through tgcn_cheb_forward_f32.  x3: (q, n, C) contiguous; Wt: (K*C, N)."""
    _lib.require_device(x3, Wt, bias)
    L = _lib.lib()
    q, n, Crow = x3.shape
    N = Wt.shape[1]
    assert x3.is_contiguous() and Wt.is_contiguous() and Wt.shape[0] == K * Crow and n == op.n
    x3 = _aligned_input(x3)
    layout, q_chunk, sched = _hops_setup(op, q, Crow, layout, q_chunk)
    ws = _workspace(L.tgcn_cheb_forward_workspace_bytes(C.byref(sched.struct), K, q, n, Crow, layout, q_chunk), x3.device)
    out = torch.empty((q, n, N), dtype=torch.float32, device=x3.device)
    _lib.check(L.tgcn_cheb_forward_f32(_lib.stream_ptr(), C.byref(op.struct), C.byref(sched.struct), mode, K, q, n, Crow,
                                       N, _lib.ptr(x3), _lib.ptr(Wt), _lib.ptr(bias), bias_kind, _lib.ptr(out), layout,
                                       q_chunk, _lib.ptr(ws), ws.numel()))
    return out


@_on_device
def cheb_forward_compact(plan, x3, Wt, bias, bias_kind, K, q_chunk=None, mode=MODE_POWER, W_left=None, keep=False):
    """Layer forward on an operand with left-out vertices (graph.CompactPlan) through ONE call of tgcn_cheb_compact_layer_f32: hop tensors only
    for the kept vertices, both recurrences.  x3: (q, n, C) contiguous; Wt: (K*C, N) in the working basis (folded for MODE_POWER); W_left:
    (C, N) matrix of the left-out vertices (MODE_CHEBYSHEV: W_0 - W_2 + W_4 - ..., left_out_weight; MODE_POWER: None = W'_0).
    keep=True: the hop tensors are written into one caller-owned buffer and returned as the layer's basis -- the list compact_terms gives
    ([x3, P_1, ..] for MODE_POWER, [T_0, T_1, ..] for MODE_CHEBYSHEV; compact terms are (q, n_c + 1, C) with a zero last row) -> (out, terms)."""
    _lib.require_device(x3, Wt, bias, W_left)
    L = _lib.lib()
    q, n, Crow = x3.shape
    N = Wt.shape[1]
    assert x3.is_contiguous() and Wt.is_contiguous() and Wt.shape[0] == K * Crow and n == plan.n and K >= 2
    x3 = _aligned_input(x3)
    auto_chunk = False
    if q_chunk is None:
        q_chunk = COMPACT_Q_CHUNK
    if q_chunk is None:
        # time steps per pass: the hops still run one time step per launch; a pass's projection reads a per-vertex bias ONCE for all its
        # time steps (the streaming projection keeps the bias row of a tile in registers across the samples of the pass).  cfg5 (round 5, same
        # box): 282.3 / 279.8 / 278.6 ms per forward at 4 / 8 / 16 time steps per pass -- 1.3 % for 77 GB of workspace at 16, so the K-1 compact
        # hop tensors of a pass are held to COMPACT_WS_FRACTION (a quarter) of the memory that is free when the shape is first seen (cfg5: 8 per
        # pass, 39 GB), in passes of equal size; an allocation that fails later (the process has allocated more since, or shares the GPU) halves
        # the choice instead of failing the forward
        q_chunk = 1
        if bias_kind == BIAS_VERTEX_CHANNEL and q > 1:
            key = (K, Crow, q)
            q_chunk = plan.q_chunk_cache.get(key)
            if q_chunk is None:            # asked once per shape: no host query on later forwards (nor under hipGraph capture)
                free = torch.cuda.mem_get_info(x3.device)[0]
                per_q = (K - 1) * (plan.n_c + 1) * Crow * 4
                most = int(max(1, min(q, 16, int(free * COMPACT_WS_FRACTION) // max(per_q, 1))))
                passes = -(-q // most)
                q_chunk = plan.q_chunk_cache[key] = -(-q // passes)
            auto_chunk = True
    sched = plan.schedule_for(Crow, Crow % 4 == 0)
    kept = None
    if keep:
        nt = K if mode == MODE_CHEBYSHEV else K - 1
        kept = torch.empty((nt, q, plan.n_c + 1, Crow), dtype=torch.float32, device=x3.device)
    out = torch.empty((q, n, N), dtype=torch.float32, device=x3.device)
    while True:
        ws_bytes = L.tgcn_cheb_compact_layer_workspace_bytes(C.byref(sched.struct), mode, K, q, plan.n_c, Crow, q_chunk, 1 if keep else 0)
        try:
            ws = _workspace(ws_bytes, x3.device)
            break
        except torch.OutOfMemoryError:
            if not auto_chunk or q_chunk <= 1:
                raise
            torch.cuda.empty_cache()
            q_chunk = plan.q_chunk_cache[(K, Crow, q)] = max(1, q_chunk // 2)        # the cached choice no longer fits: fewer time steps per pass from now on
    _lib.check(L.tgcn_cheb_compact_layer_f32(_lib.stream_ptr(), C.byref(plan.first.struct), C.byref(plan.rest.struct), C.byref(sched.struct), mode, K, q, n,
                                             Crow, N, _lib.ptr(x3), _lib.ptr(Wt), _lib.ptr(W_left), _lib.ptr(bias), bias_kind, _lib.ptr(out),
                                             _lib.ptr(plan.rows), _lib.ptr(plan.empty), plan.n_empty, q_chunk, _lib.ptr(kept),
                                             _lib.ptr(ws), ws.numel()))
    if not keep:
        return out
    terms = ([x3] if mode == MODE_POWER else []) + [kept[i] for i in range(kept.shape[0])]
    return out, terms


COMPACT_WS_FRACTION = 0.25       # share of the free device memory the compact hop tensors of one pass may take (cheb_forward_compact)
COMPACT_SLAB_BYTES = 64 << 20    # a hop launch covers one sample when a sample's (n_c, C) slab is larger (the gather working set stays one slab)


def compact_plan_for(op, mode, K, q, n, C_row, N=None):
    """The graph.CompactPlan a layer of this shape runs on, or None: square operands with enough vertices to leave out of the hop tensors
    (graph.GraphOperand.compact_plan), 2 <= K <= 32, row layout 0 -- the vertex-major layout 1 of short per-sample rows has no compact
    form (measured slower on cfg5n, docs/EXPERIMENTS.md A.4).  Mode 0 keeps the rows with entries, mode 1 also every referenced vertex
    (closed form T_k[i] = x[i], 0, -x[i], ... for the isolated rest).  N is not used."""
    if not COMPACT or not (2 <= K <= 32) or op.n != op.n_cols or choose_layout(q, n, C_row) == 1:
        return None
    return op.compact_plan("rows" if mode == MODE_POWER else "closed")


def _compact_buffer(plan, q, C_row, device):
    """(q, n_c + 1, C): row n_c of every sample is the zero row entries pointing at a left-out vertex gather from"""
    t = torch.empty((q, plan.n_c + 1, C_row), dtype=torch.float32, device=device)
    t[:, plan.n_c].zero_()
    return t


def _gather_rows(src3, rows64, plan, out=None):
    """src3[:, rows] into a compact buffer (tgcn_pack_rows_f32; one contiguous (n_c, C) block per sample)"""
    out = _compact_buffer(plan, src3.shape[0], src3.shape[2], src3.device) if out is None else out
    for b in range(src3.shape[0]):
        pack_rows(src3[b], rows64, out[b, : plan.n_c])
    return out


def _compact_hop(op, X, Y, plan, z=None, alpha=1.0, beta=0.0):
    """Y[:, :n_c] = alpha * op X + beta * z[:, :n_c]; one launch per sample when a sample's slab is beyond COMPACT_SLAB_BYTES"""
    q = X.shape[0]
    n_c = plan.n_c
    per_sample = q > 1 and n_c * X.shape[2] * 4 > COMPACT_SLAB_BYTES
    for sl in ([slice(b, b + 1) for b in range(q)] if per_sample else [slice(0, q)]):
        csr_hop(op, X[sl], z=None if z is None else z[sl, :n_c], alpha=alpha, beta=beta, out=Y[sl, :n_c])


@_on_device
def compact_terms(plan, x3, K, mode):
    """The K terms of the layer's basis with hop tensors for the plan's n_c kept vertices only (a backward without a kept basis recomputes them
    here; the forward itself is one driver call, cheb_forward_compact).
    mode 0: [x3, P_1, ..., P_{K-1}], P_k = L^k x (monomials: the basis of the FOLDED weight); term 0 is x itself in the caller's labels.
    mode 1: [T_0, ..., T_{K-1}] Chebyshev, every term compact (T_0 = x packed to the kept rows).
    Compact terms are views of ONE (T, q, n_c + 1, C) buffer whose last rows are zero."""
    q, n, Crow = x3.shape
    nt = K if mode == MODE_CHEBYSHEV else K - 1
    buf = torch.empty((max(nt, 1), q, plan.n_c + 1, Crow), dtype=torch.float32, device=x3.device)
    buf[:, :, plan.n_c].zero_()
    if mode == MODE_POWER:
        terms = [x3]
        for k in range(1, K):
            _compact_hop(plan.first if k == 1 else plan.rest, terms[k - 1], buf[k - 1], plan)
            terms.append(buf[k - 1])
        return terms
    terms = [_gather_rows(x3, plan.rows64(), plan, out=buf[0])]
    for k in range(1, K):
        if k == 1:
            _compact_hop(plan.rest, terms[0], buf[1], plan)
        else:
            _compact_hop(plan.rest, terms[k - 1], buf[k], plan, z=terms[k - 2], alpha=2.0, beta=-1.0)
        terms.append(buf[k])
    return terms


_sign_cache = {}


def _left_out_fold(K, device):
    """(K, K) fold matrix whose column 0 holds the signs +1, 0, -1, 0, ... of T_k of an isolated vertex: tgcn_fold_weight_f32 with it puts
    W_0 - W_2 + W_4 - ... into out[0]"""
    key = (K, str(device))
    with _fold_lock:
        m = _sign_cache.get(key)
        if m is None:
            m = torch.zeros(K, K, dtype=torch.float32)
            for k in range(0, K, 2):
                m[k, 0] = 1.0 if k % 4 == 0 else -1.0
            m = _sign_cache[key] = m.to(device)
    return m


def left_out_weight(W_kcn, mode):
    """(C, N) matrix of the vertices a plan leaves out: out[i] = x[i] @ this + bias.  mode 0 (W in the monomial basis): W'_0 -- every
    P_k[i], k >= 1, is zero.  mode 1: W_0 - W_2 + W_4 - ... -- T_k[i] = x[i], 0, -x[i], 0, ... for an isolated vertex (the signed sum
    runs in tgcn_fold_weight_f32)."""
    W_kcn = W_kcn.contiguous()
    if mode == MODE_POWER:
        return W_kcn[0]
    return fold_weight(_left_out_fold(W_kcn.shape[0], W_kcn.device), W_kcn)[0]


@_on_device
def project_mapped(terms, term_bs, W2d, bias, bias_kind, n_vertices, rowmap, mapped_terms, q, out, interleave=1):
    """out[b, rowmap[m]] = sum_t terms[t][b, row_t(m)] @ W[t] + bias through tgcn_cheb_project_mapped_f32; terms: tensors whose sample b starts
    term_bs[t] floats after sample b-1; W2d: (T*Kc, N); out: (q, n_vertices, N) contiguous.
    interleave = q > 1: vertex-major terms ((rows, q, Kc): the samples of a vertex are consecutive rows), one launch for all samples."""
    L = _lib.lib()
    T = len(terms)
    Kc = W2d.shape[0] // T
    N = W2d.shape[1]
    M = int(rowmap.numel()) * interleave
    if M == 0:
        return out
    a = (C.c_void_p * T)(*[t.data_ptr() for t in terms])
    lda = (C.c_int64 * T)(*[Kc] * T)
    a_bs = (C.c_int64 * T)(*term_bs)
    _lib.check(L.tgcn_cheb_project_mapped_f32(_lib.stream_ptr(), M, Kc, N, T, a, lda, _lib.ptr(W2d), _lib.ptr(bias), bias_kind, n_vertices, interleave,
                                              _lib.ptr(rowmap), mapped_terms, 1 if interleave > 1 else q, a_bs, n_vertices * N, _lib.ptr(out), N))
    return out


@_on_device
def compact_forward(plan, x3, Wt_kcn, bias, bias_kind, mode, keep=True):
    """Layer forward with compact hop tensors that also hands back the basis (training forward, and the Chebyshev-recurrence classes): ONE
    driver call (cheb_forward_compact -> tgcn_cheb_compact_layer_f32; round 4 issued the hops and the two row-mapped projections from here).
    Wt_kcn: (K, C, N) in the WORKING basis (folded for mode 0).  -> (out (q, n, N), terms or None)"""
    _lib.require_device(x3, Wt_kcn, bias)
    q, n, Crow = x3.shape
    K, _, N = Wt_kcn.shape
    assert x3.is_contiguous() and n == plan.n and 2 <= K <= 32
    b = bias.contiguous() if bias is not None else None
    W_left = left_out_weight(Wt_kcn, mode) if (mode == MODE_CHEBYSHEV and plan.n_empty) else None
    res = cheb_forward_compact(plan, x3, Wt_kcn.reshape(K * Crow, N).contiguous(), b, bias_kind, K, mode=mode, W_left=W_left, keep=keep)
    return res if keep else (res, None)


@_on_device
def compact_wgrad(plan, x3, terms, g, mode):
    """dW (K, C, N) in the working basis from compact terms: the kept rows of g are gathered once (g_c), term k >= 1 contracts with them;
    the left-out vertices enter through x only -- term 0 for mode 0, and with alternating signs at every even k for mode 1 (T_k[i] = +-x[i])."""
    q, n, Crow = x3.shape
    N = g.shape[2]
    K = len(terms)
    g_c = _gather_rows(g, plan.rows64(), plan)                               # (q, n_c + 1, N), zero last row
    gc2 = g_c.reshape(q * (plan.n_c + 1), N)
    S_all = cheb_wgrad([x3.reshape(q * n, Crow)], g.reshape(q * n, N))[0]     # x^T g over every vertex
    flat = lambda t: t.reshape(q * (plan.n_c + 1), Crow)
    if mode == MODE_POWER:
        rest = cheb_wgrad([flat(t) for t in terms[1:]], gc2) if K > 1 else None
        return torch.cat([S_all.unsqueeze(0), rest]) if K > 1 else S_all.unsqueeze(0)
    dW = cheb_wgrad([flat(t) for t in terms], gc2)
    S_out = S_all - dW[0]                                                      # x^T g over the isolated vertices only
    for k in range(0, K, 2):
        dW[k] += S_out if k % 4 == 0 else -S_out
    return dW


@_on_device
def cheb_forward_pool(op, x3, Wt, bias, bias_kind, mode, K, pool, z, idx, layout=None, q_chunk=None):
    """relu + max-pool fused layer on the hops-then-projection path (tgcn_cheb_forward_pool_f32) into z (q, n/pool, N) and the
    arg-max bytes idx.  x3: (q, n, C) contiguous; Wt: (K*C, N) in the working basis."""
    _lib.require_device(x3, Wt, bias, z, idx)
    L = _lib.lib()
    q, n, Crow = x3.shape
    N = Wt.shape[1]
    assert x3.is_contiguous() and Wt.is_contiguous() and Wt.shape[0] == K * Crow and n == op.n and z.is_contiguous() and idx.is_contiguous()
    x3 = _aligned_input(x3)
    layout, q_chunk, sched = _hops_setup(op, q, Crow, layout, q_chunk)
    ws = _workspace(L.tgcn_cheb_forward_pool_workspace_bytes(C.byref(sched.struct), K, q, n, Crow, N, layout, q_chunk, pool), x3.device)
    _lib.check(L.tgcn_cheb_forward_pool_f32(_lib.stream_ptr(), C.byref(op.struct), C.byref(sched.struct), mode, K, q, n, Crow, N,
                                            _lib.ptr(x3), _lib.ptr(Wt), _lib.ptr(bias), bias_kind, pool, _lib.ptr(z), _lib.ptr(idx),
                                            layout, q_chunk, _lib.ptr(ws), ws.numel()))
    return z


def pool_epilogue_is_fused(op, q, Crow, N, K, pool, layout=None, q_chunk=None):
    """True when cheb_forward_pool runs relu + pool inside the projection kernel for this shape (no scratch for the layer output)."""
    L = _lib.lib()
    layout, q_chunk, sched = _hops_setup(op, q, Crow, layout, q_chunk)
    base = L.tgcn_cheb_forward_workspace_bytes(C.byref(sched.struct), K, q, op.n, Crow, layout, q_chunk)
    return L.tgcn_cheb_forward_pool_workspace_bytes(C.byref(sched.struct), K, q, op.n, Crow, N, layout, q_chunk, pool) < base + q * op.n * N * 4


@_on_device
def cheb_stack(op, x3, K, mode, _operand_labels=False):
    """The (K, q, n, C) stack `_chebyshev` / `_time_chebyshev` return (gcn.py:52-79,126-154,208-237), or the
    true-recurrence stack for mode 1.  Materialising path: every hop writes its slice of the stack."""
    _lib.require_device(x3)
    if op.perm is not None and not _operand_labels:       # reordered operand: relabel on the way in and out (the shared operand is never touched)
        return relabel_rows(cheb_stack(op, relabel_rows(x3, op.perm, op.inv_perm), K, mode, _operand_labels=True), op.inv_perm, op.perm, dim=2)
    q, n, Crow = x3.shape
    st = torch.empty((K, q, n, Crow), dtype=torch.float32, device=x3.device)
    st[0].copy_(x3)
    if K > 1:
        csr_hop(op, st[0], out=st[1])
    p_prev = st[1] if K > 1 else None
    for k in range(2, K):
        if mode == MODE_POWER:      # P_k = L P_{k-1} (hidden chain), Xt[k] = 2 P_k - Xt[k-2]
            _, p_prev = csr_hop(op, p_prev, z=st[k - 2], alpha=2.0, beta=-1.0, want_p=True, out=st[k])
        else:
            csr_hop(op, st[k - 1], z=st[k - 2], alpha=2.0, beta=-1.0, out=st[k])
    return st


_fold_cache = {}
_fold_lock = threading.Lock()     # shared by the threads of nn.DataParallel replicas


def power_fold_matrix(K, device=None, dtype=torch.float32):
    key = (K, str(device), dtype)
    with _fold_lock:
        c = _fold_cache.get(key)
        if c is None:
            c = _fold_cache[key] = _power_fold_matrix(K, device, dtype)
    return c


def _power_fold_matrix(K, device=None, dtype=torch.float32):
    """c[k, j] with Xt[k] = sum_j c[k, j] L^j x for the reference_power recursion: c[0]=e0, c[1]=e1,
    c[k] = 2 e_k - c[k-2].  Folding it into the weight (W'_j = sum_k c[k,j] W_k) turns the layer into one
    monomial chain: no subtrahend reads, no second output (verified there to <= 6.3e-7)."""
    c = torch.zeros(K, K, dtype=torch.float64)
    for k in range(K):
        c[k, k] = 1.0 if k < 2 else 2.0
        if k >= 2:
            c[k] -= c[k - 2]
    return c.to(device=device, dtype=dtype)


@_on_device
def fold_weight(fold, W, transpose=False):
    """W'[j] = sum_k fold[k, j] W[k]  (transpose: sum_k fold[j, k] W[k]) for a (K, C, N) weight, in libtgcn_hip.so: the
    forward path issues no vendor-library GEMM"""
    _lib.require_device(fold, W)
    K = W.shape[0]
    Wc = W.contiguous()
    out = torch.empty_like(Wc)
    _lib.check(_lib.lib().tgcn_fold_weight_f32(_lib.stream_ptr(), K, Wc.numel() // K, _lib.ptr(fold), _lib.ptr(Wc), _lib.ptr(out),
                                               1 if transpose else 0))
    return out


def _power_fold(mode, W_kcn):
    """fold matrix of a (K, C, N) reference-basis weight for MODE_POWER with K > 2, else None (the two bases agree).  _series_operands
    writes this rule and _working_weight's out in place (it runs at 0.3 ms per call): a change here is a change there"""
    return power_fold_matrix(W_kcn.shape[0], W_kcn.device) if (mode == MODE_POWER and W_kcn.shape[0] > 2) else None


def _working_weight(fold, W_kcn):
    """the weight in the basis the kernels work in: folded to the monomial basis when there is a fold (tgcn_fold_weight_f32)"""
    return fold_weight(fold, W_kcn) if fold is not None else W_kcn


# ----------------------------------------------------------------------------------------- autograd
def small_path_tile(op, C_row, mode, pool=False):
    """Channel tile (16 / 8) of the one-launch LDS-resident kernel, or 0 when the shape does not fit it
    (pool: with the fused relu + pool epilogue)."""
    if op.n_cols != op.n or not SMALL_PATH:
        return 0
    fn = _lib.lib().tgcn_cheb_forward_small_pool_supported if pool else _lib.lib().tgcn_cheb_forward_small_supported
    return fn(op.n, op.nnz, int(C_row), int(mode))


@_on_device
def cheb_forward_small(op, x3, W_kcn, fold, bias, bias_kind, mode):
    """Whole layer in one launch (tgcn_cheb_forward_small_f32).  W_kcn: (K, C, N) RAW weight when `fold` is given."""
    _lib.require_device(x3, W_kcn, bias, fold)
    q, n, Crow = x3.shape
    K, _, N = W_kcn.shape
    out = torch.empty((q, n, N), dtype=torch.float32, device=x3.device)
    _lib.check(_lib.lib().tgcn_cheb_forward_small_f32(_lib.stream_ptr(), C.byref(op.struct), mode, K, q, Crow, N, _lib.ptr(x3),
                                                      _lib.ptr(W_kcn), _lib.ptr(fold), _lib.ptr(bias), bias_kind, _lib.ptr(out)))
    return out


def small_plan(op, C_row, N, q, mode, pool=0, basis=False):
    """The kernel and launch configuration cheb_forward_small / the fused small-pool call (basis=False) or cheb_basis_small (basis=True) takes
    for this operand, row length, width and batch (tgcn_cheb_small_plan: the function the launch entries get it from), as a dict: form
    (0 output-side, 1 narrow input-side, 2 basis, 3 fp32 matrix pipe, 4 bf16x3 matrix pipe), tile, cp, spw, dense_lds, threads, lds_bytes,
    grid_x, grid_y.  A host query: nothing launches; raises TgcnError where the launch entry would refuse."""
    pl = _lib.SmallPlanStruct()
    _lib.check(_lib.lib().tgcn_cheb_small_plan(op.n, op.nnz, 1 if op.dense is not None else 0, int(mode), int(C_row), int(N), int(q), int(pool),
                                               1 if basis else 0, C.byref(pl)))
    return {k: int(getattr(pl, k)) for k, _ in _lib.SmallPlanStruct._fields_}


def small_basis_tile(op, C_row, mode):
    """Channel tile of the one-launch basis kernel (weight gradient on small graphs), or 0 when the operand does not fit."""
    if op.n_cols != op.n or not SMALL_PATH:
        return 0
    return _lib.lib().tgcn_cheb_basis_small_supported(op.n, op.nnz, int(C_row), int(mode))


@_on_device
def cheb_basis_small(op, x3, K, mode):
    """Terms of the layer's basis as a list of K (q, n, C) tensors (term 0 is x3 itself): monomials L^k x for
    MODE_POWER (the basis of the folded weight), Chebyshev T_k x for MODE_CHEBYSHEV.  One launch."""
    _lib.require_device(x3)
    q, n, Crow = x3.shape
    if K == 1:
        return [x3]
    stack = torch.empty((K - 1, q, n, Crow), dtype=torch.float32, device=x3.device)
    # the kernel indexes terms k = 1 .. K-1 of a (K, q, n, C) stack: pass the address term 0 would have
    base = stack.data_ptr() - q * n * Crow * 4
    _lib.check(_lib.lib().tgcn_cheb_basis_small_f32(_lib.stream_ptr(), C.byref(op.struct), mode, K, q, Crow, _lib.ptr(x3), base))
    return [x3] + [stack[k] for k in range(K - 1)]


@_on_device
def cheb_forward_pf(op, x3, Wt_kcn, bias, bias_kind, mode):
    """Project-first form (tgcn_cheb_forward_pf_f32): ONE projection x . [W_0 | ... | W_{K-1}], then Horner / Clenshaw
    on the (q, n, N) results.  Wt_kcn: (K, C, N), already folded for MODE_POWER."""
    _lib.require_device(x3, Wt_kcn, bias)
    L = _lib.lib()
    q, n, Crow = x3.shape
    K, _, N = Wt_kcn.shape
    Wcat = weight_layout(Wt_kcn, 0)
    sched = op.schedule_for(N, N % 4 == 0)
    ws = _workspace(L.tgcn_cheb_forward_pf_workspace_bytes(C.byref(sched.struct), K, q, n, N), x3.device)
    out = torch.empty((q, n, N), dtype=torch.float32, device=x3.device)
    _lib.check(L.tgcn_cheb_forward_pf_f32(_lib.stream_ptr(), C.byref(op.struct), C.byref(sched.struct), mode, K, q, n, Crow, N,
                                          _lib.ptr(x3), _lib.ptr(Wcat), _lib.ptr(bias), bias_kind, _lib.ptr(out), _lib.ptr(ws),
                                          ws.numel()))
    return out


PROJECT_FIRST = True   # developer switch
COMPACT = True         # developer switch: compact hop tensors for operands with many empty rows (graph.CompactPlan)
COMPACT_BF16 = True    # developer switch: the bf16 reference-power layers take the compact plan too (compact_forward_bf16); COMPACT gates both
COMPACT_Q_CHUNK = None # developer switch: time steps per pass of the compacted forward (None: chosen by cheb_forward_compact)


def use_project_first(q, n, C_row, N):
    """Hops move N floats per row instead of C: take it when the output is at most half as wide as the input row."""
    return PROJECT_FIRST and 2 * N <= C_row and q <= 65535


@dataclasses.dataclass(frozen=True)
class LayerPath:
    """How one single-GPU layer call runs (_layer_path).  kind "small": one launch, the graph in LDS (cheb_forward_small); "project_first":
    cheb_forward_pf; "compact": hop tensors for the kept vertices of `plan` only (mode 0: cheb_forward_compact, mode 1 and training with the
    basis kept: compact_forward); "hops": hops-then-projection on row `layout` (cheb_forward_raw, training: forward_keeping_basis).
    pool_fused: relu + pool run inside the layer's launches (small-pool kernel, cheb_forward_pool), not as one more pass over its output."""
    kind: str
    plan: object = None
    layout: int = 0
    pool_fused: bool = False


def _layer_path(op, q, n, C_row, N, K, mode, pool=0, general=None, compact=True):
    """The one place that decides the LayerPath of a layer on (op, x (q, n, C_row), W (K, C_row, N)).
    pool: relu + max-pool layer -- the small-pool kernel only when the operand has no dense copy for the matrix pipe (there the plain small
    kernel + one relu / pool pass is faster: HCP shape 136 + 15 us against 330 us).
    general: replaces the project-first test -- the input gradient, the layer on (L^T, g, W^T), takes a compact plan of L^T only when the
    FORWARD shape is neither small nor project-first; "project_first" then means "neither small nor compact".
    compact=False: decide without building the compact plan ("hops" then stands for both general paths)."""
    if pool:
        dense_mfma = op.dense is not None and (C_row <= 32 or (C_row <= 64 and op.n <= 128))
        if small_path_tile(op, C_row, mode, pool=True) and not dense_mfma:
            return LayerPath("small", pool_fused=True)
    if small_path_tile(op, C_row, mode):
        return LayerPath("small")
    if general is None:
        general = not use_project_first(q, n, C_row, N)
    if not general:
        return LayerPath("project_first")
    plan = compact_plan_for(op, mode, K, q, n, C_row, N) if compact else None
    if plan is not None:
        return LayerPath("compact", plan=plan)
    return LayerPath("hops", layout=choose_layout(q, n, C_row), pool_fused=bool(pool))


@_on_device
def layer_forward(op, x3, W, fold, b, bias_kind, mode, path=None):
    """Forward of the layer on its LayerPath (all in libtgcn_hip.so; `path`: a choice the caller has made already).  W: (K, C, N) in the
    reference basis with its fold (the small-graph kernel folds inside), or in the working basis and fold None."""
    K, Crow, N = W.shape
    if path is None:
        path = _layer_path(op, x3.shape[0], x3.shape[1], Crow, N, K, mode)
    if path.kind == "small":
        return cheb_forward_small(op, x3, W, fold, b, bias_kind, mode)
    Wt = _working_weight(fold, W)
    if path.kind == "project_first":
        return cheb_forward_pf(op, x3, Wt, b, bias_kind, mode)
    if path.kind == "compact" and mode == MODE_POWER:       # many structurally empty rows: compact hop tensors, one call
        return cheb_forward_compact(path.plan, x3, Wt.reshape(K * Crow, N).contiguous(), b, bias_kind, K)
    if path.kind == "compact":                              # the same for the Chebyshev recurrence (closed form for isolated vertices)
        return compact_forward(path.plan, x3, Wt, b, bias_kind, mode, keep=False)[0]
    return cheb_forward_raw(op, x3, Wt.reshape(K * Crow, N).contiguous(), b, bias_kind, mode, K, layout=path.layout)


@_on_device
def relayout_qnc_to_nqc(x3):
    """(q, n, C) -> (n, q, C) contiguous (tgcn_relayout_qnc_to_nqc_f32: LDS-tiled transpose for C <= 32, coalesced row copy beyond)."""
    q, n, Crow = x3.shape
    if q == 1:
        return x3.contiguous().view(n, 1, Crow)          # one sample: the same memory
    _lib.require_device(x3)
    out = torch.empty((n, q, Crow), dtype=torch.float32, device=x3.device)
    _lib.check(_lib.lib().tgcn_relayout_qnc_to_nqc_f32(_lib.stream_ptr(), _lib.ptr(x3.contiguous()), _lib.ptr(out), q, n, Crow))
    return out


KEEP_BASIS_BYTES = 2 << 30    # training on the hops-then-projection path keeps the hop tensors for the backward up to this size


@dataclasses.dataclass(frozen=True)
class KeptBasis:
    """The basis a training forward kept for the weight gradient (ChebLayerFn -> layer_backward): compact_terms' list of compact hop
    tensors for `plan` (compact_forward), or, with plan None, the K full-size terms as (q*n, C) row views (forward_keeping_basis), in
    (vertex, sample) row order when vertex_major (layout 1), else (sample, vertex)."""
    terms: list
    plan: object = None
    vertex_major: bool = False


@_on_device
def forward_keeping_basis(op, x3, Wt, bias, bias_kind, mode, layout):
    """Hops-then-projection forward on row `layout` that hands the K hop tensors to the caller (they ARE the basis the weight gradient
    needs: monomials L^k x for the folded weight, Chebyshev T_k x for mode 1), instead of recomputing them in backward.
    Same kernels as tgcn_cheb_forward_f32, one call per hop.  -> (out (q, n, N), KeptBasis)"""
    q, n, Crow = x3.shape
    K, _, N = Wt.shape
    nq = layout == 1
    x0 = relayout_qnc_to_nqc(x3).view(1, n, q * Crow) if nq else x3
    terms = [x0]
    for k in range(1, K):
        if mode == MODE_POWER or k == 1:
            terms.append(csr_hop(op, terms[k - 1]))
        else:
            terms.append(csr_hop(op, terms[k - 1], z=terms[k - 2], alpha=2.0, beta=-1.0))
    rows = [t.reshape(q * n, Crow) for t in terms]
    out = cheb_project(rows, Wt, bias, bias_kind, n, interleave=q if nq else 1).view(q, n, N)
    return out, KeptBasis(rows, vertex_major=nq)


class ChebLayerFn(torch.autograd.Function):
    """out = sum_k T_k x W_k + bias with T_k given by `mode`; x3 (q,n,C), W (K, C, N) in the REFERENCE basis.
    For MODE_POWER the weight is folded to the monomial basis (W'_j = sum_k c[k,j] W_k): inside the kernel on the
    small-graph path, by tgcn_fold_weight_f32 otherwise; backward applies the transposed fold to the weight gradient."""

    @staticmethod
    @_on_device
    def forward(ctx, x3, W, bias, op, mode, bias_kind, grad_mode=True, values=None):
        # `values`: the operand's stored values in CSR order as a tensor of the autograd graph (learnable edge weights of ChebConv /
        # ChebTimeConv).  The forward computes with the values packed in `op` (equal by construction); the tensor only receives the gradient.
        if values is not None and (mode != MODE_CHEBYSHEV or op.perm is not None or values.numel() != op.nnz):
            raise _lib.TgcnError("learnable operand values: Chebyshev-recurrence layers on an operand in the caller's labels only")
        K, Crow, N = W.shape
        x3 = x3.contiguous()
        W = W.contiguous()
        b = bias.contiguous() if bias is not None else None
        q, n, _ = x3.shape
        fold = _power_fold(mode, W)
        ctx.basis = None
        path = _layer_path(op, q, n, Crow, N, K, mode)
        # grad_mode: whether the CALLER records gradients (inside forward() grad mode is always off, and needs_input_grad only
        # mirrors requires_grad): an inference call under torch.no_grad() keeps nothing for a backward that never comes
        train = grad_mode and ctx.needs_input_grad[1]
        if train and path.kind == "compact" and K * q * (path.plan.n_c + 1) * Crow * 4 <= KEEP_BASIS_BYTES:
            # training forward on an operand with left-out vertices: compact hop tensors, kept for the weight gradient
            out, terms = compact_forward(path.plan, x3, _working_weight(fold, W), b, bias_kind, mode)
            ctx.basis = KeptBasis(terms, plan=path.plan)
        elif train and path.kind == "hops" and K > 1 and K * x3.numel() * 4 <= KEEP_BASIS_BYTES:
            out, ctx.basis = forward_keeping_basis(op, x3, _working_weight(fold, W), b, bias_kind, mode, path.layout)
        else:
            out = layer_forward(op, x3, W, fold, b, bias_kind, mode, path=path)
        ctx.save_for_backward(x3, W, None if values is None else values.detach())
        ctx.values_epoch = op.values_epoch
        ctx.op, ctx.mode, ctx.bias_kind, ctx.fold = op, mode, bias_kind, fold
        ctx.bias_shape = None if bias is None else bias.shape
        return out

    @staticmethod
    @_on_device
    def backward(ctx, g):
        x3, W, vals = ctx.saved_tensors
        _values_guard(ctx.op, ctx.values_epoch, vals)
        gx, gW, gb = layer_backward(ctx.op, ctx.mode, ctx.fold, x3, W, g, ctx.bias_kind, ctx.bias_shape, ctx.needs_input_grad,
                                    basis=ctx.basis)
        basis, ctx.basis = ctx.basis, None
        gv = None
        if len(ctx.needs_input_grad) > 7 and ctx.needs_input_grad[7]:
            kept = None
            if basis is not None and basis.plan is None and not basis.vertex_major and ctx.mode == MODE_CHEBYSHEV:
                kept = [r.view(x3.shape) for r in basis.terms]              # full-size T_0 .. T_{K-1} in (sample, vertex) row order
            gv = chebyshev_values_grad(ctx.op, x3, W, g, basis=kept)
        return gx, gW, gb, None, None, None, None, gv


@_on_device
def _monomial_stack(op, x3, K):
    st = torch.empty((K,) + tuple(x3.shape), dtype=torch.float32, device=x3.device)
    st[0].copy_(x3)
    for k in range(1, K):
        csr_hop(op, st[k - 1], out=st[k])
    return st


def _pad_rows(op, x3, weight_kcn, mode):
    """Rows whose length is not a multiple of 4 floats (the HCP horizon H = 15) take the scalar-load forms of the hop and
    projection kernels.  On the hops-then-projection path pad them with zero channels to the next multiple of 4 (zero
    rows in the weight): 7 % more hop traffic at C = 15, projection 0.37 -> 0.2 ms on the 59 k-vertex mesh shape.
    torch's pad is differentiable, so the gradients come back sliced."""
    K, C, N = weight_kcn.shape
    if C % 4 == 0 or C < 7 or _layer_path(op, x3.shape[0], x3.shape[1], C, N, K, mode, compact=False).kind != "hops":
        return x3, weight_kcn
    pad = (-C) % 4
    return torch.nn.functional.pad(x3, (0, pad)), torch.nn.functional.pad(weight_kcn, (0, 0, 0, pad))


def _to_operand_labels(op, x3, bias, bias_kind):
    """A reordered operand (GraphOperand.reordered) works in its own vertex labels: gather the rows of x and of a per-vertex
    bias into them (differentiable torch index ops: plumbing, no arithmetic)."""
    if op.perm is None:
        return x3, bias
    x3 = relabel_rows(x3, op.perm, op.inv_perm)
    if bias is not None and bias_kind == BIAS_VERTEX_CHANNEL:
        bias = relabel_rows(bias.reshape(op.n, -1), op.perm, op.inv_perm, dim=0)
    return x3, bias


def cheb_layer(op, x3, weight_kcn, bias, bias_kind, mode, values=None):
    """Differentiable fused layer; weight_kcn: (K, C, N) in the reference basis.  values: the operand's values (CSR order) as an autograd
    tensor when they are learnable (nn._EdgeBase builds it from edge_weight).  The weight's dtype picks the path: float32, or bfloat16
    (cheb_layer_bf16); any other is a TgcnError."""
    if param_dtype(weight_kcn, bias, "cheb_layer") == BF16:
        return cheb_layer_bf16(op, x3, weight_kcn, bias, bias_kind, mode, values)
    x3, weight_kcn = _pad_rows(op, x3, weight_kcn, mode)
    x3, bias = _to_operand_labels(op, x3, bias, bias_kind)
    out = ChebLayerFn.apply(x3, weight_kcn, bias, op, mode, bias_kind, torch.is_grad_enabled(), values)
    return out if op.perm is None else relabel_rows(out, op.inv_perm, op.perm)


@_on_device
def layer_backward(op, mode, fold, x3, W, g, bias_kind, bias_shape, needs, basis=None):
    """Gradients of the layer w.r.t. (x3, W, bias).  All contractions run in libtgcn_hip.so: the basis is recomputed
    with the hop kernel, dW is the MFMA weight-gradient kernel, G = g W^T is the projection kernel with the transposed
    weight, dx is Horner (mode 0) / Clenshaw (mode 1) on L^T with the hop kernel; only the bias reduction and the
    K x K fold of the weight gradient are torch ops.  Graphs that fit in LDS take two one-launch kernels instead of the
    2(K-1) hops: the basis kernel for dW and the forward kernel on L^T for dx."""
    K, Crow, N = W.shape
    q, n, _ = x3.shape
    Wt = _working_weight(fold, W) if needs[0] else W                   # the basis the kernels work in
    g = g.contiguous()
    g2d = g.reshape(q * n, N)
    gx = gW = None
    path = _layer_path(op, q, n, Crow, N, K, mode)
    if needs[1]:
        x3c = x3.contiguous()
        if (basis is not None and basis.plan is not None) or path.kind == "compact":
            # operand with left-out vertices: the basis exists (kept by the forward, or recomputed here) for the kept vertices only
            if basis is None:
                basis = KeptBasis(compact_terms(path.plan, x3c, K, mode), plan=path.plan)
            gW = compact_wgrad(basis.plan, x3c, basis.terms, g, mode)
        elif basis is not None:                                       # hop tensors kept by the forward (forward_keeping_basis)
            g_rows = relayout_qnc_to_nqc(g).view(q * n, N) if basis.vertex_major else g2d     # same row order as the terms
            gW = cheb_wgrad(basis.terms, g_rows)
        else:
            if small_basis_tile(op, Crow, mode):                      # small graphs: the whole basis in one launch
                terms = cheb_basis_small(op, x3c, K, mode)
            else:
                # x3c is in the operand's labels already (the layer relabels x on the way in): no second relabel inside cheb_stack
                terms = cheb_stack(op, x3c, K, MODE_CHEBYSHEV, _operand_labels=True) if mode == MODE_CHEBYSHEV else _monomial_stack(op, x3c, K)
            gW = cheb_wgrad([terms[k].reshape(q * n, Crow) for k in range(K)], g2d)
        if fold is not None:                                          # back to the reference basis
            gW = fold_weight(fold, gW, transpose=True)
    if needs[0]:
        # dx = sum_k T_k(L^T) g W_k^T IS the layer on (L^T, g, W^T): on small graphs the one-launch kernel, with left-out vertices in L^T
        # compact hop tensors -- the latter only where the forward shape is on a general path
        opT = op.transpose()
        dx = _layer_path(opT, q, n, N, Crow, K, mode, general=path.kind in ("compact", "hops"))
        if dx.kind in ("small", "compact"):
            gx = layer_forward(opT, g, weight_layout(Wt, 1), None, None, BIAS_NONE, mode, path=dx)
        else:
            # G[m, k*C + c] = sum_n g[m, n] W[k, c, n]: one projection with the (N, K*C) transposed weight, then the adjoint hops
            Wcat = weight_layout(Wt, 2).view(1, N, K * Crow)
            Gall = cheb_project([g2d], Wcat, None, BIAS_NONE, n).view(q, n, K * Crow)
            G = [Gall[:, :, k * Crow:(k + 1) * Crow] for k in range(K)]        # strided views, rows contiguous
            gx = _adjoint_hops(opT, G, mode).contiguous()
    return gx, gW, _bias_grad(g, bias_kind, bias_shape, needs[2])


class ChebReluPoolFn(torch.autograd.Function):
    """z = max over `pool` consecutive vertices of relu(layer(x)): the callers' `gcn_pool_4(F.relu(layer(x)))`
    (examples/pytorch_based/pytorch_hcp_tgcn.py:134-141) with the epilogue fused -- inside the one-launch kernel on
    small graphs (the layer output never reaches HBM), as one extra pass otherwise."""

    @staticmethod
    @_on_device
    def forward(ctx, x3, W, bias, op, mode, bias_kind, pool):
        K, Crow, N = W.shape
        x3 = x3.contiguous()
        W = W.contiguous()
        b = bias.contiguous() if bias is not None else None
        q, n, _ = x3.shape
        assert n % pool == 0, "pooling needs n divisible by the pool size"
        fold = _power_fold(mode, W)
        z = torch.empty((q, n // pool, N), dtype=torch.float32, device=x3.device)
        idx = torch.empty((q, n // pool, N), dtype=torch.uint8, device=x3.device)
        L = _lib.lib()
        path = _layer_path(op, q, n, Crow, N, K, mode, pool=pool)
        if path.pool_fused and path.kind == "small":
            _lib.check(L.tgcn_cheb_forward_small_pool_f32(_lib.stream_ptr(), C.byref(op.struct), mode, K, q, Crow, N, _lib.ptr(x3),
                                                          _lib.ptr(W), _lib.ptr(fold), _lib.ptr(b), bias_kind, 1, pool,
                                                          _lib.ptr(z), _lib.ptr(idx)))
        elif path.pool_fused:
            # hops-then-projection path: bias + relu + max over `pool` vertices inside the projection's epilogue where the shape allows
            # (tgcn_cheb_forward_pool_f32: the (q, n, N) layer output is then never written), one extra pass over scratch otherwise
            cheb_forward_pool(op, x3, _working_weight(fold, W).reshape(K * Crow, N).contiguous(), b, bias_kind, mode, K, pool, z, idx,
                              layout=path.layout)
        else:
            y = layer_forward(op, x3, W, fold, b, bias_kind, mode, path=path)
            _lib.check(L.tgcn_relu_pool_f32(_lib.stream_ptr(), _lib.ptr(y), _lib.ptr(z), _lib.ptr(idx), q, n, N, pool))
        ctx.save_for_backward(x3, W, z, idx)
        ctx.op, ctx.mode, ctx.bias_kind, ctx.fold, ctx.pool = op, mode, bias_kind, fold, pool
        ctx.bias_shape = None if bias is None else bias.shape
        return z

    @staticmethod
    @_on_device
    def backward(ctx, gz):
        x3, W, z, idx = ctx.saved_tensors
        q, n, _ = x3.shape
        N = W.shape[2]
        gy = torch.empty((q, n, N), dtype=torch.float32, device=gz.device)
        _lib.check(_lib.lib().tgcn_relu_pool_bwd_f32(_lib.stream_ptr(), _lib.ptr(gz.contiguous()), _lib.ptr(z), _lib.ptr(idx),
                                                     _lib.ptr(gy), q, n, N, ctx.pool))
        gx, gW, gb = layer_backward(ctx.op, ctx.mode, ctx.fold, x3, W, gy, ctx.bias_kind, ctx.bias_shape, ctx.needs_input_grad)
        return gx, gW, gb, None, None, None, None


def cheb_relu_pool(op, x3, weight_kcn, bias, bias_kind, mode, pool):
    """Differentiable relu + max-pool fused layer; weight in the reference basis."""
    if param_dtype(weight_kcn, bias, "cheb_relu_pool") == BF16:
        raise _lib.TgcnError("cheb_relu_pool: bfloat16 parameters are not supported (run the layer, then gcn_pool / gcn_pool_4)")
    x3, weight_kcn = _pad_rows(op, x3, weight_kcn, mode)
    if op.perm is not None:
        # pooling groups consecutive vertices of the CALLER's labelling, which are scattered rows of a reordered operand: the
        # epilogue cannot be fused there -- the layer's output is relabelled back first, then one relu + pool pass (HIP)
        return ReluPoolFn.apply(cheb_layer(op, x3, weight_kcn, bias, bias_kind, mode), pool)
    return ChebReluPoolFn.apply(x3, weight_kcn, bias, op, mode, bias_kind, pool)


class ReluPoolFn(torch.autograd.Function):
    """z = max over `pool` consecutive vertices of relu(y) as its own pass (tgcn_relu_pool_f32 / _bwd)."""

    @staticmethod
    @_on_device
    def forward(ctx, y, pool):
        _lib.require_device(y)
        y = y.float().contiguous()
        q, n, N = y.shape
        assert n % pool == 0, "pooling needs n divisible by the pool size"
        z = torch.empty((q, n // pool, N), dtype=torch.float32, device=y.device)
        idx = torch.empty((q, n // pool, N), dtype=torch.uint8, device=y.device)
        _lib.check(_lib.lib().tgcn_relu_pool_f32(_lib.stream_ptr(), _lib.ptr(y), _lib.ptr(z), _lib.ptr(idx), q, n, N, pool))
        ctx.save_for_backward(z, idx)
        ctx.shape, ctx.pool = (q, n, N), pool
        return z

    @staticmethod
    @_on_device
    def backward(ctx, gz):
        z, idx = ctx.saved_tensors
        q, n, N = ctx.shape
        gy = torch.empty((q, n, N), dtype=torch.float32, device=gz.device)
        _lib.check(_lib.lib().tgcn_relu_pool_bwd_f32(_lib.stream_ptr(), _lib.ptr(gz.contiguous()), _lib.ptr(z), _lib.ptr(idx), _lib.ptr(gy),
                                                     q, n, N, ctx.pool))
        return gy, None


@_on_device
def pack_rows(src, idx, out):
    """out[i] = src[idx[i]] for a (rows, C) view with contiguous rows (halo messages of the vertex-sharded layer)"""
    _lib.require_device(src, idx, out)
    assert src.dim() == 2 and src.stride(1) == 1 and out.is_contiguous() and idx.dtype == torch.int64 and idx.is_contiguous()
    _lib.check(_lib.lib().tgcn_pack_rows_f32(_lib.stream_ptr(), _lib.ptr(src), src.stride(0), _lib.ptr(idx), idx.numel(), src.shape[1],
                                             _lib.ptr(out)))
    return out


# ----------------------------------------------------------------------------------------- pooling
class PoolMaxFn(torch.autograd.Function):
    @staticmethod
    @_on_device
    def forward(ctx, x, p):
        _lib.require_device(x)
        ctx.bf16 = x.dtype == BF16       # a max is exact: a bf16 input runs the fp32 kernel and gets its result back in bf16, as torch.max would
        x = x.float().contiguous()       # the kernel reads fp32; the reference's torch.max takes any dtype (gcn.py:246-255)
        q, n, f = x.shape
        out = torch.empty((q, n // p, f), dtype=torch.float32, device=x.device)
        idx = torch.empty((q, n // p, f), dtype=torch.int32, device=x.device)
        _lib.check(_lib.lib().tgcn_pool_max_f32(_lib.stream_ptr(), _lib.ptr(x), _lib.ptr(out), _lib.ptr(idx), q, n, f, p))
        ctx.save_for_backward(idx)
        ctx.shape, ctx.p = (q, n, f), p
        return out.to(BF16) if ctx.bf16 else out

    @staticmethod
    @_on_device
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        q, n, f = ctx.shape
        gi = torch.empty((q, n, f), dtype=torch.float32, device=g.device)
        _lib.check(_lib.lib().tgcn_pool_max_bwd_f32(_lib.stream_ptr(), _lib.ptr(g.float().contiguous()), _lib.ptr(idx), _lib.ptr(gi),
                                                    q, n, f, ctx.p))
        return (gi.to(BF16) if ctx.bf16 else gi), None


# ----------------------------------------------------------------------------------------- bfloat16 layers
BF16 = torch.bfloat16


def param_dtype(weight, bias, what):
    """The compute dtype a layer's parameters pick: float32 (the fp32 path) or bfloat16 (cheb_layer_bf16).  Any other dtype, or a weight
    and a bias of two dtypes, is refused here, before anything launches (the kernels would read the buffers as something they are not)."""
    wd = weight.dtype
    if wd not in (torch.float32, BF16):
        raise _lib.TgcnError("%s: parameters of dtype %s are not supported (float32, or bfloat16 for the bf16 path)" % (what, wd))
    if bias is not None and bias.dtype != wd:
        raise _lib.TgcnError("%s: weight is %s but bias is %s -- convert both (module.to(dtype))" % (what, wd, bias.dtype))
    return wd


def _dense_bf16(t):
    """(nb, rows, C) bf16 view with a contiguous last dim -> tgcn_dense (strides in elements)"""
    assert t.dim() == 3 and t.dtype == BF16 and (t.shape[2] == 1 or t.stride(2) == 1), (t.shape, t.stride())
    return _lib.DenseStruct(t.data_ptr(), int(t.stride(0)), int(t.stride(1)))


def _aligned16_bf16(C_row, *tensors):
    ok = C_row % 8 == 0
    for t in tensors:
        if t is not None:
            ok = ok and t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0
    return ok


def schedule_for_bf16(op, C_row, aligned16):
    """The schedule of a bf16 row of C_row elements: with 16-byte lanes it has the lane shape of an fp32 row of C_row/2 floats, otherwise
    of an unaligned fp32 row of C_row (tgcn_csr_hop_bf16; the operand's schedule cache keys on lanes per row)."""
    return op.schedule_for(C_row // 2, True) if aligned16 else op.schedule_for(C_row, False)


@_on_device
def csr_hop_bf16(op, x, z=None, alpha=1.0, beta=0.0, out=None, z2=None, gamma=0.0):
    """csr_hop on bf16 rows (tgcn_csr_hop2_bf16): y = alpha * L x + beta * z (+ gamma * z2), fp32 sums, y rounded once to bf16."""
    _lib.require_device(x, z, z2)
    L = _lib.lib()
    assert x.dim() == 3 and x.dtype == BF16 and x.shape[1] == op.n_cols, (x.shape, x.dtype, op.n_cols)
    nb, _, Crow = x.shape
    y = torch.empty((nb, op.n, Crow), dtype=BF16, device=x.device) if out is None else out
    for t in (y, z, z2):
        assert t is None or (tuple(t.shape) == (nb, op.n, Crow) and t.dtype == BF16), (t.shape, t.dtype)
    al = _aligned16_bf16(Crow, x, z, y, z2)
    nb_max = 65535 // max(1, -(-Crow // (512 if al else 64)))
    if nb > nb_max:
        for b0 in range(0, nb, nb_max):
            sl = slice(b0, min(nb, b0 + nb_max))
            csr_hop_bf16(op, x[sl], None if z is None else z[sl], alpha, beta, y[sl], None if z2 is None else z2[sl], gamma)
        return y
    sched = schedule_for_bf16(op, Crow, al)
    ws = _workspace(L.tgcn_csr_hop_bf16_workspace_bytes(C.byref(sched.struct), nb, Crow, 1 if al else 0), x.device, floor=16)
    X, Y = _dense_bf16(x), _dense_bf16(y)
    Z = _dense_bf16(z) if z is not None else None
    Z2 = _dense_bf16(z2) if z2 is not None else None
    _lib.check(L.tgcn_csr_hop2_bf16(_lib.stream_ptr(), C.byref(op.struct), C.byref(sched.struct), nb, Crow, C.byref(X),
                                    C.byref(Z) if Z is not None else None, float(alpha), float(beta),
                                    C.byref(Z2) if Z2 is not None else None, float(gamma), C.byref(Y), None, _lib.ptr(ws), ws.numel()))
    return y


@_on_device
def cheb_project_bf16(terms, W, bias, bias_kind, n_vertices, out_dtype=BF16, bias_cols=0, interleave=1):
    """out = sum_t terms[t] @ W[t] + bias (tgcn_cheb_project_bf16): terms: list of (M, Kc) bf16 with contiguous rows, W: (T, Kc, N) bf16, bias
    fp32 / bf16 on the first bias_cols columns (0: all); interleave as in cheb_project.  -> (M, N) in out_dtype (fp32, or rounded once to bf16)."""
    _lib.require_device(W, bias, *terms)
    L = _lib.lib()
    T = len(terms)
    M, Kc = terms[0].shape
    N = W.shape[-1]
    W = W.reshape(T * Kc, N).contiguous()
    dt = out_dtype if T <= 32 else torch.float32       # more than 32 terms: fp32 partial sums across the chunks, one rounding at the end
    out = torch.empty((M, N), dtype=dt, device=W.device)
    b = bias.contiguous() if bias is not None else None
    bdt = _lib.DTYPE_BF16 if (b is not None and b.dtype == BF16) else _lib.DTYPE_F32
    for t0 in range(0, T, 32):
        nt = min(32, T - t0)
        last = t0 + nt >= T
        a = (C.c_void_p * nt)(*[terms[t0 + i].data_ptr() for i in range(nt)])
        lda = (C.c_int64 * nt)(*[terms[t0 + i].stride(0) for i in range(nt)])
        _lib.check(L.tgcn_cheb_project_bf16(_lib.stream_ptr(), M, Kc, N, nt, a, lda, _lib.ptr(W[t0 * Kc:]), _lib.ptr(b) if last else None,
                                            bias_kind if last else 0, bdt, bias_cols, n_vertices, interleave, 1 if t0 > 0 else 0, _lib.ptr(out), N,
                                            _lib.DTYPE_BF16 if dt == BF16 else _lib.DTYPE_F32))
    return out if dt == out_dtype else out.to(out_dtype)


@_on_device
def cheb_wgrad_bf16(terms, g2d):
    """dW[t] = terms[t]^T @ g2d -> (T, Kc, N) fp32 (tgcn_cheb_wgrad_bf16); terms: list of (M, Kc) bf16 with contiguous rows, g2d: (M, N) bf16."""
    _lib.require_device(g2d, *terms)
    L = _lib.lib()
    T = len(terms)
    M, Kc = terms[0].shape
    N = g2d.shape[1]
    dW = torch.empty((T, Kc, N), dtype=torch.float32, device=g2d.device)
    for t0 in range(0, T, 32):
        nt = min(32, T - t0)
        ws = _workspace(L.tgcn_cheb_wgrad_workspace_bytes(M, Kc, N, nt), g2d.device, floor=16)
        a = (C.c_void_p * nt)(*[terms[t0 + i].data_ptr() for i in range(nt)])
        lda = (C.c_int64 * nt)(*[terms[t0 + i].stride(0) for i in range(nt)])
        _lib.check(L.tgcn_cheb_wgrad_bf16(_lib.stream_ptr(), M, Kc, N, nt, a, lda, _lib.ptr(g2d), g2d.stride(0),
                                          _lib.ptr(dW[t0:]), _lib.ptr(ws), ws.numel()))
    return dW


@_on_device
def pack_rows_bf16(src, idx, out):
    """pack_rows on bf16 rows (tgcn_pack_rows_bf16): out[i] = src[idx[i]], the values unchanged"""
    _lib.require_device(src, idx, out)
    assert src.dim() == 2 and src.dtype == BF16 and out.dtype == BF16 and src.stride(1) == 1 and out.is_contiguous()
    assert idx.dtype == torch.int64 and idx.is_contiguous()
    _lib.check(_lib.lib().tgcn_pack_rows_bf16(_lib.stream_ptr(), _lib.ptr(src), src.stride(0), _lib.ptr(idx), idx.numel(), src.shape[1], _lib.ptr(out)))
    return out


@_on_device
def project_mapped_bf16(terms, term_bs, W2d, bias, bias_kind, n_vertices, rowmap, mapped_terms, q, out):
    """out[b, rowmap[m]] = sum_t terms[t][b, row_t(m)] @ W[t] + bias through tgcn_cheb_project_mapped_bf16 (project_mapped on bf16 terms and
    weight, interleave 1); term_bs in elements; out: (q, n_vertices, N) contiguous, bf16 (rounded once) or fp32."""
    T = len(terms)
    Kc = W2d.shape[0] // T
    N = W2d.shape[1]
    M = int(rowmap.numel())
    if M == 0:
        return out
    a = (C.c_void_p * T)(*[t.data_ptr() for t in terms])
    lda = (C.c_int64 * T)(*[Kc] * T)
    a_bs = (C.c_int64 * T)(*term_bs)
    bdt = _lib.DTYPE_BF16 if (bias is not None and bias.dtype == BF16) else _lib.DTYPE_F32
    _lib.check(_lib.lib().tgcn_cheb_project_mapped_bf16(_lib.stream_ptr(), M, Kc, N, T, a, lda, _lib.ptr(W2d), _lib.ptr(bias), bias_kind, bdt, n_vertices,
                                                        _lib.ptr(rowmap), mapped_terms, q, a_bs, n_vertices * N, _lib.ptr(out), N,
                                                        _lib.DTYPE_BF16 if out.dtype == BF16 else _lib.DTYPE_F32))
    return out


def _compact_hops_bf16(plan, x3, buf):
    """buf[k - 1][:, :n_c] = P_k = L^k x for k = 1 .. K-1 on the kept rows of `plan` (bf16 hops: plan.first gathers from x3, plan.rest from
    the previous compact term); buf: (K-1, q, n_c + 1, C) with zero rows n_c.  _compact_hop's rule at 2 bytes per element: one launch per
    sample when a sample's (n_c, C) slab is beyond COMPACT_SLAB_BYTES"""
    q, n_c = x3.shape[0], plan.n_c
    per_sample = q > 1 and n_c * x3.shape[2] * 2 > COMPACT_SLAB_BYTES
    src = x3
    for k in range(buf.shape[0]):
        op = plan.first if k == 0 else plan.rest
        for sl in ([slice(b, b + 1) for b in range(q)] if per_sample else [slice(0, q)]):
            csr_hop_bf16(op, src[sl], out=buf[k][sl, :n_c])
        src = buf[k]


def _compact_q_chunk_bf16(plan, q, K, C_row, device):
    """samples per pass of the compacted bf16 forward: equal passes whose K-1 compact terms stay within COMPACT_WS_FRACTION of the memory that
    is free when the shape is first seen; asked once per shape (no host query on later calls, nor under hipGraph capture)"""
    key = ("bf16", K, C_row, q)
    qc = plan.q_chunk_cache.get(key)
    if qc is None:
        free = torch.cuda.mem_get_info(device)[0]
        per_q = (K - 1) * (plan.n_c + 1) * C_row * 2
        most = int(max(1, min(q, int(free * COMPACT_WS_FRACTION) // max(per_q, 1))))
        passes = -(-q // most)
        qc = plan.q_chunk_cache[key] = -(-q // passes)
    return qc


@_on_device
def compact_forward_bf16(plan, x3, Wt, bias, bias_kind, keep=False):
    """Reference-power layer forward on bf16 tensors with hop tensors for the plan's n_c kept vertices only: K-1 bf16 hops on (q, n_c + 1, C)
    buffers, then two row-mapped bf16 projections written in place into the (q, n, N) bf16 output -- the kept rows (x through plan.rows, the
    compact terms at their own rows) and the left-out rows (x[i] . W'_0 + bias through plan.empty).  Wt: (K, C, N) bf16 in the working basis.
    The samples run in equal passes (_compact_q_chunk_bf16); keep=True is one pass whose compact terms are returned as the basis
    [x3, P_1, ..., P_{K-1}].  Every row holds the bits the uncompacted bf16 layer gives it.  -> (out, terms or None)"""
    _lib.require_device(x3, Wt, bias)
    q, n, Crow = x3.shape
    K, _, N = Wt.shape
    assert x3.is_contiguous() and Wt.is_contiguous() and n == plan.n and 2 <= K <= 32 and x3.dtype == BF16 and Wt.dtype == BF16
    auto = not keep
    qc = _compact_q_chunk_bf16(plan, q, K, Crow, x3.device) if auto else q
    while True:
        try:
            buf = torch.empty((K - 1, qc, plan.n_c + 1, Crow), dtype=BF16, device=x3.device)
            break
        except torch.OutOfMemoryError:
            if not auto or qc <= 1:
                raise
            torch.cuda.empty_cache()
            qc = plan.q_chunk_cache[("bf16", K, Crow, q)] = max(1, qc // 2)      # the cached choice no longer fits: fewer samples per pass from now on
    buf[:, :, plan.n_c].zero_()
    out = torch.empty((q, n, N), dtype=BF16, device=x3.device)
    W2 = Wt.view(K * Crow, N)
    cs = (plan.n_c + 1) * Crow
    for b0 in range(0, q, qc):
        nb = min(qc, q - b0)
        xs, bs = x3[b0:b0 + nb], buf[:, :nb]
        _compact_hops_bf16(plan, xs, bs)
        project_mapped_bf16([xs] + [bs[k] for k in range(K - 1)], [n * Crow] + [cs] * (K - 1), W2, bias, bias_kind, n, plan.rows, 1, nb, out[b0:b0 + nb])
        if plan.n_empty:
            project_mapped_bf16([xs], [n * Crow], W2[:Crow], bias, bias_kind, n, plan.empty, 1, nb, out[b0:b0 + nb])
    return out, ([x3] + [buf[k] for k in range(K - 1)] if keep else None)


@_on_device
def compact_wgrad_bf16(plan, x3, terms, g):
    """dW (K, C, N) fp32 in the working basis from the compact bf16 terms [x3, P_1, ..]: dW_0 = x^T g over every vertex, dW_k = P_k^T g_c for
    k >= 1 with g_c the kept rows of g gathered once (tgcn_pack_rows_bf16) into a zero-tailed (q, n_c + 1, N) buffer; both contractions are
    tgcn_cheb_wgrad_bf16"""
    q, n, Crow = x3.shape
    N = g.shape[2]
    dW0 = cheb_wgrad_bf16([x3.view(q * n, Crow)], g.view(q * n, N))
    if len(terms) == 1:
        return dW0
    g_c = torch.empty((q, plan.n_c + 1, N), dtype=BF16, device=g.device)
    g_c[:, plan.n_c].zero_()
    rows64 = plan.rows64()
    for b in range(q):
        pack_rows_bf16(g[b], rows64, g_c[b, : plan.n_c])
    rest = cheb_wgrad_bf16([t.view(q * (plan.n_c + 1), Crow) for t in terms[1:]], g_c.view(q * (plan.n_c + 1), N))
    return torch.cat([dW0, rest])


def _working_weight_bf16(fold, W):
    """the bf16 weight in the kernels' basis: the fold of the dense-L classes (coefficients +-1 / +-2) runs in fp32 on the upcast weight and
    is rounded to bf16 once"""
    return fold_weight(fold, W.float()).to(BF16) if fold is not None else W


def _basis_bf16(op, x3, K, mode, out=None):
    """the K terms of the layer's basis on bf16 rows, one bf16 hop each: monomials L^k x (MODE_POWER: the basis of the folded weight),
    Chebyshev T_k x (MODE_CHEBYSHEV); term 0 is x3.  out: a (K,) + x3.shape bf16 tensor whose slices the terms are written into (term 0 is
    copied there)"""
    if out is not None:
        out[0].copy_(x3)
    terms = [x3 if out is None else out[0]]
    for k in range(1, K):
        dst = None if out is None else out[k]
        if mode == MODE_POWER or k == 1:
            terms.append(csr_hop_bf16(op, terms[k - 1], out=dst))
        else:
            terms.append(csr_hop_bf16(op, terms[k - 1], z=terms[k - 2], alpha=2.0, beta=-1.0, out=dst))
    return terms


def _forward_pf_bf16(op, x3, Wt, b, bias_kind, mode):
    """project-first form on a bf16 layer: Z = x . [W_0 | ... | W_{K-1}] in fp32 (bias on Z_0), the fp32 Horner / Clenshaw hops on the
    N-wide rows, one rounding"""
    q, n, Crow = x3.shape
    K, _, N = Wt.shape
    Wcat = weight_layout(Wt.float(), 0).to(BF16)                       # (C, K*N): a re-layout of bf16 values, exact
    Z = cheb_project_bf16([x3.view(q * n, Crow)], Wcat.view(1, Crow, K * N), b, bias_kind, n, out_dtype=torch.float32,
                          bias_cols=N).view(q, n, K * N)
    return _adjoint_hops(op, [Z[:, :, k * N:(k + 1) * N] for k in range(K)], mode).to(BF16)


class ChebLayerBf16Fn(torch.autograd.Function):
    """The layer with bf16 parameters: bf16 tensors, fp32 sums, each rounding point once (DESIGN.md "bf16 layers").  Paths (_layer_path):
    "small" -- the fp32 one-launch kernels on the upcast operands, output rounded; "project_first" -- _forward_pf_bf16; otherwise the bf16
    hops and tgcn_cheb_project_bf16 at full size, or, for MODE_POWER on an operand with a compact plan (compact_plan_for, COMPACT_BF16),
    compact_forward_bf16 / compact_wgrad_bf16: hop tensors for the kept vertices only, the same bits in the output (MODE_CHEBYSHEV is not
    compacted: its left-out weight W_0 - W_2 + ... would be one more rounding point).  Backward: dW = basis^T g on the bf16
    matrix pipe (the kept basis, or recomputed with the bf16 hop), fold transposed in fp32, rounded; dx = the layer on (L^T, g, W^T) with
    fp32 adjoint hops on the fp32 output of the bf16 projection, rounded; the bias gradient is reduced in fp32.  The small path's backward
    is the fp32 layer_backward on the upcast operands, each gradient rounded."""

    @staticmethod
    @_on_device
    def forward(ctx, x3, W, bias, op, mode, bias_kind, grad_mode=True):
        x3 = x3.to(BF16).contiguous()
        W = W.contiguous()
        b = bias.to(BF16).contiguous() if bias is not None else None
        K, Crow, N = W.shape
        q, n, _ = x3.shape
        fold = _power_fold(mode, W)
        path = _layer_path(op, q, n, Crow, N, K, mode, compact=False)
        ctx.basis = None
        plan = None
        if path.kind == "hops" and mode == MODE_POWER and COMPACT_BF16:
            plan = compact_plan_for(op, mode, K, q, n, Crow, N)
        if path.kind == "small":
            out = cheb_forward_small(op, x3.float(), W.float(), fold, None if b is None else b.float(), bias_kind, mode).to(BF16)
        else:
            Wt = _working_weight_bf16(fold, W)
            if path.kind == "project_first":
                out = _forward_pf_bf16(op, x3, Wt, b, bias_kind, mode)
            elif plan is not None:
                keep = bool(grad_mode and ctx.needs_input_grad[1] and K * q * (plan.n_c + 1) * Crow * 2 <= KEEP_BASIS_BYTES)
                out, ctx.basis = compact_forward_bf16(plan, x3, Wt.contiguous(), b, bias_kind, keep=keep)
            else:
                terms = _basis_bf16(op, x3, K, mode)
                out = cheb_project_bf16([t.view(q * n, Crow) for t in terms], Wt, b, bias_kind, n).view(q, n, N)
                if grad_mode and ctx.needs_input_grad[1] and K * x3.numel() * 2 <= KEEP_BASIS_BYTES:
                    ctx.basis = terms
        ctx.save_for_backward(x3, W)
        ctx.op, ctx.mode, ctx.bias_kind, ctx.fold, ctx.path, ctx.plan = op, mode, bias_kind, fold, path, plan
        ctx.bias_shape = None if bias is None else bias.shape
        return out

    @staticmethod
    @_on_device
    def backward(ctx, g):
        x3, W = ctx.saved_tensors
        needs = ctx.needs_input_grad
        op, mode, fold = ctx.op, ctx.mode, ctx.fold
        K, Crow, N = W.shape
        q, n, _ = x3.shape
        rnd = lambda t: None if t is None else t.to(BF16)
        if ctx.path.kind == "small":
            gx, gW, gb = layer_backward(op, mode, fold, x3.float(), W.float(), g.float(), ctx.bias_kind, ctx.bias_shape, needs[:3])
            return rnd(gx), rnd(gW), rnd(gb), None, None, None, None
        g = g.to(BF16).contiguous()
        gx = gW = None
        if needs[1] and ctx.plan is not None:
            terms = ctx.basis
            if terms is None:                                           # over KEEP_BASIS_BYTES: the same compact hops again
                buf = torch.empty((K - 1, q, ctx.plan.n_c + 1, Crow), dtype=BF16, device=x3.device)
                buf[:, :, ctx.plan.n_c].zero_()
                _compact_hops_bf16(ctx.plan, x3, buf)
                terms = [x3] + [buf[k] for k in range(K - 1)]
            dW = compact_wgrad_bf16(ctx.plan, x3, terms, g)
            gW = (fold_weight(fold, dW, transpose=True) if fold is not None else dW).to(BF16)
        elif needs[1]:
            terms = ctx.basis if ctx.basis is not None else _basis_bf16(op, x3, K, mode)
            dW = cheb_wgrad_bf16([t.view(q * n, Crow) for t in terms], g.view(q * n, N))
            gW = (fold_weight(fold, dW, transpose=True) if fold is not None else dW).to(BF16)
        ctx.basis = None
        if needs[0]:
            Wt = _working_weight_bf16(fold, W)
            WT = weight_layout(Wt.float(), 2).to(BF16)                  # (N, K*C)
            Gall = cheb_project_bf16([g.view(q * n, N)], WT.view(1, N, K * Crow), None, BIAS_NONE, n,
                                     out_dtype=torch.float32).view(q, n, K * Crow)
            gx = _adjoint_hops(op.transpose(), [Gall[:, :, k * Crow:(k + 1) * Crow] for k in range(K)], mode).to(BF16)
        gb = rnd(_bias_grad(g.float(), ctx.bias_kind, ctx.bias_shape, needs[2]))
        return gx, gW, gb, None, None, None, None


def _pad_rows_bf16(op, x3, weight_kcn, mode):
    """_pad_rows for bf16 rows: on the bf16 hops path rows of C >= 7 elements that are not a multiple of 8 get zero channels up to one
    (16-byte lanes; zero rows in the weight)"""
    K, C, N = weight_kcn.shape
    if C % 8 == 0 or C < 7 or _layer_path(op, x3.shape[0], x3.shape[1], C, N, K, mode, compact=False).kind != "hops":
        return x3, weight_kcn
    pad = (-C) % 8
    return torch.nn.functional.pad(x3, (0, pad)), torch.nn.functional.pad(weight_kcn, (0, 0, 0, pad))


def cheb_layer_bf16(op, x3, weight_kcn, bias, bias_kind, mode, values=None):
    """cheb_layer with bfloat16 parameters: x is cast to bf16 once, output and gradients are bf16 (ChebLayerBf16Fn)."""
    if values is not None:
        raise _lib.TgcnError("cheb_layer: learnable edge weights (edge_weight.requires_grad) are not supported with bfloat16 parameters")
    x3 = x3.to(BF16)
    x3, weight_kcn = _pad_rows_bf16(op, x3, weight_kcn, mode)
    x3, bias = _to_operand_labels(op, x3, bias, bias_kind)        # (the relabelling kernel is fp32: bf16 values pass through it exactly)
    out = ChebLayerBf16Fn.apply(x3, weight_kcn, bias, op, mode, bias_kind, torch.is_grad_enabled())
    return out if op.perm is None else relabel_rows(out, op.inv_perm, op.perm).to(BF16)


class ChebSeriesBf16Fn(torch.autograd.Function):
    """ChebSeriesFn with bfloat16 parameters, at the rounding points of the bf16 layers (DESIGN.md 3.9 / 3.10 "bf16"): the series is bf16 (the
    caller's: check_series_bf16), the stack (K, S, n, ld) comes from the bf16 hops on rows of T*f elements (_basis_bf16: every hop rounds once), the
    weight is folded in fp32 and rounded once (_working_weight_bf16), the sliding-window projection (tgcn_cheb_project_series_conv_bf16) sums in
    fp32, adds the bias in fp32 and rounds once; out is bf16 in either layout.  Rows of T*f >= 7 elements that are no multiple of 8 are padded
    with trailing zeros up to one (ld, the 16-byte hop form) -- never by channels: a time row stays f contiguous elements.
    The plan queries -- the forward's and, when the series needs a gradient, the input gradient's -- are asked before the hops.  A geom with a
    dilation > 1 (at stride 1) takes the _dilated_bf16 entries, planned as step 1.
    Backward (tgcn_cheb_series_conv_backward_bf16): dW fp32 from the bf16 stack (kept at 2 B per element) and the bf16 g, fold transposed in
    fp32, rounded; d series = the fp32 G through the fp32 adjoint hops on L^T, rounded once; the bias gradient is reduced in fp32 and
    rounded."""

    @staticmethod
    @_on_device
    def forward(ctx, series, weight_khfg, bias, op, mode, bias_kind, as_series, geom=(1, 0, 0)):
        L = _lib.lib()
        S, n, T, f = series.shape
        K, H, _, N = weight_khfg.shape
        stride, left, right, dil = _geom4(geom)
        nwin = (T + left + right - (H - 1) * dil - 1) // stride + 1
        hc, lds = C.c_int32(0), C.c_int32(0)
        _lib.check(L.tgcn_series_conv_plan_bf16(H, f, N, int(f % 8 == 0), stride, C.byref(hc), C.byref(lds)))
        if ctx.needs_input_grad[0]:       # the input gradient's own span (phase 0 at step 1 over g as a series of N channels): refused here, not in the backward
            st = min(stride, T + left + right)      # (dilated: stride 1, all H weight time rows in the one launch)
            _lib.check(L.tgcn_series_conv_plan_bf16(-(-H // st), N, K * f, int(N % 8 == 0), 1, C.byref(hc), C.byref(lds)))
        W = weight_khfg.to(BF16).contiguous().view(K, H * f, N)
        fold = _power_fold(mode, W)
        Wt = _working_weight_bf16(fold, W)
        # the series is in the operand's labels already (cheb_time_windows relabelled it): bf16, or its bf16 values in fp32 behind that relabelling
        stack, ld = _series_stack_bf16(op, series.to(BF16).contiguous().view(S, n, T * f), K, mode)
        out = torch.empty((S, n, nwin, N) if as_series else (S * nwin, n, N), dtype=BF16, device=stack.device)
        b = bias.to(BF16).contiguous() if bias is not None else None
        args = (_lib.stream_ptr(), S, n, T, f, H, N, K, _lib.ptr(stack), ld, _lib.ptr(Wt), _lib.ptr(b), _lib.DTYPE_BF16, bias_kind,
                1 if as_series else 0, _lib.ptr(out), stride, left, right)
        if dil > 1:
            _lib.check(L.tgcn_cheb_project_series_dilated_bf16(*args, dil))
        else:
            _lib.check(L.tgcn_cheb_project_series_conv_bf16(*args))
        ctx.save_for_backward(Wt)
        ctx.stack = stack if ctx.needs_input_grad[1] else None       # the basis the weight gradient contracts with g, 2 B per element
        _series_ctx(ctx, op, mode, fold, bias, bias_kind, as_series, (S, n, T, f, H, N, K),
                    bf16=(ld, (series.dtype, weight_khfg.dtype, None if bias is None else bias.dtype)))
        ctx.geom = (stride, left, right, dil) if dil > 1 else (stride, left, right)      # never (): there is no default-geometry bf16 entry
        return out

    @staticmethod
    @_on_device
    def backward(ctx, g):
        return _series_backward(ctx, ctx.saved_tensors[0], g) + (None,) * 5


# ----------------------------------------------------------------------------------------- streaming state
class SeriesStreamState:
    """What a causal time layer keeps between two chunks of a recording (cheb_time_stream, DESIGN.md 3.10 "Streaming state"): the last
    C = (H-1)*dilation time rows of its own hop stack in a ring (K, S, n, ring_ld), in the operand's vertex labels and the layer's dtype --
    slot j (elements j*f ..) holds the row whose absolute index is j (mod C), head = seen mod C is the slot of the oldest row kept, seen
    the number of time rows passed through.  A zero ring is the causal zero padding, so a fresh state starts a recording.  Made for one
    operand, dtype, (S, n, f, K, H) and dilation; updated in place by every call.  H == 1 keeps no ring (C == 0, ring None).
    capturable=True keeps the position on the device -- pos, an int64 tensor {head, seen} next to the ring, read by the kernels and moved
    by a launch of its own -- so that one step captured into a hipGraph can be replayed for the whole recording (GraphedStream).  head and
    seen then READ pos: each read synchronises with the device, so leave them alone between the steps of a hot loop.
    stride is the window step the state was made for (cheb_time_stream(..., stride=s)): the ring is the same -- every row, not every s-th --
    and seen counts INPUT rows; the step only says which windows a chunk returns, so a state serves one step."""

    def __init__(self, op, dtype, S, n, f, K, H, dilation, device, capturable=False, stride=1):
        self.op, self.dtype, self.dilation, self.stride = op, dtype, int(dilation), int(stride)
        self.S, self.n, self.f, self.K, self.H = int(S), int(n), int(f), int(K), int(H)
        self.C = (self.H - 1) * self.dilation
        self.ring_ld = self.C * self.f      # f % 4 == 0 (bf16: 8) makes it a multiple of the 16-byte staging unit; any other f stages narrow
        self.ring = torch.zeros((self.K, self.S, self.n, self.ring_ld), dtype=dtype, device=device) if self.C else None
        self.capturable = bool(capturable)
        self.pos = torch.zeros(2, dtype=torch.int64, device=device) if self.capturable else None
        self._head = self._seen = 0

    @property
    def head(self):
        """slot of the oldest row kept; a capturable state reads it from the device (synchronises)"""
        return int(self.pos[0]) if self.capturable else self._head

    @property
    def seen(self):
        """time rows passed through; a capturable state reads it from the device (synchronises)"""
        return int(self.pos[1]) if self.capturable else self._seen

    def reset(self):
        """start a new recording: zero ring, head = seen = 0 (a capturable state: stream-ordered zero_() of ring and pos, no synchronisation)"""
        if self.ring is not None:
            self.ring.zero_()
        if self.capturable:
            self.pos.zero_()
        self._head = self._seen = 0
        return self

    def mismatch(self, dtype, S, n, f, K, H, dilation, stride=1):
        """None when the state was made for this call's dtype, shape, dilation and stride, else what differs (the operand is
        cheb_time_stream's check)"""
        if self.dtype != dtype:
            return "dtype %s, the call is %s" % (self.dtype, dtype)
        if self.dilation != dilation:
            return "dilation %d, the call has %d" % (self.dilation, dilation)
        if self.stride != stride:
            return "stride %d, the call has %d" % (self.stride, stride)
        if (self.S, self.n, self.f, self.K, self.H) != (S, n, f, K, H):
            return "(S, n, f, K, H) = %s, the call has %s" % ((self.S, self.n, self.f, self.K, self.H), (S, n, f, K, H))
        return None

    def advance(self, Tc):
        """the host's position moves by one chunk; a capturable state's moves on the device (tgcn_series_stream_advance's kernel)"""
        if self.capturable:
            return
        self._seen += Tc
        if self.C:
            self._head = (self._head + Tc) % self.C


def stream_is_capturing():
    """True while the current stream records a hipGraph (torch.cuda.graph); False without touching the device when none is initialised"""
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


def stream_windows(seen, Tc, stride):
    """(m, off) of a chunk of Tc time rows behind `seen` rows at window step `stride`: window j of the causal series ends at absolute row
    j * stride, so the chunk returns the m = ceil((seen + Tc) / stride) - ceil(seen / stride) windows j with seen <= j * stride < seen + Tc,
    the first of them at chunk row off = (-seen) mod stride.  Over the chunks of a recording of T rows the m add up to (T - 1) // stride + 1."""
    return -(-(seen + Tc) // stride) - -(-seen // stride), (-seen) % stride


def _stream_weight(weight_khfg, bias, mode, dtype):
    """(working weight, bias) of a streaming step in the state's dtype: the (K, H*f, N) view of the weight in the kernels' basis -- folded on
    every call, as forward_series does: each chunk is projected with the weight of its own call -- and the contiguous bias"""
    K, H, f, N = weight_khfg.shape
    W = weight_khfg.to(dtype).contiguous().view(K, H * f, N)
    fold = _power_fold(mode, W)
    return (_working_weight_bf16 if dtype == BF16 else _working_weight)(fold, W), None if bias is None else bias.to(dtype).contiguous()


@_on_device
def _stream_chunk(chunk, weight_khfg, bias, op, mode, bias_kind, state, pool=0):
    """one chunk (S, n, Tc, f) in the operand's labels through the ring of `state`, in this order: the plan query; the working weight
    (_stream_weight) and the K-1 hops on rows of Tc*f (_series_stack / _series_stack_bf16); the arguments every entry begins with; the ring's
    position, the host's head or the device's pos; ONE entry -- the projection and the ring update; the position moved.  The entry:
    state.stride > 1 (planned at that step): the _stream_strided entry, H == 1 included; out is (S, n, m, N) (stream_windows), empty when no
    window ends inside the chunk.  H == 1 at step 1: no ring, the _conv entry on the chunk (pool: the pooled series entry), and for a
    capturable state tgcn_series_stream_advance behind it.  pool = 2 / 4 (float32, step 1: cheb_time_stream_relu_pool; planned by
    tgcn_series_pool_plan): the _stream_pool entry, relu + pool as the epilogue, z (S, n/pool, Tc, N).  Else the _stream entry, or for a
    capturable state the _stream_pos entry, which like the strided and the pooled one reads state.pos and moves it on the device."""
    L = _lib.lib()
    S, n, Tc, f = chunk.shape
    K, H, _, N = weight_khfg.shape
    bf16 = state.dtype == BF16
    step = state.stride
    hc, lds = C.c_int32(0), C.c_int32(0)
    if pool:
        _lib.check(L.tgcn_series_pool_plan(H, f, N, int(f % 4 == 0), 1, pool, C.byref(hc), C.byref(lds)))
    elif bf16:
        _lib.check(L.tgcn_series_conv_plan_bf16(H, f, N, int(f % 8 == 0), step, C.byref(hc), C.byref(lds)))
    else:
        _lib.check(L.tgcn_series_conv_plan(H, f, N, int(f % 4 == 0), step, C.byref(hc), C.byref(lds)))
    Wt, b = _stream_weight(weight_khfg, bias, mode, state.dtype)
    if bf16:
        stack, ld = _series_stack_bf16(op, chunk.to(BF16).contiguous().view(S, n, Tc * f), K, mode)
    else:
        stack = _series_stack(op, _aligned_input(chunk.float().contiguous().view(S, n, Tc * f)), K, mode)
    # a capturable state takes only chunks of Tc % step == 0 (stream_precheck): off = 0 and m = Tc / step whatever the device position holds
    m, off = (Tc, 0) if step == 1 else ((Tc // step, 0) if state.capturable else stream_windows(state.seen, Tc, step))
    out = torch.empty((S, n // pool if pool else n, m, N), dtype=state.dtype, device=stack.device)
    # what every entry begins with: the chunk's shape, its stack (bf16: and the stack's ld), the weight and the bias (bf16: and its dtype)
    args = (_lib.stream_ptr(), S, n, Tc, f, H, N, K, _lib.ptr(stack)) + ((ld, _lib.ptr(Wt), _lib.ptr(b), _lib.DTYPE_BF16, bias_kind) if bf16 else
                                                                          (_lib.ptr(Wt), _lib.ptr(b), bias_kind))
    # the ring's position: the device's pos, or the host's head -- with seen above the only reads of a position, both of a host-head state alone
    head, pos = (0, _lib.ptr(state.pos)) if state.capturable else (state.head, None)
    ring = (_lib.ptr(state.ring), state.ring_ld)
    if step > 1:        # H == 1 included; both positions, the step and the first window's row; it moves a device position itself
        entry = L.tgcn_cheb_project_series_stream_strided_bf16 if bf16 else L.tgcn_cheb_project_series_stream_strided_f32
        _lib.check(entry(*args, _lib.ptr(out) if m else None, *ring, head, pos, step, off))
    elif not state.C:   # no ring: the series entry on the chunk itself as a series, at step 1 with no padding
        if pool:
            _lib.check(L.tgcn_cheb_project_series_pool_f32(*args, 1, _lib.ptr(out), None, pool, 1, 0, 0, 1))
        else:
            entry = L.tgcn_cheb_project_series_conv_bf16 if bf16 else L.tgcn_cheb_project_series_conv_f32
            _lib.check(entry(*args, 1, _lib.ptr(out), 1, 0, 0))
    elif pool:         # both positions, as the strided entries take them
        _lib.check(L.tgcn_cheb_project_series_stream_pool_f32(*args, _lib.ptr(out), pool, *ring, head, pos, state.dilation))
    else:               # a host-head entry and a _pos entry, each with the one position it reads
        entry = ((L.tgcn_cheb_project_series_stream_pos_bf16 if bf16 else L.tgcn_cheb_project_series_stream_pos_f32) if state.capturable else
                 (L.tgcn_cheb_project_series_stream_bf16 if bf16 else L.tgcn_cheb_project_series_stream_f32))
        _lib.check(entry(*args, _lib.ptr(out), *ring, pos if state.capturable else head, state.dilation))
    if state.capturable and not state.C and step == 1:      # no ring, but seen still counts: the series entries know no position
        _lib.check(L.tgcn_series_stream_advance(_lib.stream_ptr(), pos, Tc, 0))
    state.advance(Tc)
    return out


# "auto" fuses a step of at most this many time rows: the largest measured Tc at which the fused step beat the parent commit's eager step by
# more than the spread of three repeats of each.  profiles/r14_series_stream_fused.json (DESIGN.md 3.10 "One launch per step"): the fused
# step is slower at Tc = 1, 8 and 64 (1.15 against 0.69 ms per chunk at Tc = 1, spreads under 0.03 ms), so 0 -- "auto" never fuses, and
# fused=True is the opt-in.
STREAM_FUSED_AUTO_MAX_TC = 0


def _stream_small_plan(op, f, H, N, K, Tc, dilation, mode):
    """tgcn_cheb_stream_small_plan on a square operand -> (rc, tb, dense, lds_bytes)"""
    tb, dense, lds = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = _lib.lib().tgcn_cheb_stream_small_plan(op.n, op.nnz, int(mode), int(f), int(H), int(N), int(K), int(Tc), int(dilation),
                                                C.byref(tb), C.byref(dense), C.byref(lds))
    return rc, tb.value, dense.value, lds.value


def stream_fused_supported(op, f, H, N, K, Tc, dilation, mode):
    """True where cheb_time_stream(..., fused=True) runs a float32 step of Tc time rows on this operand: a square operand, a ring (H >= 2)
    and a plan that accepts (tgcn_cheb_stream_small_plan: operand and term buffers in one workgroup's LDS).  A host query: nothing launches."""
    if op.n_cols != op.n or H < 2 or min(f, N, K, Tc, dilation) < 1:
        return False
    return _stream_small_plan(op, f, H, N, K, Tc, dilation, mode)[0] == 0


@_on_device
def _stream_chunk_fused(chunk, weight_khfg, bias, op, mode, bias_kind, state):
    """_stream_chunk's step in one launch (tgcn_cheb_stream_small_f32; float32, H >= 2, a plan that accepted): the fold in power mode with
    K > 2, the fused entry on the chunk itself -- hops, projection and ring update out of LDS -- and, for a capturable state, the advance"""
    L = _lib.lib()
    S, n, Tc, f = chunk.shape
    K, H, _, N = weight_khfg.shape
    Wt, b = _stream_weight(weight_khfg, bias, mode, torch.float32)
    x3 = chunk.float().contiguous().view(S, n, Tc * f)
    out = torch.empty((S, n, Tc, N), dtype=torch.float32, device=x3.device)
    pos = _lib.ptr(state.pos) if state.capturable else None
    _lib.check(L.tgcn_cheb_stream_small_f32(_lib.stream_ptr(), C.byref(op.struct), int(mode), S, Tc, f, H, N, K, _lib.ptr(x3), _lib.ptr(Wt),
                                            _lib.ptr(b), bias_kind, _lib.ptr(out), _lib.ptr(state.ring), state.ring_ld,
                                            0 if state.capturable else state.head, pos, state.dilation))
    if state.capturable:        # behind the step on the same stream: every workgroup has read the old head
        _lib.check(L.tgcn_series_stream_advance(_lib.stream_ptr(), pos, Tc, state.C))
    state.advance(Tc)
    return out


def stream_precheck(chunk, weight, bias, state, dilation, who="cheb_time_stream", capturable=False, fused=False, stride=1):
    """Everything cheb_time_stream refuses that does not need the operand -- the modules run it before they build one.
    -> (dtype, (S, n, f, K, H), the dilation the call runs at)
    stride: an integer >= 1; stride > 1 is refused together with dilation > 1 (series_geometry's rule), with fused=True (the one-launch
    step has no window step; "auto" takes the unfused path), with a state made for another stride, and on a capturable state for a chunk
    with Tc % stride != 0 -- a captured step needs a static output shape, and chunks of whole steps keep off = 0 and m = Tc / stride
    whatever the device position holds (a shape rule: nothing is read from the device)."""
    dt = param_dtype(weight, bias, who)
    if fused is not False and fused is not True and fused != "auto":
        raise _lib.TgcnError("%s: fused is False, True or \"auto\", got %r" % (who, fused))
    if fused is True:       # the one-launch step is fp32 and needs a ring ("auto" takes the general route for both)
        if dt == BF16:
            raise _lib.TgcnError("%s: fused=True runs in float32 only -- the parameters are bfloat16 (fused=False or \"auto\")" % who)
        if weight.dim() in (3, 4) and weight.shape[1] == 1:
            raise _lib.TgcnError("%s: fused=True needs a ring, and a one-tap layer (H = 1) keeps none (fused=False or \"auto\")" % who)
    if chunk.dim() not in (3, 4) or weight.dim() != chunk.dim():
        raise _lib.TgcnError("%s: a (S, n, Tc) chunk takes a (K, H, N) weight and a (S, n, Tc, f) chunk a (K, H, f, N) weight (got %s and %s)"
                             % (who, tuple(chunk.shape), tuple(weight.shape)))
    f = chunk.shape[3] if chunk.dim() == 4 else 1
    if chunk.dim() == 4 and weight.shape[2] != f:
        raise _lib.TgcnError("%s: the chunk has %d channels, the weight %d" % (who, f, weight.shape[2]))
    S, n, Tc = chunk.shape[:3]
    K, H, N = weight.shape[0], weight.shape[1], weight.shape[-1]
    if Tc < 1:
        raise _lib.TgcnError("%s: a chunk holds at least one time row, got %s" % (who, tuple(chunk.shape)))
    series_geometry(Tc, H, stride, "causal", who, dilation)  # the dilation's and the step's rules (not both above 1); causal padding is the only one
    stride = int(stride)
    if stride > 1 and fused is True:
        raise _lib.TgcnError("%s: fused=True has no window step (stride=%d) -- the one-launch step runs at stride 1 (fused=False or \"auto\")"
                             % (who, stride))
    dilation = series_dilation(H, dilation)
    if dt == BF16 and chunk.dtype != BF16:
        raise _lib.TgcnError("%s: the parameters are bfloat16 but the chunk is %s -- cast it once (chunk.to(torch.bfloat16))" % (who, chunk.dtype))
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (chunk, weight, bias)):
        raise _lib.TgcnError("%s: streaming has no backward -- call it under torch.no_grad() (training stays with forward_series / "
                             "cheb_time_windows)" % who)
    if state is not None:
        if not isinstance(state, SeriesStreamState):
            raise _lib.TgcnError("%s: state is a SeriesStreamState or None, got %s" % (who, type(state).__name__))
        bad = state.mismatch(dt, S, n, f, K, H, dilation, stride)
        if bad:
            raise _lib.TgcnError("%s: the state was made for %s -- one state per layer and recording batch" % (who, bad))
        if capturable and not state.capturable:
            raise _lib.TgcnError("%s: capturable=True with a state that keeps its head on the host -- the state's kind rules; start the "
                                 "recording with state=None, capturable=True" % who)
    if stride > 1 and (state.capturable if state is not None else capturable) and Tc % stride:
        raise _lib.TgcnError("%s: a capturable state with stride=%d takes chunks of whole steps (Tc %% stride == 0), got Tc = %d -- a captured "
                             "step needs a static output shape" % (who, stride, Tc))
    # a head kept on the host is a launch argument: a captured step would replay the head of the capture on every chunk
    if (H - 1) * dilation > 0 and not (state.capturable if state is not None else capturable) and stream_is_capturing():
        raise _lib.TgcnError("%s: the stream is capturing a hipGraph and the state keeps its ring position on the host, which a replay "
                             "cannot move -- make the state with capturable=True (tgcn_amd.GraphedStream captures a chain)" % who)
    return dt, (S, n, f, K, H), dilation


def _stream_enter(op, chunk, weight, bias, bias_kind, state, dt, dims, dilation, capturable, stride=1):
    """what the two cheb_time_stream* functions do behind their refusals (stream_precheck's answers in dt, dims, dilation) and in front of
    the step -> (chunk (S, n, Tc, f), weight (K, H, f, N), bias, state): tensors on one device, a new state where none came, a 3-D chunk
    and weight unsqueezed, chunk and bias in the operand's labels -- the ring lives in them"""
    _lib.require_device(chunk, weight, bias)
    if state is None:
        S, n, f, K, H = dims
        state = SeriesStreamState(op, dt, S, n, f, K, H, dilation, chunk.device, capturable=capturable, stride=stride)
    if chunk.dim() == 3:
        chunk, weight = chunk.unsqueeze(3), weight.unsqueeze(2)
    chunk, bias = _to_operand_labels(op, chunk, bias, bias_kind)
    return chunk, weight, bias, state


def _stream_leave(op, out, dt):
    """a step's output back in the caller's labels (a reordered operand; an output without windows has nothing to relabel), in the layer's
    dtype: the relabelling kernel is fp32, and bf16 values pass through it exactly"""
    if op.perm is not None and out.shape[2]:
        out = relabel_rows(out, op.inv_perm, op.perm).to(dt)
    return out


def cheb_time_stream(op, chunk, weight, bias, bias_kind, mode=MODE_POWER, state=None, dilation=1, capturable=False, fused=False, stride=1):
    """The causal streaming layer on the NEXT Tc time rows of S recordings (inference only): chunk (S, n, Tc) with weight (K, H, N), or
    (S, n, Tc, f) with weight (K, H, f, N) -> (out (S, n, Tc, N) contiguous, state).  out equals rows [state.seen, state.seen + Tc) of
    cheb_time_windows(op, whole, ..., as_series=True, padding="causal", dilation=dilation) on the whole series: the layer keeps the last
    (H-1)*dilation time rows of its hop stack in state's ring (SeriesStreamState), the projection reads each window from the ring and the
    chunk's stack, and every time row is hopped once.  state=None starts a recording (a zero ring = the causal padding); the state is updated
    in place and returned.  The series layout is the only one: a chain is l2(relu(o1), s2) with one state per layer.
    TgcnError before an operand is relabelled or anything launches: a state made for another operand, dtype, shape or dilation; grad mode with
    a chunk or a parameter that requires grad (there is no backward: torch.no_grad(); training stays with cheb_time_windows); bfloat16
    parameters with a chunk of another dtype; dilation < 1.  H == 1 keeps no ring and runs the _conv entry on the chunk.
    capturable=True with state=None makes a state whose ring position lives on the device (SeriesStreamState), the kind a step captured
    into a hipGraph needs; with a state given the state's kind rules, and capturable=True next to a host-head state is a TgcnError.  A
    host-head state with a ring is refused while the current stream is capturing: its replay would read a stale head.
    fused=True runs the step in ONE launch (tgcn_cheb_stream_small_f32: hops, projection and ring update out of LDS, one workgroup per
    recording) on the same state -- fused and unfused calls may alternate within a recording.  It asks the plan first and raises TgcnError
    before anything launches for bfloat16 parameters, H = 1, a non-square operand and a plan that refuses (stream_fused_supported tells).
    fused="auto" fuses where the plan accepts and Tc <= STREAM_FUSED_AUTO_MAX_TC, and is fused=False everywhere else.  The results agree to
    rounding (the hops add their neighbours in another order), not bit for bit.
    stride=s (an integer >= 1, a property of the state like the dilation) returns only the windows of cheb_time_windows(op, whole, ...,
    as_series=True, padding="causal", stride=s) that END inside the chunk.  Window j ends at absolute row j*s, so with seen = state.seen
    the call returns the m = ceil((seen + Tc)/s) - ceil(seen/s) windows j in [ceil(seen/s), ceil((seen + Tc)/s)), the first at chunk row
    off = (-seen) mod s: out is (S, n, m, N), and over a recording of T rows the m add up to (T-1)//s + 1.  The hops, the ring (every
    row, not every s-th) and the position run as at stride 1, and seen counts INPUT rows.  m may be 0 (host-head states only, e.g.
    Tc = 1 at an odd seen with s = 2): out is then an empty (S, n, 0, N) tensor and no projection launches; a chain skips its later
    layers for such a chunk, because an empty chunk is still refused.  A capturable state takes only chunks with Tc % s == 0 (off = 0,
    m = Tc/s on every step: a captured step has a static shape).  TgcnError before anything launches: stride > 1 with dilation > 1, with
    fused=True (fused="auto" runs unfused), with a state of another stride."""
    dt, (S, n, f, K, H), dilation = stream_precheck(chunk, weight, bias, state, dilation, capturable=capturable, fused=fused, stride=stride)
    stride = int(stride)
    if stride > 1:
        fused = False       # "auto": the one-launch step has no window step (True was refused above)
    if state is not None and state.op is not op:
        raise _lib.TgcnError("cheb_time_stream: the state was made for another operand -- one state per layer and graph")
    if fused is not False:
        Tc, N = chunk.shape[2], weight.shape[-1]
        if fused is True:
            if op.n_cols != op.n:
                raise _lib.TgcnError("cheb_time_stream: fused=True needs a square operand, got %d x %d" % (op.n, op.n_cols))
            if _stream_small_plan(op, f, H, N, K, Tc, dilation, mode)[0] != 0:
                raise _lib.TgcnError("cheb_time_stream: fused=True, but n = %d, nnz = %d, f = %d, N = %d do not fit the one-launch step "
                                     "(stream_fused_supported; fused=False or \"auto\")" % (op.n, op.nnz, f, N))
        else:
            fused = (dt != BF16 and H >= 2 and Tc <= STREAM_FUSED_AUTO_MAX_TC and op.n_cols == op.n
                     and _stream_small_plan(op, f, H, N, K, Tc, dilation, mode)[0] == 0)
    with torch.no_grad():
        chunk, weight, bias, state = _stream_enter(op, chunk, weight, bias, bias_kind, state, dt, (S, n, f, K, H), dilation, capturable, stride)
        out = (_stream_chunk_fused if fused else _stream_chunk)(chunk, weight, bias, op, mode, bias_kind, state)
        return _stream_leave(op, out, dt), state


def cheb_time_stream_relu_pool(op, chunk, weight, bias, bias_kind, mode, pool, state=None, dilation=1, capturable=False):
    """cheb_time_stream with relu and the max over `pool` consecutive vertices in the projection's epilogue (inference only): chunk
    (S, n, Tc[, f]) -> (z (S, n/pool, Tc, N), state), z bit-identical to tgcn_relu_pool_f32 on cheb_time_stream's out.  The state is
    cheb_time_stream's own and leaves the call as that function leaves it, so pooled and unpooled steps may alternate within a recording
    and GraphedStream captures a chain with pooled layers unchanged; state, dilation and capturable as there.
    A reordered operand runs the unfused composition (series_pool_is_fused).  TgcnError before anything launches: bfloat16 parameters,
    pool outside {2, 4}, n % pool != 0, and every refusal cheb_time_stream makes; there is no fused= and no stride= (a state made for a
    window step is refused as a state of another stride)."""
    who = "cheb_time_stream_relu_pool"
    if param_dtype(weight, bias, who) == BF16:
        raise _lib.TgcnError("%s: bfloat16 parameters are not supported (run the layer, then gcn_pool / gcn_pool_4)" % who)
    dt, (S, n, f, K, H), dilation = stream_precheck(chunk, weight, bias, state, dilation, who, capturable=capturable)
    pool = check_pool(pool, n, who)
    if state is not None and state.op is not op:
        raise _lib.TgcnError("%s: the state was made for another operand -- one state per layer and graph" % who)
    with torch.no_grad():
        chunk, weight, bias, state = _stream_enter(op, chunk, weight, bias, bias_kind, state, dt, (S, n, f, K, H), dilation, capturable)
        if series_pool_is_fused(op, pool, stream=True):
            return _stream_chunk(chunk, weight, bias, op, mode, bias_kind, state, pool=pool), state
        out = _stream_chunk(chunk, weight, bias, op, mode, bias_kind, state)
        return _relu_pool_view(_stream_leave(op, out, dt), pool), state
