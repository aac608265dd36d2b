"""Drop-in modules: the class surface of tgcn/nn/gcn.py (and tgcn/nn/gcn_matmul.py) on the HIP path.

Same constructor / forward signatures, parameter names, shapes and initialisation as the reference
(state_dict compatible); `L` stays a plain attribute (not saved, not moved by .to(), gcn.py:18,92,168).
The forward of every class is one call into libtgcn_hip.so (K-1 CSR hops + MFMA projection); nothing here
falls back to torch ops or the CPU.
"""
import collections
import math
import threading

import torch
from torch.nn import Parameter

from . import _lib, functional as F
from .graph import GraphOperand


def uniform(size, tensor):
    """U(-1/sqrt(size), 1/sqrt(size)) in place; None is ignored (reference: tgcn/nn/gcn.py:240-243)."""
    bound = 1.0 / math.sqrt(size)
    if tensor is not None:
        tensor.data.uniform_(-bound, bound)


def gcn_pool(x):
    """Max over pairs of consecutive vertices, (q,n,f)->(q,n/2,f) (reference: gcn.py:246-249)."""
    return F.PoolMaxFn.apply(x, 2)


def gcn_pool_4(x):
    """Max over 4 consecutive vertices (reference: gcn.py:252-255)."""
    return F.PoolMaxFn.apply(x, 4)


class _OperandCache:
    """One GraphOperand per (source object identity, version, device): DataParallel replicas on other devices
    and in-place edits of L / edge_index get their own.  An entry keeps its source objects alive: identity and
    data_ptr only name a tensor while it exists -- once freed, the allocator may hand the same address (and Python the
    same id) to a new edge_index of the same shape, which must not find the old operand."""

    MAX_ENTRIES = 16      # least recently used beyond this (a per-subject edge_index in a training loop: pygeo_hcp.py:284 swaps the graph per subject)

    def __init__(self):
        self._d = collections.OrderedDict()
        self._lock = threading.Lock()     # nn.DataParallel runs the replicas' forwards in threads that share this object

    # copies and pickles of a module start with an empty cache (entries hold device pointers in ctypes structs)
    def __deepcopy__(self, memo):
        return _OperandCache()

    def __getstate__(self):
        return {}

    def __setstate__(self, state):
        self._d = collections.OrderedDict()
        self._lock = threading.Lock()

    def peek(self, key):
        """the cached object of `key` or None; builds nothing and leaves the order of use alone"""
        with self._lock:
            hit = self._d.get(key)
            return None if hit is None else hit[0]

    def get(self, key, build, sources=()):
        with self._lock:
            hit = self._d.get(key)
            if hit is None:
                if F.stream_is_capturing():       # a build synchronises (and allocates outside torch): not inside a hipGraph capture
                    raise _lib.TgcnError(_BUILD_IN_CAPTURE)
                hit = self._d[key] = (build(), tuple(sources))
                while len(self._d) > self.MAX_ENTRIES:        # evict the least recently used entry only: the others keep their operands
                    self._d.popitem(last=False)
            else:
                self._d.move_to_end(key)
            return hit[0]


_BUILD_IN_CAPTURE = ("tgcn_amd: a graph operand would have to be built while the current stream is capturing a hipGraph, and the build "
                     "synchronises -- the operand has to be built by a warm-up step on the same graph arguments (the same L / edge_index / "
                     "edge_weight objects, unchanged) before the capture begins")
_LEARNABLE_IN_CAPTURE = ("tgcn_amd: learnable edge weights (edge_weight.requires_grad) cannot run inside a hipGraph capture -- the operand's "
                         "values are re-packed from the weight by host-driven passes that synchronise, and a replay would not repeat them; "
                         "train edge weights with the eager step")
_warmup_notes = None      # a list while a GraphedTrainStep warm-up runs: what the step did that a capture cannot (graphed.py reads it)


def _np_fingerprint(L):
    """scipy / ndarray operands carry no version counter: tag the first and last stored values so that an in-place
    edit is (very likely) noticed."""
    from .numpy_api import _fingerprint
    return _fingerprint(L)


def _compute_dtype(module, edge_weight=None):
    """The dtype a module computes in, from its parameters (F.param_dtype): float32, or bfloat16 when the weight is bf16 -- the input is then
    cast to bf16 once.  Refuses any other dtype, mixed weight / bias dtypes and, for bf16, learnable edge weights, before anything launches."""
    dt = F.param_dtype(module.weight, module.bias, type(module).__name__)
    if dt == torch.bfloat16 and edge_weight is not None and edge_weight.requires_grad:
        raise _lib.TgcnError("%s: learnable edge weights (edge_weight.requires_grad) are not supported with bfloat16 parameters" % type(module).__name__)
    return dt


def _tensor_key(t):
    return None if t is None else (t.data_ptr(), t._version, tuple(t.shape), str(t.device))


class _DenseLBase(torch.nn.Module):
    """Shared plumbing of the three classes that take L in the constructor."""

    def _operand_key(self, device):
        L = self.L
        dense = isinstance(L, torch.Tensor) and L.layout == torch.strided
        return (id(L), L.data_ptr() if dense else None, getattr(L, "_version", 0), tuple(L.shape) if hasattr(L, "shape") else None,
                str(device), None if isinstance(L, torch.Tensor) else _np_fingerprint(L))

    def _operand(self, device):
        L = self.L
        return self._ops.get(self._operand_key(device), lambda: GraphOperand.from_any(L, device), sources=(L,))

    def _num_vertices(self):
        return self.L.shape[0] if hasattr(self.L, "shape") else self.L[0].shape[0]

    def reset_parameters(self):
        size = self.in_channels * self.weight.size(0)
        uniform(size, self.weight)
        uniform(size, self.bias)

    def __repr__(self):
        return '{}({}, {}, filter_order={})'.format(self.__class__.__name__, self.in_channels, self.out_channels,
                                                    self.weight.size(0))

    def _stack(self, X4):
        """X4: (q, n, h, f) or (q, n, f) -> stack (K, ...) in the reference_power recursion."""
        sh = X4.shape
        x3 = X4.reshape(sh[0], sh[1], -1).float().contiguous()
        st = F.cheb_stack(self._operand(x3.device), x3, self.filter_order, F.MODE_POWER)
        return st.reshape((self.filter_order,) + tuple(sh))


class TGCNCheb(_DenseLBase):
    """reference: tgcn/nn/gcn.py:8-79.  x (q, n, f) -> (q, n, g); weight (K, f, g); bias (1, n, g)."""

    def __init__(self, L, in_channels, out_channels, filter_order, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = Parameter(torch.Tensor(filter_order, in_channels, out_channels))
        self.L = L
        self.filter_order = filter_order
        self._ops = _OperandCache()
        if bias:
            self.bias = Parameter(torch.Tensor(1, self._num_vertices(), out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def _layer_args(self, x):
        x3 = x.to(_compute_dtype(self)).contiguous()
        return (self._operand(x3.device), x3, self.weight, self.bias,
                F.BIAS_NONE if self.bias is None else F.BIAS_VERTEX_CHANNEL, F.MODE_POWER)

    def forward(self, x):
        return F.cheb_layer(*self._layer_args(x))

    def _time_chebyshev(self, X):
        return self._stack(X)


class TGCNCheb_H(_DenseLBase):
    """reference: tgcn/nn/gcn.py:82-154.  x (q, n, h[, f]) -> (q, n, g); weight (K, H, f, g); bias (1, n, g)."""

    def __init__(self, L, in_channels, out_channels, filter_order, horizon, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = Parameter(torch.Tensor(filter_order, horizon, in_channels, out_channels))
        self.L = L
        self.filter_order = filter_order
        self._ops = _OperandCache()
        if bias:
            self.bias = Parameter(torch.Tensor(1, self._num_vertices(), out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def _layer_args(self, x):
        dt = _compute_dtype(self)
        if x.dim() == 3:
            x = x.unsqueeze(3)
        q, n, h, f = x.shape
        x3 = x.to(dt).reshape(q, n, h * f).contiguous()
        W = self.weight.reshape(self.weight.shape[0], h * f, self.out_channels)
        return (self._operand(x3.device), x3, W, self.bias,
                F.BIAS_NONE if self.bias is None else F.BIAS_VERTEX_CHANNEL, F.MODE_POWER)

    def forward(self, x):
        return F.cheb_layer(*self._layer_args(x))

    def _time_chebyshev(self, X):
        if X.dim() == 3:
            X = X.unsqueeze(3)
        return self._stack(X)

    def forward_series(self, series, as_series=False, stride=1, padding=0, dilation=1, time_chunk=None, fused=False):
        """Additive API (not in the reference): series (S, n, T) or (S, n, T, f) raw recordings, f == in_channels -> the layer's output
        for all T-H+1 sliding windows of every recording without materialising the windows (load/data_hcp.py:116-154 builds them on
        the host and the hops then run H times too often): layer(xw) for xw[s*(T-H+1) + w, i, h, c] = series[s, i, w + h, c].
        as_series=False returns (S*(T-H+1), n, g), the order of that batch; as_series=True the same numbers as (S, n, T-H+1, g),
        contiguous -- a series again, so layer2.forward_series(act(layer1.forward_series(x, as_series=True))) chains two time layers with
        no transpose and no windows.  Differentiable: the backward runs the hops once per call too.
        stride, padding: the layer as a convolution over time (F.cheb_time_windows): padding = p, (left, right) or "causal" (H-1 zero time
        rows in front, so a chain keeps its outputs aligned with the input's time axis), each side at most H-1; stride keeps every
        stride-th window.  nwin = (T + left + right - H) // stride + 1 replaces T-H+1 above.
        dilation: the taps of a window lie that many time rows apart, xw[., i, h, c] = padded_series[s, i, w*stride + h*dilation, c]; the
        window spans He = (H-1)*dilation + 1 rows and He replaces H in the padding rules and in nwin ("causal" = He-1 rows in front).
        dilation > 1 needs stride=1.  A causal chain with dilations 1, 2, 4, ... sees hundreds of time steps with a few taps per layer.
        time_chunk=Tc (an integer >= 1; None: the calls above) trains on recordings whose hop stack does not fit: the same tensor and the
        same gradients, computed Tc time rows at a time through the streaming ring of forward_stream in both directions, so that memory
        follows the chunk and nothing of size K*T is allocated (F.ChebSeriesChunkFn; one more hop pass in the backward).  The causal
        layer at step 1 only: padding="causal", stride=1, any dilation, float32 parameters, either layout -- TgcnError before the operand
        is built for anything else.  The causal output has T rows; the windows that lie inside the recording are out[:, :, He-1:]
        (as_series=True) of it.
        fused=True runs the layer's forward in one launch on a graph that fits in LDS (float32, stride=1, no time_chunk, any legal
        padding and dilation, either layout; the backward is the unfused one on a stack the same launch writes when the weight trains).
        TgcnError where it cannot -- before the operand is built for bfloat16 parameters, stride > 1 and a time_chunk, before anything
        launches for a reordered operand and a shape the plan refuses (F.series_fused_supported).  fused="auto" fuses where that is
        measured to pay (F.SERIES_FUSED_AUTO) and is the fused=False call elsewhere."""
        return _forward_series(self, "TGCNCheb_H.forward_series", series, None, None, as_series, stride, padding, dilation, time_chunk, fused)

    def forward_stream(self, chunk, state=None, dilation=1, capturable=False, fused=False, stride=1):
        """Additive API, inference only: the causal layer on the next Tc time rows of S recordings.  chunk (S, n, Tc) or (S, n, Tc, f) ->
        (out (S, n, Tc, g) contiguous, state); out equals rows [seen, seen + Tc) of forward_series(whole, as_series=True, padding="causal",
        dilation=dilation), seen = the time rows already passed through state (F.SeriesStreamState: the last (H-1)*dilation rows of the hop
        stack in a ring, updated in place; None starts a recording, state.reset() another one).  Every time row is hopped once and memory
        follows the chunk, not the recording.  A chain keeps one state per layer: l2.forward_stream(relu(o1), s2, dilation=2).
        No autograd (TgcnError in grad mode when the chunk or a parameter requires grad: use torch.no_grad()); training stays with
        forward_series.  A state of another shape, dtype, dilation or layer raises TgcnError before anything launches.
        capturable=True (with state=None; afterwards the state's kind rules) keeps the ring's position on the device, so that the step can
        be captured into a hipGraph and replayed -- GraphedStream does the capture; state.head / state.seen then synchronise when read.
        A state that keeps its head on the host is refused (TgcnError) while the current stream is capturing.
        fused=True runs the step in one launch on a graph that fits in LDS (float32, H >= 2; TgcnError where it cannot:
        F.stream_fused_supported), fused="auto" where that is measured to pay (F.STREAM_FUSED_AUTO_MAX_TC); the state is the same, so
        fused and unfused calls may alternate (F.cheb_time_stream).
        stride=s (an integer >= 1; the state is made for one step) returns the rows of forward_series(whole, as_series=True,
        padding="causal", stride=s) whose window ENDS inside the chunk: window j ends at absolute row j*s, so the call returns
        m = ceil((seen + Tc)/s) - ceil(seen/s) rows, the first at chunk row off = (-seen) mod s, as (S, n, m, g); over a recording of T
        rows the m add up to (T-1)//s + 1.  The ring still keeps every row and seen counts input rows.  m may be 0 (host-head states):
        the call returns an empty (S, n, 0, g) tensor, and a chain skips its later layers for that chunk -- forward_stream refuses an
        empty chunk.  A capturable state takes chunks with Tc % s == 0 only (m = Tc/s on every step, so GraphedStream's next layer sees
        chunks of Tc/s rows).  TgcnError: stride > 1 with dilation > 1, with fused=True ("auto" runs unfused), with a state of another
        stride."""
        return _forward_stream(self, "TGCNCheb_H.forward_stream", chunk, None, None, state, dilation, capturable, fused, stride)


def _state_operand_check(module, state, key):
    """A state belongs to the operand object it was made with, and that operand is still in the module's cache under this call's key when the
    call continues its recording.  Anything else -- another layer's state, another graph, a graph the cache has evicted since -- is refused
    here, by a look into the cache, so that no operand is built for a call that is refused."""
    if state is not None and module._ops.peek(key) is not state.op:
        raise _lib.TgcnError("%s.forward_stream: the state was made for another operand -- one state per layer and graph (a graph this "
                             "layer's operand cache no longer holds starts a new recording: state=None)" % type(module).__name__)


def _stream_args(module, chunk):
    """(chunk, weight) of a forward_stream call as F.cheb_time_stream takes them, after the shape checks (_series_args' rules)"""
    name = type(module).__name__
    K, H, f, g = module.weight.shape
    if chunk.dim() not in (3, 4):
        raise _lib.TgcnError("%s.forward_stream: the chunk is (S, n, Tc) or (S, n, Tc, f), got %s" % (name, tuple(chunk.shape)))
    if (chunk.shape[3] if chunk.dim() == 4 else 1) != f:
        raise _lib.TgcnError("%s.forward_stream: the chunk has %d channel(s), the layer in_channels = %d"
                             % (name, chunk.shape[3] if chunk.dim() == 4 else 1, f))
    return chunk, (module.weight.reshape(K, H, g) if chunk.dim() == 3 else module.weight)


def _series_args(module, series, stride=1, padding=0, dilation=1):
    """(series, weight, (stride, left, right, dilation)) of a forward_series call as F.cheb_time_windows takes them -- a 3-D series with the (K, H, g) weight, a 4-D one with
    (K, H, f, g) -- after the shape and geometry checks: TgcnError before anything is built or launched."""
    name = type(module).__name__
    K, H, f, g = module.weight.shape
    if series.dim() not in (3, 4):
        raise _lib.TgcnError("%s.forward_series: the series is (S, n, T) or (S, n, T, f), got %s" % (name, tuple(series.shape)))
    if (series.shape[3] if series.dim() == 4 else 1) != f:
        raise _lib.TgcnError("%s.forward_series: the series has %d channel(s), the layer in_channels = %d"
                             % (name, series.shape[3] if series.dim() == 4 else 1, f))
    stride, left, right, _ = F.series_geometry(series.shape[2], H, stride, padding, "%s.forward_series" % name, dilation)
    return series, (module.weight.reshape(K, H, g) if series.dim() == 3 else module.weight), (stride, left, right, F.series_dilation(H, dilation))


def _time_operand(layer, x, edge_index, edge_weight, key=False):
    """the operand a time layer runs the series or chunk x on -- TGCNCheb_H's L on x's device, ChebTimeConv's graph arguments on x's
    vertices and device -- built and cached by the layer; key=True: only its key in the layer's cache, nothing is built"""
    get = layer._operand_key if key else layer._operand
    return get(x.device) if isinstance(layer, _DenseLBase) else get(x, edge_index, edge_weight)


def _forward_series(layer, who, series, edge_index, edge_weight, as_series, stride, padding, dilation, time_chunk, fused):
    """the two forward_series methods behind their own refusals: every refusal that needs no operand, the operand, F.cheb_time_windows"""
    bf16 = _compute_dtype(layer, edge_weight) == torch.bfloat16      # F.cheb_time_windows routes it: every call but the scalar-load form
    F.check_series_fused(fused, stride, time_chunk, bf16, who)
    series, W, geom = _series_args(layer, series, stride, padding, dilation)
    F.check_time_chunk(time_chunk, stride, padding, bf16, who)
    if bf16:
        F.check_series_bf16(layer.weight.shape[2], as_series, geom, series.dtype)
    op = _time_operand(layer, series, edge_index, edge_weight)
    return F.cheb_time_windows(op, series, W, *_series_pool_bias(layer), as_series=as_series, stride=geom[0],
                               padding=geom[1:3] if time_chunk is None else "causal", dilation=geom[3], time_chunk=time_chunk, fused=fused)


def _forward_stream(layer, who, chunk, edge_index, edge_weight, state, dilation, capturable, fused, stride):
    """the two forward_stream methods behind their own refusals: every refusal that needs no operand -- a state made for another one
    among them, by a look at the key -- then the operand and F.cheb_time_stream"""
    _compute_dtype(layer, edge_weight)
    chunk, W = _stream_args(layer, chunk)
    F.stream_precheck(chunk, W, layer.bias, state, dilation, who, capturable, fused=fused, stride=stride)
    _state_operand_check(layer, state, _time_operand(layer, chunk, edge_index, edge_weight, key=True))
    op = _time_operand(layer, chunk, edge_index, edge_weight)
    return F.cheb_time_stream(op, chunk, W, *_series_pool_bias(layer), state=state, dilation=dilation, capturable=capturable, fused=fused,
                              stride=stride)


class GCNCheb(_DenseLBase):
    """reference: tgcn/nn/gcn.py:158-237.  x (q, n[, f]) -> (q, n, g); weight (K, f, g); bias (1, 1, g)."""

    def __init__(self, L, in_channels, out_channels, filter_order, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = Parameter(torch.Tensor(filter_order, in_channels, out_channels))
        self.L = L
        self.filter_order = filter_order
        self._ops = _OperandCache()
        if bias:
            self.bias = Parameter(torch.Tensor(1, 1, out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def _layer_args(self, x):
        dt = _compute_dtype(self)
        if x.dim() == 2:
            x = x.unsqueeze(2)
        x3 = x.to(dt).contiguous()
        return (self._operand(x3.device), x3, self.weight, self.bias,
                F.BIAS_NONE if self.bias is None else F.BIAS_CHANNEL, F.MODE_POWER)

    def forward(self, x):
        return F.cheb_layer(*self._layer_args(x))

    def _chebyshev(self, X):
        if X.dim() == 2:
            X = X.unsqueeze(2)
        return self._stack(X)


# ------------------------------------------------------------------------------------ COO helpers
_spmm_ops = _OperandCache()


def _stamp(t):
    return (t.data_ptr(), t._version)


def _refresh_values(op, weight, make_vals):
    """A LEARNABLE weight changes every optimizer step (and a computed one is a new tensor every forward) while the pattern stays: the operand is
    cached by pattern and only its packed values are refreshed in place (GraphOperand.update_values) -- a cache keyed on the weight's version would
    rebuild CSR, schedule and transpose per step and keep up to 16 stale operands alive.
    "Has the weight changed" = (data_ptr, _version) against the stamp of the last packing.  That pair only names a tensor while its storage is
    alive -- a freed weight's address can be handed to the next one, version 0 again -- so the operand holds the detached alias of the tensor it
    was packed from (shares storage and version counter, keeps no autograd graph): same address then means same storage, and its version counter
    says whether it was written."""
    if _warmup_notes is not None:
        _warmup_notes.append(_LEARNABLE_IN_CAPTURE)
    if F.stream_is_capturing():
        raise _lib.TgcnError(_LEARNABLE_IN_CAPTURE)
    stamp = _stamp(weight)
    if getattr(op, "_packed_stamp", None) != stamp:
        with op._lock:
            if getattr(op, "_packed_stamp", None) != stamp:
                op.update_values(make_vals())
                op._packed_alias = weight.detach()
                op._packed_stamp = stamp
    return op


def _coo_operand(index, value, m, device, n_cols=None):
    """m x n_cols operand: the reference's gather / scatter_add form takes any number of source rows (gcn.py:296-308)."""
    n_cols = int(m if n_cols is None else n_cols)
    if value.requires_grad:          # learnable values: one operand per PATTERN, values refreshed in place
        key = ("learnable", _tensor_key(index), int(m), n_cols, str(device))
        op = _spmm_ops.get(key, lambda: GraphOperand.from_coo(int(m), index[0], index[1], value.detach(), device, n_cols=n_cols), sources=(index,))
        return _refresh_values(op, value, lambda: value.detach().to(device=op.device, dtype=torch.float32).reshape(-1)[_coo_order(index, op)])
    key = (_tensor_key(index), _tensor_key(value), int(m), n_cols, str(device))
    return _spmm_ops.get(key, lambda: GraphOperand.from_coo(int(m), index[0], index[1], value.detach(), device, n_cols=n_cols),
                         sources=(index, value.detach()))      # the detached alias shares storage and version counter: the address cannot be reused, no graph is kept


def _coo_order(index, op):
    """entry order of GraphOperand.from_coo: sorted by (row, col), duplicates in their given order (tests/test_device_build.py pins both builders to it)"""
    key = ("order", _tensor_key(index), op.n, op.n_cols, str(op.device))
    return _spmm_ops.get(key, lambda: torch.argsort(index[0].to(op.device).long() * max(op.n, op.n_cols) + index[1].to(op.device).long(), stable=True),
                         sources=(index,))


def _coo_values(index, value, op):
    """`value` in the operand's CSR order as a tensor of the autograd graph (None when it needs no gradient): entries sorted by (row, col),
    duplicates in their given order -- the order GraphOperand.from_coo packs (tests/test_device_build.py pins the two builders to it)."""
    if value is None or not value.requires_grad:
        return None
    return value.to(device=op.device, dtype=torch.float32).reshape(-1)[_coo_order(index, op)]


def _spmm3(op, x3, values):
    """one hop, differentiable in the matrix and (when given) in the operand's values"""
    if values is None and not x3.requires_grad:
        return F.csr_hop(op, x3)
    return F.SpmmFn.apply(x3, values, op)


def spmm(index, value, m, matrix):
    """out[r] += v_e * matrix[c] over axis 0 (reference: gcn.py:258-278)."""
    matrix = matrix if matrix.dim() > 1 else matrix.unsqueeze(-1)
    op = _coo_operand(index, value, m, matrix.device, matrix.shape[0])
    x3 = matrix.float().reshape(1, matrix.shape[0], -1).contiguous()
    return _spmm3(op, x3, _coo_values(index, value, op)).reshape((m,) + tuple(matrix.shape[1:]))


def spmm_batch_2(index, value, m, matrix):
    """Same product over axis 1 of (q, n[, f]) (reference: gcn.py:281-310; a 2-D input gains a channel axis)."""
    if matrix.dim() == 2:
        matrix = matrix.unsqueeze(-1)
    return spmm_batch_3(index, value, m, matrix)


def spmm_batch_3(index, value, m, matrix):
    """Same product over axis 1 of (q, n, h, f) (reference: gcn.py:313-345)."""
    op = _coo_operand(index, value, m, matrix.device, matrix.shape[1])
    sh = matrix.shape
    x3 = matrix.float().reshape(sh[0], sh[1], -1).contiguous()
    return _spmm3(op, x3, _coo_values(index, value, op)).reshape((sh[0], m) + tuple(sh[2:]))


# ------------------------------------------------------------------------------------ edge-list classes
class _EdgeBase(torch.nn.Module):
    def _operand(self, x, edge_index, edge_weight):
        n = x.size(1)
        if edge_weight is not None:
            assert edge_weight.reshape(-1).size(0) == edge_index.size(1)
        w = None if edge_weight is None else edge_weight.detach()        # shares storage and version counter; keeps no autograd graph alive
        if edge_weight is not None and edge_weight.requires_grad:
            # learnable weights: ONE operand per edge_index; the values lap_e = coef_e * w_e are refreshed in place when the weight has changed
            key = ("learnable", _tensor_key(edge_index), n, str(x.device))
            op = self._ops.get(key, lambda: GraphOperand.from_edge_index(edge_index, w, n, x.device), sources=(edge_index,))

            def vals():
                src, coef = self._links(edge_index, n, x.device)
                return coef * w.to(device=x.device, dtype=torch.float32).reshape(-1)[src]
            # (the first build's values are re-packed by the same formula as every later refresh, so that equal weights give bit-equal
            # operands whatever the history of the module: the builder rounds -d^-1/2 w d^-1/2 in another order)
            return _refresh_values(op, edge_weight, vals)
        key = self._operand_key(x, edge_index, edge_weight)
        return self._ops.get(key, lambda: GraphOperand.from_edge_index(edge_index, w, n, x.device), sources=(edge_index, w))

    @staticmethod
    def _operand_key(x, edge_index, edge_weight):
        """the cache key of a graph with fixed weights"""
        return (_tensor_key(edge_index), _tensor_key(edge_weight), x.size(1), str(x.device))

    def _links(self, edge_index, n, dev):
        """(source edge of every stored entry, its constant coefficient -deg^-1/2[row] deg^-1/2[col]) in the operand's CSR order, once per edge_index"""
        def links():
            row, col = edge_index[0].to(dev).long(), edge_index[1].to(dev).long()
            ids = (row != col).nonzero().flatten()
            r, c = row[ids], col[ids]
            order = torch.argsort(r * n + c, stable=True)            # the order GraphOperand.from_coo packs: (row, col), duplicates as given
            dis = torch.bincount(r, minlength=n).to(torch.float32).pow(-0.5)
            dis[torch.isinf(dis)] = 0
            return ids[order], (-(dis[r] * dis[c]))[order]
        return self._ops.get(("links", _tensor_key(edge_index), n, str(dev)), links, sources=(edge_index,))

    def _values(self, x, edge_index, edge_weight, op):
        """The operand's values in CSR order as a function of a LEARNABLE edge_weight (None otherwise): lap_e = -deg^-1/2[row] w_e deg^-1/2[col]
        with the unweighted source degree (gcn.py:408-413), i.e. a constant coefficient per kept edge times its weight -- differentiable index
        plumbing; the arithmetic of the gradient itself is F.chebyshev_values_grad."""
        if edge_weight is None or not edge_weight.requires_grad:
            return None
        n, dev = x.size(1), x.device
        src, coef = self._links(edge_index, n, dev)
        assert src.numel() == op.nnz
        return coef * edge_weight.to(device=dev, dtype=torch.float32).reshape(-1)[src]

    def reset_parameters(self):
        size = self.in_channels * self.weight.size(0)
        uniform(size, self.weight)
        uniform(size, self.bias)

    def __repr__(self):
        return '{}({}, {}, K={})'.format(self.__class__.__name__, self.in_channels, self.out_channels, self.weight.size(0))


class ChebConv(_EdgeBase):
    """reference: tgcn/nn/gcn.py:348-442.  forward(x (q,n[,f]), edge_index (2,E), edge_weight=None) -> (q,n,g)."""

    def __init__(self, in_channels, out_channels, K, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = Parameter(torch.Tensor(K, in_channels, out_channels))
        self._ops = _OperandCache()
        if bias:
            self.bias = Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def _layer_args(self, x, edge_index, edge_weight=None):
        dt = _compute_dtype(self, edge_weight)
        op = self._operand(x, edge_index, edge_weight)
        if x.dim() < 3:
            x = x.unsqueeze(-1)
        return (op, x.to(dt).contiguous(), self.weight, self.bias,
                F.BIAS_NONE if self.bias is None else F.BIAS_CHANNEL, F.MODE_CHEBYSHEV)

    def forward(self, x, edge_index, edge_weight=None):
        args = self._layer_args(x, edge_index, edge_weight)
        return F.cheb_layer(*args, values=self._values(x, edge_index, edge_weight, args[0]))


class ChebTimeConv(_EdgeBase):
    """reference: tgcn/nn/gcn.py:445-538.  forward(x (q,n,h[,f]), edge_index, edge_weight=None) -> (q,n,g)."""

    def __init__(self, in_channels, out_channels, K, H, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = Parameter(torch.Tensor(K, H, in_channels, out_channels))
        self._ops = _OperandCache()
        if bias:
            self.bias = Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def _layer_args(self, x, edge_index, edge_weight=None):
        dt = _compute_dtype(self, edge_weight)
        op = self._operand(x, edge_index, edge_weight)
        if x.dim() < 4:
            x = x.unsqueeze(-1)
        q, n, h, f = x.shape
        W = self.weight.reshape(self.weight.shape[0], h * f, self.out_channels)
        return (op, x.to(dt).reshape(q, n, h * f).contiguous(), W, self.bias,
                F.BIAS_NONE if self.bias is None else F.BIAS_CHANNEL, F.MODE_CHEBYSHEV)

    def forward(self, x, edge_index, edge_weight=None):
        args = self._layer_args(x, edge_index, edge_weight)
        return F.cheb_layer(*args, values=self._values(x, edge_index, edge_weight, args[0]))


    def forward_series(self, series, edge_index, edge_weight=None, as_series=False, stride=1, padding=0, dilation=1, time_chunk=None,
                       fused=False):
        """Additive API: TGCNCheb_H.forward_series' contract for this class -- series (S, n, T) or (S, n, T, f), f == in_channels, ->
        forward(xw, edge_index, edge_weight) on the windowed batch xw[s*(T-H+1) + w, i, h, c] = series[s, i, w + h, c], as
        (S*(T-H+1), n, g) or, as_series=True, (S, n, T-H+1, g); true recurrence, per-channel bias.  The operand is the one forward builds
        and caches.  A learnable edge_weight (requires_grad) raises TgcnError: its gradient needs the basis of every window, which
        this entry exists not to form -- call forward on materialised windows to train edge weights.
        stride, padding, dilation and time_chunk as in TGCNCheb_H.forward_series (time_chunk: the causal layer at step 1 in float32, walked
        Tc time rows at a time in both directions, out[:, :, He-1:] the windows inside the recording).  fused: as in
        TGCNCheb_H.forward_series (the true recurrence runs in the one-launch layer as it does in the hops)."""
        if edge_weight is not None and edge_weight.requires_grad:
            raise _lib.TgcnError("ChebTimeConv.forward_series: learnable edge weights (edge_weight.requires_grad) are not supported -- "
                                 "use forward on the windowed batch")
        return _forward_series(self, "ChebTimeConv.forward_series", series, edge_index, edge_weight, as_series, stride, padding, dilation,
                               time_chunk, fused)

    def forward_stream(self, chunk, edge_index, edge_weight=None, state=None, dilation=1, capturable=False, fused=False, stride=1):
        """Additive API, inference only: TGCNCheb_H.forward_stream's contract for this class -- chunk (S, n, Tc[, f]) -> (out (S, n, Tc, g),
        state), the rows [seen, seen + Tc) of forward_series(whole, edge_index, edge_weight, as_series=True, padding="causal",
        dilation=dilation); true recurrence, per-channel bias.  The state belongs to the operand of (edge_index, edge_weight): another graph
        needs its own.  A learnable edge_weight raises TgcnError, as in forward_series.  capturable and fused: as in
        TGCNCheb_H.forward_stream.  stride=s: as there -- the m = ceil((seen + Tc)/s) - ceil(seen/s) rows of forward_series(...,
        padding="causal", stride=s) whose window ends inside the chunk, the first at chunk row off = (-seen) mod s, as (S, n, m, g); m may
        be 0 (an empty tensor; a chain skips its later layers for that chunk, an empty chunk being refused); a capturable state takes
        Tc % s == 0 only."""
        if edge_weight is not None and edge_weight.requires_grad:
            raise _lib.TgcnError("ChebTimeConv.forward_stream: learnable edge weights (edge_weight.requires_grad) are not supported -- "
                                 "streaming is inference only; detach() the weight")
        return _forward_stream(self, "ChebTimeConv.forward_stream", chunk, edge_index, edge_weight, state, dilation, capturable, fused, stride)


# ------------------------------------------------------------------------------------ a streaming chain as one hipGraph
def _stream_states(states):
    """the SeriesStreamState objects of what a step returned: one state, or a list / tuple of them"""
    flat = [states] if isinstance(states, F.SeriesStreamState) else (list(states) if isinstance(states, (list, tuple)) else None)
    if not flat or not all(isinstance(st, F.SeriesStreamState) for st in flat):
        raise _lib.TgcnError("GraphedStream: step(chunk, states) returns (out, states) with states a SeriesStreamState or a list / tuple of them")
    return flat


class GraphedStream:
    """One step of a streaming chain captured into a hipGraph and replayed chunk after chunk (DESIGN.md 3.10 "Streaming state"): a step of a
    few time rows on a small graph is dozens of short launches, and the host time between them is a large part of it.
    step(chunk, states) -> (out, states) is the caller's chain; states is None on the first call and the chain passes capturable=True in it:
        def step(chunk, states):
            s1, s2 = states or (None, None)
            o1, s1 = l1.forward_stream(chunk, state=s1, capturable=True)
            o2, s2 = l2.forward_stream(torch.relu(o1), state=s2, dilation=2, capturable=True)
            return o2, (s1, s2)
    The constructor runs `warmup` >= 1 eager steps on a side stream (they build operands, states and lazily loaded code), resets every
    state and captures one step on a static copy of example_chunk, all under torch.no_grad().  gs(chunk) copies the chunk into the static
    input, replays the graph and returns the STATIC output: the next call overwrites it, so clone() what must be kept.  gs.reset() starts
    another recording; gs.states is what step returned.  One graph per chunk shape: a chunk of another shape, dtype or device than the
    example raises TgcnError, and so does a step whose states keep a ring position on the host (refused before the capture)."""

    def __init__(self, step, example_chunk, warmup=3):
        _lib.require_device(example_chunk)
        if not isinstance(warmup, int) or warmup < 1:
            raise _lib.TgcnError("GraphedStream: warmup is an integer >= 1 (the first eager step makes the states), got %r" % (warmup,))
        self._in = example_chunk.detach().clone()
        with torch.cuda.device(self._in.device), torch.no_grad():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                states = None
                for _ in range(warmup):
                    _, states = step(self._in, states)
            torch.cuda.current_stream().wait_stream(side)
            flat = _stream_states(states)
            for st in flat:
                if st.C and not st.capturable:
                    raise _lib.TgcnError("GraphedStream: the step returned a state that keeps its ring position on the host, which a "
                                         "replay cannot move -- pass capturable=True to forward_stream / cheb_time_stream")
            for st in flat:
                st.reset()
            self.states, self._flat = states, flat
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._out, _ = step(self._in, states)

    def __call__(self, chunk):
        if chunk.shape != self._in.shape or chunk.dtype != self._in.dtype or chunk.device != self._in.device:
            raise _lib.TgcnError("GraphedStream: captured for chunks %s %s on %s, got %s %s on %s -- one graph per chunk shape"
                                 % (tuple(self._in.shape), self._in.dtype, self._in.device, tuple(chunk.shape), chunk.dtype, chunk.device))
        self._in.copy_(chunk)
        self.graph.replay()
        return self._out

    def reset(self):
        """start another recording: every state's ring and position zeroed, stream-ordered"""
        for st in self._flat:
            st.reset()
        return self


# ------------------------------------------------------------------------------------ fused caller pattern
def cheb_relu_pool(layer, x, *graph_args, pool=4):
    """gcn_pool_4(F.relu(layer(x, ...)))  (pool=4)  /  gcn_pool(F.relu(layer(x, ...)))  (pool=2)  in one fused op:
    additive API for the pattern of examples/pytorch_based/pytorch_hcp_tgcn.py:134-141 and pytorch_mnist_gcn.py.
    `layer` is any of the five modules above; graph_args are ChebConv's (edge_index[, edge_weight])."""
    if _compute_dtype(layer) != torch.float32:
        raise _lib.TgcnError("cheb_relu_pool: bfloat16 parameters are not supported (run the layer, then gcn_pool / gcn_pool_4)")
    if len(graph_args) > 1 and graph_args[1] is not None and graph_args[1].requires_grad:
        # learnable edge weights: the gradient w.r.t. them belongs to the layer function; relu + pool as their own pass behind it
        return F.ReluPoolFn.apply(layer(x, *graph_args), pool)
    return F.cheb_relu_pool(*layer._layer_args(x, *graph_args), pool)


def _series_pool_layer(layer, graph_args, who):
    """(edge_index, edge_weight) of a cheb_series_relu_pool / cheb_stream_relu_pool call after the checks that need no operand: the layer's
    class, float32 parameters, fixed edge weights"""
    if not isinstance(layer, (TGCNCheb_H, ChebTimeConv)):
        raise _lib.TgcnError("%s: the layer is a TGCNCheb_H or a ChebTimeConv, got %s" % (who, type(layer).__name__))
    edge = isinstance(layer, ChebTimeConv)
    if len(graph_args) not in ((1, 2) if edge else (0,)):
        raise _lib.TgcnError("%s: %s takes %s after the series" % (who, type(layer).__name__, "edge_index[, edge_weight]" if edge else "no graph arguments"))
    edge_index, edge_weight = (tuple(graph_args) + (None, None))[:2]
    if _compute_dtype(layer, edge_weight) != torch.float32:
        raise _lib.TgcnError("%s: bfloat16 parameters are not supported (run the layer, then gcn_pool / gcn_pool_4)" % who)
    if edge_weight is not None and edge_weight.requires_grad:
        raise _lib.TgcnError("%s: learnable edge weights (edge_weight.requires_grad) are not supported -- use forward on the windowed batch, "
                             "then gcn_pool / gcn_pool_4" % who)
    return edge_index, edge_weight


def _series_pool_bias(layer):
    """(bias, bias_kind, mode) of the two time layers as the F.cheb_time_* functions take them"""
    if isinstance(layer, TGCNCheb_H):
        return (None if layer.bias is None else layer.bias.reshape(-1), F.BIAS_NONE if layer.bias is None else F.BIAS_VERTEX_CHANNEL, F.MODE_POWER)
    return layer.bias, F.BIAS_NONE if layer.bias is None else F.BIAS_CHANNEL, F.MODE_CHEBYSHEV


def _series_pool_call(layer, series, graph_args, who, pool, stride, padding, dilation, edges=None):
    """((op, series, weight, bias, bias_kind, mode), (stride, left, right, dilation)): how an F.cheb_time_windows_relu_* call begins, and the
    checked geometry for its keywords -- behind the layer's, the pool's and forward_series' refusals, the operand built last; edges is
    _series_pool_layer's answer where the wrapper has asked already"""
    edge_index, edge_weight = edges if edges is not None else _series_pool_layer(layer, graph_args, who)
    if series.dim() in (3, 4):
        F.check_pool(pool, series.shape[1], who)
    series, W, geom = _series_args(layer, series, stride, padding, dilation)
    return (_time_operand(layer, series, edge_index, edge_weight), series, W) + _series_pool_bias(layer), geom


def cheb_series_relu_pool(layer, series, *graph_args, pool=4, as_series=False, stride=1, padding=0, dilation=1):
    """gcn_pool_4(F.relu(layer.forward_series(series, ...)))  (pool=4; pool=2: gcn_pool)  in one fused op -- the caller pattern of
    cheb_relu_pool for the streaming time-window layers.  layer is a TGCNCheb_H or a ChebTimeConv, graph_args are ChebTimeConv's
    (edge_index[, edge_weight]); as_series, stride, padding, dilation as in forward_series.  -> z (S*nwin, n/pool, g) or, as_series=True,
    (S, n/pool, nwin, g): a series on the coarsened graph, which the next layer streams over.  relu and the max over `pool` consecutive
    vertices run in the projection's epilogue, so the layer's full output -- the large tensor of this path, g/f times the series -- is never
    allocated, in inference or in training; values and all gradients are bit-identical to the hand-written composition
    (F.cheb_time_windows_relu_pool).  A single channel runs the MFMA kernels in every geometry; an operand the layer keeps reordered runs
    the unfused calls.  Dropout between relu and pool, as in the reference's training script, is cheb_series_relu_dropout_pool: the same
    epilogue with a counter-based mask (cheb_relu_dropout_pool for the batch layers).
    TgcnError before an operand is built: bfloat16 parameters, pool outside {2, 4}, n % pool != 0, a learnable edge_weight, and every
    refusal forward_series makes for the same arguments.  No time_chunk: the causal layer in time chunks through this epilogue is
    cheb_series_relu_pool_chunked."""
    args, geom = _series_pool_call(layer, series, graph_args, "cheb_series_relu_pool", pool, stride, padding, dilation)
    return F.cheb_time_windows_relu_pool(*args, pool, as_series=as_series, stride=geom[0], padding=geom[1:3], dilation=geom[3])


def cheb_series_relu_dropout_pool(layer, series, *graph_args, p=0.5, pool=4, training=True, seed=None, as_series=False, stride=1, padding=0,
                                  dilation=1):
    """gcn_pool_4(F.dropout(F.relu(layer.forward_series(series, ...)), p, training))  (pool=4; pool=2: gcn_pool)  in one fused op -- the
    training pattern of examples/pytorch_based/pytorch_hcp_tgcn.py:134-137 on the streaming layers.  cheb_series_relu_pool's arguments,
    shapes and refusals; relu, the dropout and the pool run in the projection's epilogue, so the layer's full output, its relu, a mask and
    the dropped copy are never allocated, in the forward or the backward.
    The mask is not torch's: element e = ((s * nwin + w) * n + v) * N + c of the layer's output, in the caller's vertex labels, is kept iff
    word e & 3 of Philox4x32-10 on the counter e >> 2 under the key `seed` is >= p * 2^32, and a kept value is multiplied by 1 / (1 - p)
    (F.dropout_params, F.dropout_keep_mask).  It does not depend on as_series, the tile or the operand's ordering, the
    backward regenerates nothing (a positive pooled value was kept), and values and gradients are bit-identical to the composition with
    that mask.  seed=None draws a seed on the series' device (torch.randint: follows torch.manual_seed, legal inside a hipGraph capture,
    a new mask on every replay); an integer in [0, 2^62) or a one-element int64 tensor on the series' device fixes it.
    training=False or p == 0 is cheb_series_relu_pool, launch for launch.  An operand the layer keeps reordered runs the unpooled layer,
    relabels back, then one relu + dropout + pool pass -- the same mask.
    TgcnError before an operand is built: p outside [0, 1), a seed outside [0, 2^62), a seed tensor that is not one int64 element on the
    series' device, and everything cheb_series_relu_pool refuses.  No time_chunk: cheb_series_relu_pool_chunked walks the causal layer in
    time chunks through this epilogue, with the same mask."""
    who = "cheb_series_relu_dropout_pool"
    F.dropout_params(p, who)
    if isinstance(series, torch.Tensor):
        F.dropout_seed(seed, series.device, who, draw=False)
    if not training or p == 0:
        return cheb_series_relu_pool(layer, series, *graph_args, pool=pool, as_series=as_series, stride=stride, padding=padding, dilation=dilation)
    args, geom = _series_pool_call(layer, series, graph_args, who, pool, stride, padding, dilation)
    return F.cheb_time_windows_relu_dropout_pool(*args, pool, p, seed, as_series=as_series, stride=geom[0], padding=geom[1:3], dilation=geom[3])


def cheb_series_relu_pool_chunked(layer, series, *graph_args, time_chunk, pool=4, p=0.0, training=True, seed=None, as_series=False, dilation=1):
    """gcn_pool_4(F.dropout(F.relu(layer.forward_series(series, ..., padding="causal", dilation=dilation, time_chunk=time_chunk)), p, training))
    (pool=4; pool=2: gcn_pool)  in one op that uses BOTH memory features of the streaming layers: relu, the dropout and the pool run in the
    projection's epilogue, and the recording is walked time_chunk rows at a time through the streaming ring in both directions.  Neither the
    hop stack (K times the series), nor the layer's output (g/f times the series), nor that output's gradient is ever allocated: a training
    step holds the pooled tensors and chunk-sized buffers.  layer is a TGCNCheb_H or a ChebTimeConv, graph_args are ChebTimeConv's
    (edge_index[, edge_weight]).  -> z (S*T, n/pool, g) or, as_series=True, (S, n/pool, T, g).
    The geometry is always the causal layer at step 1 (what the ring implements): no stride and no padding keyword.  p == 0 or
    training=False is relu + pool without a mask.  Otherwise the mask is cheb_series_relu_dropout_pool's with nwin = T: element
    e = ((s*T + t)*n + v)*g + c of the layer's output in the caller's vertex labels, reproduced by F.dropout_keep_mask, the same for every
    time_chunk; seed as there.  z, d series and dW are bit-identical to the hand-written composition at the same time_chunk; d bias is
    summed chunk by chunk (agrees to rounding).  float32 only.
    An operand the layer keeps reordered runs forward_series(time_chunk=...), then one relu (+ dropout) + pool pass: the same values and
    mask, but the layer's output is allocated there -- the memory saving is absent.
    TgcnError before an operand is built: bfloat16 parameters, a learnable edge_weight, a bad pool, p, seed or time_chunk, n % pool != 0."""
    who = "cheb_series_relu_pool_chunked"
    F.dropout_params(p, who)
    if isinstance(series, torch.Tensor):
        F.dropout_seed(seed, series.device, who, draw=False)
    edges = _series_pool_layer(layer, graph_args, who)       # the layer's refusals come ahead of time_chunk's
    if time_chunk is None:
        raise _lib.TgcnError("%s: time_chunk is an integer >= 1, got None -- without chunks this is cheb_series_relu_pool / "
                             "cheb_series_relu_dropout_pool" % who)
    F.check_time_chunk(time_chunk, 1, "causal", False, who)
    args, geom = _series_pool_call(layer, series, graph_args, who, pool, 1, "causal", dilation, edges)
    return F.cheb_time_windows_relu_pool_chunked(*args, pool, time_chunk, p=p if training else 0.0, seed=seed, as_series=as_series,
                                                 dilation=geom[3])


def cheb_series_relu_pool_fused(layer, series, *graph_args, pool=4, p=0.0, training=True, seed=None, as_series=False, padding=0, dilation=1,
                                fused=True):
    """gcn_pool_4(F.dropout(F.relu(layer.forward_series(series, ..., fused=True)), p, training))  (pool=4; pool=2: gcn_pool)  in ONE launch on
    a graph that fits in LDS -- the opening block of the reference's HCP network (examples/pytorch_based/pytorch_hcp_tgcn.py:134-137) on the
    148-parcel graph: the hops, the window projection, the bias, relu, the dropout and the pool of a tile of windows per workgroup, the
    max taken in the accumulator registers (F.cheb_time_windows_relu_pool_fused, F.ChebSeriesSmallReluPoolFn).  layer is a TGCNCheb_H or a
    ChebTimeConv, graph_args are ChebTimeConv's (edge_index[, edge_weight]); as_series, padding, dilation as in forward_series.
    -> z (S*nwin, n/pool, g) or, as_series=True, (S, n/pool, nwin, g).  The layer's full output is never allocated; z and all gradients are
    bit-identical to relu (+ dropout) + pool as their own pass behind forward_series(..., fused=True).  p == 0 or training=False runs
    without a mask; otherwise the mask, p and seed are cheb_series_relu_dropout_pool's.  No stride and no time_chunk.
    fused=True raises TgcnError where the one-launch layer cannot run -- before an operand is built: bfloat16 parameters, a learnable
    edge_weight, a bad pool, p, seed, padding or dilation, n % pool != 0; before anything launches: an operand the layer keeps reordered
    and a shape the plan refuses (F.series_pool_fused_supported).  fused="auto" runs it where F.SERIES_POOL_FUSED_AUTO says it pays and is
    cheb_series_relu_pool / cheb_series_relu_dropout_pool elsewhere."""
    who = "cheb_series_relu_pool_fused"
    if fused is not True and not (isinstance(fused, str) and fused == "auto"):
        raise _lib.TgcnError("%s: fused is True or \"auto\", got %r" % (who, fused))
    F.dropout_params(p, who)
    if isinstance(series, torch.Tensor):
        F.dropout_seed(seed, series.device, who, draw=False)
    args, geom = _series_pool_call(layer, series, graph_args, who, pool, 1, padding, dilation)
    return F.cheb_time_windows_relu_pool_fused(*args, pool, p=p if training else 0.0, seed=seed, as_series=as_series, padding=geom[1:3],
                                               dilation=geom[3], fused=fused)


def cheb_relu_dropout_pool(layer, x, *graph_args, p=0.5, pool=4, training=True, seed=None):
    """gcn_pool_4(F.dropout(F.relu(layer(x, ...)), p, training))  (pool=4; pool=2: gcn_pool)  for the batch layers -- any of the five
    modules, graph_args as in cheb_relu_pool: the layer, then ONE relu + dropout + pool pass (tgcn_relu_dropout_pool_f32) in place of three
    torch passes and a stored mask.  The mask is cheb_series_relu_dropout_pool's on the element index e = (q * n + v) * N + c of the layer's
    (q, n, N) output; seed as there.  training=False or p == 0 is cheb_relu_pool.  Not fused into the layer's own kernels.
    TgcnError before anything launches: p outside [0, 1), a bad seed, bfloat16 parameters, pool outside {2, 4}, n % pool != 0."""
    who = "cheb_relu_dropout_pool"
    thr, scale = F.dropout_params(p, who)
    F.dropout_seed(seed, x.device, who, draw=False)
    if not training or p == 0:
        return cheb_relu_pool(layer, x, *graph_args, pool=pool)
    if _compute_dtype(layer) != torch.float32:
        raise _lib.TgcnError("%s: bfloat16 parameters are not supported (run the layer, then gcn_pool / gcn_pool_4)" % who)
    if x.dim() >= 2:
        F.check_pool(pool, x.shape[1], who)
    y = layer(x, *graph_args)
    return F.ReluDropoutPoolFn.apply(y, pool, y.shape[2], F.dropout_seed(seed, y.device, who), thr, scale)


def cheb_stream_relu_pool(layer, chunk, *graph_args, pool=4, state=None, dilation=1, capturable=False):
    """gcn_pool_4(F.relu(out)) of (out, state) = layer.forward_stream(chunk, ...) in one fused op (inference only): -> (z (S, n/pool, Tc, g),
    state).  The state is forward_stream's own F.SeriesStreamState and leaves the call as forward_stream leaves it: pooled and unpooled
    steps may alternate on it, and a chain with pooled layers is captured by GraphedStream unchanged (capturable=True).  layer,
    graph_args and pool as in cheb_series_relu_pool; state, dilation, capturable as in forward_stream.  TgcnError before an operand is
    built: bfloat16 parameters, pool outside {2, 4}, n % pool != 0, a learnable edge_weight, and every refusal forward_stream makes.
    No fused= and no stride=."""
    who = "cheb_stream_relu_pool"
    edge_index, edge_weight = _series_pool_layer(layer, graph_args, who)
    chunk, W = _stream_args(layer, chunk)
    F.check_pool(pool, chunk.shape[1], who)
    F.stream_precheck(chunk, W, layer.bias, state, dilation, who, capturable)      # refusals come before the operand is built
    _state_operand_check(layer, state, _time_operand(layer, chunk, edge_index, edge_weight, key=True))
    op = _time_operand(layer, chunk, edge_index, edge_weight)
    return F.cheb_time_stream_relu_pool(op, chunk, W, *_series_pool_bias(layer), pool, state=state, dilation=dilation, capturable=capturable)

