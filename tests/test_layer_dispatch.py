"""CPU test of which library entry points a layer call launches, in which order and with which scalar arguments.

`_lib.lib` is replaced by a recorder: launching entries return 0 and are logged with their int / float arguments, host queries
(`*_supported`, `*_workspace_bytes`, lane and geometry queries) answer from the case and are not logged.  Operands and compact plans are
stubs, tensors live on the CPU and hold whatever the fake launches left in them: only the launch sequence is checked, against EXPECTED."""
import contextlib
import ctypes

import pytest
import torch

from tgcn_amd import _lib
from tgcn_amd import functional as F

QUERIES = ("tgcn_hop_lanes_per_row", "tgcn_hop_vec_width", "tgcn_hop_groups_per_block", "tgcn_last_error", "tgcn_abi_version")
SCALARS = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_float, ctypes.c_double)


class _Recorder:
    def __init__(self, small):
        self.calls, self.small = [], small
        self.nulls = []           # per logged call: the positions of its void* arguments that were null

    def __getattr__(self, name):
        if name.endswith("_supported"):
            return lambda n, nnz, C, mode: self.small.get((name[len("tgcn_"):-len("_supported")], n, C), 0)
        if name.endswith("_workspace_bytes"):
            return lambda *a: 1024
        if name in QUERIES:
            return lambda *a: 4

        def launch(*args):
            types = _lib.SIGNATURES[name][1]
            nums = [("%g" % a if isinstance(a, float) else str(a)) for a, t in zip(args, types) if t in SCALARS]
            self.calls.append(" ".join([name[len("tgcn_"):].replace("_f32", "")] + nums))
            self.nulls.append(tuple(i for i, (a, t) in enumerate(zip(args, types)) if t is ctypes.c_void_p and not getattr(a, "value", a)))
            return 0
        return launch


class _Sched:
    struct = _lib.SchedStruct()


class _Plan:
    def __init__(self, n, n_c, n_empty):
        self.n, self.n_c, self.n_empty = n, n_c, n_empty
        self.first, self.rest = _Op(n_c, 4 * n_c, n_cols=n), _Op(n_c, 4 * n_c, n_cols=n_c + 1)
        self.rows = torch.zeros(n_c, dtype=torch.int32)
        self.empty = torch.zeros(n_empty, dtype=torch.int32)
        self.q_chunk_cache = {}

    def schedule_for(self, C_row, aligned16=True):
        return _Sched()

    def rows64(self):
        return self.rows.long()


class _Op:
    """n x n operand: `plans` maps a compact_plan kind to a plan (absent: None); `T` is the transposed operand (default: itself)"""

    def __init__(self, n, nnz, plans=(), dense=False, perm=False, T=None, n_cols=None):
        self.n, self.n_cols = n, n if n_cols is None else n_cols
        self.nnz = nnz
        self.struct = _lib.CsrStruct()
        self.plans = dict(plans)
        self.dense = torch.zeros(n, n) if dense else None
        self.perm = torch.arange(n - 1, -1, -1) if perm else None
        self.inv_perm = self.perm
        self.values_epoch = 0
        self.T = T

    def schedule_for(self, C_row, aligned16=True):
        return _Sched()

    def compact_plan(self, kind="rows"):
        return self.plans.get(kind)

    def transpose(self):
        return self if self.T is None else self.T


N_V = 64
T_WIN = 12      # series length of the "windows" cases


def _op(kind):
    if kind == "plain":
        return _Op(N_V, 256)
    if kind == "dense":
        return _Op(N_V, 256, dense=True)
    if kind == "reordered":
        return _Op(N_V, 256, perm=True)
    if kind == "compact":
        return _Op(N_V, 256, plans={"rows": _Plan(N_V, 40, 24), "closed": _Plan(N_V, 48, 16)})
    if kind == "compactT":        # no plan of its own, its transpose has one
        return _Op(N_V, 256, T=_Op(N_V, 256, plans={"rows": _Plan(N_V, 40, 24), "closed": _Plan(N_V, 48, 16)}))
    raise KeyError(kind)


@pytest.fixture
def recorder(monkeypatch):
    def make(small):
        rec = _Recorder(small)
        monkeypatch.setattr(_lib, "lib", lambda: rec)
        monkeypatch.setattr(_lib, "require_device", lambda *t: None)
        monkeypatch.setattr(_lib, "stream_ptr", lambda: ctypes.c_void_p(0))
        monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
        monkeypatch.setattr(torch.cuda, "mem_get_info", lambda d=None: (1 << 34, 1 << 35))
        return rec
    return make


def _small(spec):
    """("small", C) / ("small_pool", C) / ("basis_small", C) -> tile 16 for the operand of N_V vertices"""
    return {(name, N_V, C): 16 for name, C in spec}


# id: (entry, operand, q, C, N, K, mode, small, extra)
CASES = {
    "small-K5-power": ("layer", "plain", 2, 8, 8, 5, 0, [("cheb_forward_small", 8), ("cheb_basis_small", 8), ("cheb_forward_small", 8)], {}),
    "project-first-K3-cheb": ("layer", "plain", 2, 64, 16, 3, 1, [], {}),
    "compact-power-K5": ("layer", "compact", 2, 32, 32, 5, 0, [], {}),
    "compact-cheb-K3": ("layer", "compact", 2, 32, 32, 3, 1, [], {}),
    "compact-power-over-keep": ("layer", "compact", 2, 32, 32, 5, 0, [], {"keep_bytes": 0}),
    "compact-cheb-over-keep": ("layer", "compact", 2, 32, 32, 3, 1, [], {"keep_bytes": 0}),
    "compact-layout1-cheb": ("layer", "compact", 4, 8, 16, 3, 1, [], {}),
    "dx-compact-transpose-power": ("layer", "compactT", 2, 32, 32, 3, 0, [], {}),
    "dx-compact-transpose-cheb": ("layer", "compactT", 2, 32, 32, 4, 1, [], {}),
    "hops-layout0-K2-power": ("layer", "plain", 2, 32, 32, 2, 0, [], {}),
    "hops-layout0-K5-power-over-keep": ("layer", "plain", 2, 32, 32, 5, 0, [], {"keep_bytes": 0}),
    "hops-layout1-K5-cheb": ("layer", "plain", 4, 8, 16, 5, 1, [], {}),
    "hops-layout1-K5-cheb-over-keep": ("layer", "plain", 4, 8, 16, 5, 1, [], {"keep_bytes": 0}),
    "hops-K1-power": ("layer", "plain", 2, 32, 32, 1, 0, [], {}),
    "odd-width-padded": ("layer", "plain", 1, 15, 32, 3, 0, [], {}),
    "odd-width-small-not-padded": ("layer", "plain", 1, 15, 32, 3, 0, [("cheb_forward_small", 15)], {}),
    "reordered-vertex-bias": ("layer", "reordered", 2, 32, 32, 3, 1, [], {"bias_kind": 2}),
    "reordered-project-first-cheb": ("layer", "reordered", 2, 64, 16, 3, 1, [], {}),
    "reordered-project-first-power": ("layer", "reordered", 2, 64, 16, 3, 0, [], {}),
    "reordered-hops-cheb-over-keep": ("layer", "reordered", 2, 32, 32, 3, 1, [], {"keep_bytes": 0}),
    "reordered-hops-power-over-keep": ("layer", "reordered", 2, 32, 32, 3, 0, [], {"keep_bytes": 0}),
    "values-grad-kept-basis": ("layer", "plain", 2, 32, 32, 4, 1, [], {"values": True}),
    "values-grad-compact": ("layer", "compact", 2, 32, 32, 3, 1, [], {"values": True}),
    "values-grad-small": ("layer", "plain", 2, 8, 8, 3, 1, [("cheb_forward_small", 8), ("cheb_forward_small", 8)], {"values": True}),
    "pool-small": ("pool", "plain", 2, 8, 8, 3, 0, [("cheb_forward_small_pool", 8), ("cheb_forward_small", 8)], {}),
    "pool-dense-mfma": ("pool", "dense", 2, 8, 8, 3, 0, [("cheb_forward_small_pool", 8), ("cheb_forward_small", 8)], {}),
    "pool-fused-hops": ("pool", "plain", 2, 32, 32, 5, 0, [], {}),
    "pool-compact-unfused": ("pool", "compact", 2, 32, 32, 3, 1, [], {}),
    "pool-reordered": ("pool", "reordered", 2, 32, 32, 3, 0, [], {}),
    "windows-power-K3": ("windows", "plain", 2, 6, 8, 3, 0, [], {}),
    "windows-cheb-K4-reordered-relabel-once": ("windows", "reordered", 2, 6, 8, 4, 1, [], {}),
    "windows-K1": ("windows", "plain", 2, 6, 8, 1, 1, [], {}),
}


def _run(case, train, after_forward=lambda: None):
    entry, kind, q, C, N, K, mode, _, extra = case
    op = _op(kind)
    bias_kind = extra.get("bias_kind", F.BIAS_CHANNEL)
    torch.manual_seed(0)
    if entry == "windows":
        x = torch.randn(q, N_V, T_WIN)
        W = torch.randn(K, C, N)
        bias = torch.randn(N)
        leaves = [x, W, bias]
    else:
        x = torch.randn(q, N_V, C)
        W = torch.randn(K, C, N)
        bias = torch.randn(N_V, N) if bias_kind == F.BIAS_VERTEX_CHANNEL else torch.randn(N)
        leaves = [x, W, bias]
    values = torch.randn(op.nnz) if extra.get("values") else None
    if values is not None:
        leaves.append(values)
    for t in leaves:
        t.requires_grad_(train)
    with (contextlib.nullcontext() if train else torch.no_grad()):
        if entry == "layer":
            out = F.cheb_layer(op, x, W, bias, bias_kind, mode, values=values)
        elif entry == "pool":
            out = F.cheb_relu_pool(op, x, W, bias, bias_kind, mode, 4)
        else:
            out = F.cheb_time_windows(op, x, W, bias, bias_kind, mode)
    after_forward()
    if train:
        out.backward(torch.ones_like(out))


@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("name", list(CASES))
def test_layer_launches(name, train, recorder, monkeypatch):
    case = CASES[name]
    if "keep_bytes" in case[8]:
        monkeypatch.setattr(F, "KEEP_BASIS_BYTES", case[8]["keep_bytes"])
    rec = recorder(_small(case[7]))
    _run(case, train)
    assert rec.calls == EXPECTED["%s/%s" % (name, "training" if train else "inference")]


def _relabels(calls):
    """(rows, row width) of every pack_rows launch in `calls` -- its scalar arguments are (source stride, rows, row width)"""
    return sorted(tuple(int(a) for a in c.split()[2:]) for c in calls if c.startswith("pack_rows "))


@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("name", [k for k, c in CASES.items() if c[1] == "reordered"])
def test_reordered_operand_relabels_each_tensor_once(name, train, recorder, monkeypatch):
    """A reordered operand relabels each data tensor exactly once on the way in (x / the series, and a per-vertex bias) and the result
    once on the way out; the backward relabels the same tensors' gradients once each.  Any other pack_rows launch means that data
    already in the operand's labels was relabelled again (cheb_stack called without _operand_labels), i.e. hops on the wrong matrix."""
    entry, _, q, C, N, K, mode, small, extra = CASES[name]
    if "keep_bytes" in extra:
        monkeypatch.setattr(F, "KEEP_BASIS_BYTES", extra["keep_bytes"])
    rec = recorder(_small(small))
    fwd = []
    _run(CASES[name], train, after_forward=lambda: fwd.extend(rec.calls))
    if entry == "windows":
        once = [(q * N_V, T_WIN), (q * (T_WIN - C + 1) * N_V, N)]
    else:
        once = [(q * N_V, C), (q * N_V, N)]
    if extra.get("bias_kind") == F.BIAS_VERTEX_CHANNEL:
        once.append((N_V, N))
    assert _relabels(fwd) == sorted(once)
    assert _relabels(rec.calls) == sorted(once * (2 if train else 1))


# launches of the unchanged dispatch, one string per call: entry point (without tgcn_ / _f32) and its scalar arguments
EXPECTED = {
    'small-K5-power/inference': [
        'cheb_forward_small 0 5 2 8 8 1',
    ],
    'small-K5-power/training': [
        'cheb_forward_small 0 5 2 8 8 1',
        'fold_weight 5 64 0',
        'cheb_basis_small 0 5 2 8',
        'cheb_wgrad 128 8 8 5 8 1024',
        'fold_weight 5 64 1',
        'weight_layout 5 8 8 1',
        'cheb_forward_small 0 5 2 8 8 0',
    ],
    'project-first-K3-cheb/inference': [
        'weight_layout 3 64 16 0',
        'cheb_forward_pf 1 3 2 64 64 16 1 1024',
    ],
    'project-first-K3-cheb/training': [
        'weight_layout 3 64 16 0',
        'cheb_forward_pf 1 3 2 64 64 16 1 1024',
        'csr_hop2 2 64 1 0 0 1024',
        'csr_hop2 2 64 2 -1 0 1024',
        'cheb_wgrad 128 64 16 3 16 1024',
        'weight_layout 3 64 16 2',
        'cheb_project 128 16 192 1 0 64 1 0 192',
        'csr_hop2 2 64 2 -1 1 1024',
        'csr_hop2 2 64 1 -1 1 1024',
    ],
    'compact-power-K5/inference': [
        'fold_weight 5 1024 0',
        'cheb_compact_layer 0 5 2 64 32 32 1 24 1 1024',
    ],
    'compact-power-K5/training': [
        'fold_weight 5 1024 0',
        'cheb_compact_layer 0 5 2 64 32 32 1 24 1 1024',
        'fold_weight 5 1024 0',
        'pack_rows 32 40 32',
        'pack_rows 32 40 32',
        'cheb_wgrad 128 32 32 1 32 1024',
        'cheb_wgrad 82 32 32 4 32 1024',
        'fold_weight 5 1024 1',
        'weight_layout 5 32 32 1',
        'cheb_compact_layer 0 5 2 64 32 32 0 24 1 1024',
    ],
    'compact-cheb-K3/inference': [
        'fold_weight 3 1024 0',
        'cheb_compact_layer 1 3 2 64 32 32 1 16 1 1024',
    ],
    'compact-cheb-K3/training': [
        'fold_weight 3 1024 0',
        'cheb_compact_layer 1 3 2 64 32 32 1 16 1 1024',
        'pack_rows 32 48 32',
        'pack_rows 32 48 32',
        'cheb_wgrad 128 32 32 1 32 1024',
        'cheb_wgrad 98 32 32 3 32 1024',
        'weight_layout 3 32 32 1',
        'fold_weight 3 1024 0',
        'cheb_compact_layer 1 3 2 64 32 32 0 16 1 1024',
    ],
    'compact-power-over-keep/inference': [
        'fold_weight 5 1024 0',
        'cheb_compact_layer 0 5 2 64 32 32 1 24 1 1024',
    ],
    'compact-power-over-keep/training': [
        'fold_weight 5 1024 0',
        'cheb_compact_layer 0 5 2 64 32 32 1 24 1 1024',
        'fold_weight 5 1024 0',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 1 0 0 1024',
        'pack_rows 32 40 32',
        'pack_rows 32 40 32',
        'cheb_wgrad 128 32 32 1 32 1024',
        'cheb_wgrad 82 32 32 4 32 1024',
        'fold_weight 5 1024 1',
        'weight_layout 5 32 32 1',
        'cheb_compact_layer 0 5 2 64 32 32 0 24 1 1024',
    ],
    'compact-cheb-over-keep/inference': [
        'fold_weight 3 1024 0',
        'cheb_compact_layer 1 3 2 64 32 32 1 16 1 1024',
    ],
    'compact-cheb-over-keep/training': [
        'fold_weight 3 1024 0',
        'cheb_compact_layer 1 3 2 64 32 32 1 16 1 1024',
        'pack_rows 32 48 32',
        'pack_rows 32 48 32',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 2 -1 0 1024',
        'pack_rows 32 48 32',
        'pack_rows 32 48 32',
        'cheb_wgrad 128 32 32 1 32 1024',
        'cheb_wgrad 98 32 32 3 32 1024',
        'weight_layout 3 32 32 1',
        'fold_weight 3 1024 0',
        'cheb_compact_layer 1 3 2 64 32 32 0 16 1 1024',
    ],
    'compact-layout1-cheb/inference': [
        'cheb_forward 1 3 4 64 8 16 1 1 4 1024',
    ],
    'compact-layout1-cheb/training': [
        'relayout_qnc_to_nqc 4 64 8',
        'csr_hop2 1 32 1 0 0 1024',
        'csr_hop2 1 32 2 -1 0 1024',
        'cheb_project 256 8 16 3 1 64 4 0 16',
        'relayout_qnc_to_nqc 4 64 16',
        'cheb_wgrad 256 8 16 3 16 1024',
        'weight_layout 3 8 16 2',
        'cheb_project 256 16 24 1 0 64 1 0 24',
        'csr_hop2 4 8 2 -1 1 1024',
        'csr_hop2 4 8 1 -1 1 1024',
    ],
    'dx-compact-transpose-power/inference': [
        'fold_weight 3 1024 0',
        'cheb_forward 0 3 2 64 32 32 1 0 2 1024',
    ],
    'dx-compact-transpose-power/training': [
        'fold_weight 3 1024 0',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 1 0 0 1024',
        'cheb_project 128 32 32 3 1 64 1 0 32',
        'fold_weight 3 1024 0',
        'cheb_wgrad 128 32 32 3 32 1024',
        'fold_weight 3 1024 1',
        'weight_layout 3 32 32 1',
        'cheb_compact_layer 0 3 2 64 32 32 0 24 1 1024',
    ],
    'dx-compact-transpose-cheb/inference': [
        'cheb_forward 1 4 2 64 32 32 1 0 2 1024',
    ],
    'dx-compact-transpose-cheb/training': [
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 2 -1 0 1024',
        'csr_hop2 2 32 2 -1 0 1024',
        'cheb_project 128 32 32 4 1 64 1 0 32',
        'cheb_wgrad 128 32 32 4 32 1024',
        'weight_layout 4 32 32 1',
        'fold_weight 4 1024 0',
        'cheb_compact_layer 1 4 2 64 32 32 0 16 1 1024',
    ],
    'hops-layout0-K2-power/inference': [
        'cheb_forward 0 2 2 64 32 32 1 0 2 1024',
    ],
    'hops-layout0-K2-power/training': [
        'csr_hop2 2 32 1 0 0 1024',
        'cheb_project 128 32 32 2 1 64 1 0 32',
        'cheb_wgrad 128 32 32 2 32 1024',
        'weight_layout 2 32 32 2',
        'cheb_project 128 32 64 1 0 64 1 0 64',
        'csr_hop2 2 32 1 1 0 1024',
    ],
    'hops-layout0-K5-power-over-keep/inference': [
        'fold_weight 5 1024 0',
        'cheb_forward 0 5 2 64 32 32 1 0 2 1024',
    ],
    'hops-layout0-K5-power-over-keep/training': [
        'fold_weight 5 1024 0',
        'cheb_forward 0 5 2 64 32 32 1 0 2 1024',
        'fold_weight 5 1024 0',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 1 0 0 1024',
        'cheb_wgrad 128 32 32 5 32 1024',
        'fold_weight 5 1024 1',
        'weight_layout 5 32 32 2',
        'cheb_project 128 32 160 1 0 64 1 0 160',
        'csr_hop2 2 32 1 1 0 1024',
        'csr_hop2 2 32 1 1 0 1024',
        'csr_hop2 2 32 1 1 0 1024',
        'csr_hop2 2 32 1 1 0 1024',
    ],
    'hops-layout1-K5-cheb/inference': [
        'cheb_forward 1 5 4 64 8 16 1 1 4 1024',
    ],
    'hops-layout1-K5-cheb/training': [
        'relayout_qnc_to_nqc 4 64 8',
        'csr_hop2 1 32 1 0 0 1024',
        'csr_hop2 1 32 2 -1 0 1024',
        'csr_hop2 1 32 2 -1 0 1024',
        'csr_hop2 1 32 2 -1 0 1024',
        'cheb_project 256 8 16 5 1 64 4 0 16',
        'relayout_qnc_to_nqc 4 64 16',
        'cheb_wgrad 256 8 16 5 16 1024',
        'weight_layout 5 8 16 2',
        'cheb_project 256 16 40 1 0 64 1 0 40',
        'csr_hop2 4 8 2 -1 1 1024',
        'csr_hop2 4 8 2 -1 1 1024',
        'csr_hop2 4 8 2 -1 1 1024',
        'csr_hop2 4 8 1 -1 1 1024',
    ],
    'hops-layout1-K5-cheb-over-keep/inference': [
        'cheb_forward 1 5 4 64 8 16 1 1 4 1024',
    ],
    'hops-layout1-K5-cheb-over-keep/training': [
        'cheb_forward 1 5 4 64 8 16 1 1 4 1024',
        'csr_hop2 4 8 1 0 0 1024',
        'csr_hop2 4 8 2 -1 0 1024',
        'csr_hop2 4 8 2 -1 0 1024',
        'csr_hop2 4 8 2 -1 0 1024',
        'cheb_wgrad 256 8 16 5 16 1024',
        'weight_layout 5 8 16 2',
        'cheb_project 256 16 40 1 0 64 1 0 40',
        'csr_hop2 4 8 2 -1 1 1024',
        'csr_hop2 4 8 2 -1 1 1024',
        'csr_hop2 4 8 2 -1 1 1024',
        'csr_hop2 4 8 1 -1 1 1024',
    ],
    'hops-K1-power/inference': [
        'cheb_forward 0 1 2 64 32 32 1 0 2 1024',
    ],
    'hops-K1-power/training': [
        'cheb_forward 0 1 2 64 32 32 1 0 2 1024',
        'cheb_wgrad 128 32 32 1 32 1024',
        'weight_layout 1 32 32 2',
        'cheb_project 128 32 32 1 0 64 1 0 32',
    ],
    'odd-width-padded/inference': [
        'fold_weight 3 512 0',
        'cheb_forward 0 3 1 64 16 32 1 0 1 1024',
    ],
    'odd-width-padded/training': [
        'fold_weight 3 512 0',
        'csr_hop2 1 16 1 0 0 1024',
        'csr_hop2 1 16 1 0 0 1024',
        'cheb_project 64 16 32 3 1 64 1 0 32',
        'fold_weight 3 512 0',
        'cheb_wgrad 64 16 32 3 32 1024',
        'fold_weight 3 512 1',
        'weight_layout 3 16 32 2',
        'cheb_project 64 32 48 1 0 64 1 0 48',
        'csr_hop2 1 16 1 1 0 1024',
        'csr_hop2 1 16 1 1 0 1024',
    ],
    'odd-width-small-not-padded/inference': [
        'cheb_forward_small 0 3 1 15 32 1',
    ],
    'odd-width-small-not-padded/training': [
        'cheb_forward_small 0 3 1 15 32 1',
        'fold_weight 3 480 0',
        'csr_hop2 1 15 1 0 0 1024',
        'csr_hop2 1 15 1 0 0 1024',
        'cheb_wgrad 64 15 32 3 32 1024',
        'fold_weight 3 480 1',
        'weight_layout 3 15 32 2',
        'cheb_project 64 32 45 1 0 64 1 0 45',
        'csr_hop2 1 15 1 1 0 1024',
        'csr_hop2 1 15 1 1 0 1024',
    ],
    'reordered-vertex-bias/inference': [
        'pack_rows 32 128 32',
        'pack_rows 32 64 32',
        'cheb_forward 1 3 2 64 32 32 2 0 2 1024',
        'pack_rows 32 128 32',
    ],
    'reordered-vertex-bias/training': [
        'pack_rows 32 128 32',
        'pack_rows 32 64 32',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 2 -1 0 1024',
        'cheb_project 128 32 32 3 2 64 1 0 32',
        'pack_rows 32 128 32',
        'pack_rows 32 128 32',
        'cheb_wgrad 128 32 32 3 32 1024',
        'weight_layout 3 32 32 2',
        'cheb_project 128 32 96 1 0 64 1 0 96',
        'csr_hop2 2 32 2 -1 1 1024',
        'csr_hop2 2 32 1 -1 1 1024',
        'pack_rows 32 64 32',
        'pack_rows 32 128 32',
    ],
    'reordered-project-first-cheb/inference': [
        'pack_rows 64 128 64',
        'weight_layout 3 64 16 0',
        'cheb_forward_pf 1 3 2 64 64 16 1 1024',
        'pack_rows 16 128 16',
    ],
    'reordered-project-first-cheb/training': [
        'pack_rows 64 128 64',
        'weight_layout 3 64 16 0',
        'cheb_forward_pf 1 3 2 64 64 16 1 1024',
        'pack_rows 16 128 16',
        'pack_rows 16 128 16',
        'csr_hop2 2 64 1 0 0 1024',
        'csr_hop2 2 64 2 -1 0 1024',
        'cheb_wgrad 128 64 16 3 16 1024',
        'weight_layout 3 64 16 2',
        'cheb_project 128 16 192 1 0 64 1 0 192',
        'csr_hop2 2 64 2 -1 1 1024',
        'csr_hop2 2 64 1 -1 1 1024',
        'pack_rows 64 128 64',
    ],
    'reordered-project-first-power/inference': [
        'pack_rows 64 128 64',
        'fold_weight 3 1024 0',
        'weight_layout 3 64 16 0',
        'cheb_forward_pf 0 3 2 64 64 16 1 1024',
        'pack_rows 16 128 16',
    ],
    'reordered-project-first-power/training': [
        'pack_rows 64 128 64',
        'fold_weight 3 1024 0',
        'weight_layout 3 64 16 0',
        'cheb_forward_pf 0 3 2 64 64 16 1 1024',
        'pack_rows 16 128 16',
        'pack_rows 16 128 16',
        'fold_weight 3 1024 0',
        'csr_hop2 2 64 1 0 0 1024',
        'csr_hop2 2 64 1 0 0 1024',
        'cheb_wgrad 128 64 16 3 16 1024',
        'fold_weight 3 1024 1',
        'weight_layout 3 64 16 2',
        'cheb_project 128 16 192 1 0 64 1 0 192',
        'csr_hop2 2 64 1 1 0 1024',
        'csr_hop2 2 64 1 1 0 1024',
        'pack_rows 64 128 64',
    ],
    'reordered-hops-cheb-over-keep/inference': [
        'pack_rows 32 128 32',
        'cheb_forward 1 3 2 64 32 32 1 0 2 1024',
        'pack_rows 32 128 32',
    ],
    'reordered-hops-cheb-over-keep/training': [
        'pack_rows 32 128 32',
        'cheb_forward 1 3 2 64 32 32 1 0 2 1024',
        'pack_rows 32 128 32',
        'pack_rows 32 128 32',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 2 -1 0 1024',
        'cheb_wgrad 128 32 32 3 32 1024',
        'weight_layout 3 32 32 2',
        'cheb_project 128 32 96 1 0 64 1 0 96',
        'csr_hop2 2 32 2 -1 1 1024',
        'csr_hop2 2 32 1 -1 1 1024',
        'pack_rows 32 128 32',
    ],
    'reordered-hops-power-over-keep/inference': [
        'pack_rows 32 128 32',
        'fold_weight 3 1024 0',
        'cheb_forward 0 3 2 64 32 32 1 0 2 1024',
        'pack_rows 32 128 32',
    ],
    'reordered-hops-power-over-keep/training': [
        'pack_rows 32 128 32',
        'fold_weight 3 1024 0',
        'cheb_forward 0 3 2 64 32 32 1 0 2 1024',
        'pack_rows 32 128 32',
        'pack_rows 32 128 32',
        'fold_weight 3 1024 0',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 1 0 0 1024',
        'cheb_wgrad 128 32 32 3 32 1024',
        'fold_weight 3 1024 1',
        'weight_layout 3 32 32 2',
        'cheb_project 128 32 96 1 0 64 1 0 96',
        'csr_hop2 2 32 1 1 0 1024',
        'csr_hop2 2 32 1 1 0 1024',
        'pack_rows 32 128 32',
    ],
    'values-grad-kept-basis/inference': [
        'cheb_forward 1 4 2 64 32 32 1 0 2 1024',
    ],
    'values-grad-kept-basis/training': [
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 2 -1 0 1024',
        'csr_hop2 2 32 2 -1 0 1024',
        'cheb_project 128 32 32 4 1 64 1 0 32',
        'cheb_wgrad 128 32 32 4 32 1024',
        'weight_layout 4 32 32 2',
        'cheb_project 128 32 128 1 0 64 1 0 128',
        'csr_hop2 2 32 2 -1 1 1024',
        'csr_hop2 2 32 2 -1 1 1024',
        'csr_hop2 2 32 1 -1 1 1024',
        'weight_layout 4 32 32 2',
        'cheb_project 128 32 128 1 0 64 1 0 128',
        'csr_sddmm 64 2 32 2 0',
        'csr_hop2 2 32 2 -1 1 1024',
        'csr_sddmm 64 2 32 2 1',
        'csr_hop2 2 32 2 -1 1 1024',
        'csr_sddmm 64 2 32 1 1',
    ],
    'values-grad-compact/inference': [
        'fold_weight 3 1024 0',
        'cheb_compact_layer 1 3 2 64 32 32 1 16 1 1024',
    ],
    'values-grad-compact/training': [
        'fold_weight 3 1024 0',
        'cheb_compact_layer 1 3 2 64 32 32 1 16 1 1024',
        'pack_rows 32 48 32',
        'pack_rows 32 48 32',
        'cheb_wgrad 128 32 32 1 32 1024',
        'cheb_wgrad 98 32 32 3 32 1024',
        'weight_layout 3 32 32 1',
        'fold_weight 3 1024 0',
        'cheb_compact_layer 1 3 2 64 32 32 0 16 1 1024',
        'csr_hop2 2 32 1 0 0 1024',
        'weight_layout 3 32 32 2',
        'cheb_project 128 32 96 1 0 64 1 0 96',
        'csr_sddmm 64 2 32 2 0',
        'csr_hop2 2 32 2 -1 1 1024',
        'csr_sddmm 64 2 32 1 1',
    ],
    'values-grad-small/inference': [
        'cheb_forward_small 1 3 2 8 8 1',
    ],
    'values-grad-small/training': [
        'cheb_forward_small 1 3 2 8 8 1',
        'csr_hop2 2 8 1 0 0 1024',
        'csr_hop2 2 8 2 -1 0 1024',
        'cheb_wgrad 128 8 8 3 8 1024',
        'weight_layout 3 8 8 1',
        'cheb_forward_small 1 3 2 8 8 0',
        'csr_hop2 2 8 1 0 0 1024',
        'weight_layout 3 8 8 2',
        'cheb_project 128 8 24 1 0 64 1 0 24',
        'csr_sddmm 64 2 8 2 0',
        'csr_hop2 2 8 2 -1 1 1024',
        'csr_sddmm 64 2 8 1 1',
    ],
    'pool-small/inference': [
        'cheb_forward_small_pool 0 3 2 8 8 1 1 4',
    ],
    'pool-small/training': [
        'cheb_forward_small_pool 0 3 2 8 8 1 1 4',
        'relu_pool_bwd 2 64 8 4',
        'fold_weight 3 64 0',
        'csr_hop2 2 8 1 0 0 1024',
        'csr_hop2 2 8 1 0 0 1024',
        'cheb_wgrad 128 8 8 3 8 1024',
        'fold_weight 3 64 1',
        'weight_layout 3 8 8 1',
        'cheb_forward_small 0 3 2 8 8 0',
    ],
    'pool-dense-mfma/inference': [
        'cheb_forward_small 0 3 2 8 8 1',
        'relu_pool 2 64 8 4',
    ],
    'pool-dense-mfma/training': [
        'cheb_forward_small 0 3 2 8 8 1',
        'relu_pool 2 64 8 4',
        'relu_pool_bwd 2 64 8 4',
        'fold_weight 3 64 0',
        'csr_hop2 2 8 1 0 0 1024',
        'csr_hop2 2 8 1 0 0 1024',
        'cheb_wgrad 128 8 8 3 8 1024',
        'fold_weight 3 64 1',
        'weight_layout 3 8 8 1',
        'cheb_forward_small 0 3 2 8 8 0',
    ],
    'pool-fused-hops/inference': [
        'fold_weight 5 1024 0',
        'cheb_forward_pool 0 5 2 64 32 32 1 4 0 2 1024',
    ],
    'pool-fused-hops/training': [
        'fold_weight 5 1024 0',
        'cheb_forward_pool 0 5 2 64 32 32 1 4 0 2 1024',
        'relu_pool_bwd 2 64 32 4',
        'fold_weight 5 1024 0',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 1 0 0 1024',
        'cheb_wgrad 128 32 32 5 32 1024',
        'fold_weight 5 1024 1',
        'weight_layout 5 32 32 2',
        'cheb_project 128 32 160 1 0 64 1 0 160',
        'csr_hop2 2 32 1 1 0 1024',
        'csr_hop2 2 32 1 1 0 1024',
        'csr_hop2 2 32 1 1 0 1024',
        'csr_hop2 2 32 1 1 0 1024',
    ],
    'pool-compact-unfused/inference': [
        'fold_weight 3 1024 0',
        'cheb_compact_layer 1 3 2 64 32 32 1 16 1 1024',
        'relu_pool 2 64 32 4',
    ],
    'pool-compact-unfused/training': [
        'fold_weight 3 1024 0',
        'cheb_compact_layer 1 3 2 64 32 32 1 16 1 1024',
        'relu_pool 2 64 32 4',
        'relu_pool_bwd 2 64 32 4',
        'pack_rows 32 48 32',
        'pack_rows 32 48 32',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 2 -1 0 1024',
        'pack_rows 32 48 32',
        'pack_rows 32 48 32',
        'cheb_wgrad 128 32 32 1 32 1024',
        'cheb_wgrad 98 32 32 3 32 1024',
        'weight_layout 3 32 32 1',
        'fold_weight 3 1024 0',
        'cheb_compact_layer 1 3 2 64 32 32 0 16 1 1024',
    ],
    'pool-reordered/inference': [
        'pack_rows 32 128 32',
        'fold_weight 3 1024 0',
        'cheb_forward 0 3 2 64 32 32 1 0 2 1024',
        'pack_rows 32 128 32',
        'relu_pool 2 64 32 4',
    ],
    'pool-reordered/training': [
        'pack_rows 32 128 32',
        'fold_weight 3 1024 0',
        'csr_hop2 2 32 1 0 0 1024',
        'csr_hop2 2 32 1 0 0 1024',
        'cheb_project 128 32 32 3 1 64 1 0 32',
        'pack_rows 32 128 32',
        'relu_pool 2 64 32 4',
        'relu_pool_bwd 2 64 32 4',
        'pack_rows 32 128 32',
        'fold_weight 3 1024 0',
        'cheb_wgrad 128 32 32 3 32 1024',
        'fold_weight 3 1024 1',
        'weight_layout 3 32 32 2',
        'cheb_project 128 32 96 1 0 64 1 0 96',
        'csr_hop2 2 32 1 1 0 1024',
        'csr_hop2 2 32 1 1 0 1024',
        'pack_rows 32 128 32',
    ],
    'windows-power-K3/inference': [
        'fold_weight 3 48 0',
        'csr_hop2 2 12 1 0 0 1024',
        'csr_hop2 2 12 1 0 0 1024',
        'cheb_project_windows 64 12 6 8 3 1',
        'cheb_project_windows 64 12 6 8 3 1',
    ],
    'windows-power-K3/training': [
        'fold_weight 3 48 0',
        'csr_hop2 2 12 1 0 0 1024',
        'csr_hop2 2 12 1 0 0 1024',
        'cheb_project_windows 64 12 6 8 3 1',
        'cheb_project_windows 64 12 6 8 3 1',
        'cheb_windows_backward 2 64 12 6 8 3 1024',
        'csr_hop2 2 12 1 1 0 1024',
        'csr_hop2 2 12 1 1 0 1024',
        'fold_weight 3 48 1',
    ],
    'windows-cheb-K4-reordered-relabel-once/inference': [
        'pack_rows 12 128 12',
        'csr_hop2 2 12 1 0 0 1024',
        'csr_hop2 2 12 2 -1 0 1024',
        'csr_hop2 2 12 2 -1 0 1024',
        'cheb_project_windows 64 12 6 8 4 1',
        'cheb_project_windows 64 12 6 8 4 1',
        'pack_rows 8 896 8',
    ],
    'windows-cheb-K4-reordered-relabel-once/training': [
        'pack_rows 12 128 12',
        'csr_hop2 2 12 1 0 0 1024',
        'csr_hop2 2 12 2 -1 0 1024',
        'csr_hop2 2 12 2 -1 0 1024',
        'cheb_project_windows 64 12 6 8 4 1',
        'cheb_project_windows 64 12 6 8 4 1',
        'pack_rows 8 896 8',
        'pack_rows 8 896 8',
        'cheb_windows_backward 2 64 12 6 8 4 1024',
        'csr_hop2 2 12 2 -1 1 1024',
        'csr_hop2 2 12 2 -1 1 1024',
        'csr_hop2 2 12 1 -1 1 1024',
        'pack_rows 12 128 12',
    ],
    'windows-K1/inference': [
        'cheb_project_windows 64 12 6 8 1 1',
        'cheb_project_windows 64 12 6 8 1 1',
    ],
    'windows-K1/training': [
        'cheb_project_windows 64 12 6 8 1 1',
        'cheb_project_windows 64 12 6 8 1 1',
        'cheb_windows_backward 2 64 12 6 8 1 1024',
    ],
}
