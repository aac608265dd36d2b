"""Hub rows as wave segments (graph.HUB_MIN / HUB_SEG, docs/EXPERIMENTS.md A.9): rows of more than HUB_MIN entries are cut into segments of
HUB_SEG consecutive entries that one WAVE handles (its four lane groups fold inside the wave: one partial row per HUB_SEG entries), stored
behind the whole-row wave segments among the leading nwseg entries of the seg_* arrays.  The rule is gated on the size of the plain schedule's
partial rows, so the tests force it through the switches at HUB_MIN = 256, HUB_SEG = 128 on a 3,000-vertex graph with planted rows:

    128 entries   whole-row wave segment             384   exact multiple of HUB_SEG
    129, 256      lane-group segments (no hub rows)  1000
    257, 385      last hub segment of ONE entry      9000  71 slots: the workgroup path of the fix-up (nhuge)
                  (three of four lane groups empty)

Two whole rows + 89 hub segments = 91 wave-handled segments: the first workgroup of four waves holds whole-row (written directly) and slotted
segments side by side, the last one is partly filled (three waves).

Tolerance of the GPU tests: BASELINE.md section 4, max|a - b| / max|b| <= 1e-5 against fp64 (scipy); bf16 rows: one rounding of the stored
row, 2^-8 relative to the largest output, on top of fp32 sums of bf16-exact inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

N = 3000
PLANTED = ((5, 128), (2100, 128), (17, 129), (300, 256), (1234, 257), (2, 384), (2998, 385), (640, 1000), (77, 9000))
HUB_MIN, HUB_SEG = 256, 128


def _coo(seed=0):
    """20,000 random entries in the rows that are not planted (so the planted degrees are exact) + the planted rows"""
    rng = np.random.default_rng(seed)
    free = np.setdiff1d(np.arange(N), [r for r, _ in PLANTED])
    row, col = free[rng.integers(0, free.size, 20000)], rng.integers(0, N, 20000)
    for r, d in PLANTED:
        row = np.concatenate([row, np.full(d, r)])
        col = np.concatenate([col, rng.integers(0, N, d)])
    val = (rng.standard_normal(row.shape[0]) / 4).astype(np.float32)
    return row, col, val


def _force(monkeypatch, graph):
    monkeypatch.setattr(graph, "HUB_MIN", HUB_MIN)
    monkeypatch.setattr(graph, "HUB_SEG", HUB_SEG)
    monkeypatch.setattr(graph, "HUB_GATE_BYTES", 0)


def _operand(device="cpu"):
    from tgcn_amd.graph import GraphOperand
    row, col, val = _coo()
    return GraphOperand.from_coo(N, torch.as_tensor(row).to(device), torch.as_tensor(col).to(device), torch.as_tensor(val).to(device))


SCHED_COUNTS = ("lanes_per_row", "row_thresh", "nblk", "nseg", "nlong", "nhuge", "npartial", "seg_mode", "row_mix", "nwseg")


def _sched_arrays(s):
    return (("blk_row", s.nblk + 1), ("seg_row", s.nseg), ("seg_e0", s.nseg), ("seg_e1", s.nseg), ("seg_slot", s.nseg), ("long_row", s.nlong),
            ("long_slot", s.nlong + 1 if s.nlong else 0))


def _assert_equal_schedules(a, b):
    for f in SCHED_COUNTS:
        assert getattr(a, f) == getattr(b, f), f
    for f, cnt in _sched_arrays(b):
        assert torch.equal(getattr(a, f)[:cnt].cpu(), getattr(b, f)[:cnt].cpu()), f


# ------------------------------------------------------------------------------------------------ CPU: the torch builder

def test_hub_schedule_structure(monkeypatch):
    from tgcn_amd import graph
    _force(monkeypatch, graph)
    op = _operand()
    s = op.schedule(16)
    rowptr = op.rowptr.numpy().astype(np.int64)
    deg = np.diff(rowptr)
    for r, d in PLANTED:
        assert deg[r] == d
    seg_row, e0, e1, slot = (t.numpy()[: s.nseg] for t in (s.seg_row, s.seg_e0, s.seg_e1, s.seg_slot))
    n_whole = int(((deg > 32) & (deg <= 128)).sum())
    hub_rows = np.nonzero(deg > HUB_MIN)[0]
    n_hub = int(((deg[hub_rows] + HUB_SEG - 1) // HUB_SEG).sum())
    assert n_whole == 2 and n_hub == 3 + 3 + 4 + 8 + 71
    assert s.nwseg == n_whole + n_hub and s.nwseg % 4 != 0
    # every entry once: short rows through the row blocks, the others through exactly one segment
    covered = np.zeros(op.nnz, np.int32)
    for r in np.nonzero(deg <= s.row_thresh)[0]:
        covered[rowptr[r]:rowptr[r + 1]] += 1
    for i in range(s.nseg):
        r, ln = seg_row[i], e1[i] - e0[i]
        assert rowptr[r] <= e0[i] < e1[i] <= rowptr[r + 1]
        covered[e0[i]:e1[i]] += 1
        if i < n_whole:                      # whole rows, written directly
            assert e0[i] == rowptr[r] and e1[i] == rowptr[r + 1] and 32 < ln <= 128 and slot[i] < 0
        elif i < s.nwseg:                    # hub wave segments: HUB_SEG entries from the row's start on, the last one shorter
            assert deg[r] > HUB_MIN and ln <= HUB_SEG and slot[i] >= 0 and (e0[i] - rowptr[r]) % HUB_SEG == 0
            assert ln == HUB_SEG or e1[i] == rowptr[r + 1]
        else:                                # lane-group segments of the rows between: exactly as without the rule
            assert 128 < deg[r] <= HUB_MIN and ln <= 32 and slot[i] >= 0 and (e0[i] - rowptr[r]) % 32 == 0
            assert ln == 32 or e1[i] == rowptr[r + 1]
    assert np.all(covered == 1)
    assert int((e1[n_whole: s.nwseg] - e0[n_whole: s.nwseg] == 1).sum()) == 2            # the last segments of the 257- and the 385-entry row
    # slots: consecutive per row in entry order, every slot used once, rows by decreasing slot count, nhuge = rows above 64 slots
    long_row, long_slot = s.long_row.numpy(), s.long_slot.numpy()
    assert long_slot[0] == 0 and long_slot[s.nlong] == s.npartial
    assert np.array_equal(np.sort(slot[slot >= 0]), np.arange(s.npartial))
    assert sorted(long_row[: s.nlong]) == sorted(np.nonzero(deg > 128)[0])
    for i in range(s.nlong):
        mine = np.nonzero(seg_row == long_row[i])[0]
        mine = mine[np.argsort(e0[mine])]
        assert np.array_equal(slot[mine], np.arange(long_slot[i], long_slot[i + 1]))
        d = deg[long_row[i]]
        assert long_slot[i + 1] - long_slot[i] == (-(-d // HUB_SEG) if d > HUB_MIN else -(-d // 32))
    nslots = np.diff(long_slot[: s.nlong + 1])
    assert np.all(np.diff(nslots) <= 0)
    assert s.nhuge == 1 and nslots[0] == 71 and np.all(nslots[s.nhuge:] <= 64)
    assert s.npartial == n_hub + 5 + 8
    # three runs, each in order of first column
    first_col = op.edges[:, 0].numpy()[e0]
    for a, b in ((0, n_whole), (n_whole, s.nwseg), (s.nwseg, s.nseg)):
        assert np.all(np.diff(first_col[a:b]) >= 0)


@pytest.mark.parametrize("lpr", [1, 4, 16, 64])
def test_default_gate_leaves_small_schedules_alone(lpr, monkeypatch):
    """The gate at its default: a graph whose partial rows fit the Infinity Cache gets the arrays of the rule switched off -- also with hub rows
    above the default HUB_MIN; and the forced rule touches 16-lane schedules only."""
    from tgcn_amd import graph
    op = _operand()
    assert int(np.diff(op.rowptr.numpy()).max()) > graph.HUB_MIN
    default = graph.Schedule(op.rowptr, op.n, lpr, edges=op.edges)
    monkeypatch.setattr(graph, "HUB_MIN", 0)
    off = graph.Schedule(op.rowptr, op.n, lpr, edges=op.edges)
    _assert_equal_schedules(default, off)
    _force(monkeypatch, graph)
    forced = graph.Schedule(op.rowptr, op.n, lpr, edges=op.edges)
    if lpr == 16:
        assert forced.npartial < off.npartial and forced.nwseg > off.nwseg
    else:
        _assert_equal_schedules(forced, off)


def test_gate_counts_the_plain_partial_rows(monkeypatch):
    """npartial_plain * lanes * 16 B against the gate: the rule switches on exactly above it"""
    from tgcn_amd import graph
    op = _operand()
    monkeypatch.setattr(graph, "HUB_MIN", 0)
    plain = graph.Schedule(op.rowptr, op.n, 16, edges=op.edges)
    monkeypatch.setattr(graph, "HUB_MIN", HUB_MIN)
    monkeypatch.setattr(graph, "HUB_SEG", HUB_SEG)
    monkeypatch.setattr(graph, "HUB_GATE_BYTES", plain.npartial * 16 * 16)
    at = graph.Schedule(op.rowptr, op.n, 16, edges=op.edges)
    _assert_equal_schedules(at, plain)
    monkeypatch.setattr(graph, "HUB_GATE_BYTES", plain.npartial * 16 * 16 - 1)
    above = graph.Schedule(op.rowptr, op.n, 16, edges=op.edges)
    assert above.npartial < plain.npartial


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def hub_case():
    """operand on the device, its forced schedule (torch builder), inputs and the fp64 products -- made once"""
    from tgcn_amd import graph
    keep = (graph.HUB_MIN, graph.HUB_SEG, graph.HUB_GATE_BYTES)
    graph.HUB_MIN, graph.HUB_SEG, graph.HUB_GATE_BYTES = HUB_MIN, HUB_SEG, 0
    try:
        op = _operand("cuda")
        s16 = op.schedule(16)              # C = 64 fp32 and C = 128 bf16
    finally:
        graph.HUB_MIN, graph.HUB_SEG, graph.HUB_GATE_BYTES = keep
    assert s16.nwseg == 91 and s16.nhuge == 1
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, N, 64)).astype(np.float32)
    z = rng.standard_normal((2, N, 64)).astype(np.float32)
    A = op.to_scipy().astype(np.float64)
    S = np.stack([A @ x[b].astype(np.float64) for b in range(2)])
    return {"op": op, "x": x, "z": z, "S": S, "A": A}


def _rel(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.gpu
def test_library_builder_equals_torch_builder_with_the_rule_forced(gpu_device, monkeypatch):
    from tgcn_amd import graph, _lib
    L = _lib.lib()
    op = _operand("cuda")
    _force(monkeypatch, graph)
    py_s = graph.Schedule(op.rowptr, op.n, 16, edges=op.edges, builder="torch")
    assert py_s.nwseg == 91
    try:
        _lib.check(L.tgcn_set_tuning(b"sched_hub_min", HUB_MIN))
        _lib.check(L.tgcn_set_tuning(b"sched_hub_seg", HUB_SEG))
        _lib.check(L.tgcn_set_tuning(b"sched_hub_gate_mb", 0))
        lib_s = graph.Schedule.__new__(graph.Schedule)
        lib_s._build_library(op.rowptr, op.n, 16, op.edges, op.n_cols)
        lib_4 = graph.Schedule.__new__(graph.Schedule)
        lib_4._build_library(op.rowptr, op.n, 4, op.edges, op.n_cols)
    finally:
        L.tgcn_reset_tuning()
    _assert_equal_schedules(lib_s, py_s)
    _assert_equal_schedules(lib_4, graph.Schedule(op.rowptr, op.n, 4, edges=op.edges, builder="torch"))      # other widths: untouched
    monkeypatch.undo()
    _assert_equal_schedules(graph.Schedule(op.rowptr, op.n, 16, edges=op.edges, builder="library"),           # default gate: the plain schedule
                            graph.Schedule(op.rowptr, op.n, 16, edges=op.edges, builder="torch"))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "alpha_beta_z", "p_output", "streaming"])
def test_hop_f32_with_hub_segments(form, hub_case, gpu_device):
    from tgcn_amd import _lib, functional as F
    L = _lib.lib()
    op = hub_case["op"]
    x, z = torch.as_tensor(hub_case["x"]).cuda(), torch.as_tensor(hub_case["z"]).cuda()
    S = hub_case["S"]
    try:
        if form == "streaming":
            _lib.check(L.tgcn_set_tuning(b"hop_variant", 6))      # the non-temporal form of large outputs, forced on a small one
        if form == "alpha_beta_z":
            y = F.csr_hop(op, x, z=z, alpha=2.0, beta=-1.0)
            ref = 2.0 * S - hub_case["z"].astype(np.float64)
        elif form == "p_output":
            y, p = F.csr_hop(op, x, z=z, alpha=2.0, beta=-1.0, want_p=True)
            ref = 2.0 * S - hub_case["z"].astype(np.float64)
            err_p = _rel(p.cpu().numpy(), S)
            print("P output: %.3e" % err_p)
            assert err_p <= 1e-5
        else:
            y = F.csr_hop(op, x)
            ref = S
        y2 = F.csr_hop(op, x) if form in ("plain", "streaming") else None
        torch.cuda.synchronize()
    finally:
        L.tgcn_reset_tuning()
    err = _rel(y.cpu().numpy(), ref)
    print("%s (nb = 2): %.3e" % (form, err))
    assert err <= 1e-5
    if y2 is not None:
        assert torch.equal(y, y2)                                  # fixed fold order: two runs are bitwise equal


@pytest.mark.gpu
def test_hop_bf16_with_hub_segments(hub_case, gpu_device):
    from tgcn_amd import functional as F
    op = hub_case["op"]
    rng = np.random.default_rng(11)
    xb = torch.as_tensor(rng.standard_normal((1, N, 128)).astype(np.float32)).cuda().to(torch.bfloat16)
    y = F.csr_hop_bf16(op, xb)
    y2 = F.csr_hop_bf16(op, xb)
    assert y.dtype == torch.bfloat16 and op.schedule_for(64).nwseg == 91
    ref = hub_case["A"] @ xb[0].float().cpu().numpy().astype(np.float64)
    err = _rel(y[0].float().cpu().numpy(), ref)
    print("bf16 C = 128: %.3e" % err)
    assert err <= 2.0 ** -8 + 1e-5
    assert torch.equal(y, y2)


@pytest.mark.gpu
def test_compact_layer_with_hub_segments(gpu_device, monkeypatch):
    """tgcn_cheb_compact_layer_f32 through a CompactPlan whose schedule carries hub wave segments, against the uncompacted path on the plain
    schedule: the same graph with 1,000 vertices without entries appended"""
    from tgcn_amd import functional as F, graph
    n, q, Cc, Nn, K = N + 1000, 2, 64, 64, 5
    row, col, val = _coo(3)
    dev = lambda a: torch.as_tensor(a).cuda()
    rng = np.random.default_rng(5)
    x = dev(rng.standard_normal((q, n, Cc)).astype(np.float32))
    W = dev((rng.standard_normal((K, Cc, Nn)) / np.sqrt(K * Cc)).astype(np.float32))
    bias = dev(rng.standard_normal((n, Nn)).astype(np.float32))
    W2 = F.fold_weight(F.power_fold_matrix(K, x.device), W).reshape(K * Cc, Nn).contiguous()
    monkeypatch.setattr(graph, "COMPACT_MIN_ROWS", 1)
    monkeypatch.setattr(graph, "HUB_MIN", 0)
    plain_op = graph.GraphOperand.from_coo(n, dev(row), dev(col), dev(val))
    plain = F.cheb_forward_raw(plain_op, x, W2, bias, 2, F.MODE_POWER, K, layout=0, q_chunk=1)
    assert plain_op.schedule_for(Cc).nwseg == 2
    _force(monkeypatch, graph)
    op = graph.GraphOperand.from_coo(n, dev(row), dev(col), dev(val))
    plan = op.compact_plan()
    assert plan is not None and plan.n_c < n and plan.schedule_for(Cc).nwseg == 91
    comp = F.cheb_forward_compact(plan, x, W2, bias, 2, K, q_chunk=1)
    comp2 = F.cheb_forward_compact(plan, x, W2, bias, 2, K, q_chunk=2)
    err = float((comp - plain).abs().max() / plain.abs().max())
    print("compact layer, hub segments against the plain schedule: %.3e" % err)
    assert err <= 1e-5
    assert torch.equal(comp, comp2)


@pytest.mark.gpu
def test_shipped_segment_length_forced_on_the_small_graph(gpu_device, monkeypatch):
    """HUB_SEG = 64, what ships behind the gate (16 entries per lane group: one entry load each), at HUB_MIN = 256: both builders, the plain and
    the streaming form against fp64"""
    from tgcn_amd import graph, _lib, functional as F
    L = _lib.lib()
    monkeypatch.setattr(graph, "HUB_MIN", HUB_MIN)
    monkeypatch.setattr(graph, "HUB_SEG", 64)
    monkeypatch.setattr(graph, "HUB_GATE_BYTES", 0)
    op = _operand("cuda")
    s = op.schedule(16)
    assert s.nwseg == 2 + 5 + 6 + 7 + 16 + 141 and s.nhuge == 1
    rng = np.random.default_rng(13)
    x = rng.standard_normal((1, N, 64)).astype(np.float32)
    ref = op.to_scipy().astype(np.float64) @ x[0].astype(np.float64)
    xd = torch.as_tensor(x).cuda()
    try:
        _lib.check(L.tgcn_set_tuning(b"sched_hub_min", HUB_MIN))
        _lib.check(L.tgcn_set_tuning(b"sched_hub_seg", 64))
        _lib.check(L.tgcn_set_tuning(b"sched_hub_gate_mb", 0))
        lib_s = graph.Schedule.__new__(graph.Schedule)
        lib_s._build_library(op.rowptr, op.n, 16, op.edges, op.n_cols)
        L.tgcn_reset_tuning()
        y = F.csr_hop(op, xd)
        _lib.check(L.tgcn_set_tuning(b"hop_variant", 6))
        ys = F.csr_hop(op, xd)
        torch.cuda.synchronize()
    finally:
        L.tgcn_reset_tuning()
    _assert_equal_schedules(lib_s, s)
    for name, got in (("plain", y), ("streaming", ys)):
        err = _rel(got[0].cpu().numpy(), ref)
        print("HUB_SEG = 64, %s: %.3e" % (name, err))
        assert err <= 1e-5
