"""The compacted fp32 layer with its projections BESIDE the hops (tgcn_cheb_compact_layer_f32): the left-out rows' projection and
the kept rows' projection of every group of time steps but the last run on the library's side stream in the claiming form of the streaming
kernel.  The path is meant for operands whose hop tensors exceed the Infinity Cache; here the size gate is lowered ("compact_overlap_min_mb"
= 0) and the streaming kernel asked for at every row count ("project_variant" = 6), so a 3,000-vertex graph takes it.  Whatever runs where,
every output row is computed by the same kernel arithmetic: overlap on must equal overlap off BIT FOR BIT -- both recurrences, K = 2 and 5,
1 ... 9 time steps (one group, a ragged last group, several side groups), several passes, kept terms, repeated calls (counter and event
reuse), a non-default stream -- and under stream capture nothing may reach the side stream."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_VERT, C_ROW, N_OUT = 3000, 64, 64


@pytest.fixture(scope="module")
def operand(gpu_device):
    """about 40 % isolated vertices (no entries, never pointed at); rows of <= 32, 33 ... 128 and several hundred entries among the others"""
    from tgcn_amd import graph
    rng = np.random.default_rng(5)
    live = np.sort(rng.permutation(N_VERT)[: int(N_VERT * 0.6)])
    deg = rng.integers(1, 33, live.size)
    deg[rng.permutation(live.size)[:60]] = rng.integers(33, 129, 60)
    deg[[3, 500, 1700]] = (300, 450, 700)
    row = np.repeat(live, deg)
    col = live[rng.integers(0, live.size, row.size)]
    val = (rng.standard_normal(row.size) / 6).astype(np.float32)
    old = graph.COMPACT_MIN_ROWS
    graph.COMPACT_MIN_ROWS = 1
    try:
        op = graph.GraphOperand.from_coo(N_VERT, torch.as_tensor(row).cuda(), torch.as_tensor(col).cuda(), torch.as_tensor(val).cuda())
        plans = {0: op.compact_plan("rows"), 1: op.compact_plan("closed")}
    finally:
        graph.COMPACT_MIN_ROWS = old
    for plan in plans.values():
        assert plan is not None and plan.n_c == live.size and plan.n_empty == N_VERT - live.size
    sched = plans[0].schedule_for(C_ROW, True)
    assert sched.nseg > 0 and sched.nlong > 0          # rows above the threshold: segments and the fix-up launch run between the projections
    return op, plans


def _weights(mode, K, seed):
    from tgcn_amd import functional as F
    g = torch.Generator(device="cuda").manual_seed(seed)
    W = torch.randn((K, C_ROW, N_OUT), device="cuda", generator=g) / (K * C_ROW) ** 0.5
    bias = torch.randn((N_VERT, N_OUT), device="cuda", generator=g)
    W_left = F.left_out_weight(W, mode) if mode == F.MODE_CHEBYSHEV else None
    return W.reshape(K * C_ROW, N_OUT).contiguous(), W_left, bias


def _forward(plan, x, W2, W_left, bias, mode, K, q_chunk, keep, overlap, group=4):
    """-> ([out, kept terms ...], kernels that went to the side stream)"""
    from tgcn_amd import functional as F, _lib
    L = _lib.lib()
    for key, v in ((b"project_variant", 6), (b"compact_overlap_min_mb", 0), (b"compact_overlap", overlap), (b"compact_overlap_group", group)):
        _lib.check(L.tgcn_set_tuning(key, v))
    before = L.tgcn_side_stream_launches()
    res = F.cheb_forward_compact(plan, x, W2, bias, 2, K, q_chunk=q_chunk, mode=mode, W_left=W_left, keep=keep)
    out, terms = res if keep else (res, [])
    return [out] + [t for t in terms if t is not x], L.tgcn_side_stream_launches() - before


def _side_launches(q, qc, group):
    """the left-out rows' projection plus one per group but the last, in every pass of more than one group"""
    total = 0
    for q0 in range(0, q, qc):
        qn = min(qc, q - q0)
        if qn > group:
            total += 1 + (qn - 1) // group
    return total


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", [2, 5])
def test_overlap_on_equals_overlap_off(mode, K, operand, gpu_device):
    _, plans = operand
    plan = plans[mode]
    W2, W_left, bias = _weights(mode, K, 10 * K + mode)
    g = torch.Generator(device="cuda").manual_seed(K + mode)
    xs = torch.randn((9, N_VERT, C_ROW), device="cuda", generator=g)
    for q, q_chunk, keep, group in [(q, q, keep, 4) for q in (1, 3, 5, 9) for keep in (False, True)] + [(9, 4, False, 4), (9, 4, False, 2)]:
        x = xs[:q].contiguous()
        want, n_off = _forward(plan, x, W2, W_left, bias, mode, K, q_chunk, keep, 0, group)
        got, n_on = _forward(plan, x, W2, W_left, bias, mode, K, q_chunk, keep, 1, group)
        again, n_again = _forward(plan, x, W2, W_left, bias, mode, K, q_chunk, keep, 1, group)     # the counter and the events once more
        assert n_off == 0 and n_on == n_again == _side_launches(q, q_chunk, group), (q, q_chunk, keep, group, n_off, n_on)
        assert len(want) == len(got) == len(again) == 1 + (0 if not keep else (K if mode == 1 else K - 1))
        for a, b, c in zip(want, got, again):
            assert not torch.isnan(a).any()
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32)), (q, q_chunk, keep, group)
    assert _side_launches(9, 9, 4) == 3 and _side_launches(5, 5, 4) == 2 and _side_launches(9, 4, 4) == 0 and _side_launches(9, 4, 2) == 4


def test_overlap_on_a_non_default_stream(operand, gpu_device):
    _, plans = operand
    W2, W_left, bias = _weights(0, 5, 3)
    x = torch.randn((9, N_VERT, C_ROW), device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    want, _ = _forward(plans[0], x, W2, W_left, bias, 0, 5, 9, False, 0)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got, n_on = _forward(plans[0], x, W2, W_left, bias, 0, 5, 9, False, 1)
        # work queued on the caller's stream after the call sees the whole result: the side stream was joined into it
        copy = got[0].clone()
    s.synchronize()
    assert n_on == 3
    assert torch.equal(want[0].view(torch.int32), copy.view(torch.int32))


def test_stream_capture_keeps_off_the_side_stream(operand, gpu_device):
    _, plans = operand
    W2, W_left, bias = _weights(1, 5, 4)
    x = torch.randn((9, N_VERT, C_ROW), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    eager, n_eager = _forward(plans[1], x, W2, W_left, bias, 1, 5, 9, False, 1)
    assert n_eager == 3
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured, n_cap = _forward(plans[1], x, W2, W_left, bias, 1, 5, 9, False, 1)
    assert n_cap == 0          # a captured graph gets no parallel branch
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager[0].view(torch.int32), captured[0].view(torch.int32))
