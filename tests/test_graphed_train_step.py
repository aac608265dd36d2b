"""tgcn_amd.GraphedTrainStep against the eager training loop on an identically seeded copy of the model and optimizer: the eager loop
is existing code, the wrapper is what is under test.  GPU only.

Shapes: the ring graphs of tests/test_end_to_end.py (160 and 40 vertices), batch 6 (even, no multiple of 4), TGCNCheb_H(L0, 1, 16, 3, 5) ->
relu -> gcn_pool_4 -> GCNCheb(L2, 16, 24, 3) -> relu -> gcn_pool_4 -> Linear(240, 6) -> log_softmax with nll_loss: the smallest that still
pool twice and have the per-vertex bias, the channel bias and a torch layer in one step.

Tolerances: losses as tests/test_end_to_end.py's capture test (rtol 2e-4, atol 1e-5); parameters after the steps the same rtol relative to
the largest absolute parameter value.  Where the two loops were measured bit-identical the test asserts torch.equal (EXACT below;
DESIGN.md 3.11 lists the cases)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF

import tgcn_amd
from tgcn_amd import _lib
from test_end_to_end import _ring_graph

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-4, 1e-5
# bfloat16 keeps 8 significand bits where float32 keeps 24: one rounding is 2^-8 relative instead of 2^-24, and the tolerance above is a
# bound on accumulated float32 roundings, so the same number of bfloat16 roundings is bounded by it times 2^-8 / 2^-24 = 2^16.
BF16_SCALE = 2.0 ** -8 / 2.0 ** -24
EXACT = True      # replay and eager loop run the same kernels on the same values in the same order: measured bit-identical in every case


@pytest.fixture(scope="module")
def graphs():
    rng = np.random.default_rng(1)
    return _ring_graph(160, 30, rng), _ring_graph(40, 8, rng)


class Net(nn.Module):
    def __init__(self, L0, L2, bn=False):
        super().__init__()
        self.tgcn1 = tgcn_amd.TGCNCheb_H(L0, 1, 16, 3, 5)
        self.gcn2 = tgcn_amd.GCNCheb(L2, 16, 24, 3)
        self.bn = nn.BatchNorm1d(10 * 24) if bn else None
        self.fc = nn.Linear(10 * 24, 6)

    def forward(self, x):
        x = tgcn_amd.gcn_pool_4(TF.relu(self.tgcn1(x)))
        x = tgcn_amd.gcn_pool_4(TF.relu(self.gcn2(x)))
        x = x.reshape(x.shape[0], -1).to(self.fc.weight.dtype)
        if self.bn is not None:
            x = self.bn(x)
        return TF.log_softmax(self.fc(x), dim=1)


def _batches(sizes, shape, classes, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [((torch.randn((q,) + shape, generator=g).to(device="cuda", dtype=dtype),), torch.randint(0, classes, (q,), generator=g).cuda())
            for q in sizes]


def _eager_loop(model, opt, loss_fn, batches, before=None, after=None):
    losses = []
    for i, (inp, y) in enumerate(batches):
        if before is not None:
            before(model, i)
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(model(*inp), y)
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
        if after is not None:
            after(opt, i)
    return losses


def _graphed_loop(gts, batches, before=None, after=None):
    losses = []
    for i, (inp, y) in enumerate(batches):
        if before is not None:
            before(gts.model, i)
        losses.append(gts(inp if len(inp) > 1 else inp[0], y).clone())
        if after is not None:
            after(gts.optimizer, i)
    return losses


def _compare(name, got, ref, model_g, model_e, scale=1.0, exact=EXACT):
    """losses per step and all parameters and buffers after the steps; prints each figure before it asserts"""
    got, ref = torch.stack(got).double().cpu(), torch.stack(ref).double().cpu()
    same_loss = torch.equal(got, ref)
    print("%s: losses %s, bit-identical %s, max |diff| %.3e" % (name, [round(float(v), 6) for v in ref], same_loss, float((got - ref).abs().max())))
    state_g, state_e = dict(model_g.state_dict()), dict(model_e.state_dict())
    assert sorted(state_g) == sorted(state_e)
    pmax = max(float(v.abs().max()) for v in state_e.values() if v.is_floating_point())
    worst, same = 0.0, True
    for k in state_e:
        same = same and torch.equal(state_g[k], state_e[k])
        worst = max(worst, float((state_g[k].double() - state_e[k].double()).abs().max()))
    print("%s: parameters bit-identical %s, max |diff| %.3e against max |p| %.3e" % (name, same, worst, pmax))
    assert torch.isfinite(ref).all()
    assert np.allclose(got.numpy(), ref.numpy(), rtol=RTOL * scale, atol=ATOL * scale), (got, ref)
    assert worst <= RTOL * scale * pmax, (worst, pmax)
    if exact:
        assert same_loss and same


def _pair(make):
    """(model, optimizer) twice from the same seed"""
    out = []
    for _ in range(2):
        torch.manual_seed(3)
        out.append(make())
    return out


def _sgd(net):
    return torch.optim.SGD(net.parameters(), lr=0.05, momentum=0.5)


# ---------------------------------------------------------------------------------------------------------------- 1
def test_sgd_with_momentum_matches_the_eager_loop(gpu_device, graphs):
    def make():
        net = Net(*graphs).cuda()
        return net, _sgd(net)
    (net_e, opt_e), (net_g, opt_g) = _pair(make)
    batches = _batches([6] * 5, (160, 5), 6)
    ref = _eager_loop(net_e, opt_e, TF.nll_loss, batches)
    gts = tgcn_amd.GraphedTrainStep(net_g, opt_g, TF.nll_loss, batches[0][0], batches[0][1])
    got = _graphed_loop(gts, batches)
    assert gts.recaptures == 0
    _compare("sgd momentum", got, ref, net_g, net_e)
    assert gts.output.shape == (6, 6) and not gts.output.requires_grad


def test_the_example_batch_passed_again_between_other_batches(gpu_device, graphs):
    """the example objects are not copied while the static buffers hold them -- and are copied again once another batch has been in"""
    def make():
        net = Net(*graphs).cuda()
        return net, _sgd(net)
    (net_e, opt_e), (net_g, opt_g) = _pair(make)
    b = _batches([6] * 2, (160, 5), 6)
    batches = [b[0], b[0], b[1], b[0], b[0]]
    ref = _eager_loop(net_e, opt_e, TF.nll_loss, batches)
    gts = tgcn_amd.GraphedTrainStep(net_g, opt_g, TF.nll_loss, b[0][0], b[0][1])
    got = _graphed_loop(gts, batches)
    _compare("example batch again", got, ref, net_g, net_e)
    b[0][0][0].mul_(2.0)          # the example tensor edited in place: its version says so, and the edit is copied in
    ref = _eager_loop(net_e, opt_e, TF.nll_loss, b[:1])
    _compare("example batch edited", [gts(b[0][0][0], b[0][1]).clone()], ref, net_g, net_e)


def test_a_loss_that_is_not_0_dim_is_refused_with_the_state_put_back(gpu_device, graphs):
    torch.manual_seed(3)
    net = Net(*graphs, bn=True).cuda()
    opt = _sgd(net)
    (x,), y = _batches([6], (160, 5), 6)[0]
    kept = {k: v.detach().clone() for k, v in net.state_dict().items()}
    with pytest.raises(_lib.TgcnError, match="returns a 0-dim tensor, got \\(6,\\)"):
        tgcn_amd.GraphedTrainStep(net, opt, lambda out, t: TF.nll_loss(out, t, reduction="none"), x, y)
    for k, v in kept.items():
        assert torch.equal(net.state_dict()[k], v), k
    assert not opt.state and all(p.grad is None for p in net.parameters())


# ---------------------------------------------------------------------------------------------------------------- 2
def test_construction_is_not_a_training_step(gpu_device, graphs):
    torch.manual_seed(5)
    net = Net(*graphs, bn=True).cuda()
    opt = _sgd(net)
    (x,), y = _batches([6], (160, 5), 6)[0]
    # one real step first, so that the optimizer has state of its own that must come back, and the statistics are not their initial values
    opt.zero_grad(set_to_none=True)
    TF.nll_loss(net(x), y).backward()
    opt.step()
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    assert "bn.running_mean" in before and "bn.num_batches_tracked" in before and int(before["bn.num_batches_tracked"]) == 1
    state_before = copy.deepcopy(opt.state_dict()["state"])
    assert state_before and all(torch.is_tensor(s["momentum_buffer"]) for s in state_before.values())
    tgcn_amd.GraphedTrainStep(net, opt, TF.nll_loss, x, y, warmup=3)
    after = net.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    state_after = opt.state_dict()["state"]
    assert sorted(state_after) == sorted(state_before)
    for i, s in state_before.items():
        assert torch.equal(state_after[i]["momentum_buffer"], s["momentum_buffer"]), i
    # and from a fresh optimizer: the state the warm-up made is zero, where torch's first step starts
    torch.manual_seed(5)
    net2 = Net(*graphs, bn=True).cuda()
    opt2 = torch.optim.Adam(net2.parameters(), lr=1e-2, capturable=True)
    before2 = {k: v.detach().clone() for k, v in net2.state_dict().items()}
    tgcn_amd.GraphedTrainStep(net2, opt2, TF.nll_loss, x, y, warmup=2)
    for k, v in before2.items():
        assert torch.equal(net2.state_dict()[k], v), k
    for s in opt2.state.values():
        for k, v in s.items():
            assert torch.is_tensor(v) and not bool(v.any()), k


# ---------------------------------------------------------------------------------------------------------------- 3
def test_adam_with_exponential_lr_recaptures_when_the_rate_moves(gpu_device, graphs):
    def make():
        net = Net(*graphs).cuda()
        return net, torch.optim.Adam(net.parameters(), lr=1e-2, capturable=True)
    (net_e, opt_e), (net_g, opt_g) = _pair(make)
    batches = _batches([6] * 6, (160, 5), 6)
    scheds = {}

    def after(opt, i):      # the scheduler steps after calls 2 and 4 of 6
        if i in (1, 3):
            scheds[id(opt)].step()
    scheds[id(opt_e)] = torch.optim.lr_scheduler.ExponentialLR(opt_e, gamma=0.5)
    ref = _eager_loop(net_e, opt_e, TF.nll_loss, batches, after=after)
    gts = tgcn_amd.GraphedTrainStep(net_g, opt_g, TF.nll_loss, batches[0][0], batches[0][1])
    scheds[id(opt_g)] = torch.optim.lr_scheduler.ExponentialLR(opt_g, gamma=0.5)
    got = _graphed_loop(gts, batches, after=after)
    assert opt_g.param_groups[0]["lr"] == opt_e.param_groups[0]["lr"] == 1e-2 * 0.25
    assert gts.recaptures == 2
    _compare("adam + ExponentialLR", got, ref, net_g, net_e)
    # without a scheduler nothing is captured again
    (net_e, opt_e), (net_g, opt_g) = _pair(make)
    ref = _eager_loop(net_e, opt_e, TF.nll_loss, batches)
    gts = tgcn_amd.GraphedTrainStep(net_g, opt_g, TF.nll_loss, batches[0][0], batches[0][1])
    got = _graphed_loop(gts, batches)
    assert gts.recaptures == 0
    _compare("adam", got, ref, net_g, net_e)


# ---------------------------------------------------------------------------------------------------------------- 4
def test_other_shapes(gpu_device, graphs):
    def make():
        net = Net(*graphs).cuda()
        return net, _sgd(net)
    (net_e, opt_e), (net_g, opt_g) = _pair(make)
    batches = _batches([6, 6, 4, 6], (160, 5), 6)
    ref = _eager_loop(net_e, opt_e, TF.nll_loss, batches)
    gts = tgcn_amd.GraphedTrainStep(net_g, opt_g, TF.nll_loss, batches[0][0], batches[0][1], other_shapes="eager")
    got, kinds = [], []
    for (x,), y in batches:
        loss = gts(x, y)
        kinds.append(loss is gts._loss)
        assert gts.output.shape == (x.shape[0], 6)
        got.append(loss.clone())
    assert kinds == [True, True, False, True]      # the batch of 4 ran eagerly (a fresh loss tensor), the batch of 6 behind it replayed
    assert gts.recaptures == 0
    _compare("other_shapes=eager", got, ref, net_g, net_e)
    # the default refuses
    torch.manual_seed(3)
    net, opt = make()
    gts = tgcn_amd.GraphedTrainStep(net, opt, TF.nll_loss, batches[0][0], batches[0][1])
    for (x,), y in batches[:2]:
        gts(x, y)
    kept = [p.detach().clone() for p in net.parameters()]
    with pytest.raises(_lib.TgcnError, match="one graph per batch shape"):
        gts(batches[2][0][0], batches[2][1])
    with pytest.raises(_lib.TgcnError, match="one graph per batch shape"):
        gts(batches[0][0][0].double(), batches[0][1])
    assert all(torch.equal(p, k) for p, k in zip(net.parameters(), kept))
    net.eval()
    with pytest.raises(_lib.TgcnError, match="model.training is False"):
        gts(batches[3][0][0], batches[3][1])
    net.train()
    gts(batches[3][0][0], batches[3][1])


# ---------------------------------------------------------------------------------------------------------------- 5, 6
class SeriesNet(nn.Module):
    """one streaming time layer through a pooled epilogue, a linear head per window"""

    def __init__(self, L0, kind):
        super().__init__()
        self.kind = kind
        self.layer = tgcn_amd.ChebTimeConv(2, 8, 3, 3) if kind == "edge_chunked" else tgcn_amd.TGCNCheb_H(L0, 2, 8, 3, 3)
        self.fc = nn.Linear(40 * 8, 6)
        self.seed = None

    def forward(self, series, *graph_args):
        if self.kind == "dropout":
            z = tgcn_amd.cheb_series_relu_dropout_pool(self.layer, series, p=0.5, seed=self.seed)
        elif self.kind == "chunked":
            z = tgcn_amd.cheb_series_relu_pool_chunked(self.layer, series, time_chunk=5, p=0.0)
        else:
            z = tgcn_amd.cheb_series_relu_pool_chunked(self.layer, series, *graph_args, time_chunk=5, p=0.0, dilation=2)
        return TF.log_softmax(self.fc(z.reshape(z.shape[0], -1)), dim=1)


def _series_batches(steps, windows, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [((torch.randn((2, 160, 12, 2), generator=g).cuda(),), torch.randint(0, 6, (2 * windows,), generator=g).cuda()) for _ in range(steps)]


def test_series_dropout_with_a_seed_tensor(gpu_device, graphs):
    def make():
        net = SeriesNet(graphs[0], "dropout").cuda()
        net.seed = torch.zeros(1, dtype=torch.int64, device="cuda")
        return net, _sgd(net)
    (net_e, opt_e), (net_g, opt_g) = _pair(make)
    batches = _series_batches(5, 10)          # 12 time rows, H = 3: 10 windows per recording

    def before(model, i):      # the caller owns the seed: rewritten before every step, in both loops
        model.seed.fill_(1000 + 17 * i)
    ref = _eager_loop(net_e, opt_e, TF.nll_loss, batches, before=before)
    gts = tgcn_amd.GraphedTrainStep(net_g, opt_g, TF.nll_loss, batches[0][0], batches[0][1])
    got = _graphed_loop(gts, batches, before=before)
    _compare("series dropout, seed tensor", got, ref, net_g, net_e)
    # the dropout is active: the same step under another seed gives another loss
    assert not torch.equal(ref[0], _eager_loop(*_pair(make)[0], TF.nll_loss, batches[:1], before=lambda m, i: m.seed.fill_(5))[0])


def test_series_dropout_draws_a_new_mask_on_every_replay(gpu_device, graphs):
    torch.manual_seed(3)
    net = SeriesNet(graphs[0], "dropout").cuda()      # seed=None: drawn on the device inside the captured step
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    (x,), y = _series_batches(1, 10)[0]
    kept = [p.detach().clone() for p in net.parameters()]
    gts = tgcn_amd.GraphedTrainStep(net, opt, TF.nll_loss, x, y)
    gts(x, y)
    first = gts.output.clone()
    gts(x, y)
    assert all(torch.equal(p, k) for p, k in zip(net.parameters(), kept))      # lr = 0: the same function both times
    assert not torch.equal(first, gts.output)


@pytest.mark.parametrize("kind", ["chunked", "edge_chunked"])
def test_chunk_loop_in_the_step(gpu_device, graphs, kind):
    """time_chunk=5 on 12 time rows: chunks of 5, 5 and 2 rows, so the ring wraps and the last chunk is short; the ChebTimeConv at dilation 2
    keeps 4 ring rows"""
    edge_index = graphs[0].nonzero().t().contiguous().cuda()

    def make():
        net = SeriesNet(graphs[0], kind).cuda()
        return net, _sgd(net)
    (net_e, opt_e), (net_g, opt_g) = _pair(make)
    batches = _series_batches(5, 12)          # the causal layer: 12 output rows per recording
    if kind == "edge_chunked":
        batches = [((x, edge_index), y) for (x,), y in batches]
    ref = _eager_loop(net_e, opt_e, TF.nll_loss, batches)
    gts = tgcn_amd.GraphedTrainStep(net_g, opt_g, TF.nll_loss, batches[0][0], batches[0][1])
    got = _graphed_loop(gts, batches)
    _compare("chunk loop, %s" % kind, got, ref, net_g, net_e)


class PathsNet(nn.Module):
    """the other training paths a step may contain, one per kind: the fused caller patterns of the batch layers, the unchunked pooled series
    call, the one-launch series layer, forward_series with time_chunk, and the two layer classes no other case runs"""

    def __init__(self, L0, L2, kind):
        super().__init__()
        self.kind = kind
        if kind == "relu_pool":
            self.l1, self.l2 = tgcn_amd.TGCNCheb_H(L0, 1, 16, 3, 5), tgcn_amd.GCNCheb(L2, 16, 24, 3)
            self.fc = nn.Linear(10 * 24, 6)
        elif kind == "tgcn_cheb":
            self.l1, self.l2 = tgcn_amd.TGCNCheb(L0, 5, 16, 3), tgcn_amd.ChebTimeConv(2, 8, 3, 4)
            self.fc = nn.Linear(40 * 8, 6)
        else:
            self.l1 = tgcn_amd.TGCNCheb_H(L0, 2, 8, 3, 3)
            self.fc = nn.Linear(40 * 8, 6)
        self.seed = None

    def forward(self, x, *graph_args):
        if self.kind == "relu_pool":
            x = tgcn_amd.cheb_relu_pool(self.l1, x, pool=4)
            x = tgcn_amd.cheb_relu_dropout_pool(self.l2, x, p=0.25, pool=4, seed=self.seed)
        elif self.kind == "tgcn_cheb":
            x = tgcn_amd.gcn_pool_4(TF.relu(self.l1(x)))                     # (q, 40, 16)
            x = TF.relu(self.l2(x.reshape(x.shape[0], 40, 4, 4)[..., :2].contiguous(), *graph_args))
        elif self.kind == "series_relu_pool":
            x = tgcn_amd.cheb_series_relu_pool(self.l1, x, pool=4)
        elif self.kind == "series_fused":
            x = tgcn_amd.gcn_pool_4(TF.relu(self.l1.forward_series(x, fused=True)))
        else:
            x = tgcn_amd.gcn_pool_4(TF.relu(self.l1.forward_series(x, padding="causal", time_chunk=5)))
        return TF.log_softmax(self.fc(x.reshape(x.shape[0], -1)), dim=1)


@pytest.mark.parametrize("kind", ["relu_pool", "tgcn_cheb", "series_relu_pool", "series_fused", "series_time_chunk"])
def test_other_training_paths_in_the_step(gpu_device, graphs, kind):
    def make():
        net = PathsNet(*graphs, kind).cuda()
        net.seed = torch.full((1,), 77, dtype=torch.int64, device="cuda")
        return net, _sgd(net)
    (net_e, opt_e), (net_g, opt_g) = _pair(make)
    if kind in ("relu_pool", "tgcn_cheb"):
        batches = _batches([6] * 3, (160, 5), 6)
        if kind == "tgcn_cheb":      # the ChebTimeConv runs on the coarse graph's edges
            edge_index = graphs[1].nonzero().t().contiguous().cuda()
            batches = [((x, edge_index), y) for (x,), y in batches]
    else:
        batches = _series_batches(3, 12 if kind == "series_time_chunk" else 10)
    ref = _eager_loop(net_e, opt_e, TF.nll_loss, batches)
    gts = tgcn_amd.GraphedTrainStep(net_g, opt_g, TF.nll_loss, batches[0][0], batches[0][1])
    got = _graphed_loop(gts, batches)
    _compare("other paths, %s" % kind, got, ref, net_g, net_e)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_bfloat16_model(gpu_device, graphs):
    def make():
        net = Net(*graphs).cuda().to(torch.bfloat16)
        return net, _sgd(net)
    (net_e, opt_e), (net_g, opt_g) = _pair(make)
    batches = _batches([6] * 5, (160, 5), 6, dtype=torch.bfloat16)
    ref = _eager_loop(net_e, opt_e, TF.nll_loss, batches)
    gts = tgcn_amd.GraphedTrainStep(net_g, opt_g, TF.nll_loss, batches[0][0], batches[0][1])
    got = _graphed_loop(gts, batches)
    assert got[0].dtype == torch.bfloat16
    _compare("bfloat16", got, ref, net_g, net_e, scale=BF16_SCALE)


# ---------------------------------------------------------------------------------------------------------------- 8
class EdgeNet(nn.Module):
    def __init__(self, E=None):
        super().__init__()
        self.conv = tgcn_amd.ChebConv(1, 4, 3)
        self.fc = nn.Linear(160 * 4, 6)
        self.ew = nn.Parameter(torch.ones(E)) if E else None

    def forward(self, x, edge_index):
        return TF.log_softmax(self.fc(TF.relu(self.conv(x, edge_index, self.ew)).reshape(x.shape[0], -1)), dim=1)


def test_learnable_edge_weight_is_refused_before_the_capture(gpu_device, graphs):
    """documented: a step that trains edge weights raises TgcnError after the warm-up, with everything restored and nothing captured"""
    edge_index = graphs[0].nonzero().t().contiguous().cuda()
    torch.manual_seed(3)
    net = EdgeNet(edge_index.shape[1]).cuda()
    opt = _sgd(net)
    (x,), y = _batches([6], (160,), 6)[0]
    kept = {k: v.detach().clone() for k, v in net.state_dict().items()}
    with pytest.raises(_lib.TgcnError, match="learnable edge weights.*cannot run inside a hipGraph capture"):
        tgcn_amd.GraphedTrainStep(net, opt, TF.nll_loss, (x, edge_index), y)
    assert not torch.cuda.is_current_stream_capturing()
    for k, v in kept.items():
        assert torch.equal(net.state_dict()[k], v), k
    # fixed weights on the same model shape train under the wrapper
    (net_e, opt_e), (net_g, opt_g) = _pair(lambda: (lambda n: (n, _sgd(n)))(EdgeNet().cuda()))
    batches = [((xb, edge_index), yb) for (xb,), yb in _batches([6] * 3, (160,), 6)]
    ref = _eager_loop(net_e, opt_e, TF.nll_loss, batches)
    gts = tgcn_amd.GraphedTrainStep(net_g, opt_g, TF.nll_loss, batches[0][0], batches[0][1])
    got = _graphed_loop(gts, batches)
    _compare("ChebConv, fixed weights", got, ref, net_g, net_e)


# ---------------------------------------------------------------------------------------------------------------- 9
def test_operand_build_during_a_capture_raises(gpu_device, graphs):
    """a ChebConv warmed up on one edge_index object, called inside a hand-made capture with another of the same shape: the cache misses and
    the layer refuses to build (a Python exception; the capture ends cleanly and the device stays usable)"""
    edge_a = graphs[0].nonzero().t().contiguous().cuda()
    edge_b = edge_a.clone()
    torch.manual_seed(3)
    net = EdgeNet().cuda()
    x = torch.randn(6, 160, device="cuda")
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            want = net(x, edge_a)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(_lib.TgcnError, match="built by a warm-up step on the same graph arguments"):
            with torch.cuda.graph(graph):
                twice = x * 2.0          # the capture holds a node of its own
                net(twice, edge_b)
        assert not torch.cuda.is_current_stream_capturing()
        del graph
        torch.cuda.synchronize()
        assert torch.equal(net(x, edge_a), want)
        assert torch.equal(net(x, edge_b), want)      # outside a capture the same call builds its operand as before
