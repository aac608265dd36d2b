"""Dropout between relu and the pool of the streaming layers' fused epilogue (cheb_series_relu_dropout_pool / cheb_relu_dropout_pool,
DESIGN.md 3.10 "dropout in the relu + pool epilogue"), against the composition a caller writes by hand with the numpy mask of
tests/test_dropout_mask.py: y = forward_series(...), t = relu(y) * m, z = ReluPoolFn(t).

Both classes, S = 2, K = 3, H = 3, T = 40 (38 windows: two window blocks, the second ragged), n = 48 at pool 2 and 4 and n = 50 at pool 2
(waves without a vertex in the last quad), f in {one channel as a 3-D series, 3, 4}, N in {8, 40} (40: columns past N in the last tile;
both are multiples of 4 -- the quad-shared Philox -- so N = 5 and 9 run the per-element form), with the layer's bias (per vertex for
TGCNCheb_H, per channel for ChebTimeConv) and without, three geometries, both layouts, p in {0.1, 0.5}.

  1. z and the three gradients are torch.equal to the composition's.  (One channel, window-major, default geometry: forward_series runs
     the scalar-load form there, whose sums have another order; the unfused layer of that one case is ChebSeriesFn -- Case.composition.)
  2. the as_series=True result is the permuted window-major result for the same seed.
  3. a reordered operand: torch.equal to the composition on ITS unfused output with the same mask, and within 1e-5 of the plain operand.
  4. seeds: the same seed twice, seed=None twice, torch.manual_seed before each.
  5. training=False and p=0 are cheb_series_relu_pool.
  6. a NaN and a +Inf in the series come out where the composition puts them; a dropped +Inf is NaN.
  7. the batch layers: cheb_relu_dropout_pool on GCNCheb and TGCNCheb_H against its composition.
  8. one captured training step replayed twice: two masks, each the composition's for the seed read back.
  9. memory: the peak of the fused forward above the pre-call level stays below the bytes of the unpooled output."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from test_dropout_mask import keep_mask, mask_values, scale_of
from test_series_channels import TOL
from test_series_dilation import CLASSES, K_TERMS, S_REC
from test_series_relu_pool import _layer_on, _series, window_major

gpu = pytest.mark.gpu
pytestmark = [pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]

H_TAPS, T_LEN = 3, 40
# (kwargs, (stride, left, right, dilation)) at H = 3
GEOS = [(dict(), (1, 0, 0, 1)), (dict(stride=2, padding=1), (2, 1, 1, 1)), (dict(padding="causal", dilation=2), (1, 4, 0, 2))]
SEED = (0x2468ACE << 32) | 0x13579BDF          # a key with both halves set


def _nwin(T, H, geo):
    stride, left, right, dil = geo
    return (T + left + right - (H - 1) * dil - 1) // stride + 1


def test_the_shapes_hit_what_they_are_here_for():
    assert _nwin(T_LEN, H_TAPS, GEOS[0][1]) == 38                  # 32 + 6
    assert _nwin(T_LEN, H_TAPS, GEOS[1][1]) == 20 and _nwin(T_LEN, H_TAPS, GEOS[2][1]) == 40          # a step; two phases of 20
    assert 0 < SEED < 2 ** 62 and SEED >> 32 and SEED & 0xFFFFFFFF


class Case:
    """one layer on a random graph of n vertices: the fused call, the unfused layer, with the module's bias or (functional entries) without"""

    def __init__(self, cls, n, f, N, seed):
        from tgcn_amd import functional as F
        self.F, self.cls, self.n = F, cls, n
        self.layer, self.extra = _layer_on(cls, n, f, N, H_TAPS, seed)
        self.mode = F.MODE_POWER if cls == "TGCNCheb_H" else F.MODE_CHEBYSHEV
        probe = torch.empty(1, n, 1, device="cuda")
        self.op = self.layer._operand(probe.device) if cls == "TGCNCheb_H" else self.layer._operand(probe, self.extra[0], None)

    def weight(self, s):
        W = self.layer.weight
        return W if s.dim() == 4 else W.reshape(K_TERMS, W.shape[1], -1)

    def fused(self, s, pool, p, seed, bias=True, op=None, **kw):
        import tgcn_amd
        if bias and op is None:
            return tgcn_amd.cheb_series_relu_dropout_pool(self.layer, s, *self.extra, p=p, pool=pool, seed=seed, **kw)
        b, kind = (self.layer.bias.reshape(-1), self.F.BIAS_VERTEX_CHANNEL if self.cls == "TGCNCheb_H" else self.F.BIAS_CHANNEL) if bias else (None, 0)
        return self.F.cheb_time_windows_relu_dropout_pool(op or self.op, s, self.weight(s), b, kind, self.mode, pool, p, seed, **kw)

    def layer_out(self, s, bias=True, op=None, **kw):
        if bias and op is None:
            return self.layer.forward_series(s, *self.extra, **kw)
        b, kind = (self.layer.bias.reshape(-1), self.F.BIAS_VERTEX_CHANNEL if self.cls == "TGCNCheb_H" else self.F.BIAS_CHANNEL) if bias else (None, 0)
        return self.F.cheb_time_windows(op or self.op, s, self.weight(s), b, kind, self.mode, **kw)

    def composition(self, s, pool, p, seed, as_series, bias=True, op=None, **kw):
        """ReluPoolFn on relu(y) * m: the mask by element index ((s * nwin + w) * n + v) * N + c, whatever the layout of y.
        One channel, window-major, default geometry is the one call forward_series runs in the scalar-load form (ChebWindowsFn), whose
        kernels sum in another order than the MFMA kernels every fused call runs (DESIGN.md 3.10 has the undropped function's figures for
        that row).  There the unfused layer is ChebSeriesFn itself -- the MFMA call forward_series makes for every other argument, and the
        one the library's own unfused route (a reordered operand) makes for this one -- in the same window-major layout, so that the bias
        gradient is the same torch reduction too."""
        if not as_series and s.dim() == 3 and not kw and op is None:
            kind = (self.F.BIAS_VERTEX_CHANNEL if self.cls == "TGCNCheb_H" else self.F.BIAS_CHANNEL) if bias else self.F.BIAS_NONE
            y = self.F.ChebSeriesFn.apply(s.unsqueeze(3), self.layer.weight, self.layer.bias.reshape(-1) if bias else None, self.op, self.mode, kind,
                                          False, (1, 0, 0, 1))
        else:
            y = self.layer_out(s, bias, op, as_series=as_series, **kw)
        if as_series:
            S, n, nwin, N = y.shape
            m = torch.from_numpy(np.ascontiguousarray(mask_values(seed, (S, nwin, n, N), p).transpose(0, 2, 1, 3))).cuda()
            t = torch.relu(y) * m
            return self.F.ReluPoolFn.apply(t.reshape(S, n, nwin * N), pool).view(S, n // pool, nwin, N), y, m
        m = torch.from_numpy(mask_values(seed, tuple(y.shape), p)).cuda()
        return self.F.ReluPoolFn.apply(torch.relu(y) * m, pool), y, m


def _grads(case, x, run):
    """(z, d series, dW, db) of one forward + backward; run(series) -> z; the pooled gradient is drawn from z's shape"""
    case.layer.zero_grad()
    x = x.clone().requires_grad_(True)
    z = run(x)
    gz = torch.randn(z.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(11))
    z.backward(gz)
    g = lambda t: None if t is None else t.clone()
    return z.detach(), x.grad.clone(), g(case.layer.weight.grad), g(case.layer.bias.grad)


def _check_against_the_composition(case, x, pool, tag, ps=(0.1, 0.5), biases=(True, False)):
    for kw, geo in GEOS:
        for p in ps:
            for bias in biases:
                zs = {}
                for as_series in (False, True):
                    got = _grads(case, x, lambda s: case.fused(s, pool, p, SEED, bias, as_series=as_series, **kw))
                    want = _grads(case, x, lambda s: case.composition(s, pool, p, SEED, as_series, bias, **kw)[0])
                    z = got[0]
                    assert (z == 0).any() and (z > 0).any() and not torch.isnan(z).any(), (tag, kw, p, bias)
                    for a, b, what in zip(got, want, ("z", "d series", "dW", "db")):
                        if a is None or b is None:
                            assert a is None and b is None and not bias, (tag, kw, p, bias, as_series, what)      # the functional call without a bias
                            continue
                        assert torch.equal(a, b), (tag, kw, p, bias, as_series, what, float((a - b).abs().max()))
                    zs[as_series] = z
                    with torch.no_grad():           # no arg-max is stored without grad mode; the values do not depend on it
                        assert torch.equal(case.fused(x, pool, p, SEED, bias, as_series=as_series, **kw), z), (tag, kw, p, bias, as_series)
                # 2. one mask for both layouts
                assert torch.equal(window_major(zs[True]), zs[False]), (tag, kw, p, bias)


# ---------------------------------------------------------------------------------------------------------------- 1. / 2. the composition
@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("n,pool", [(48, 2), (48, 4), (50, 2)])
@pytest.mark.parametrize("f", [1, 3, 4])
def test_values_and_gradients_equal_the_composition_bit_for_bit(f, n, pool, cls, gpu_device):
    for N in (8, 40):
        case = Case(cls, n, f, N, seed=f + N + n)
        _check_against_the_composition(case, _series(S_REC, n, T_LEN, f, f + N), pool, (cls, n, pool, f, N))


@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("N", [5, 9])
def test_widths_that_are_no_multiple_of_four_run_one_philox_call_per_element(N, cls, gpu_device):
    case = Case(cls, 48, 4, N, seed=N)
    _check_against_the_composition(case, _series(S_REC, 48, T_LEN, 4, N), 4, (cls, N), ps=(0.5,), biases=(True,))


# ---------------------------------------------------------------------------------------------------------------- 3. reordered operand
@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
def test_a_reordered_operand_drops_the_same_elements(as_series, cls, gpu_device):
    case = Case(cls, 48, 4, 40, seed=9)
    re = case.op.reordered("degree")
    assert re.perm is not None and not case.F.series_pool_is_fused(re)
    x = _series(S_REC, 48, T_LEN, 4, 9)
    for kw, _ in GEOS:
        for pool in (2, 4):
            with torch.no_grad():
                z = case.fused(x, pool, 0.5, SEED, as_series=as_series, **kw)
                z_r = case.fused(x, pool, 0.5, SEED, op=re, as_series=as_series, **kw)
                want_r, _, _ = case.composition(x, pool, 0.5, SEED, as_series, op=re, **kw)
            # the mask of the caller's labels on the reordered operand's own unfused output, bit for bit; the plain operand's values to 1e-5
            assert torch.equal(z_r, want_r), (kw, pool)
            assert rel_err(z_r.cpu().numpy(), z.cpu().numpy()) <= TOL, (kw, pool)
    # and its gradients are the composition's
    got = _grads(case, x, lambda s: case.fused(s, 4, 0.5, SEED, op=re, as_series=as_series))
    want = _grads(case, x, lambda s: case.composition(s, 4, 0.5, SEED, as_series, op=re)[0])
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ---------------------------------------------------------------------------------------------------------------- 4. / 5. seeds, off switches
@gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_seeds_and_off_switches(cls, gpu_device):
    import tgcn_amd
    case = Case(cls, 48, 4, 40, seed=4)
    x = _series(S_REC, 48, T_LEN, 4, 4)
    run = lambda **kw: tgcn_amd.cheb_series_relu_dropout_pool(case.layer, x, *case.extra, **kw)
    with torch.no_grad():
        a, b = run(seed=77, p=0.5), run(seed=77, p=0.5)
        assert torch.equal(a, b) and not torch.equal(a, run(seed=78, p=0.5))
        assert torch.equal(a, run(seed=torch.tensor([77], device="cuda"), p=0.5))
        assert not torch.equal(run(p=0.5), run(p=0.5))                      # seed=None draws
        torch.manual_seed(5)
        c = run(p=0.5)
        torch.manual_seed(5)
        assert torch.equal(c, run(p=0.5))
        # the defaults: p = 0.5, pool = 4, training
        torch.manual_seed(5)
        assert torch.equal(c, run()) and tuple(c.shape) == (S_REC * 38, 12, 40)
        plain = tgcn_amd.cheb_series_relu_pool(case.layer, x, *case.extra)
        assert torch.equal(run(training=False), plain) and torch.equal(run(p=0), plain) and torch.equal(run(p=0.0, seed=3), plain)
        assert not torch.equal(a, plain)
        for kw in (dict(as_series=True), dict(pool=2, stride=2, padding=1)):
            assert torch.equal(run(training=False, **kw), tgcn_amd.cheb_series_relu_pool(case.layer, x, *case.extra, **kw))
    for bad in (dict(p=1.0), dict(p=-0.5), dict(seed=-1), dict(seed=2 ** 62), dict(seed=torch.tensor([1])), dict(seed=torch.tensor([1.0], device="cuda")),
                dict(seed=torch.tensor([1, 2], device="cuda")), dict(pool=3)):
        with pytest.raises(tgcn_amd._lib.TgcnError):
            run(**bad)


# ---------------------------------------------------------------------------------------------------------------- 6. non-finite values
@gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("as_series", [False, True], ids=["window-major", "series"])
def test_nan_and_inf_come_out_where_the_composition_puts_them(as_series, cls, gpu_device):
    case = Case(cls, 48, 4, 40, seed=6)
    x = _series(S_REC, 48, T_LEN, 4, 6)
    x[0, 5, 7, 1] = float("nan")
    x[1, 30, 20, 2] = float("inf")
    with torch.no_grad():
        z = case.fused(x, 4, 0.5, SEED, as_series=as_series)
        want, y, m = case.composition(x, 4, 0.5, SEED, as_series)
    # the case holds what it is here for: a +Inf of the layer's output that the mask drops (0 * Inf = NaN), NaN and finite values
    assert (torch.isposinf(y) & (m == 0)).any() and (torch.isposinf(y) & (m > 0)).any() and torch.isnan(y).any()
    assert torch.isnan(z).any() and torch.isposinf(z).any() and torch.isfinite(z).any()
    assert torch.equal(torch.isnan(z), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(z, nan=-1.0), torch.nan_to_num(want, nan=-1.0))


# ---------------------------------------------------------------------------------------------------------------- 7. batch layers
@gpu
@pytest.mark.parametrize("cls", ["GCNCheb", "TGCNCheb_H"])
@pytest.mark.parametrize("pool", [2, 4])
def test_the_batch_layers_match_their_composition(pool, cls, gpu_device):
    import tgcn_amd
    from tgcn_amd import functional as F
    q, n, N, p = 3, 48, 40, 0.5
    h, _ = _layer_on("TGCNCheb_H", n, 4, N, H_TAPS, seed=7)
    torch.manual_seed(7)
    if cls == "GCNCheb":
        layer = tgcn_amd.GCNCheb(h.L, 4, N, K_TERMS).cuda()
        x = torch.randn(q, n, 4, device="cuda")
    else:
        layer, x = h, torch.randn(q, n, H_TAPS, 4, device="cuda")
    m = torch.from_numpy(mask_values(SEED, (q, n, N), p)).cuda()
    res = []
    for fn in (lambda s: tgcn_amd.cheb_relu_dropout_pool(layer, s, p=p, pool=pool, seed=SEED), lambda s: F.ReluPoolFn.apply(torch.relu(layer(s)) * m, pool)):
        layer.zero_grad()
        xs = x.clone().requires_grad_(True)
        z = fn(xs)
        z.backward(torch.randn(z.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(pool)))
        res.append((z.detach(), xs.grad.clone(), layer.weight.grad.clone(), layer.bias.grad.clone()))
    assert tuple(res[0][0].shape) == (q, n // pool, N) and (res[0][0] == 0).any() and (res[0][0] > 0).any()
    for a, b, what in zip(res[0], res[1], ("z", "dx", "dW", "db")):
        assert torch.equal(a, b), (what, float((a - b).abs().max()))
    with torch.no_grad():
        assert torch.equal(tgcn_amd.cheb_relu_dropout_pool(layer, x, pool=pool, training=False), tgcn_amd.cheb_relu_pool(layer, x, pool=pool))
        assert torch.equal(tgcn_amd.cheb_relu_dropout_pool(layer, x, pool=pool, p=0), tgcn_amd.cheb_relu_pool(layer, x, pool=pool))
    with pytest.raises(tgcn_amd._lib.TgcnError, match=r"p is a real number in \[0, 1\)"):
        tgcn_amd.cheb_relu_dropout_pool(layer, x, p=1)


# ---------------------------------------------------------------------------------------------------------------- 8. capture
@gpu
def test_a_captured_training_step_draws_a_new_mask_on_every_replay(gpu_device):
    """forward + backward with seed=None on one stream, captured once and replayed twice: the seed is drawn inside the graph, so the two z
    differ, and each is the composition's for the seed read back from the tensor the forward kept (z.grad_fn.seed)"""
    import tgcn_amd
    case = Case("TGCNCheb_H", 48, 4, 40, seed=8)
    x = _series(S_REC, 48, T_LEN, 4, 8).requires_grad_(True)
    gz = torch.randn(S_REC * 38, 12, 40, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))

    def step():
        case.layer.zero_grad(set_to_none=True)
        x.grad = None
        z = tgcn_amd.cheb_series_relu_dropout_pool(case.layer, x, p=0.5)
        z.backward(gz)
        return z, z.grad_fn.seed

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        z, seed_t = step()
    seen = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        seed = int(seed_t)
        assert 0 <= seed < 2 ** 62
        seen.append((seed, z.detach().clone(), x.grad.clone(), case.layer.weight.grad.clone()))
    assert seen[0][0] != seen[1][0] and not torch.equal(seen[0][1], seen[1][1])
    for seed, zr, dx, dW in seen:
        want = _grads_with(case, x.detach(), gz, lambda s: case.composition(s, 4, 0.5, seed, False)[0])
        assert torch.equal(zr, want[0]) and torch.equal(dx, want[1]) and torch.equal(dW, want[2])


def _grads_with(case, x, gz, run):
    case.layer.zero_grad()
    x = x.clone().requires_grad_(True)
    z = run(x)
    z.backward(gz)
    return z.detach(), x.grad.clone(), case.layer.weight.grad.clone()


# ---------------------------------------------------------------------------------------------------------------- 9. memory
@gpu
def test_the_unpooled_output_is_never_allocated_in_training(gpu_device):
    """a condition, not a timing: S = 2, n = 48, T = 66, one channel into N = 40 at pool 4 in grad mode.  The unpooled output is
    2 * 48 * 64 * 40 floats = 983 040 bytes; the fused forward holds the stack (3 * 2 * 48 * 66 floats = 76 KB), the series' aligned copy, z
    (245 KB), the arg-max bytes (61 KB), the working weight and the seed -- about 0.4 MB"""
    import tgcn_amd
    S, n, T, N, pool = 2, 48, 66, 40, 4
    case = Case("TGCNCheb_H", n, 1, N, seed=10)
    x = _series(S, n, T, 1, 10).requires_grad_(True)
    unpooled = S * n * (T - H_TAPS + 1) * N * 4
    assert unpooled == 983040
    z = tgcn_amd.cheb_series_relu_dropout_pool(case.layer, x, p=0.1, pool=pool)          # builds the operand and the cached workspaces
    del z
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    z = tgcn_amd.cheb_series_relu_dropout_pool(case.layer, x, p=0.1, pool=pool)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak above the pre-call level: %d bytes; unpooled output: %d bytes" % (peak, unpooled))
    assert z.requires_grad and tuple(z.shape) == (S * (T - H_TAPS + 1), n // pool, N)
    assert peak < unpooled, (peak, unpooled)


def test_the_numpy_mask_helpers_agree():
    """CPU: mask_values is keep_mask on the flat index, scaled"""
    m = mask_values(SEED, (2, 3, 5), 0.5)
    keep = keep_mask(SEED, np.arange(30), 0.5).reshape(2, 3, 5)
    assert m.dtype == np.float32 and np.array_equal(m != 0, keep) and set(np.unique(m)) <= {0.0, scale_of(0.5)}
