"""Streaming time windows of multi-channel series: TGCNCheb_H.forward_series / ChebTimeConv.forward_series / F.cheb_time_windows on a
(S, n, T, f) series, in both output layouts, against the fp64 oracle run on the host-materialised windowed batch
xw[s*nwin + w, i, h, c] = series[s, i, w + h, c] (outputs O.tgcn_cheb_h_forward / O.cheb_time_conv_forward, gradients O.layer_backward folded
back onto the series).  Tolerances: outputs 1e-5 (the project's TOL), gradients 2e-5 (TOL_GRAD / TOL_WINDOWS)."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cheb_oracle as O
from test_hip_parity import _random_graph

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]
TOL = 1e-5
TOL_GRAD = 2e-5

# (n, S, T, H, f, g, K)
CASES = [(148, 2, 60, 15, 4, 32, 10),      # aligned rows, HCP window
         (300, 3, 33, 7, 3, 8, 3),         # unaligned f
         (784, 1, 40, 12, 8, 15, 5),       # g not a multiple of 16
         (500, 1, 20, 20, 2, 5, 4),        # T == H: one window
         (64, 2, 16, 5, 32, 70, 1),        # K = 1, wide f, g > 64
         (90, 2, 24, 6, 5, 12, 25)]        # Chebyshev mode, deep K
CASE_IDS = ["n%d_S%d_T%d_H%d_f%d_g%d_K%d" % c for c in CASES]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _windows(series, H):
    """the windowed batch xw[s*nwin + w, i, h, c] = series[s, i, w + h, c]"""
    S, n, T, f = series.shape
    nwin = T - H + 1
    return np.stack([series[:, :, w:w + H] for w in range(nwin)], axis=1).reshape(S * nwin, n, H, f)


def _fold(gxw, S, T):
    """d series from the gradient of the windowed batch: every window adds into the time rows it was cut from"""
    _, n, H, f = gxw.shape
    nwin = T - H + 1
    gxw = gxw.reshape(S, nwin, n, H, f)
    gs = np.zeros((S, n, T, f))
    for w in range(nwin):
        gs[:, :, w:w + H] += gxw[:, w]
    return gs


def _to_series(a, S, nwin):
    """(S*nwin, n, g) -> (S, n, nwin, g)"""
    return a.reshape((S, nwin) + a.shape[1:]).transpose(0, 2, 1, 3)


class _Setup:
    """One class on one graph: the layer, the two HIP entries under test (stream: forward_series; batch: the layer on materialised windows)
    and the fp64 references."""

    def __init__(self, cls, kind, n, f, g, K, H, seed):
        import tgcn_amd
        from tgcn_amd import functional as F
        rng = np.random.default_rng(seed)
        row, col, val = _random_graph(n, 6, rng, hubs=((2, min(60, n - 1)),))
        val = val * 0.4
        torch.manual_seed(seed)
        self.cls = cls
        if cls == "TGCNCheb_H":
            self.L = O.coo_to_csr(row, col, val, n)
            op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val))
            if kind is not None:
                op = op.reordered(kind)
            self.layer = layer = tgcn_amd.TGCNCheb_H(op, f, g, K, H).cuda()
            self.mode = "power"
            self.stream = lambda s, as_series=False: layer.forward_series(s, as_series=as_series)
            self.batch = lambda xw: layer(xw)
            self.ref_forward = lambda xw: O.tgcn_cheb_h_forward(self.L, xw, self.W64(), layer.bias.detach().cpu().numpy())
            self.bias_grad = lambda go: go.astype(np.float64).sum(axis=0, keepdims=True)
        else:
            ei = np.stack([row, col]).astype(np.int64)
            ew = (0.4 * rng.uniform(0.5, 1.5, row.shape[0])).astype(np.float32) if cls == "ChebTimeConv_w" else None
            r, c, lap = O.edge_laplacian(ei, ew, n)
            self.L = O.coo_to_csr(r, c, lap, n)
            self.layer = layer = tgcn_amd.ChebTimeConv(f, g, K, H).cuda()
            self.mode = "chebyshev"
            eid, ewd = _dev(ei), (None if ew is None else _dev(ew))
            if kind is None:
                self.stream = lambda s, as_series=False: layer.forward_series(s, eid, ewd, as_series=as_series)
                self.batch = lambda xw: layer(xw, eid, ewd)
            else:       # the module builds its own operand from the edge list: the reordered one goes through the functional entry
                op = layer._operand(torch.empty(1, n, 1, device="cuda"), eid, ewd).reordered(kind)
                self.stream = lambda s, as_series=False: F.cheb_time_windows(op, s, layer.weight, layer.bias, F.BIAS_CHANNEL, F.MODE_CHEBYSHEV,
                                                                             as_series=as_series)
                self.batch = lambda xw: F.cheb_layer(op, xw.reshape(xw.shape[0], n, H * f), layer.weight.reshape(K, H * f, g), layer.bias,
                                                     F.BIAS_CHANNEL, F.MODE_CHEBYSHEV)
            self.ref_forward = lambda xw: O.cheb_time_conv_forward(xw, ei, ew, self.W64(), layer.bias.detach().cpu().numpy())
            self.bias_grad = lambda go: go.astype(np.float64).sum(axis=(0, 1))

    def W64(self):
        return self.layer.weight.detach().cpu().numpy()


def _grads(setup, series, go, as_series):
    """(out, d series, dW, db) of one streaming forward + backward; go in the layout of the output"""
    setup.layer.zero_grad()
    st = _dev(series).requires_grad_(True)
    out = setup.stream(st, as_series)
    out.backward(_dev(go))
    return out.detach(), st.grad.cpu().numpy(), setup.layer.weight.grad.cpu().numpy().copy(), setup.layer.bias.grad.cpu().numpy().copy()


@pytest.mark.parametrize("kind", [None, "degree"], ids=["plain", "degree"])
@pytest.mark.parametrize("cls", ["TGCNCheb_H", "ChebTimeConv", "ChebTimeConv_w"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_series_channels_vs_oracle(case, cls, kind, gpu_device):
    n, S, T, H, f, g, K = case
    nwin = T - H + 1
    su = _Setup(cls, kind, n, f, g, K, H, seed=n + T)
    rng = np.random.default_rng([n, T, f])
    series = rng.standard_normal((S, n, T, f)).astype(np.float32)
    xw = _windows(series, H)
    ref = su.ref_forward(xw)
    go = rng.standard_normal((S * nwin, n, g)).astype(np.float32)
    gxw, gW = O.layer_backward(su.L, xw, su.W64(), go, su.mode)
    gs, gb = _fold(gxw, S, T), su.bias_grad(go)

    out, ds, dW, db = _grads(su, series, go, False)
    errs = dict(out=rel_err(out.cpu().numpy(), ref), ds=rel_err(ds, gs), dW=rel_err(dW, gW), db=rel_err(db.reshape(gb.shape), gb))
    print("window-major", errs)
    assert tuple(out.shape) == (S * nwin, n, g)
    assert errs["out"] <= TOL, errs
    assert max(errs["ds"], errs["dW"], errs["db"]) <= TOL_GRAD, errs

    # the series layout: the same numbers, and the same gradients through it
    out_s, ds_s, dW_s, db_s = _grads(su, series, np.ascontiguousarray(_to_series(go, S, nwin)), True)
    assert tuple(out_s.shape) == (S, n, nwin, g) and out_s.is_contiguous()
    assert torch.equal(out_s, out.view(S, nwin, n, g).permute(0, 2, 1, 3))
    errs_s = dict(ds=rel_err(ds_s, gs), dW=rel_err(dW_s, gW), db=rel_err(db_s.reshape(gb.shape), gb),
                  ds_vs=rel_err(ds_s, ds), dW_vs=rel_err(dW_s, dW), db_vs=rel_err(db_s, db))
    print("series layout", errs_s)
    assert max(errs_s.values()) <= TOL_GRAD, errs_s

    # determinism of the weight gradient: the same call twice
    _, _, dW2, _ = _grads(su, series, go, False)
    assert np.array_equal(dW2, dW)

    # the layer on the materialised windows (HIP path) agrees with the same reference: the two paths are interchangeable
    with torch.no_grad():
        e = rel_err(su.batch(_dev(xw)).cpu().numpy(), ref)
    print("materialised", e)
    assert e <= TOL, e


@pytest.mark.parametrize("S,n,T,H", [(2, 148, 20, 6), (1, 300, 9, 9)])
def test_single_channel_4d_series_is_the_3d_call(S, n, T, H, gpu_device):
    """(S, n, T, 1) with as_series=False takes the single-channel path: bit-equal to the 3-D call"""
    su = _Setup("TGCNCheb_H", None, n, 1, 8, 3, H, seed=n)
    series = _dev(np.random.default_rng(n).standard_normal((S, n, T)).astype(np.float32))
    with torch.no_grad():
        a, b = su.stream(series), su.stream(series.unsqueeze(3))
        c = su.stream(series, True)
    assert torch.equal(a, b)
    ref = su.ref_forward(_windows(series.unsqueeze(3).cpu().numpy(), H))
    assert rel_err(a.cpu().numpy(), ref) <= TOL
    assert rel_err(c.cpu().numpy(), _to_series(ref, S, T - H + 1)) <= TOL      # f = 1 in the series layout: the multi-channel kernels


def test_two_layer_chain_vs_oracle(gpu_device):
    """l2.forward_series(relu(l1.forward_series(x, as_series=True))) against the oracle on twice-materialised windows: output and all
    five gradients (series, both weights, both biases)."""
    import tgcn_amd
    n, S, T = 148, 2, 30
    rng = np.random.default_rng(77)
    row, col, val = _random_graph(n, 6, rng, hubs=((2, 60),))
    val = val * 0.4
    L = O.coo_to_csr(row, col, val, n)
    op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val))
    torch.manual_seed(7)
    l1 = tgcn_amd.TGCNCheb_H(op, 1, 8, 4, 5).cuda()
    l2 = tgcn_amd.TGCNCheb_H(op, 8, 16, 3, 4).cuda()
    H1, H2 = 5, 4
    T1 = T - H1 + 1                   # length of the hidden series
    nwin2 = T1 - H2 + 1
    series = rng.standard_normal((S, n, T)).astype(np.float32)
    W1, b1 = l1.weight.detach().cpu().numpy(), l1.bias.detach().cpu().numpy()
    W2, b2 = l2.weight.detach().cpu().numpy(), l2.bias.detach().cpu().numpy()
    # oracle, forward
    xw1 = _windows(series[..., None].astype(np.float64), H1)                              # (S*T1, n, H1, 1)
    pre = O.tgcn_cheb_h_forward(L.astype(np.float64), xw1, W1.astype(np.float64), b1.astype(np.float64)).astype(np.float64)
    hid = _to_series(np.maximum(pre, 0), S, T1)                                            # (S, n, T1, 8)
    xw2 = _windows(hid, H2)
    ref = O.tgcn_cheb_h_forward(L.astype(np.float64), xw2, W2.astype(np.float64), b2.astype(np.float64))
    # oracle, backward
    go = rng.standard_normal(ref.shape).astype(np.float32)
    gxw2, gW2 = O.layer_backward(L, xw2, W2, go, "power")
    gb2 = go.astype(np.float64).sum(axis=0, keepdims=True)
    ghid = _fold(gxw2, S, T1) * (hid > 0)                                                  # (S, n, T1, 8)
    gpre = np.ascontiguousarray(ghid.transpose(0, 2, 1, 3)).reshape(S * T1, n, 8)
    gxw1, gW1 = O.layer_backward(L, xw1, W1, gpre, "power")
    gb1 = gpre.sum(axis=0, keepdims=True)
    gs = _fold(gxw1, S, T)[..., 0]
    # HIP path
    st = _dev(series).requires_grad_(True)
    h = torch.relu(l1.forward_series(st, as_series=True))
    assert tuple(h.shape) == (S, n, T1, 8)
    out = l2.forward_series(h)
    assert tuple(out.shape) == (S * nwin2, n, 16)
    out.backward(_dev(go))
    errs = dict(out=rel_err(out.detach().cpu().numpy(), ref), ds=rel_err(st.grad.cpu().numpy(), gs),
                dW1=rel_err(l1.weight.grad.cpu().numpy(), gW1), db1=rel_err(l1.bias.grad.cpu().numpy(), gb1),
                dW2=rel_err(l2.weight.grad.cpu().numpy(), gW2), db2=rel_err(l2.bias.grad.cpu().numpy(), gb2))
    print(errs)
    assert errs.pop("out") <= TOL
    assert max(errs.values()) <= TOL_GRAD, errs


def test_series_backward_past_the_weight_gradient_block_cap(gpu_device):
    """TGCNCheb_H(L, 4, 32, 3, 15).forward_series on one 40-step recording of the 90 k-vertex mesh: 26 windows x 90 k vertices = 2.34 M rows,
    past the 1024 row blocks of 64 rows of the weight gradient (each block sums ~2300 rows).  The reference is O.windows_backward per
    input channel: the layer is a sum over its input channels."""
    import tgcn_amd
    from tools import synth
    from test_backward_at_scale import _host_L, THREADS
    n, row, col, val = synth.sheet_mesh(300, device=gpu_device)
    op = tgcn_amd.GraphOperand.from_coo(n, row, col, val, gpu_device)
    S, T, H, f, N, K = 1, 40, 15, 4, 32, 3
    nwin = T - H + 1
    assert S * nwin * n > 1024 * 64
    torch.manual_seed(1)
    layer = tgcn_amd.TGCNCheb_H(op, f, N, K, H).cuda()
    gen = torch.Generator(device="cuda").manual_seed(0)
    series = torch.randn((S, n, T, f), device="cuda", generator=gen).requires_grad_(True)
    out = layer.forward_series(series)
    go = torch.randn(out.shape, device="cuda", generator=gen)
    out.backward(go)
    del out
    L = _host_L(op)
    W = layer.weight.detach().cpu().numpy()
    rs, rW = np.zeros((S, n, T, f)), np.zeros((K, H, f, N))
    for c in range(f):
        rs[..., c], rW[:, :, c] = O.windows_backward(L, series.detach()[..., c].cpu().numpy(), W[:, :, c], go.cpu().numpy(), "power", threads=THREADS)
    ref_b = go.double().sum(dim=0, keepdim=True).cpu().numpy()
    errs = dict(ds=rel_err(series.grad.cpu().numpy(), rs), dW=rel_err(layer.weight.grad.cpu().numpy(), rW),
                dWk=max(rel_err(layer.weight.grad[k].cpu().numpy(), rW[k]) for k in range(K)),
                db=rel_err(layer.bias.grad.cpu().numpy(), ref_b))
    print(errs)
    assert max(errs.values()) <= TOL_GRAD, errs
