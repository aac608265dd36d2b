"""The training-scale gradient references of oracle/cheb_oracle.py (layer_backward_gside, windows_backward) against O.layer_backward,
which tests/golden pins to the reference's own autograd: CPU only, small random non-symmetric graphs, both recursions."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import cheb_oracle as O


def _graph(n, rng, deg=4, scale=0.3):
    """Non-symmetric: independent random (row, col) pairs, a hub row and an empty row; values scaled so K = 25 stays bounded."""
    m = n * deg
    row = np.concatenate([rng.integers(0, n, m), np.full(n // 2, 1)])
    col = np.concatenate([rng.integers(0, n, m), rng.integers(0, n, n // 2)])
    keep = row != 3
    val = rng.standard_normal(keep.sum()) * scale / np.sqrt(deg)
    L = O.coo_to_csr(row[keep], col[keep], val, n)
    assert abs(L - L.T).max() > 0
    return L


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 5, 25])
@pytest.mark.parametrize("mode", ["power", "chebyshev"])
def test_layer_backward_gside_matches_layer_backward(mode, K, threads):
    rng = np.random.default_rng(10 * K + (mode == "power"))
    n, q, H, f, g = 37, 3, 4, 2, 5
    L = _graph(n, rng)
    x = rng.standard_normal((q, n, H, f))
    W = rng.standard_normal((K, H, f, g))
    go = rng.standard_normal((q, n, g))
    gx, gW = O.layer_backward(L, x, W, go, mode)
    hx, hW = O.layer_backward_gside(L, x, W, go, mode, threads=threads)
    assert hx.shape == x.shape and hW.shape == W.shape
    assert rel_err(hx, gx) <= 1e-12
    for k in range(K):                      # every term on its own scale
        assert rel_err(hW[k], gW[k]) <= 1e-12, k


@pytest.mark.parametrize("K,H,T", [(1, 3, 7), (2, 1, 5), (5, 4, 9), (25, 3, 6), (4, 6, 6)])
@pytest.mark.parametrize("mode", ["power", "chebyshev"])
def test_windows_backward_matches_layer_backward_on_the_windows(mode, K, H, T):
    """windows_backward on the series == layer_backward on the materialised windows, folded back onto the series."""
    rng = np.random.default_rng(100 * K + T + (mode == "power"))
    n, S, g = 23, 2, 3
    L = _graph(n, rng)
    series = rng.standard_normal((S, n, T))
    W = rng.standard_normal((K, H, g))
    nwin = T - H + 1
    go = rng.standard_normal((S * nwin, n, g))
    xw = np.stack([series[s, :, w:w + H] for s in range(S) for w in range(nwin)])          # (S*nwin, n, H)
    gxw, gW = O.layer_backward(L, xw[..., None], W[:, :, None, :], go, mode)
    gs = np.zeros_like(series)
    for s in range(S):
        for w in range(nwin):
            gs[s, :, w:w + H] += gxw[s * nwin + w, :, :, 0]
    hs, hW = O.windows_backward(L, series, W, go, mode, threads=2)
    assert hs.shape == series.shape and hW.shape == W.shape
    assert rel_err(hs, gs) <= 1e-12
    for k in range(K):
        assert rel_err(hW[k], gW[k, :, 0]) <= 1e-12, k
