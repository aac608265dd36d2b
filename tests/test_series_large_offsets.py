"""The streaming time-window kernels on tensors beyond 2^31 and 2^32 elements: hop stacks, outputs in both layouts, pooled outputs with their
arg-max bytes, input gradients, weight gradients and rings, through the C ABI and through the modules.

The method is PERIODIC DATA.  A fp64 reference of 4 G elements is not affordable and sampled rows would miss a wrapped range, so the big
problem is a tiling of a small one: n = P * m vertices, every big operand built on the device as big[.., s, i, ..] = small[.., i % P, ..]
((s*n + i) % P == i % P), a per-vertex bias b0[i % P].  A wave tile of the sliding-window GEMMs belongs to one (recording, vertex) pair -- a
vertex quad in the pooled form, P % 4 == 0 -- and its arithmetic depends on that row, W and the bias only, so the big call must reproduce the
small call (S = 1, n = P, every other number, leading dimension and alignment the same: the same instantiation, the same HC) BIT FOR BIT at
every element.  The whole big output, NaN-filled before the call, is compared on the device slab by slab as integers; the small call is
compared with fp64 numpy on the materialised windows (tests/test_series_dilation.py's helpers and bounds: outputs 1e-5, gradients 2e-5 of the
tensor's maximum; bf16 outputs by tests/test_series_stream_bf16.py's two rules).  Together: a high-precision reference for every element.

A wrapped offset (by 2^31 or 2^32 elements) must not land on identical data: neither is a whole multiple of P * row length -- P = 1020 has
odd factors -- which the CPU tests assert for every shape, with which tensor passes which line, that the guards admit the shape, and that a
test's tensors stay under 64 GB.

Sums over all rows (weight and bias gradients) are not periodic bit for bit, and a tiled fp32 sum of 10^8 coherent terms drifts past the
bound by rounding alone.  Their output gradient has SPARSE SUPPORT: zero except on the first and last 1024 (s, i) rows and 512 rows on each
side of every row where the stack's or g's element offset crosses a multiple of 2^31; the fp64 reference is the small problem's at g
accumulated onto g_small[i % P].  A wrapped offset turns contributions into zeros or foreign rows.

Not run here: the one-launch small-graph step (its operands fit LDS), the distributed layers, the scalar-load form (one recording per launch)
and the pooled stream entry with a device position."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from conftest import rel_err
from test_bf16_layers import EMUL_ULPS, bf
from test_series_channels import TOL, TOL_GRAD
from test_series_dilation import fold_dilated, nwin_of, windows_dilated

gpu = pytest.mark.gpu
BF = torch.bfloat16
ULP_BOUND = EMUL_ULPS * 2.0 ** -8

P = 1020                   # the period: P % 4 == 0 (vertex quads, pool groups), odd factors 3 * 5 * 17 (no power of two is a multiple)
S_BIG, M_TILES = 2, 2060
N_BIG = P * M_TILES        # 2,101,200 vertices; S * n = 4,202,400 rows
SN = S_BIG * N_BIG
LINE31, LINE32 = 2 ** 31, 2 ** 32
BUDGET = 64 * 10 ** 9      # bytes of device memory a test's tensors may sum to
SLAB = 1 << 28             # elements compared per step


def case(name, entry, dt="f32", T=130, f=4, H=2, N=4, K=2, stride=1, pl=0, pr=0, d=1, as_series=1, pool=0, bias_kind=2, crosses=None, **kw):
    c = types.SimpleNamespace(name=name, entry=entry, dt=dt, T=T, f=f, H=H, N=N, K=K, stride=stride, pl=pl, pr=pr, d=d, as_series=as_series,
                              pool=pool, bias_kind=bias_kind, crosses=crosses or {}, **kw)
    c.Tf = T * f
    c.nwin = (T + pl + pr - ((H - 1) * d + 1)) // stride + 1
    c.esize = 2 if dt == "bf16" else 4
    return c


# 1. the hop stack (K, S, n, T*f) past 2^32 elements; N = 4 with a per-vertex bias, the output past 2^31 where the windows are many
STACK = [
    case("series-f4", "series", crosses={"stack": LINE32, "out": LINE31}),
    case("conv-step2-pads", "conv", H=3, stride=2, pl=1, pr=1, as_series=0, crosses={"stack": LINE32}),
    case("dilated3-causal", "dilated", H=3, d=3, pl=6, crosses={"stack": LINE32, "out": LINE31}),
    case("series-f3-scalar-staging", "series", T=174, f=3, as_series=0, crosses={"stack": LINE32, "out": LINE31}),
    case("conv-bf16", "conv", dt="bf16", T=65, f=8, H=3, stride=2, pl=1, pr=1, crosses={"stack": LINE32}),
    case("dilated-bf16", "dilated", dt="bf16", T=65, f=8, H=3, d=3, pl=6, as_series=0, crosses={"stack": LINE32}),
]
# 2. the output past 2^32 in both layouts: K = 1, f = 1, 32 windows, N = 33 (NT = 4 with a ragged last column tile)
_wide = dict(T=33, f=1, H=2, N=33, K=1, bias_kind=1)
OUTPUT = [
    case("out-series-f32", "series", as_series=1, crosses={"out": LINE32}, **_wide),
    case("out-windows-f32", "series", as_series=0, crosses={"out": LINE32, "window stride": LINE31}, **_wide),
    case("out-series-bf16", "conv", dt="bf16", as_series=1, crosses={"out": LINE32}, **_wide),
    case("out-windows-bf16", "conv", dt="bf16", as_series=0, crosses={"out": LINE32, "window stride": LINE31}, **_wide),
]
# 3. pooled output z and its arg-max bytes past 2^32: N = 64, one tap pair, few windows
POOLED = [
    case("pool4-series", "pool", T=65, H=2, N=64, K=1, pool=4, as_series=1, crosses={"z": LINE32}),
    case("pool2-windows", "pool", T=33, H=2, N=64, K=1, pool=2, as_series=0, crosses={"z": LINE32}),
]
# 4. the input gradient G (K, S, n, T*f) past 2^32 (dW = NULL): the column-group stride o_gs = S*n*Tf; a step of 3 > H = 2 is the memset path
INPUT_GRAD = [
    case("G-plain", "series", crosses={"G": LINE32, "g": LINE31}),
    case("G-conv-step3-over-H", "conv", H=2, stride=3, pl=1, pr=1, as_series=0, crosses={"G": LINE32}),
    case("G-dilated3", "dilated", H=3, d=3, pl=6, as_series=0, crosses={"G": LINE32, "g": LINE31}),
    case("G-conv-step3-bf16", "conv", dt="bf16", T=65, f=8, H=2, N=8, stride=3, pl=1, pr=1, crosses={"G": LINE32}),
    case("G-dilated3-bf16", "dilated", dt="bf16", T=65, f=8, H=3, N=8, d=3, pl=6, as_series=0, crosses={"G": LINE32}),
]
# 5. the weight gradient (G = NULL) with a stack past 2^32 and a g past 2^31, sparse-support g as a series
WEIGHT_GRAD = [
    case("W-plain", "series", crosses={"stack": LINE32, "g": LINE31}),
    case("W-conv-step2-pads", "conv", H=3, N=8, stride=2, pl=1, pr=1, crosses={"stack": LINE32, "g": LINE31}),
    case("W-dilated3", "dilated", H=3, d=3, pl=6, crosses={"stack": LINE32, "g": LINE31}),
    case("W-conv-bf16", "conv", dt="bf16", T=65, f=8, H=3, N=16, stride=2, pl=1, pr=1, crosses={"stack": LINE32, "g": LINE31}),
    case("W-dilated3-bf16", "dilated", dt="bf16", T=65, f=8, H=3, N=8, d=3, pl=6, crosses={"stack": LINE32, "g": LINE31}),
]
# 6. the ring (K, S, n, ring_ld) past 2^32: C*f = 512, a chunk of 16 rows at a nonzero head; the window step at dilation 1 with H = 129.
# A chunk shorter than the dilation makes 16 one-window phase tiles per vertex row: 16.8 M workgroups of 256, a grid past 2^32 THREADS, which
# the runtime does not run whole in one launch: the launchers issue it in parts ("Grids in parts").
_ring = dict(T=16, N=4, K=2, bias_kind=1)
_threads = {"ring": LINE32, "grid threads": LINE32}
RING = [
    case("stream-f32", "stream", H=3, d=64, crosses=_threads, **_ring),
    case("stream-pos-f32", "stream_pos", H=3, d=64, crosses=_threads, **_ring),
    case("stream-bf16", "stream", dt="bf16", f=8, H=3, d=32, crosses=_threads, **_ring),
    case("stream-strided-f32", "stream_strided", H=129, d=1, step=2, win_off=1, crosses={"ring": LINE32}, **_ring),
    case("stream-pos-bf16", "stream_pos", dt="bf16", f=8, H=3, d=32, crosses=_threads, **_ring),
    case("stream-strided-bf16", "stream_strided", dt="bf16", f=8, H=65, d=1, step=2, win_off=1, crosses={"ring": LINE32}, **_ring),
    case("stream-pool4-f32", "stream_pool", H=3, d=64, pool=4, crosses=_threads, **_ring),
    # the _at entry writes the chunk's rows [57, 73) into an output of 130 time rows, 2.19 G elements, in either layout
    case("stream-at-series-f32", "stream_at", H=3, d=64, out_T=130, t0=57, crosses=dict(_threads, out=LINE31), **_ring),
    case("stream-at-windows-f32", "stream_at", H=3, d=64, out_T=130, t0=57, as_series=0, crosses=dict(_threads, out=LINE31), **_ring),
]
# 6b. the chunk backward: the whole output gradient g (S, n, 130, N) past 2^31 read in place from row 57 on (the second tap's rows run past
# its end), G of the chunk bitwise (periodic g, no ring); dW with the carried ring (K, S, n, 512) past 2^32 and a sparse-support g
CHUNK = [
    case("chunk-backward-series", "chunk", H=3, d=64, out_T=130, t0=57, crosses={"ring": LINE32, "g": LINE31}, **_ring),
    case("chunk-backward-windows", "chunk", H=3, d=64, out_T=130, t0=57, as_series=0, crosses={"ring": LINE32, "g": LINE31}, **_ring),
]
FORWARD = STACK + OUTPUT + POOLED


def ids(cases):
    return dict(argvalues=cases, ids=[c.name for c in cases])


def ring_slots(c):
    return (c.H - 1) * c.d


for _c in RING + CHUNK:
    _c.head = ring_slots(_c) - 8          # nonzero, and the chunk's 16 rows wrap round the ring's end


def stream_windows(c):
    """windows that end inside the chunk: every row, or every step-th from win_off on"""
    return (c.T - c.win_off - 1) // c.step + 1 if c.entry == "stream_strided" else c.T


# ---------------------------------------------------------------------------------------------------------------- plain integer arithmetic
def tensors_of(c, group):
    """name -> (elements, bytes per element, row length) of every big tensor a test of this case holds"""
    rows = SN // c.pool if c.pool else SN
    t = {}
    if group in ("forward", "wgrad"):
        t["stack"] = (c.K * SN * c.Tf, c.esize, c.Tf)
    if group == "forward":
        t["z" if c.pool else "out"] = (rows * c.nwin * c.N, c.esize, c.nwin * c.N if c.as_series else c.N)
        if c.pool:
            t["idx"] = (rows * c.nwin * c.N, 1, c.nwin * c.N if c.as_series else c.N)
        if c.bias_kind == 2:
            t["bias"] = (N_BIG * c.N, c.esize, c.N)
    if group in ("igrad", "wgrad"):
        t["g"] = (SN * c.nwin * c.N, c.esize, c.nwin * c.N if c.as_series else c.N)
    if group == "igrad":
        t["G"] = (c.K * SN * c.Tf, 4, c.Tf)
    if group == "ring":
        Cf = ring_slots(c) * c.f
        t["ring"] = (c.K * SN * Cf, c.esize, Cf)
        t["stack"] = (c.K * SN * c.Tf, c.esize, c.Tf)
        rows_out = c.out_T if c.entry == "stream_at" else stream_windows(c)
        t["out"] = ((SN // c.pool if c.pool else SN) * rows_out * c.N, c.esize, rows_out * c.N if c.as_series else c.N)
    if group == "chunk":
        Cf = ring_slots(c) * c.f
        t.update(ring=(c.K * SN * Cf, 4, Cf), stack=(c.K * SN * c.Tf, 4, c.Tf), G=(c.K * SN * c.Tf, 4, c.Tf),
                 g=(SN * c.out_T * c.N, 4, c.out_T * c.N if c.as_series else c.N))
    return t


def workspace_bytes(c, S, n):
    """the backward workspace query of the case's geometry: 0 where series_geom refuses the shape (it needs no device)"""
    from tgcn_amd import _lib
    L = _lib.lib()
    dims = (S, n, c.T, c.f, c.H, c.N, c.K)
    if c.entry.startswith("stream") or c.entry == "chunk":
        return L.tgcn_cheb_series_chunk_backward_workspace_bytes(*dims, c.d)
    if c.entry == "series":
        return L.tgcn_cheb_series_backward_workspace_bytes(*dims)
    sfx = "_bf16" if c.dt == "bf16" else ""
    if c.entry == "conv":
        return getattr(L, "tgcn_cheb_series_conv_backward%s_workspace_bytes" % sfx)(*dims, c.stride, c.pl, c.pr)
    return getattr(L, "tgcn_cheb_series_dilated_backward%s_workspace_bytes" % sfx)(*dims, c.stride, c.pl, c.pr, c.d)


def plan(c, H, f, N, stride):
    """(rc, hc, lds) of the launch planner for the case's element type; dilated launches are planned as step 1"""
    from tgcn_amd import _lib
    L = _lib.lib()
    hc, lds = C.c_int32(-1), C.c_int32(-1)
    if c.dt == "bf16":
        rc = L.tgcn_series_conv_plan_bf16(H, f, N, int(f % 8 == 0), stride, C.byref(hc), C.byref(lds))
    elif c.pool:
        rc = L.tgcn_series_pool_plan(H, f, N, int(f % 4 == 0), stride, c.pool, C.byref(hc), C.byref(lds))
    else:
        rc = L.tgcn_series_conv_plan(H, f, N, int(f % 4 == 0), stride, C.byref(hc), C.byref(lds))
    return rc, hc.value, lds.value


def grid_x(c, nwin, d=1):
    """series_launch_plan's workgroups: wave tiles of 32 windows (phase-major with a dilation), four per workgroup; pooled: one per quad"""
    tpv = -(-nwin // 32) if d == 1 else min(d, nwin) * -(-((nwin - 1) // d + 1) // 32)
    return S_BIG * -(-N_BIG // 4) * tpv if c.pool else -(-(SN * tpv) // 4)


def wgrad_rows_per_block(M, weight_floats):
    """series_wgrad_rows_per_block in tgcn_hip.hip: at most 1024 row blocks of at least 64 rows, a multiple of 16; partials held to 256 MB"""
    rpb = (max((M + 1023) // 1024, 64) + 15) // 16 * 16
    most = max((256 << 20) // (weight_floats * 4), 1)
    if -(-M // rpb) > most:
        rpb = (-(-M // most) + 15) // 16 * 16
    return rpb


def wgrad_plan(c):
    """(M, rows per block, blocks), the block count read back from the workspace query: flipped weight slot + one weight per block"""
    wf = c.K * c.H * c.f * c.N
    M = SN * c.nwin
    rpb = wgrad_rows_per_block(M, wf)
    blocks = (workspace_bytes(c, S_BIG, N_BIG) - (wf * 4 + 255) // 256 * 256) // (wf * 4)
    return M, rpb, blocks


def sparse_rows(c):
    """the (s, i) rows of the sparse-support g: the first and last 1024 and 512 on each side of every row in which the element offset of the
    stack (any term) or of g crosses a multiple of 2^31"""
    rows = [np.arange(1024), np.arange(SN - 1024, SN)]
    cross = []
    for j in range(1, (c.K * SN * c.Tf) // LINE31 + 1):          # stack: row r of term k starts at (k*S*n + r) * Tf
        r = j * LINE31 // c.Tf
        cross.append(r % SN)
    for j in range(1, (SN * c.nwin * c.N) // LINE31 + 1):        # g as a series: row r starts at r * nwin * N
        cross.append(j * LINE31 // (c.nwin * c.N))
    for r in cross:
        rows.append(np.arange(max(r - 512, 0), min(r + 512, SN)))
    return np.unique(np.concatenate(rows)), cross


def chunk_sparse_rows(c):
    """sparse_rows for the chunk backward: the crossings of the ring (K, S, n, C*f) and of the whole output gradient as a series"""
    Cf = ring_slots(c) * c.f
    cross = [(j * LINE31 // Cf) % SN for j in range(1, c.K * SN * Cf // LINE31 + 1)]
    cross += [j * LINE31 // (c.out_T * c.N) for j in range(1, SN * c.out_T * c.N // LINE31 + 1)]
    rows = [np.arange(1024), np.arange(SN - 1024, SN)] + [np.arange(max(r - 512, 0), min(r + 512, SN)) for r in cross]
    return np.unique(np.concatenate(rows)), cross


GROUPS = [("forward", FORWARD), ("igrad", INPUT_GRAD), ("wgrad", WEIGHT_GRAD), ("ring", RING), ("chunk", CHUNK)]
ALL = [(g, c) for g, cases in GROUPS for c in cases]
ALL_IDS = dict(argvalues=ALL, ids=["%s-%s" % (g, c.name) for g, c in ALL])


@pytest.mark.parametrize("group,c", **ALL_IDS)
def test_each_shape_crosses_the_line_it_names(group, c):
    t = tensors_of(c, group)
    assert c.crosses, "every case is here for a line"
    for name, line in c.crosses.items():
        if name == "window stride":          # window-major output: the last window's offset w * n * N alone
            assert not c.as_series and (c.nwin - 1) * N_BIG * c.N > line
            continue
        if name == "grid threads":           # workgroups of 256 along x: more than one launch holds
            assert grid_x(c, stream_windows(c), c.d) * 256 > line
            continue
        assert t[name][0] > line, (c.name, name, t[name][0], line)
        if name == "z":
            assert t["idx"][0] > line
    assert N_BIG % P == 0 and S_BIG >= 2 and (not c.pool or (P % 4 == 0 and N_BIG % c.pool == 0))
    if group in ("ring", "chunk"):
        assert 0 < c.head < ring_slots(c) and c.T < ring_slots(c) and ring_slots(c) * c.f == 512
        assert c.head + c.T > ring_slots(c)          # the chunk's rows wrap round the ring's end


@pytest.mark.parametrize("group,c", **ALL_IDS)
def test_a_wrapped_offset_lands_on_other_data(group, c):
    """neither 2^31 nor 2^32 elements is a whole multiple of the period of any big tensor, P rows of its row length"""
    for name, (numel, esize, row) in tensors_of(c, group).items():
        for line in (LINE31, LINE32):
            assert line % (P * row) != 0, (c.name, name, row)


@pytest.mark.parametrize("group,c", **ALL_IDS)
def test_the_guards_admit_each_shape(group, c):
    """series_geom / series_stream_check through the workspace queries, the LDS plans, and the grid limits in plain integers"""
    assert workspace_bytes(c, S_BIG, N_BIG) > 0 and workspace_bytes(c, 1, P) > 0
    lim = 2 ** 31 - 1
    if group == "chunk":       # the GEMM over g (H weight time rows of N channels, K*f columns, phase-major tiles) and the weight gradient's rows
        rc, hc, lds = plan(c, c.H, c.N, c.K * c.f, 1)
        assert rc == 0 and hc == c.H and grid_x(c, c.T, c.d) <= lim and 0 <= c.t0 and c.t0 + c.T <= c.out_T
        assert c.t0 + c.d < c.out_T < c.t0 + c.T + c.d        # the middle tap's rows of g run past its end, the first tap's lie wholly past it
        rows, cross = chunk_sparse_rows(c)
        assert len(cross) >= 3 and 2048 < len(rows) < 16384
    if group == "ring":
        stride = c.step if c.entry == "stream_strided" else 1
        small = plan(c, c.H, c.f, c.N, stride)
        assert small[0] == 0 and small[1] == c.H
        assert grid_x(c, stream_windows(c), c.d) <= lim and ring_slots(c) * c.f < lim
    elif group in ("forward", "wgrad"):
        rc, hc, lds = plan(c, c.H, c.f, c.N, c.stride)
        assert rc == 0 and hc == c.H and lds <= 64 * 1024, (rc, hc, lds)
        assert grid_x(c, c.nwin, c.d) <= lim
    if group == "igrad":       # the GEMM over g: ceil(H / stride) weight time rows of N channels, K*f columns, step 1
        rc, hc, lds = plan(c, -(-c.H // c.stride), c.N, c.K * c.f, 1)
        assert rc == 0 and lds <= 64 * 1024
        assert grid_x(c, c.T, c.d) <= lim
    if group == "wgrad":
        M, rpb, blocks = wgrad_plan(c)
        print(c.name, "M = %d rows, %d rows per block, %d blocks" % (M, rpb, blocks))
        # the library's own block count bounds its rows per block from below, whatever rule made it: blocks * rpb >= M
        assert blocks == -(-M // rpb) and -(-M // blocks) > 65536, (M, rpb, blocks)
        assert rpb + c.nwin < lim and rpb // c.nwin + N_BIG < lim
        rows, cross = sparse_rows(c)
        assert len(cross) >= 3 and 2048 < len(rows) < 16384


@pytest.mark.parametrize("group,c", **ALL_IDS)
def test_each_test_stays_under_its_memory_budget(group, c):
    assert device_bytes(c, group) < BUDGET


def device_bytes(c, group):
    """the tensors of the case, the workspace, and the comparison's temporaries (a slab of flags and of counts)"""
    ws = workspace_bytes(c, S_BIG, N_BIG) if group in ("igrad", "wgrad", "chunk") else 0
    return sum(numel * esize for numel, esize, _ in tensors_of(c, group).values()) + ws + 10 * SLAB + (1 << 30)


# ---------------------------------------------------------------------------------------------------------------- device helpers
def need(c, group):
    """skip, with the figure, where the device has less free memory than the case's tensors take"""
    free = torch.cuda.mem_get_info()[0]
    want = device_bytes(c, group)
    if free < want:
        pytest.skip("%s needs %.1f GB of free device memory, %.1f GB are free" % (c.name, want / 1e9, free / 1e9))


def release():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def torch_dt(c):
    return BF if c.dt == "bf16" else torch.float32


def bits(t):
    return t if t.dtype == torch.uint8 else t.view(torch.int16 if t.dtype == BF else torch.int32)


def rows_view(big, small, lead=0):
    """(lead.., S, n, row..) and (lead.., 1, p, row..) -> views (lead.., S*m, p, L) and (lead.., 1, p, L) that broadcast: vertex i of any
    recording is i % p (p = P, or P / pool for a pooled output); the dimensions behind the vertex are one row of L elements"""
    shape, period = tuple(big.shape[:lead]), small.shape[lead + 1]
    L = big[(0,) * (lead + 2)].numel()
    assert small.shape[lead] == 1 and big.shape[lead + 1] % period == 0 and small[(0,) * (lead + 2)].numel() == L and tuple(small.shape[:lead]) == shape
    return big.view(shape + (-1, period, L)), small.reshape(shape + (1, period, L))


def windows_view(big, small, S, nwin):
    """window-major (S*nwin, n, N) and (nwin, p, N) -> (S, nwin, m, p, N) and (1, nwin, 1, p, N)"""
    period, N = small.shape[-2], big.shape[-1]
    return big.view(S, nwin, -1, period, N), small.view(1, nwin, 1, period, N)


def tile_into(view, small):
    view.copy_(small.expand_as(view))


def tiled_rows(small, S, n):
    """small (K, 1, P, L) -> big (K, S, n, L), made on the device"""
    big = torch.empty((small.shape[0], S, n, small.shape[3]), dtype=small.dtype, device=small.device)
    tile_into(*rows_view(big, small, 1))
    return big


def mismatches(big, small):
    """how many elements of big differ, as bits, from small broadcast over it: counted on the device, one slab of SLAB elements at a time"""
    big, small = bits(big), bits(small).expand_as(big)
    d = max(range(big.dim()), key=lambda a: big.shape[a])
    step = max(1, SLAB // (big.numel() // big.shape[d]))
    bad = torch.zeros((), dtype=torch.int64, device=big.device)
    for a in range(0, big.shape[d], step):
        b = min(step, big.shape[d] - a)
        bad += (big.narrow(d, a, b) != small.narrow(d, a, b)).sum()
    return int(bad)


def test_the_tiling_and_the_comparison_on_a_toy():
    """the helpers every GPU test rests on, on the CPU: tile, compare as bits, count one flipped element, in both layouts"""
    torch.manual_seed(0)
    small = torch.randn(2, 1, 6, 5)
    big = tiled_rows(small, 3, 24)
    assert all(torch.equal(big[:, s, 6 * j:6 * j + 6], small[:, 0]) for s in range(3) for j in range(4))
    assert mismatches(*rows_view(big, small, 1)) == 0
    big[1, 2, 17, 3] = float("nan")
    assert mismatches(*rows_view(big, small, 1)) == 1
    out_small = torch.randn(1, 6, 7, 2).to(BF)              # as a series (S, n, nwin, N)
    out = torch.empty(3, 24, 7, 2, dtype=BF)
    tile_into(*rows_view(out, out_small))
    assert torch.equal(out[2, 18:24], out_small[0]) and mismatches(*rows_view(out, out_small)) == 0
    win_small = torch.randn(7, 6, 2)                        # window-major (S*nwin, n, N)
    win = torch.empty(3 * 7, 24, 2)
    tile_into(*windows_view(win, win_small, 3, 7))
    assert torch.equal(win.view(3, 7, 24, 2)[1, :, 12:18], win_small) and mismatches(*windows_view(win, win_small, 3, 7)) == 0
    win[20, 23, 1] += 1
    assert mismatches(*windows_view(win, win_small, 3, 7)) == 1


def nan_filled(shape, dt):
    return torch.full(shape, 255, dtype=dt, device="cuda") if dt == torch.uint8 else torch.full(shape, float("nan"), dtype=dt, device="cuda")


def np64(t):
    return t.detach().double().cpu().numpy()


def operands(c, seed, device="cuda"):
    """the small problem's stack (K, 1, P, T*f), weight (K, H*f, N) and bias ([N] or per vertex [P*N]) in the case's element type"""
    gen = torch.Generator(device=device).manual_seed(seed)
    dt = torch_dt(c)
    stack = torch.randn((c.K, 1, P, c.Tf), device=device, generator=gen).to(dt)
    W = (torch.randn((c.K, c.H * c.f, c.N), device=device, generator=gen) * 0.5).to(dt)
    bias = torch.randn((P * c.N if c.bias_kind == 2 else c.N,), device=device, generator=gen).to(dt)
    return stack, W, bias, gen


def big_bias(c, bias):
    return bias.view(1, -1).expand(M_TILES, -1).contiguous().view(-1) if c.bias_kind == 2 else bias


# ---------------------------------------------------------------------------------------------------------------- fp64 on the small problem
def small_windows(c, stack):
    """(K, nwin, P, H, f) fp64: the materialised windows of the small stack, by test_series_dilation's rule, every stride-th of them"""
    x = np64(stack).reshape(c.K, P, c.T, c.f)
    xw = windows_dilated(x, c.H, c.d, c.pl, c.pr).reshape(c.K, nwin_of(c.T, c.H, c.d, c.pl, c.pr), P, c.H, c.f)[:, ::c.stride]
    assert xw.shape[1] == c.nwin
    return xw


def out64(c, xw, W, bias):
    """window-major (nwin, P, N)"""
    ref = np.einsum("kwihc,khcn->win", xw, np64(W).reshape(c.K, c.H, c.f, c.N))
    b = np64(bias)
    return ref + (b.reshape(1, P, c.N) if c.bias_kind == 2 else b)


def check_small_output(c, got_windows_major, ref, what="out"):
    """fp32: 1e-5 of the maximum.  bf16: within EMUL_ULPS ulps of the fp64 result rounded once, and twice that emulation's own error"""
    gv = np64(got_windows_major)
    if c.dt == "bf16":
        emu = bf(ref)
        d_emu, e64, tol = float(np.abs(gv - emu).max() / np.abs(emu).max()), rel_err(gv, ref), 2 * rel_err(emu, ref)
        print(c.name, what, "vs emulation %.2e (bound %.2e) vs fp64 %.2e (bound %.2e)" % (d_emu, ULP_BOUND, e64, tol))
        assert d_emu <= ULP_BOUND and e64 <= tol, (d_emu, e64, tol)
    else:
        e = rel_err(gv, ref)
        print(c.name, what, "vs fp64 %.2e" % e)
        assert e <= TOL, e


def weight_grad64(c, xw, g_rows):
    """(K, H*f, N) from the windows and g as (P, nwin, N)"""
    return np.einsum("kwihc,iwn->khcn", xw, g_rows).reshape(c.K, c.H * c.f, c.N)


@pytest.mark.parametrize("c", **ids(INPUT_GRAD + WEIGHT_GRAD))
def test_the_three_fp64_references_are_one_bilinear_form(c):
    """<out(x, W), g> = <x, G(g, W)> = <W, dW(x, g)> on the case's geometry: a slip in the window rule of one reference shows here, on the CPU"""
    stack, W, bias, gen = operands(c, 3, "cpu")
    g = np.random.default_rng(5).standard_normal((c.nwin, P, c.N))
    xw = small_windows(c, stack)
    y = np.einsum("kwihc,khcn->win", xw, np64(W).reshape(c.K, c.H, c.f, c.N))
    a = (y * g).sum()
    b = (np64(stack).reshape(c.K, P, c.Tf) * input_grad64(c, g, W)).sum()
    d = (np64(W) * weight_grad64(c, xw, g.transpose(1, 0, 2))).sum()
    assert abs(a - b) <= 1e-9 * abs(a) and abs(a - d) <= 1e-9 * abs(a), (a, b, d)


# ---------------------------------------------------------------------------------------------------------------- 1 - 3: the forward entries
def call_forward(c, S, n, stack, W, bias, out, idx=None):
    from tgcn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    dims = (_lib.stream_ptr(), S, n, c.T, c.f, c.H, c.N, c.K, p(stack))
    if c.dt == "bf16":
        args = dims + (c.Tf, p(W), p(bias), _lib.DTYPE_BF16, c.bias_kind, c.as_series, p(out), c.stride, c.pl, c.pr)
        rc = L.tgcn_cheb_project_series_conv_bf16(*args) if c.entry == "conv" else L.tgcn_cheb_project_series_dilated_bf16(*args, c.d)
    else:
        args = dims + (p(W), p(bias), c.bias_kind, c.as_series)
        if c.entry == "series":
            rc = L.tgcn_cheb_project_series_f32(*args, p(out))
        elif c.entry == "conv":
            rc = L.tgcn_cheb_project_series_conv_f32(*args, p(out), c.stride, c.pl, c.pr)
        elif c.entry == "dilated":
            rc = L.tgcn_cheb_project_series_dilated_f32(*args, p(out), c.stride, c.pl, c.pr, c.d)
        else:
            rc = L.tgcn_cheb_project_series_pool_f32(*args, p(out), p(idx), c.pool, c.stride, c.pl, c.pr, c.d)
    _lib.check(rc)


def out_shape(c, S, n):
    n = n // c.pool if c.pool else n
    return (S, n, c.nwin, c.N) if c.as_series else (S * c.nwin, n, c.N)


def out_views(c, big, small):
    return rows_view(big, small) if c.as_series else windows_view(big, small, S_BIG, c.nwin)


def windows_major(c, small):
    return small[0].permute(1, 0, 2) if c.as_series else small


@gpu
@pytest.mark.parametrize("c", **ids(FORWARD))
def test_forward_entry_on_a_tiled_problem_equals_the_small_call_bit_for_bit(c, gpu_device):
    need(c, "forward")
    dt = torch_dt(c)
    stack, W, bias, _ = operands(c, 11)
    small = nan_filled(out_shape(c, 1, P), dt)
    small_idx = nan_filled(out_shape(c, 1, P), torch.uint8) if c.pool else None
    call_forward(c, 1, P, stack, W, bias, small, small_idx)
    assert not torch.isnan(small).any()
    ref = out64(c, small_windows(c, stack), W, bias)
    if c.pool:       # relu + max over `pool` consecutive vertices; the stored offset names a member that attains it
        y = np.maximum(ref, 0.0).reshape(c.nwin, P // c.pool, c.pool, c.N)
        check_small_output(c, windows_major(c, small), y.max(axis=2), "z")
        at = np.take_along_axis(y, np64(windows_major(c, small_idx)).astype(np.int64)[:, :, None, :], axis=2)[:, :, 0]
        assert small_idx.max() < c.pool and rel_err(at, y.max(axis=2)) <= TOL
    else:
        check_small_output(c, windows_major(c, small), ref)
    big_stack = tiled_rows(stack, S_BIG, N_BIG)
    bb = big_bias(c, bias)
    out = nan_filled(out_shape(c, S_BIG, N_BIG), dt)
    idx = nan_filled(out_shape(c, S_BIG, N_BIG), torch.uint8) if c.pool else None
    call_forward(c, S_BIG, N_BIG, big_stack, W, bb, out, idx)
    bad = mismatches(*out_views(c, out, small))
    bad_idx = mismatches(*out_views(c, idx, small_idx)) if c.pool else 0
    print(c.name, "stack %.3f G elements, output %.3f G elements, %d + %d mismatches" % (big_stack.numel() / 1e9, out.numel() / 1e9, bad, bad_idx))
    del big_stack, out, idx, bb
    release()
    assert bad == 0 and bad_idx == 0, (bad, bad_idx)


# ---------------------------------------------------------------------------------------------------------------- 4, 5: the backward entries
def call_backward(c, S, n, stack, g, W, G, dW):
    from tgcn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    nbytes = workspace_bytes(c, S, n)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dims = (_lib.stream_ptr(), S, n, c.T, c.f, c.H, c.N, c.K, p(stack))
    if c.dt == "bf16":
        args = dims + (c.Tf, p(g), c.as_series, p(W), p(G), p(dW), p(ws), nbytes, c.stride, c.pl, c.pr)
        rc = L.tgcn_cheb_series_conv_backward_bf16(*args) if c.entry == "conv" else L.tgcn_cheb_series_dilated_backward_bf16(*args, c.d)
    else:
        args = dims + (p(g), c.as_series, p(W), p(G), p(dW), p(ws), nbytes)
        if c.entry == "series":
            rc = L.tgcn_cheb_series_backward_f32(*args)
        elif c.entry == "conv":
            rc = L.tgcn_cheb_series_conv_backward_f32(*args, c.stride, c.pl, c.pr)
        else:
            rc = L.tgcn_cheb_series_dilated_backward_f32(*args, c.stride, c.pl, c.pr, c.d)
    _lib.check(rc)
    torch.cuda.synchronize()       # the workspace is freed on return


def input_grad64(c, g_windows_major, W):
    """(K, P, T*f): every tap's product folded back onto the time row it was read from, the padding rows dropped"""
    gxw = np.einsum("win,khcn->kwihc", g_windows_major, np64(W).reshape(c.K, c.H, c.f, c.N))
    nwin1 = nwin_of(c.T, c.H, c.d, c.pl, c.pr)
    full = np.zeros((c.K, nwin1, P, c.H, c.f))
    full[:, ::c.stride] = gxw
    return fold_dilated(full.reshape(c.K * nwin1, P, c.H, c.f), c.K, c.T, c.d, c.pl, c.pr).reshape(c.K, P, c.Tf)


@gpu
@pytest.mark.parametrize("c", **ids(INPUT_GRAD))
def test_input_gradient_past_2_32_equals_the_small_call_bit_for_bit(c, gpu_device):
    need(c, "igrad")
    dt = torch_dt(c)
    _, W, _, gen = operands(c, 12)
    g_small = torch.randn(out_shape(c, 1, P), device="cuda", generator=gen).to(dt)
    G_small = nan_filled((c.K, 1, P, c.Tf), torch.float32)
    call_backward(c, 1, P, None, g_small, W, G_small, None)
    assert not torch.isnan(G_small).any()
    e = rel_err(np64(G_small).reshape(c.K, P, c.Tf), input_grad64(c, np64(windows_major(c, g_small)), W))
    print(c.name, "small G vs fp64 %.2e" % e)
    assert e <= TOL_GRAD, e
    g = torch.empty(out_shape(c, S_BIG, N_BIG), dtype=dt, device="cuda")
    tile_into(*out_views(c, g, g_small))
    G = nan_filled((c.K, S_BIG, N_BIG, c.Tf), torch.float32)
    call_backward(c, S_BIG, N_BIG, None, g, W, G, None)
    bad = mismatches(*rows_view(G, G_small, 1))
    print(c.name, "G %.3f G elements, g %.3f G elements, %d mismatches" % (G.numel() / 1e9, g.numel() / 1e9, bad))
    del g, G
    release()
    assert bad == 0, bad


@gpu
@pytest.mark.parametrize("c", **ids(WEIGHT_GRAD))
def test_weight_gradient_of_a_stack_past_2_32_vs_fp64(c, gpu_device):
    need(c, "wgrad")
    dt = torch_dt(c)
    stack, W, _, gen = operands(c, 13)
    M, rpb, blocks = wgrad_plan(c)
    print(c.name, "M = %d rows, %d rows per block, %d blocks" % (M, rpb, blocks))
    assert -(-M // blocks) > 65536          # from the library's block count alone: blocks * rows per block >= M
    rows, _ = sparse_rows(c)
    vals = torch.randn((len(rows), c.nwin * c.N), device="cuda", generator=gen).to(dt)
    g = torch.zeros((S_BIG, N_BIG, c.nwin, c.N), dtype=dt, device="cuda")
    g.view(SN, c.nwin * c.N)[torch.as_tensor(rows, device="cuda")] = vals
    big_stack = tiled_rows(stack, S_BIG, N_BIG)
    dW = nan_filled((c.K, c.H * c.f, c.N), torch.float32)
    call_backward(c, S_BIG, N_BIG, big_stack, g, None, None, dW)
    got = np64(dW)
    del g, big_stack
    release()
    # the small problem's reference at g accumulated in fp64 onto its vertex i % P
    g_small = np.zeros((P, c.nwin * c.N))
    np.add.at(g_small, rows % P, np64(vals))
    ref = weight_grad64(c, small_windows(c, stack), g_small.reshape(P, c.nwin, c.N))
    e = rel_err(got, ref)
    print(c.name, "dW vs fp64 %.2e over %d rows with a gradient" % (e, len(rows)))
    assert not np.isnan(got).any() and e <= TOL_GRAD, e


# ---------------------------------------------------------------------------------------------------------------- 6: the ring
def call_stream(c, S, n, stack, W, bias, out, ring, pos):
    from tgcn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    ring_ld = ring_slots(c) * c.f
    dims = (_lib.stream_ptr(), S, n, c.T, c.f, c.H, c.N, c.K, p(stack))
    if c.dt == "bf16":
        mid = (c.Tf, p(W), p(bias), _lib.DTYPE_BF16, c.bias_kind, p(out), p(ring), ring_ld)
        if c.entry == "stream":
            rc = L.tgcn_cheb_project_series_stream_bf16(*dims, *mid, c.head, c.d)
        elif c.entry == "stream_pos":
            rc = L.tgcn_cheb_project_series_stream_pos_bf16(*dims, *mid, p(pos), c.d)
        else:
            rc = L.tgcn_cheb_project_series_stream_strided_bf16(*dims, *mid, c.head, None, c.step, c.win_off)
    elif c.entry == "stream":
        rc = L.tgcn_cheb_project_series_stream_f32(*dims, p(W), p(bias), c.bias_kind, p(out), p(ring), ring_ld, c.head, c.d)
    elif c.entry == "stream_pos":
        rc = L.tgcn_cheb_project_series_stream_pos_f32(*dims, p(W), p(bias), c.bias_kind, p(out), p(ring), ring_ld, p(pos), c.d)
    elif c.entry == "stream_pool":
        rc = L.tgcn_cheb_project_series_stream_pool_f32(*dims, p(W), p(bias), c.bias_kind, p(out), c.pool, p(ring), ring_ld, c.head, None, c.d)
    elif c.entry == "stream_at":
        rc = L.tgcn_cheb_project_series_stream_at_f32(*dims, p(W), p(bias), c.bias_kind, p(out), c.out_T, c.t0, c.as_series, p(ring), ring_ld, c.head, c.d)
    else:
        rc = L.tgcn_cheb_project_series_stream_strided_f32(*dims, p(W), p(bias), c.bias_kind, p(out), p(ring), ring_ld, c.head, None, c.step, c.win_off)
    _lib.check(rc)


def stream_out_shape(c, S, n):
    if c.entry == "stream_at":
        return (S, n, c.out_T, c.N) if c.as_series else (S * c.out_T, n, c.N)
    return (S, n // c.pool if c.pool else n, stream_windows(c), c.N)


def past_and_chunk(c, ring0, stack):
    """fp64 (K, P, C + Tc, f): the C rows before the chunk in time order (row t < 0 is slot (head + t + C) mod C), then the chunk"""
    Cr = ring_slots(c)
    past = np64(ring0).reshape(c.K, P, Cr, c.f)[:, :, [(c.head + j) % Cr for j in range(Cr)]]
    return np.concatenate([past, np64(stack).reshape(c.K, P, c.T, c.f)], axis=2)


def updated_ring(c, ring0, stack):
    """the ring update on the small problem: chunk row j to slot (head + j) mod C"""
    Cr = ring_slots(c)
    want = ring0.clone().view(c.K, 1, P, Cr, c.f)
    for j in range(max(0, c.T - Cr), c.T):
        want[:, :, :, (c.head + j) % Cr] = stack.view(c.K, 1, P, c.T, c.f)[:, :, :, j]
    return want.view_as(ring0)


@gpu
@pytest.mark.parametrize("c", **ids(RING))
def test_stream_entry_on_a_ring_past_2_32_equals_the_small_call_bit_for_bit(c, gpu_device):
    need(c, "ring")
    dt = torch_dt(c)
    Cr, seen = ring_slots(c), 5 * ring_slots(c) + c.head
    stack, W, bias, gen = operands(c, 14)
    ring0 = torch.randn((c.K, 1, P, Cr * c.f), device="cuda", generator=gen).to(dt)
    ring_small = ring0.clone()
    small = nan_filled(stream_out_shape(c, 1, P), dt)
    pos = torch.tensor([c.head, seen], dtype=torch.int64, device="cuda") if c.entry == "stream_pos" else None
    call_stream(c, 1, P, stack, W, bias, small, ring_small, pos)
    # fp64 on the windows that end in the chunk
    xw = windows_dilated(past_and_chunk(c, ring0, stack), c.H, c.d, 0, 0).reshape(c.K, c.T, P, c.H, c.f)
    if c.entry == "stream_strided":
        xw = xw[:, c.win_off::c.step]
    ref = out64(c, xw, W, bias)
    if c.entry == "stream_at":       # the chunk's rows of the whole output; every other row keeps its NaN
        whole = small[0].permute(1, 0, 2) if c.as_series else small
        got = whole[c.t0:c.t0 + c.T]
        assert torch.isnan(whole[:c.t0]).all() and torch.isnan(whole[c.t0 + c.T:]).all()
    else:
        got = small[0].permute(1, 0, 2)
    if c.pool:
        ref = np.maximum(ref, 0.0).reshape(ref.shape[0], P // c.pool, c.pool, c.N).max(axis=2)
    assert not torch.isnan(got).any()
    check_small_output(c, got, ref)
    assert torch.equal(ring_small, updated_ring(c, ring0, stack))
    if pos is not None:
        assert pos.tolist() == [(c.head + c.T) % Cr, seen + c.T]
        pos = torch.tensor([c.head, seen], dtype=torch.int64, device="cuda")
    ring = tiled_rows(ring0, S_BIG, N_BIG)
    big_stack = tiled_rows(stack, S_BIG, N_BIG)
    out = nan_filled(stream_out_shape(c, S_BIG, N_BIG), dt)
    call_stream(c, S_BIG, N_BIG, big_stack, W, bias, out, ring, pos)
    views = windows_view(out, small, S_BIG, c.out_T) if c.entry == "stream_at" and not c.as_series else rows_view(out, small)
    bad_out, bad_ring = mismatches(*views), mismatches(*rows_view(ring, ring_small, 1))
    print(c.name, "ring %.3f G elements, output %.3f G, %d mismatches in the output, %d in the updated ring"
          % (ring.numel() / 1e9, out.numel() / 1e9, bad_out, bad_ring))
    if pos is not None:
        assert pos.tolist() == [(c.head + c.T) % Cr, seen + c.T]
    del ring, big_stack, out
    release()
    assert bad_out == 0 and bad_ring == 0, (bad_out, bad_ring)


def call_chunk_backward(c, S, n, stack, ring, g, W, G, dW):
    from tgcn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    nbytes = workspace_bytes(c, S, n)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(L.tgcn_cheb_series_chunk_backward_f32(_lib.stream_ptr(), S, n, c.T, c.f, c.H, c.N, c.K, p(stack), p(ring), ring_slots(c) * c.f,
                                                     c.head if ring is not None else 0, p(g), c.out_T, c.t0, c.as_series, p(W), p(G), p(dW), p(ws), nbytes,
                                                     c.d))
    torch.cuda.synchronize()


def g_shape(c, S, n):
    return (S, n, c.out_T, c.N) if c.as_series else (S * c.out_T, n, c.N)


@gpu
@pytest.mark.parametrize("c", **ids(CHUNK))
def test_chunk_backward_input_gradient_from_a_g_past_2_31_bit_for_bit(c, gpu_device):
    """G of the chunk from the whole periodic output gradient, no ring: chunk row u sums g[t0 + u + (H-1-h)*d] W[h]^T over the rows that exist"""
    need(c, "chunk")
    _, W, _, gen = operands(c, 15)
    g_small = torch.randn(g_shape(c, 1, P), device="cuda", generator=gen)
    G_small = nan_filled((c.K, 1, P, c.Tf), torch.float32)
    call_chunk_backward(c, 1, P, None, None, g_small, W, G_small, None)
    gs = np64(g_small[0].permute(1, 0, 2) if c.as_series else g_small)           # (out_T, P, N)
    W64 = np64(W).reshape(c.K, c.H, c.f, c.N)
    ref = np.zeros((c.K, P, c.T, c.f))
    for h in range(c.H):
        for u in range(c.T):
            t = c.t0 + u + (c.H - 1 - h) * c.d
            if t < c.out_T:
                ref[:, :, u] += np.einsum("in,kcn->kic", gs[t], W64[:, h])
    e = rel_err(np64(G_small).reshape(ref.shape), ref)
    print(c.name, "small G vs fp64 %.2e" % e)
    assert not torch.isnan(G_small).any() and e <= TOL_GRAD, e
    g = torch.empty(g_shape(c, S_BIG, N_BIG), device="cuda")
    tile_into(*(rows_view(g, g_small) if c.as_series else windows_view(g, g_small, S_BIG, c.out_T)))
    G = nan_filled((c.K, S_BIG, N_BIG, c.Tf), torch.float32)
    call_chunk_backward(c, S_BIG, N_BIG, None, None, g, W, G, None)
    bad = mismatches(*rows_view(G, G_small, 1))
    print(c.name, "g %.3f G elements, %d mismatches in G" % (g.numel() / 1e9, bad))
    del g, G
    release()
    assert bad == 0, bad


@gpu
@pytest.mark.parametrize("c", **ids(CHUNK))
def test_chunk_backward_weight_gradient_with_a_ring_past_2_32_vs_fp64(c, gpu_device):
    """the carried weight gradient: windows that end in the chunk, their early rows from the ring; sparse-support g; then the ring update"""
    need(c, "chunk")
    Cr = ring_slots(c)
    stack, W, _, gen = operands(c, 16)
    ring0 = torch.randn((c.K, 1, P, Cr * c.f), device="cuda", generator=gen)
    rows, _ = chunk_sparse_rows(c)
    vals = torch.randn((len(rows), c.out_T, c.N), device="cuda", generator=gen)
    g = torch.zeros(g_shape(c, S_BIG, N_BIG), device="cuda")
    at = torch.as_tensor(rows, device="cuda")
    if c.as_series:
        g.view(SN, c.out_T, c.N)[at] = vals
    else:
        g.view(S_BIG, c.out_T, N_BIG, c.N)[at // N_BIG, :, at % N_BIG] = vals
    ring = tiled_rows(ring0, S_BIG, N_BIG)
    big_stack = tiled_rows(stack, S_BIG, N_BIG)
    dW = nan_filled((c.K, c.H * c.f, c.N), torch.float32)
    call_chunk_backward(c, S_BIG, N_BIG, big_stack, ring, g, None, None, dW)
    got = np64(dW)
    bad_ring = mismatches(*rows_view(ring, updated_ring(c, ring0, stack), 1))
    del g, ring, big_stack
    release()
    g_small = np.zeros((P, c.out_T, c.N))
    np.add.at(g_small, rows % P, np64(vals))
    xw = windows_dilated(past_and_chunk(c, ring0, stack), c.H, c.d, 0, 0).reshape(c.K, c.T, P, c.H, c.f)
    ref = weight_grad64(c, xw, g_small[:, c.t0:c.t0 + c.T])
    e = rel_err(got, ref)
    print(c.name, "dW vs fp64 %.2e over %d rows with a gradient, %d mismatches in the updated ring" % (e, len(rows), bad_ring))
    assert not np.isnan(got).any() and e <= TOL_GRAD and bad_ring == 0, (e, bad_ring)


# ---------------------------------------------------------------------------------------------------------------- the modules, end to end
# m copies of one P-vertex graph at vertex offsets j*P (block-diagonal), so the hops are periodic too: the layers on a periodic series give
# the small layer's fp64 oracle output tiled.  The hop kernel may group the rows of the big graph differently, so this is a comparison to
# rounding (the project's 1e-5 / 2e-5 of the maximum), not bit for bit.
MOD = types.SimpleNamespace(K=3, S=2, m=700, f=4, g=8, H=3, chunks=(40, 24, 64), stream_dilation=64, time_chunk=32)
MOD.n = P * MOD.m
MOD.SN = MOD.S * MOD.n
# Time rows per kind of test, and the one tensor each is here for.  T = 128 puts the hop stack (K, S, n, T*f) and the stream's ring at 2.19 G
# elements.  The chunked layer never holds a whole stack and relabel_rows sees the series and the output only, so those two run at T = 256,
# where the as-series output (and its gradient) holds 2.92 G elements.
MOD_T = dict(train=128, stream=128, pool=128, chunked=256, reordered=256)
MOD_CROSSES = dict(train="stack", stream="ring", pool="stack", chunked="out", reordered="out")


def module_tensors(kind):
    """name -> elements of the big tensors a module test holds at its peak (fp32; the bf16 stream holds half the bytes)"""
    T = MOD_T[kind]
    e = dict(series=MOD.SN * T * MOD.f, out=MOD.SN * T * MOD.g)
    if kind in ("train", "reordered", "pool"):
        e["stack"] = MOD.K * MOD.SN * T * MOD.f
    if kind == "train":          # and the backward: the output gradient, G, the adjoint hops' result and a temporary of its size, d series
        e.update(go=e["out"], G=e["stack"], adjoint=2 * e["stack"], dseries=e["series"])
    if kind == "chunked":        # chunk-sized stacks and G, whole-size output, gradients and series
        per = MOD.K * MOD.SN * MOD.time_chunk * MOD.f
        e.update(go=e["out"], stack=per, G=per, adjoint=2 * per, dseries=e["series"], ring=MOD.K * MOD.SN * (MOD.H - 1) * MOD.f)
    if kind == "reordered":      # the relabelled series and the output before it is relabelled back
        e.update(relabelled=e["series"], out_operand_labels=e["out"])
    if kind == "stream":
        e.update(ring=MOD.K * MOD.SN * (MOD.H - 1) * MOD.stream_dilation * MOD.f, stack=MOD.K * MOD.SN * max(MOD.chunks) * MOD.f)
    if kind == "pool":
        e["out"] //= 4
    if kind == "chunked":
        assert e["go"] == e["out"]
    return e


def test_the_module_shapes_cross_their_lines_and_fit():
    assert sum(MOD.chunks) == MOD_T["stream"] and MOD_T["chunked"] % MOD.time_chunk == 0 and MOD.n % 4 == 0
    for kind, T in MOD_T.items():
        e = module_tensors(kind)
        assert e[MOD_CROSSES[kind]] > LINE31, (kind, MOD_CROSSES[kind], e[MOD_CROSSES[kind]])       # ONE tensor of every test passes 2^31 elements
        assert 4 * sum(e.values()) + (2 << 30) < BUDGET, kind
        for row in (T * MOD.f, T * MOD.g, (MOD.H - 1) * MOD.stream_dilation * MOD.f):
            assert LINE31 % (P * row) != 0 and LINE32 % (P * row) != 0
    for kind in ("train", "chunked"):
        rows, blocks = module_sparse_rows(MOD_T[kind])
        assert 2048 < len(rows) < 8192 and 4 <= len(blocks) <= 12
    # the chunked layer's own tensors stay small -- that is its point; its ring and stack past the line are the C ABI cases of CHUNK
    assert module_tensors("chunked")["stack"] < LINE31 and module_tensors("chunked")["ring"] < LINE31


def module_sparse_rows(T):
    """rows (s*n + i) with an output gradient: the first and last 1024 and 512 on each side of every row in which the element offset of the
    stack (K, S, n, T*f) or of the as-series output gradient (S, n, T, g) crosses a multiple of 2^31; and the P-vertex blocks they touch"""
    rows = [np.arange(1024), np.arange(MOD.SN - 1024, MOD.SN)]
    cross = [(j * LINE31 // (T * MOD.f)) % MOD.SN for j in range(1, MOD.K * MOD.SN * T * MOD.f // LINE31 + 1)]
    cross += [j * LINE31 // (T * MOD.g) for j in range(1, MOD.SN * T * MOD.g // LINE31 + 1)]
    for r in cross:
        rows.append(np.arange(max(r - 512, 0), min(r + 512, MOD.SN)))
    rows = np.unique(np.concatenate(rows))
    return rows, np.unique(rows // P)


@functools.lru_cache(maxsize=None)
def small_problem(cls, T, bf16=False, dilation=1):
    """the P-vertex graph, the parameters, the small series and its fp64 oracle output (T, P, g) window-major, computed once"""
    from oracle import cheb_oracle as O
    from test_series_bf16 import _graph
    from test_series_dilation_bf16 import series_emulate, series_fp64
    L = _graph(P, 77).tocsr()
    rng = np.random.default_rng(78)
    W = (rng.standard_normal((MOD.K, MOD.H, MOD.f, MOD.g)) * 0.3).astype(np.float32)
    series = rng.standard_normal((1, P, T, MOD.f)).astype(np.float32)
    coo = L.tocoo()
    if cls == "TGCNCheb_H":
        b, L_op, mode, ei = rng.uniform(-0.5, 0.5, (1, P, MOD.g)).astype(np.float32), L, "power", None
    else:
        ei = np.stack([coo.row, coo.col]).astype(np.int64)
        row, col, lap = O.edge_laplacian(ei, None, P)
        b, L_op, mode = rng.uniform(-0.5, 0.5, (MOD.g,)).astype(np.float32), O.coo_to_csr(row, col, lap, P), "chebyshev"
    geom = (dilation, (MOD.H - 1) * dilation, 0)
    r = lambda a: bf(a) if bf16 else a.astype(np.float64)
    zero = np.zeros((T, P, MOD.g))
    ref = series_fp64(L_op, r(series), r(W), r(b), zero, mode, geom)[0]
    emu = series_emulate(L_op, r(series), r(W), r(b), zero, mode, geom)[0] if bf16 else None
    return types.SimpleNamespace(cls=cls, T=T, L=L, coo=coo, ei=ei, L_op=L_op, mode=mode, W=W, b=b, series=series, geom=geom, ref=ref, emu=emu)


def small_backward(sp_, go_windows_major):
    """(d series (P, T, f), dW, db) of the small layer in fp64 at one output gradient (T, P, g)"""
    from test_series_dilation_bf16 import series_fp64
    _, gs, gW, gb = series_fp64(sp_.L_op, sp_.series.astype(np.float64), sp_.W.astype(np.float64), sp_.b.astype(np.float64), go_windows_major, sp_.mode,
                                sp_.geom)
    return gs[0], gW, gb


class BigLayer:
    """the layer on the block-diagonal graph with the small problem's parameters (a per-vertex bias tiled), and the periodic series"""

    def __init__(self, sp_, dt=torch.float32):
        import tgcn_amd
        off = (torch.arange(MOD.m, device="cuda", dtype=torch.int64) * P).view(-1, 1)
        row, col = (off + torch.as_tensor(sp_.coo.row.astype(np.int64), device="cuda")).view(-1), (off + torch.as_tensor(sp_.coo.col.astype(np.int64), device="cuda")).view(-1)
        self.sp, self.extra = sp_, ()
        if sp_.cls == "TGCNCheb_H":
            val = torch.as_tensor(sp_.coo.data.astype(np.float32), device="cuda").repeat(MOD.m)
            self.op = tgcn_amd.GraphOperand.from_coo(MOD.n, row, col, val)
            self.layer = tgcn_amd.TGCNCheb_H(self.op, MOD.f, MOD.g, MOD.K, MOD.H).cuda()
            bias = torch.as_tensor(sp_.b, device="cuda").expand(MOD.m, P, MOD.g).reshape(1, MOD.n, MOD.g)
        else:
            self.layer = tgcn_amd.ChebTimeConv(MOD.f, MOD.g, MOD.K, MOD.H).cuda()
            self.extra = (torch.stack([row, col]), None)
            bias = torch.as_tensor(sp_.b, device="cuda")
        with torch.no_grad():
            self.layer.weight.copy_(torch.as_tensor(sp_.W, device="cuda"))
            self.layer.bias.copy_(bias)
        self.layer = self.layer.to(dt)
        self.series = torch.empty((MOD.S, MOD.n, sp_.T, MOD.f), dtype=dt, device="cuda")
        tile_into(*rows_view(self.series, torch.as_tensor(sp_.series, device="cuda").to(dt)))


def tiled_error(big, ref):
    """max |big - ref broadcast| in fp64 on the device, slab by slab; big and ref are views that broadcast (rows_view's)"""
    ref = ref.expand_as(big)
    d = max(range(big.dim()), key=lambda a: big.shape[a])
    step = max(1, (SLAB // 4) // (big.numel() // big.shape[d]))
    worst = torch.zeros((), dtype=torch.float64, device=big.device)
    for a in range(0, big.shape[d], step):
        b = min(step, big.shape[d] - a)
        worst = torch.maximum(worst, (big.narrow(d, a, b).double() - ref.narrow(d, a, b)).abs().max())
    return float(worst)


def series_ref(ref_windows_major, t0=0, t1=None, pool=0):
    """the oracle's (T, P, g) as the series rows (1, P', t1 - t0, g) on the device in fp64; pool: relu + max over 4 consecutive vertices first"""
    y = ref_windows_major
    if pool:
        y = np.maximum(y, 0.0).reshape(y.shape[0], P // pool, pool, y.shape[2]).max(axis=2)
    return torch.as_tensor(np.ascontiguousarray(y.transpose(1, 0, 2)[None, :, t0:t1]), device="cuda")


def check_output(name, out, ref_windows_major, t0=0, t1=None, pool=0, emu=None):
    ref = series_ref(ref_windows_major, t0, t1, pool)
    den = float(ref.abs().max())
    e = tiled_error(*rows_view(out, ref)) / den
    if emu is None:
        print(name, "output %.3f G elements vs the tiled oracle %.2e" % (out.numel() / 1e9, e))
        assert e <= TOL, (name, e)
    else:        # bf16: the two rules of tests/test_series_stream_bf16.py
        em = series_ref(emu, t0, t1)
        d_emu, tol = tiled_error(*rows_view(out, em)) / float(em.abs().max()), 2 * float((em - ref).abs().max()) / den
        print(name, "vs emulation %.2e (bound %.2e) vs fp64 %.2e (bound %.2e)" % (d_emu, ULP_BOUND, e, tol))
        assert d_emu <= ULP_BOUND and e <= tol, (name, d_emu, e, tol)


def module_need(kind, bytes_per=4):
    want = bytes_per * sum(module_tensors(kind).values()) + (2 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < want:
        pytest.skip("the %s test needs %.1f GB of free device memory, %.1f GB are free" % (kind, want / 1e9, free / 1e9))
    torch.cuda.reset_peak_memory_stats()


def train_step(cls, kind, **kw):
    """forward_series(as_series=True, padding="causal") and one backward with the sparse-support output gradient, against the oracle: the
    output tiled, weight.grad and bias.grad at the gradient accumulated onto its vertex i % P, series.grad per touched block and exact
    zeros in every other block"""
    module_need(kind)
    T = MOD_T[kind]
    sp_ = small_problem(cls, T)
    big = BigLayer(sp_)
    series = big.series.requires_grad_(True)
    out = big.layer.forward_series(series, *big.extra, as_series=True, padding="causal", **kw)
    assert tuple(out.shape) == (MOD.S, MOD.n, T, MOD.g) and module_tensors(kind)["out"] == out.numel()
    check_output("%s %s" % (cls, kind), out.detach(), sp_.ref)
    rows, blocks = module_sparse_rows(T)
    gen = torch.Generator(device="cuda").manual_seed(5)
    vals = torch.randn((len(rows), T * MOD.g), device="cuda", generator=gen)
    go = torch.zeros_like(out)
    go.view(MOD.SN, T * MOD.g)[torch.as_tensor(rows, device="cuda")] = vals
    out.backward(go)
    del out, go
    vals = np64(vals).reshape(len(rows), T, MOD.g)
    g_small = np.zeros((P, T, MOD.g))
    np.add.at(g_small, rows % P, vals)
    _, gW, gb = small_backward(sp_, g_small.transpose(1, 0, 2))
    db = np64(big.layer.bias.grad)
    if cls == "TGCNCheb_H":      # a per-vertex bias: the big gradient folded onto vertex i % P
        db = db.reshape(MOD.m, P, MOD.g).sum(axis=0).reshape(gb.shape)
    errs = dict(dW=rel_err(np64(big.layer.weight.grad), gW), db=rel_err(db.reshape(gb.shape), gb))
    grad = series.grad.view(MOD.SN // P, P, T, MOD.f)
    touched = torch.zeros(MOD.SN // P, dtype=torch.bool, device="cuda")
    for a in range(0, MOD.SN // P, 128):
        touched[a:a + 128] = (grad[a:a + 128] != 0).flatten(1).any(dim=1)
    touched = set(torch.nonzero(touched).view(-1).tolist())
    assert touched <= set(blocks.tolist()), sorted(touched - set(blocks.tolist()))[:8]
    for blk in blocks:
        g_blk = np.zeros((P, T, MOD.g))
        sel = rows // P == blk
        g_blk[rows[sel] % P] = vals[sel]
        errs["ds block %d" % blk] = rel_err(np64(grad[blk]), small_backward(sp_, g_blk.transpose(1, 0, 2))[0])
    peak = torch.cuda.max_memory_allocated()
    print(cls, kind, errs, "peak device memory %.1f GB" % (peak / 1e9))
    del grad, series, big
    release()
    assert max(errs.values()) <= TOL_GRAD, errs
    assert peak < BUDGET


@gpu
@pytest.mark.parametrize("cls", ["TGCNCheb_H", "ChebTimeConv"])
def test_forward_series_and_backward_on_a_stack_past_2_31(cls, gpu_device):
    train_step(cls, "train")


@gpu
@pytest.mark.parametrize("cls", ["TGCNCheb_H", "ChebTimeConv"])
def test_time_chunked_forward_series_and_backward_with_an_output_past_2_31(cls, gpu_device):
    """the _stream_at and _chunk_backward entries with the carried weight gradient, eight chunks of 32 rows: they write into and read from
    the whole as-series output and its gradient, 2.92 G elements each, at (s*n + i) * T * g + t0 * g; the chunk's own stack, G and ring stay
    far below 2^31 here (the chunked layer's point) and pass the line in the C ABI cases of CHUNK above"""
    train_step(cls, "chunked", time_chunk=MOD.time_chunk)


@gpu
@pytest.mark.filterwarnings("ignore:GraphOperand.reordered")
def test_forward_series_on_a_degree_reordered_operand(gpu_device):
    """forward only, T = 256: relabel_rows moves the series (1.46 G elements) in and the output (2.92 G elements, past 2^31) back"""
    from tgcn_amd import functional as F
    module_need("reordered")
    sp_ = small_problem("TGCNCheb_H", MOD_T["reordered"])
    big = BigLayer(sp_)
    with torch.no_grad():
        out = F.cheb_time_windows(big.op.reordered("degree"), big.series, big.layer.weight, big.layer.bias.reshape(-1), F.BIAS_VERTEX_CHANNEL,
                                  F.MODE_POWER, as_series=True, padding="causal")
    assert out.numel() == module_tensors("reordered")["out"] > LINE31
    check_output("reordered", out, sp_.ref)
    del out, big
    release()


@gpu
@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])
def test_forward_stream_in_three_chunks_with_a_ring_past_2_31(dt, gpu_device):
    """dilation 64: the ring (K, S, n, 128 * f) holds 2.2 G elements; each chunk's rows against the tiled oracle of the whole series"""
    module_need("stream", 4 if dt == torch.float32 else 2)
    sp_ = small_problem("TGCNCheb_H", MOD_T["stream"], dt == BF, MOD.stream_dilation)
    big = BigLayer(sp_, dt)
    state, t = None, 0
    with torch.no_grad():
        for Tc in MOD.chunks:
            out, state = big.layer.forward_stream(big.series[:, :, t:t + Tc], state, dilation=MOD.stream_dilation)
            assert tuple(out.shape) == (MOD.S, MOD.n, Tc, MOD.g) and out.dtype == dt and state.ring.numel() > LINE31
            check_output("stream rows [%d, %d)" % (t, t + Tc), out, sp_.ref, t, t + Tc, emu=sp_.emu)
            t += Tc
            del out
    del state, big
    release()


@gpu
def test_series_relu_pool_on_a_stack_past_2_31(gpu_device):
    """cheb_series_relu_pool(pool=4) against gcn_pool_4(relu(.)) of the tiled oracle, forward only"""
    import tgcn_amd
    module_need("pool")
    sp_ = small_problem("ChebTimeConv", MOD_T["pool"])
    big = BigLayer(sp_)
    with torch.no_grad():
        z = tgcn_amd.cheb_series_relu_pool(big.layer, big.series, *big.extra, pool=4, as_series=True, padding="causal")
    assert tuple(z.shape) == (MOD.S, MOD.n // 4, sp_.T, MOD.g)
    check_output("relu + pool 4", z, sp_.ref, pool=4)
    del z, big
    release()
