"""The one-launch small-graph kernels (csrc/small_graph.h) at the batch sizes where their launchers put several samples into one workgroup.
The launch configuration depends on the batch q: small_forward_kernel, small_narrow_kernel and small_basis_kernel run spw samples side by
side (thread = (slot, vertex)) once the grid keeps 512 workgroups, the narrow kernel widens its column tile to 32 / 64 once q * tiles >= 256,
and the matrix-pipe kernels take S = 4 / 2 samples once the grid keeps 192.  Every case below is a shape whose plan (F.small_plan, the
function the launch entries themselves get their numbers from) has spw >= 2 AND a tail workgroup with dead slots (q % spw != 0), or the
stated narrow tile; the CPU test pins those plans, the GPU tests compare the kernels at these batches with fp64, with the same call in
chunks of 64 samples (spw = 1), and check dead slots, slot isolation, the fused relu + pool epilogue and the module backward.

Operands.  Sparse: exactly 7 n entries (rows repeat(arange(n), 7), seeded random columns, values standard_normal * 0.5), then the entries of
rows 0 and 9 are moved to row 3: two empty rows and one 21-entry row, nnz = 7 n.  Dense: n = 148, exactly 100 entries per row, values
standard_normal * 0.05 (nnz = 14800 >= n^2 / 4: the operand keeps a dense copy and is for the matrix pipe).

Plans are written (form, tile, cp, spw, q % spw, threads) for mode 0 and mode 1; form 0 small_forward_kernel, 1 small_narrow_kernel,
2 small_basis_kernel, 3 fp32 matrix pipe, 4 bf16x3 matrix pipe.

Measured on an MI355X when the file was written, rel_err against fp64 on the sample subset, mode 0 / mode 1 (the bar is TOL = 1e-5):
F1 4.0e-7 / 4.9e-7; F2 3.1e-7 / 2.4e-7; F3 5.1e-7 / 5.5e-7; F4 7.0e-7 / 6.6e-7; F5 3.4e-7 / 7.1e-7; F6 2.0e-7 / 2.2e-7; F7 3.2e-7 / 3.1e-7;
N1 1.4e-7 / 1.2e-7; N2 1.3e-7 / 1.6e-7; N3 1.4e-7 / 1.2e-7; N4 2.0e-7 / 2.3e-7; N5 1.9e-7 / 1.5e-7; D1 2.4e-7 / 3.3e-7; D2 2.4e-7 / 3.7e-7;
D1f 2.0e-7 / 2.9e-7; B1 1.9e-7 / 1.5e-7; B2 1.3e-7 / 2.0e-7; B3 1.7e-7 / 1.6e-7; B4 2.3e-7 / 1.7e-7; B5 2.0e-7 / 1.6e-7; with the pool epilogue
F1 4.4e-7 / 4.1e-7; F2 3.1e-7 / 2.7e-7; F6 2.2e-7 / 2.0e-7; N1 1.2e-7 / 1.2e-7; N3 1.2e-7 / 1.4e-7; N4 2.8e-7 / 1.7e-7; N6 1.6e-7 / 1.7e-7.
Every bitwise comparison (full batch against 64-sample chunks, pooled output against the rule on the unpooled output) held."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import nonfinite_ref as R
from conftest import rel_err
from oracle import cheb_oracle as O

TOL = 1e-5            # BASELINE.md section 4, conftest.rel_err
K = 5
CHUNK = 64            # samples per call of the chunked run: spw = 1 in every plan (asserted on the host)
NAN = float("nan")
GUARD = 64
FWD, NARROW, BASIS, MFMA, X3 = 0, 1, 2, 3, 4

# id -> shape, tuning switches, pool variant and the plans of the two modes
FORWARD_CASES = {
    "F1": dict(n=196, C=32, N=64, q=511, pool=4, plans=((FWD, 16, 32, 4, 3, 1024), (FWD, 16, 32, 3, 1, 768))),
    # ragged column tile (37 = 2 * 16 + 5, N % 4 != 0), a spw that is no power of two
    "F2": dict(n=300, C=12, N=37, q=701, pool=2, plans=((FWD, 16, 16, 3, 2, 960), (FWD, 16, 16, 2, 1, 640))),
    # input row in pieces (C > 32)
    "F3": dict(n=49, C=40, N=128, q=1030, plans=((FWD, 16, 32, 16, 6, 1024), (FWD, 16, 32, 16, 6, 1024))),
    # limited by LDS in mode 1, C % 32 != 0
    "F4": dict(n=60, C=100, N=128, q=1100, plans=((FWD, 16, 32, 16, 12, 1024), (FWD, 16, 32, 13, 8, 832)), lds=(None, 161568)),
    # the operand as a dense matrix in LDS; the matrix pipe refuses C = 100
    "F5": dict(n=148, dense=True, C=100, N=64, q=601, plans=((FWD, 16, 32, 3, 1, 576), (FWD, 16, 32, 2, 1, 384)), dense_lds=1),
    "F6": dict(n=100, C=3, N=24, q=1030, pool=4, tuning=(b"small_narrow", 0), plans=((FWD, 16, 4, 4, 2, 512), (FWD, 16, 4, 4, 2, 512))),
    "F7": dict(n=500, C=16, N=64, q=513, plans=((FWD, 16, 16, 2, 1, 1024), (FWD, 16, 16, 1, 0, 512)), lds=(159040, None)),
    "N1": dict(n=100, C=1, N=64, q=1025, pool=4, plans=((NARROW, 64, 0, 2, 1, 256), (NARROW, 64, 0, 2, 1, 256))),
    "N2": dict(n=196, C=3, N=32, q=300, plans=((NARROW, 32, 0, 1, 0, 256), (NARROW, 32, 0, 1, 0, 256))),
    # N % 4 != 0: scalar stores, 27 dead columns of the 64-wide tile
    "N3": dict(n=196, C=3, N=37, q=300, pool=2, plans=((NARROW, 64, 0, 1, 0, 256), (NARROW, 64, 0, 1, 0, 256))),
    "N4": dict(n=320, C=2, N=64, q=1025, pool=4, plans=((NARROW, 64, 0, 2, 1, 640), (NARROW, 64, 0, 2, 1, 640))),
    # two column tiles
    "N5": dict(n=196, C=1, N=128, q=515, plans=((NARROW, 64, 0, 2, 1, 512), (NARROW, 64, 0, 2, 1, 512))),
    # matrix pipe, K = 10
    "D1": dict(n=148, dense=True, C=15, N=32, q=387, K=10, plans=((X3, 16, 0, 4, 3, 640), (X3, 16, 0, 2, 1, 640))),
    "D2": dict(n=148, dense=True, C=15, N=32, q=301, K=10, plans=((X3, 16, 0, 2, 1, 640), (X3, 16, 0, 2, 1, 640))),
    "D1f": dict(n=148, dense=True, C=15, N=32, q=387, K=10, tuning=(b"small_dense", 1), plans=((MFMA, 16, 0, 4, 3, 640), (MFMA, 16, 0, 2, 1, 640))),
}
# the raw entry with pool = 7: 64 % 7 != 0, so one input channel falls to the output-side kernel
N6 = dict(n=196, C=1, N=64, q=1025, pool=7, plans=((FWD, 16, 4, 4, 1, 1024), (FWD, 16, 4, 4, 1, 1024)), lds=(None, 162560))
BASIS_CASES = {
    "B1": dict(n=196, C=32, q=513, plans=((BASIS, 16, 0, 2, 1, 512), (BASIS, 16, 0, 2, 1, 512))),
    "B2": dict(n=300, C=12, q=1031, plans=((BASIS, 16, 0, 2, 1, 640), (BASIS, 16, 0, 2, 1, 640))),
    "B3": dict(n=49, C=40, q=1030, plans=((BASIS, 16, 0, 6, 4, 384), (BASIS, 16, 0, 6, 4, 384))),
    "B4": dict(n=100, C=3, q=2050, plans=((BASIS, 4, 0, 4, 2, 512), (BASIS, 4, 0, 4, 2, 512))),
    "B5": dict(n=196, C=7, q=1027, plans=((BASIS, 8, 0, 2, 1, 512), (BASIS, 8, 0, 2, 1, 512))),
}
POOL_CASES = [k for k, c in FORWARD_CASES.items() if c.get("pool")]
GUARDED = ("F1", "F3", "N1", "B3", "D1")
BIAS_KIND = {name: i % 3 for i, name in enumerate(FORWARD_CASES)}       # none / per channel / per vertex, cycled over the cases
MODES = pytest.mark.parametrize("mode", [0, 1], ids=["power", "chebyshev"])


# ---------------------------------------------------------------------------------------------------------------- operands
@functools.lru_cache(maxsize=None)
def _coo(n, dense=False):
    rng = np.random.default_rng(1000 + n + (7 if dense else 0))
    if dense:
        assert n == 148
        row = np.repeat(np.arange(n), 100)
        col = np.concatenate([rng.choice(n, 100, replace=False) for _ in range(n)])
        val = (rng.standard_normal(row.shape[0]) * 0.05).astype(np.float32)
        return row, col, val
    row = np.repeat(np.arange(n), 7)
    col = rng.integers(0, n, 7 * n)
    val = (rng.standard_normal(7 * n) * 0.5).astype(np.float32)
    row[(row == 0) | (row == 9)] = 3
    return row, col, val


@functools.lru_cache(maxsize=None)
def _operand(n, dense=False, device="cuda"):
    """(GraphOperand on `device`, the operand as fp64 scipy CSR)"""
    from tgcn_amd.graph import GraphOperand
    row, col, val = _coo(n, dense)
    op = GraphOperand.from_coo(n, torch.as_tensor(row), torch.as_tensor(col), torch.as_tensor(val), device=device)
    assert op.nnz == (14800 if dense else 7 * n) and (op.dense is not None) == dense
    if not dense:
        counts = np.bincount(row, minlength=n)
        assert counts[0] == 0 and counts[9] == 0 and counts[3] == 21
    return op, O.coo_to_csr(row, col, val, n).astype(np.float64)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _set_tuning(case):
    from tgcn_amd import _lib
    if case.get("tuning"):
        _lib.check(_lib.lib().tgcn_set_tuning(*case["tuning"]))


def _plan_tuple(pl, q):
    return (pl["form"], pl["tile"], pl["cp"], pl["spw"], q % pl["spw"], pl["threads"])


# ---------------------------------------------------------------------------------------------------------------- the plans (host only)
def test_the_shapes_hit_what_they_are_here_for():
    """The plan of every case, both modes, as the launch entries compute it (F.small_plan -> tgcn_cheb_small_plan, the function they call):
    the table above, the grid that follows from it, and spw = 1 for the 64-sample chunks the device comparison runs against.  Then the
    coverage the cases exist for: every kernel form and tile with spw >= 2 and a tail workgroup, narrow tiles 32 and 64, matrix pipe S = 4
    and S = 2 with q % S != 0."""
    from tgcn_amd import _lib, functional as F
    seen = set()
    cases = [(k, c, False) for k, c in FORWARD_CASES.items()] + [("N6", N6, False)] + [(k, c, True) for k, c in BASIS_CASES.items()]
    for name, case, basis in cases:
        op, _ = _operand(case["n"], case.get("dense", False), device="cpu")
        _lib.lib().tgcn_reset_tuning()
        _set_tuning(case)
        for mode in (0, 1):
            N, q = case.get("N", 0), case["q"]
            for pool in sorted({0, case.get("pool", 0)} if name != "N6" else {7}):
                pl = F.small_plan(op, case["C"], N, q, mode, pool=pool, basis=basis)
                assert _plan_tuple(pl, q) == case["plans"][mode], (name, mode, pool, pl)
                assert pl["dense_lds"] == case.get("dense_lds", 0), (name, mode, pl)
                assert pl["grid_x"] == -(-q // pl["spw"]) and pl["grid_y"] == -(-(case["C"] if basis else N) // pl["tile"]), (name, mode, pl)
                assert pl["lds_bytes"] <= 160 * 1024 and pl["threads"] <= 1024
                if case.get("lds", (None, None))[mode] is not None:
                    assert pl["lds_bytes"] == case["lds"][mode], (name, mode, pl)
            small = F.small_plan(op, case["C"], N, CHUNK, mode, pool=case.get("pool", 0), basis=basis)
            assert small["spw"] == 1, (name, mode, small)
            assert small["form"] == pl["form"] or pl["form"] == X3 and small["form"] == MFMA, (name, mode, small)
            if pl["spw"] >= 2 and q % pl["spw"]:
                seen.add(pl["form"] if pl["form"] >= MFMA else (pl["form"], pl["tile"], pl["cp"]))
                if pl["form"] >= MFMA:
                    seen.add(("S", pl["spw"]))
            if pl["form"] == NARROW:
                seen.add(("NT", pl["tile"]))
    _lib.lib().tgcn_reset_tuning()
    want = {(FWD, 16, 32), (FWD, 16, 16), (FWD, 16, 4), (NARROW, 64, 0), (BASIS, 16, 0), (BASIS, 8, 0), (BASIS, 4, 0), MFMA, X3,
            ("S", 4), ("S", 2), ("NT", 32), ("NT", 64)}
    assert want <= seen, want - seen


def test_small_plan_refuses_where_the_entries_refuse():
    from tgcn_amd import _lib, functional as F
    L = _lib.lib()
    pl = _lib.SmallPlanStruct()
    call = lambda *a: L.tgcn_cheb_small_plan(*a, C.byref(pl))
    INVALID, UNSUPPORTED = -1, -4            # TGCN_ERR_INVALID, TGCN_ERR_UNSUPPORTED
    ok = (196, 1372, 0, 0, 32, 64, 511, 0, 0)
    assert call(*ok) == 0 and pl.spw == 4
    assert L.tgcn_cheb_small_plan(*ok, None) == INVALID
    for bad in ((196, 1372, 0, 0, 32, 64, 0, 0, 0), (196, 1372, 0, 0, 32, 0, 511, 0, 0), (196, 1372, 0, 0, 32, 64, 511, 5, 0),
                (196, 1372, 0, 0, 32, 64, 511, 256, 0), (196, 1372, 0, 0, 0, 64, 511, 0, 1)):
        assert call(*bad) == INVALID, bad
    for big in ((1025, 7000, 0, 0, 32, 64, 511, 0, 0), (196, 1372, 0, 0, 129, 64, 511, 0, 0), (196, 1372, 0, 2, 32, 64, 511, 0, 0),
                (196, 1372, 0, 0, 32, 64, 2 ** 31, 0, 0), (1025, 7000, 0, 0, 32, 0, 511, 0, 1), (196, (1 << 20) + 1, 0, 0, 32, 64, 511, 0, 0)):
        assert call(*big) == UNSUPPORTED, big
    assert b"small_plan" in L.tgcn_last_error()
    with pytest.raises(_lib.TgcnError):
        F.small_plan(_operand(196, device="cpu")[0], 129, 64, 511, 0)


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def _subset(q, spw, seed):
    """sample 0, the last sample of the first (full) workgroup, every sample of the last workgroup, 16 seeded others"""
    first_of_last = (q - 1) // spw * spw
    s = {0, spw - 1} | set(range(first_of_last, q))
    s |= set(np.random.default_rng(seed).choice(q, 16, replace=False).tolist())
    return np.array(sorted(s))


def _inputs(name, case, mode):
    rng = np.random.default_rng([sum(map(ord, name)), mode])
    n, Crow, N, q, Kc = case["n"], case["C"], case.get("N", 0), case["q"], case.get("K", K)
    x = rng.standard_normal((q, n, Crow)).astype(np.float32)
    W = (rng.standard_normal((Kc, Crow, max(N, 1))) / np.sqrt(Kc * Crow)).astype(np.float32)
    kind = BIAS_KIND.get(name, 1)
    bias = None if kind == 0 else rng.standard_normal(N if kind == 1 else (n, N)).astype(np.float32)
    return x, W, kind, bias


def _forward64(L, x, W, bias, mode):
    stack = O.stack_reference_power if mode == 0 else O.stack_chebyshev
    ref = np.einsum("kqnc,kcg->qng", stack(L, x.astype(np.float64), W.shape[0]), W.astype(np.float64))
    return ref if bias is None else ref + bias


def _basis64(L, x, Kc, mode):
    if mode == 1:
        return O.stack_chebyshev(L, x.astype(np.float64), Kc)
    P = [x.astype(np.float64)]
    for _ in range(1, Kc):
        P.append(O._apply(L, P[-1]))
    return np.stack(P)


def _fold(mode, Kc):
    from tgcn_amd import functional as F
    return F.power_fold_matrix(Kc, "cuda") if (mode == 0 and Kc > 2) else None


def _nan_out(shape, dtype=torch.float32, fill=NAN):
    numel = int(np.prod(shape))
    buf = torch.full((GUARD + numel + GUARD,), fill, dtype=dtype, device="cuda")
    return buf[GUARD:GUARD + numel].view(shape), buf


def _guards_untouched(buf, numel, fill=NAN):
    g = torch.cat([buf[:GUARD], buf[GUARD + numel:]])
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


def _raw_forward(op, x, W, fold, bias, kind, mode, out, relu=0, pool=0, idx=None):
    from tgcn_amd import _lib
    q, n, Crow = x.shape
    _lib.check(_lib.lib().tgcn_cheb_forward_small_pool_f32(_lib.stream_ptr(), C.byref(op.struct), mode, W.shape[0], q, Crow, W.shape[2],
                                                           _lib.ptr(x), _lib.ptr(W), _lib.ptr(fold), _lib.ptr(bias), kind, relu, pool,
                                                           _lib.ptr(out), _lib.ptr(idx)))


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _chunks_run_the_same_sums(F, op, case, mode, full, basis):
    """True where every 64-sample chunk runs the full call's kernel form and tile, or only the narrow kernel's tile width differs (each
    output column is the same fmaf chain over (k, c) whatever the width): then a sample's sums do not depend on its slot and the two runs
    must agree bit for bit."""
    q = case["q"]
    for qc in {CHUNK, q % CHUNK} - {0}:
        pl = F.small_plan(op, case["C"], case.get("N", 0), qc, mode, basis=basis)
        assert pl["spw"] == 1
        if pl["form"] != full["form"] or (pl["tile"] != full["tile"] and full["form"] != NARROW):
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------- 1-3: forward
@pytest.mark.gpu
@MODES
@pytest.mark.parametrize("name", list(FORWARD_CASES))
def test_forward_at_the_batch(name, mode, gpu_device):
    """F.cheb_forward_small at the full batch: (1) against the fp64 oracle on sample 0, the last sample of a full workgroup, every sample
    of the tail workgroup and 16 seeded others; (2) every sample against the same call in chunks of 64 (spw = 1), bit for bit where the
    plans say both run the same kernel form and tile; (3) for the guarded cases the same launch into an output inside NaN guards: the
    dead slots of the tail workgroup write nothing."""
    from tgcn_amd import functional as F
    case = FORWARD_CASES[name]
    op, L = _operand(case["n"], case.get("dense", False))
    _set_tuning(case)
    q = case["q"]
    x, W, kind, bias = _inputs(name, case, mode)
    pl = F.small_plan(op, case["C"], case["N"], q, mode)
    assert _plan_tuple(pl, q) == case["plans"][mode]
    xd, Wd, bd, fold = _dev(x), _dev(W), None if bias is None else _dev(bias), _fold(mode, W.shape[0])
    out = F.cheb_forward_small(op, xd, Wd, fold, bd, kind, mode)
    sub = _subset(q, pl["spw"], 1)
    err = rel_err(out[torch.as_tensor(sub).cuda()].cpu().numpy(), _forward64(L, x[sub], W, bias, mode))
    print("%s mode %d plan %s rel_err %.3g" % (name, mode, _plan_tuple(pl, q), err))
    assert err <= TOL, (name, mode, err)
    chunked = torch.cat([F.cheb_forward_small(op, xd[i:i + CHUNK], Wd, fold, bd, kind, mode) for i in range(0, q, CHUNK)])
    if _chunks_run_the_same_sums(F, op, case, mode, pl, False):
        assert _bits_equal(out, chunked), (name, mode, "differs from the spw = 1 run at samples",
                                           (out != chunked).any(dim=2).any(dim=1).nonzero().flatten()[:8].tolist())
    else:           # another kernel form (bf16x3 matrix pipe against the fp32 one below S = 2): other sums, the project's bar
        assert rel_err(out.cpu().numpy(), chunked.cpu().numpy()) <= TOL, (name, mode)
    if name in GUARDED:
        o, buf = _nan_out(out.shape)
        _raw_forward(op, xd, Wd, fold, bd, kind, mode, o)
        torch.cuda.synchronize()
        assert _guards_untouched(buf, o.numel()), (name, mode)
        assert _bits_equal(o, out)


@pytest.mark.gpu
@MODES
@pytest.mark.parametrize("name", list(BASIS_CASES))
def test_basis_at_the_batch(name, mode, gpu_device):
    """F.cheb_basis_small at the full batch: the three checks of test_forward_at_the_batch on every term k = 1 .. K-1."""
    from tgcn_amd import _lib, functional as F
    case = BASIS_CASES[name]
    op, L = _operand(case["n"])
    q, n, Crow = case["q"], case["n"], case["C"]
    x = _inputs(name, case, mode)[0]
    pl = F.small_plan(op, Crow, 0, q, mode, basis=True)
    assert _plan_tuple(pl, q) == case["plans"][mode]
    xd = _dev(x)
    terms = F.cheb_basis_small(op, xd, K, mode)
    sub = _subset(q, pl["spw"], 2)
    ref = _basis64(L, x[sub], K, mode)
    subd = torch.as_tensor(sub).cuda()
    errs = [rel_err(terms[k][subd].cpu().numpy(), ref[k]) for k in range(1, K)]
    print("%s mode %d plan %s rel_err %.3g" % (name, mode, _plan_tuple(pl, q), max(errs)))
    assert max(errs) <= TOL, (name, mode, errs)
    assert _chunks_run_the_same_sums(F, op, case, mode, pl, True)
    parts = [F.cheb_basis_small(op, xd[i:i + CHUNK], K, mode) for i in range(0, q, CHUNK)]
    for k in range(1, K):
        assert _bits_equal(terms[k], torch.cat([p[k] for p in parts])), (name, mode, k)
    if name in GUARDED:
        stack, buf = _nan_out((K - 1, q, n, Crow))
        base = stack.data_ptr() - q * n * Crow * 4          # the address term 0 would have (F.cheb_basis_small)
        _lib.check(_lib.lib().tgcn_cheb_basis_small_f32(_lib.stream_ptr(), C.byref(op.struct), mode, K, q, Crow, _lib.ptr(xd), base))
        torch.cuda.synchronize()
        assert _guards_untouched(buf, stack.numel()), (name, mode)
        for k in range(1, K):
            assert _bits_equal(stack[k - 1], terms[k])


# ---------------------------------------------------------------------------------------------------------------- 4: slots do not leak
def _bfs(A, start, hops):
    reach = np.zeros(A.shape[0], bool)
    reach[start] = True
    for _ in range(hops):
        reach = reach | ((A @ reach.astype(np.float64)) > 0)
    return reach


def _expect_cones(clean, poisoned, samples, cone, what):
    """(q, n, F): NaN in every channel at (s, cone) for s in samples, bit-identical to the clean run everywhere else"""
    mask = np.zeros(clean.shape[:2], bool)
    mask[np.asarray(samples)[:, None], np.nonzero(cone)[0][None, :]] = True
    inside = torch.as_tensor(mask, device=clean.device)
    assert torch.isnan(poisoned[inside]).all(), what + ": a finite value inside the cone"
    a, b = clean[~inside].contiguous(), poisoned[~inside].contiguous()
    bad = (a.view(torch.int32) != b.view(torch.int32)).nonzero()
    assert bad.numel() == 0, "%s: %d values outside the cones differ from the clean run, first at (sample, vertex) = %s" % (
        what, bad.shape[0], np.argwhere(~mask)[int(bad[0, 0])].tolist())
    assert not torch.isnan(a).any(), what


@pytest.mark.gpu
@MODES
@pytest.mark.parametrize("name", ["F1", "N1", "B1"])
def test_samples_do_not_leak_across_slots(name, mode, gpu_device):
    """NaN at one vertex of the sample in slot 1 of workgroup 0 and of the last live sample of the tail workgroup: every other sample is
    bit-identical to the clean run, the two poisoned ones are NaN exactly inside the cone of K - 1 hops (term k of the basis: exactly where
    its recurrence puts the NaN -- walks of k entries for L^k x, of k, k - 2, ... entries for T_k x)."""
    from tgcn_amd import functional as F
    basis = name in BASIS_CASES
    case = BASIS_CASES[name] if basis else FORWARD_CASES[name]
    op, L = _operand(case["n"])
    q, v0 = case["q"], 5
    x, W, kind, bias = _inputs(name, case, mode)
    pl = F.small_plan(op, case["C"], case.get("N", 0), q, mode, basis=basis)
    assert pl["spw"] >= 2 and q % pl["spw"], pl
    poisoned = [1, q - 1]
    xb = x.copy()
    xb[poisoned, v0] = NAN
    A = abs(L)
    cone = _bfs(A, v0, K - 1)
    assert cone[v0] and not cone[0] and not cone[9] and cone.sum() < case["n"]           # the empty rows read nobody
    if basis:
        # a term alone is not a sum over all walk lengths (this operand has no self loops): L^k x is NaN where a walk of exactly k
        # entries ends in v0, and T_k = 2 L T_{k-1} - T_{k-2} where L T_{k-1} or T_{k-2} is
        step = lambda s: (A @ s.astype(np.float64)) > 0
        hit = [np.arange(case["n"]) == v0]
        for k in range(1, K):
            hit.append(step(hit[-1]) | (hit[-2] if (mode == 1 and k >= 2) else False))
        assert all((h <= _bfs(A, v0, k)).all() for k, h in enumerate(hit)) and not hit[1][v0]
        tc, tp = F.cheb_basis_small(op, _dev(x), K, mode), F.cheb_basis_small(op, _dev(xb), K, mode)
        for k in range(1, K):
            _expect_cones(tc[k], tp[k], poisoned, hit[k], "%s term %d" % (name, k))
        return
    Wd, bd, fold = _dev(W), None if bias is None else _dev(bias), _fold(mode, K)
    run = lambda a: F.cheb_forward_small(op, _dev(a), Wd, fold, bd, kind, mode)
    _expect_cones(run(x), run(xb), poisoned, cone, name)


# ---------------------------------------------------------------------------------------------------------------- 5: relu + pool epilogue
def _pool_rule_all(y, pool):
    """R.pool_rule (members ascending, the first maximum wins, a NaN takes over once and stays; relu keeps NaN) on whole arrays: the rule
    itself loops in Python over every element, which at these batches is minutes.  test_relu_pool_epilogue_at_the_batch checks this
    restatement against R.pool_rule on the sample subset before it relies on it."""
    q, n, Fc = y.shape
    g = y.reshape(q, n // pool, pool, Fc)
    best, bi = g[:, :, 0].copy(), np.zeros((q, n // pool, Fc), np.uint8)
    for m in range(1, pool):
        v = g[:, :, m]
        take = (v > best) | ((v != v) & (best == best))
        best, bi = np.where(take, v, best), np.where(take, np.uint8(m), bi)
    z = np.where(best > 0, best, np.where(best != best, best, y.dtype.type(0.0)))
    return z, bi


@pytest.mark.gpu
@MODES
@pytest.mark.parametrize("name", POOL_CASES + ["N6"])
def test_relu_pool_epilogue_at_the_batch(name, mode, gpu_device):
    """tgcn_cheb_forward_small_pool_f32 (relu, pool, pool_idx) at the full batch, output and pool_idx inside guards: values and indices
    are the rule applied to the unpooled output of F.cheb_forward_small on the same inputs, bit for bit, and the values are within TOL of
    the rule applied to the fp64 oracle's output on the sample subset.  N6 (pool = 7 on one input channel) runs the output-side kernel,
    so its unpooled run is taken with small_narrow = 0: the same kernel, the same sums."""
    from tgcn_amd import _lib, functional as F
    case = N6 if name == "N6" else FORWARD_CASES[name]
    op, L = _operand(case["n"])
    _set_tuning(case)
    q, n, N, pool = case["q"], case["n"], case["N"], case["pool"]
    x, W, kind, bias = _inputs(name, case, mode)
    pl = F.small_plan(op, case["C"], N, q, mode, pool=pool)
    assert _plan_tuple(pl, q) == case["plans"][mode]
    xd, Wd, bd, fold = _dev(x), _dev(W), None if bias is None else _dev(bias), _fold(mode, K)
    z, zbuf = _nan_out((q, n // pool, N))
    idx, ibuf = _nan_out((q, n // pool, N), torch.uint8, 99)
    _raw_forward(op, xd, Wd, fold, bd, kind, mode, z, relu=1, pool=pool, idx=idx)
    torch.cuda.synchronize()
    assert _guards_untouched(zbuf, z.numel()) and _guards_untouched(ibuf, idx.numel(), 99), (name, mode)
    if name == "N6":
        _lib.check(_lib.lib().tgcn_set_tuning(b"small_narrow", 0))
    unpooled = F.cheb_forward_small(op, xd, Wd, fold, bd, kind, mode).cpu().numpy()
    assert F.small_plan(op, case["C"], N, q, mode)["form"] == pl["form"]
    zref, iref = _pool_rule_all(unpooled, pool)
    sub = _subset(q, pl["spw"], 3)
    zsub, isub = R.pool_rule(unpooled[sub], pool)
    assert np.array_equal(zsub.view(np.int32), zref[sub].view(np.int32)) and np.array_equal(isub, iref[sub])
    got, goti = z.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(got.view(np.int32), zref.view(np.int32)), (name, mode, np.argwhere(got.view(np.int32) != zref.view(np.int32))[:4].tolist())
    assert np.array_equal(goti, iref), (name, mode, np.argwhere(goti != iref)[:4].tolist())
    z64 = _pool_rule_all(_forward64(L, x[sub], W, bias, mode), pool)[0]
    err = rel_err(got[sub], z64)
    print("%s mode %d pool %d plan %s rel_err %.3g" % (name, mode, pool, _plan_tuple(pl, q), err))
    assert err <= TOL, (name, mode, err)


# ---------------------------------------------------------------------------------------------------------------- 6: through the modules
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["GCNCheb_F1", "GCNCheb_F1_relu_pool4", "TGCNCheb_H_N1"])
def test_modules_forward_and_backward_at_the_batch(which, gpu_device, monkeypatch):
    """GCNCheb(L, 32, 64, 5) on F1's graph at q = 511 (plain and through cheb_relu_pool(pool=4)) and TGCNCheb_H(L, 1, 64, 5, 3) on N1's graph
    at q = 1025 (C = H f = 3: the narrow kernel): the forward, and the one-launch backward -- the forward kernel on L^T for x.grad, the basis
    kernel + weight gradient -- against the fp64 references of tests/test_backward_at_scale.py at its tolerance, on the small path."""
    import tgcn_amd
    from tgcn_amd import functional as F
    from test_backward_at_scale import _PathRecorder, _check_grads
    pooled = which.endswith("pool4")
    gcn = which.startswith("GCNCheb")
    case = FORWARD_CASES["F1" if gcn else "N1"]
    op, L = _operand(case["n"])
    q, n = case["q"], case["n"]
    torch.manual_seed(1)
    layer = (tgcn_amd.GCNCheb(op, 32, 64, K) if gcn else tgcn_amd.TGCNCheb_H(op, 1, 64, K, 3)).cuda()
    Crow = 32 if gcn else 3
    for mode_q in ((Crow, 64), (64, Crow)):                   # the forward, and the input gradient's layer on L^T
        assert F.small_plan(op.transpose() if mode_q[0] == 64 else op, mode_q[0], mode_q[1], q, 0)["spw"] >= 2
    assert F.small_plan(op, Crow, 0, q, 0, basis=True)["spw"] >= 2
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((q, n, Crow), device="cuda", generator=gen)
    rec = _PathRecorder(monkeypatch)
    xt = x.clone().requires_grad_(True)
    out = tgcn_amd.cheb_relu_pool(layer, xt, pool=4) if pooled else layer(xt)
    go = torch.randn(out.shape, device="cuda", generator=gen)
    out.backward(go)
    kind, basis = rec.only()
    assert kind == "small" and basis is None
    Wn = layer.weight.detach().cpu().numpy()
    x4 = x.cpu().numpy() if gcn else x.cpu().numpy()[..., None]
    with torch.no_grad():
        y = layer(x)
    sub = _subset(q, 4, 4)
    fwd = O.gcn_cheb_forward if gcn else O.tgcn_cheb_h_forward
    yref = fwd(L, x.cpu().numpy()[sub], Wn, layer.bias.detach().cpu().numpy())
    assert rel_err(y.cpu().numpy()[sub], yref) <= TOL
    gy = go.cpu().numpy()
    if pooled:            # relu + pool backward by the rule, on the device's own unpooled output (its arg-max is what test 5 pins)
        yn = y.cpu().numpy()
        z, bi = _pool_rule_all(yn, 4)
        assert np.array_equal(out.detach().cpu().numpy().view(np.int32), z.view(np.int32))
        gy4 = np.zeros((q, n // 4, 4, 64), np.float32)
        np.put_along_axis(gy4, bi[:, :, None, :].astype(np.int64), np.where(z > 0, gy, np.float32(0))[:, :, None, :], axis=2)
        gy = gy4.reshape(q, n, 64)
    rx, rW = O.layer_backward_gside(L, x4, Wn, gy, "power")
    ref_b = gy.astype(np.float64).sum(axis=(0, 1)).reshape(layer.bias.shape) if gcn else gy.astype(np.float64).sum(axis=0, keepdims=True)
    _check_grads(xt.grad, layer.weight.grad, layer.bias.grad, rx.reshape(x.shape), rW, ref_b)
