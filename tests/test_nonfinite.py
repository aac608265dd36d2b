"""+-Inf and NaN stay where a per-term evaluation puts them.  Two kinds of error cannot show on finite data: a product
of a padding value with a real one (0 * neighbour is 0 for a finite neighbour and NaN for +-Inf / NaN: the k dimension rounded up to a tile,
rows past M, columns past N, clamped indices, ring slots, zero time padding) and a comparison that drops a NaN (max, relu, arg-max).

Every case comes from tests/nonfinite_ref.py, whose float64 per-term references and coverage conditions tests/test_nonfinite_ref.py checks
on the CPU.  Outputs are compared by CLASS (finite / +Inf / -Inf / NaN) element by element and by the kernel's usual tolerance on the
finite part: 1e-5 for fp32 outputs, 2e-5 for gradients; bf16 outputs of operands that are exact in bf16 are one rounding of an fp32 sum of
exact products, half a bf16 ulp of the value: 2^-8 of max|ref| under the project's metric (the bound tests/test_series_bf16.py uses for the
same situation).  Guard regions are ordinary allocated memory filled with NaN -- a larger tensor of which the operand is a view -- and
nothing reads or writes outside an allocation.

  A1 hops (fp32, two-hop form, bf16, fp64)     A2 projections and weight gradients, with the bf16x3 deviation pinned
  A3 every time-window entry, forward and backward, the poison in the chunk and in the ring
  A4 the relu / max-pool rule on crafted groups, arg-max bytes and backward included
  A5 the one-launch small-graph kernels, sparse (the cone of a 12 x 12 grid) and dense (the whole sample: the documented deviation)
  B1 / B2 locality on the graph of cheb_layer, forward and backward, on every layer path and in both recurrences
  B3 locality in time and on the graph of forward_series / forward_stream on every streaming path"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import nonfinite_ref as R
from conftest import rel_err
from oracle import cheb_oracle as O
from test_series_channels import _dev

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:GraphOperand.reordered")]
TOL = 1e-5
TOL_GRAD = 2e-5
TOL_BF16 = 2.0 ** -8
TOL_F64 = 1e-12           # fp64 sums of at most a few thousand O(1) terms
NAN = float("nan")
GUARD = 64                # floats of NaN in front of and behind a guarded operand (a multiple of 4: the 16-byte alignment is kept)


def _guarded(a, dtype=torch.float32, front=GUARD):
    """the array on the device as a contiguous view into a larger NaN-filled buffer -> (view, buffer)"""
    a = np.ascontiguousarray(a)
    buf = torch.full((front + a.size + GUARD,), NAN, dtype=dtype, device="cuda")
    view = buf[front:front + a.size].view(a.shape)
    view.copy_(torch.as_tensor(a).to(dtype))
    return view, buf


def _nan_out(shape, dtype=torch.float32):
    """an output as a view into a NaN-filled buffer, GUARD elements in front and behind -> (view, buffer)"""
    numel = int(np.prod(shape))
    buf = torch.full((GUARD + numel + GUARD,), NAN, dtype=dtype, device="cuda")
    return buf[GUARD:GUARD + numel].view(shape), buf


def _guards_untouched(buf, numel):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + numel:]).all())


def _padded_rows(a, ld, dtype=torch.float32):
    """a (..., C) as a view with row stride ld > C into a NaN-filled (..., ld) buffer"""
    a = np.ascontiguousarray(a)
    buf = torch.full(a.shape[:-1] + (ld,), NAN, dtype=dtype, device="cuda")
    view = buf[..., :a.shape[-1]]
    view.copy_(torch.as_tensor(a).to(dtype))
    return view, buf


def _np(t):
    return t.detach().double().cpu().numpy()


# ================================================================================================================ A1: hops
hop_case = functools.lru_cache(maxsize=None)(R.hop_case)


@functools.lru_cache(maxsize=None)
def _hop_operand():
    from tgcn_amd.graph import GraphOperand
    row, col, val, mk = R.hop_graph(seed=0)
    return GraphOperand.from_coo(mk["n"], _dev(row), _dev(col), _dev(val))


def _ld(C_row):
    """a leading dimension > C: one that keeps 16-byte rows for the 16-byte forms, an odd one for the others"""
    return C_row + 8 if C_row % 4 == 0 else C_row + 3


@pytest.mark.parametrize("C_row", [1, 4, 16, 64, 300])
@pytest.mark.parametrize("poison", R.HOP_POISONS)
def test_hop_fp32(poison, C_row, gpu_device):
    """F.csr_hop: X and the output are views with ld > C into NaN-filled buffers"""
    from tgcn_amd import functional as F
    row, col, val, mk, x, ref = hop_case(poison, C_row)
    op = _hop_operand()
    xv, _ = _padded_rows(x, _ld(C_row))
    yv, ybuf = _padded_rows(np.full(ref.shape, NAN, np.float32), _ld(C_row))
    F.csr_hop(op, xv, out=yv)
    R.assert_matches(_np(yv), ref, TOL, "csr_hop %s C=%d" % (poison, C_row))
    assert torch.isnan(ybuf[..., C_row:]).all(), "the padding behind the output rows was written"
    assert (R.cls(_np(yv)[0]) == R.FIN).all()
    for i in mk["iso"]:
        assert (_np(yv)[:, i] == 0).all()


@pytest.mark.parametrize("C_row", [1, 4, 16, 64, 300])
def test_hop_fp32_z_terms(C_row, gpu_device):
    """y = alpha L x + beta z + gamma z2: -Inf in a row of z and NaN in a row of z2 (non-zero factors) reach that row and no other, on top of
    the +Inf / -Inf pair in X; also through the one-z form with want_p, whose P = L x must not see z"""
    from tgcn_amd import functional as F
    row, col, val, mk, x, _ = hop_case("inf_minus_inf", C_row)
    n = mk["n"]
    rng = np.random.default_rng(C_row)
    z = rng.choice([-2.0, -1.0, 1.0, 2.0], x.shape).astype(np.float32)
    z2 = rng.choice([-2.0, -1.0, 1.0, 2.0], x.shape).astype(np.float32)
    z[1, 100], z2[1, 200], z2[0, mk["iso"][0]] = -R.INF, NAN, R.INF
    op = _hop_operand()
    xv, zv, z2v = (_padded_rows(a, _ld(C_row))[0] for a in (x, z, z2))
    ref2 = R.order_checked(lambda rev: R.hop_ref(n, row, col, val, x, z, 2.0, -1.0, z2, 0.5, reverse=rev), "hop2")
    R.check_coverage(ref2, "hop2", neighbour_axis=1)
    y = F.csr_hop(op, xv, z=zv, alpha=2.0, beta=-1.0, z2=z2v, gamma=0.5)
    R.assert_matches(_np(y), ref2, TOL, "csr_hop z2 C=%d" % C_row)
    assert R.cls(_np(y)[0, mk["iso"][0]]).tolist() == [R.PINF] * C_row          # an isolated vertex: exactly beta z + gamma z2
    ref1 = R.hop_ref(n, row, col, val, x, z, 2.0, -1.0)
    y, p = F.csr_hop(op, xv, z=zv, alpha=2.0, beta=-1.0, want_p=True)
    R.assert_matches(_np(y), ref1, TOL, "csr_hop z C=%d" % C_row)
    R.assert_matches(_np(p), R.hop_ref(n, row, col, val, x), TOL, "csr_hop P C=%d" % C_row)


@pytest.mark.parametrize("C_row", [1, 4, 16, 64, 300])
@pytest.mark.parametrize("poison", R.HOP_POISONS)
def test_hop_bf16(poison, C_row, gpu_device):
    """F.csr_hop_bf16 on operands that are exact in bf16; ld > C (a multiple of 8 where the 16-byte form applies)"""
    from tgcn_amd import functional as F
    row, col, val, mk, x, ref = hop_case(poison, C_row)
    ld = C_row + 8 if C_row % 8 == 0 else C_row + 3
    xv, _ = _padded_rows(x, ld, torch.bfloat16)
    yv, ybuf = _padded_rows(np.full(ref.shape, NAN, np.float32), ld, torch.bfloat16)
    F.csr_hop_bf16(_hop_operand(), xv, out=yv)
    R.assert_matches(_np(yv), ref, TOL_BF16, "csr_hop_bf16 %s C=%d" % (poison, C_row))
    assert torch.isnan(ybuf[..., C_row:]).all()


@pytest.mark.parametrize("C_row", [1, 4, 16, 64, 300])
def test_hop_bf16_z_terms(C_row, gpu_device):
    """the bf16 two-hop form y = alpha L x + beta z + gamma z2 with -Inf in a row of z and NaN in a row of z2"""
    from tgcn_amd import functional as F
    row, col, val, mk, x, _ = hop_case("inf_minus_inf", C_row)
    n = mk["n"]
    rng = np.random.default_rng(C_row)
    z = rng.choice([-2.0, -1.0, 1.0, 2.0], x.shape).astype(np.float32)
    z2 = rng.choice([-2.0, -1.0, 1.0, 2.0], x.shape).astype(np.float32)
    z[1, 100], z2[1, 200], z2[0, mk["iso"][0]] = -R.INF, NAN, R.INF
    ld = C_row + 8 if C_row % 8 == 0 else C_row + 3
    xv, zv, z2v = (_padded_rows(a, ld, torch.bfloat16)[0] for a in (x, z, z2))
    ref = R.order_checked(lambda rev: R.hop_ref(n, row, col, val, x, z, 2.0, -1.0, z2, 0.5, reverse=rev), "hop2 bf16")
    y = F.csr_hop_bf16(_hop_operand(), xv, z=zv, alpha=2.0, beta=-1.0, z2=z2v, gamma=0.5)
    R.assert_matches(_np(y), ref, TOL_BF16, "csr_hop_bf16 z2 C=%d" % C_row)


@pytest.mark.parametrize("C_row", [1, 4, 16, 64, 300])
@pytest.mark.parametrize("poison", R.HOP_POISONS)
def test_hop_fp64(poison, C_row, gpu_device):
    """tgcn_csr_hop_f64 on the plain CSR of the same entries in stored order; the samples ride in the row: F = nb * C doubles"""
    from tgcn_amd import _lib
    row, col, val, mk, x, ref = hop_case(poison, C_row)
    n, nb = mk["n"], x.shape[0]
    order = np.argsort(row, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(np.int32)
    rp, ci, va = _dev(rowptr), _dev(col[order].astype(np.int32)), _dev(val[order].astype(np.float64))
    X, _ = _guarded(np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(n, nb * C_row), torch.float64)
    Y, ybuf = _nan_out((n, nb * C_row), torch.float64)
    _lib.check(_lib.lib().tgcn_csr_hop_f64(_lib.stream_ptr(), n, _lib.ptr(rp), _lib.ptr(ci), _lib.ptr(va), nb * C_row, _lib.ptr(X), None,
                                           C.c_double(1.0), C.c_double(0.0), _lib.ptr(Y), None))
    got = _np(Y).reshape(n, nb, C_row).transpose(1, 0, 2)
    R.assert_matches(got, ref, TOL_F64, "csr_hop_f64 %s C=%d" % (poison, C_row))
    assert _guards_untouched(ybuf, Y.numel())


# ================================================================================================================ A2: projections
project_case = functools.lru_cache(maxsize=None)(R.project_case)
project_large_case = functools.lru_cache(maxsize=None)(R.project_large_case)
EXACT_VARIANTS = (0, 1, 2, 4, 5)      # at M = 130 rows "auto" is an exact-fp32 kernel too (bf16x3 starts at 8192 rows)
X3_VARIANT = 3                        # bf16x3 always


def _lda(Kc):
    return Kc + 4 if Kc % 4 == 0 else Kc + 3


def _project(terms, W, bias, variant, bf16=False):
    from tgcn_amd import _lib, functional as F
    dt = torch.bfloat16 if bf16 else torch.float32
    tv = [_padded_rows(t, _lda(t.shape[1]) + (4 if bf16 else 0), dt)[0] for t in terms]
    _lib.check(_lib.lib().tgcn_set_tuning(b"project_variant", variant))
    if bf16:
        return F.cheb_project_bf16(tv, _dev(W).to(dt), None if bias is None else _dev(bias), F.BIAS_CHANNEL if bias is not None else F.BIAS_NONE,
                                   terms[0].shape[0], out_dtype=torch.float32)
    return F.cheb_project(tv, _dev(W), None if bias is None else _dev(bias), F.BIAS_CHANNEL if bias is not None else F.BIAS_NONE, terms[0].shape[0])


@pytest.mark.parametrize("variant", EXACT_VARIANTS)
@pytest.mark.parametrize("N", [3, 16, 70])
@pytest.mark.parametrize("Kc", [3, 33, 64])
def test_project_exact_variants(Kc, N, variant, gpu_device):
    """the exact-fp32 projection kernels: NaN at A[0][0][0], +Inf in row 64 of term 2, -Inf at A[1][129][Kc-1], lda > Kc with NaN padding;
    every row without a poison is finite and accurate, the poisoned rows have the reference's classes.
    Which kernel a variant reaches at M = 130 rows and three terms, by project_choose (tgcn_hip.hip): the weight image, 3 * ceil4(Kc) * nt * 64
    bytes, is at most 48 KB here, under the 80 KB limit, so variants 0, 2 and 4 all take the W-resident kernel (auto leaves it for the
    vector-ALU kernel from 4096 rows and for bf16x3 from 8192 only); variant 1 takes the exact streaming-W kernel at every shape; variant 5
    takes the vector-ALU kernel where nterms * Kc <= 16 and N % 4 == 0 -- (Kc, N) = (3, 16) alone -- and the W-resident kernel elsewhere.
    Three distinct kernels, then: W-resident (scalar loads at Kc = 3 and 33, 16-byte loads at 64), streaming-W, and vector-ALU in one case.
    The bf16x3 kernels are variant 3 (tiled, and wide from 96 columns) and variant 6 (streaming), tested below."""
    terms, W, bias, ref = project_case(Kc, N)
    out = _project(terms, W, bias, variant)
    R.assert_matches(_np(out), ref, TOL, "cheb_project variant %d Kc=%d N=%d" % (variant, Kc, N))


@pytest.mark.parametrize("N", [3, 16, 70])
@pytest.mark.parametrize("Kc", [3, 33, 64])
def test_project_bf16(Kc, N, gpu_device):
    """F.cheb_project_bf16 (fp32 output): Inf and NaN are bf16 values, the products are exact, the k tail of the last 32-wide step reads zeros"""
    terms, W, bias, ref = project_case(Kc, N)
    out = _project(terms, W, bias, 0, bf16=True)
    R.assert_matches(_np(out), ref, TOL, "cheb_project_bf16 Kc=%d N=%d" % (Kc, N))


@pytest.mark.parametrize("N", [3, 16, 70, 130])
@pytest.mark.parametrize("Kc", [3, 33, 64])
def test_project_bf16x3_pinned_deviation(Kc, N, gpu_device):
    """DOCUMENTED DEVIATION, pinned: the bf16x3 kernels split a = a1 + a2 + a3 with a1 = bf16(a); for a = +-Inf the
    residual a - a1 is NaN, so a row that holds +-Inf comes out NaN in EVERY column where the exact product has the sign of the Inf.
    What stays: a NaN row is NaN, locality -- a poisoned row never touches another row -- and the accuracy of every clean row.  N = 130
    reaches the wide form (A fragments from registers)."""
    terms, W, bias, ref = project_case(Kc, N)
    out = _np(_project(terms, W, bias, X3_VARIANT))
    want = ref.copy()
    want[list(R.PROJECT_POISON_ROWS)] = NAN
    R.assert_matches(out, want, TOL, "bf16x3 Kc=%d N=%d" % (Kc, N))


@pytest.mark.parametrize("variant", EXACT_VARIANTS + (X3_VARIANT,))
@pytest.mark.parametrize("Kc,N", [(3, 16), (33, 3), (64, 70)])
def test_project_large_finite_inputs(Kc, N, variant, gpu_device):
    """a finite row at 3.0e38 and one at FLT_MAX against weights of 1e-3: every exact product and sum is finite.  The exact kernels return
    them; bf16x3 (pinned deviation) returns the 3.0e38 row, which bf16 still holds, and NaN for the FLT_MAX row: bf16(FLT_MAX) is Inf and the
    residual -Inf.  Every other row is finite and accurate either way."""
    terms, W, ref = project_large_case(Kc, N)
    out = _np(_project(terms, W, None, variant))
    want = ref.copy()
    if variant == X3_VARIANT:
        want[100] = NAN
    R.assert_matches(out, want, TOL, "large inputs variant %d" % variant)
    small = np.ones(ref.shape[0], bool)
    small[[7, 100]] = False
    assert rel_err(out[small], ref[small]) <= TOL                      # the O(1) rows by their own scale, not the 1e35 rows'


def _wgrad_ref(terms, g, reverse=False):
    order = range(g.shape[0])[::-1] if reverse else range(g.shape[0])
    dW = np.zeros((len(terms), terms[0].shape[1], g.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for m in order:
            for t in range(len(terms)):
                dW[t] += np.asarray(terms[t][m], np.float64)[:, None] * g[m].astype(np.float64)[None, :]
    return dW


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", [3, 16, 70])
@pytest.mark.parametrize("Kc", [3, 33, 64])
def test_project_weight_gradient(Kc, N, bf16, gpu_device):
    """F.cheb_wgrad / _bf16: dW[t, c, :] = sum_m A_t[m, c] G[m, :] with the poisons of project_case in A: exactly dW[0, 0], dW[1, Kc-1] and
    dW[2] are non-finite, with the reference's classes; dW[3] and the rest of dW[0], dW[1] are finite and accurate"""
    from tgcn_amd import functional as F
    terms, W, bias, _ = project_case(Kc, N, nterms=4)        # four terms: at Kc = 3 more than half of dW stays finite
    g = np.random.default_rng([Kc, N]).choice([-1.5, -1.0, -0.5, 0.5, 1.0, 1.5], (terms[0].shape[0], N)).astype(np.float32)
    ref = R.order_checked(lambda rev: _wgrad_ref(terms, g, rev), "wgrad")
    R.check_coverage(ref, "wgrad Kc=%d N=%d" % (Kc, N), neighbour_axis=1)
    nonfin = (R.cls(ref) != R.FIN).all(axis=2)
    want = np.zeros(nonfin.shape, bool)
    want[0, 0], want[1, Kc - 1], want[2, :] = True, True, True
    assert np.array_equal(nonfin, want)
    dt = torch.bfloat16 if bf16 else torch.float32
    tv = [_padded_rows(t, _lda(Kc) + (4 if bf16 else 0), dt)[0] for t in terms]
    gv, _ = _padded_rows(g, N + 5, dt)
    dW = (F.cheb_wgrad_bf16 if bf16 else F.cheb_wgrad)(tv, gv)
    R.assert_matches(_np(dW), ref, TOL_GRAD, "wgrad %s Kc=%d N=%d" % (dt, Kc, N))


@pytest.mark.parametrize("Kc,N,K", [(3, 3, 2), (33, 16, 3), (64, 70, 2)])
def test_project_first(Kc, N, K, gpu_device):
    """F.project_first: Z = x . [W_0 | ... | W_{K-1}] with the bias on the first N columns, plain and through a row map; NaN at x[0][0][0],
    +Inf in one middle row, -Inf at the last element of the last row of the last sample"""
    from tgcn_amd import functional as F
    q, rows = 2, 130
    rng = np.random.default_rng([Kc, N, K])
    vals = np.array([-1.5, -1.0, -0.75, -0.5, 0.5, 0.75, 1.0, 1.5], np.float32)
    x = rng.choice(vals, (q, rows, Kc)).astype(np.float32)
    Wcat = rng.choice(vals, (Kc, K * N)).astype(np.float32)
    bias = rng.choice(vals, (N,)).astype(np.float32)
    x[0, 0, 0], x[0, 64, :], x[q - 1, rows - 1, Kc - 1] = NAN, R.INF, -R.INF
    R.check_inputs(x, Wcat, bias)
    fullb = np.concatenate([bias, np.zeros((K - 1) * N, np.float32)])
    ref = np.stack([R.order_checked(lambda rev: R.project_ref([x[b]], Wcat[None], fullb, reverse=rev), "project_first") for b in range(q)])
    R.check_coverage(ref, "project_first", neighbour_axis=1)
    assert (R.cls(ref) != R.FIN).any(axis=2).sum() == 3
    Z = F.project_first(_dev(x), _dev(Wcat), _dev(bias), F.BIAS_CHANNEL, K, N)
    R.assert_matches(_np(Z), ref, TOL, "project_first Kc=%d N=%d K=%d" % (Kc, N, K))
    perm = rng.permutation(rows).astype(np.int32)                  # output row of input row m
    Zm = F.project_first(_dev(x), _dev(Wcat), _dev(bias), F.BIAS_CHANNEL, K, N, rowmap=_dev(perm))
    want = np.empty_like(ref)
    want[:, perm] = ref
    R.assert_matches(_np(Zm), want, TOL, "project_first mapped")



def _has_x3_stream(Kc, N):
    """the dispatch's rule for the streaming bf16x3 kernel (project_choose): rows of 32 / 64 floats, at most 64 columns, the vector
    epilogue (N % 4 == 0) and 16-byte aligned operands, which every case here has.  test_project_variant_6 holds the library to it through
    tgcn_cheb_project_stream_f32, which runs that kernel or refuses."""
    return Kc in (32, 64) and N <= 64 and N % 4 == 0


def _x3_pin(ref, rows):
    want = ref.copy()
    want[..., rows, :] = NAN
    return want


@pytest.mark.parametrize("N", [3, 16, 64])
@pytest.mark.parametrize("Kc", [32, 33, 64])
def test_project_variant_6(Kc, N, gpu_device):
    """"project_variant" 6: the streaming bf16x3 kernel (project_x3_stream_kernel, the headline's projection) wherever the shape has it, at
    M = 130 rows too.  Which shapes have it is asked of the library: tgcn_cheb_project_stream_f32 forces that kernel and answers
    TGCN_ERR_UNSUPPORTED where it does not exist; where it exists, variant 6 gives the same bits, and they are the bf16x3 deviation (a row
    holding +-Inf is NaN in every column, split3); elsewhere variant 6 falls to an exact kernel and the reference's classes hold.  The
    large finite inputs likewise: FLT_MAX gives a NaN row on the bf16x3 kernel, 3.0e38 is accurate."""
    from tgcn_amd import _lib, functional as F
    terms, W, bias, ref = project_case(Kc, N)
    M = terms[0].shape[0]
    tv = [_padded_rows(t, _lda(Kc))[0] for t in terms]
    Wd, bd = _dev(W.reshape(3 * Kc, N)), _dev(bias)
    a = (C.c_void_p * 3)(*[t.data_ptr() for t in tv])
    lda = (C.c_int64 * 3)(*[t.stride(0) for t in tv])
    forced = torch.full((M, N), NAN, device="cuda")
    rc = _lib.lib().tgcn_cheb_project_stream_f32(_lib.stream_ptr(), M, Kc, N, 3, a, lda, _lib.ptr(Wd), _lib.ptr(bd), F.BIAS_CHANNEL, M, None, 0, 1, None, 0,
                                                 _lib.ptr(forced), N, None)
    assert rc == (0 if _has_x3_stream(Kc, N) else -4), (rc, Kc, N)
    out = _project(terms, W, bias, 6)
    if _has_x3_stream(Kc, N):
        assert torch.equal(out.view(torch.int32), forced.view(torch.int32))
        R.assert_matches(_np(out), _x3_pin(ref, list(R.PROJECT_POISON_ROWS)), TOL, "variant 6, bf16x3 stream Kc=%d N=%d" % (Kc, N))
    else:
        assert torch.isnan(forced).all()
        R.assert_matches(_np(out), ref, TOL, "variant 6, exact Kc=%d N=%d" % (Kc, N))
    terms, W, ref = project_large_case(Kc, N)
    out = _np(_project(terms, W, None, 6))
    R.assert_matches(out, _x3_pin(ref, [100]) if _has_x3_stream(Kc, N) else ref, TOL, "variant 6, large inputs Kc=%d N=%d" % (Kc, N))
    small = np.ones(ref.shape[0], bool)
    small[[7, 100]] = False
    assert rel_err(out[small], ref[small]) <= TOL


mapped_case = functools.lru_cache(maxsize=None)(R.mapped_case)
MAPPED_SHAPES = [(3, 3), (33, 16), (32, 16), (64, 64), (64, 70)]


def _mapped_expect(out, ref, rowmap, pinned, tol, what):
    """out (q, n_vertices, N) pre-filled with 7: tile row m at vertex rowmap[m], every vertex the map does not name untouched"""
    out = _np(out)
    want = _x3_pin(ref, [0, 64, R.MAPPED_M - 1]) if pinned else ref
    if pinned:
        want[0] = ref[0]                       # sample 0 holds no poison
    R.assert_matches(out[:, rowmap], want, tol, what)
    rest = np.ones(out.shape[1], bool)
    rest[rowmap] = False
    assert (out[:, rest] == 7.0).all(), what + ": a vertex the map does not name was written"


@pytest.mark.parametrize("variant", [4, 3, 6], ids=["exact", "bf16x3", "variant6"])
@pytest.mark.parametrize("Kc,N", MAPPED_SHAPES)
def test_project_mapped_fp32(Kc, N, variant, gpu_device):
    """tgcn_cheb_project_mapped_f32 (F.project_mapped): a permuted row map over 130 of 200 vertices, term 0 read through the map, two
    compact terms read at the tile row, two samples in one call.  The poison rows land where the map puts them; a NaN vertex of term 0 that
    the map does not name reaches nothing.  Exact kernels: the reference's classes; the bf16x3 kernels (variant 3, and variant 6 where the
    streaming kernel exists): the pinned deviation."""
    from tgcn_amd import _lib, functional as F
    terms, W, bias, rowmap, ref = mapped_case(Kc, N)
    q = ref.shape[0]
    tv = [_guarded(t)[0] for t in terms]
    out = torch.full((q, R.MAPPED_NV, N), 7.0, device="cuda")
    _lib.check(_lib.lib().tgcn_set_tuning(b"project_variant", variant))
    F.project_mapped(tv, [R.MAPPED_NV * Kc, R.MAPPED_M * Kc, R.MAPPED_M * Kc], _dev(W.reshape(3 * Kc, N)), _dev(bias), F.BIAS_CHANNEL, R.MAPPED_NV,
                     _dev(rowmap), 1, q, out)
    pinned = variant == 3 or (variant == 6 and _has_x3_stream(Kc, N))
    _mapped_expect(out, ref, rowmap, pinned, TOL, "project_mapped variant %d Kc=%d N=%d" % (variant, Kc, N))


@pytest.mark.parametrize("Kc,N", MAPPED_SHAPES)
def test_project_mapped_bf16(Kc, N, gpu_device):
    """tgcn_cheb_project_mapped_bf16 (fp32 output) on the same map and poisons: Inf and NaN are bf16 values and the products exact"""
    from tgcn_amd import functional as F
    terms, W, bias, rowmap, ref = mapped_case(Kc, N)
    q = ref.shape[0]
    tv = [_guarded(t, torch.bfloat16)[0] for t in terms]
    out = torch.full((q, R.MAPPED_NV, N), 7.0, device="cuda")
    F.project_mapped_bf16(tv, [R.MAPPED_NV * Kc, R.MAPPED_M * Kc, R.MAPPED_M * Kc], _dev(W.reshape(3 * Kc, N)).bfloat16(), _dev(bias), F.BIAS_CHANNEL,
                          R.MAPPED_NV, _dev(rowmap), 1, q, out)
    _mapped_expect(out, ref, rowmap, False, TOL, "project_mapped_bf16 Kc=%d N=%d" % (Kc, N))


# ================================================================================================================ A3: time windows
series_case = functools.lru_cache(maxsize=None)(R.series_case)
POISON_TS = sorted(R.SERIES_POISON_T)


def _series_args(stack, W, bias):
    """(head, (W, bias, bias_kind), keep-alive) of an fp32 time-window entry: the stack is a view into a NaN-filled buffer, so the floats in
    front of the first and behind the last vertex row are NaN"""
    from tgcn_amd import _lib
    K, S, n, T, f = stack.shape
    H, N = W.shape[1], W.shape[3]
    sv, sbuf = _guarded(stack.reshape(K, S, n, T * f))
    Wd, bd = _dev(W.reshape(K, H * f, N)), _dev(bias.reshape(-1))
    return (_lib.stream_ptr(), S, n, T, f, H, N, K, _lib.ptr(sv)), (_lib.ptr(Wd), _lib.ptr(bd), 2), (sv, sbuf, Wd, bd)


def _call_series(entry, stack, W, bias, geom=(), nwin=None, window_major=False):
    """one forward entry (series / conv / dilated by the length of geom) -> (S, n, nwin, N) float64"""
    from tgcn_amd import _lib
    K, S, n, T, f = stack.shape
    N = W.shape[3]
    head, mid, keep = _series_args(stack, W, bias)
    out, obuf = _nan_out((S * nwin, n, N) if window_major else (S, n, nwin, N))
    _lib.check(getattr(_lib.lib(), entry)(*head, *mid, 0 if window_major else 1, _lib.ptr(out), *geom))
    assert _guards_untouched(obuf, out.numel())
    o = _np(out)
    return o.reshape(S, nwin, n, N).transpose(0, 2, 1, 3) if window_major else o


@pytest.mark.parametrize("t", POISON_TS)
@pytest.mark.parametrize("N", [3, 16])
@pytest.mark.parametrize("f,H", R.SERIES_FH)
def test_series_forward(f, H, N, t, gpu_device):
    """tgcn_cheb_project_series_f32 in both output layouts: every window whose taps do not include the poisoned time row is finite and
    accurate, the others have the reference's classes.  H*f mod 4 != 0 is the ragged last k step of the scalar-load form, whose A side used
    to read the first floats of the time row BEHIND the window (zero weight rows cancel those only while they are finite)."""
    stack, W, bias, ref, touched = series_case(f, H, N, t, R.SERIES_POISON_T[t])
    for wm in (False, True):
        out = _call_series("tgcn_cheb_project_series_f32", stack, W, bias, nwin=ref.shape[2], window_major=wm)
        R.assert_matches(out, ref, TOL, "series f=%d H=%d N=%d t=%d window_major=%s" % (f, H, N, t, wm))


GEOMS = [dict(stride=2, padl=2, padr=1), dict(padl=4), dict(dil=2, padl=3, padr=1), dict(dil=3), dict(dil=2, padl=8)]


@pytest.mark.parametrize("t", POISON_TS)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "_".join("%s%d" % kv for kv in g.items()))
@pytest.mark.parametrize("f,H", [(1, 5), (3, 7), (2, 3), (5, 3), (8, 5)])
def test_series_conv_and_dilated(f, H, geom, t, gpu_device):
    """the _conv entry (a window step, zero padding on both sides) and the _dilated entry (dilation 2 and 3): the zero padding is an absent
    term and the rows between two taps belong to other windows"""
    stride, padl, padr, dil = geom.get("stride", 1), geom.get("padl", 0), geom.get("padr", 0), geom.get("dil", 1)
    if padl > (H - 1) * dil:
        padl = (H - 1) * dil
    stack, W, bias, ref, touched = series_case(f, H, 3, t, R.SERIES_POISON_T[t], stride=stride, padl=padl, padr=padr, dil=dil)
    if dil == 1:
        out = _call_series("tgcn_cheb_project_series_conv_f32", stack, W, bias, (stride, padl, padr), ref.shape[2])
    else:
        out = _call_series("tgcn_cheb_project_series_dilated_f32", stack, W, bias, (stride, padl, padr, dil), ref.shape[2])
    R.assert_matches(out, ref, TOL, "conv/dilated f=%d H=%d %s t=%d" % (f, H, geom, t))


def test_series_forward_chunked_horizon(gpu_device):
    """HC < H: the horizon staged in chunks of weight time rows (f = 66, H = 40: the plan is asserted), scalar loads, a ragged last k step in
    every chunk -- each chunk's tail lies in front of time rows of later windows"""
    from test_series_channels_regimes import series_plan
    f, H, N, T, t = 66, 40, 10, 80, 60
    rc, hc, lds = series_plan(H, f, N)
    assert rc == 0 and 1 <= hc < H and (hc * f) % 4 != 0, (rc, hc, lds)
    stack, W, bias, ref, touched = series_case(f, H, N, t, R.INF, T=T)
    assert touched.sum() == 20 and not touched[:21].any()
    out = _call_series("tgcn_cheb_project_series_f32", stack, W, bias, nwin=ref.shape[2])
    R.assert_matches(out, ref, TOL, "chunked horizon")


@pytest.mark.parametrize("pool", [2, 4])
@pytest.mark.parametrize("t", POISON_TS)
@pytest.mark.parametrize("f,H,dil", [(1, 5, 1), (3, 7, 1), (2, 3, 2), (4, 3, 1)])
def test_series_pool_forward(f, H, dil, t, pool, gpu_device):
    """tgcn_cheb_project_series_pool_f32 (n = 8): relu + max over the vertices of a group of the reference's output, by the rule"""
    from tgcn_amd import _lib
    N, n = 3, 8
    stack, W, bias, ref, touched = series_case(f, H, N, t, R.SERIES_POISON_T[t], n=n, dil=dil)
    S, nwin = ref.shape[0], ref.shape[2]
    zref = R.pool_rule(ref.reshape(S, n, nwin * N), pool)[0].reshape(S, n // pool, nwin, N)
    clean = np.ones(ref.shape[:3], bool)
    clean[R.POISON_AT[1], R.POISON_AT[2], touched] = False
    assert np.array_equal((R.cls(zref) == R.FIN).all(axis=3) | ~clean.reshape(S, n // pool, pool, nwin).all(axis=2), np.ones(zref.shape[:3], bool))
    head, mid, keep = _series_args(stack, W, bias)
    z, zbuf = _nan_out(zref.shape)
    idx = torch.full(zref.shape, 255, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().tgcn_cheb_project_series_pool_f32(*head, *mid, 1, _lib.ptr(z), _lib.ptr(idx), pool, 1, 0, 0, dil))
    R.assert_matches(_np(z), zref, TOL, "series pool f=%d H=%d dil=%d t=%d pool=%d" % (f, H, dil, t, pool))
    assert _guards_untouched(zbuf, z.numel()) and int(idx.max()) < pool


def _stream_case(f, H, N, dil, where, n=5):
    """a chunk of Tc = 48 time rows behind C = (H-1)*dil ring rows; where: a chunk row >= 0 or a ring row < 0 to poison.
    -> (whole stack (K, S, n, C + Tc, f), W, bias, ref (S, n, Tc, N), C)"""
    Cr, Tc = (H - 1) * dil, R.SERIES_T
    value = R.SERIES_POISON_T.get(where, NAN if where % 2 else R.INF)
    stack, W, bias, ref, touched = series_case(f, H, N, Cr + where, value, n=n, T=Cr + Tc, dil=dil)
    assert ref.shape[2] == Tc
    return stack, W, bias, ref, Cr


def _stream_args(stack, W, bias, Cr, head_slot):
    """the chunk's stack and the ring (ring_ld > C*f, NaN behind the slots) of a stream entry"""
    from tgcn_amd import _lib
    K, S, n, Tall, f = stack.shape
    H, N = W.shape[1], W.shape[3]
    Tc = Tall - Cr
    sv, sbuf = _guarded(np.ascontiguousarray(stack[:, :, :, Cr:]).reshape(K, S, n, Tc * f))
    ring_ld = Cr * f + (4 if f % 4 == 0 else 3)
    ring = _dev(R.ring_of(stack[:, :, :, :Cr], head_slot, ring_ld))
    Wd, bd = _dev(W.reshape(K, H * f, N)), _dev(bias.reshape(-1))
    head = (_lib.stream_ptr(), S, n, Tc, f, H, N, K, _lib.ptr(sv), _lib.ptr(Wd), _lib.ptr(bd), 2)
    return head, ring, ring_ld, (sv, sbuf, Wd, bd)


def _ring_after(stack, Cr, head_slot, ring_ld, Tc):
    """the ring the entry has to leave: the last C rows of the chunk, slot (head + Tc + j) mod C for the j-th of them"""
    return R.ring_of(stack[:, :, :, -Cr:], (head_slot + Tc) % Cr, ring_ld)


STREAM_WHERE = [20, 31, 32, R.SERIES_T - 1, -1, -2]      # chunk rows, then the ring: its newest row and the one before


@pytest.mark.parametrize("where", STREAM_WHERE)
@pytest.mark.parametrize("f,H,dil", [(1, 5, 1), (3, 7, 1), (2, 3, 2), (5, 3, 1), (1, 5, 2), (8, 5, 1)])
def test_series_stream_entries(f, H, dil, where, gpu_device):
    """tgcn_cheb_project_series_stream_f32, _pos_f32 and _at_f32 on one chunk behind a ring whose head is not slot 0: the poison in the chunk
    or in the ring; the ring afterwards holds the chunk's last C rows bit for bit (the poison included) and NaN padding untouched"""
    from tgcn_amd import _lib
    L = _lib.lib()
    N = 3
    stack, W, bias, ref, Cr = _stream_case(f, H, N, dil, where)
    S, n, Tc = ref.shape[:3]
    hs = 1 % Cr
    for kind in ("head", "pos", "at"):
        head, ring, ring_ld, keep = _stream_args(stack, W, bias, Cr, hs)
        if kind == "at":
            out, obuf = _nan_out((S, n, Tc + 5, N))
            _lib.check(L.tgcn_cheb_project_series_stream_at_f32(*head, _lib.ptr(out), Tc + 5, 3, 1, _lib.ptr(ring), ring_ld, hs, dil))
            assert torch.isnan(out[:, :, :3]).all() and torch.isnan(out[:, :, 3 + Tc:]).all()
            got = _np(out[:, :, 3:3 + Tc])
        else:
            out, obuf = _nan_out((S, n, Tc, N))
            if kind == "pos":
                pos = torch.tensor([hs, 7], dtype=torch.int64, device="cuda")
                _lib.check(L.tgcn_cheb_project_series_stream_pos_f32(*head, _lib.ptr(out), _lib.ptr(ring), ring_ld, _lib.ptr(pos), dil))
                assert pos.tolist() == [(hs + Tc) % Cr, 7 + Tc]
            else:
                _lib.check(L.tgcn_cheb_project_series_stream_f32(*head, _lib.ptr(out), _lib.ptr(ring), ring_ld, hs, dil))
            got = _np(out)
        R.assert_matches(got, ref, TOL, "stream %s f=%d H=%d dil=%d where=%d" % (kind, f, H, dil, where))
        assert _guards_untouched(obuf, out.numel())
        assert np.array_equal(ring.cpu().numpy(), _ring_after(stack, Cr, hs, ring_ld, Tc), equal_nan=True), kind


@pytest.mark.parametrize("where", STREAM_WHERE)
@pytest.mark.parametrize("f,H", [(1, 5), (3, 7), (2, 3), (4, 3)])
def test_series_stream_strided_entry(f, H, where, gpu_device):
    """tgcn_cheb_project_series_stream_strided_f32 at window step 2 and 5 (below and above the horizon of H = 3), both phases of step 2:
    the rows between two windows of a span, and for step >= H the first row of the NEXT window, lie behind a window's last tap"""
    from tgcn_amd import _lib
    N = 3
    stack, W, bias, ref, Cr = _stream_case(f, H, N, 1, where)
    S, n, Tc = ref.shape[:3]
    hs = 1 % Cr
    for stride, off in ((2, 0), (2, 1), (5, 3)):
        head, ring, ring_ld, keep = _stream_args(stack, W, bias, Cr, hs)
        want = ref[:, :, off::stride]
        out, obuf = _nan_out(want.shape)
        _lib.check(_lib.lib().tgcn_cheb_project_series_stream_strided_f32(*head, _lib.ptr(out), _lib.ptr(ring), ring_ld, hs, None, stride, off))
        R.assert_matches(_np(out), want, TOL, "strided f=%d H=%d where=%d step=%d off=%d" % (f, H, where, stride, off))
        assert _guards_untouched(obuf, out.numel())
        assert np.array_equal(ring.cpu().numpy(), _ring_after(stack, Cr, hs, ring_ld, Tc), equal_nan=True)


@pytest.mark.parametrize("where", STREAM_WHERE)
@pytest.mark.parametrize("f,H,dil", [(1, 5, 1), (3, 7, 1), (2, 3, 2), (4, 3, 1)])
def test_series_stream_pool_entry(f, H, dil, where, gpu_device):
    """tgcn_cheb_project_series_stream_pool_f32 (n = 8, pool 2 and 4, the host's head and the device position)"""
    from tgcn_amd import _lib
    N, n = 3, 8
    stack, W, bias, ref, Cr = _stream_case(f, H, N, dil, where, n=n)
    S, _, Tc = ref.shape[:3]
    hs = 1 % Cr
    for pool, use_pos in ((2, False), (4, True)):
        zref = R.pool_rule(ref.reshape(S, n, Tc * N), pool)[0].reshape(S, n // pool, Tc, N)
        head, ring, ring_ld, keep = _stream_args(stack, W, bias, Cr, hs)
        z, zbuf = _nan_out(zref.shape)
        pos = torch.tensor([hs, 0], dtype=torch.int64, device="cuda") if use_pos else None
        _lib.check(_lib.lib().tgcn_cheb_project_series_stream_pool_f32(*head, _lib.ptr(z), pool, _lib.ptr(ring), ring_ld, hs,
                                                                       _lib.ptr(pos) if use_pos else None, dil))
        R.assert_matches(_np(z), zref, TOL, "stream pool f=%d H=%d dil=%d where=%d pool=%d" % (f, H, dil, where, pool))
        assert _guards_untouched(zbuf, z.numel())
        assert np.array_equal(ring.cpu().numpy(), _ring_after(stack, Cr, hs, ring_ld, Tc), equal_nan=True)


def _bf16_ld(Tf):
    return (Tf + 7) // 8 * 8 + 8          # > T*f, a multiple of 8: the 16-byte form stays reachable


@pytest.mark.parametrize("t", POISON_TS)
@pytest.mark.parametrize("geom", [dict(), dict(stride=2, padl=2, padr=1), dict(dil=2, padl=3, padr=1)], ids=["plain", "step2", "dil2"])
@pytest.mark.parametrize("f,H", [(1, 5), (3, 7), (5, 3), (8, 5)])
def test_series_bf16_forward(f, H, geom, t, gpu_device):
    """the bf16 twins (_conv_bf16 / _dilated_bf16): vertex rows stack_ld > T*f elements apart with NaN padding, operands exact in bf16"""
    from tgcn_amd import _lib
    N = 3
    stride, padl, padr, dil = geom.get("stride", 1), geom.get("padl", 0), geom.get("padr", 0), geom.get("dil", 1)
    padl = min(padl, (H - 1) * dil)
    stack, W, bias, ref, touched = series_case(f, H, N, t, R.SERIES_POISON_T[t], stride=stride, padl=padl, padr=padr, dil=dil)
    K, S, n, T, _ = stack.shape
    ld = _bf16_ld(T * f)
    sv, sbuf = _padded_rows(stack.reshape(K, S, n, T * f), ld, torch.bfloat16)
    Wd, bd = _dev(W.reshape(K, H * f, N)).bfloat16(), _dev(bias.reshape(-1))
    out, obuf = _nan_out(ref.shape, torch.bfloat16)
    head = (_lib.stream_ptr(), S, n, T, f, H, N, K, _lib.ptr(sbuf), ld, _lib.ptr(Wd), _lib.ptr(bd), _lib.DTYPE_F32, 2, 1, _lib.ptr(out))
    if dil == 1:
        _lib.check(_lib.lib().tgcn_cheb_project_series_conv_bf16(*head, stride, padl, padr))
    else:
        _lib.check(_lib.lib().tgcn_cheb_project_series_dilated_bf16(*head, stride, padl, padr, dil))
    R.assert_matches(_np(out), ref, TOL_BF16, "series bf16 f=%d H=%d %s t=%d" % (f, H, geom, t))
    assert _guards_untouched(obuf, out.numel())


@pytest.mark.parametrize("where", STREAM_WHERE)
@pytest.mark.parametrize("f,H,dil", [(1, 5, 1), (3, 7, 1), (8, 5, 2)])
def test_series_stream_bf16_entry(f, H, dil, where, gpu_device):
    """tgcn_cheb_project_series_stream_bf16: chunk rows stack_ld apart, a bf16 ring with NaN behind its slots"""
    from tgcn_amd import _lib
    N = 3
    stack, W, bias, ref, Cr = _stream_case(f, H, N, dil, where)
    K, S, n, Tall, _ = stack.shape
    Tc, hs = Tall - Cr, 1 % Cr
    ld = _bf16_ld(Tc * f)
    sv, sbuf = _padded_rows(np.ascontiguousarray(stack[:, :, :, Cr:]).reshape(K, S, n, Tc * f), ld, torch.bfloat16)
    ring_ld = Cr * f + (8 if f % 8 == 0 else 3)
    ring = _dev(R.ring_of(stack[:, :, :, :Cr], hs, ring_ld)).bfloat16()
    Wd, bd = _dev(W.reshape(K, H * f, N)).bfloat16(), _dev(bias.reshape(-1))
    out, obuf = _nan_out(ref.shape, torch.bfloat16)
    _lib.check(_lib.lib().tgcn_cheb_project_series_stream_bf16(_lib.stream_ptr(), S, n, Tc, f, H, N, K, _lib.ptr(sbuf), ld, _lib.ptr(Wd), _lib.ptr(bd),
                                                               _lib.DTYPE_F32, 2, _lib.ptr(out), _lib.ptr(ring), ring_ld, hs, dil))
    R.assert_matches(_np(out), ref, TOL_BF16, "stream bf16 f=%d H=%d dil=%d where=%d" % (f, H, dil, where))
    assert _guards_untouched(obuf, out.numel())
    assert np.array_equal(ring.float().cpu().numpy(), _ring_after(stack, Cr, hs, ring_ld, Tc), equal_nan=True)


@pytest.mark.parametrize("t", [20, 31, 43])
@pytest.mark.parametrize("N", [3, 16])
@pytest.mark.parametrize("f,H", R.SERIES_FH)
def test_series_backward(f, H, N, t, gpu_device):
    """tgcn_cheb_series_backward_f32.  Poison in g (one window of one vertex, every column): the input gradient G -- the forward's kernel over g
    as a series of N channels, H*N mod 4 != 0 for N = 3 -- is non-finite exactly at the H time rows that window covers.  Poison in the stack
    (one time row): G does not read the stack and stays finite; dW is non-finite exactly in the poisoned term."""
    from tgcn_amd import _lib
    L = _lib.lib()
    stack, W, bias, _, _ = series_case(f, H, N, 20, None)            # value None: a clean stack
    K, S, n, T, _ = stack.shape
    nwin = T - H + 1
    tw = min(t, nwin - 1)
    rng = np.random.default_rng([f, H, N, t])
    g = rng.choice([-1.5, -1.0, -0.5, 0.5, 1.0, 1.5], (S, n, nwin, N)).astype(np.float32)
    gp = g.copy()
    gp[1, 2, tw, :] = R.SERIES_POISON_T.get(t, R.INF)
    R.check_inputs(g)
    Gref = R.order_checked(lambda rev: R.series_dgrad_ref(gp, W, T, reverse=rev), "dgrad")
    R.check_coverage(Gref, "dgrad", neighbour_axis=3)
    want = np.zeros((S, n, T), bool)
    want[1, 2, tw:tw + H] = True
    assert np.array_equal((R.cls(Gref) != R.FIN).all(axis=(0, 4)), want) and np.array_equal((R.cls(Gref) != R.FIN).any(axis=(0, 4)), want)
    sp = stack.copy()
    sp[R.POISON_AT[0], R.POISON_AT[1], R.POISON_AT[2], t, :] = R.SERIES_POISON_T.get(t, R.INF)
    dWref = R.order_checked(lambda rev: R.series_wgrad_ref(sp, g, H, reverse=rev), "wgrad")
    R.check_coverage(dWref, "series wgrad")
    assert (R.cls(dWref[1 - R.POISON_AT[0]]) == R.FIN).all() and (R.cls(dWref[R.POISON_AT[0]]) != R.FIN).any()

    need = L.tgcn_cheb_series_backward_workspace_bytes(S, n, T, f, H, N, K)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    Wd = _dev(W.reshape(K, H * f, N))

    def run(st, gg, want_dW):
        sv, sbuf = _guarded(st.reshape(K, S, n, T * f))
        gv, gbuf = _guarded(gg)
        G, Gbuf = _nan_out((K, S, n, T * f))
        dW = torch.full((K, H * f, N), NAN, device="cuda") if want_dW else None
        _lib.check(L.tgcn_cheb_series_backward_f32(_lib.stream_ptr(), S, n, T, f, H, N, K, _lib.ptr(sv), _lib.ptr(gv), 1, _lib.ptr(Wd), _lib.ptr(G),
                                                   _lib.ptr(dW), _lib.ptr(ws), ws.numel()))
        assert _guards_untouched(Gbuf, G.numel())
        return _np(G).reshape(K, S, n, T, f), (None if dW is None else _np(dW).reshape(K, H, f, N))
    G, _ = run(stack, gp, False)
    R.assert_matches(G, Gref, TOL_GRAD, "G, poison in g: f=%d H=%d N=%d t=%d" % (f, H, N, t))
    G, dW = run(sp, g, True)
    R.assert_matches(G, R.series_dgrad_ref(g, W, T), TOL_GRAD, "G, poison in the stack")
    R.assert_matches(dW, dWref, TOL_GRAD, "dW, poison in the stack: f=%d H=%d N=%d t=%d" % (f, H, N, t))


@pytest.mark.parametrize("geom", [dict(stride=2, padl=2, padr=1), dict(stride=3, padl=0, padr=2), dict(dil=2, padl=3, padr=1), dict(dil=3)],
                         ids=lambda g: "_".join("%s%d" % kv for kv in g.items()))
@pytest.mark.parametrize("f,H,N", [(1, 5, 3), (3, 7, 3), (2, 3, 6), (4, 3, 16)])
def test_series_conv_and_dilated_backward(f, H, N, geom, gpu_device):
    """the input gradient of tgcn_cheb_series_conv_backward_f32 (one launch of the forward's kernel per phase of the window step, each over
    the weight time rows of its phase) and of _dilated_backward_f32, with one window of g poisoned: G is non-finite exactly at the taps of
    that window that lie inside the recording"""
    from tgcn_amd import _lib
    L = _lib.lib()
    stride, padl, padr, dil = geom.get("stride", 1), geom.get("padl", 0), geom.get("padr", 0), geom.get("dil", 1)
    padl = min(padl, (H - 1) * dil)
    stack, W, bias, ref, _ = series_case(f, H, N, 20, None, stride=stride, padl=padl, padr=padr, dil=dil)
    K, S, n, T, _ = stack.shape
    nwin = ref.shape[2]
    for tw, value in ((nwin // 2, R.INF), (0, NAN), (nwin - 1, -R.INF)):
        g = np.random.default_rng([f, H, N, tw]).choice([-1.5, -1.0, -0.5, 0.5, 1.0, 1.5], (S, n, nwin, N)).astype(np.float32)
        g[1, 2, tw, :] = value
        Gref = R.order_checked(lambda rev: R.series_dgrad_ref(g, W, T, stride, padl, dil, reverse=rev), "dgrad")
        R.check_coverage(Gref, "dgrad %s" % geom, neighbour_axis=3)
        taps = tw * stride - padl + np.arange(H) * dil
        want = np.zeros((S, n, T), bool)
        want[1, 2, taps[(taps >= 0) & (taps < T)]] = True
        assert np.array_equal((R.cls(Gref) != R.FIN).any(axis=(0, 4)), want)
        gv, _ = _guarded(g)
        sv, _ = _guarded(stack.reshape(K, S, n, T * f))
        G, Gbuf = _nan_out((K, S, n, T * f))
        Wd = _dev(W.reshape(K, H * f, N))
        if dil == 1:
            need = L.tgcn_cheb_series_conv_backward_workspace_bytes(S, n, T, f, H, N, K, stride, padl, padr)
            ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
            _lib.check(L.tgcn_cheb_series_conv_backward_f32(_lib.stream_ptr(), S, n, T, f, H, N, K, _lib.ptr(sv), _lib.ptr(gv), 1, _lib.ptr(Wd), _lib.ptr(G), None,
                                                            _lib.ptr(ws), ws.numel(), stride, padl, padr))
        else:
            need = L.tgcn_cheb_series_dilated_backward_workspace_bytes(S, n, T, f, H, N, K, stride, padl, padr, dil)
            ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
            _lib.check(L.tgcn_cheb_series_dilated_backward_f32(_lib.stream_ptr(), S, n, T, f, H, N, K, _lib.ptr(sv), _lib.ptr(gv), 1, _lib.ptr(Wd), _lib.ptr(G), None,
                                                               _lib.ptr(ws), ws.numel(), stride, padl, padr, dil))
        R.assert_matches(_np(G).reshape(K, S, n, T, f), Gref, TOL_GRAD, "G f=%d H=%d N=%d %s window %d" % (f, H, N, geom, tw))
        assert _guards_untouched(Gbuf, G.numel())



def _series_backward_call(kind, stack, g, W, geom, want_dW, bf16=False):
    """one backward entry ("plain" / "conv" / "dilated"; bf16: the _bf16 twin of conv / dilated) -> (G (K, S, n, T, f), dW (K, H, f, N) or None);
    stack, g and G are views into NaN-filled buffers, the bf16 stack has rows stack_ld > T*f apart"""
    from tgcn_amd import _lib
    L = _lib.lib()
    K, S, n, T, f = stack.shape
    H, N = W.shape[1], W.shape[3]
    stride, padl, padr, dil = geom
    dt = torch.bfloat16 if bf16 else torch.float32
    if bf16:
        ld = _bf16_ld(T * f)
        sv = _padded_rows(stack.reshape(K, S, n, T * f), ld, dt)[1]
    else:
        sv = _guarded(stack.reshape(K, S, n, T * f))[0]
    gv, _ = _guarded(g, dt)
    Wd = _dev(W.reshape(K, H * f, N)).to(dt)
    G, Gbuf = _nan_out((K, S, n, T * f))
    dW = torch.full((K, H * f, N), NAN, device="cuda") if want_dW else None
    shape = (S, n, T, f, H, N, K)
    tail = {"plain": (), "conv": (stride, padl, padr), "dilated": (stride, padl, padr, dil)}[kind]
    name = {"plain": "tgcn_cheb_series_backward", "conv": "tgcn_cheb_series_conv_backward", "dilated": "tgcn_cheb_series_dilated_backward"}[kind]
    need = getattr(L, name + ("_bf16" if bf16 else "") + "_workspace_bytes")(*shape, *tail)
    assert need > 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    head = (_lib.stream_ptr(),) + shape + ((_lib.ptr(sv), ld) if bf16 else (_lib.ptr(sv),))
    _lib.check(getattr(L, name + ("_bf16" if bf16 else "_f32"))(*head, _lib.ptr(gv), 1, _lib.ptr(Wd), _lib.ptr(G), _lib.ptr(dW), _lib.ptr(ws), ws.numel(), *tail))
    assert _guards_untouched(Gbuf, G.numel())
    return _np(G).reshape(K, S, n, T, f), (None if dW is None else _np(dW).reshape(K, H, f, N))


BACKWARD_GEOMS = [("conv", (2, 2, 1, 1)), ("conv", (3, 0, 2, 1)), ("dilated", (1, 3, 1, 2)), ("dilated", (1, 0, 0, 3))]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,geom", BACKWARD_GEOMS, ids=["step2", "step3", "dil2", "dil3"])
@pytest.mark.parametrize("f,H,N", [(1, 5, 3), (3, 7, 3), (2, 3, 6), (8, 3, 16)])
def test_series_conv_and_dilated_backward_both_gradients(f, H, N, kind, geom, bf16, gpu_device):
    """tgcn_cheb_series_conv_backward_f32 / _dilated_backward_f32 and their _bf16 twins with BOTH gradients asked for.  Poison in g (one
    window): G is non-finite exactly at that window's taps inside the recording (dW, which sums over every window, is not asked for then).
    Poison in the stack (one time row of one term): G does not read the stack and stays finite and accurate, dW is non-finite in the
    poisoned term only, with the reference's classes."""
    stride, padl, padr, dil = geom
    padl = min(padl, (H - 1) * dil)
    geom = (stride, padl, padr, dil)
    stack, W, bias, ref, _ = series_case(f, H, N, 20, None, stride=stride, padl=padl, padr=padr, dil=dil)
    K, S, n, T, _ = stack.shape
    nwin = ref.shape[2]
    g = np.random.default_rng([f, H, N, stride, dil]).choice([-1.5, -1.0, -0.5, 0.5, 1.0, 1.5], (S, n, nwin, N)).astype(np.float32)
    gp = g.copy()
    gp[1, 2, nwin // 2, :] = R.INF
    Gref = R.order_checked(lambda rev: R.series_dgrad_ref(gp, W, T, stride, padl, dil, reverse=rev), "dgrad")
    R.check_coverage(Gref, "dgrad", neighbour_axis=3)
    G, _ = _series_backward_call(kind, stack, gp, W, geom, False, bf16)
    R.assert_matches(G, Gref, TOL_GRAD, "G, poison in g: %s %s f=%d H=%d N=%d" % (kind, geom, f, H, N))
    sp = stack.copy()
    k0 = R.POISON_AT[0]
    sp[k0, R.POISON_AT[1], R.POISON_AT[2], 20, :] = NAN
    dWref = R.order_checked(lambda rev: R.series_wgrad_ref(sp, g, H, stride, padl, dil, reverse=rev), "wgrad")
    R.check_coverage(dWref, "series wgrad")
    assert (R.cls(dWref[1 - k0]) == R.FIN).all() and (R.cls(dWref[k0]) != R.FIN).any()
    G, dW = _series_backward_call(kind, sp, g, W, geom, True, bf16)
    R.assert_matches(G, R.series_dgrad_ref(g, W, T, stride, padl, dil), TOL_GRAD, "G, poison in the stack")
    R.assert_matches(dW, dWref, TOL_GRAD, "dW, poison in the stack: %s %s f=%d H=%d N=%d" % (kind, geom, f, H, N))


CHUNK_G = dict(g_T=60, g_t0=5)


@pytest.mark.parametrize("where", ["g_in_chunk", "g_behind_chunk", "g_before_chunk", "stack_row", "ring_row"])
@pytest.mark.parametrize("f,H,N,dil", [(1, 5, 3, 1), (3, 7, 3, 1), (2, 3, 3, 2), (4, 3, 16, 1), (1, 5, 16, 2)])
def test_series_chunk_backward(f, H, N, dil, where, gpu_device):
    """tgcn_cheb_series_chunk_backward_f32, the backward of forward_series(time_chunk=): a chunk of 48 rows behind a ring of C rows, g the
    whole output gradient of 60 rows read from row 5 on.  G is rows [5, 53) of the dilated backward on the whole g (its GEMM is the forward's
    kernel over g: H*N mod 4 != 0 at N = 3) -- a poisoned row of g inside the chunk or within C rows behind it reaches exactly its taps, one
    before the chunk reaches nothing; dW sums the windows that end in the chunk, rows before it from the ring -- a poisoned row of the
    stack or of the ring makes the poisoned term non-finite and no other; the ring afterwards holds the chunk's last C rows."""
    from tgcn_amd import _lib
    L = _lib.lib()
    Cr, Tc = (H - 1) * dil, R.SERIES_T
    g_T, g_t0 = CHUNK_G["g_T"], CHUNK_G["g_t0"]
    stack, W, bias, _, _ = series_case(f, H, N, 20, None, T=Cr + Tc, dil=dil)      # rows [0, C): the ring, oldest first; then the chunk
    K, S, n, _, _ = stack.shape
    g = np.random.default_rng([f, H, N, dil]).choice([-1.5, -1.0, -0.5, 0.5, 1.0, 1.5], (S, n, g_T, N)).astype(np.float32)
    k0, s0, i0 = R.POISON_AT
    if where.startswith("g_"):
        row = {"g_in_chunk": g_t0 + 20, "g_behind_chunk": g_t0 + Tc + 1, "g_before_chunk": g_t0 - 1}[where]
        g[s0, i0, row, :] = R.INF
    else:
        stack[k0, s0, i0, Cr + 20 if where == "stack_row" else Cr - 1, :] = NAN
    Gref = R.order_checked(lambda rev: R.series_dgrad_ref(g, W, g_T, 1, Cr, dil, reverse=rev), "chunk dgrad")[:, :, :, g_t0:g_t0 + Tc]
    if where in ("g_in_chunk", "g_behind_chunk"):
        R.check_coverage(Gref, "chunk dgrad " + where, neighbour_axis=3)
    else:
        assert (R.cls(Gref) == R.FIN).all()
    want_dW = not where.startswith("g_")
    hs = 1 % Cr
    sv, _ = _guarded(np.ascontiguousarray(stack[:, :, :, Cr:]).reshape(K, S, n, Tc * f))
    ring_ld = Cr * f + (4 if f % 4 == 0 else 3)
    ring = _dev(R.ring_of(stack[:, :, :, :Cr], hs, ring_ld))
    gv, _ = _guarded(g)
    Wd = _dev(W.reshape(K, H * f, N))
    G, Gbuf = _nan_out((K, S, n, Tc * f))
    dW = torch.full((K, H * f, N), NAN, device="cuda") if want_dW else None
    need = L.tgcn_cheb_series_chunk_backward_workspace_bytes(S, n, Tc, f, H, N, K, dil)
    assert need > 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    _lib.check(L.tgcn_cheb_series_chunk_backward_f32(_lib.stream_ptr(), S, n, Tc, f, H, N, K, _lib.ptr(sv), _lib.ptr(ring), ring_ld, hs, _lib.ptr(gv), g_T, g_t0, 1,
                                                     _lib.ptr(Wd), _lib.ptr(G), _lib.ptr(dW), _lib.ptr(ws), ws.numel(), dil))
    R.assert_matches(_np(G).reshape(K, S, n, Tc, f), Gref, TOL_GRAD, "chunk G %s f=%d H=%d N=%d dil=%d" % (where, f, H, N, dil))
    assert _guards_untouched(Gbuf, G.numel())
    if want_dW:
        gc = g[:, :, g_t0:g_t0 + Tc]
        dWref = R.order_checked(lambda rev: R.series_wgrad_ref(stack, gc, H, 1, 0, dil, reverse=rev), "chunk wgrad")
        R.check_coverage(dWref, "chunk wgrad")
        assert (R.cls(dWref[1 - k0]) == R.FIN).all() and (R.cls(dWref[k0]) != R.FIN).any()
        R.assert_matches(_np(dW).reshape(K, H, f, N), dWref, TOL_GRAD, "chunk dW %s f=%d H=%d N=%d dil=%d" % (where, f, H, N, dil))
    assert np.array_equal(ring.cpu().numpy(), _ring_after(stack, Cr, hs, ring_ld, Tc), equal_nan=True)


@pytest.mark.parametrize("where", STREAM_WHERE)
@pytest.mark.parametrize("f,H", [(1, 5), (3, 7), (8, 3)])
def test_series_stream_pos_and_strided_bf16_entries(f, H, where, gpu_device):
    """tgcn_cheb_project_series_stream_pos_bf16 (the ring position in device memory) and _stream_strided_bf16 (window step 2, both phases,
    and a step above the horizon): chunk rows stack_ld apart, a bf16 ring with NaN behind its slots"""
    from tgcn_amd import _lib
    L = _lib.lib()
    N = 3
    stack, W, bias, ref, Cr = _stream_case(f, H, N, 1, where)
    K, S, n, Tall, _ = stack.shape
    Tc, hs = Tall - Cr, 1 % Cr
    ld = _bf16_ld(Tc * f)
    ring_ld = Cr * f + (8 if f % 8 == 0 else 3)
    Wd, bd = _dev(W.reshape(K, H * f, N)).bfloat16(), _dev(bias.reshape(-1))
    for stride, off in ((1, 0), (2, 0), (2, 1), (9, 4)):
        sbuf = _padded_rows(np.ascontiguousarray(stack[:, :, :, Cr:]).reshape(K, S, n, Tc * f), ld, torch.bfloat16)[1]
        ring = _dev(R.ring_of(stack[:, :, :, :Cr], hs, ring_ld)).bfloat16()
        want = ref[:, :, off::stride]
        out, obuf = _nan_out(want.shape, torch.bfloat16)
        head = (_lib.stream_ptr(), S, n, Tc, f, H, N, K, _lib.ptr(sbuf), ld, _lib.ptr(Wd), _lib.ptr(bd), _lib.DTYPE_F32, 2, _lib.ptr(out), _lib.ptr(ring), ring_ld)
        if stride == 1:
            pos = torch.tensor([hs, 3], dtype=torch.int64, device="cuda")
            _lib.check(L.tgcn_cheb_project_series_stream_pos_bf16(*head, _lib.ptr(pos), 1))
            assert pos.tolist() == [(hs + Tc) % Cr, 3 + Tc]
        else:
            _lib.check(L.tgcn_cheb_project_series_stream_strided_bf16(*head, hs, None, stride, off))
        R.assert_matches(_np(out), want, TOL_BF16, "bf16 stream step=%d off=%d f=%d H=%d where=%d" % (stride, off, f, H, where))
        assert _guards_untouched(obuf, out.numel())
        assert np.array_equal(ring.float().cpu().numpy(), _ring_after(stack, Cr, hs, ring_ld, Tc), equal_nan=True)


# ================================================================================================================ A4: the relu / pool rule
@pytest.mark.parametrize("F_cols", [1, 3, 16])
@pytest.mark.parametrize("pool", [2, 4])
def test_relu_pool_and_pool_max_rule(pool, F_cols, gpu_device):
    """tgcn_relu_pool_f32 and tgcn_pool_max_f32 with their backwards on the crafted groups (an exact positive tie, a tie at 0, all negative,
    NaN at each member position, two NaNs, -Inf with finite values, +Inf, +Inf with NaN, -0.0): classes, values by == (so +-0 are equal),
    the arg-max exactly, and the gradient at that member and only there"""
    from tgcn_amd import _lib
    L = _lib.lib()
    y = R.pool_input(pool, F_cols)
    q, n, _ = y.shape
    yv, _ = _guarded(y)
    gz = np.arange(1, q * (n // pool) * F_cols + 1, dtype=np.float32).reshape(q, n // pool, F_cols)
    for relu in (True, False):
        zref, iref = R.pool_rule(y, pool, relu)
        z, zbuf = _nan_out(zref.shape)
        idx = torch.full(zref.shape, 99, dtype=torch.uint8 if relu else torch.int32, device="cuda")
        _lib.check((L.tgcn_relu_pool_f32 if relu else L.tgcn_pool_max_f32)(_lib.stream_ptr(), _lib.ptr(yv), _lib.ptr(z), _lib.ptr(idx), q, n, F_cols, pool))
        got = z.cpu().numpy()
        assert np.array_equal(R.cls(got), R.cls(zref)), R.class_mismatch(got, zref)
        fin = R.cls(zref) == R.FIN
        assert (got[fin] == zref[fin]).all() and _guards_untouched(zbuf, z.numel())
        assert np.array_equal(idx.cpu().numpy().astype(np.int64), iref.astype(np.int64))
        gy, gbuf = _nan_out(y.shape)
        gzd = _dev(gz)                 # held in a name: a temporary's memory may be handed out again before the kernel has read it
        if relu:
            _lib.check(L.tgcn_relu_pool_bwd_f32(_lib.stream_ptr(), _lib.ptr(gzd), _lib.ptr(z), _lib.ptr(idx), _lib.ptr(gy), q, n, F_cols, pool))
        else:
            _lib.check(L.tgcn_pool_max_bwd_f32(_lib.stream_ptr(), _lib.ptr(gzd), _lib.ptr(idx), _lib.ptr(gy), q, n, F_cols, pool))
        assert np.array_equal(gy.cpu().numpy(), R.pool_bwd_rule(gz, zref, iref, pool, relu)) and _guards_untouched(gbuf, gy.numel())


@pytest.mark.parametrize("pool", [2, 4])
def test_series_pool_epilogue_rule(pool, gpu_device):
    """the pooled epilogue of the time-window kernel (windows.h) on the crafted groups: one channel, one tap, one term, W = [[1]] and no
    bias, so the layer output IS the input (x * 1, no other term) and time plays the role of the columns; z and the arg-max bytes against the
    rule, and bit-identical to tgcn_relu_pool_f32"""
    from tgcn_amd import _lib
    L = _lib.lib()
    T = 40                                            # one full block of 32 windows plus a tail
    y = R.pool_input(pool, T)                         # (S, n, T): vertex groups x time
    S, n, _ = y.shape
    assert n % 4 == 0 or pool == 2
    zref, iref = R.pool_rule(y, pool)
    sv, _ = _guarded(y.reshape(1, S, n, T))
    W1 = torch.ones(1, device="cuda")
    z, zbuf = _nan_out((S, n // pool, T, 1))
    idx = torch.full((S, n // pool, T, 1), 99, dtype=torch.uint8, device="cuda")
    _lib.check(L.tgcn_cheb_project_series_pool_f32(_lib.stream_ptr(), S, n, T, 1, 1, 1, 1, _lib.ptr(sv), _lib.ptr(W1), None, 0, 1, _lib.ptr(z),
                                                   _lib.ptr(idx), pool, 1, 0, 0, 1))
    got = z.cpu().numpy()[..., 0]
    assert np.array_equal(R.cls(got), R.cls(zref)), R.class_mismatch(got, zref)
    fin = R.cls(zref) == R.FIN
    assert (got[fin] == zref[fin]).all() and _guards_untouched(zbuf, z.numel())
    assert np.array_equal(idx.cpu().numpy()[..., 0], iref)
    z2, i2 = torch.empty_like(z[..., 0]), torch.empty_like(idx[..., 0])
    _lib.check(L.tgcn_relu_pool_f32(_lib.stream_ptr(), _lib.ptr(sv), _lib.ptr(z2), _lib.ptr(i2), S, n, T, pool))
    assert torch.equal(z2.view(torch.int32), z[..., 0].contiguous().view(torch.int32)) and torch.equal(i2, idx[..., 0])


def _crafted_rows(pool, cols=6):
    """the crafted groups as a batch of single-channel samples: x (2 * cols, n, 1), group g of sample j in every rotation of pool_input"""
    y = R.pool_input(pool, cols)
    return np.ascontiguousarray(y.transpose(0, 2, 1)).reshape(2 * cols, y.shape[1], 1)


def _ring_operand(n):
    """a small sparse operand (a ring with self loops); the K = 1 layers below never apply it"""
    import tgcn_amd
    r = np.arange(n)
    row, col = np.concatenate([r, r, r]), np.concatenate([r, (r + 1) % n, (r - 1) % n])
    return tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(np.full(row.shape[0], 0.5, np.float32)))


def _assert_pool_rule(z, idx, zref, iref, what):
    got = z.cpu().numpy()
    assert np.array_equal(R.cls(got), R.cls(zref)), (what, R.class_mismatch(got, zref))
    fin = R.cls(zref) == R.FIN
    assert (got[fin] == zref[fin]).all(), what
    assert np.array_equal(idx.cpu().numpy(), iref), what


@pytest.mark.parametrize("narrow", [1, 0], ids=["input-side", "output-side"])
@pytest.mark.parametrize("pool", [2, 4])
def test_small_graph_pool_epilogue_rule(pool, narrow, gpu_device):
    """the two one-launch small-graph kernels with the relu + pool epilogue (small_graph.h; the "small_narrow" switch picks between them for
    one input channel) on the crafted groups: K = 1, one channel in, N output columns, W = all ones and no bias, so every column of the
    layer output IS the input (x * 1, no zero weight that would turn a NaN neighbour's product into the sum)"""
    from tgcn_amd import _lib, functional as F
    L = _lib.lib()
    x = _crafted_rows(pool)
    q, n, _ = x.shape
    op = _ring_operand(n)
    for N in (1, 3):
        assert L.tgcn_cheb_forward_small_pool_supported(op.n, op.nnz, 1, F.MODE_POWER) > 0
        zref, iref = R.pool_rule(np.repeat(x, N, axis=2), pool)
        z, zbuf = _nan_out(zref.shape)
        idx = torch.full(zref.shape, 99, dtype=torch.uint8, device="cuda")
        _lib.check(L.tgcn_set_tuning(b"small_narrow", narrow))
        xd, W1 = _dev(x), torch.ones(N, device="cuda")      # held in names: a temporary's memory may be handed out again before the launch
        _lib.check(L.tgcn_cheb_forward_small_pool_f32(_lib.stream_ptr(), C.byref(op.struct), F.MODE_POWER, 1, q, 1, N, _lib.ptr(xd),
                                                      _lib.ptr(W1), None, None, 0, 1, pool, _lib.ptr(z), _lib.ptr(idx)))
        _assert_pool_rule(z, idx, zref, iref, "small-graph pool %d narrow=%d N=%d" % (pool, narrow, N))
        assert _guards_untouched(zbuf, z.numel())


@pytest.mark.parametrize("variant,N", [(4, 4), (4, 64), (3, 16), (3, 64), (3, 96), (3, 112)],
                         ids=["exact_N4", "exact_N64", "bf16x3_N16", "bf16x3_N64", "bf16x3wide_N96", "bf16x3wide_N112"])
@pytest.mark.parametrize("pool", [2, 4])
def test_projection_pool_epilogue_rule(pool, variant, N, gpu_device):
    """F.cheb_forward_pool with the epilogue inside the projection (asserted through pool_epilogue_is_fused; row layout 0): the W-resident
    exact kernel, the bf16x3 kernel (N <= 64) and the wide bf16x3 kernel (N >= 96, four-float rows) on the crafted groups: K = 1, the
    crafted value in each of four input channels, W = all ones, no bias, so every output column is 4 x exactly (sums of equal small dyadic
    values) and the rule on 4 x is the rule on x.  bf16x3 turns an input of +-Inf into NaN (the pinned deviation of split3), so its
    reference is the rule applied to the input with +-Inf replaced."""
    from tgcn_amd import _lib, functional as F
    x = _crafted_rows(pool, cols=8)
    q, n, _ = x.shape
    op = _ring_operand(n)
    _lib.check(_lib.lib().tgcn_set_tuning(b"project_variant", variant))
    assert F.pool_epilogue_is_fused(op, q, 4, N, 1, pool, layout=0), "the shape is here for the fused epilogue"
    xin = np.where(np.isinf(x), np.float32(NAN), x) if variant == 3 else x
    zref, iref = R.pool_rule(np.repeat(4 * xin, N, axis=2), pool)
    z = torch.full(zref.shape, NAN, device="cuda")
    idx = torch.full(zref.shape, 99, dtype=torch.uint8, device="cuda")
    F.cheb_forward_pool(op, _dev(np.repeat(x, 4, axis=2)), torch.ones((4, N), device="cuda"), None, F.BIAS_NONE, F.MODE_POWER, 1, pool, z, idx,
                        layout=0)
    _assert_pool_rule(z, idx, zref, iref, "projection pool %d variant %d N=%d" % (pool, variant, N))


# ================================================================================================================ A5: small-graph kernels
def _bfs(A, start, hops):
    """bool[n]: the vertices i whose output reads x[start] within `hops` applications of the pattern A (out[i] reads x[j] for stored (i, j))"""
    reach = np.zeros(A.shape[0], bool)
    reach[start] = True
    for _ in range(hops):
        reach = reach | ((A @ reach.astype(np.float64)) > 0)
    return reach


def _expect_cone(out_c, out_p, s, cone, what):
    """out (q, n', N): NaN in every channel at (sample s, cone), bit-identical to the clean run everywhere else"""
    mask = np.zeros(out_c.shape[:2], bool)
    mask[s, cone] = True
    inside = torch.as_tensor(mask, device=out_p.device)
    assert out_p.shape == out_c.shape and mask.any()
    assert torch.isnan(out_p[inside]).all(), what + ": a finite value inside the cone"
    a, b = out_c[~inside].contiguous(), out_p[~inside].contiguous()
    bad = (a.view(torch.int32) != b.view(torch.int32)).nonzero() if a.dtype == torch.float32 else (a.view(torch.int16) != b.view(torch.int16)).nonzero()
    assert bad.numel() == 0, "%s: %d values outside the cone differ from the clean run, first at (sample, vertex) = %s" % (
        what, bad.shape[0], np.argwhere(~mask)[int(bad[0, 0])].tolist())
    assert not torch.isnan(a).any(), what


@functools.lru_cache(maxsize=None)
def _grid_operand(side=12):
    import tgcn_amd
    n = side * side
    r = np.arange(n)
    steps = ((0, np.ones(n, bool)), (1, r % side < side - 1), (-1, r % side > 0), (side, r < n - side), (-side, r >= side))     # self loop, E, W, S, N
    row = np.concatenate([r[ok] for _, ok in steps])
    col = np.concatenate([r[ok] + d for d, ok in steps])
    val = np.random.default_rng(side).choice([-0.5, -0.25, 0.25, 0.5], row.shape[0]).astype(np.float32)
    op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val))
    return op, O.coo_to_csr(row, col, val, n).astype(np.float64)


@pytest.mark.parametrize("mode", [0, 1], ids=["power", "chebyshev"])
@pytest.mark.parametrize("Crow,narrow", [(8, 1), (3, 1), (3, 0), (20, 1)], ids=["C8", "C3_input-side", "C3_output-side", "C20"])
def test_small_graph_sparse_kernels(Crow, narrow, mode, gpu_device):
    """cheb_forward_small and cheb_basis_small on a 12 x 12 grid held as CSR in LDS, three samples, NaN at one vertex of sample 1: samples 0
    and 2 are finite and accurate, sample 1 is NaN exactly inside the cone of K - 1 hops (per-entry propagation: no structural zero is
    multiplied) and bit-identical to the clean run outside; term k of the basis is NaN exactly within k hops"""
    from test_reordered_operands import _forward64, _stack
    from tgcn_amd import _lib, functional as F
    op, Lc = _grid_operand()
    assert op.dense is None and F.small_path_tile(op, Crow, mode) and F.small_basis_tile(op, Crow, mode)
    n, q, N, K, v0 = op.n, 3, 6, 3, 5 * 12 + 6
    rng = np.random.default_rng([Crow, mode])
    x = rng.standard_normal((q, n, Crow)).astype(np.float32)
    W = (rng.standard_normal((K, Crow, N)) / np.sqrt(K * Crow)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    xb = x.copy()
    xb[1, v0] = NAN
    A = abs(Lc)
    cone = _bfs(A, v0, K - 1)
    assert cone.sum() == 13                                          # the L1 ball of radius 2 in the grid
    _lib.check(_lib.lib().tgcn_set_tuning(b"small_narrow", narrow))
    fold = F.power_fold_matrix(K, "cuda") if mode == F.MODE_POWER else None
    run = lambda a: F.cheb_forward_small(op, _dev(a), _dev(W), fold, _dev(b), F.BIAS_CHANNEL, mode)
    out_c, out_p = run(x), run(xb)
    assert rel_err(out_c.cpu().numpy(), _forward64(Lc, x, W, b, mode)) <= TOL
    _expect_cone(out_c, out_p, 1, cone, "cheb_forward_small C=%d" % Crow)
    tc, tp = F.cheb_basis_small(op, _dev(x), K, mode), F.cheb_basis_small(op, _dev(xb), K, mode)
    mono = [x.astype(np.float64)]
    for _ in range(1, K):
        mono.append(O._apply(Lc, mono[-1]))
    ref = np.stack(mono) if mode == F.MODE_POWER else _stack(Lc, x, K, mode)
    for k in range(1, K):
        assert rel_err(tc[k].cpu().numpy(), ref[k]) <= TOL
        _expect_cone(tc[k], tp[k], 1, _bfs(A, v0, k), "cheb_basis_small term %d" % k)


@pytest.mark.parametrize("small_dense,q", [(2, 3), (1, 3), (0, 3), (2, 300), (1, 300)], ids=["auto_q3", "mfma_q3", "valu_q3", "x3_q300", "mfma_q300"])
def test_small_graph_dense_kernels_documented_deviation(small_dense, q, gpu_device):
    """DOCUMENTED DEVIATION, pinned: the 148-parcel DTI operand is held densely in LDS and multiplies structural zeros
    too, so one NaN activation makes EVERY vertex of that sample NaN ("small_dense" 2: bf16x3 when the batch fills the chip, 1: exact fp32
    MFMA, 0: the vector-ALU kernels, whose cone on this nearly complete graph is the whole sample as well).  The other samples are
    bit-identical to the clean run, finite and accurate."""
    import os
    from conftest import GOLDEN, load_golden
    from test_reordered_operands import _forward64
    import tgcn_amd
    from tgcn_amd import _lib, functional as F
    gd = load_golden(os.path.join(GOLDEN, "operand_dti148_lmax2.npz"))
    n = int(gd["n"])
    op = tgcn_amd.GraphOperand.from_coo(n, _dev(gd["a_row"]), _dev(gd["a_col"]), _dev(gd["a_val"]))
    Lc = O.coo_to_csr(gd["a_row"], gd["a_col"], gd["a_val"], n).astype(np.float64)
    Crow, N, K, mode = 15, 32, 4, F.MODE_POWER
    assert op.dense is not None and F.small_path_tile(op, Crow, mode)
    rng = np.random.default_rng(q)
    x = rng.standard_normal((q, n, Crow)).astype(np.float32)
    W = (rng.standard_normal((K, Crow, N)) / np.sqrt(K * Crow)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    xb = x.copy()
    xb[1, 77] = NAN
    _lib.check(_lib.lib().tgcn_set_tuning(b"small_dense", small_dense))
    fold = F.power_fold_matrix(K, "cuda")
    run = lambda a: F.cheb_forward_small(op, _dev(a), _dev(W), fold, _dev(b), F.BIAS_CHANNEL, mode)
    out_c, out_p = run(x), run(xb)
    assert rel_err(out_c.cpu().numpy(), _forward64(Lc, x, W, b, mode)) <= TOL
    _expect_cone(out_c, out_p, 1, np.ones(n, bool), "dense small operand, small_dense=%d q=%d" % (small_dense, q))


@pytest.mark.parametrize("which", ["grid", "dti"])
def test_small_graph_stream_kernel(which, gpu_device):
    """small_stream_kernel (forward_stream(fused=True): hops, projection and ring update of a chunk in one launch) on a batch of three
    recordings, NaN at one vertex of recording 1 at chunk row 10, H = 5: recordings 0 and 2 are bit-identical to the clean run and agree with
    the unfused step; recording 1 is NaN at rows 10 .. 14 exactly inside the cone of K - 1 hops on the grid, whose CSR the kernel holds, and
    at every vertex on the DTI operand, which it holds densely (the plan says which: the documented deviation); everything else of
    recording 1 is bit-identical to the clean run, and the ring, which keeps the last four hop rows, holds no NaN."""
    import os
    from conftest import GOLDEN, load_golden
    import tgcn_amd
    from tgcn_amd import functional as F
    if which == "grid":
        op, Lc = _grid_operand()
        v0 = 5 * 12 + 6
    else:
        gd = load_golden(os.path.join(GOLDEN, "operand_dti148_lmax2.npz"))
        op = tgcn_amd.GraphOperand.from_coo(int(gd["n"]), _dev(gd["a_row"]), _dev(gd["a_col"]), _dev(gd["a_val"] * 0.05))
        Lc, v0 = O.coo_to_csr(gd["a_row"], gd["a_col"], gd["a_val"] * 0.05, int(gd["n"])).astype(np.float64), 77
    n, S, Tc, f, g, K, H = op.n, 3, 16, 3, 6, 3, 5
    rc, tb, dense, lds = F._stream_small_plan(op, f, H, g, K, Tc, 1, F.MODE_POWER)
    assert rc == 0 and dense == (1 if which == "dti" else 0), (rc, tb, dense, lds)
    cone = np.ones(n, bool) if dense else _bfs(abs(Lc), v0, K - 1)
    assert dense or cone.sum() == 13
    torch.manual_seed(3)
    layer = tgcn_amd.TGCNCheb_H(op, f, g, K, H).cuda()
    x = np.random.default_rng(7).standard_normal((S, n, Tc, f)).astype(np.float32)
    xb = x.copy()
    xb[1, v0, 10, :] = NAN
    with torch.no_grad():
        (oc, sc), (ob, sb) = (layer.forward_stream(_dev(a), fused=True) for a in (x, xb))
        plain, _ = layer.forward_stream(_dev(x))
    assert rel_err(oc.cpu().numpy(), plain.cpu().numpy()) <= TOL
    _b3_expect(oc, ob, list(range(10, 10 + H)), np.nonzero(cone)[0], "small_stream_kernel " + which)
    assert not torch.isnan(sb.ring).any() and torch.equal(sb.ring, sc.ring)      # the ring keeps the hop rows 12 .. 15: none of them is row 10


# ================================================================================================================ B1 / B2: layers
@pytest.mark.parametrize("mode", [0, 1], ids=["power", "chebyshev"])
@pytest.mark.parametrize("case", ["small", "project_first", "hops_layout0", "hops_layout1", "hops_layout0_over_keep", "hops_layout1_over_keep",
                                  "compact", "compact_over_keep"])
def test_layer_locality_forward_and_backward(case, mode, gpu_device, monkeypatch):
    """F.cheb_layer on every layer path of tests/test_reordered_operands.py::LAYER_CASES (the path is asserted), inference and training
    forward, fp32 and bf16, plain and with relu + pool, each run clean and with NaN in all channels of one vertex of the last sample: inside
    the cone of K - 1 hops (breadth-first search on the pattern; with pooling: the groups that hold a cone vertex) every output is NaN,
    outside the poisoned run is BIT-IDENTICAL to the clean one, and the clean run meets 1e-5 against the fp64 oracle.
    Backward: NaN in grad_out at one (sample, vertex) makes dx NaN exactly in the cone of the transposed pattern in that sample and leaves
    every other dx bit-identical; dW and db are NaN throughout."""
    from test_reordered_operands import LAYER_CASES, _forward64, _graph, _operand
    from tgcn_amd import functional as F
    n, isolated, q, Crow, N, K, path_kind, layout, keep = LAYER_CASES[case]
    if keep is not None:
        monkeypatch.setattr(F, "KEEP_BASIS_BYTES", keep)
    op, Lc = _operand(n, isolated, None)
    if case == "small":
        K = 2          # three hops of this graph (300 vertices, 8 entries per row) reach every vertex: one hop leaves most of the sample outside
    path = F._layer_path(op, q, n, Crow, N, K, mode)
    assert path.kind == path_kind and (path_kind != "hops" or path.layout == layout), path
    row, col, _ = _graph(n, isolated)
    v0, s = int(row[row.shape[0] // 2]), q - 1
    A = abs(Lc).tocsr()
    whole = path.kind == "small" and op.dense is not None               # a dense operand in LDS: the documented deviation
    cone = np.ones(n, bool) if whole else _bfs(A, v0, K - 1)
    cone_t = np.ones(n, bool) if whole else _bfs(A.T.tocsr(), v0, K - 1)
    assert cone[v0] and cone.sum() >= 3 and (whole or (not cone.all() and not cone_t.all())), "no vertex outside the cone: locality would be vacuous"
    rng = np.random.default_rng([list(LAYER_CASES).index(case), mode, 5])
    x = rng.standard_normal((q, n, Crow)).astype(np.float32)
    W = (rng.standard_normal((K, Crow, N)) / np.sqrt(K * Crow)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    xb = x.copy()
    xb[s, v0] = NAN
    want = _forward64(Lc, x, W, b, mode)
    Wd, bd = _dev(W), _dev(b)

    with torch.no_grad():
        out_c, out_p = (F.cheb_layer(op, _dev(a), Wd, bd, F.BIAS_CHANNEL, mode) for a in (x, xb))
        assert rel_err(out_c.cpu().numpy(), want) <= TOL
        _expect_cone(out_c, out_p, s, cone, "inference")
        h_c, h_p = (F.cheb_layer_bf16(op, _dev(a).bfloat16(), Wd.bfloat16(), bd.bfloat16(), F.BIAS_CHANNEL, mode) for a in (x, xb))
        _expect_cone(h_c, h_p, s, cone, "bf16 inference")
        for pool in (2, 4):
            z_c, z_p = (F.cheb_relu_pool(op, _dev(a), Wd, bd, F.BIAS_CHANNEL, mode, pool) for a in (x, xb))
            assert rel_err(z_c.cpu().numpy(), np.maximum(want.reshape(q, n // pool, pool, N).max(axis=2), 0)) <= TOL
            _expect_cone(z_c, z_p, s, cone.reshape(n // pool, pool).any(axis=1), "relu + pool %d" % pool)

    # training forward (the basis may be kept) and the backward, clean and with NaN in grad_out
    g = rng.standard_normal((q, n, N)).astype(np.float32)
    gb = g.copy()
    gb[s, v0] = NAN
    grads = {}
    for name, xin, gin in (("clean", x, g), ("x", xb, None), ("g", x, gb)):
        leaves = [_dev(a).requires_grad_(True) for a in (xin, W, b)]
        out = F.cheb_layer(op, *leaves, F.BIAS_CHANNEL, mode)
        if gin is None:
            _expect_cone(grads["clean"][0], out.detach(), s, cone, "training forward")
            continue
        out.backward(_dev(gin))
        grads[name] = (out.detach(),) + tuple(t.grad for t in leaves)
    assert torch.equal(grads["clean"][0], grads["g"][0])
    _expect_cone(grads["clean"][1], grads["g"][1], s, cone_t, "dx")
    assert torch.isnan(grads["g"][2]).all() and torch.isnan(grads["g"][3]).all(), "dW and db of a NaN grad_out"
    assert not torch.isnan(grads["clean"][2]).any() and not torch.isnan(grads["clean"][3]).any()


# ================================================================================================================ B3: streaming layers
B3_T, B3_TC, B3_TSTAR, B3_H = 48, 16, 20, 5


@functools.lru_cache(maxsize=None)
def _b3_setup(f, K=3, g=6, n=64):
    """a TGCNCheb_H on a sparse symmetric pattern (n = 64, so the one-launch step fits), the series with and without NaN in every channel of
    vertex v0 of recording 1 at time t*, and the cone: the vertices within K-1 hops of v0"""
    import tgcn_amd
    rng = np.random.default_rng(100 + f)
    r0 = np.arange(n)
    row = np.concatenate([r0, (r0 + 1) % n, r0, r0])                  # a ring with self loops plus one chord per vertex, made symmetric
    col = np.concatenate([(r0 + 1) % n, r0, r0, (r0 * 7 + 3) % n])
    row, col = np.concatenate([row, col[3 * n:]]), np.concatenate([col, row[3 * n:]])
    val = rng.choice([-0.5, -0.25, 0.25, 0.5], row.shape[0]).astype(np.float32)
    adj = np.zeros((n, n), bool)
    adj[row, col] = True
    assert np.array_equal(adj, adj.T)
    v0, S = 10, 2
    reach = np.zeros(n, bool)
    reach[v0] = True
    for _ in range(K - 1):                                             # breadth-first: out[i] reads x[j] for every stored (i, j)
        reach = reach | adj[:, reach].any(axis=1)
    assert 3 <= reach.sum() <= n // 2 and (reach.reshape(n // 4, 4).any(axis=1).sum() < n // 4)
    op = tgcn_amd.GraphOperand.from_coo(n, _dev(row), _dev(col), _dev(val))
    torch.manual_seed(f)
    layer = tgcn_amd.TGCNCheb_H(op, f, g, K, B3_H).cuda()
    clean = rng.standard_normal((S, n, B3_T, f)).astype(np.float32)
    bad = clean.copy()
    bad[1, v0, B3_TSTAR, :] = NAN
    return layer, O.coo_to_csr(row, col, val, n), clean, bad, reach


def _b3_expect(out_c, out_p, nan_rows, cone, what):
    """out (S, n', T', g): NaN in every channel at (recording 1, cone vertex, nan_rows), bit-identical to the clean run everywhere else"""
    mask = np.zeros(out_c.shape[:3], bool)
    mask[1][np.ix_(cone, nan_rows)] = True
    assert mask.any() and not mask.all() and out_p.shape == out_c.shape
    inside = torch.as_tensor(mask, device=out_p.device)
    assert torch.isnan(out_p[inside]).all(), what + ": a finite value inside the cone"
    a, b = out_c[~inside].contiguous(), out_p[~inside].contiguous()
    bad = (a.view(torch.int32) != b.view(torch.int32)).nonzero()
    assert bad.numel() == 0, "%s: %d values outside the cone differ from the clean run, first at (s, i, t) = %s" % (
        what, bad.shape[0], np.argwhere(~mask)[int(bad[0, 0])].tolist())
    assert not torch.isnan(a).any()


@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("f", [1, 3, 4])
def test_streaming_layers_are_local_in_time_and_on_the_graph(f, dil, gpu_device):
    """forward_series (whole and time_chunk=16), forward_stream in chunks of 16 (plain, stride=2, fused=True, relu + pool) and GraphedStream
    on a causal TGCNCheb_H with H = 5: NaN at one vertex at t* = 20.  Outputs at times before t* -- in earlier chunks and in the same chunk --
    and after t* + (H-1)*dil are bit-identical to the clean run; so is everything outside the vertex cone, and between the taps of a dilated
    window; inside the cone the outputs at t* + h*dil are NaN.  Once the span is over the carried ring holds no NaN."""
    import tgcn_amd
    from tgcn_amd import functional as F
    from tgcn_amd.nn import GraphedStream, cheb_stream_relu_pool
    layer, Lcsr, clean, bad, reach = _b3_setup(f)
    cone = np.nonzero(reach)[0]
    S, n, T, _ = clean.shape
    g, K, H = layer.out_channels, layer.filter_order, B3_H
    Cr = (H - 1) * dil
    nan_t = [B3_TSTAR + h * dil for h in range(H)]
    assert nan_t[-1] < 2 * B3_TC                       # the span ends inside the second chunk: the third starts from a clean ring
    xc, xp = _dev(clean), _dev(bad)
    chunks = lambda x: [x[:, :, t0:t0 + B3_TC].contiguous() for t0 in range(0, T, B3_TC)]

    with torch.no_grad():
        # the whole causal series, against the fp64 oracle on the materialised (zero-padded, dilated) windows
        whole_c = layer.forward_series(xc, as_series=True, padding="causal", dilation=dil)
        padded = np.concatenate([np.zeros((S, n, Cr, f)), clean.astype(np.float64)], axis=2)
        xw = np.stack([padded[:, :, w:w + Cr + 1:dil] for w in range(T)], axis=1).reshape(S * T, n, H, f)
        ref = O.tgcn_cheb_h_forward(Lcsr, xw, layer.weight.detach().cpu().numpy(), layer.bias.detach().cpu().numpy())
        assert rel_err(whole_c.cpu().numpy(), ref.reshape(S, T, n, g).transpose(0, 2, 1, 3)) <= TOL
        _b3_expect(whole_c, layer.forward_series(xp, as_series=True, padding="causal", dilation=dil), nan_t, cone, "forward_series")
        tc_c = layer.forward_series(xc, as_series=True, padding="causal", dilation=dil, time_chunk=B3_TC)
        assert rel_err(tc_c.cpu().numpy(), whole_c.cpu().numpy()) <= TOL
        _b3_expect(tc_c, layer.forward_series(xp, as_series=True, padding="causal", dilation=dil, time_chunk=B3_TC), nan_t, cone, "time_chunk")

        def stream(x, **kw):
            """the recording chunk by chunk -> (outputs concatenated in time, the state's ring after the second chunk)"""
            outs, st, ring = [], None, None
            for j, ch in enumerate(chunks(x)):
                o, st = layer.forward_stream(ch, state=st, dilation=dil, **kw)
                outs.append(o)
                if j == 1:
                    ring = st.ring.clone()
            return torch.cat(outs, dim=2), ring

        variants = [("forward_stream", {})]
        if F.stream_fused_supported(layer._operand(xc.device), f, H, g, K, B3_TC, dil, F.MODE_POWER):
            variants.append(("fused", dict(fused=True)))
        else:
            pytest.fail("the one-launch step does not take n = %d: the case is there to run it" % n)
        for name, kw in variants:
            oc, ring_c = stream(xc, **kw)
            op_, ring_p = stream(xp, **kw)
            assert rel_err(oc.cpu().numpy(), whole_c.cpu().numpy()) <= TOL, name
            _b3_expect(oc, op_, nan_t, cone, name)
            assert not torch.isnan(ring_p).any(), name + ": a NaN is still in the ring after the last window that holds t*"
            assert torch.equal(ring_p, ring_c), name
        if dil == 1:                                   # a window step runs at dilation 1 only
            kw = dict(stride=2)
            oc, _ = stream(xc, **kw)
            op_, ring_p = stream(xp, **kw)
            assert torch.equal(oc, whole_c[:, :, ::2])
            _b3_expect(oc, op_, [t // 2 for t in nan_t if t % 2 == 0], cone, "stride=2")
            assert not torch.isnan(ring_p).any()

        # relu + pool: the cone is the pool groups that hold one of its vertices
        for pool in (2, 4):
            groups = np.nonzero(reach.reshape(n // pool, pool).any(axis=1))[0]

            def pooled(x):
                outs, st = [], None
                for ch in chunks(x):
                    o, st = cheb_stream_relu_pool(layer, ch, pool=pool, state=st, dilation=dil)
                    outs.append(o)
                return torch.cat(outs, dim=2), st.ring
            zc, _ = pooled(xc)
            zp, ring_p = pooled(xp)
            zr = R.pool_rule(whole_c.cpu().numpy().reshape(S, n, T * g), pool)[0].reshape(S, n // pool, T, g)
            assert np.array_equal(zc.cpu().numpy(), zr)
            _b3_expect(zc, zp, nan_t, groups, "relu + pool %d" % pool)
            assert not torch.isnan(ring_p).any()

    # GraphedStream: one captured step replayed for the three chunks
    def step(chunk, states):
        o, s = layer.forward_stream(chunk, state=states, dilation=dil, capturable=True)
        return o, s
    gs = GraphedStream(step, chunks(xc)[0])
    outs = {}
    for name, x in (("clean", xc), ("bad", xp)):
        gs.reset()
        outs[name] = torch.cat([gs(ch).clone() for ch in chunks(x)], dim=2)
    assert torch.equal(outs["clean"], whole_c) or rel_err(outs["clean"].cpu().numpy(), whole_c.cpu().numpy()) <= TOL
    _b3_expect(outs["clean"], outs["bad"], nan_t, cone, "GraphedStream")
    assert not torch.isnan(gs.states.ring).any()
