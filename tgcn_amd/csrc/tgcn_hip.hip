// tgcn_hip.hip -- gfx950 (MI355X) kernels + C ABI for the Chebyshev (time-)graph convolution.
// See include/tgcn_hip.h for the contract and DESIGN.md for layout / roofline notes.
//
// One translation unit; the kernels live in topic headers included once inside the anonymous namespace below:
//   common.h         error reporting, launch timing (tgcn_profile_*), tuning switches, LDS attribute bookkeeping, and how a launcher picks a
//                    kernel's template instantiation: with_flags / with_one_of (run-time values as constants), launch_kernel(_parts)
//   hop.h            hop_kernel<LPR,VEC,U,R> / hop_fixup_kernel: row-block + column-ordered-segment CSR x dense rows,
//                    fused Y = alpha (L X) + beta Z (+ gamma Z2) (+ P = L X); deterministic segment fold
//   project.h        out = sum_t A_t W_t + bias: exact fp32 MFMA (streaming / W-resident), bf16x3 (two forms), narrow VALU
//   wgrad.h          dW_t = A_t^T G, two deterministic stages on the fp32 MFMA
//   small_graph.h    graphs that fit in LDS: whole layer / basis in ONE launch (sparse, first-layer, dense matrix-pipe)
//   pool_relayout.h  (Q,n,C) -> (n,Q,C), gcn_pool / gcn_pool_4, relu + pool pass
//   windows.h        streaming time windows of multi-channel series: sliding-window fp32 MFMA GEMM (forward, input gradient), weight gradient
//   windows_bf16.h   the same on bf16 tensors: sliding-window bf16 MFMA GEMM, flipped bf16 weight, weight gradient (fp32 sums)
//   device_build.h   operand / schedule construction on the device: prefix sums, stable radix sort, CSR build, schedule kernels
//   graph_build.h    tgcn_graph_* / tgcn_sched_* / tgcn_csr_build_f32: host-side orchestration of device_build.h (one-off per operand)
// This file: the extern "C" entry points (argument checks, workspace carving, launches) declared in tgcn_hip.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <math.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <new>
#include <numeric>
#include <mutex>
#include <set>
#include <type_traits>
#include <utility>
#include <vector>

#include "tgcn_hip.h"

namespace {

#include "common.h"
#include "hop.h"
#include "project.h"
#include "wgrad.h"
#include "small_graph.h"
#include "pool_relayout.h"
#include "dropout.h"
#include "windows.h"
#include "windows_bf16.h"
#include "stream_small.h"
#include "series_small.h"
#include "device_build.h"
#include "graph_build.h"

}  // namespace

// ==================================================================================================
// C ABI
// ==================================================================================================
extern "C" {

const char* tgcn_last_error(void) { return g_err; }
int tgcn_abi_version(void) { return TGCN_ABI_VERSION; }

void tgcn_reset_tuning(void) {
  g_hop_variant.store(0); g_hop_remap.store(1); g_hop_seg_remap.store(0); g_hop_mix.store(0); g_hop_stream.store(1); g_hop_lds_pad.store(0);
  g_proj_variant.store(0); g_small_dense.store(2); g_small_narrow.store(1); g_x3_form.store(2); g_x3_tail.store(1);
  g_x3_stream_cap.store(0); g_overlap.store(1); g_overlap_group.store(3); g_overlap_min_mb.store(256);
  g_sched_hub_min.store(512); g_sched_hub_seg.store(64); g_sched_hub_gate_mb.store(256);
}

int tgcn_set_tuning(const char* key, int32_t value) {
  if (key && strcmp(key, "hop_variant") == 0) { g_hop_variant.store(value); return TGCN_OK; }
  if (key && strcmp(key, "hop_xcd_remap") == 0) { g_hop_remap.store(value != 0); return TGCN_OK; }
  if (key && strcmp(key, "hop_seg_remap") == 0) { g_hop_seg_remap.store(value != 0); return TGCN_OK; }
  if (key && strcmp(key, "hop_mix") == 0) { g_hop_mix.store(value); return TGCN_OK; }
  if (key && strcmp(key, "hop_stream") == 0) { g_hop_stream.store(value != 0); return TGCN_OK; }
  if (key && strcmp(key, "hop_lds_pad") == 0) { if (value < 0 || value > 160 * 1024) TGCN_FAIL(TGCN_ERR_INVALID, "set_tuning: hop_lds_pad %d", value); g_hop_lds_pad.store(value); return TGCN_OK; }
  if (key && strcmp(key, "project_variant") == 0) { g_proj_variant.store(value); return TGCN_OK; }
  if (key && strcmp(key, "small_dense") == 0) { g_small_dense.store(value); return TGCN_OK; }
  if (key && strcmp(key, "small_narrow") == 0) { g_small_narrow.store(value); return TGCN_OK; }
  if (key && strcmp(key, "x3_form") == 0) { g_x3_form.store(value); return TGCN_OK; }
  if (key && strcmp(key, "x3_tail") == 0) { g_x3_tail.store(value != 0); return TGCN_OK; }
  if (key && strcmp(key, "x3_stream_cap") == 0) { if (value < 0) TGCN_FAIL(TGCN_ERR_INVALID, "set_tuning: x3_stream_cap %d", value); g_x3_stream_cap.store(value); return TGCN_OK; }
  if (key && strcmp(key, "compact_overlap") == 0) { g_overlap.store(value != 0); return TGCN_OK; }
  if (key && strcmp(key, "compact_overlap_group") == 0) { if (value < 1) TGCN_FAIL(TGCN_ERR_INVALID, "set_tuning: compact_overlap_group %d", value); g_overlap_group.store(value); return TGCN_OK; }
  if (key && strcmp(key, "compact_overlap_min_mb") == 0) { if (value < 0) TGCN_FAIL(TGCN_ERR_INVALID, "set_tuning: compact_overlap_min_mb %d", value); g_overlap_min_mb.store(value); return TGCN_OK; }
  if (key && strcmp(key, "sched_hub_min") == 0) { if (value < 0) TGCN_FAIL(TGCN_ERR_INVALID, "set_tuning: sched_hub_min %d", value); g_sched_hub_min.store(value); return TGCN_OK; }
  if (key && strcmp(key, "sched_hub_seg") == 0) { if (value < 1) TGCN_FAIL(TGCN_ERR_INVALID, "set_tuning: sched_hub_seg %d", value); g_sched_hub_seg.store(value); return TGCN_OK; }
  if (key && strcmp(key, "sched_hub_gate_mb") == 0) { if (value < 0) TGCN_FAIL(TGCN_ERR_INVALID, "set_tuning: sched_hub_gate_mb %d", value); g_sched_hub_gate_mb.store(value); return TGCN_OK; }
  TGCN_FAIL(TGCN_ERR_INVALID, "set_tuning: unknown key");
}

int64_t tgcn_side_stream_launches(void) { return g_side_launches; }

int tgcn_profile_start(int32_t capacity) {
  if (capacity <= 0) TGCN_FAIL(TGCN_ERR_INVALID, "profile: capacity %d", capacity);
  for (auto& r : g_prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  g_prof.clear();
  g_prof.reserve(capacity);
  g_prof_cap = capacity;
  return TGCN_OK;
}

int tgcn_profile_stop(int32_t* kinds, float* ms, int32_t capacity, int32_t* count) {
  g_prof_cap = 0;
  int n = 0;
  for (auto& r : g_prof) {
    float t = 0.f;
    if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) t = -1.f;
    if (n < capacity && kinds && ms) { kinds[n] = r.kind; ms[n] = t; ++n; }
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  g_prof.clear();
  if (count) *count = n;
  return TGCN_OK;
}

int tgcn_hop_vec_width(int32_t C, int aligned16) { return C > 0 ? hop_geom(C, aligned16).vec : 0; }
int tgcn_hop_lanes_per_row(int32_t C, int aligned16) { return C > 0 ? hop_geom(C, aligned16).lpr : 0; }
int tgcn_hop_groups_per_block(int32_t C, int aligned16) { return C > 0 ? kBlock / hop_geom(C, aligned16).lpr : 0; }

size_t tgcn_csr_hop_workspace_bytes(const tgcn_csr_sched* sched, int32_t nb, int32_t C, int aligned16) {
  if (!sched || C <= 0 || nb <= 0) return 0;
  return (size_t)sched->npartial * (size_t)nb * (size_t)hop_geom(C, aligned16).cpad * sizeof(float);
}

int tgcn_csr_hop_f32(void* stream, const tgcn_csr* A, const tgcn_csr_sched* S, int32_t nb, int32_t C,
                     const tgcn_dense* X, const tgcn_dense* Z, float alpha, float beta, const tgcn_dense* Y,
                     const tgcn_dense* P, void* workspace, size_t workspace_bytes) {
  return tgcn_csr_hop2_f32(stream, A, S, nb, C, X, Z, alpha, beta, nullptr, 0.f, Y, P, workspace, workspace_bytes);
}

static int hop_impl(void* stream, const tgcn_csr* A, const tgcn_csr_sched* S, int32_t nb, int32_t C,
                    const tgcn_dense* X, const tgcn_dense* Z, float alpha, float beta, const tgcn_dense* Z2, float gamma,
                    const tgcn_dense* Y, const tgcn_dense* P, void* workspace, size_t workspace_bytes, int bf16 = 0);

int tgcn_csr_hop2_f32(void* stream, const tgcn_csr* A, const tgcn_csr_sched* S, int32_t nb, int32_t C,
                      const tgcn_dense* X, const tgcn_dense* Z, float alpha, float beta, const tgcn_dense* Z2, float gamma,
                      const tgcn_dense* Y, const tgcn_dense* P, void* workspace, size_t workspace_bytes) {
  return hop_impl(stream, A, S, nb, C, X, Z, alpha, beta, Z2, gamma, Y, P, workspace, workspace_bytes);
}

// bf16: rows of bf16 elements (tgcn_csr_hop_bf16; strides in elements, hop_geom_bf16), fp32 sums and partial rows.
static int hop_impl(void* stream, const tgcn_csr* A, const tgcn_csr_sched* S, int32_t nb, int32_t C,
                    const tgcn_dense* X, const tgcn_dense* Z, float alpha, float beta, const tgcn_dense* Z2, float gamma,
                    const tgcn_dense* Y, const tgcn_dense* P, void* workspace, size_t workspace_bytes, int bf16) {
  if (!A || !S || !X || !X->ptr) TGCN_FAIL(TGCN_ERR_INVALID, "hop: null operand");
  if (int drc = check_pointer_device(X->ptr, (hipStream_t)stream, "hop")) return drc;
  if ((!Y || !Y->ptr) && (!P || !P->ptr)) TGCN_FAIL(TGCN_ERR_INVALID, "hop: no output");
  if (A->n <= 0 || A->nnz < 0 || A->nnz >= (int64_t)INT32_MAX || A->n >= (int64_t)INT32_MAX)
    TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "hop: n=%lld nnz=%lld outside int32 index range", (long long)A->n, (long long)A->nnz);
  if (nb <= 0 || C <= 0) TGCN_FAIL(TGCN_ERR_INVALID, "hop: nb=%d C=%d", nb, C);
  if (!A->rowptr || (A->nnz > 0 && !A->edges) || !S->blk_row) TGCN_FAIL(TGCN_ERR_INVALID, "hop: null CSR/schedule array");
  const int al = bf16 ? (aligned8(X) && aligned8(Z) && aligned8(Z2) && aligned8(Y) && aligned8(P))
                      : (aligned4(X) && aligned4(Z) && aligned4(Z2) && aligned4(Y) && aligned4(P));
  const HopGeom g = bf16 ? hop_geom_bf16(C, al) : hop_geom(C, al);
  if (S->lanes_per_row != g.lpr)
    TGCN_FAIL(TGCN_ERR_INVALID, "hop: schedule built for %d lanes/row, C=%d (aligned16=%d) needs %d", S->lanes_per_row, C, al, g.lpr);
  if (S->nblk <= 0 || S->row_thresh <= 0) TGCN_FAIL(TGCN_ERR_INVALID, "hop: empty schedule");
  if (S->nseg < 0 || S->nlong < 0 || S->nhuge < 0 || S->nhuge > S->nlong || S->npartial < 0) TGCN_FAIL(TGCN_ERR_INVALID, "hop: bad schedule counts");
  if (S->seg_mode != 0 && !(S->seg_mode == 1 && g.lpr < 64)) TGCN_FAIL(TGCN_ERR_INVALID, "hop: seg_mode %d with %d lanes per row", S->seg_mode, g.lpr);
  if ((int64_t)nb * g.nchunks > 65535) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "hop: nb*chunks=%lld > 65535", (long long)nb * g.nchunks);
  if (S->nseg > 0 && (!S->seg_row || !S->seg_e0 || !S->seg_e1 || !S->seg_slot)) TGCN_FAIL(TGCN_ERR_INVALID, "hop: null segment arrays");
  if (S->npartial > 0) {
    const size_t need = (size_t)S->npartial * nb * g.cpad * sizeof(float);
    if (!workspace || workspace_bytes < need) TGCN_FAIL(TGCN_ERR_WORKSPACE, "hop: workspace %zu < %zu", workspace_bytes, need);
    if (!S->long_row || !S->long_slot || S->nlong <= 0) TGCN_FAIL(TGCN_ERR_INVALID, "hop: null long-row arrays");
  }
  HopParams p;
  memset(&p, 0, sizeof(p));
  p.rowptr = A->rowptr; p.ev = A->edges; p.blk_row = S->blk_row;
  p.seg_row = S->seg_row; p.seg_e0 = S->seg_e0; p.seg_e1 = S->seg_e1; p.seg_slot = S->seg_slot;
  p.long_row = S->long_row; p.long_slot = S->long_slot;
  p.X = X->ptr; p.x_bs = X->batch_stride; p.x_ld = X->row_stride;
  if (Z && Z->ptr) { p.Z = Z->ptr; p.z_bs = Z->batch_stride; p.z_ld = Z->row_stride; }
  if (Z2 && Z2->ptr) { p.Z2 = Z2->ptr; p.z2_bs = Z2->batch_stride; p.z2_ld = Z2->row_stride; p.gamma = gamma; }
  if (Y && Y->ptr) { p.Y = Y->ptr; p.y_bs = Y->batch_stride; p.y_ld = Y->row_stride; }
  if (P && P->ptr) { p.P = P->ptr; p.p_bs = P->batch_stride; p.p_ld = P->row_stride; }
  p.partial = (float*)workspace;
  p.alpha = alpha; p.beta = beta;
  p.nblk = S->nblk; p.nseg = S->nseg; p.nlong = S->nlong; p.nhuge = S->nhuge; p.row_thresh = S->row_thresh;
  p.C = C; p.nb = nb; p.nchunks = g.nchunks; p.cpad = g.cpad; p.remap = g_hop_remap.load();
  p.seg_mode = S->seg_mode; p.seg_remap = g_hop_seg_remap.load();
  if (S->nwseg < 0 || S->nwseg > S->nseg || (S->nwseg > 0 && (S->seg_mode != 0 || g.lpr >= 64))) TGCN_FAIL(TGCN_ERR_INVALID, "hop: nwseg %d of %d segments", S->nwseg, S->nseg);
  p.nwseg = S->nwseg;
  {
    // the REQUEST only (1: row blocks dealt among the segment blocks, -1: segment blocks first); launch_hop turns it into the
    // period once it knows the real number of segment blocks of the kernel it launches (rows interleaved per group differ by variant)
    const int mix = g_hop_mix.load();
    p.mix_period = (mix == 1 || (mix == 0 && S->row_mix)) ? 1 : (mix == 2 ? -1 : 0);
  }
  p.stream_out = !bf16 && ((int64_t)A->n * C * (int64_t)sizeof(float) * nb > ((int64_t)256 << 20)) && g_hop_stream.load();
  const int gpb = kBlock / g.lpr;
  const int seg_blocks = (S->nseg + gpb - 1) / gpb;
  const dim3 grid((unsigned)(S->nblk + seg_blocks), (unsigned)(nb * g.nchunks));
  const int fix_blocks = S->nhuge + (S->nlong - S->nhuge + gpb - 1) / gpb;
  const dim3 fix_grid((unsigned)(fix_blocks > 0 ? fix_blocks : 1), (unsigned)(nb * g.nchunks));
  hipStream_t st = (hipStream_t)stream;
  if (bf16) return g.vec == 8 ? launch_hop_vec<8, hbf16>(st, p, g.lpr, grid, fix_grid) : launch_hop_vec<1, hbf16>(st, p, g.lpr, grid, fix_grid);
  return g.vec == 4 ? launch_hop_vec<4>(st, p, g.lpr, grid, fix_grid) : launch_hop_vec<1>(st, p, g.lpr, grid, fix_grid);
}

size_t tgcn_csr_hop_bf16_workspace_bytes(const tgcn_csr_sched* sched, int32_t nb, int32_t C, int aligned16) {
  if (!sched || C <= 0 || nb <= 0) return 0;
  return (size_t)sched->npartial * (size_t)nb * (size_t)hop_geom_bf16(C, aligned16).cpad * sizeof(float);
}

int tgcn_csr_hop_bf16(void* stream, const tgcn_csr* A, const tgcn_csr_sched* S, int32_t nb, int32_t C,
                      const tgcn_dense* X, const tgcn_dense* Z, float alpha, float beta, const tgcn_dense* Y,
                      const tgcn_dense* P, void* workspace, size_t workspace_bytes) {
  return hop_impl(stream, A, S, nb, C, X, Z, alpha, beta, nullptr, 0.f, Y, P, workspace, workspace_bytes, 1);
}

int tgcn_csr_hop2_bf16(void* stream, const tgcn_csr* A, const tgcn_csr_sched* S, int32_t nb, int32_t C,
                       const tgcn_dense* X, const tgcn_dense* Z, float alpha, float beta, const tgcn_dense* Z2, float gamma,
                       const tgcn_dense* Y, const tgcn_dense* P, void* workspace, size_t workspace_bytes) {
  return hop_impl(stream, A, S, nb, C, X, Z, alpha, beta, Z2, gamma, Y, P, workspace, workspace_bytes, 1);
}

// What the compacted layer (and tgcn_cheb_project_stream_f32) ask of project_impl beyond a plain call:
struct StreamAsk {
  bool query;          // launch nothing: `streams` = whether this call would take the streaming bf16x3 kernel
  bool streams;
  bool force;          // the streaming kernel also below its row threshold (a part of a pass that takes it as a whole); TGCN_ERR_UNSUPPORTED where the shape has none
  int32_t* claim;      // non-null: the 256-thread claiming form on a capped number of workgroups, tiles from this device counter (zeroed here, stream-ordered)
};
static int project_impl(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const float* const* a,
                        const int64_t* lda, const float* W, const float* bias, int32_t bias_kind,
                        int64_t n_vertices, int64_t interleave, int32_t accumulate, float* out, int64_t ldo,
                        int32_t win_n, int32_t win_t, int32_t bias_cols = -1, const int32_t* rowmap = nullptr, uint32_t mapped = 0,
                        int32_t nbatch = 1, const int64_t* a_bs = nullptr, int64_t out_bs = 0, int32_t pool = 0, uint8_t* pool_idx = nullptr,
                        StreamAsk* ask = nullptr);

// THE dispatch of the projection: which kernel a shape takes.  project_impl launches what this returns and project_pool_fusable asks the
// same function, so the fused relu + pool epilogue can never be requested from a kernel that does not have it.
// project_variant: 0 auto (vector-ALU kernel for a few scalars per row, bf16x3 on large problems, else exact fp32: W-resident when the
// weight fits, streaming otherwise), 1 exact-fp32 streaming, 2 exact-fp32 (W-resident with 16-row wave tiles when it fits), 3 bf16x3 always,
// 4 exact fp32 auto, 5 vector-ALU kernel whenever it applies, 6 the streaming bf16x3 kernel whenever the shape has it (also below its row threshold).
enum ProjKernel { kProjNarrow, kProjResident, kProjX3, kProjX3Wide, kProjStream, kProjX3Stream };
constexpr int64_t kX3StreamMinRows = 32768;          // fewer rows: the tiled kernels (a persistent grid of 4096 waves wants >= a few tiles each)
constexpr size_t kX3StreamMaxLds = 150 * 1024;       // the three bf16 planes of the whole weight in fragment order
static inline int x3_stream_nt(int32_t N) { return N <= 16 ? 1 : (N <= 32 ? 2 : 4); }
static inline size_t x3_stream_lds(int32_t Kc, int32_t N, int32_t nterms) { return (size_t)nterms * (Kc / 32) * x3_stream_nt(N) * 3 * 1024; }
struct ProjChoice {
  ProjKernel kernel;
  int nt;            // 16-column tiles per workgroup of the W-resident kernel
  int nts;           // 16-column tiles per workgroup of the streaming / bf16x3 kernels
  size_t wbytes;     // LDS image of the weight for the W-resident kernel
  bool pool_epilogue;   // the kernel can end in relu + max over consecutive rows (through its vector epilogue)
  int pool_max;         // ... over groups whose size divides this: 16 (rows of a wave's tile in LDS scratch), 4 in the wide bf16x3 kernel (a lane's four accumulator rows)
};
// stream_ok: the call has nothing the streaming kernel lacks (pool epilogue, accumulate, interleave, windows) -- project_impl knows,
// the shape-only query (pool fusability) passes false: that form lives in project_x3_kernel.
static ProjChoice project_choose(int64_t M, int32_t Kc, int32_t N, int32_t nterms, bool vec4, bool vec_epilogue, bool has_rowmap, bool windows,
                                 bool stream_ok = false, int32_t nbatch = 1, bool force_stream = false) {
  ProjChoice c;
  const int pv = g_proj_variant.load();
  c.nt = N <= 16 ? 1 : (N <= 32 ? 2 : 4);
  c.wbytes = (size_t)nterms * ((Kc + 3) / 4 * 4) * c.nt * 16 * sizeof(float);
  // streaming-W / bf16x3 kernels: widest column tile that keeps padding low, so A is read once per block and no MFMA works
  // on padding (N = 160 -> one block of 10 tiles instead of three of 4)
  const int tiles = (N + 15) / 16;
  c.nts = tiles <= 1 ? 1 : tiles <= 2 ? 2 : tiles <= 4 ? 4 : tiles <= 6 ? 6 : tiles <= 8 ? 8 : 10;
  if (tiles > 10) {   // several column blocks: the width with the least padded tiles
    int best = 10, waste = (10 - tiles % 10) % 10;
    for (int w : {8, 6, 4}) { const int ws = (w - tiles % w) % w; if (ws < waste) { waste = ws; best = w; } }
    c.nts = best;
  }
  c.pool_epilogue = false;
  c.pool_max = 16;
  (void)has_rowmap;     // every kernel reads mapped terms / writes mapped rows through proj_arow / proj_orow
  if ((pv == 0 || pv == 5) && (int64_t)Kc * nterms <= kNarrowMaxK && !windows && vec_epilogue && N <= 1024 && (M >= 4096 || pv == 5)) {
    c.kernel = kProjNarrow;           // a few scalars per row: the output streams from the vector ALU
    return c;
  }
  const bool use_x3 = pv == 3 || (pv == 0 && M >= 8192 && (int64_t)Kc * nterms >= 64);
  // rows of 32 / 64 floats, <= 64 output columns, whole weight resident as bf16 planes: the barrier-free streaming form
  if (stream_ok && !windows && vec4 && vec_epilogue && (Kc == 32 || Kc == 64) && N <= 64 && x3_stream_lds(Kc, N, nterms) <= kX3StreamMaxLds &&
      x3_stream_lds(Kc, N, nterms) <= (size_t)lds_optin_limit() && M < (int64_t)INT32_MAX &&
      /* n_vertices is checked by the caller of this function where it matters: project_impl passes it through stream_ok */
      (pv == 6 || force_stream || (pv == 0 && use_x3 && M * (int64_t)nbatch >= kX3StreamMinRows))) {
    c.kernel = kProjX3Stream;
    return c;
  }
  if (c.wbytes <= (size_t)kResMaxWBytes && pv != 1 && !use_x3) {
    c.kernel = kProjResident;
    c.pool_epilogue = vec_epilogue;
    return c;
  }
  if (use_x3) {
    c.kernel = (vec4 && c.nts >= 6 && g_x3_form.load() == 2) ? kProjX3Wide : kProjX3;      // wide outputs: A fragments from registers
    c.pool_epilogue = (c.kernel == kProjX3 && c.nts <= 4 && vec_epilogue) || c.kernel == kProjX3Wide;
    if (c.kernel == kProjX3Wide) c.pool_max = 4;
    return c;
  }
  c.kernel = kProjStream;
  return c;
}

// Whether the projection of this shape (aligned operands, no row map) ends in a kernel with the fused relu + pool epilogue.
static bool project_pool_fusable(int64_t M, int32_t Kc, int32_t N, int32_t nterms, int32_t pool) {
  if (pool < 2 || 16 % pool != 0 || M % pool != 0 || N % 4 != 0 || nterms > kMaxTerms) return false;
  const ProjChoice c = project_choose(M, Kc, N, nterms, Kc % 4 == 0, true, false, false);
  return c.pool_epilogue && c.pool_max % pool == 0;
}

int tgcn_cheb_project_f32(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const float* const* a,
                          const int64_t* lda, const float* W, const float* bias, int32_t bias_kind,
                          int64_t n_vertices, int64_t interleave, int32_t accumulate, float* out, int64_t ldo) {
  return project_impl(stream, M, Kc, N, nterms, a, lda, W, bias, bias_kind, n_vertices, interleave, accumulate, out, ldo, 0, 0);
}

int tgcn_cheb_project_mapped_f32(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const float* const* a, const int64_t* lda,
                                 const float* W, const float* bias, int32_t bias_kind, int64_t n_vertices, int64_t interleave, const int32_t* rowmap,
                                 uint32_t mapped_terms, int32_t nbatch, const int64_t* a_bs, int64_t out_bs, float* out, int64_t ldo) {
  if (!rowmap || nbatch < 1 || (nbatch > 1 && !a_bs) || interleave < 1)
    TGCN_FAIL(TGCN_ERR_INVALID, "project_mapped: bad argument");
  int64_t zero_bs[kMaxTerms] = {0};
  return project_impl(stream, M, Kc, N, nterms, a, lda, W, bias, bias_kind, n_vertices, interleave, 0, out, ldo, 0, 0, -1, rowmap, mapped_terms, nbatch,
                      a_bs ? a_bs : zero_bs, out_bs);
}

int tgcn_cheb_project_stream_f32(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const float* const* a, const int64_t* lda,
                                 const float* W, const float* bias, int32_t bias_kind, int64_t n_vertices, const int32_t* rowmap, uint32_t mapped_terms,
                                 int32_t nbatch, const int64_t* a_bs, int64_t out_bs, float* out, int64_t ldo, int32_t* tile_counter) {
  if (nbatch < 1 || (nbatch > 1 && !a_bs)) TGCN_FAIL(TGCN_ERR_INVALID, "project_stream: bad argument");
  int64_t zero_bs[kMaxTerms] = {0};
  StreamAsk ask = {false, false, true, tile_counter};
  return project_impl(stream, M, Kc, N, nterms, a, lda, W, bias, bias_kind, n_vertices, 1, 0, out, ldo, 0, 0, -1, rowmap, mapped_terms, nbatch,
                      a_bs ? a_bs : zero_bs, out_bs, 0, nullptr, &ask);
}

int tgcn_cheb_project_windows_f32(void* stream, int64_t n_vertices, int32_t T, int32_t H, int32_t N, int32_t nterms,
                                  const float* const* series, const float* W, const float* bias, int32_t bias_kind,
                                  float* out) {
  if (T < H || H < 1) TGCN_FAIL(TGCN_ERR_INVALID, "project_windows: need 1 <= H <= T");
  const int32_t nwin = T - H + 1;
  int64_t lda[kMaxTerms];
  for (int t = 0; t < kMaxTerms; ++t) lda[t] = T;
  return project_impl(stream, n_vertices * nwin, H, N, nterms, series, lda, W, bias, bias_kind, n_vertices, nwin, 0, out, N, nwin, T);
}

static int project_impl(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const float* const* a,
                        const int64_t* lda, const float* W, const float* bias, int32_t bias_kind,
                        int64_t n_vertices, int64_t interleave, int32_t accumulate, float* out, int64_t ldo,
                        int32_t win_n, int32_t win_t, int32_t bias_cols, const int32_t* rowmap, uint32_t mapped,
                        int32_t nbatch, const int64_t* a_bs, int64_t out_bs, int32_t pool, uint8_t* pool_idx, StreamAsk* ask) {
  if (nbatch < 1 || (nbatch > 1 && !a_bs)) TGCN_FAIL(TGCN_ERR_INVALID, "project: nbatch %d", nbatch);
  if (M <= 0 || Kc <= 0 || N <= 0 || nterms <= 0 || !a || !lda || !W || !out) TGCN_FAIL(TGCN_ERR_INVALID, "project: bad argument");
  if (int drc = check_pointer_device(out, (hipStream_t)stream, "project")) return drc;
  if (nterms > kMaxTerms) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "project: nterms %d > %d (chunk with accumulate=1)", nterms, kMaxTerms);
  if (bias_kind < 0 || bias_kind > 2 || (bias_kind && !bias)) TGCN_FAIL(TGCN_ERR_INVALID, "project: bias_kind %d", bias_kind);
  if (interleave < 1 || n_vertices < 1) TGCN_FAIL(TGCN_ERR_INVALID, "project: interleave/n_vertices");
  if (interleave > 1 && !rowmap && M != interleave * n_vertices) TGCN_FAIL(TGCN_ERR_INVALID, "project: M != interleave*n_vertices");
  if (rowmap && win_n != 0) TGCN_FAIL(TGCN_ERR_INVALID, "project: a row map excludes windows");
  if (rowmap && interleave != 1 && (M % interleave != 0 || nbatch != 1))
    TGCN_FAIL(TGCN_ERR_INVALID, "project: row map with interleave %lld: M must be mapped vertices x interleave, one sample batch", (long long)interleave);
  ProjParams p;
  memset(&p, 0, sizeof(p));
  p.rowmap = rowmap; p.mapped = rowmap ? mapped : 0u;
  bool vec4 = (Kc % 4 == 0) && win_n == 0;   // windows start at any float: scalar loads
  p.win_n = win_n; p.win_t = win_t;
  p.bias_cols = bias_cols < 0 ? N : bias_cols;   // bias rows have bias_cols floats
  p.bias_ld = p.bias_cols;
  for (int t = 0; t < nterms; ++t) {
    if (!a[t]) TGCN_FAIL(TGCN_ERR_INVALID, "project: null term %d", t);
    p.a[t] = a[t];
    p.lda[t] = lda[t];
    vec4 = vec4 && (((uintptr_t)a[t] & 15) == 0) && (lda[t] % 4 == 0);
  }
  p.W = W; p.bias = bias; p.out = out; p.M = M; p.ldo = ldo; p.n_vertices = n_vertices; p.interleave = interleave;
  p.Kc = Kc; p.N = N; p.nterms = nterms; p.bias_kind = bias_kind; p.accumulate = accumulate;
  p.vec_epilogue = (N % 4 == 0) && (ldo % 4 == 0) && (((uintptr_t)out & 15) == 0) && (!bias || ((uintptr_t)bias & 15) == 0) &&
                   (p.bias_cols % 4 == 0);
  bool strides4 = (out_bs % 4 == 0);
  if (nbatch > 1) for (int t = 0; t < nterms; ++t) strides4 = strides4 && (a_bs[t] % 4 == 0);
  const bool stream_ok = pool <= 1 && !accumulate && interleave == 1 && win_n == 0 && strides4 && bias_cols < 0 && n_vertices < (int64_t)INT32_MAX;
  const ProjChoice choice = project_choose(M, Kc, N, nterms, vec4, p.vec_epilogue != 0, rowmap != nullptr, win_n != 0, stream_ok, nbatch, ask && ask->force);
  if (ask && ask->query) { ask->streams = choice.kernel == kProjX3Stream; return TGCN_OK; }
  if (ask && (ask->force || ask->claim) && choice.kernel != kProjX3Stream)
    TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "project: no streaming bf16x3 kernel for this shape (rows of 32 / 64 floats, <= 64 columns, 16-byte aligned operands; Kc=%d N=%d terms=%d)", Kc, N, nterms);
  if (rowmap && interleave != 1 && choice.kernel != kProjNarrow)
    TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "project: a row map together with interleave is the vector-ALU kernel's form (nterms*Kc <= %d, N %% 4 == 0, M >= 4096)", kNarrowMaxK);
  if (pool > 1) {     // fused relu + max-pool epilogue: only where the dispatch takes a kernel that has it
    if (rowmap || interleave != 1 || accumulate || win_n != 0 || nbatch != 1 || pool < 2 || choice.pool_max % pool != 0 || M % pool != 0 || !choice.pool_epilogue ||
        n_vertices % pool != 0)
      TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "project: no fused pool epilogue for this shape (M=%lld Kc=%d N=%d terms=%d pool=%d)", (long long)M, Kc, N, nterms, pool);
    p.pool = pool; p.pool_idx = pool_idx;
  }
  p.nbatch = 1;
  if (nbatch > 1) {
    // samples sharing the tile rows: inside project_x3_kernel<NT, true>, a host loop otherwise
    if ((choice.kernel == kProjX3 && vec4) || choice.kernel == kProjX3Stream) {
      p.nbatch = nbatch; p.out_bs = out_bs;
      for (int t = 0; t < nterms; ++t) {
        p.a_bs[t] = a_bs[t];
        if (a_bs[t] % 4 != 0) TGCN_FAIL(TGCN_ERR_INVALID, "project: sample stride of term %d not a multiple of 4 floats", t);
      }
      if (out_bs % 4 != 0) p.vec_epilogue = 0;
    } else {
      const float* ab[kMaxTerms];
      for (int b = 0; b < nbatch; ++b) {
        for (int t = 0; t < nterms; ++t) ab[t] = a[t] + (int64_t)b * a_bs[t];
        const int rc = project_impl(stream, M, Kc, N, nterms, ab, lda, W, bias, bias_kind, n_vertices, interleave, accumulate,
                                    out + (int64_t)b * out_bs, ldo, win_n, win_t, bias_cols, rowmap, mapped);
        if (rc != TGCN_OK) return rc;
      }
      return TGCN_OK;
    }
  }
  const int nt = choice.nt;
  hipStream_t st = (hipStream_t)stream;
  const int kc4 = (Kc + 3) / 4 * 4;
  const size_t wbytes = choice.wbytes;
  const unsigned gy = (unsigned)((N + nt * 16 - 1) / (nt * 16));
  if (choice.kernel == kProjNarrow) {
    // a few scalars per row: stream the output from the vector ALU (project_narrow_kernel)
    const int L = N / 4, RP = kBlock / L;
    const int ktot = Kc * nterms;
    int iters = (40 * 1024 / 4 - ktot * N) / (ktot * RP * 4);    // A values of a block: about 40 KB of LDS with the weights
    iters = iters < 1 ? 1 : (iters > 16 ? 16 : iters);
    const int rows_per_block = RP * 4 * iters;
    const int64_t nb = (M + rows_per_block - 1) / rows_per_block;
    if (nb > (int64_t)INT32_MAX) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "project: M too large");
    const size_t lds = ((size_t)ktot * N + (size_t)ktot * rows_per_block) * sizeof(float);
    allow_large_lds((const void*)project_narrow_kernel, 160 * 1024);
    ProfScope ps(TGCN_PROF_PROJECT, st);
    hipLaunchKernelGGL(project_narrow_kernel, dim3((unsigned)nb), dim3(kBlock), lds, st, p, iters);
    TGCN_CHECK_LAUNCH("tgcn_cheb_project_f32 (narrow)");
    return TGCN_OK;
  }
  if (choice.kernel == kProjX3Stream) {
    const int snt = x3_stream_nt(N);
    const size_t lds = x3_stream_lds(Kc, N, nterms);
    const int64_t ntiles = (M + 15) / 16;
    int32_t* claim = ask ? ask->claim : nullptr;
    int64_t gx = (ntiles + 15) / 16;
    if (gx > cu_count()) gx = cu_count();           // persistent: one 1024-thread workgroup per CU, waves take tiles round robin
    if (claim) {
      // the form that runs beside other kernels: 256-thread workgroups, at most `cap` of them, tiles claimed from *claim.  One per two CUs:
      // what the hops lose is the same per byte streamed beside them at 64 ... 256 workgroups, the forward is 1 ms shorter at 128 than at 256 (A.7)
      const int64_t cap = g_x3_stream_cap.load() > 0 ? g_x3_stream_cap.load() : (cu_count() + 1) / 2;
      gx = (ntiles + 3) / 4;
      if (gx > cap) gx = cap;
      if (hipMemsetAsync(claim, 0, sizeof(int32_t), st) != hipSuccess) TGCN_FAIL(TGCN_ERR_LAUNCH, "project: memset of the tile counter failed");
    }
    ProfScope ps(TGCN_PROF_PROJECT, st);
    const DynLds dl(lds, (int)kX3StreamMaxLds);
    with_one_of<1, 2, 4>(snt, [&](auto NT) { with_one_of<1, 2>(Kc == 32 ? 1 : 2, [&](auto KT) {
      if (claim) launch_kernel(project_x3_claim_kernel<NT, KT>, dim3((unsigned)gx), dim3(256), dl, st, p, ntiles, claim);
      else launch_kernel(project_x3_stream_kernel<NT, KT>, dim3((unsigned)gx), dim3(1024), dl, st, p, ntiles);
    }); });
    TGCN_CHECK_LAUNCH("tgcn_cheb_project_f32 (bf16x3 streaming)");
    return TGCN_OK;
  }
  const bool use_x3 = choice.kernel == kProjX3 || choice.kernel == kProjX3Wide;
  if (choice.kernel == kProjResident) {
    const int rt = g_proj_variant.load() == 2 ? 1 : 2;                  // 8 waves x 32 rows (variant 2: 16 waves x 16 rows)
    const int res_rows = 16 * rt, res_waves = 1024 / rt / 64;
    const size_t lds = wbytes + (size_t)kResScratchFloats * sizeof(float);
    const int64_t ntiles = (M + res_rows - 1) / res_rows;
    int64_t gx = (ntiles + res_waves - 1) / res_waves;
    if (gx > cu_count()) gx = cu_count();    // one persistent workgroup per CU (LDS-limited residency)
    const dim3 grid((unsigned)gx, gy);
    ProfScope ps(TGCN_PROF_PROJECT, st);
    const DynLds dl(lds, kResMaxWBytes + kResScratchFloats * (int)sizeof(float));
    with_one_of<1, 2, 4>(nt, [&](auto NT) { with_flags([&](auto V4) {
      const auto rt1 = project_resident_kernel<NT, V4, 1>, rt2 = project_resident_kernel<NT, V4, 2>;
      allow_large_lds((const void*)(rt == 1 ? rt2 : rt1), dl.optin);      // both forms are opted in, whichever runs
      launch_kernel(rt == 1 ? rt1 : rt2, grid, dim3(1024 / rt), dl, st, p, kc4, ntiles);
    }, vec4); });
    TGCN_CHECK_LAUNCH("tgcn_cheb_project_f32 (resident)");
    return TGCN_OK;
  }
  const int64_t mb = (M + 127) / 128;
  if (mb > (int64_t)INT32_MAX) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "project: M too large");
  const int tiles = (N + 15) / 16, nts = choice.nts;
  const dim3 grid((unsigned)mb, (unsigned)((tiles + nts - 1) / nts));
  ProfScope ps(TGCN_PROF_PROJECT, st);
  if (use_x3) {      // bf16x3 products on the bf16 matrix pipe
    const int64_t gx3 = (M + 255) / 256 * p.nbatch;                   // sample-fastest: the nbatch workgroups of a tile are neighbours
    if (gx3 > (int64_t)INT32_MAX) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "project: grid too large");
    const dim3 grid3((unsigned)gx3, grid.y);
    // project_x3v2_kernel runs one workgroup per CU: when the last round of 256-row tiles would fill at most ~60 % of the CUs,
    // its rows go out as 128-row tiles (twice the workgroups, about half the duration each)
    const int64_t B = (M + 255) / 256, rem = B % cu_count();
    int64_t main_blocks = B, tail_blocks = 0;
    if (rem != 0 && rem * 8 <= (int64_t)cu_count() * 5 && g_x3_tail.load()) {
      main_blocks = B - rem;
      tail_blocks = (M - main_blocks * 256 + 127) / 128;
    }
    const dim3 grid3v2((unsigned)(main_blocks + tail_blocks), grid.y);
    // a plain `if` on NT: project_x3v2_kernel is built for all six tile counts, the wide outputs (compute-bound) launch it for 6, 8 and 10
    with_one_of<1, 2, 4, 6, 8, 10>(nts, [&](auto NT) { with_flags([&](auto V4) {
      if (NT >= 6 && choice.kernel == kProjX3Wide) launch_kernel(project_x3v2_kernel<NT>, grid3v2, dim3(512), 0, st, p, (int)main_blocks);
      else launch_kernel(project_x3_kernel<NT, V4>, grid3, dim3(512), 0, st, p);
    }, vec4); });
    TGCN_CHECK_LAUNCH("tgcn_cheb_project_f32 (bf16x3)");
    return TGCN_OK;
  }
  with_one_of<1, 2, 4, 6, 8, 10>(nts, [&](auto NT) { with_flags([&](auto V4) {
    launch_kernel(project_kernel<NT, V4>, grid, dim3(kBlock), 0, st, p);
  }, vec4); });
  TGCN_CHECK_LAUNCH("tgcn_cheb_project_f32");
  return TGCN_OK;
}

static int64_t wgrad_rows_per_block(int64_t M) {
  int64_t rpb = (M + 1023) / 1024;            // at most 1024 row blocks (partials to fold) ...
  if (rpb < 64) rpb = 64;                     // ... of at least 64 rows
  return (rpb + 15) / 16 * 16;
}
static int wgrad_blocks(int64_t M) {
  const int64_t rpb = wgrad_rows_per_block(M);
  return (int)((M + rpb - 1) / rpb);
}

size_t tgcn_cheb_wgrad_workspace_bytes(int64_t M, int32_t Kc, int32_t N, int32_t nterms) {
  if (M <= 0 || Kc <= 0 || N <= 0 || nterms <= 0) return 0;
  return (size_t)wgrad_blocks(M) * nterms * Kc * N * sizeof(float);
}

int tgcn_cheb_wgrad_f32(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const float* const* a,
                        const int64_t* lda, const float* G, int64_t ldg, float* dW, void* workspace, size_t workspace_bytes) {
  if (M <= 0 || Kc <= 0 || N <= 0 || nterms <= 0 || !a || !lda || !G || !dW) TGCN_FAIL(TGCN_ERR_INVALID, "wgrad: bad argument");
  if (nterms > kMaxTerms) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "wgrad: nterms %d > %d", nterms, kMaxTerms);
  const size_t need = tgcn_cheb_wgrad_workspace_bytes(M, Kc, N, nterms);
  if (!workspace || workspace_bytes < need) TGCN_FAIL(TGCN_ERR_WORKSPACE, "wgrad: workspace %zu < %zu", workspace_bytes, need);
  WgradParams p;
  memset(&p, 0, sizeof(p));
  for (int t = 0; t < nterms; ++t) {
    if (!a[t]) TGCN_FAIL(TGCN_ERR_INVALID, "wgrad: null term %d", t);
    p.a[t] = a[t];
    p.lda[t] = lda[t];
  }
  p.G = G; p.partial = (float*)workspace; p.dW = dW; p.M = M; p.ldg = ldg;
  p.Kc = Kc; p.N = N; p.nterms = nterms; p.nblocks = wgrad_blocks(M);
  p.rows_per_block = wgrad_rows_per_block(M);
  const int ctiles = (Kc + 15) / 16;
  const int tgroups = (nterms + kWgTerms - 1) / kWgTerms;
  if ((N + 63) / 64 > 65535 || (int64_t)ctiles * tgroups > 65535) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "wgrad: Kc=%d N=%d too wide", Kc, N);
  hipStream_t st = (hipStream_t)stream;
  { ProfScope ps(TGCN_PROF_WGRAD, st);
    hipLaunchKernelGGL(wgrad_partial_kernel, dim3(p.nblocks, (N + 63) / 64, ctiles * tgroups), dim3(64), 0, st, p); }
  { ProfScope ps(TGCN_PROF_WGRAD, st);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)(((int64_t)nterms * Kc * N + 63) / 64)), dim3(1024), 0, st, p); }
  TGCN_CHECK_LAUNCH("tgcn_cheb_wgrad_f32");
  return TGCN_OK;
}

int tgcn_cheb_project_bf16(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const void* const* a, const int64_t* lda,
                           const void* W, const void* bias, int32_t bias_kind, int32_t bias_dtype, int32_t bias_cols, int64_t n_vertices,
                           int64_t interleave, int32_t accumulate, void* out, int64_t ldo, int32_t out_dtype) {
  if (M <= 0 || Kc <= 0 || N <= 0 || nterms <= 0 || !a || !lda || !W || !out || ldo < N) TGCN_FAIL(TGCN_ERR_INVALID, "project_bf16: bad argument");
  if (int drc = check_pointer_device(out, (hipStream_t)stream, "project_bf16")) return drc;
  if (nterms > kMaxTerms) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "project_bf16: nterms %d > %d (chunk with accumulate=1)", nterms, kMaxTerms);
  if ((int64_t)nterms * Kc >= (int64_t)INT32_MAX / 2) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "project_bf16: nterms * Kc too large");
  if (bias_kind < 0 || bias_kind > 2 || (bias_kind && !bias)) TGCN_FAIL(TGCN_ERR_INVALID, "project_bf16: bias_kind %d", bias_kind);
  if ((bias_dtype != TGCN_DTYPE_F32 && bias_dtype != TGCN_DTYPE_BF16) || (out_dtype != TGCN_DTYPE_F32 && out_dtype != TGCN_DTYPE_BF16))
    TGCN_FAIL(TGCN_ERR_INVALID, "project_bf16: dtype codes %d / %d", bias_dtype, out_dtype);
  if (interleave < 1 || n_vertices < 1) TGCN_FAIL(TGCN_ERR_INVALID, "project_bf16: interleave/n_vertices");
  if (interleave > 1 && M != interleave * n_vertices) TGCN_FAIL(TGCN_ERR_INVALID, "project_bf16: M != interleave*n_vertices");
  ProjBf16Params p;
  memset(&p, 0, sizeof(p));
  bool vec8 = Kc % 8 == 0;
  for (int t = 0; t < nterms; ++t) {
    if (!a[t]) TGCN_FAIL(TGCN_ERR_INVALID, "project_bf16: null term %d", t);
    p.a[t] = (const hbf16*)a[t];
    p.lda[t] = lda[t];
    vec8 = vec8 && (((uintptr_t)a[t] & 15) == 0) && (lda[t] % 8 == 0);
  }
  p.W = (const hbf16*)W; p.bias = bias; p.out = out;
  p.M = M; p.ldo = ldo; p.n_vertices = n_vertices; p.interleave = interleave;
  p.Kc = Kc; p.N = N; p.nterms = nterms; p.bias_kind = bias_kind; p.bias_bf16 = bias_dtype == TGCN_DTYPE_BF16;
  p.bias_cols = (bias_cols <= 0 || bias_cols > N) ? N : bias_cols;
  p.accumulate = accumulate; p.out_bf16 = out_dtype == TGCN_DTYPE_BF16;
  const int tiles = (N + 15) / 16;
  const int nt = tiles <= 1 ? 1 : (tiles <= 2 ? 2 : 4);
  const int64_t gx = (M + 127) / 128;
  if (gx > (int64_t)INT32_MAX) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "project_bf16: M too large");
  const dim3 grid((unsigned)gx, (unsigned)((tiles + nt - 1) / nt));
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(TGCN_PROF_PROJECT, st);
  with_one_of<1, 2, 4>(nt, [&](auto NT) { with_flags([&](auto V8) {
    launch_kernel(project_bf16_kernel<NT, V8>, grid, dim3(256), 0, st, p);
  }, vec8); });
  TGCN_CHECK_LAUNCH("tgcn_cheb_project_bf16");
  return TGCN_OK;
}

int tgcn_cheb_project_mapped_bf16(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const void* const* a, const int64_t* lda,
                                  const void* W, const void* bias, int32_t bias_kind, int32_t bias_dtype, int64_t n_vertices, const int32_t* rowmap,
                                  uint32_t mapped_terms, int32_t nbatch, const int64_t* a_bs, int64_t out_bs, void* out, int64_t ldo,
                                  int32_t out_dtype) {
  if (!rowmap || nbatch < 1 || (nbatch > 1 && !a_bs)) TGCN_FAIL(TGCN_ERR_INVALID, "project_mapped_bf16: bad argument");
  if (M <= 0 || Kc <= 0 || N <= 0 || nterms <= 0 || !a || !lda || !W || !out || ldo < N) TGCN_FAIL(TGCN_ERR_INVALID, "project_mapped_bf16: bad argument");
  if (int drc = check_pointer_device(out, (hipStream_t)stream, "project_mapped_bf16")) return drc;
  if (nterms > kMaxTerms) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "project_mapped_bf16: nterms %d > %d", nterms, kMaxTerms);
  if ((int64_t)nterms * Kc >= (int64_t)INT32_MAX / 2) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "project_mapped_bf16: nterms * Kc too large");
  if (bias_kind < 0 || bias_kind > 2 || (bias_kind && !bias)) TGCN_FAIL(TGCN_ERR_INVALID, "project_mapped_bf16: bias_kind %d", bias_kind);
  if ((bias_dtype != TGCN_DTYPE_F32 && bias_dtype != TGCN_DTYPE_BF16) || (out_dtype != TGCN_DTYPE_F32 && out_dtype != TGCN_DTYPE_BF16))
    TGCN_FAIL(TGCN_ERR_INVALID, "project_mapped_bf16: dtype codes %d / %d", bias_dtype, out_dtype);
  if (n_vertices < 1) TGCN_FAIL(TGCN_ERR_INVALID, "project_mapped_bf16: n_vertices");
  ProjBf16MappedParams p;
  memset(&p, 0, sizeof(p));
  bool vec8 = Kc % 8 == 0;
  for (int t = 0; t < nterms; ++t) {
    if (!a[t]) TGCN_FAIL(TGCN_ERR_INVALID, "project_mapped_bf16: null term %d", t);
    p.lda[t] = lda[t];
    p.a_bs[t] = nbatch > 1 ? a_bs[t] : 0;
    vec8 = vec8 && (((uintptr_t)a[t] & 15) == 0) && (lda[t] % 8 == 0) && (p.a_bs[t] % 8 == 0);
  }
  p.W = (const hbf16*)W; p.bias = bias;
  p.M = M; p.ldo = ldo; p.n_vertices = n_vertices; p.interleave = 1;
  p.Kc = Kc; p.N = N; p.nterms = nterms; p.bias_kind = bias_kind; p.bias_bf16 = bias_dtype == TGCN_DTYPE_BF16;
  p.bias_cols = N; p.out_bf16 = out_dtype == TGCN_DTYPE_BF16;
  p.rowmap = rowmap; p.mapped = mapped_terms; p.out_bs = out_bs;
  const int tiles = (N + 15) / 16;
  const int nt = tiles <= 1 ? 1 : (tiles <= 2 ? 2 : 4);
  const int64_t gx = (M + 127) / 128;
  if (gx > (int64_t)INT32_MAX) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "project_mapped_bf16: M too large");
  hipStream_t st = (hipStream_t)stream;
  const size_t out_elem = p.out_bf16 ? 2 : 4;
  for (int32_t b0 = 0; b0 < nbatch; b0 += 65535) {       // the samples ride on grid.z
    const int32_t nb = std::min<int32_t>(65535, nbatch - b0);
    for (int t = 0; t < nterms; ++t) p.a[t] = (const hbf16*)a[t] + (int64_t)b0 * p.a_bs[t];
    p.out = (char*)out + (size_t)((int64_t)b0 * out_bs) * out_elem;
    const dim3 grid((unsigned)gx, (unsigned)((tiles + nt - 1) / nt), (unsigned)nb);
    ProfScope ps(TGCN_PROF_PROJECT, st);
    with_one_of<1, 2, 4>(nt, [&](auto NT) { with_flags([&](auto V8) {
      launch_kernel(project_bf16_kernel<NT, V8, true>, grid, dim3(256), 0, st, p);
    }, vec8); });
  }
  TGCN_CHECK_LAUNCH("tgcn_cheb_project_mapped_bf16");
  return TGCN_OK;
}

int tgcn_cheb_wgrad_bf16(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const void* const* a, const int64_t* lda,
                         const void* G, int64_t ldg, float* dW, void* workspace, size_t workspace_bytes) {
  if (M <= 0 || Kc <= 0 || N <= 0 || nterms <= 0 || !a || !lda || !G || !dW) TGCN_FAIL(TGCN_ERR_INVALID, "wgrad_bf16: bad argument");
  if (nterms > kMaxTerms) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "wgrad_bf16: nterms %d > %d", nterms, kMaxTerms);
  const size_t need = tgcn_cheb_wgrad_workspace_bytes(M, Kc, N, nterms);
  if (!workspace || workspace_bytes < need) TGCN_FAIL(TGCN_ERR_WORKSPACE, "wgrad_bf16: workspace %zu < %zu", workspace_bytes, need);
  WgradBf16Params p;
  memset(&p, 0, sizeof(p));
  for (int t = 0; t < nterms; ++t) {
    if (!a[t]) TGCN_FAIL(TGCN_ERR_INVALID, "wgrad_bf16: null term %d", t);
    p.a[t] = (const hbf16*)a[t];
    p.lda[t] = lda[t];
  }
  p.G = (const hbf16*)G; p.partial = (float*)workspace; p.M = M; p.ldg = ldg;
  p.Kc = Kc; p.N = N; p.nterms = nterms;
  p.rows_per_block = wgrad_rows_per_block(M);
  WgradParams r;                   // the fold of the partials: wgrad_reduce_kernel reads partial, dW and the sizes only
  memset(&r, 0, sizeof(r));
  r.partial = p.partial; r.dW = dW; r.Kc = Kc; r.N = N; r.nterms = nterms; r.nblocks = wgrad_blocks(M);
  const int ctiles = (Kc + 15) / 16;
  const int tgroups = (nterms + kWgTerms - 1) / kWgTerms;
  if ((N + 63) / 64 > 65535 || (int64_t)ctiles * tgroups > 65535) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "wgrad_bf16: Kc=%d N=%d too wide", Kc, N);
  hipStream_t st = (hipStream_t)stream;
  { ProfScope ps(TGCN_PROF_WGRAD, st);
    hipLaunchKernelGGL(wgrad_bf16_partial_kernel, dim3(r.nblocks, (N + 63) / 64, ctiles * tgroups), dim3(64), 0, st, p); }
  { ProfScope ps(TGCN_PROF_WGRAD, st);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)(((int64_t)nterms * Kc * N + 63) / 64)), dim3(1024), 0, st, r); }
  TGCN_CHECK_LAUNCH("tgcn_cheb_wgrad_bf16");
  return TGCN_OK;
}

int tgcn_relayout_qnc_to_nqc_f32(void* stream, const float* in, float* out, int64_t Q, int64_t n, int32_t C) {
  if (!in || !out || Q <= 0 || n <= 0 || C <= 0) TGCN_FAIL(TGCN_ERR_INVALID, "relayout: bad argument");
  if (C > 32) {       // wide rows: a coalesced row copy
    const bool v4 = (C % 4 == 0) && (((uintptr_t)in & 15) == 0) && (((uintptr_t)out & 15) == 0);
    const int64_t units = Q * n * (v4 ? C / 4 : C);
    ProfScope ps(TGCN_PROF_RELAYOUT, (hipStream_t)stream);
    if (v4) hipLaunchKernelGGL((relayout_rows_kernel<4>), dim3(grid_1d(units)), dim3(kBlock), 0, (hipStream_t)stream, in, out, Q, n, C);
    else hipLaunchKernelGGL((relayout_rows_kernel<1>), dim3(grid_1d(units)), dim3(kBlock), 0, (hipStream_t)stream, in, out, Q, n, C);
    TGCN_CHECK_LAUNCH("tgcn_relayout_qnc_to_nqc_f32 (wide rows)");
    return TGCN_OK;
  }
  const int64_t gy = (Q + kRelT - 1) / kRelT;
  if (gy > 65535) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "relayout: Q too large");
  const int vt = relayout_vertex_tile(C);
  const dim3 grid((unsigned)((n + vt - 1) / vt), (unsigned)gy);
  ProfScope ps(TGCN_PROF_RELAYOUT, (hipStream_t)stream);
  hipLaunchKernelGGL(relayout_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, in, out, Q, n, (int)C, vt);
  TGCN_CHECK_LAUNCH("tgcn_relayout_qnc_to_nqc_f32");
  return TGCN_OK;
}

// Workspace layout of the layer forward (all offsets 256-byte aligned):
//   [xt]        n*q*C floats           (layout 1 only: re-laid input)
//   [hop 1..K-1] (K-1) * qc*n*C floats
//   [partial]   long-row segment scratch for one hop
static void fwd_ws_layout(const tgcn_csr_sched* S, int32_t K, int64_t q, int64_t n, int32_t C, int32_t layout,
                          int64_t qc, size_t* off_xt, size_t* off_hops, size_t* hop_bytes, size_t* off_part, size_t* total) {
  size_t o = 0;
  *off_xt = o;
  if (layout == 1) o += align_up((size_t)q * n * C * sizeof(float), 256);
  *off_hops = o;
  // consecutive hop tensors are staggered by an odd multiple of 256 B on top of their size: the projection streams
  // all K of them at once and equally aligned streams collide on the same DRAM channels (measured: -6 %)
  *hop_bytes = align_up((size_t)qc * n * C * sizeof(float), 256) + 65 * 256;
  o += (size_t)(K > 1 ? K - 1 : 0) * *hop_bytes;
  *off_part = o;
  const int32_t nb = layout == 1 ? 1 : (int32_t)qc;
  const int32_t Crow = layout == 1 ? (int32_t)(q * C) : C;
  o += align_up(tgcn_csr_hop_workspace_bytes(S, nb, Crow, 1), 256);
  *total = o;
}

int tgcn_cheb_forward_small_pool_supported(int64_t n, int64_t nnz, int32_t C, int32_t mode) {
  int dense = 0;
  return small_config(n, nnz, C, mode, &dense);
}

int tgcn_cheb_forward_small_supported(int64_t n, int64_t nnz, int32_t C, int32_t mode) {
  int dense = 0;
  const int ntc = small_config(n, nnz, C, mode, &dense);
  if (ntc) return ntc;
  return (g_small_dense.load() && dense_mfma_config(n, nnz, C, mode, 1, 1, false)) ? 16 : 0;
}

int tgcn_cheb_forward_small_f32(void* stream, const tgcn_csr* A, int32_t mode, int32_t K, int64_t q, int32_t C, int32_t N,
                                const float* x, const float* W, const float* fold, const float* bias, int32_t bias_kind,
                                float* out) {
  return tgcn_cheb_forward_small_pool_f32(stream, A, mode, K, q, C, N, x, W, fold, bias, bias_kind, 0, 0, out, nullptr);
}

int tgcn_cheb_forward_small_pool_f32(void* stream, const tgcn_csr* A, int32_t mode, int32_t K, int64_t q, int32_t C, int32_t N,
                                     const float* x, const float* W, const float* fold, const float* bias, int32_t bias_kind,
                                     int32_t relu, int32_t pool, float* out, uint8_t* pool_idx) {
  if (!A || !x || !W || !out || K < 1 || q < 1 || N < 1) TGCN_FAIL(TGCN_ERR_INVALID, "forward_small: bad argument");
  if (int drc = check_pointer_device(x, (hipStream_t)stream, "forward_small")) return drc;
  if (pool < 0 || pool > 255 || (pool > 0 && A->n % pool != 0) || (pool == 0 && relu)) TGCN_FAIL(TGCN_ERR_INVALID, "forward_small: pool=%d relu=%d n=%lld", pool, relu, (long long)A->n);
  if (bias_kind < 0 || bias_kind > 2 || (bias_kind && !bias)) TGCN_FAIL(TGCN_ERR_INVALID, "forward_small: bias_kind %d", bias_kind);
  if (fold && mode != 0) TGCN_FAIL(TGCN_ERR_INVALID, "forward_small: fold is for mode 0");
  if (q > 2147483647LL) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "forward_small: grid too large");
  SmallParams p;
  p.rowptr = A->rowptr; p.ev = A->edges; p.x = x; p.W = W; p.fold = fold; p.bias = bias; p.out = out;
  p.n = (int32_t)A->n; p.nnz = (int32_t)A->nnz; p.q = (int32_t)q; p.K = K; p.C = C; p.N = N; p.mode = mode; p.bias_kind = bias_kind; p.dense = 0; p.relu = relu; p.pool = pool; p.pool_idx = pool_idx;
  p.npad = 0; p.spw = 1;
  p.Ld = A->dense;
  tgcn_small_plan pl;     // kernel form, tile, samples per workgroup, grid, block and LDS: small_plan (small_graph.h), also behind tgcn_cheb_small_plan
  const char* why = "";
  if (const int prc = small_plan(A->n, A->nnz, A->dense != nullptr, mode, C, N, q, pool, false, &pl, &why)) {
    if (why[0] == 'g') TGCN_FAIL(prc, "forward_small: grid too large");
    TGCN_FAIL(prc, "forward_small: n=%lld nnz=%lld C=%d does not fit in LDS", (long long)A->n, (long long)A->nnz, C);
  }
  hipStream_t st = (hipStream_t)stream;
  p.spw = pl.spw;
  if (pl.form >= 3) {   // dense operand (e.g. the 148-parcel DTI graph) on the matrix pipe: fp32, or bf16 with the three-way split
    ProfScope ps(TGCN_PROF_SMALL, st);
    if (pl.form == 4) launch_small_dense_x3<false>(st, p, pl);
    else launch_small_dense<false>(st, p, pl);
    TGCN_CHECK_LAUNCH("tgcn_cheb_forward_small_f32 (dense)");
    return TGCN_OK;
  }
  p.dense = pl.dense_lds;
  p.npad = (p.n + 63) / 64 * 64;
  const DynLds lds((size_t)pl.lds_bytes, 160 * 1024);
  const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y);
  const unsigned nthreads = (unsigned)pl.threads;
  ProfScope ps(TGCN_PROF_SMALL, st);
  if (pl.form == 1) {   // first layers: recursion on the 4-float input side, all of NT output channels per workgroup (small_narrow_kernel)
    with_one_of<64, 32, 16>(pl.tile, [&](auto NT) { launch_kernel(small_narrow_kernel<NT>, grid, dim3(nthreads), lds, st, p); });
    TGCN_CHECK_LAUNCH("tgcn_cheb_forward_small_f32 (narrow input)");
    return TGCN_OK;
  }
  with_one_of<16, 8>(pl.tile, [&](auto NTC) { with_one_of<4, 16, 32>(pl.cp, [&](auto CP) {
    launch_kernel(small_forward_kernel<NTC, CP>, grid, dim3(nthreads), lds, st, p);
  }); });
  TGCN_CHECK_LAUNCH("tgcn_cheb_forward_small_f32");
  return TGCN_OK;
}

int tgcn_cheb_small_plan(int64_t n, int64_t nnz, int32_t has_dense_copy, int32_t mode, int32_t C, int32_t N, int64_t q, int32_t pool,
                         int32_t basis, tgcn_small_plan* plan) {
  if (!plan || q < 1) TGCN_FAIL(TGCN_ERR_INVALID, "small_plan: bad argument");
  if (basis ? C < 1 : N < 1) TGCN_FAIL(TGCN_ERR_INVALID, "small_plan: bad argument");
  if (!basis && (pool < 0 || pool > 255 || (pool > 0 && n % pool != 0))) TGCN_FAIL(TGCN_ERR_INVALID, "small_plan: pool=%d n=%lld", pool, (long long)n);
  const char* why = "";
  tgcn_small_plan pl;
  if (const int rc = small_plan(n, nnz, has_dense_copy != 0, mode, C, N, q, pool, basis != 0, &pl, &why))
    TGCN_FAIL(rc, "small_plan: n=%lld nnz=%lld C=%d N=%d q=%lld: %s", (long long)n, (long long)nnz, C, N, (long long)q, why);
  *plan = pl;
  return TGCN_OK;
}

int tgcn_cheb_basis_small_supported(int64_t n, int64_t nnz, int32_t C, int32_t mode) {
  int dense = 0;
  const int ct = basis_config(n, nnz, C, mode, &dense);
  if (ct) return ct;
  return (g_small_dense.load() && dense_mfma_config(n, nnz, C, mode, 1, 1, true)) ? 16 : 0;
}

int tgcn_cheb_basis_small_f32(void* stream, const tgcn_csr* A, int32_t mode, int32_t K, int64_t q, int32_t C,
                              const float* x, float* stack) {
  if (!A || !x || !stack || K < 1 || q < 1 || C < 1) TGCN_FAIL(TGCN_ERR_INVALID, "basis_small: bad argument");
  if (!tgcn_cheb_basis_small_supported(A->n, A->nnz, C, mode))
    TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "basis_small: n=%lld nnz=%lld does not fit in LDS", (long long)A->n, (long long)A->nnz);
  if (K == 1) return TGCN_OK;
  SmallParams p;
  memset(&p, 0, sizeof(p));
  p.rowptr = A->rowptr; p.ev = A->edges; p.x = x; p.out = stack;
  p.n = (int32_t)A->n; p.nnz = (int32_t)A->nnz; p.q = (int32_t)q; p.K = K; p.C = C; p.mode = mode;
  p.Ld = A->dense;
  tgcn_small_plan pl;     // small_plan (small_graph.h), also behind tgcn_cheb_small_plan
  const char* why = "";
  if (const int prc = small_plan(A->n, A->nnz, A->dense != nullptr, mode, C, 0, q, 0, true, &pl, &why)) {
    if (why[0] == 'g') TGCN_FAIL(prc, "basis_small: grid too large");
    TGCN_FAIL(prc, "basis_small: n=%lld nnz=%lld does not fit in LDS", (long long)A->n, (long long)A->nnz);
  }
  hipStream_t st = (hipStream_t)stream;
  p.spw = pl.spw;
  ProfScope ps(TGCN_PROF_SMALL_BASIS, st);
  if (pl.form >= 3) {
    if (pl.form == 4) launch_small_dense_x3<true>(st, p, pl);
    else launch_small_dense<true>(st, p, pl);
    TGCN_CHECK_LAUNCH("tgcn_cheb_basis_small_f32 (dense)");
    return TGCN_OK;
  }
  p.dense = pl.dense_lds;
  p.npad = (p.n + 63) / 64 * 64;
  const DynLds lds((size_t)pl.lds_bytes, 160 * 1024);
  const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y);
  const unsigned nthreads = (unsigned)pl.threads;
  with_one_of<16, 8, 4>(pl.tile, [&](auto CT) { launch_kernel(small_basis_kernel<CT>, grid, dim3(nthreads), lds, st, p); });
  TGCN_CHECK_LAUNCH("tgcn_cheb_basis_small_f32");
  return TGCN_OK;
}

size_t tgcn_cheb_forward_workspace_bytes(const tgcn_csr_sched* S, int32_t K, int64_t q, int64_t n, int32_t C,
                                         int32_t layout, int64_t q_chunk) {
  if (!S || K < 1 || q < 1 || n < 1 || C < 1) return 0;
  const int64_t qc = (layout == 1 || q_chunk <= 0 || q_chunk > q) ? q : q_chunk;
  size_t a, b, c, d, total;
  fwd_ws_layout(S, K, q, n, C, layout, qc, &a, &b, &c, &d, &total);
  return total;
}

static int forward_impl(void* stream, const tgcn_csr* A, const tgcn_csr_sched* S, int32_t mode, int32_t K,
                        int64_t q, int64_t n, int32_t C, int32_t N, const float* x, const float* W,
                        const float* bias, int32_t bias_kind, float* out, int32_t layout, int64_t q_chunk,
                        void* workspace, size_t workspace_bytes, int32_t pool, uint8_t* pool_idx);

int tgcn_cheb_forward_f32(void* stream, const tgcn_csr* A, const tgcn_csr_sched* S, int32_t mode, int32_t K,
                          int64_t q, int64_t n, int32_t C, int32_t N, const float* x, const float* W,
                          const float* bias, int32_t bias_kind, float* out, int32_t layout, int64_t q_chunk,
                          void* workspace, size_t workspace_bytes) {
  return forward_impl(stream, A, S, mode, K, q, n, C, N, x, W, bias, bias_kind, out, layout, q_chunk, workspace, workspace_bytes, 0, nullptr);
}

// shapes whose layer forward can end in the fused relu + pool epilogue: (sample, vertex) row order, one projection call per pass
static bool forward_pool_fusable(int32_t K, int64_t q, int64_t n, int32_t C, int32_t N, int32_t layout, int64_t q_chunk, int32_t pool) {
  if (layout != 0 || K > kMaxTerms || n % pool != 0) return false;
  const int64_t qc = (q_chunk <= 0 || q_chunk > q) ? q : q_chunk;
  // every pass must take the same kind of kernel: check the full and the last (shorter) pass
  const int64_t last = q % qc ? q % qc : qc;
  return project_pool_fusable(qc * n, C, N, K, pool) && project_pool_fusable(last * n, C, N, K, pool);
}

size_t tgcn_cheb_forward_pool_workspace_bytes(const tgcn_csr_sched* S, int32_t K, int64_t q, int64_t n, int32_t C, int32_t N,
                                              int32_t layout, int64_t q_chunk, int32_t pool) {
  if (!S || K < 1 || q < 1 || n < 1 || C < 1 || N < 1 || pool < 1) return 0;
  // the base figure is 0 for K = 1 on a schedule without partial rows (no hop tensors, no scratch for partial sums): such a layer
  // still needs the scratch for its output when the shape cannot take the fused epilogue
  const size_t base = tgcn_cheb_forward_workspace_bytes(S, K, q, n, C, layout, q_chunk);
  return align_up(base, 256) + (forward_pool_fusable(K, q, n, C, N, layout, q_chunk, pool) ? 0 : align_up((size_t)q * n * N * sizeof(float), 256));
}

int tgcn_cheb_forward_pool_f32(void* stream, const tgcn_csr* A, const tgcn_csr_sched* S, int32_t mode, int32_t K, int64_t q,
                               int64_t n, int32_t C, int32_t N, const float* x, const float* W, const float* bias, int32_t bias_kind,
                               int32_t pool, float* out, uint8_t* pool_idx, int32_t layout, int64_t q_chunk, void* workspace,
                               size_t workspace_bytes) {
  if (pool < 1 || pool > 255 || n % pool != 0 || !out) TGCN_FAIL(TGCN_ERR_INVALID, "forward_pool: pool=%d n=%lld", pool, (long long)n);
  const size_t base = align_up(tgcn_cheb_forward_workspace_bytes(S, K, q, n, C, layout, q_chunk), 256);
  const bool aligned = (((uintptr_t)out & 15) == 0) && (!bias || ((uintptr_t)bias & 15) == 0) && (!pool_idx || ((uintptr_t)pool_idx & 3) == 0);
  const bool fusable = pool > 1 && forward_pool_fusable(K, q, n, C, N, layout, q_chunk, pool);
  if (fusable && aligned)       // the (q, n, N) layer output is never written
    return forward_impl(stream, A, S, mode, K, q, n, C, N, x, W, bias, bias_kind, out, layout, q_chunk, workspace, workspace_bytes, pool, pool_idx);
  // other shapes: the layer into scratch, then the relu + pool pass
  const size_t need = base + align_up((size_t)q * n * N * sizeof(float), 256);
  if (fusable && (!workspace || workspace_bytes < need))
    // the query sized the workspace for the fused epilogue (it cannot see the pointers): say what is wrong instead of "workspace"
    TGCN_FAIL(TGCN_ERR_INVALID, "forward_pool: the fused relu + pool epilogue of this shape needs out and bias 16-byte aligned and pool_idx 4-byte aligned "
                                "(out %p, bias %p, pool_idx %p); align them or pass %zu bytes of workspace for the two-pass form", (void*)out, (const void*)bias, (void*)pool_idx, need);
  if (!workspace || workspace_bytes < need) TGCN_FAIL(TGCN_ERR_WORKSPACE, "forward_pool: workspace %zu < %zu", workspace_bytes, need);
  float* y = (float*)((char*)workspace + base);
  int rc = forward_impl(stream, A, S, mode, K, q, n, C, N, x, W, bias, bias_kind, y, layout, q_chunk, workspace, base, 0, nullptr);
  if (rc != TGCN_OK) return rc;
  return tgcn_relu_pool_f32(stream, y, out, pool_idx, q, n, N, pool);
}

static int forward_impl(void* stream, const tgcn_csr* A, const tgcn_csr_sched* S, int32_t mode, int32_t K,
                        int64_t q, int64_t n, int32_t C, int32_t N, const float* x, const float* W,
                        const float* bias, int32_t bias_kind, float* out, int32_t layout, int64_t q_chunk,
                        void* workspace, size_t workspace_bytes, int32_t pool, uint8_t* pool_idx) {
  if (!A || !S || !x || !W || !out) TGCN_FAIL(TGCN_ERR_INVALID, "forward: null operand");
  if (int drc = check_pointer_device(x, (hipStream_t)stream, "forward")) return drc;
  if (K < 1 || q < 1 || n < 1 || C < 1 || N < 1 || n != A->n) TGCN_FAIL(TGCN_ERR_INVALID, "forward: bad shape (n=%lld, L is %lld)", (long long)n, (long long)A->n);
  if (mode != 0 && mode != 1) TGCN_FAIL(TGCN_ERR_INVALID, "forward: mode %d", mode);
  if (layout != 0 && layout != 1) TGCN_FAIL(TGCN_ERR_INVALID, "forward: layout %d", layout);
  if (layout == 1 && (C > 32 || q * C > (int64_t)INT32_MAX)) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "forward: layout 1 needs C <= 32");
  // rows of a multiple of 4 floats are read with 16-byte loads; other widths take the scalar forms and may start anywhere
  if ((C % 4 == 0 && ((uintptr_t)x & 15)) || ((uintptr_t)workspace & 15)) TGCN_FAIL(TGCN_ERR_INVALID, "forward: x/workspace must be 16-byte aligned");
  const int64_t qc = (layout == 1 || q_chunk <= 0 || q_chunk > q) ? q : q_chunk;
  size_t off_xt, off_hops, hop_bytes, off_part, total;
  fwd_ws_layout(S, K, q, n, C, layout, qc, &off_xt, &off_hops, &hop_bytes, &off_part, &total);
  if (total > 0 && (!workspace || workspace_bytes < total)) TGCN_FAIL(TGCN_ERR_WORKSPACE, "forward: workspace %zu < %zu", workspace_bytes, total);
  char* ws = (char*)workspace;
  float* part = (float*)(ws + off_part);
  const size_t part_bytes = total - off_part;
  const float* terms[kMaxTerms];
  int64_t ldas[kMaxTerms];
  int rc;

  for (int64_t q0 = 0; q0 < q; q0 += qc) {
    const int64_t qn = (q - q0 < qc) ? (q - q0) : qc;
    // operand view of this pass
    int32_t nb, Crow;
    const float* x0;
    if (layout == 1) {
      float* xt = (float*)(ws + off_xt);
      if ((rc = tgcn_relayout_qnc_to_nqc_f32(stream, x, xt, q, n, C)) != TGCN_OK) return rc;
      x0 = xt; nb = 1; Crow = (int32_t)(q * C);
    } else {
      x0 = x + q0 * n * C; nb = (int32_t)qn; Crow = C;
    }
    const int64_t bs = (int64_t)n * Crow;
    auto hop_ptr = [&](int k) -> float* {
      return k == 0 ? const_cast<float*>(x0) : (float*)(ws + off_hops + (size_t)(k - 1) * hop_bytes);
    };
    for (int k = 1; k < K; ++k) {
      tgcn_dense X = {hop_ptr(k - 1), bs, Crow};
      tgcn_dense Y = {hop_ptr(k), bs, Crow};
      if (mode == 0 || k == 1) {
        rc = tgcn_csr_hop_f32(stream, A, S, nb, Crow, &X, nullptr, 1.f, 0.f, &Y, nullptr, part, part_bytes);
      } else {
        tgcn_dense Zd = {hop_ptr(k - 2), bs, Crow};
        rc = tgcn_csr_hop_f32(stream, A, S, nb, Crow, &X, &Zd, 2.f, -1.f, &Y, nullptr, part, part_bytes);
      }
      if (rc != TGCN_OK) return rc;
    }
    // projection, in chunks of <= 32 terms
    const int64_t M = (layout == 1) ? n * q : qn * n;
    const int pl = pool > 1 ? pool : 1;              // pooled epilogue (layout 0, K <= 32 terms): output rows shrink by the pool
    float* o0 = (layout == 1) ? out : out + q0 * (n / pl) * N;
    for (int k0 = 0; k0 < K; k0 += kMaxTerms) {
      const int nt = (K - k0 < kMaxTerms) ? K - k0 : kMaxTerms;
      for (int t = 0; t < nt; ++t) { terms[t] = hop_ptr(k0 + t); ldas[t] = C; }
      const bool last = (k0 + nt >= K);
      rc = project_impl(stream, M, C, N, nt, terms, ldas, W + (size_t)k0 * C * N, last ? bias : nullptr,
                        last ? bias_kind : 0, n, layout == 1 ? q : 1, k0 > 0 ? 1 : 0, o0, N, 0, 0, -1, nullptr, 0, 1, nullptr, 0,
                        pool > 1 ? pool : 0, pool_idx ? pool_idx + q0 * (n / pl) * N : nullptr);
      if (rc != TGCN_OK) return rc;
    }
  }
  return TGCN_OK;
}

// Workspace of the compacted layer: the hop tensors -- K-1 (mode 0: terms 1..K-1) or K (mode 1: T_0 = x packed to the kept rows, then
// T_1..T_{K-1}) buffers of qc x (n_c + 1) x C floats (row n_c of every sample is the zero row that entries pointing at a left-out
// vertex gather from) -- unless the caller keeps the terms in its own memory, then the long-row scratch of one hop.
static int compact_nterm_bufs(int32_t mode, int32_t K) { return mode == 1 ? K : (K > 1 ? K - 1 : 0); }

static void cfwd_ws_layout(const tgcn_csr_sched* S, int32_t mode, int32_t K, int64_t n_c, int32_t C, int64_t qc, int keep, size_t* hop_bytes,
                           size_t* off_part, size_t* total) {
  *hop_bytes = align_up((size_t)qc * (size_t)(n_c + 1) * C * sizeof(float), 256) + 65 * 256;   // staggered like fwd_ws_layout
  *off_part = keep ? 0 : (size_t)compact_nterm_bufs(mode, K) * *hop_bytes;
  *total = *off_part + align_up(tgcn_csr_hop_workspace_bytes(S, 1, C, 1), 256);      // hops run one time step per launch
  *total += 256;            // last: the tile counter of the side stream's projections (one at a time: the side stream is one queue)
}

size_t tgcn_cheb_compact_layer_workspace_bytes(const tgcn_csr_sched* S, int32_t mode, int32_t K, int64_t q, int64_t n_c, int32_t C, int64_t q_chunk,
                                               int32_t keep_terms) {
  if (!S || K < 2 || q < 1 || n_c < 1 || C < 1 || (mode != 0 && mode != 1)) return 0;
  const int64_t qc = (keep_terms || q_chunk <= 0 || q_chunk > q) ? q : q_chunk;
  size_t a, b, total;
  cfwd_ws_layout(S, mode, K, n_c, C, qc, keep_terms != 0, &a, &b, &total);
  return total;
}

size_t tgcn_cheb_forward_compact_workspace_bytes(const tgcn_csr_sched* S, int32_t K, int64_t q, int64_t n_c, int32_t C, int64_t q_chunk) {
  return tgcn_cheb_compact_layer_workspace_bytes(S, 0, K, q, n_c, C, q_chunk, 0);
}

int tgcn_cheb_forward_compact_f32(void* stream, const tgcn_csr* A_first, const tgcn_csr* A_rest, const tgcn_csr_sched* S, int32_t K,
                                  int64_t q, int64_t n, int32_t C, int32_t N, const float* x, const float* W, const float* bias,
                                  int32_t bias_kind, float* out, const int32_t* rows, const int32_t* empty_rows, int64_t n_empty,
                                  int64_t q_chunk, void* workspace, size_t workspace_bytes) {
  return tgcn_cheb_compact_layer_f32(stream, A_first, A_rest, S, 0, K, q, n, C, N, x, W, nullptr, bias, bias_kind, out, rows, empty_rows, n_empty,
                                     q_chunk, nullptr, workspace, workspace_bytes);
}

int tgcn_cheb_compact_layer_f32(void* stream, const tgcn_csr* A_first, const tgcn_csr* A_rest, const tgcn_csr_sched* S, int32_t mode, int32_t K,
                                int64_t q, int64_t n, int32_t C, int32_t N, const float* x, const float* W, const float* W_left, const float* bias,
                                int32_t bias_kind, float* out, const int32_t* rows, const int32_t* empty_rows, int64_t n_empty,
                                int64_t q_chunk, float* keep_terms, void* workspace, size_t workspace_bytes) {
  if (!A_first || !A_rest || !S || !x || !W || !out || !rows) TGCN_FAIL(TGCN_ERR_INVALID, "compact_layer: null operand");
  if (int drc = check_pointer_device(x, (hipStream_t)stream, "compact_layer")) return drc;
  const int64_t n_c = A_first->n;
  if (mode != 0 && mode != 1) TGCN_FAIL(TGCN_ERR_INVALID, "compact_layer: mode %d", mode);
  if (K < 2 || K > kMaxTerms || q < 1 || n < 1 || C < 1 || N < 1) TGCN_FAIL(TGCN_ERR_INVALID, "compact_layer: bad shape (K=%d)", K);
  if (A_rest->n != n_c || A_rest->nnz != A_first->nnz || n_c < 1 || n_empty < 0 || n_c + n_empty != n || (n_empty > 0 && !empty_rows))
    TGCN_FAIL(TGCN_ERR_INVALID, "compact_layer: %lld compact + %lld left-out rows for n=%lld", (long long)n_c, (long long)n_empty, (long long)n);
  if (mode == 1 && n_empty > 0 && !W_left) TGCN_FAIL(TGCN_ERR_INVALID, "compact_layer: mode 1 needs W_left (W_0 - W_2 + W_4 - ...) for the left-out vertices");
  if ((C % 4 == 0 && ((uintptr_t)x & 15)) || ((uintptr_t)workspace & 15) || ((uintptr_t)keep_terms & 15))
    TGCN_FAIL(TGCN_ERR_INVALID, "compact_layer: x / workspace / keep_terms must be 16-byte aligned");
  const int64_t qc = (keep_terms || q_chunk <= 0 || q_chunk > q) ? q : q_chunk;      // kept terms: every sample's hop tensors survive the call
  if (qc > 65535) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "compact_layer: %lld samples per pass", (long long)qc);
  size_t hop_bytes, off_part, total;
  cfwd_ws_layout(S, mode, K, n_c, C, qc, keep_terms != nullptr, &hop_bytes, &off_part, &total);
  if (!workspace || workspace_bytes < total) TGCN_FAIL(TGCN_ERR_WORKSPACE, "compact_layer: workspace %zu < %zu", workspace_bytes, total);
  char* ws = (char*)workspace;
  float* part = (float*)(ws + off_part);
  const size_t part_bytes = total - 256 - off_part;
  int32_t* claim = (int32_t*)(ws + total - 256);
  const int64_t bs_c = (n_c + 1) * (int64_t)C;            // sample stride of a compact hop tensor
  const int k_first = mode == 1 ? 0 : 1;                  // first term that lives in a compact buffer
  // term k of the pass: in the caller's buffer the terms are contiguous ([term][q][n_c + 1][C]), in the workspace staggered
  auto hop_ptr = [&](int k) -> float* {
    const int i = k - k_first;
    return keep_terms ? keep_terms + (int64_t)i * q * bs_c : (float*)(ws + (size_t)i * hop_bytes);
  };
  hipStream_t st = (hipStream_t)stream;
  // the zero row of every hop tensor (gathered from by the next hop); no hop writes it, so once per call
  for (int k = k_first; k < K; ++k)
    if (hipMemset2DAsync(hop_ptr(k) + n_c * (int64_t)C, (size_t)bs_c * sizeof(float), 0, (size_t)C * sizeof(float), (size_t)qc, st) != hipSuccess)
      TGCN_FAIL(TGCN_ERR_LAUNCH, "compact_layer: memset failed");
  const float* terms[kMaxTerms];
  int64_t ldas[kMaxTerms];
  for (int k = 0; k < K; ++k) ldas[k] = C;
  int rc;
  int64_t a_bs[kMaxTerms];
  a_bs[0] = mode == 1 ? bs_c : n * (int64_t)C;
  for (int k = 1; k < K; ++k) a_bs[k] = bs_c;
  const bool vec_rows = (C % 4 == 0) && (((uintptr_t)x & 15) == 0);
  // Projections beside the hops: a hop launch leaves the matrix pipes, the LDS and most of the HBM bandwidth unused, and the
  // projections are streams that need little else.  Where a pass's projections take the streaming kernel, the left-out rows' projection
  // of the whole pass and the kept rows' projection of every group of `grp` time steps but the last go to the side stream in the
  // co-schedulable form (256-thread workgroups that claim their tiles), the former from the start of the pass, the latter behind its
  // group's last hop; the last group's projection follows on the caller's stream with the chip to itself.  The side stream is joined at the
  // end of every pass (the next pass's hops overwrite the hop tensors).  Only where one time step's hop tensor exceeds the Infinity Cache
  // (smaller operands are launch-bound) and never under stream capture (a captured graph gets no parallel branch).  Same kernels' arithmetic
  // row by row: the result does not depend on the path.
  const int64_t grp = g_overlap_group.load();
  bool overlap = g_overlap.load() != 0 && n_c * (int64_t)C * (int64_t)sizeof(float) > ((int64_t)g_overlap_min_mb.load() << 20) && qc > grp;
  if (overlap) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); overlap = false; }
    else if (cs != hipStreamCaptureStatusNone) overlap = false;
  }
  SideStream* side = overlap ? side_stream() : nullptr;
  if (overlap && !side) TGCN_FAIL(TGCN_ERR_LAUNCH, "compact_layer: no side stream");
  // joins the side stream into the caller's on every way out of a pass, errors included
  struct SideJoin {
    SideStream* s; hipStream_t st; bool forked = false;
    int fork() {
      hipEvent_t e = s->event();
      if (hipEventRecord(e, st) != hipSuccess || hipStreamWaitEvent(s->st, e, 0) != hipSuccess) return -1;
      forked = true;
      return 0;
    }
    int join() {
      if (!forked) return 0;
      forked = false;
      hipEvent_t e = s->event();
      return (hipEventRecord(e, s->st) != hipSuccess || hipStreamWaitEvent(st, e, 0) != hipSuccess) ? -1 : 0;
    }
    ~SideJoin() { (void)join(); }
  } sj{side, st};
  for (int64_t q0 = 0; q0 < q; q0 += qc) {
    const int64_t qn = (q - q0 < qc) ? (q - q0) : qc;
    const float* x0 = x + q0 * n * C;
    float* const o = out + q0 * n * N;
    const float* const W_empty = (mode == 1 || W_left) ? W_left : W;
    const float* xt[1] = {x0};
    const int64_t xbs[1] = {n * (int64_t)C};
    terms[0] = mode == 1 ? hop_ptr(0) : x0;
    for (int k = 1; k < K; ++k) terms[k] = hop_ptr(k);
    // what of this pass goes to the side stream: asked of the projection's own dispatch, for the pass as a whole
    bool side_kept = false, side_empty = false;
    if (overlap && qn > grp) {            // at least two groups: something to run beside
      StreamAsk ask = {true, false, false, nullptr};
      rc = project_impl(stream, n_c, C, N, K, terms, ldas, W, bias, bias_kind, n, 1, 0, o, N, 0, 0, -1, rows, mode == 1 ? 0u : 1u, (int32_t)qn, a_bs,
                        n * (int64_t)N, 0, nullptr, &ask);
      if (rc != TGCN_OK) return rc;
      side_kept = ask.streams;
      if (n_empty > 0) {
        rc = project_impl(stream, n_empty, C, N, 1, xt, ldas, W_empty, bias, bias_kind, n, 1, 0, o, N, 0, 0, -1, empty_rows, 1u, (int32_t)qn, xbs,
                          n * (int64_t)N, 0, nullptr, &ask);
        if (rc != TGCN_OK) return rc;
        side_empty = ask.streams;
      }
    }
    if (side_kept || side_empty) {
      if (sj.fork() != 0) TGCN_FAIL(TGCN_ERR_LAUNCH, "compact_layer: fork to the side stream failed");
    }
    if (side_empty) {
      StreamAsk ask = {false, false, true, claim};
      rc = project_impl(side->st, n_empty, C, N, 1, xt, ldas, W_empty, bias, bias_kind, n, 1, 0, o, N, 0, 0, -1, empty_rows, 1u, (int32_t)qn, xbs,
                        n * (int64_t)N, 0, nullptr, &ask);
      if (rc != TGCN_OK) return rc;
      ++g_side_launches;
    }
    // the kept rows' projection of time steps [b0, b1) of the pass, every term and the output moved to the group's first time step
    auto project_group = [&](int64_t b0, int64_t b1, bool on_side) -> int {
      const float* gt[kMaxTerms];
      for (int k = 0; k < K; ++k) gt[k] = terms[k] + b0 * a_bs[k];
      StreamAsk ask = {false, false, true, on_side ? claim : nullptr};
      return project_impl(on_side ? (void*)side->st : stream, n_c, C, N, K, gt, ldas, W, bias, bias_kind, n, 1, 0, o + b0 * n * N, N, 0, 0, -1, rows,
                          mode == 1 ? 0u : 1u, (int32_t)(b1 - b0), a_bs, n * (int64_t)N, 0, nullptr, &ask);
    };
    // hops: one launch per hop and time step (a launch's gather working set stays one (n_c, C) slab).
    // mode 0 (monomials of the folded weight): P_1 = A_first x (columns in the caller's labels), P_k = A_rest P_{k-1}.
    // mode 1 (Chebyshev): T_0 = the kept rows of x, T_1 = A_rest T_0, T_k = 2 A_rest T_{k-1} - T_{k-2}.
    for (int64_t b = 0; b < qn; ++b) {
      if (mode == 1) {
        const int64_t units = vec_rows ? n_c * (C / 4) : n_c * (int64_t)C;
        if (vec_rows) hipLaunchKernelGGL((gather_rows_i32_kernel<4>), dim3(grid_1d(units)), dim3(kBlock), 0, st, x0 + b * n * C, rows, hop_ptr(0) + b * bs_c, n_c, C, (int64_t)C);
        else hipLaunchKernelGGL((gather_rows_i32_kernel<1>), dim3(grid_1d(units)), dim3(kBlock), 0, st, x0 + b * n * C, rows, hop_ptr(0) + b * bs_c, n_c, C, (int64_t)C);
        TGCN_CHECK_LAUNCH("compact_layer (pack the kept rows of x)");
      }
      for (int k = 1; k < K; ++k) {
        tgcn_dense X = {(mode == 0 && k == 1) ? const_cast<float*>(x0) + b * n * C : hop_ptr(k - 1) + b * bs_c, 0, C};
        tgcn_dense Y = {hop_ptr(k) + b * bs_c, 0, C};
        if (mode == 1 && k >= 2) {
          tgcn_dense Zd = {hop_ptr(k - 2) + b * bs_c, 0, C};
          rc = hop_impl(stream, A_rest, S, 1, C, &X, &Zd, 2.f, -1.f, nullptr, 0.f, &Y, nullptr, part, part_bytes);
        } else {
          rc = hop_impl(stream, (mode == 0 && k == 1) ? A_first : A_rest, S, 1, C, &X, nullptr, 1.f, 0.f, nullptr, 0.f, &Y, nullptr, part, part_bytes);
        }
        if (rc != TGCN_OK) return rc;
      }
      // a group of time steps is through its hops: its projection goes behind them on the side stream, beside the next group's hops
      if (side_kept && (b + 1) % grp == 0 && b + 1 < qn) {
        hipEvent_t e = side->event();
        if (hipEventRecord(e, st) != hipSuccess || hipStreamWaitEvent(side->st, e, 0) != hipSuccess)
          TGCN_FAIL(TGCN_ERR_LAUNCH, "compact_layer: event for the side stream failed");
        if ((rc = project_group(b + 1 - grp, b + 1, true)) != TGCN_OK) return rc;
        ++g_side_launches;
      }
    }
    // projection of the pass's qn time steps in one launch per row class: the per-vertex bias is read once per pass (once per group where
    // the groups' projections run beside the hops)
    // kept vertices: all K terms (mode 0: x through the row map, hop tensors in compact rows; mode 1: every term in compact rows)
    if (side_kept) rc = project_group((qn - 1) / grp * grp, qn, false);
    else rc = project_impl(stream, n_c, C, N, K, terms, ldas, W, bias, bias_kind, n, 1, 0, o, N, 0, 0, -1, rows, mode == 1 ? 0u : 1u, (int32_t)qn, a_bs,
                           n * (int64_t)N);
    if (rc != TGCN_OK) return rc;
    // the others.  mode 0: P_k = 0 for k >= 1, so out = x W'_0 + bias.  mode 1: the left-out vertices are ISOLATED (no entries, never pointed at):
    // T_k = x, 0, -x, 0, ... so out = x (W_0 - W_2 + W_4 - ...) + bias = x W_left + bias.
    if (n_empty > 0 && !side_empty) {
      rc = project_impl(stream, n_empty, C, N, 1, xt, ldas, W_empty, bias, bias_kind, n, 1, 0, o, N, 0, 0, -1, empty_rows, 1u, (int32_t)qn,
                        xbs, n * (int64_t)N);
      if (rc != TGCN_OK) return rc;
    }
    if (sj.join() != 0) TGCN_FAIL(TGCN_ERR_LAUNCH, "compact_layer: join of the side stream failed");
  }
  return TGCN_OK;
}

int tgcn_relu_pool_f32(void* stream, const float* x, float* out, uint8_t* idx, int64_t q, int64_t n, int32_t f, int32_t p) {
  if (!x || !out || q <= 0 || n <= 0 || f <= 0 || p <= 0 || p > 255 || n % p != 0) TGCN_FAIL(TGCN_ERR_INVALID, "relu_pool: bad argument");
  const int64_t total = q * (n / p) * f;
  hipLaunchKernelGGL(relu_pool_kernel, dim3(grid_1d(total)), dim3(kBlock), 0, (hipStream_t)stream, x, out, idx, total, (int)f, (int)p);
  TGCN_CHECK_LAUNCH("tgcn_relu_pool_f32");
  return TGCN_OK;
}

int tgcn_relu_dropout_pool_f32(void* stream, const float* y, float* out, uint8_t* idx, int64_t q, int64_t n, int32_t f, int32_t pool, int32_t N,
                               const int64_t* seed, uint32_t thr, float scale) {
  if (!y || !out || q <= 0 || n <= 0 || f <= 0 || pool <= 0 || pool > 255 || n % pool != 0 || N <= 0 || f % N != 0 || !seed ||
      !dropout_scale_ok(scale))
    TGCN_FAIL(TGCN_ERR_INVALID, "relu_dropout_pool: bad argument");
  const int64_t total = q * (n / pool) * f;
  const DropoutParams d{seed, thr, scale};
  hipLaunchKernelGGL(relu_dropout_pool_kernel, dim3(grid_1d(total)), dim3(kBlock), 0, (hipStream_t)stream, y, out, idx, total, n, (int)f, (int)pool,
                     (int)N, d);
  TGCN_CHECK_LAUNCH("tgcn_relu_dropout_pool_f32");
  return TGCN_OK;
}

int tgcn_dropout_keep_u8(void* stream, const int64_t* seed, int64_t e0, int64_t count, uint32_t thr, uint8_t* out) {
  if (!seed || !out || e0 < 0 || count <= 0 || e0 > INT64_MAX - count) TGCN_FAIL(TGCN_ERR_INVALID, "dropout_keep: bad argument");
  hipLaunchKernelGGL(dropout_keep_kernel, dim3(grid_1d(count)), dim3(kBlock), 0, (hipStream_t)stream, seed, (uint64_t)e0, count, thr, out);
  TGCN_CHECK_LAUNCH("tgcn_dropout_keep_u8");
  return TGCN_OK;
}

int tgcn_relu_pool_bwd_f32(void* stream, const float* grad_z, const float* z, const uint8_t* idx, float* grad_y, int64_t q,
                           int64_t n, int32_t f, int32_t p) {
  if (!grad_z || !z || !idx || !grad_y || q <= 0 || n <= 0 || f <= 0 || p <= 0 || n % p != 0) TGCN_FAIL(TGCN_ERR_INVALID, "relu_pool_bwd: bad argument");
  const int64_t total = q * (n / p) * f;
  hipLaunchKernelGGL(relu_pool_bwd_kernel, dim3(grid_1d(total)), dim3(kBlock), 0, (hipStream_t)stream, grad_z, z, idx, grad_y, total, (int)f, (int)p);
  TGCN_CHECK_LAUNCH("tgcn_relu_pool_bwd_f32");
  return TGCN_OK;
}

// tgcn_relu_pool_bwd_f32's routing for time rows [t0, t0 + rows) of whole pooled tensors into a dense slab (pool_relayout.h)
int tgcn_relu_pool_bwd_rows_f32(void* stream, const float* grad_z, const float* z, const uint8_t* idx, float* grad_y, int64_t S, int64_t n,
                                int32_t out_T, int32_t t0, int32_t rows, int32_t N, int32_t pool, int32_t as_series, float scale) {
  if (!grad_z || !z || !idx || !grad_y || S <= 0 || n <= 0 || N <= 0 || pool <= 0 || pool > 255 || n % pool != 0 || out_T < 1 || t0 < 0 || rows < 1 ||
      (int64_t)t0 + rows > (int64_t)out_T || !isfinite(scale))
    TGCN_FAIL(TGCN_ERR_INVALID, "relu_pool_bwd_rows: bad argument");
  if (S > INT64_MAX / n || S * n > INT64_MAX / out_T || S * n * out_T > INT64_MAX / N) TGCN_FAIL(TGCN_ERR_INVALID, "relu_pool_bwd_rows: bad argument");
  const int64_t total = S * n * rows * N;
  hipLaunchKernelGGL(relu_pool_bwd_rows_kernel, dim3(grid_1d(total)), dim3(kBlock), 0, (hipStream_t)stream, grad_z, z, idx, grad_y, total, n, (int64_t)out_T,
                     (int64_t)t0, (int64_t)rows, (int)N, (int)pool, as_series != 0, scale);
  TGCN_CHECK_LAUNCH("tgcn_relu_pool_bwd_rows_f32");
  return TGCN_OK;
}

// Workspace of the project-first path: Z (q*n x K*N) + 3 result buffers (q*n x N) + hop scratch.
static void pf_ws_layout(const tgcn_csr_sched* S, int32_t K, int64_t q, int64_t n, int32_t N, size_t* z_bytes, size_t* y_bytes,
                         size_t* off_part, size_t* total) {
  *z_bytes = align_up((size_t)q * n * K * N * sizeof(float), 256);
  *y_bytes = align_up((size_t)q * n * N * sizeof(float), 256);
  *off_part = *z_bytes + 3 * *y_bytes;
  *total = *off_part + align_up(tgcn_csr_hop_workspace_bytes(S, (int32_t)q, N, N % 4 == 0), 256);
}

size_t tgcn_cheb_forward_pf_workspace_bytes(const tgcn_csr_sched* S, int32_t K, int64_t q, int64_t n, int32_t N) {
  if (!S || K < 1 || q < 1 || n < 1 || N < 1) return 0;
  size_t a, b, c, t;
  pf_ws_layout(S, K, q, n, N, &a, &b, &c, &t);
  return t;
}

int tgcn_cheb_forward_pf_f32(void* stream, const tgcn_csr* A, const tgcn_csr_sched* S, int32_t mode, int32_t K, int64_t q,
                             int64_t n, int32_t C, int32_t N, const float* x, const float* Wcat, const float* bias,
                             int32_t bias_kind, float* out, void* workspace, size_t workspace_bytes) {
  if (!A || !S || !x || !Wcat || !out) TGCN_FAIL(TGCN_ERR_INVALID, "forward_pf: null operand");
  if (int drc = check_pointer_device(x, (hipStream_t)stream, "forward_pf")) return drc;
  if (K < 1 || q < 1 || n < 1 || C < 1 || N < 1 || n != A->n || q > 65535) TGCN_FAIL(TGCN_ERR_INVALID, "forward_pf: bad shape");
  if (mode != 0 && mode != 1) TGCN_FAIL(TGCN_ERR_INVALID, "forward_pf: mode %d", mode);
  size_t z_bytes, y_bytes, off_part, total;
  pf_ws_layout(S, K, q, n, N, &z_bytes, &y_bytes, &off_part, &total);
  if (!workspace || workspace_bytes < total || ((uintptr_t)workspace & 15)) TGCN_FAIL(TGCN_ERR_WORKSPACE, "forward_pf: workspace %zu < %zu", workspace_bytes, total);
  char* ws = (char*)workspace;
  const int64_t M = q * n, KN = (int64_t)K * N;
  float* Zb = (K == 1) ? out : (float*)ws;      // K == 1: the projection IS the layer
  const float* a1[1] = {x};
  const int64_t lda1[1] = {C};
  int rc = project_impl(stream, M, C, (int32_t)KN, 1, a1, lda1, Wcat, bias, bias_kind, n, 1, 0, Zb, KN, 0, 0, N);
  if (rc != TGCN_OK || K == 1) return rc;
  float* part = (float*)(ws + off_part);
  const size_t part_bytes = total - off_part;
  auto zview = [&](int j) { return tgcn_dense{Zb + (int64_t)j * N, n * KN, KN}; };
  auto ybuf = [&](int i) { return tgcn_dense{(float*)(ws + z_bytes + (size_t)i * y_bytes), n * (int64_t)N, N}; };
  const tgcn_dense outd = {out, n * (int64_t)N, N};
  if (mode == 0) {            // Horner: Y_j = Z_j + L Y_{j+1}
    tgcn_dense cur = zview(K - 1);
    for (int j = K - 2; j >= 0; --j) {
      const tgcn_dense zj = zview(j);
      const tgcn_dense dst = (j == 0) ? outd : ybuf(j & 1);
      rc = tgcn_csr_hop2_f32(stream, A, S, (int32_t)q, N, &cur, &zj, 1.f, 1.f, nullptr, 0.f, &dst, nullptr, part, part_bytes);
      if (rc != TGCN_OK) return rc;
      cur = dst;
    }
  } else {                    // Clenshaw: b_k = Z_k + 2 L b_{k+1} - b_{k+2};  out = Z_0 + L b_1 - b_2
    tgcn_dense b1 = zview(K - 1), b2 = {nullptr, 0, 0};
    for (int k = K - 2; k >= 0; --k) {
      const tgcn_dense zk = zview(k);
      const tgcn_dense dst = (k == 0) ? outd : ybuf(k % 3);
      rc = tgcn_csr_hop2_f32(stream, A, S, (int32_t)q, N, &b1, b2.ptr ? &b2 : nullptr, k == 0 ? 1.f : 2.f, -1.f, &zk, 1.f, &dst,
                             nullptr, part, part_bytes);
      if (rc != TGCN_OK) return rc;
      b2 = b1;
      b1 = dst;
    }
  }
  return TGCN_OK;
}

// The first step of the project-first form on its own: the vertex-sharded layer (tgcn_amd/dist.py) issues its hops itself -- each one behind
// an exchange of the previous result's cut rows -- so it needs Z without the recursion that tgcn_cheb_forward_pf_f32 runs behind it.
int tgcn_cheb_project_first_f32(void* stream, int64_t q, int64_t rows, int32_t C, int32_t K, int32_t N, const float* x, const float* Wcat,
                                const float* bias, int32_t bias_kind, const int32_t* rowmap, float* Z) {
  if (!x || !Wcat || !Z) TGCN_FAIL(TGCN_ERR_INVALID, "project_first: null operand");
  if (q < 1 || rows < 1 || C < 1 || K < 1 || N < 1 || (int64_t)K * N > (int64_t)INT32_MAX) TGCN_FAIL(TGCN_ERR_INVALID, "project_first: bad shape");
  if (int drc = check_pointer_device(x, (hipStream_t)stream, "project_first")) return drc;
  const int64_t KN = (int64_t)K * N;
  const float* a1[1] = {x};
  const int64_t lda1[1] = {C};
  if (!rowmap) return project_impl(stream, q * rows, C, (int32_t)KN, 1, a1, lda1, Wcat, bias, bias_kind, rows, 1, 0, Z, KN, 0, 0, N);
  const int64_t a_bs[1] = {rows * (int64_t)C};
  return project_impl(stream, rows, C, (int32_t)KN, 1, a1, lda1, Wcat, bias, bias_kind, rows, 1, 0, Z, KN, 0, 0, N, rowmap, 0u, (int32_t)q, a_bs, rows * KN);
}

static int windows_chunks(int64_t M) { const int64_t c = (M + 16383) / 16384; return (int)(c < 1 ? 1 : (c > 256 ? 256 : c)); }

size_t tgcn_cheb_windows_wgrad_workspace_bytes(int64_t S, int64_t n_vertices, int32_t T, int32_t H, int32_t N, int32_t K) {
  if (S < 1 || n_vertices < 1 || H < 1 || T < H || N < 1 || K < 1) return 0;
  return (size_t)windows_chunks(S * (T - H + 1) * n_vertices) * K * H * N * sizeof(float);
}

int tgcn_cheb_windows_backward_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t H, int32_t N, int32_t K,
                                   const float* stack, const float* g, const float* W, float* G, float* dW, void* workspace,
                                   size_t workspace_bytes) {
  if (S < 1 || n_vertices < 1 || H < 1 || T < H || N < 1 || K < 1 || !g) TGCN_FAIL(TGCN_ERR_INVALID, "windows_backward: bad argument");
  if ((int64_t)K * H > 65535) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "windows_backward: K*H > 65535");
  hipStream_t st = (hipStream_t)stream;
  if (G) {
    if (!W) TGCN_FAIL(TGCN_ERR_INVALID, "windows_backward: the input gradient needs W");
    hipLaunchKernelGGL(windows_dgrad_kernel, dim3(grid_1d((int64_t)K * S * n_vertices * T)), dim3(kBlock), 0, st, g, W, G, S, n_vertices, T, H, N, K);
  }
  if (dW) {
    if (!stack) TGCN_FAIL(TGCN_ERR_INVALID, "windows_backward: the weight gradient needs the hop tensors");
    const int nchunks = windows_chunks(S * (T - H + 1) * n_vertices);
    const size_t need = (size_t)nchunks * K * H * N * sizeof(float);
    if (!workspace || workspace_bytes < need) TGCN_FAIL(TGCN_ERR_WORKSPACE, "windows_backward: workspace %zu < %zu", workspace_bytes, need);
    hipLaunchKernelGGL(windows_wgrad_partial_kernel, dim3((unsigned)(K * H), (unsigned)((N + 63) / 64), (unsigned)nchunks), dim3(kBlock), 0, st, stack, g,
                       (float*)workspace, S, n_vertices, T, H, N, nchunks);
    const int64_t count = (int64_t)K * H * N;
    hipLaunchKernelGGL(windows_wgrad_reduce_kernel, dim3(grid_1d(count)), dim3(kBlock), 0, st, (const float*)workspace, dW, count, nchunks);
  }
  TGCN_CHECK_LAUNCH("tgcn_cheb_windows_backward_f32");
  return TGCN_OK;
}

// ---- streaming time windows of multi-channel series (windows.h, windows_bf16.h)
// The host side of every entry below is built from four pieces: one geometry (series_geom, series_stream_check), one set
// of fillers for the kernels' parameter structs, one trait per element type (SeriesF32, SeriesBf16) and three drivers templated on it --
// series_forward (a whole series), series_chunk_forward (a chunk behind a ring) and series_backward.  The exported entries name their
// rule and forward.
// The drivers are templates, so the section leaves the extern "C" block; its exported entries keep C linkage from tgcn_hip.h's declarations.
}  // extern "C"

// Chooses HC (weight time rows per staged span) and the dynamic LDS of series_gemm_kernel: the whole horizon when four spans and the weight
// tile fit 64 KB, else the largest chunk that does, else the largest that fits the device's opt-in limit; 0 when even one row does not.
// stride: the window step (the span of hc rows then holds 31 * min(stride, hc) + hc time rows, series_span_floats).
static int series_gemm_lds(int H, int f, int NT, bool vec, int stride, int* hc_out) {
  const int ws = kSgKT * series_ws_stride(NT);
  auto bytes = [&](int hc) { return (size_t)(ws + 4 * (size_t)series_span_floats(hc, f, vec, stride)) * sizeof(float); };      // 64-bit
  const size_t limits[2] = {64 * 1024, (size_t)lds_optin_limit()};
  for (size_t lim : limits)
    for (int hc = H; hc >= 1; --hc)
      if (bytes(hc) <= lim) { *hc_out = hc; return (int)bytes(hc); }      // <= the limit: the kernel's 32-bit span arithmetic is safe
  return 0;
}

// series_gemm_lds's three regimes on bf16 span bytes: the weight tile is NT*16 columns of kPbLd bf16
static int series_gemm_bf16_lds(int H, int f, int NT, bool vec, int stride, int* hc_out) {
  auto bytes = [&](int hc) { return ((size_t)NT * 16 * kPbLd + 4 * (size_t)series_bf16_span_elems(hc, f, vec, stride)) * sizeof(hbf16); };   // 64-bit
  const size_t limits[2] = {64 * 1024, (size_t)lds_optin_limit()};
  for (size_t lim : limits)
    for (int hc = H; hc >= 1; --hc)
      if (bytes(hc) <= lim) { *hc_out = hc; return (int)bytes(hc); }
  return 0;
}
typedef int (*SeriesLdsFn)(int H, int f, int NT, bool vec, int stride, int* hc_out);

static int series_gemm_nt(int N) { return N <= 16 ? 1 : (N <= 32 ? 2 : 4); }

// The pooled form's scratch [wave][window][col] lives where the weight tile and the spans were: the launch takes the larger of the two
static int series_pool_lds(int gemm_lds, int NT) { const int sc = 4 * kSgWin * NT * 16 * (int)sizeof(float); return gemm_lds > sc ? gemm_lds : sc; }
static bool series_pool_ok(int64_t n, int32_t pool) { return (pool == 2 || pool == 4) && n >= 1 && n % pool == 0; }

// The four plan queries: pooled asks for pool 2 / 4 and answers the pooled launch's bytes
static int series_plan(const char* who, SeriesLdsFn lds_of, int32_t H, int32_t f, int32_t N, bool vec, int32_t stride, bool pooled, int32_t pool,
                       int32_t* hc, int32_t* lds_bytes) {
  if (H < 1 || f < 1 || N < 1 || stride < 1 || (pooled && pool != 2 && pool != 4) || !hc || !lds_bytes) TGCN_FAIL(TGCN_ERR_INVALID, "%s: bad argument", who);
  int h = 0;
  const int lds = lds_of(H, f, series_gemm_nt(N), vec, stride, &h);
  if (!lds) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "%s: %d channels per time row do not fit the LDS span", who, f);
  *hc = h; *lds_bytes = pooled ? series_pool_lds(lds, series_gemm_nt(N)) : lds;
  return TGCN_OK;
}

int tgcn_series_gemm_plan(int32_t H, int32_t f, int32_t N, int32_t vec, int32_t* hc, int32_t* lds_bytes) {
  return series_plan("series_gemm_plan", series_gemm_lds, H, f, N, vec != 0, 1, false, 0, hc, lds_bytes);
}
int tgcn_series_conv_plan(int32_t H, int32_t f, int32_t N, int32_t vec, int32_t stride, int32_t* hc, int32_t* lds_bytes) {
  return series_plan("series_conv_plan", series_gemm_lds, H, f, N, vec != 0, stride, false, 0, hc, lds_bytes);
}
int tgcn_series_pool_plan(int32_t H, int32_t f, int32_t N, int32_t vec, int32_t stride, int32_t pool, int32_t* hc, int32_t* lds_bytes) {
  return series_plan("series_pool_plan", series_gemm_lds, H, f, N, vec != 0, stride, true, pool, hc, lds_bytes);
}
int tgcn_series_conv_plan_bf16(int32_t H, int32_t f, int32_t N, int32_t vec, int32_t stride, int32_t* hc, int32_t* lds_bytes) {
  return series_plan("series_conv_plan_bf16", series_gemm_bf16_lds, H, f, N, vec != 0 && f % 8 == 0, stride, false, 0, hc, lds_bytes);
}

// Phase-major tiles of the DILATED kernels: min(dil, nwin) phases hold a window, the longest ceil(nwin / dil) of them.
// 2 <= dil < the padded series (series_dilated_check), so nothing here leaves 32 bits.
static void series_dilated_tiles(int32_t nwin, int32_t dil, int32_t* tpp, int32_t* tpv) {
  const int32_t nph = dil < nwin ? dil : nwin;
  *tpp = ((nwin - 1) / dil + 1 + kSgWin - 1) / kSgWin;
  *tpv = nph * *tpp;
}

// Everything about one GEMM launch that can refuse: the tiles and the grid's limits, then the plan.  Both launchers start here, and so does
// the chunk backward, which has to know before its first launch.
struct SeriesLaunchPlan { int32_t tpp, tpv, hc, lds, NT; int64_t nq, ntiles, gx, gy; };
// A launch holds fewer than 2^32 threads along x.  The runtime this was met on (ROCm 7.2, gfx950) counts a grid's work-items in 32 bits and runs a
// larger grid only modulo 2^32, without an error: 16 one-window phase tiles per vertex on 4.2 M vertex rows are 16.8 M workgroups of 256, and
// only (16.8 M * 256) mod 2^32 threads ran.  Another runtime may refuse such a grid instead; either way no launch here asks for one.  The
// launchers issue the grid in parts of kSeriesGridPart workgroups, each told its first workgroup (blk0); the parts write disjoint tiles.
// A launch error of any part is what every driver ends on (series_launched: hipGetLastError after its last launch).
constexpr int64_t kSeriesGridPart = (int64_t)UINT32_MAX / kBlock;
static int series_launch_plan(SeriesLdsFn lds_of, int64_t S, int64_t n, int32_t nwin, int32_t H, int32_t f, int32_t N, bool vec, int stride, int dil,
                              int pool, const char* who, SeriesLaunchPlan* o) {
  o->tpp = 0; o->tpv = (nwin + kSgWin - 1) / kSgWin;
  if (dil > 1) series_dilated_tiles(nwin, dil, &o->tpp, &o->tpv);
  o->nq = pool ? (n + 3) / 4 : 0;                      // pooled: one workgroup per (recording, vertex quad, window block)
  o->ntiles = S * (pool ? o->nq : n) * o->tpv;
  o->gx = pool ? o->ntiles : (o->ntiles + 3) / 4;
  o->NT = series_gemm_nt(N);
  o->gy = ((int64_t)N + o->NT * 16 - 1) / (o->NT * 16);
  if (o->gx > (int64_t)INT32_MAX || o->gy > 65535) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "%s: grid too large", who);
  o->lds = lds_of(H, f, o->NT, vec, stride, &o->hc);
  if (!o->lds) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "%s: %d channels per time row do not fit the LDS span", who, f);
  return TGCN_OK;
}

// ---- which instantiation a GEMM launch takes.  Choosing is apart from launching: series_form maps the launcher's arguments to a kernel
// family and its flags, series_*_form_built name the forms the library holds (the launcher's `if constexpr` guard, and what its refusals
// ask), and the static_asserts pin arguments -> form, one row per form an entry reaches.
//   stride >= 2: STRIDED; dil >= 2 (at step 1, planned as step 1): DILATED; stride 1 (the input gradient's phases included): neither
//   carry (the stream entries): CARRY, the time rows before the chunk staged from p.ring -- at step 1 (dilated or not), or STRIDED && CARRY
//     for a window step on a chunk (the _stream_strided entry, p.win_off)
//   pool (2 / 4; 0: none): POOLED, the same form with one workgroup per (recording, vertex quad, window block) and the scratch's bytes where
//     they exceed the GEMM's; not built with a window step on a chunk
//   drop (with pool, on a whole series): series_gemm_pool_dropout_kernel in the pooled form's place, on the same plan -- the dropout adds no LDS
//   at (with drop, at step 1; a chunk's place in the whole series): series_gemm_chunk_pool_dropout_kernel, behind the ring (carry) or without one
// Precedence where both a step and a dilation arrive: a whole series looks at the dilation first, a chunk behind a ring at the step first.
// `at` without a ring is one tap (series_chunk_forward plans it at dil 1): never DILATED, whatever dil says.
enum SeriesFamily { kSgGemm, kSgDrop, kSgDropAt };
struct SeriesForm { SeriesFamily family; bool strided, dilated, carry, pooled; };
constexpr SeriesForm series_form(int stride, int dil, bool carry, int pool, bool drop, bool at) {
  const SeriesFamily family = at ? kSgDropAt : (drop ? kSgDrop : kSgGemm);
  if (carry || at) return {family, stride > 1, carry && stride <= 1 && dil > 1, carry, pool != 0};
  return {family, dil <= 1 && stride != 1, dil > 1, false, pool != 0};
}
// series_gemm_kernel<NT, VEC, STRIDED, DILATED, CARRY, POOLED>: 11 forms
constexpr bool series_gemm_form_built(bool s, bool d, bool c, bool p) { return !(s && d) && !(s && c && p); }
// series_gemm_pool_dropout_kernel<NT, VEC, STRIDED, DILATED>: the pooled forms of a whole series
constexpr bool series_drop_form_built(bool s, bool d, bool c, bool p) { return series_gemm_form_built(s, d, c, p) && p && !c; }
// series_gemm_chunk_pool_dropout_kernel<NT, VEC, DILATED, CARRY>: the pooled forms at step 1, dilated only behind a ring
constexpr bool series_drop_at_form_built(bool s, bool d, bool c, bool p) { return series_gemm_form_built(s, d, c, p) && p && !s && (c || !d); }

constexpr bool series_form_is(SeriesForm f, SeriesFamily family, bool s, bool d, bool c, bool p) {
  return f.family == family && f.strided == s && f.dilated == d && f.carry == c && f.pooled == p;
}
//                                       stride dil carry pool drop   at                STRIDED DILATED CARRY POOLED
static_assert(series_form_is(series_form(1, 1, false, 2, true,  true),  kSgDropAt, false, false, false, true), "");
static_assert(series_form_is(series_form(1, 3, false, 2, true,  true),  kSgDropAt, false, false, false, true), "");      // one tap: dil is not looked at
static_assert(series_form_is(series_form(1, 2, true,  2, true,  true),  kSgDropAt, false, true,  true,  true), "");
static_assert(series_form_is(series_form(1, 1, true,  4, true,  true),  kSgDropAt, false, false, true,  true), "");
static_assert(series_form_is(series_form(1, 2, false, 2, true,  false), kSgDrop,   false, true,  false, true), "");
static_assert(series_form_is(series_form(1, 1, false, 4, true,  false), kSgDrop,   false, false, false, true), "");
static_assert(series_form_is(series_form(2, 1, false, 2, true,  false), kSgDrop,   true,  false, false, true), "");
static_assert(series_form_is(series_form(1, 2, true,  2, false, false), kSgGemm,   false, true,  true,  true), "");
static_assert(series_form_is(series_form(1, 1, true,  4, false, false), kSgGemm,   false, false, true,  true), "");
static_assert(series_form_is(series_form(1, 2, false, 2, false, false), kSgGemm,   false, true,  false, true), "");
static_assert(series_form_is(series_form(1, 1, false, 4, false, false), kSgGemm,   false, false, false, true), "");
static_assert(series_form_is(series_form(3, 1, false, 2, false, false), kSgGemm,   true,  false, false, true), "");
static_assert(series_form_is(series_form(2, 1, true,  0, false, false), kSgGemm,   true,  false, true,  false), "");
static_assert(series_form_is(series_form(2, 2, true,  0, false, false), kSgGemm,   true,  false, true,  false), "");     // a chunk: the step first
static_assert(series_form_is(series_form(1, 2, true,  0, false, false), kSgGemm,   false, true,  true,  false), "");
static_assert(series_form_is(series_form(1, 1, true,  0, false, false), kSgGemm,   false, false, true,  false), "");
static_assert(series_form_is(series_form(1, 2, false, 0, false, false), kSgGemm,   false, true,  false, false), "");
static_assert(series_form_is(series_form(2, 2, false, 0, false, false), kSgGemm,   false, true,  false, false), "");     // a whole series: the dilation first
static_assert(series_form_is(series_form(1, 1, false, 0, false, false), kSgGemm,   false, false, false, false), "");
static_assert(series_form_is(series_form(2, 1, false, 0, false, false), kSgGemm,   true,  false, false, false), "");
// the three refusals: a pooled window step on a chunk; dropout without the pool or behind a ring without `at`; `at` with a step
static_assert(!series_gemm_form_built(true, false, true, true) && series_form_is(series_form(2, 1, true, 2, false, false), kSgGemm, true, false, true, true), "");
static_assert(!series_drop_form_built(false, false, false, false) && !series_drop_form_built(false, false, true, true), "");
static_assert(!series_drop_at_form_built(true, false, false, true) && !series_drop_at_form_built(false, true, false, true), "");

static int series_gemm_launch(hipStream_t st, SeriesGemmParams& p, int64_t S, bool vec, const char* who, int stride = 1, int dil = 1,
                              bool carry = false, int pool = 0, const DropoutParams* drop = nullptr, const SeriesDropAt* at = nullptr) {
  SeriesLaunchPlan lp;
  if (int rc = series_launch_plan(series_gemm_lds, S, p.n, p.nwin, p.H, p.f, p.N, vec, stride, dil, pool, who, &lp)) return rc;
  const SeriesForm fm = series_form(stride, dil, carry, pool, drop != nullptr, at != nullptr);
  if (!series_gemm_form_built(fm.strided, fm.dilated, fm.carry, fm.pooled))
    TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "%s: a pooled window step on a chunk is not built", who);
  if (drop && !(at ? fm.pooled : series_drop_form_built(fm.strided, fm.dilated, fm.carry, fm.pooled)))
    TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "%s: dropout is built into the pooled epilogue of a whole series", who);
  if (at && !(drop && series_drop_at_form_built(fm.strided, fm.dilated, fm.carry, fm.pooled)))
    TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "%s: a chunk's mask is built at step 1 with dropout", who);
  p.tpv = lp.tpv; p.dil = dil; p.ntiles = lp.ntiles; p.pool = pool;
  if (dil > 1) p.tpp = lp.tpp;
  if (pool) p.nq = lp.nq;
  const int hc = lp.hc, lds = pool ? series_pool_lds(lp.lds, lp.NT) : lp.lds;
  p.HC = hc;
  p.stride = stride; p.lst = series_span_lst(hc, stride); p.fp = series_row_floats(hc, p.f, vec, stride);
  ProfScope ps(TGCN_PROF_PROJECT, st);
  const auto run = [&](auto kernel, const auto&... extra) {
    launch_kernel_parts(kernel, lp.gx, kSeriesGridPart, (unsigned)lp.gy, dim3(kBlock), lds, st, p, extra...);
  };
  with_one_of<1, 2, 4>(lp.NT, [&](auto NT) { with_flags([&](auto V, auto St, auto Di, auto Ca, auto Po) {
    if constexpr (series_gemm_form_built(St, Di, Ca, Po)) {
      if (fm.family == kSgGemm) run(series_gemm_kernel<NT, V, St, Di, Ca, Po>);
    }
    if constexpr (series_drop_form_built(St, Di, Ca, Po)) {
      if (fm.family == kSgDrop) run(series_gemm_pool_dropout_kernel<NT, V, St, Di>, *drop);
    }
    if constexpr (series_drop_at_form_built(St, Di, Ca, Po)) {
      if (fm.family == kSgDropAt) run(series_gemm_chunk_pool_dropout_kernel<NT, V, Di, Ca>, *drop, *at);
    }
  }, vec, fm.strided, fm.dilated, fm.carry, fm.pooled); });
  return TGCN_OK;
}

// series_gemm_bf16_kernel<NT, VEC, STRIDED, OutT, DILATED, CARRY>: 8 forms.  out_f32 (the input gradient's fp32 columns; otherwise bf16
// output) exists only without a ring and at step 1, dilated or not -- one launch per phase of a stepped layer's input gradient, each at
// step 1.  There is no bf16 pool, dropout or `at`.  The step and the dilation as above.
struct SeriesBf16Form { bool strided, out_f32, dilated, carry; };
constexpr SeriesBf16Form series_bf16_form(int stride, int dil, bool carry, bool out_f32) {
  if (carry) return {stride > 1, false, stride <= 1 && dil > 1, true};
  return {dil <= 1 && !out_f32 && stride != 1, out_f32, dil > 1, false};
}
constexpr bool series_bf16_form_built(bool s, bool o, bool d, bool c) { return !(s && d) && !(o && (s || c)); }

constexpr bool series_bf16_form_is(SeriesBf16Form f, bool s, bool o, bool d, bool c) {
  return f.strided == s && f.out_f32 == o && f.dilated == d && f.carry == c;
}
//                                                 stride dil carry out_f32   STRIDED f32    DILATED CARRY
static_assert(series_bf16_form_is(series_bf16_form(2, 1, true,  false), true,  false, false, true), "");
static_assert(series_bf16_form_is(series_bf16_form(2, 2, true,  false), true,  false, false, true), "");      // a chunk: the step first
static_assert(series_bf16_form_is(series_bf16_form(1, 2, true,  false), false, false, true,  true), "");
static_assert(series_bf16_form_is(series_bf16_form(1, 1, true,  false), false, false, false, true), "");
static_assert(series_bf16_form_is(series_bf16_form(1, 1, true,  true),  false, false, false, true), "");      // a chunk's output is bf16
static_assert(series_bf16_form_is(series_bf16_form(1, 2, false, true),  false, true,  true,  false), "");
static_assert(series_bf16_form_is(series_bf16_form(1, 2, false, false), false, false, true,  false), "");
static_assert(series_bf16_form_is(series_bf16_form(2, 2, false, false), false, false, true,  false), "");     // a whole series: the dilation first
static_assert(series_bf16_form_is(series_bf16_form(1, 1, false, true),  false, true,  false, false), "");
static_assert(series_bf16_form_is(series_bf16_form(2, 1, false, true),  false, true,  false, false), "");     // fp32 columns: at step 1
static_assert(series_bf16_form_is(series_bf16_form(1, 1, false, false), false, false, false, false), "");
static_assert(series_bf16_form_is(series_bf16_form(2, 1, false, false), true,  false, false, false), "");

static int series_gemm_bf16_launch(hipStream_t st, SeriesGemmBf16Params& p, int64_t S, bool vec, bool out_f32, const char* who, int stride = 1,
                                   int dil = 1, bool carry = false) {
  SeriesLaunchPlan lp;
  if (int rc = series_launch_plan(series_gemm_bf16_lds, S, p.n, p.nwin, p.H, p.f, p.N, vec, stride, dil, 0, who, &lp)) return rc;
  p.tpv = lp.tpv; p.dil = dil; p.ntiles = lp.ntiles;
  if (dil > 1) p.tpp = lp.tpp;
  const int hc = lp.hc;
  p.HC = hc;
  p.stride = stride; p.lst = series_span_lst(hc, stride); p.fp = vec ? series_bf16_row_elems(p.f, p.lst) : p.f;
  const SeriesBf16Form fm = series_bf16_form(stride, dil, carry, out_f32);
  ProfScope ps(TGCN_PROF_PROJECT, st);
  with_one_of<1, 2, 4>(lp.NT, [&](auto NT) { with_flags([&](auto V, auto St, auto F32, auto Di, auto Ca) {
    if constexpr (series_bf16_form_built(St, F32, Di, Ca))
      launch_kernel_parts(series_gemm_bf16_kernel<NT, V, St, std::conditional_t<F32, float, hbf16>, Di, Ca>, lp.gx, kSeriesGridPart, (unsigned)lp.gy,
                          dim3(kBlock), lp.lds, st, p);
  }, vec, fm.strided, fm.out_f32, fm.dilated, fm.carry); });
  return TGCN_OK;
}

// ---- one trait per element type: what the drivers below need to know about fp32 and bf16 tensors
struct SeriesF32 {
  typedef float Elem;
  typedef SeriesGemmParams Params;
  typedef SeriesWgradParams WgradParams;
  static constexpr int kUnit = 4;                    // elements per 16-byte access
  static constexpr const char* kSuffix = "_f32";     // "tgcn_cheb_" + who + kSuffix is the entry's name
  static constexpr SeriesLdsFn lds = series_gemm_lds;
  static int launch(hipStream_t st, Params& p, int64_t S, bool vec, bool, const char* who, int stride, int dil, bool carry, int pool,
                    const DropoutParams* drop = nullptr, const SeriesDropAt* at = nullptr) {
    return series_gemm_launch(st, p, S, vec, who, stride, dil, carry, pool, drop, at);
  }
  static void set_bias(Params& p, const void* bias, int32_t kind, int32_t) { p.bias = (const float*)bias; p.bias_kind = kind; }
  static void flip(hipStream_t st, const float* W, float* Wd, int K, int H, int f, int N, int stride) {
    hipLaunchKernelGGL(series_flip_weight_kernel, dim3(grid_1d((int64_t)K * H * f * N)), dim3(kBlock), 0, st, W, Wd, K, H, f, N, stride);
  }
  static void wgrad_rows(WgradParams& q, int64_t ld) { q.Tf = (int32_t)ld; }
  static void wgrad_ring(WgradParams& q, const void* ring, int64_t S, int64_t n, int64_t ring_ld, int32_t C, int32_t head) {
    q.ring = (const float*)ring; q.ring_ks = S * n * ring_ld; q.ring_is = ring_ld; q.C = C; q.head = head;
  }
  // conv: a step or padding; carried: the chunk behind a ring.  series_wgrad_partial_kernel<CONV, DIL, CARRY>: dilated taps and a carried
  // chunk are CONV geometries whatever `conv` says -- 5 forms
  static void wgrad(hipStream_t st, dim3 grid, const WgradParams& q, bool conv, bool dilated, bool carried) {
    with_flags([&](auto Co, auto Di, auto Ca) {
      if constexpr (Co || (!Di && !Ca)) launch_kernel(series_wgrad_partial_kernel<Co, Di, Ca>, grid, dim3(64), 0, st, q);
    }, conv || dilated || carried, dilated, carried);
  }
};

struct SeriesBf16 {
  typedef hbf16 Elem;
  typedef SeriesGemmBf16Params Params;
  typedef SeriesWgradBf16Params WgradParams;
  static constexpr int kUnit = 8;
  static constexpr const char* kSuffix = "";         // who ends in _bf16
  static constexpr SeriesLdsFn lds = series_gemm_bf16_lds;
  static int launch(hipStream_t st, Params& p, int64_t S, bool vec, bool out_f32, const char* who, int stride, int dil, bool carry, int,
                    const DropoutParams* = nullptr, const SeriesDropAt* = nullptr) {      // no bf16 dropout
    return series_gemm_bf16_launch(st, p, S, vec, out_f32, who, stride, dil, carry);
  }
  static void set_bias(Params& p, const void* bias, int32_t kind, int32_t dtype) { p.bias = bias; p.bias_kind = kind; p.bias_bf16 = dtype == TGCN_DTYPE_BF16; }
  static void flip(hipStream_t st, const hbf16* W, hbf16* Wd, int K, int H, int f, int N, int stride) {
    hipLaunchKernelGGL(series_flip_weight_bf16_kernel, dim3(grid_1d((int64_t)K * H * f * N)), dim3(kBlock), 0, st, W, Wd, K, H, f, N, stride);
  }
  static void wgrad_rows(WgradParams& q, int64_t ld) { q.st_is = ld; }
  static void wgrad_ring(WgradParams&, const void*, int64_t, int64_t, int64_t, int32_t, int32_t) {}      // no bf16 chunk backward
  static void wgrad(hipStream_t st, dim3 grid, const WgradParams& q, bool conv, bool dilated, bool) {      // <CONV, DIL>: 3 forms, as above
    with_flags([&](auto Co, auto Di) {
      if constexpr (Co || !Di) launch_kernel(series_wgrad_bf16_partial_kernel<Co, Di>, grid, dim3(64), 0, st, q);
    }, conv || dilated, dilated);
  }
};

// ---- one geometry
static bool series_shape_ok(int64_t S, int64_t n, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K) {
  return S >= 1 && n >= 1 && n < (int64_t)INT32_MAX && f >= 1 && H >= 1 && T >= H && N >= 1 && K >= 1 && (int64_t)T * f < (int64_t)INT32_MAX &&
         (int64_t)H * f < (int64_t)INT32_MAX / 2 && (int64_t)H * N < (int64_t)INT32_MAX / 2 && (int64_t)K * f < (int64_t)INT32_MAX;
}

// The geometry of the strided, zero-padded entries: pads within a window (every window touches a real row), the padded series holds a window,
// and 64 padded series stay inside 32-bit time arithmetic (a wave addresses 32 windows of it)
static bool series_conv_shape_ok(int64_t S, int64_t n, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K, int32_t stride, int32_t pl, int32_t pr) {
  if (!(H >= 1 && T >= 1 && stride >= 1 && pl >= 0 && pr >= 0 && pl < H && pr < H)) return false;
  const int64_t Tp = (int64_t)T + pl + pr;
  return Tp >= H && Tp * 64 < (int64_t)INT32_MAX && Tp * f < (int64_t)INT32_MAX && series_shape_ok(S, n, (int32_t)Tp, f, H, N, K);
}
// A step beyond the padded series leaves one window, as every step above Tp - H does: clamped, so that 32 * stride stays a 32-bit number
static int32_t series_conv_stride(int32_t T, int32_t stride, int32_t pl, int32_t pr) { return stride < T + pl + pr ? stride : T + pl + pr; }
static int64_t series_conv_nwin(int32_t T, int32_t H, int32_t stride, int32_t pl, int32_t pr) { return ((int64_t)T + pl + pr - H) / stride + 1; }

// Dilated taps: the window spans He = (H - 1) * dilation + 1 time rows, and He takes H's place in the geometry rules of the _conv entries.
// TGCN_OK, TGCN_ERR_INVALID for a bad value, TGCN_ERR_UNSUPPORTED for dilation > 1 with stride > 1 (not built).  *He_out: the span.
// For H >= 2 the span bounds the dilation, dil < He <= Tp < 2^25: the 32 windows of a wave, dil time rows apart, stay inside 32 bits.
static int series_dilated_check(int64_t S, int64_t n, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K, int32_t stride, int32_t pl, int32_t pr,
                                int32_t dil, int32_t* He_out) {
  if (dil < 1 || H < 1 || T < 1) return TGCN_ERR_INVALID;
  const int64_t He = ((int64_t)H - 1) * dil + 1;
  if (He > (int64_t)T + (pl > 0 ? pl : 0) + (pr > 0 ? pr : 0) || He >= (int64_t)INT32_MAX / 64) return TGCN_ERR_INVALID;
  // the He-row window in the _conv rules (pads below He, the padded series holds a window, 32-bit time arithmetic); the weight's own H for the rest
  if (!series_conv_shape_ok(S, n, T, f, (int32_t)He, N, K, stride, pl, pr) || !series_shape_ok(S, n, (int32_t)((int64_t)T + pl + pr), f, H, N, K))
    return TGCN_ERR_INVALID;
  if (dil > 1 && stride > 1) return TGCN_ERR_UNSUPPORTED;
  if (dil > 1 && dil >= He) return TGCN_ERR_INVALID;   // H == 1: no span bounds the dilation (series_geom takes it as the undilated window)
  *He_out = (int32_t)He;
  return TGCN_OK;
}

// What a whole-series entry runs at, from what its caller passed, under the entry's rule: plain (no step, no pads: T * 64 is not bounded),
// conv (step and pads; the step clamped) or dilated (conv's rules on the He-row window; at dilation 1 conv itself).  One tap has nothing to
// dilate: H == 1 at any dilation >= 1 is the undilated window (at stride 1; with a step the combination stays refused like every
// dilation > 1), so no dilation without a bound reaches a kernel.  Every forward entry, backward entry and workspace query starts here.
enum SeriesRule { kSeriesPlain, kSeriesConv, kSeriesDilated };
struct SeriesGeom { int32_t stride, pl, pr, dil, He; int64_t nwin; };
static int series_geom(SeriesRule rule, int64_t S, int64_t n, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K, int32_t stride, int32_t pl,
                       int32_t pr, int32_t dil, SeriesGeom* g) {
  if (rule == kSeriesDilated && (dil == 1 || (H == 1 && dil > 1 && stride == 1))) { rule = kSeriesConv; dil = 1; }
  int32_t He = H;
  if (rule == kSeriesPlain) {
    if (!series_shape_ok(S, n, T, f, H, N, K)) return TGCN_ERR_INVALID;
  } else if (rule == kSeriesConv) {
    if (!series_conv_shape_ok(S, n, T, f, H, N, K, stride, pl, pr)) return TGCN_ERR_INVALID;
    stride = series_conv_stride(T, stride, pl, pr);
  } else if (int rc = series_dilated_check(S, n, T, f, H, N, K, stride, pl, pr, dil, &He)) {
    return rc;                                           // accepted: dil > 1 at step 1
  }
  *g = SeriesGeom{stride, pl, pr, dil, He, series_conv_nwin(T, He, stride, pl, pr)};
  return TGCN_OK;
}

// The chunk entries' geometry (DESIGN.md 3.10 "Streaming state"): one chunk of Tc time rows, the C = (H - 1) * dilation rows before it in a
// ring.  TGCN_OK and *C_out, or TGCN_ERR_INVALID.  The chunk behind C zero rows is a geometry of the _dilated entries (Tp = Tc + C >= He,
// pad_left = C = He - 1), so their rules bound every number the kernels form.  One tap keeps no ring (C = 0; ring_ld and head unused) and is
// admitted only where the entry says so (one_tap).
static int series_stream_check(int64_t S, int64_t n, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K, int32_t dil, int64_t ring_ld,
                               int32_t head, int32_t* C_out, bool one_tap = false) {
  if (dil < 1 || Tc < 1 || H < (one_tap ? 1 : 2)) return TGCN_ERR_INVALID;
  if (H == 1) { *C_out = 0; return series_conv_shape_ok(S, n, Tc, f, 1, N, K, 1, 0, 0) ? TGCN_OK : TGCN_ERR_INVALID; }
  const int64_t C = ((int64_t)H - 1) * dil;
  if (C >= (int64_t)INT32_MAX / 64) return TGCN_ERR_INVALID;
  int32_t He = 0;
  if (dil > 1 ? series_dilated_check(S, n, Tc, f, H, N, K, 1, (int32_t)C, 0, dil, &He) != TGCN_OK
              : !series_conv_shape_ok(S, n, Tc, f, H, N, K, 1, (int32_t)C, 0)) return TGCN_ERR_INVALID;
  if (head < 0 || head >= C || ring_ld < C * f || ring_ld >= (int64_t)INT32_MAX) return TGCN_ERR_INVALID;
  *C_out = (int32_t)C;
  return TGCN_OK;
}

// A chunk's rows inside an output of out_T time rows (the _at entry): rows [out_t0, out_t0 + Tc) of (S, n, out_T, N) or (S*out_T, n, N)
static bool series_out_slice_ok(int32_t Tc, int32_t out_T, int32_t out_t0) {
  return out_T >= 1 && out_t0 >= 0 && (int64_t)out_t0 + Tc <= (int64_t)out_T;
}
static bool series_stack_ld_ok(int32_t T, int32_t f, int64_t stack_ld) { return stack_ld >= (int64_t)T * f && stack_ld < (int64_t)INT32_MAX; }

static int series_bias_check(const void* bias, int32_t bias_kind, int32_t bias_dtype, const char* who) {
  if (bias_kind < 0 || bias_kind > 2 || (bias_kind && !bias)) TGCN_FAIL(TGCN_ERR_INVALID, "%s: bias_kind %d", who, bias_kind);
  if (bias_dtype != TGCN_DTYPE_F32 && bias_dtype != TGCN_DTYPE_BF16) TGCN_FAIL(TGCN_ERR_INVALID, "%s: dtype code %d", who, bias_dtype);
  return TGCN_OK;
}

// What every driver ends with: the entry's name is "tgcn_cheb_" + who + the trait's suffix
static int series_launched(const char* who, const char* suffix) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) TGCN_FAIL(TGCN_ERR_LAUNCH, "tgcn_cheb_%s%s: %s", who, suffix, hipGetErrorString(e));
  return TGCN_OK;
}

// ---- one parameter builder: the fillers of SeriesGemmParams / SeriesGemmBf16Params (the same field names on purpose).  A field no filler
// names stays zero, which is what its "X only" comment in windows.h asks of a launch without X.
// The strides of rows of N values per (recording, vertex, time row): as a series (S, n, rows, N), else (S, rows, n, N)
static void series_layout(int64_t n, int64_t rows, int32_t N, int32_t as_series, int64_t* ss, int64_t* is, int64_t* ws) {
  if (as_series) { *ss = n * rows * N; *is = rows * N; *ws = N; }
  else { *ss = rows * n * N; *is = N; *ws = n * N; }
}
template <class P>
static P series_params(int64_t n, int32_t Tin, int32_t padl, int64_t nwin, int32_t H, int32_t f, int32_t N, int32_t nterms) {
  P p;
  memset(&p, 0, sizeof(p));
  p.n = n; p.Tin = Tin; p.padl = padl; p.nwin = (int32_t)nwin; p.H = H; p.f = f; p.N = N; p.nterms = nterms;
  return p;
}
// the hop stack (K, S, n, ld) with f channels per time row
template <class P, class E>
static void series_src_stack(P& p, const E* stack, int64_t S, int64_t n, int64_t ld, int32_t f) {
  p.src = stack; p.src_ks = S * n * ld; p.src_ss = n * ld; p.src_is = ld; p.src_ts = f;
}
// out: rows [t0, t0 + nwin) of n_out vertices x rows time rows x N columns, in either layout
template <class P, class E>
static void series_out(P& p, E* out, int64_t n_out, int64_t rows, int32_t N, int32_t as_series, int32_t t0 = 0) {
  series_layout(n_out, rows, N, as_series, &p.o_ss, &p.o_is, &p.o_ws);
  p.o_gs = 0; p.ocg = N;
  p.out = out + (int64_t)t0 * p.o_ws;
}
// the ring (nterms, S, n, ring_ld) of the C rows before the chunk
template <class P, class E>
static void series_ring(P& p, const E* ring, int64_t S, int64_t n, int64_t ring_ld, int32_t C, int32_t head, const int64_t* pos, int32_t win_off) {
  p.ring = ring; p.ring_ks = S * n * ring_ld; p.ring_ss = n * ring_ld; p.ring_is = ring_ld; p.C = C; p.head = head; p.pos = pos; p.win_off = win_off;
}
// the input gradient: g as a series of N channels (strides g_ss, g_is, g_ws), one term, no bias, columns (k, c) into (K, S, n, Tf); the
// caller adds W, out and its window step o_ws, and the windows (padl, nwin, H)
template <class P, class E>
static P series_over_g(const E* g, int64_t g_ss, int64_t g_is, int64_t g_ws, int32_t g_rows, int64_t S, int64_t n, int64_t Tf, int32_t f, int32_t N, int32_t K) {
  P p = series_params<P>(n, g_rows, 0, 0, 0, N, K * f, 1);
  p.src = g; p.src_ks = 0; p.src_ss = g_ss; p.src_is = g_is; p.src_ts = g_ws;
  p.o_ss = n * Tf; p.o_is = Tf; p.o_gs = S * n * Tf; p.ocg = f;
  return p;
}
// 16-byte staging and copies: whole units per time row and per row, an aligned base -- the stack's rule, and a ring that keeps it
template <class X>
static bool series_vec(int32_t f, const void* stack, int64_t ld, const void* ring = nullptr, int64_t ring_ld = 0) {
  return f % X::kUnit == 0 && ld % X::kUnit == 0 && ((uintptr_t)stack & 15) == 0 && ring_ld % X::kUnit == 0 && ((uintptr_t)ring & 15) == 0;
}

// ---- driver 1, a whole series: the _series, _conv, _dilated and _pool entries of both element types.  stack_ld: elements between vertex
// rows (fp32: T * f).  pool 0: none (the _pool entry has checked its own).  drop (fp32, with pool; the _pool_dropout entry has checked it):
// dropout between relu and the pool.
template <class X>
static int series_forward(const char* who, void* stream, SeriesRule rule, int64_t S, int64_t n, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                          const void* stack, int64_t stack_ld, const void* W, const void* bias, int32_t bias_dtype, int32_t bias_kind,
                          int32_t as_series, void* out, uint8_t* idx, int32_t pool, int32_t stride, int32_t pl, int32_t pr, int32_t dil,
                          const DropoutParams* drop = nullptr) {
  typedef typename X::Elem E;
  SeriesGeom ge;
  const int grc = series_geom(rule, S, n, T, f, H, N, K, stride, pl, pr, dil, &ge);
  if (grc == TGCN_ERR_UNSUPPORTED) TGCN_FAIL(grc, "%s: dilation %d with stride %d is not built", who, dil, stride);
  if (grc || !stack || !W || !out || !series_stack_ld_ok(T, f, stack_ld)) TGCN_FAIL(TGCN_ERR_INVALID, "%s: bad argument", who);
  if (int rc = series_bias_check(bias, bias_kind, bias_dtype, who)) return rc;
  if (int drc = check_pointer_device(out, (hipStream_t)stream, who)) return drc;
  typename X::Params p = series_params<typename X::Params>(n, T, ge.pl, ge.nwin, H, f, N, K);
  series_src_stack(p, (const E*)stack, S, n, stack_ld, f);
  p.W = (const E*)W;
  X::set_bias(p, bias, bias_kind, bias_dtype);
  series_out(p, (E*)out, pool ? n / pool : n, ge.nwin, N, as_series);      // pooled: out and idx hold n / pool vertices
  if constexpr (std::is_same<E, float>::value) p.idx = idx;
  if (int rc = X::launch((hipStream_t)stream, p, S, series_vec<X>(f, stack, stack_ld), false, who, ge.stride, ge.dil, false, pool, drop)) return rc;
  return series_launched(who, X::kSuffix);
}

int tgcn_cheb_project_series_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                 const float* stack, const float* W, const float* bias, int32_t bias_kind, int32_t as_series, float* out) {
  return series_forward<SeriesF32>("project_series", stream, kSeriesPlain, S, n_vertices, T, f, H, N, K, stack, (int64_t)T * f, W, bias, TGCN_DTYPE_F32,
                                   bias_kind, as_series, out, nullptr, 0, 1, 0, 0, 1);
}

int tgcn_cheb_project_series_conv_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                      const float* stack, const float* W, const float* bias, int32_t bias_kind, int32_t as_series, float* out,
                                      int32_t stride, int32_t pad_left, int32_t pad_right) {
  return series_forward<SeriesF32>("project_series_conv", stream, kSeriesConv, S, n_vertices, T, f, H, N, K, stack, (int64_t)T * f, W, bias,
                                   TGCN_DTYPE_F32, bias_kind, as_series, out, nullptr, 0, stride, pad_left, pad_right, 1);
}

int tgcn_cheb_project_series_dilated_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                         const float* stack, const float* W, const float* bias, int32_t bias_kind, int32_t as_series, float* out,
                                         int32_t stride, int32_t pad_left, int32_t pad_right, int32_t dilation) {
  return series_forward<SeriesF32>("project_series_dilated", stream, kSeriesDilated, S, n_vertices, T, f, H, N, K, stack, (int64_t)T * f, W, bias,
                                   TGCN_DTYPE_F32, bias_kind, as_series, out, nullptr, 0, stride, pad_left, pad_right, dilation);
}

// relu + vertex max-pool as the projection's epilogue ("relu + pool epilogue"): the _dilated entry's geometry
int tgcn_cheb_project_series_pool_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                      const float* stack, const float* W, const float* bias, int32_t bias_kind, int32_t as_series, float* z,
                                      uint8_t* idx, int32_t pool, int32_t stride, int32_t pad_left, int32_t pad_right, int32_t dilation) {
  if (!series_pool_ok(n_vertices, pool)) TGCN_FAIL(TGCN_ERR_INVALID, "project_series_pool: pool %d of %lld vertices", pool, (long long)n_vertices);
  return series_forward<SeriesF32>("project_series_pool", stream, kSeriesDilated, S, n_vertices, T, f, H, N, K, stack, (int64_t)T * f, W, bias,
                                   TGCN_DTYPE_F32, bias_kind, as_series, z, idx, pool, stride, pad_left, pad_right, dilation);
}

// dropout between relu and the pool of the entry above ("dropout in the relu + pool epilogue"): the mask's own rules, then
// that entry's driver with its checks and codes; all of them before a pointer is read
int tgcn_cheb_project_series_pool_dropout_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                              const float* stack, const float* W, const float* bias, int32_t bias_kind, int32_t as_series, float* z,
                                              uint8_t* idx, int32_t pool, int32_t stride, int32_t pad_left, int32_t pad_right, int32_t dilation,
                                              const int64_t* seed, uint32_t thr, float scale) {
  if (!series_pool_ok(n_vertices, pool))
    TGCN_FAIL(TGCN_ERR_INVALID, "project_series_pool_dropout: pool %d of %lld vertices", pool, (long long)n_vertices);
  if (!seed || !dropout_scale_ok(scale)) TGCN_FAIL(TGCN_ERR_INVALID, "project_series_pool_dropout: a null seed or a scale that is not finite and >= 1");
  const DropoutParams drop{seed, thr, scale};
  return series_forward<SeriesF32>("project_series_pool_dropout", stream, kSeriesDilated, S, n_vertices, T, f, H, N, K, stack, (int64_t)T * f, W, bias,
                                   TGCN_DTYPE_F32, bias_kind, as_series, z, idx, pool, stride, pad_left, pad_right, dilation, &drop);
}

int tgcn_cheb_project_series_conv_bf16(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                       const void* stack, int64_t stack_ld, const void* W, const void* bias, int32_t bias_dtype,
                                       int32_t bias_kind, int32_t as_series, void* out, int32_t stride, int32_t pad_left, int32_t pad_right) {
  return series_forward<SeriesBf16>("project_series_conv_bf16", stream, kSeriesConv, S, n_vertices, T, f, H, N, K, stack, stack_ld, W, bias, bias_dtype,
                                    bias_kind, as_series, out, nullptr, 0, stride, pad_left, pad_right, 1);
}

int tgcn_cheb_project_series_dilated_bf16(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                          const void* stack, int64_t stack_ld, const void* W, const void* bias, int32_t bias_dtype,
                                          int32_t bias_kind, int32_t as_series, void* out, int32_t stride, int32_t pad_left, int32_t pad_right,
                                          int32_t dilation) {
  return series_forward<SeriesBf16>("project_series_dilated_bf16", stream, kSeriesDilated, S, n_vertices, T, f, H, N, K, stack, stack_ld, W, bias,
                                    bias_dtype, bias_kind, as_series, out, nullptr, 0, stride, pad_left, pad_right, dilation);
}

// ---- streaming state ("Streaming state")
// The ring update launch: rows = K * S * n rows of the stack (ld elements apart) and of the ring; esize: bytes per element (4 / 2);
// vec: 16-byte accesses (4 floats / 8 bf16 per unit), else one element; pos non-null: head is read on the device (the _pos entries)
static void series_ring_update_launch(hipStream_t st, const void* stack, void* ring, int64_t rows, int64_t stack_ld, int64_t ring_ld, int32_t f,
                                      int esize, bool vec, int32_t Tc, int32_t C, int32_t head, const int64_t* pos) {
  const int unit = vec ? 16 / esize : 1, m = Tc < C ? Tc : C, fu = f / unit;
  const dim3 grid(grid_1d(rows * m * fu));
  ProfScope ps(TGCN_PROF_RELAYOUT, st);
  const auto run = [&](auto u) {      // u: the unit of one access
    typedef decltype(u) U;
    launch_kernel(series_ring_update_kernel<U>, grid, dim3(kBlock), 0, st, (const U*)stack, (U*)ring, rows, stack_ld / unit, ring_ld / unit, fu,
                  Tc - m, m, C, head, pos);
  };
  if (vec) run(uint4());
  else if (esize == 4) run(uint32_t());
  else run(uint16_t());
}

// The position of a ring kept in device memory (the _pos entries) moves behind the ring update, in a launch of its own
static void series_stream_advance_launch(hipStream_t st, int64_t* pos, int32_t Tc, int32_t C) {
  ProfScope ps(TGCN_PROF_RELAYOUT, st);
  hipLaunchKernelGGL(series_stream_advance_kernel, dim3(1), dim3(1), 0, st, pos, Tc, C);
}

int tgcn_series_stream_advance(void* stream, int64_t* pos, int32_t Tc, int32_t C) {
  if (!pos || Tc < 1 || C < 0) TGCN_FAIL(TGCN_ERR_INVALID, "series_stream_advance: bad argument");
  series_stream_advance_launch((hipStream_t)stream, pos, Tc, C);
  TGCN_CHECK_LAUNCH("tgcn_series_stream_advance");
  return TGCN_OK;
}

// What tells the chunk entries apart.  The defaults are the _stream entry: every row of the chunk ends a window, written chunk-shaped.
struct SeriesChunkAsk {
  int32_t dil = 1, pool = 0;
  bool sliced = false;           // the _at entry (DESIGN.md 3.10 "Time chunks"): rows [out_t0, out_t0 + Tc) of an output of out_T time rows
  int32_t out_T = 0, out_t0 = 0, out_as_series = 1;
  bool one_tap = false;          // H == 1 admitted: no ring (null allowed), nothing to update
  bool stepped = false;          // the _stream_strided entries (DESIGN.md 3.10 "Window step"): windows end at chunk rows win_off + r * stride;
  int32_t stride = 1, win_off = 0;     // a chunk may end no window (out null allowed), and the position advances all the same
  uint8_t* idx = nullptr;        // the _stream_pool_at entry: sliced and pooled -- arg-max bytes in z's layout (null: not stored) and the
  const DropoutParams* drop = nullptr;       // optional mask, counted at window out_t0 + w of out_T (series_gemm_chunk_pool_dropout_kernel)
};

// ---- driver 2, a chunk of Tc time rows behind the ring of the C rows before it: the _stream, _pos, _stream_pool, _at and _stream_strided
// entries.  pos null: the host's head; non-null: head is read on the device (the head argument is unused) and the advance is the last
// launch.  Launches: the CARRY GEMM over the m windows that end inside the chunk (STRIDED && CARRY at a step >= 2; without a ring, H == 1,
// the plain forms on the chunk from row win_off on), the ring update, the advance.  At step 1 that is the _stream entry's sequence.
template <class X>
static int series_chunk_forward(const char* who, void* stream, int64_t S, int64_t n, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                const void* stack, int64_t stack_ld, const void* W, const void* bias, int32_t bias_dtype, int32_t bias_kind,
                                void* out, void* ring, int64_t ring_ld, int32_t head, int64_t* pos, const SeriesChunkAsk& ask) {
  typedef typename X::Elem E;
  hipStream_t st = (hipStream_t)stream;
  const int32_t stride = ask.stride, win_off = ask.win_off;
  int32_t C = 0;
  if (stride < 1 || win_off < 0 || win_off >= stride || series_stream_check(S, n, Tc, f, H, N, K, ask.dil, ring_ld, pos ? 0 : head, &C, ask.one_tap))
    TGCN_FAIL(TGCN_ERR_INVALID, "%s: bad argument", who);
  const bool carry = C > 0;
  const int32_t dil = carry ? ask.dil : 1;            // one tap has nothing to dilate: no dilation without a bound reaches a kernel
  const bool own_step = ask.stepped && !(stride == 1 && carry);      // the _stream_strided entries past the _stream entry's own sequence
  if (pos && !own_step) head = 0;                     // unused with a device position; the _stream_strided entries pass the caller's on
  const int32_t m = win_off < Tc ? (Tc - win_off - 1) / stride + 1 : 0;       // windows that end inside the chunk
  // the step the kernel runs at, clamped like the _conv entries' (a step above the padded chunk leaves one window)
  const int32_t sc = series_conv_stride(Tc, stride, C, 0);
  if (!stack || !W || (m > 0 && !out) || (carry && !ring) || !series_stack_ld_ok(Tc, f, stack_ld) ||
      (ask.sliced && !series_out_slice_ok(Tc, ask.out_T, ask.out_t0)))
    TGCN_FAIL(TGCN_ERR_INVALID, "%s: bad argument", who);
  if (int rc = series_bias_check(bias, bias_kind, bias_dtype, who)) return rc;
  const bool vec = carry ? series_vec<X>(f, stack, stack_ld, ring, ring_ld) : series_vec<X>(f, stack, stack_ld);
  if (own_step) {       // a chunk that ends no window still moves the ring: the plan's refusal comes first
    int hc = 0;
    if (!X::lds(H, f, series_gemm_nt(N), vec, sc, &hc)) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "%s: %d channels per time row do not fit the LDS span", who, f);
  }
  if (m > 0) {
    if (int drc = check_pointer_device(out, st, who)) return drc;
    typename X::Params p = series_params<typename X::Params>(n, Tc, C, m, H, f, N, K);
    series_src_stack(p, (const E*)stack, S, n, stack_ld, f);
    p.W = (const E*)W;
    X::set_bias(p, bias, bias_kind, bias_dtype);
    if (ask.sliced) series_out(p, (E*)out, ask.pool ? n / ask.pool : n, ask.out_T, N, ask.out_as_series, ask.out_t0);
    else series_out(p, (E*)out, ask.pool ? n / ask.pool : n, m, N, 1);      // (S, n, m, N); pooled: n / pool
    if (carry) series_ring(p, (const E*)ring, S, n, ring_ld, C, head, pos, win_off);
    else { p.src += (int64_t)win_off * f; p.Tin = Tc - win_off; }           // one tap reads no row before the chunk
    const SeriesDropAt at{ask.out_t0, ask.out_T};
    if constexpr (std::is_same<E, float>::value)
      if (ask.idx) p.idx = ask.idx + (int64_t)ask.out_t0 * p.o_ws;          // the same rows of the same layout
    if (int rc = X::launch(st, p, S, vec, false, who, sc, dil, carry, ask.pool, ask.drop, ask.drop ? &at : nullptr)) return rc;
  }
  if (carry) series_ring_update_launch(st, stack, ring, K * S * n, stack_ld, ring_ld, f, (int)sizeof(E), vec, Tc, C, head, pos);
  if (pos) series_stream_advance_launch(st, pos, Tc, C);
  return series_launched(who, X::kSuffix);
}

int tgcn_cheb_project_series_stream_f32(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                        const float* stack, const float* W, const float* bias, int32_t bias_kind, float* out, float* ring,
                                        int64_t ring_ld, int32_t head, int32_t dilation) {
  SeriesChunkAsk ask;
  ask.dil = dilation;
  return series_chunk_forward<SeriesF32>("project_series_stream", stream, S, n_vertices, Tc, f, H, N, K, stack, (int64_t)Tc * f, W, bias, TGCN_DTYPE_F32,
                                         bias_kind, out, ring, ring_ld, head, nullptr, ask);
}

int tgcn_cheb_project_series_stream_pos_f32(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                            const float* stack, const float* W, const float* bias, int32_t bias_kind, float* out, float* ring,
                                            int64_t ring_ld, int64_t* pos, int32_t dilation) {
  if (!pos) TGCN_FAIL(TGCN_ERR_INVALID, "project_series_stream_pos: bad argument");
  SeriesChunkAsk ask;
  ask.dil = dilation;
  return series_chunk_forward<SeriesF32>("project_series_stream_pos", stream, S, n_vertices, Tc, f, H, N, K, stack, (int64_t)Tc * f, W, bias,
                                         TGCN_DTYPE_F32, bias_kind, out, ring, ring_ld, 0, pos, ask);
}

// The stream entries' step with the pooled epilogue: z (S, n/pool, Tc, N).  H == 1 keeps no ring: the pooled entry on the chunk (ring, head
// and pos unused; the caller's advance counts seen).
int tgcn_cheb_project_series_stream_pool_f32(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                             const float* stack, const float* W, const float* bias, int32_t bias_kind, float* z, int32_t pool,
                                             float* ring, int64_t ring_ld, int32_t head, int64_t* pos, int32_t dilation) {
  const char* who = "project_series_stream_pool";
  if (!series_pool_ok(n_vertices, pool)) TGCN_FAIL(TGCN_ERR_INVALID, "%s: pool %d of %lld vertices", who, pool, (long long)n_vertices);
  if (H == 1) {
    if (dilation < 1) TGCN_FAIL(TGCN_ERR_INVALID, "%s: bad argument", who);
    return series_forward<SeriesF32>(who, stream, kSeriesConv, S, n_vertices, Tc, f, 1, N, K, stack, (int64_t)Tc * f, W, bias, TGCN_DTYPE_F32, bias_kind,
                                     1, z, nullptr, pool, 1, 0, 0, 1);
  }
  SeriesChunkAsk ask;
  ask.dil = dilation; ask.pool = pool;
  return series_chunk_forward<SeriesF32>(who, stream, S, n_vertices, Tc, f, H, N, K, stack, (int64_t)Tc * f, W, bias, TGCN_DTYPE_F32, bias_kind, z, ring,
                                         ring_ld, head, pos, ask);
}

// The _stream_pool entry's step (host head) into rows [out_t0, out_t0 + Tc) of a whole z of out_T time rows, in either layout, with the
// arg-max bytes and an optional mask ("Time chunks through the pooled epilogue").  seed null: the _stream_pool entry's own
// kernels, only the output's strides differ; else the chunk form of the dropout epilogue.  H == 1: no ring, the non-carry pooled forms.
int tgcn_cheb_project_series_stream_pool_at_f32(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                                const float* stack, const float* W, const float* bias, int32_t bias_kind, float* z, uint8_t* idx,
                                                int32_t pool, int32_t out_T, int32_t out_t0, int32_t out_as_series, float* ring, int64_t ring_ld,
                                                int32_t head, int32_t dilation, const int64_t* seed, uint32_t thr, float scale) {
  const char* who = "project_series_stream_pool_at";
  if (!series_pool_ok(n_vertices, pool)) TGCN_FAIL(TGCN_ERR_INVALID, "%s: pool %d of %lld vertices", who, pool, (long long)n_vertices);
  if (seed && !dropout_scale_ok(scale)) TGCN_FAIL(TGCN_ERR_INVALID, "%s: a scale that is not finite and >= 1", who);
  const DropoutParams drop{seed, thr, scale};
  SeriesChunkAsk ask;
  ask.dil = dilation; ask.pool = pool; ask.one_tap = true; ask.sliced = true; ask.out_T = out_T; ask.out_t0 = out_t0; ask.out_as_series = out_as_series;
  ask.idx = idx; ask.drop = seed ? &drop : nullptr;
  return series_chunk_forward<SeriesF32>(who, stream, S, n_vertices, Tc, f, H, N, K, stack, (int64_t)Tc * f, W, bias, TGCN_DTYPE_F32, bias_kind, z, ring,
                                         ring_ld, head, nullptr, ask);
}

int tgcn_cheb_project_series_stream_at_f32(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                           const float* stack, const float* W, const float* bias, int32_t bias_kind, float* out, int32_t out_T,
                                           int32_t out_t0, int32_t out_as_series, float* ring, int64_t ring_ld, int32_t head, int32_t dilation) {
  SeriesChunkAsk ask;
  ask.dil = dilation; ask.one_tap = true; ask.sliced = true; ask.out_T = out_T; ask.out_t0 = out_t0; ask.out_as_series = out_as_series;
  return series_chunk_forward<SeriesF32>("project_series_stream_at", stream, S, n_vertices, Tc, f, H, N, K, stack, (int64_t)Tc * f, W, bias,
                                         TGCN_DTYPE_F32, bias_kind, out, ring, ring_ld, head, nullptr, ask);
}

int tgcn_cheb_project_series_stream_strided_f32(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                                const float* stack, const float* W, const float* bias, int32_t bias_kind, float* out, float* ring,
                                                int64_t ring_ld, int32_t head, int64_t* pos, int32_t stride, int32_t win_off) {
  SeriesChunkAsk ask;
  ask.one_tap = true; ask.stepped = true; ask.stride = stride; ask.win_off = win_off;
  return series_chunk_forward<SeriesF32>("project_series_stream_strided", stream, S, n_vertices, Tc, f, H, N, K, stack, (int64_t)Tc * f, W, bias,
                                         TGCN_DTYPE_F32, bias_kind, out, ring, ring_ld, head, pos, ask);
}

int tgcn_cheb_project_series_stream_bf16(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                         const void* stack, int64_t stack_ld, const void* W, const void* bias, int32_t bias_dtype,
                                         int32_t bias_kind, void* out, void* ring, int64_t ring_ld, int32_t head, int32_t dilation) {
  SeriesChunkAsk ask;
  ask.dil = dilation;
  return series_chunk_forward<SeriesBf16>("project_series_stream_bf16", stream, S, n_vertices, Tc, f, H, N, K, stack, stack_ld, W, bias, bias_dtype,
                                          bias_kind, out, ring, ring_ld, head, nullptr, ask);
}

int tgcn_cheb_project_series_stream_pos_bf16(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                             const void* stack, int64_t stack_ld, const void* W, const void* bias, int32_t bias_dtype,
                                             int32_t bias_kind, void* out, void* ring, int64_t ring_ld, int64_t* pos, int32_t dilation) {
  if (!pos) TGCN_FAIL(TGCN_ERR_INVALID, "project_series_stream_pos_bf16: bad argument");
  SeriesChunkAsk ask;
  ask.dil = dilation;
  return series_chunk_forward<SeriesBf16>("project_series_stream_pos_bf16", stream, S, n_vertices, Tc, f, H, N, K, stack, stack_ld, W, bias, bias_dtype,
                                          bias_kind, out, ring, ring_ld, 0, pos, ask);
}

int tgcn_cheb_project_series_stream_strided_bf16(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                                 const void* stack, int64_t stack_ld, const void* W, const void* bias, int32_t bias_dtype,
                                                 int32_t bias_kind, void* out, void* ring, int64_t ring_ld, int32_t head, int64_t* pos,
                                                 int32_t stride, int32_t win_off) {
  SeriesChunkAsk ask;
  ask.one_tap = true; ask.stepped = true; ask.stride = stride; ask.win_off = win_off;
  return series_chunk_forward<SeriesBf16>("project_series_stream_strided_bf16", stream, S, n_vertices, Tc, f, H, N, K, stack, stack_ld, W, bias,
                                          bias_dtype, bias_kind, out, ring, ring_ld, head, pos, ask);
}

// ---- one launch per step (stream_small.h): the hops, the stream entry's projection and its ring update out of LDS
int tgcn_cheb_stream_small_plan(int64_t n, int64_t nnz, int32_t mode, int32_t f, int32_t H, int32_t N, int32_t K, int32_t Tc, int32_t dilation,
                                int32_t* tb, int32_t* dense, int32_t* lds_bytes) {
  if (f < 1 || H < 1 || N < 1 || K < 1 || Tc < 1 || dilation < 1 || (mode != 0 && mode != 1) || !tb || !dense || !lds_bytes)
    TGCN_FAIL(TGCN_ERR_INVALID, "stream_small_plan: bad argument");
  StreamSmallPlan pl;
  if (!stream_small_plan(n, nnz, mode, f, N, Tc, &pl))
    TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "stream_small_plan: n=%lld nnz=%lld f=%d N=%d does not fit one workgroup", (long long)n, (long long)nnz, f, N);
  *tb = pl.tb; *dense = pl.dense; *lds_bytes = pl.lds;
  return TGCN_OK;
}

int tgcn_cheb_stream_small_f32(void* stream, const tgcn_csr* A, int32_t mode, int64_t S, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                               const float* chunk, const float* W, const float* bias, int32_t bias_kind, float* out, float* ring,
                               int64_t ring_ld, int32_t head, const int64_t* pos, int32_t dilation) {
  int32_t C = 0;
  if (!A || !chunk || !W || !out || !ring || (mode != 0 && mode != 1) ||
      series_stream_check(S, A->n, Tc, f, H, N, K, dilation, ring_ld, pos ? 0 : head, &C))
    TGCN_FAIL(TGCN_ERR_INVALID, "stream_small: bad argument");
  if (bias_kind < 0 || bias_kind > 2 || (bias_kind && !bias)) TGCN_FAIL(TGCN_ERR_INVALID, "stream_small: bias_kind %d", bias_kind);
  StreamSmallPlan pl;
  if (!stream_small_plan(A->n, A->nnz, mode, f, N, Tc, &pl))
    TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "stream_small: n=%lld nnz=%lld f=%d N=%d does not fit one workgroup", (long long)A->n, (long long)A->nnz, f, N);
  // the kernel's 32-bit offsets: one recording's rows of the chunk, of the output and of one term of the ring; the whole weight
  const int64_t lim = (int64_t)INT32_MAX;
  if (S > lim || A->n * Tc * f > lim || A->n * Tc * N > lim || A->n * ring_ld > lim || (int64_t)K * H * f * N > lim)
    TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "stream_small: a recording's rows or the weight exceed 32-bit offsets");
  if (!A->rowptr || !A->edges) TGCN_FAIL(TGCN_ERR_INVALID, "stream_small: bad argument");
  if (int drc = check_pointer_device(out, (hipStream_t)stream, "stream_small")) return drc;
  StreamSmallParams p;
  memset(&p, 0, sizeof(p));
  p.rowptr = A->rowptr; p.ev = A->edges; p.chunk = chunk; p.W = W; p.bias = bias; p.out = out; p.ring = ring; p.pos = pos;
  p.S = (int32_t)S; p.ring_ld = (int32_t)ring_ld;
  p.n = (int32_t)A->n; p.nnz = (int32_t)A->nnz; p.Tc = Tc; p.f = f; p.fp = (f + 3) / 4 * 4; p.H = H; p.N = N; p.K = K;
  p.bias_kind = bias_kind; p.TB = pl.tb; p.ld = pl.ld; p.C = C; p.head = head; p.dil = dilation;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)S), block((unsigned)pl.nthr);
  ProfScope ps(TGCN_PROF_PROJECT, st);
  with_one_of<4, 2, 1>(pl.ntw, [&](auto NTW) { with_one_of<0, 1>(mode, [&](auto MODE) { with_flags([&](auto DENSE) {
    launch_kernel(small_stream_kernel<DENSE, NTW, MODE>, grid, block, pl.lds, st, p);
  }, pl.dense != 0); }); });
  TGCN_CHECK_LAUNCH("tgcn_cheb_stream_small_f32");
  return TGCN_OK;
}

// ---- one launch per series (series_small.h): the hops and the window projection of a whole-series call out of LDS
int tgcn_cheb_series_small_plan(int64_t n, int64_t nnz, int32_t mode, int32_t f, int32_t H, int32_t N, int32_t K, int32_t T, int32_t left,
                                int32_t right, int32_t dilation, int32_t* tb, int32_t* dense, int32_t* lds_bytes) {
  if (!tb || !dense || !lds_bytes) TGCN_FAIL(TGCN_ERR_INVALID, "series_small_plan: bad argument");
  SeriesSmallPlan pl;
  const int rc = series_small_plan(n, nnz, mode, f, H, N, K, T, left, right, dilation, &pl);
  if (rc == TGCN_ERR_INVALID) TGCN_FAIL(rc, "series_small_plan: bad argument");
  if (rc) TGCN_FAIL(rc, "series_small_plan: n=%lld nnz=%lld f=%d H=%d N=%d does not fit one workgroup", (long long)n, (long long)nnz, f, H, N);
  *tb = pl.tb; *dense = pl.dense; *lds_bytes = pl.lds;
  return TGCN_OK;
}

// the checks and the kernel parameters the two one-launch entries share: the plan's codes, then the entry's own; nothing is launched here
static int series_small_setup(const char* who, void* stream, const tgcn_csr* A, int32_t mode, int64_t S, int32_t T, int32_t f, int32_t H, int32_t N,
                              int32_t K, const float* series, const float* W, const float* bias, int32_t bias_kind, int32_t as_series, float* out,
                              float* stack, int32_t left, int32_t right, int32_t dilation, bool pooled, int32_t pool, const int64_t* seed,
                              float scale, SeriesSmallPlan* pl, SeriesSmallParams* p) {
  if (!A || !series || !W || !out || S < 1) TGCN_FAIL(TGCN_ERR_INVALID, "%s: bad argument", who);
  if (bias_kind < 0 || bias_kind > 2 || (bias_kind && !bias)) TGCN_FAIL(TGCN_ERR_INVALID, "%s: bias_kind %d", who, bias_kind);
  const int prc = series_small_plan(A->n, A->nnz, mode, f, H, N, K, T, left, right, dilation, pl);
  if (prc == TGCN_ERR_INVALID) TGCN_FAIL(prc, "%s: bad argument", who);
  if (prc) TGCN_FAIL(prc, "%s: n=%lld nnz=%lld f=%d H=%d N=%d does not fit one workgroup", who, (long long)A->n, (long long)A->nnz, f, H, N);
  if (pooled) {           // the pooled entry's own: pool 2 or 4 dividing the graph, and the dropout's scale
    if ((pool != 2 && pool != 4) || A->n % pool) TGCN_FAIL(TGCN_ERR_INVALID, "%s: pool %d on %lld vertices (2 or 4, dividing n)", who, pool, (long long)A->n);
    if (seed && !dropout_scale_ok(scale)) TGCN_FAIL(TGCN_ERR_INVALID, "%s: a scale that is not finite and >= 1", who);
  }
  // the kernel's 32-bit offsets: one recording's rows of the series (and of a term of the stack) and of the output; the whole weight; the grid
  const int64_t lim = (int64_t)INT32_MAX;
  if (A->n * T * f > lim || A->n * pl->nwin * N > lim || (int64_t)K * H * f * N > lim || S * pl->ntiles > lim)
    TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "%s: a recording's rows, the weight or the grid exceed 32-bit offsets", who);
  if (!A->rowptr || !A->edges) TGCN_FAIL(TGCN_ERR_INVALID, "%s: bad argument", who);
  if (int drc = check_pointer_device(out, (hipStream_t)stream, who)) return drc;
  memset(p, 0, sizeof(*p));
  p->rowptr = A->rowptr; p->ev = A->edges; p->series = series; p->W = W; p->bias = bias; p->out = out; p->stack = stack;
  p->S = (int32_t)S; p->n = (int32_t)A->n; p->nnz = (int32_t)A->nnz; p->T = T; p->f = f; p->H = H; p->N = N; p->K = K; p->bias_kind = bias_kind;
  p->TB = pl->tb; p->ld = pl->ld; p->left = left; p->dil = dilation; p->nwin = pl->nwin; p->ntiles = pl->ntiles; p->as_series = as_series ? 1 : 0;
  return TGCN_OK;
}

int tgcn_cheb_series_small_f32(void* stream, const tgcn_csr* A, int32_t mode, int64_t S, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                               const float* series, const float* W, const float* bias, int32_t bias_kind, int32_t as_series, float* out,
                               float* stack, int32_t left, int32_t right, int32_t dilation) {
  SeriesSmallPlan pl;
  SeriesSmallParams p;
  if (int rc = series_small_setup("series_small", stream, A, mode, S, T, f, H, N, K, series, W, bias, bias_kind, as_series, out, stack, left, right,
                                  dilation, false, 0, nullptr, 1.f, &pl, &p))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nblk = S * pl.ntiles, part = (int64_t)UINT32_MAX / kSrMaxThreads;      // fewer than 2^32 threads per launch (kSeriesGridPart)
  const dim3 block((unsigned)pl.nthr);
  ProfScope ps(TGCN_PROF_PROJECT, st);
  with_one_of<4, 2, 1>(pl.ntw, [&](auto NTW) { with_one_of<0, 1>(mode, [&](auto MODE) { with_flags([&](auto DENSE) {
    launch_kernel_parts(small_series_kernel<DENSE, NTW, MODE>, nblk, part, 1, block, pl.lds, st, p);
  }, pl.dense != 0); }); });
  TGCN_CHECK_LAUNCH("tgcn_cheb_series_small_f32");
  return TGCN_OK;
}

// the one-launch layer with relu (+ dropout) + pool as its epilogue (series_small.h, small_series_pool_kernel): the same plan and grid
int tgcn_cheb_series_small_pool_f32(void* stream, const tgcn_csr* A, int32_t mode, int64_t S, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                    const float* series, const float* W, const float* bias, int32_t bias_kind, int32_t as_series, float* z,
                                    uint8_t* idx, int32_t pool, float* stack, int32_t left, int32_t right, int32_t dilation, const int64_t* seed,
                                    uint32_t thr, float scale) {
  SeriesSmallPlan pl;
  SeriesSmallParams p;
  if (int rc = series_small_setup("series_small_pool", stream, A, mode, S, T, f, H, N, K, series, W, bias, bias_kind, as_series, z, stack, left,
                                  right, dilation, true, pool, seed, scale, &pl, &p))
    return rc;
  SeriesSmallPoolParams pp;
  memset(&pp, 0, sizeof(pp));
  pp.idx = idx; pp.drop.seed = seed; pp.drop.thr = thr; pp.drop.scale = scale;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nblk = S * pl.ntiles, part = (int64_t)UINT32_MAX / kSrMaxThreads;      // fewer than 2^32 threads per launch, as above
  const dim3 block((unsigned)pl.nthr);
  ProfScope ps(TGCN_PROF_PROJECT, st);
  with_one_of<4, 2, 1>(pl.ntw, [&](auto NTW) { with_one_of<0, 1>(mode, [&](auto MODE) { with_one_of<4, 2>(pool, [&](auto POOL) {
    with_flags([&](auto DENSE, auto DROP) {
      launch_kernel_parts(small_series_pool_kernel<DENSE, NTW, MODE, POOL, DROP>, nblk, part, 1, block, pl.lds, st, p, pp);
    }, pl.dense != 0, seed != nullptr);
  }); }); });
  TGCN_CHECK_LAUNCH("tgcn_cheb_series_small_pool_f32");
  return TGCN_OK;
}

// ---- backward
// Row blocks of the series weight gradient: wgrad_rows_per_block's rule, with the partials held to 256 MB (each is a whole (K, H*f, N) weight)
static int64_t series_wgrad_rows_per_block(int64_t M, int64_t weight_floats) {
  int64_t rpb = wgrad_rows_per_block(M);
  int64_t most = ((int64_t)256 << 20) / (weight_floats * (int64_t)sizeof(float));
  if (most < 1) most = 1;
  if ((M + rpb - 1) / rpb > most) rpb = ((M + most - 1) / most + 15) / 16 * 16;
  return rpb;
}

// The workspace of every backward entry: the flipped weight (fp32 or bf16, in a slot of fp32 size) and the fp32 partials
static size_t series_backward_workspace(int64_t M, int64_t wf) {
  const int64_t rpb = series_wgrad_rows_per_block(M, wf);
  return align_up((size_t)wf * sizeof(float), 256) + (size_t)((M + rpb - 1) / rpb) * wf * sizeof(float);
}
static size_t series_backward_workspace_bytes(SeriesRule rule, int64_t S, int64_t n, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                              int32_t stride, int32_t pl, int32_t pr, int32_t dil) {
  SeriesGeom ge;
  if (series_geom(rule, S, n, T, f, H, N, K, stride, pl, pr, dil, &ge)) return 0;
  return series_backward_workspace(S * n * ge.nwin, (int64_t)K * H * f * N);
}

// The weight gradient's row blocks and grid: everything about its two launches that can refuse
struct SeriesWgradPlan { int64_t M, rpb, nblocks, jtiles, tgroups; };
static int series_wgrad_plan(int64_t S, int64_t n, int64_t nwin, int32_t f, int32_t H, int32_t N, int32_t K, const char* who, SeriesWgradPlan* o) {
  o->M = S * n * nwin;
  o->rpb = series_wgrad_rows_per_block(o->M, (int64_t)K * H * f * N);
  o->nblocks = (o->M + o->rpb - 1) / o->rpb;
  o->jtiles = ((int64_t)H * f + 15) / 16; o->tgroups = (K + kWgTerms - 1) / kWgTerms;
  if (o->rpb + nwin >= (int64_t)INT32_MAX || o->rpb / nwin + n >= (int64_t)INT32_MAX || o->nblocks > (int64_t)INT32_MAX || (N + 63) / 64 > 65535 ||
      o->jtiles * o->tgroups > 65535)
    TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "%s: weight gradient shape too large", who);
  return TGCN_OK;
}

// dW from the stack (K, S, n, ld) and g (rows of N at strides g_ss, g_is, g_ws; nwin windows per vertex): partials per row block into the
// workspace behind the flipped weight's slot, then the fold.  conv: a step or padding; ring non-null: the chunk's rows before it (carried).
template <class X>
static int series_wgrad_launch(hipStream_t st, const char* who, int64_t S, int64_t n, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                               const void* stack, int64_t ld, const void* g, int64_t g_ss, int64_t g_is, int64_t g_ws, int64_t nwin, float* dW,
                               void* workspace, int32_t stride, int32_t padl, int32_t dil, bool conv, bool carried = false, const void* ring = nullptr,
                               int64_t ring_ld = 0, int32_t C = 0, int32_t head = 0) {
  typedef typename X::Elem E;
  SeriesWgradPlan w;
  if (int rc = series_wgrad_plan(S, n, nwin, f, H, N, K, who, &w)) return rc;
  const int64_t wf = (int64_t)K * H * f * N;
  typename X::WgradParams q;
  memset(&q, 0, sizeof(q));
  q.stack = (const E*)stack; q.g = (const E*)g; q.partial = (float*)((char*)workspace + align_up((size_t)wf * sizeof(float), 256));
  q.st_ks = S * n * ld; X::wgrad_rows(q, ld); q.g_ss = g_ss; q.g_is = g_is; q.g_ws = g_ws;
  q.M = w.M; q.rows_per_block = w.rpb; q.n = n;
  q.f = f; q.nwin = (int32_t)nwin; q.J = H * f; q.N = N; q.K = K;
  q.stride = stride; q.padl = padl; q.T = T; q.dil = dil;
  if (carried) X::wgrad_ring(q, ring, S, n, ring_ld, C, head);
  { ProfScope ps(TGCN_PROF_WGRAD, st);
    X::wgrad(st, dim3((unsigned)w.nblocks, (unsigned)((N + 63) / 64), (unsigned)(w.jtiles * w.tgroups)), q, conv, dil > 1, carried && C > 0); }
  WgradParams r;
  memset(&r, 0, sizeof(r));
  r.partial = q.partial; r.dW = dW; r.Kc = q.J; r.N = N; r.nterms = K; r.nblocks = (int32_t)w.nblocks;
  { ProfScope ps(TGCN_PROF_WGRAD, st);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((wf + 63) / 64)), dim3(1024), 0, st, r); }
  return TGCN_OK;
}

// ---- driver 3, both gradients of a whole series, for a window step, zero padding and dilated taps: every _backward entry of both element
// types.  G and dW are fp32; stack_ld: elements between vertex rows (fp32: T * f).
template <class X>
static int series_backward(const char* who, void* stream, SeriesRule rule, int64_t S, int64_t n, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                           const void* stack, int64_t stack_ld, const void* g_, int32_t g_as_series, const void* W, float* G, float* dW,
                           void* workspace, size_t workspace_bytes, int32_t stride, int32_t pl, int32_t pr, int32_t dil) {
  typedef typename X::Elem E;
  typedef typename X::Params P;
  hipStream_t st = (hipStream_t)stream;
  const E* g = (const E*)g_;
  SeriesGeom ge;
  const int grc = series_geom(rule, S, n, T, f, H, N, K, stride, pl, pr, dil, &ge);
  if (grc == TGCN_ERR_UNSUPPORTED) TGCN_FAIL(grc, "%s: dilation %d with stride %d is not built", who, dil, stride);
  if (grc || !g) TGCN_FAIL(TGCN_ERR_INVALID, "%s: bad argument", who);
  if (int drc = check_pointer_device(g, st, who)) return drc;
  const int64_t Tf = (int64_t)T * f, nwin = ge.nwin, wf = (int64_t)K * H * f * N;
  const size_t need = series_backward_workspace(S * n * nwin, wf);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15)) TGCN_FAIL(TGCN_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, need);
  stride = ge.stride; dil = ge.dil;
  int64_t g_ss, g_is, g_ws;
  series_layout(n, nwin, N, g_as_series, &g_ss, &g_is, &g_ws);
  if (G) {      // the forward's kernel over g as a series of N channels, columns (k, c), fp32 out; per phase of the window step, each at step 1
    if (!W) TGCN_FAIL(TGCN_ERR_INVALID, "%s: the input gradient needs W", who);
    E* Wd = (E*)workspace;
    { ProfScope ps(TGCN_PROF_RELAYOUT, st);
      X::flip(st, (const E*)W, Wd, (int)K, (int)H, (int)f, (int)N, (int)stride); }
    // the time rows of the phases ph >= H (a step longer than the window) lie between the windows: exact zeros
    if (stride > H && hipMemsetAsync(G, 0, (size_t)K * S * n * Tf * sizeof(float), st) != hipSuccess) TGCN_FAIL(TGCN_ERR_LAUNCH, "%s: memset failed", who);
    // 16-byte loads of g's time rows: whole units of N make every stride of either layout a multiple of the unit.  The phases' weights start
    // at rows of N*K*f elements: any alignment, the weight tile is loaded element by element.
    const bool vec = (N % X::kUnit == 0) && (((uintptr_t)g & 15) == 0);
    const P over_g = series_over_g<P>(g, g_ss, g_is, g_ws, (int32_t)nwin, S, n, Tf, f, N, K);      // what every launch over g shares
    if (dil > 1) {
      // dilated taps (step 1): time row t sums g[t + pl - h * dil] W[h]^T -- "window" t of the DILATED kernel over g with the flipped weight,
      // reaching (H - 1) * dil - pl rows back; all T rows in one launch
      P p = over_g;
      p.W = Wd; p.out = G; p.o_ws = f;
      p.padl = (H - 1) * dil - pl; p.nwin = T; p.H = H;
      if (int rc = X::launch(st, p, S, vec, true, who, 1, dil, false, 0)) return rc;
    } else {
      for (int ph = 0; ph < stride && ph < H; ++ph) {
        // time rows t = u * stride + ph - pl, u0 <= u <= u1; row u sums g[u - m] W[ph + m * stride]^T over m < Hp: "window" u - u0 of the
        // Hp-row kernel reaching Hp - 1 - u0 rows back
        const int Hp = series_phase_rows(H, stride, ph);
        // (a recording shorter than the phase, T + pl <= ph, has no time row of it: what its windows send there falls into the right padding)
        if ((int64_t)T - 1 + pl - ph < 0) continue;
        const int64_t u0 = ph >= pl ? 0 : (pl - ph + stride - 1) / stride, u1 = ((int64_t)T - 1 + pl - ph) / stride;
        if (u1 < u0) continue;
        P p = over_g;
        p.W = Wd + (int64_t)series_phase_row0(H, stride, ph) * N * K * f;
        p.out = G + (u0 * stride + ph - pl) * f; p.o_ws = (int64_t)stride * f;
        p.padl = (int32_t)(Hp - 1 - u0); p.nwin = (int32_t)(u1 - u0 + 1); p.H = Hp;
        if (int rc = X::launch(st, p, S, vec, true, who, 1, 1, false, 0)) return rc;
      }
    }
  }
  if (dW) {
    if (!stack || !series_stack_ld_ok(T, f, stack_ld)) TGCN_FAIL(TGCN_ERR_INVALID, "%s: the weight gradient needs the hop tensors", who);
    if (int rc = series_wgrad_launch<X>(st, who, S, n, T, f, H, N, K, stack, stack_ld, g, g_ss, g_is, g_ws, nwin, dW, workspace, stride, pl, dil,
                                        stride != 1 || pl != 0 || pr != 0)) return rc;
  }
  return series_launched(who, X::kSuffix);
}

size_t tgcn_cheb_series_backward_workspace_bytes(int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K) {
  return series_backward_workspace_bytes(kSeriesPlain, S, n_vertices, T, f, H, N, K, 1, 0, 0, 1);
}
size_t tgcn_cheb_series_conv_backward_workspace_bytes(int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                                      int32_t stride, int32_t pad_left, int32_t pad_right) {
  return series_backward_workspace_bytes(kSeriesConv, S, n_vertices, T, f, H, N, K, stride, pad_left, pad_right, 1);
}
size_t tgcn_cheb_series_dilated_backward_workspace_bytes(int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                                         int32_t stride, int32_t pad_left, int32_t pad_right, int32_t dilation) {
  return series_backward_workspace_bytes(kSeriesDilated, S, n_vertices, T, f, H, N, K, stride, pad_left, pad_right, dilation);
}
// bf16: the flipped weight in the fp32 entries' slot and the fp32 partials -- the fp32 entries' size and 256 MB cap
size_t tgcn_cheb_series_conv_backward_bf16_workspace_bytes(int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                                           int32_t stride, int32_t pad_left, int32_t pad_right) {
  return series_backward_workspace_bytes(kSeriesConv, S, n_vertices, T, f, H, N, K, stride, pad_left, pad_right, 1);
}
size_t tgcn_cheb_series_dilated_backward_bf16_workspace_bytes(int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                                              int32_t stride, int32_t pad_left, int32_t pad_right, int32_t dilation) {
  return series_backward_workspace_bytes(kSeriesDilated, S, n_vertices, T, f, H, N, K, stride, pad_left, pad_right, dilation);
}

// (1, 0, 0) at dilation 1: no step, no pads
int tgcn_cheb_series_backward_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                  const float* stack, const float* g, int32_t g_as_series, const float* W, float* G, float* dW,
                                  void* workspace, size_t workspace_bytes) {
  return series_backward<SeriesF32>("series_backward", stream, kSeriesPlain, S, n_vertices, T, f, H, N, K, stack, (int64_t)T * f, g, g_as_series, W, G, dW,
                                    workspace, workspace_bytes, 1, 0, 0, 1);
}

int tgcn_cheb_series_conv_backward_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                       const float* stack, const float* g, int32_t g_as_series, const float* W, float* G, float* dW,
                                       void* workspace, size_t workspace_bytes, int32_t stride, int32_t pad_left, int32_t pad_right) {
  return series_backward<SeriesF32>("series_conv_backward", stream, kSeriesConv, S, n_vertices, T, f, H, N, K, stack, (int64_t)T * f, g, g_as_series, W, G,
                                    dW, workspace, workspace_bytes, stride, pad_left, pad_right, 1);
}

int tgcn_cheb_series_dilated_backward_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                          const float* stack, const float* g, int32_t g_as_series, const float* W, float* G, float* dW,
                                          void* workspace, size_t workspace_bytes, int32_t stride, int32_t pad_left, int32_t pad_right,
                                          int32_t dilation) {
  return series_backward<SeriesF32>("series_dilated_backward", stream, kSeriesDilated, S, n_vertices, T, f, H, N, K, stack, (int64_t)T * f, g, g_as_series,
                                    W, G, dW, workspace, workspace_bytes, stride, pad_left, pad_right, dilation);
}

int tgcn_cheb_series_conv_backward_bf16(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                        const void* stack, int64_t stack_ld, const void* g, int32_t g_as_series, const void* W, float* G,
                                        float* dW, void* workspace, size_t workspace_bytes, int32_t stride, int32_t pad_left, int32_t pad_right) {
  return series_backward<SeriesBf16>("series_conv_backward_bf16", stream, kSeriesConv, S, n_vertices, T, f, H, N, K, stack, stack_ld, g, g_as_series, W, G,
                                     dW, workspace, workspace_bytes, stride, pad_left, pad_right, 1);
}

int tgcn_cheb_series_dilated_backward_bf16(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                           const void* stack, int64_t stack_ld, const void* g, int32_t g_as_series, const void* W, float* G,
                                           float* dW, void* workspace, size_t workspace_bytes, int32_t stride, int32_t pad_left, int32_t pad_right,
                                           int32_t dilation) {
  return series_backward<SeriesBf16>("series_dilated_backward_bf16", stream, kSeriesDilated, S, n_vertices, T, f, H, N, K, stack, stack_ld, g, g_as_series,
                                     W, G, dW, workspace, workspace_bytes, stride, pad_left, pad_right, dilation);
}

// ---- time chunks of forward_series, backward (DESIGN.md 3.10 "Time chunks"): one chunk of Tc time rows of the causal layer's two gradients.
// What the entry and its workspace query check: the chunk entries' rules (H == 1: no ring, C = 0), the chunk's place in the whole gradient,
// and the input gradient's launch over g as a series of N channels (Tc + C rows of N floats inside 32 bits).
static int series_chunk_check(int64_t S, int64_t n, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K, int32_t dil, int64_t ring_ld,
                              int32_t head, int32_t g_T, int32_t g_t0, int32_t* C_out) {
  int32_t C = 0;
  if (series_stream_check(S, n, Tc, f, H, N, K, dil, ring_ld, head, &C, true) || !series_out_slice_ok(Tc, g_T, g_t0)) return TGCN_ERR_INVALID;
  if (((int64_t)Tc + C) * N >= (int64_t)INT32_MAX || ((int64_t)Tc + C) * 64 >= (int64_t)INT32_MAX) return TGCN_ERR_INVALID;
  *C_out = C;
  return TGCN_OK;
}

size_t tgcn_cheb_series_chunk_backward_workspace_bytes(int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                                       int32_t dilation) {
  int32_t C = 0;
  if (dilation < 1 || H < 1) return 0;
  if (series_chunk_check(S, n_vertices, Tc, f, H, N, K, H == 1 ? 1 : dilation, (int64_t)(H - 1) * dilation * f, 0, Tc, 0, &C)) return 0;
  return series_backward_workspace(S * n_vertices * Tc, (int64_t)K * H * f * N);
}

int tgcn_cheb_series_chunk_backward_f32(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                        const float* stack, float* ring, int64_t ring_ld, int32_t head, const float* g, int32_t g_T,
                                        int32_t g_t0, int32_t g_as_series, const float* W, float* G, float* dW, void* workspace,
                                        size_t workspace_bytes, int32_t dilation) {
  typedef SeriesF32 X;
  const char* who = "series_chunk_backward";
  if (H == 1 && dilation >= 1) dilation = 1;      // one tap has nothing to dilate
  int32_t C = 0;
  // the one-sided form without a weight gradient reads and moves no ring: ring null, and ring_ld and head are then unused
  const bool carried = ring != nullptr && H > 1;
  if (H < 1 || dilation < 1 ||
      series_chunk_check(S, n_vertices, Tc, f, H, N, K, dilation, carried ? ring_ld : (int64_t)(H - 1) * dilation * f, carried ? head : 0, g_T, g_t0,
                         &C) || !g || (!G && !dW))
    TGCN_FAIL(TGCN_ERR_INVALID, "%s: bad argument", who);
  if ((G && !W) || ((dW || carried) && !stack) || (dW && H > 1 && !ring)) TGCN_FAIL(TGCN_ERR_INVALID, "%s: bad argument", who);
  if (int drc = check_pointer_device(g, (hipStream_t)stream, who)) return drc;
  const size_t need = tgcn_cheb_series_chunk_backward_workspace_bytes(S, n_vertices, Tc, f, H, N, K, dilation);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15)) TGCN_FAIL(TGCN_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = n_vertices, Tf = (int64_t)Tc * f;
  int64_t g_ss, g_is, g_ws;      // the WHOLE gradient's strides; the chunk's rows start g_t0 rows in
  series_layout(n, g_T, N, g_as_series, &g_ss, &g_is, &g_ws);
  const float* gc = g + (int64_t)g_t0 * g_ws;
  // ---- everything that can refuse, before the first launch: the plans the two launchers will form again
  const bool vecg = (N % 4 == 0) && (((uintptr_t)gc & 15) == 0);
  SeriesLaunchPlan lp;
  SeriesWgradPlan wp;
  if (G) if (int rc = series_launch_plan(X::lds, S, n, Tc, H, N, K * f, vecg, 1, dilation, 0, who, &lp)) return rc;
  if (dW) if (int rc = series_wgrad_plan(S, n, Tc, f, H, N, K, who, &wp)) return rc;
  if (G) {      // rows [g_t0, g_t0 + Tc) of the whole input gradient: time row t sums g[t + h' * dil] Wd[h'] over the rows of g that exist
    float* Wd = (float*)workspace;
    { ProfScope ps(TGCN_PROF_RELAYOUT, st);
      X::flip(st, W, Wd, (int)K, (int)H, (int)f, (int)N, 1); }
    const int64_t left = (int64_t)g_T - g_t0;
    // columns (k, c) into the chunk-shaped (K, S, n, Tc*f)
    X::Params p = series_over_g<X::Params>(gc, g_ss, g_is, g_ws, (int32_t)(left < (int64_t)Tc + C ? left : (int64_t)Tc + C), S, n, Tf, f, N, K);
    p.W = Wd; p.out = G; p.o_ws = f;
    p.padl = 0; p.nwin = Tc; p.H = H;
    if (int rc = X::launch(st, p, S, vecg, true, who, 1, dilation, false, 0)) return rc;
  }
  // one tap (C == 0): the window is its own row, the plain form; else the window that ends at each chunk row, its early rows from the ring
  if (dW)
    if (int rc = series_wgrad_launch<X>(st, who, S, n, Tc, f, H, N, K, stack, Tf, gc, g_ss, g_is, g_ws, Tc, dW, workspace, 1, C, dilation, C > 0, true,
                                        ring, ring_ld, C, head)) return rc;
  if (carried)       // behind both on the same stream: the weight gradient has read the old ring
    series_ring_update_launch(st, stack, ring, K * S * n, Tf, ring_ld, f, 4, series_vec<X>(f, stack, Tf, ring, ring_ld), Tc, C, head, nullptr);
  return series_launched(who, X::kSuffix);
}

extern "C" {

int tgcn_fold_weight_f32(void* stream, int32_t K, int64_t CN, const float* fold, const float* W, float* out, int32_t transpose) {
  if (K < 1 || K > 4096 || CN < 1 || !fold || !W || !out || W == out) TGCN_FAIL(TGCN_ERR_INVALID, "fold_weight: bad argument");
  hipLaunchKernelGGL(fold_weight_kernel, dim3(grid_1d(CN)), dim3(kBlock), 0, (hipStream_t)stream, fold, W, out, (int)K, CN, (int)transpose);
  TGCN_CHECK_LAUNCH("tgcn_fold_weight_f32");
  return TGCN_OK;
}

int tgcn_weight_layout_f32(void* stream, int32_t K, int32_t C, int32_t N, const float* W, float* out, int32_t kind) {
  if (K < 1 || C < 1 || N < 1 || !W || !out || W == out || kind < 0 || kind > 2) TGCN_FAIL(TGCN_ERR_INVALID, "weight_layout: bad argument");
  hipLaunchKernelGGL(weight_layout_kernel, dim3(grid_1d((int64_t)K * C * N)), dim3(kBlock), 0, (hipStream_t)stream, W, out, (int)K, (int)C, (int)N, (int)kind);
  TGCN_CHECK_LAUNCH("tgcn_weight_layout_f32");
  return TGCN_OK;
}

int tgcn_csr_hop_f64(void* stream, int64_t n, const int32_t* rowptr, const int32_t* col, const double* val, int64_t F,
                     const double* X, const double* Z, double alpha, double beta, double* Y, double* P) {
  if (n <= 0 || F <= 0 || !rowptr || !X || (!Y && !P)) TGCN_FAIL(TGCN_ERR_INVALID, "hop_f64: bad argument");
  const int64_t gx = (F + 63) / 64, gy = (n + 3) / 4;
  if (gx > (int64_t)INT32_MAX || gy > 65535 * 1024LL) TGCN_FAIL(TGCN_ERR_UNSUPPORTED, "hop_f64: grid too large");
  for (int64_t y0 = 0; y0 < gy; y0 += 65535) {       // grid.y limit: slices of 65535 row tiles
    const int64_t ny = gy - y0 < 65535 ? gy - y0 : 65535;
    const int64_t r0 = y0 * 4, rows = (n - r0 < ny * 4) ? n - r0 : ny * 4;
    hipLaunchKernelGGL(hop_f64_kernel, dim3((unsigned)gx, (unsigned)ny), dim3(kBlock), 0, (hipStream_t)stream, rows, rowptr + r0, col, val, F, X,
                       Z ? Z + r0 * F : nullptr, alpha, beta, Y ? Y + r0 * F : nullptr, P ? P + r0 * F : nullptr);
  }
  TGCN_CHECK_LAUNCH("tgcn_csr_hop_f64");
  return TGCN_OK;
}

int tgcn_csr_sddmm_f32(void* stream, const tgcn_csr* A, int64_t n_cols, int32_t nb, int32_t C, const tgcn_dense* rows, const tgcn_dense* cols,
                       float alpha, float* dval, int32_t accumulate) {
  if (!A || !rows || !cols || !rows->ptr || !cols->ptr || !dval || nb < 1 || C < 1 || n_cols < 1 || !A->rowptr || (A->nnz > 0 && !A->edges))
    TGCN_FAIL(TGCN_ERR_INVALID, "sddmm: bad argument");
  if (A->nnz == 0) return TGCN_OK;
  const bool v4 = (C % 4 == 0) && aligned4(rows) && aligned4(cols);
  const unsigned grid = grid_1d(A->nnz * 16);
  if (v4) hipLaunchKernelGGL((sddmm_kernel<4>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, A->n, A->nnz, A->rowptr, A->edges, nb, C, rows->ptr,
                             rows->batch_stride, rows->row_stride, cols->ptr, cols->batch_stride, cols->row_stride, alpha, dval, (int)accumulate);
  else hipLaunchKernelGGL((sddmm_kernel<1>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, A->n, A->nnz, A->rowptr, A->edges, nb, C, rows->ptr,
                          rows->batch_stride, rows->row_stride, cols->ptr, cols->batch_stride, cols->row_stride, alpha, dval, (int)accumulate);
  TGCN_CHECK_LAUNCH("tgcn_csr_sddmm_f32");
  return TGCN_OK;
}

int tgcn_pack_rows_f32(void* stream, const float* src, int64_t ld_src, const int64_t* idx, int64_t nrows, int32_t C, float* out) {
  if (!src || !idx || !out || nrows < 0 || C <= 0 || ld_src < C) TGCN_FAIL(TGCN_ERR_INVALID, "pack_rows: bad argument");
  if (nrows == 0) return TGCN_OK;
  hipLaunchKernelGGL(pack_rows_kernel, dim3(grid_1d(nrows * C)), dim3(kBlock), 0, (hipStream_t)stream, src, idx, out, nrows, C, ld_src);
  TGCN_CHECK_LAUNCH("tgcn_pack_rows_f32");
  return TGCN_OK;
}

int tgcn_pack_rows_bf16(void* stream, const void* src, int64_t ld_src, const int64_t* idx, int64_t nrows, int32_t C, void* out) {
  if (!src || !idx || !out || nrows < 0 || C <= 0 || ld_src < C) TGCN_FAIL(TGCN_ERR_INVALID, "pack_rows_bf16: bad argument");
  if (nrows == 0) return TGCN_OK;
  hipStream_t st = (hipStream_t)stream;
  if (C % 8 == 0 && ld_src % 8 == 0 && (((uintptr_t)src | (uintptr_t)out) & 15) == 0)
    hipLaunchKernelGGL((pack_rows_2b_kernel<uint4>), dim3(grid_1d(nrows * (C / 8))), dim3(kBlock), 0, st, (const uint4*)src, idx, (uint4*)out, nrows, C / 8,
                       ld_src / 8);
  else
    hipLaunchKernelGGL((pack_rows_2b_kernel<uint16_t>), dim3(grid_1d(nrows * C)), dim3(kBlock), 0, st, (const uint16_t*)src, idx, (uint16_t*)out, nrows, C,
                       ld_src);
  TGCN_CHECK_LAUNCH("tgcn_pack_rows_bf16");
  return TGCN_OK;
}

int tgcn_pool_max_f32(void* stream, const float* x, float* out, int32_t* idx, int64_t q, int64_t n, int32_t f, int32_t p) {
  if (!x || !out || q <= 0 || n <= 0 || f <= 0 || p <= 0 || n % p != 0) TGCN_FAIL(TGCN_ERR_INVALID, "pool: bad argument (n=%lld p=%d)", (long long)n, p);
  const int64_t total = q * (n / p) * f;
  hipLaunchKernelGGL(pool_max_kernel, dim3(grid_1d(total)), dim3(kBlock), 0, (hipStream_t)stream, x, out, idx, total, (int)f, (int)p);
  TGCN_CHECK_LAUNCH("tgcn_pool_max_f32");
  return TGCN_OK;
}

int tgcn_pool_max_bwd_f32(void* stream, const float* grad_out, const int32_t* idx, float* grad_in, int64_t q, int64_t n, int32_t f, int32_t p) {
  if (!grad_out || !idx || !grad_in || q <= 0 || n <= 0 || f <= 0 || p <= 0 || n % p != 0) TGCN_FAIL(TGCN_ERR_INVALID, "pool_bwd: bad argument");
  const int64_t total = q * (n / p) * f;
  hipLaunchKernelGGL(pool_max_bwd_kernel, dim3(grid_1d(total)), dim3(kBlock), 0, (hipStream_t)stream, grad_out, idx, grad_in, total, (int)f, (int)p);
  TGCN_CHECK_LAUNCH("tgcn_pool_max_bwd_f32");
  return TGCN_OK;
}

}  // extern "C"
