// series_small.h -- a whole-series time-window layer on a graph that fits in LDS, in ONE launch (tgcn_cheb_series_small_f32)
// Part of the single translation unit tgcn_hip.hip (included once, inside its anonymous namespace, after stream_small.h).
#pragma once

// --------------------------------------------------------------------------------------------------
// small_series_kernel: hops, window projection and bias of a tile of windows, the operand resident in LDS
// --------------------------------------------------------------------------------------------------
// The general whole-series call is K - 1 hop launches with their fix-ups and the window projection: about twenty short
// dependent launches per layer.  A whole series hands no ring from one call to the next, so here workgroup (s, j) owns the output windows
// [j*TB, min((j+1)*TB, nwin)) of recording s -- all n vertices, all N columns -- and reads nothing another workgroup writes: it loads the
// span of R = TB + (H-1)*dil time rows its windows touch, from row j*TB - left on (rows outside [0, T) are zeros: padding only moves the time
// origin), and runs every hop on the whole span, halo included.  The grid is S * ntiles independent workgroups.
// A vertex row of the span is the R*f contiguous (t, c) floats of the recording's row, padded at its END to whole 16-byte quads (ld floats
// between rows; no per-time-row channel padding).  The operand is staged once per workgroup in small_stream_kernel's two forms (CSR entries +
// row pointers, or the dense n x (n|1) copy).  For term k = 0 .. K-1:
//   hop      thread = (vertex, 16-byte column quad), the thread groups beyond the first npad threads take further quads.  Term 0 is the span.
//            mode 0, P_k = L P_{k-1}, runs IN PLACE in one buffer: a pass of quads is summed into registers, a barrier, then written back (a
//            quad is read only in its own pass).  mode 1, T_k = 2 L T_{k-1} - T_{k-2} (the one-rounding fmaf(2, acc, -z) of
//            small_basis_kernel), keeps two buffers: T_k overwrites T_{k-2}, of which a thread reads only the element it then writes.
//            (One buffer fewer than small_stream_kernel in each mode: 784 vertices x a 28-row span x two buffers are above the LDS limit.)
//   project  out[s, i, w, :] += sum_h row_k(i, w - left + h*dil) . W[k, h*f + c, :] on v_mfma_f32_16x16x4_f32, small_stream_kernel's
//            carve-up: a wave owns a group of NTW tiles of 16 columns and every NV-th tile of 16 vertices for all TB windows of the tile;
//            its kSrAcc accumulators live through all K terms.  fp32 products and sums, terms ascending, (h, c) ascending within a term,
//            bias last.  No sum's order depends on TB or on the tile: a hop element sums its operand row in the row's order whatever the
//            column, and an output element takes its k steps in the same order at every accumulator slot.
//   stack    p.stack non-null: the term's rows this workgroup OWNS go to stack (K, S, n, T*f).  Tile j owns recording rows
//            [j*TB - left, (j+1)*TB - left), the last tile up to T: a partition of [0, T), every element written once from values computed
//            here; the halo rows behind the owned ones are computed and not stored.
// Then bias and the store of out, (S, n, nwin, N) or (S*nwin, n, N).
// Barriers: every thread of the workgroup reaches every barrier -- the pass count of a hop is uniform; threads beyond the n vertices and
// waves without an item only skip work.
// Index arithmetic: 32 bits inside the workgroup's LDS image, inside ONE recording's rows of the series, the stack and the output, and inside
// the weight -- the entry refuses n*T*f, n*nwin*N or K*H*f*N of 2^31 or more; the recording and the term enter in 64 bits.
constexpr int kSrAcc = 16;          // accumulator tiles (f32x4) per wave
constexpr int kSrMaxThreads = 1024;
constexpr int kSrLdsLimit = 160 * 1024;

struct SeriesSmallParams {
  const int32_t* rowptr;
  const tgcn_edge* ev;
  const float* series;    // (S, n, T*f), operand labels
  const float* W;         // (K, H*f, N), the kernels' working basis
  const float* bias;      // bias_kind 1: [N]; 2: [n][N]
  float* out;             // (S, n, nwin, N) or (S*nwin, n, N)
  float* stack;           // nullable: (K, S, n, T*f)
  int32_t S, n, nnz, T, f, H, N, K, bias_kind, TB, ld, left, dil, nwin, ntiles, as_series;
  int32_t blk0;           // the first workgroup of this part of the grid
};

template <bool DENSE, int NTW, int MODE>
__global__ __launch_bounds__(kSrMaxThreads) void small_series_kernel(const SeriesSmallParams p) {
#define TGCN_SERIES_SMALL_POOL 0
#include "series_small_body.inc"
#undef TGCN_SERIES_SMALL_POOL
}

// --------------------------------------------------------------------------------------------------
// small_series_pool_kernel: small_series_kernel with relu (+ dropout) and the max over POOL consecutive vertices as its epilogue
// --------------------------------------------------------------------------------------------------
// A kernel template of its own around the same body (series_small_body.inc), so that the kernels above keep their names and their code;
// it is small_series_kernel up to and including the last term's projection, the stack write included.  The accumulator fragment has D
// row = vertex vt*16 + (lane >> 4)*4 + i: the four floats of a lane's f32x4 are four consecutive vertices from a multiple of 4 on -- one
// gcn_pool_4 group (POOL 4) or two gcn_pool pairs (POOL 2).  So for each accumulator slot and column tile a lane computes, in registers,
//   t[i] = acc[i] + bias(v_i, col)                        (a bias of kind 2 differs per vertex)
//   DROP: t[i] = relu_dropout(t[i], dropout_keep(seed, e_i, thr), scale),  e_i = ((s*nwin + w)*n + v_i)*N + col in 64 bits (dropout.h)
//   the pool by relu_pool_kernel's rules: members ascending, the first maximum wins, a NaN wins over a number
//   z = best > 0 ? best : (best != best ? best : 0), and the arg-max byte where idx is non-null
// and the max needs no LDS scratch, no barrier and no other lane.  A group is stored iff its first vertex is < n (n % POOL == 0: the
// entry's check, so a group is whole or absent).  p.out is z -- (S, n/POOL, nwin, N) as a series, else (S*nwin, n/POOL, N) -- and idx has
// its layout.  DROP runs one Philox call per element (four per lane, slot and column tile) where N % 4 != 0.  N % 4 == 0: the four columns
// col & ~3 .. + 3 of one vertex share a call, the four lanes of a quad run one call each -- lane j vertex j's -- and exchange the words by
// windows.h's series_quad_bcast: one call per lane in place of four, the same bits.
struct SeriesSmallPoolParams {
  uint8_t* idx;           // nullable: the arg-max member of every pooled element, z's layout
  DropoutParams drop;     // DROP only
};

template <bool DENSE, int NTW, int MODE, int POOL, bool DROP>
__global__ __launch_bounds__(kSrMaxThreads) void small_series_pool_kernel(const SeriesSmallParams p, const SeriesSmallPoolParams pp) {
#define TGCN_SERIES_SMALL_POOL 1
#include "series_small_body.inc"
#undef TGCN_SERIES_SMALL_POOL
}

// The plan: TGCN_OK with threads, carve-up, floats per buffer row and the tile's windows; TGCN_ERR_INVALID for a bad value,
// TGCN_ERR_UNSUPPORTED where the shape does not fit.
//   ntw, threads   small_stream_kernel's rule: 4 / 2 / 1 column tiles per wave, one thread per vertex at least and a wave per
//                  (vertex tile, column group) where 1024 threads allow it
//   TB             the most windows (<= nwin) that the accumulators hold -- kSrAcc >= ntw * (vertex tiles per wave) * TB -- and whose span
//                  buffers (1 in mode 0, 2 in mode 1) fit the LDS next to the operand
//   ld             the span's (TB + (H-1)*dil) * f floats rounded up to whole quads, plus 4 where that makes ld / 4 even: the 16 vertices x 4 k
//                  of an A-fragment read fall into different banks
struct SeriesSmallPlan { int nthr, dense, tb, ld, lds, ntw, nwin, ntiles; };
inline int series_small_plan(int64_t n, int64_t nnz, int32_t mode, int32_t f, int32_t H, int32_t N, int32_t K, int32_t T, int32_t left, int32_t right,
                             int32_t dil, SeriesSmallPlan* out) {
  if (n < 1 || nnz < 0 || (mode != 0 && mode != 1) || f < 1 || H < 1 || N < 1 || K < 1 || T < 1 || dil < 1) return TGCN_ERR_INVALID;
  const int64_t halo = ((int64_t)H - 1) * dil;
  if (left < 0 || right < 0 || left > halo || right > halo || (int64_t)T + left + right < halo + 1) return TGCN_ERR_INVALID;
  if (halo >= (int64_t)INT32_MAX / 64 || ((int64_t)T + left + right) * f >= (int64_t)INT32_MAX) return TGCN_ERR_INVALID;
  if (n > (int64_t)kSmallMaxN || nnz > (1 << 20) || N > 1024 || (int64_t)f > kSrLdsLimit) return TGCN_ERR_UNSUPPORTED;
  const int64_t nwin = (int64_t)T + left + right - halo;
  const int nbuf = mode == 0 ? 1 : 2;
  const int ntv = (int)((n + 15) / 16), ntn = (N + 15) / 16;
  const int ntw = ntn >= 4 ? 4 : (ntn >= 2 ? 2 : 1), ng = (ntn + ntw - 1) / ntw;
  const int need = (int)((n + 63) / 64 * 64), want = 64 * (ntv * ng < kSrMaxThreads / 64 ? ntv * ng : kSrMaxThreads / 64);
  const int nthr = need > want ? need : want;
  const int nv = (nthr / 64) / ng;                                // waves that share a column group (ng <= 16 <= the waves of `want`)
  if (nv < 1) return TGCN_ERR_UNSUPPORTED;
  const int most = kSrAcc / (ntw * ((ntv + nv - 1) / nv));        // windows that the accumulators hold
  if (most < 1) return TGCN_ERR_UNSUPPORTED;
  const int64_t sparse_f = 2 * ((nnz + 1) / 2 * 2) + (n + 1 + 3) / 4 * 4;
  const int64_t dense_f = n <= 512 ? (n * (n | 1) + 3) / 4 * 4 : INT64_MAX;
  const int64_t graph = sparse_f < dense_f ? sparse_f : dense_f;
  for (int64_t tb = most < nwin ? most : nwin; tb >= 1; --tb) {
    const int64_t ncol = (tb + halo) * f;
    if (ncol > kSrLdsLimit) continue;
    const int64_t nc = (ncol + 3) / 4 * 4, ld = ((nc >> 2) & 1) ? nc : nc + 4;
    const int64_t bytes = (graph + (int64_t)nbuf * n * ld) * (int64_t)sizeof(float);
    if (bytes <= kSrLdsLimit) {
      out->nthr = nthr; out->dense = dense_f < sparse_f; out->tb = (int)tb; out->ld = (int)ld; out->lds = (int)bytes; out->ntw = ntw;
      out->nwin = (int)nwin; out->ntiles = (int)((nwin + tb - 1) / tb);
      return TGCN_OK;
    }
  }
  return TGCN_ERR_UNSUPPORTED;
}
