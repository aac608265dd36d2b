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
  extern __shared__ __align__(16) float smem[];
  // the scalars every phase reads, pinned phase by phase like small_stream_kernel's (no instruction is emitted for a pin)
#define SR_PIN4(a, b, c, d) asm volatile("" : "+s"(a), "+s"(b), "+s"(c), "+s"(d))
  int n = p.n, f = p.f, ld = p.ld, N = p.N, H = p.H, T = p.T, TB = p.TB, dil = p.dil, nwin = p.nwin;
  const int nnz = p.nnz;
  const int nthr = blockDim.x, tid = threadIdx.x;
  const int lane = tid & 63;
  int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = nthr >> 6;
  const int r = lane & 15, kq = lane >> 4;
  int ldn = n | 1;
  tgcn_edge* ev = reinterpret_cast<tgcn_edge*>(smem);
  int32_t* rowptr = reinterpret_cast<int32_t*>(smem + 2 * ((nnz + 1) / 2 * 2));
  float* Ld = smem;
  float* Y = DENSE ? smem + (n * ldn + 3) / 4 * 4 : reinterpret_cast<float*>(rowptr) + (n + 1 + 3) / 4 * 4;   // the term buffers, n x ld each

  // ---- the tile: recording so, windows [w0, w0 + tbw), the span's first float g0 inside a recording's row of T*f floats (may be negative)
  const int blk = p.blk0 + (int)blockIdx.x;
  int so = blk / p.ntiles;
  const int tj = blk - so * p.ntiles;
  int w0 = tj * TB;
  int tbw = min(TB, nwin - w0);
  const bool last = tj == p.ntiles - 1;
  int ncol = (TB + (H - 1) * dil) * f;
  int g0 = (w0 - p.left) * f;
  int Tf = T * f;

  // ---- the operand -> LDS (small_basis_kernel's two forms)
  if (DENSE) {
    for (int e = tid; e < n * ldn; e += nthr) Ld[e] = 0.f;
    __syncthreads();
    if (tid < n)
      for (int e = p.rowptr[tid]; e < p.rowptr[tid + 1]; ++e) Ld[tid * ldn + p.ev[e].col] += p.ev[e].val;
  } else {
    for (int e = tid; e < nnz; e += nthr) ev[e] = p.ev[e];
    for (int i = tid; i <= n; i += nthr) rowptr[i] = p.rowptr[i];
  }
  // ---- term 0: the span, wave = vertex, lane = float of the row; zeros outside the recording and in the row's tail
  {
    SR_PIN4(n, ld, ncol, g0); SR_PIN4(Tf, wave, nwaves, so);
    const float* srec = p.series + (int64_t)so * (n * Tf);
    for (int i = wave; i < n; i += nwaves) {
      const float* srow = srec + (unsigned)(i * Tf);
      for (int c = lane; c < ld; c += 64) {
        const int g = g0 + c;
        Y[i * ld + c] = (c < ncol && g >= 0 && g < Tf) ? srow[g] : 0.f;
      }
    }
  }

  // ---- this wave's share of the projection (small_stream_kernel's carve-up): column group of NTW tiles of 16 columns, vertex tiles wv,
  // wv + NV, ...; accumulator slot sl holds (vertex tile wv + (sl / TB) * NV, window sl % TB) x the NTW column tiles
  constexpr int NSLOT = kSrAcc / NTW;
  int ntv = (n + 15) / 16;
  const int ntn = (N + 15) / 16;
  const int NG = (ntn + NTW - 1) / NTW;
  int NV = nwaves / NG;
  const int wq = wave / NG;
  int cg0 = (wave - wq * NG) * (NTW * 16);            // first column of this wave's group
  int wv = wq < NV ? wq : ntv;                        // a wave beyond the last full row of column groups owns no vertex tile
  // hop: thread = (vertex hv, quad group hg)
  const int npad = (n + 63) / 64 * 64;
  int hgroups = nthr / npad;
  const int hv = tid % npad, hg = tid / npad;
  int nquad = (ncol + 3) >> 2;
  int J = H * f, q4 = 4 / f, df = dil * f;

  f32x4 acc[kSrAcc];
#pragma unroll
  for (int j = 0; j < kSrAcc; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k = 0; k < p.K; ++k) {
    float* Bk = MODE == 0 ? Y : Y + (k & 1) * n * ld;
    if (k > 0) {                                       // ---- hop
      SR_PIN4(n, ld, ldn, hgroups); asm volatile("" : "+s"(nquad));
      const float* B1 = MODE == 0 ? Y : Y + ((k - 1) & 1) * n * ld;
      const bool mine = hv < n && hg < hgroups;
      for (int q0 = 0; q0 < nquad; q0 += hgroups) {    // a pass: uniform count, so every thread meets the pass's barrier
        const int q = q0 + hg;
        const bool on = mine && q < nquad;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on) {
          if (DENSE) {
            for (int col = 0; col < n; ++col) {
              const float lv = Ld[hv * ldn + col];
              const float4 y = reinterpret_cast<const float4*>(B1 + col * ld)[q];
              a.x = fmaf(lv, y.x, a.x); a.y = fmaf(lv, y.y, a.y); a.z = fmaf(lv, y.z, a.z); a.w = fmaf(lv, y.w, a.w);
            }
          } else {
            for (int e = rowptr[hv]; e < rowptr[hv + 1]; ++e) {
              const tgcn_edge ed = ev[e];
              const float4 y = reinterpret_cast<const float4*>(B1 + ed.col * ld)[q];
              a.x = fmaf(ed.val, y.x, a.x); a.y = fmaf(ed.val, y.y, a.y); a.z = fmaf(ed.val, y.z, a.z); a.w = fmaf(ed.val, y.w, a.w);
            }
          }
          if (MODE == 1 && k >= 2) {                   // one rounding, like 2*X - Xt[k-2] of the reference; z is the element written below
            const float4 z = reinterpret_cast<const float4*>(Bk + hv * ld)[q];
            a.x = fmaf(2.f, a.x, -z.x); a.y = fmaf(2.f, a.y, -z.y); a.z = fmaf(2.f, a.z, -z.z); a.w = fmaf(2.f, a.w, -z.w);
          }
        }
        if (MODE == 0) __syncthreads();                // in place: every read of this pass (and of term k-1's projection) is done
        if (on) reinterpret_cast<float4*>(Bk + hv * ld)[q] = a;
      }
    }
    __syncthreads();      // term k is complete in Bk (k == 0: the span and the operand are staged)
    if (p.stack) {        // ---- the owned rows of term k -> stack: wave = vertex, lane = float of the row
      SR_PIN4(n, ld, g0, Tf); SR_PIN4(TB, f, wave, nwaves); asm volatile("" : "+s"(so));
      const int ownc = last ? ncol : TB * f;
      float* trec = p.stack + ((int64_t)k * p.S + so) * (n * Tf);
      for (int i = wave; i < n; i += nwaves) {
        float* trow = trec + (unsigned)(i * Tf);
        for (int c = lane; c < ownc; c += 64) {
          const int g = g0 + c;
          if (g >= 0 && g < Tf) trow[g] = Bk[i * ld + c];
        }
      }
    }
    {                     // ---- project
      SR_PIN4(n, ld, f, df); SR_PIN4(N, H, J, q4); SR_PIN4(ntv, NV, wv, cg0); asm volatile("" : "+s"(TB), "+s"(tbw));
      const float* Wg = p.W + (unsigned)(k * J * N + cg0);     // wave-uniform: this term, this column group
      const int clast = N - 1 - cg0;     // the last column, counted from the group's first (>= 0: the group holds a column)
      const int ksteps = (J + 3) >> 2, r4 = 4 - q4 * f;        // one k step moves (h, c) by 4 weight rows
      const int h0 = kq / f, c0 = kq - h0 * f;                 // (h, c) of this lane's weight row jj = 4 ks + kq at ks = 0
      int vt = wv, tl = 0;
#pragma unroll
      for (int sl = 0; sl < NSLOT; ++sl) {             // slot by slot: one short k loop each
        asm volatile("" : "+s"(vt), "+s"(tl));
        if (vt < ntv && tl < tbw) {                    // wave-uniform
          // branch-free taps: a vertex past n reads vertex n - 1 (its output rows are never stored), a weight row past J reads tap H - 1
          // and counts as zero
          const float* Bv = Bk + min(vt * 16 + r, n - 1) * ld + tl * f;
          int h = h0, c = c0;
          for (int ks = 0; ks < ksteps; ++ks) {
            const int jj = ks * 4 + kq;
            const float a_buf = Bv[min(h, H - 1) * df + c];
            const float av = jj < J ? a_buf : 0.f;
#pragma unroll
            for (int nl = 0; nl < NTW; ++nl) {
              // columns past N read the last column: never stored
              const float bv = Wg[(unsigned)(min(jj, J - 1) * N + min(nl * 16 + r, clast))];
              acc[sl * NTW + nl] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[sl * NTW + nl], 0, 0, 0);
            }
            h += q4; c += r4;
            if (c >= f) { c -= f; ++h; }
          }
        }
        if (++tl == TB) { tl = 0; vt += NV; }
      }
    }
  }
  // ---- epilogue (D: col = lane & 15, row = (lane >> 4) * 4 + reg): bias last; window-major rows are n*N apart, series rows N
  {
    SR_PIN4(n, N, nwin, TB); SR_PIN4(ntv, NV, wv, cg0); SR_PIN4(so, w0, tbw, wave);
    float* orec = p.out + (int64_t)so * (n * nwin * N);
    const int vs = p.as_series ? nwin * N : N, ws = p.as_series ? N : n * N;
    int vt = wv, tl = 0;
#pragma unroll
    for (int sl = 0; sl < NSLOT; ++sl) {
      asm volatile("" : "+s"(vt), "+s"(tl));
      if (vt < ntv && tl < tbw) {
#pragma unroll
        for (int nl = 0; nl < NTW; ++nl) {
          const int col = cg0 + nl * 16 + r;
          if (col < N) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int v = vt * 16 + kq * 4 + i;
              if (v < n) {
                float b = 0.f;
                if (p.bias_kind == 1) b = p.bias[col];
                else if (p.bias_kind == 2) b = p.bias[(unsigned)(v * N + col)];
                orec[(unsigned)(v * vs + (w0 + tl) * ws + col)] = acc[sl * NTW + nl][i] + b;
              }
            }
          }
        }
      }
      if (++tl == TB) { tl = 0; vt += NV; }
    }
  }
#undef SR_PIN4
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
