// stream_small.h -- one streaming step of a causal time layer on a graph that fits in LDS, in ONE launch (tgcn_cheb_stream_small_f32)
// Part of the single translation unit tgcn_hip.hip (included once, inside its anonymous namespace, after small_graph.h and windows.h).
#pragma once

// --------------------------------------------------------------------------------------------------
// small_stream_kernel: hops, projection and ring update of one chunk, the operand resident in LDS
// --------------------------------------------------------------------------------------------------
// The general stream step (DESIGN.md 3.10 "Streaming state") is K - 1 hop launches with their fix-ups, the CARRY projection and the ring
// update: about twenty short dependent launches per layer.  Here ONE workgroup owns ONE recording s -- its chunk rows, its output rows and
// every ring row (k, s, *, *) -- so nothing is handed from one workgroup to another and the whole step is one launch of S workgroups.
// The operand is staged once, in small_basis_kernel's two forms (CSR entries + row pointers, or the dense n x (n|1) copy).  The chunk's Tc
// time rows are walked in sub-chunks of TB rows (the plan's choice: LDS bytes and accumulator registers); a sub-chunk is an ordinary stream
// step on TB rows.  For term k = 0 .. K-1 of a sub-chunk:
//   hop      term k of the TB*fp columns (fp = f padded to 4) into LDS buffer k % nbuf: term 0 is the chunk, mode 0 P_k = L P_{k-1} (two
//            buffers), mode 1 T_k = 2 L T_{k-1} - T_{k-2} (three; the one-rounding fmaf(2, acc, -z) of small_basis_kernel).
//            thread = (vertex, 16-byte column quad): the thread groups beyond the first npad threads take further quads.
//   project  out[s, i, t, :] += sum_h row_k(i, t - (H-1-h)*dil) . W[k, h*f + c, :] on v_mfma_f32_16x16x4_f32: a wave owns a group of NTW tiles
//            of 16 columns and every NV-th tile of 16 vertices, for all time rows of the sub-chunk; per k step of a (vertex tile, time row)
//            it loads one A fragment and NTW B fragments (the weight, from L1 / L2), and its kSsAcc accumulators live through all K terms.
//            A tap inside the sub-chunk is read from the LDS buffer, an earlier one from the ring at slot head + tt + C (mod C: one compare
//            and subtract, series_gemm_kernel's CARRY map); fp32 products and sums, terms ascending, (h, c) ascending within a term, bias last.
//   update   after a barrier behind every projection read of term k: rows j in [max(0, TB - C), TB) of the buffer go to slots (head + j) mod C
//            of ring row (k, s, i) -- series_ring_update_kernel's in-place rule.
// Then bias and store of out (S, n, Tc, N), and the workgroup's own head moves by TB.
// Ring hand-over: the ring is written and read back by the same workgroup in one launch.  p.ring is a plain float* (never const __restrict__,
// never non-temporal), every ring load has a lane-dependent address (the vertex), so it is a vector load through the CU's own L1, the cache
// the workgroup's stores went through; and a __syncthreads() stands between the stores of one sub-chunk and the loads of the next (the barrier
// at the top of the sub-chunk loop, and two more per term).
// Barriers: every thread of the workgroup reaches every barrier -- threads beyond the n vertices and waves without an item only skip work.
// head: p.pos non-null -> pos[0] is read once, before any store, by series_ring_head's rule (0 unless 0 <= pos[0] < C); pos is never written.
// Index arithmetic: 32 bits inside the workgroup's LDS image, inside ONE recording's rows of the chunk, the output and a term of the ring,
// and inside the weight -- the entry refuses n*Tc*f, n*Tc*N, n*ring_ld or K*H*f*N of 2^31 or more; the recording and the term enter in 64 bits.
constexpr int kSsAcc = 16;          // accumulator tiles (f32x4) per wave
constexpr int kSsMaxThreads = 1024;
constexpr int kSsLdsLimit = 160 * 1024;

struct StreamSmallParams {
  const int32_t* rowptr;
  const tgcn_edge* ev;
  const float* chunk;     // (S, n, Tc*f), operand labels
  const float* W;         // (K, H*f, N), the kernels' working basis
  const float* bias;      // bias_kind 1: [N]; 2: [n][N]
  float* out;             // (S, n, Tc, N)
  float* ring;            // (K, S, n, ring_ld), slot j at j * f; read AND written here
  const int64_t* pos;     // nullable: the slot of the oldest row in device memory
  int32_t S, ring_ld;     // recordings; floats per ring row: 16 ring rows stay inside 32 bits (the entry's check)
  int32_t n, nnz, Tc, f, fp, H, N, K, bias_kind, TB, ld, C, head, dil;
};

template <bool DENSE, int NTW, int MODE>
__global__ __launch_bounds__(kSsMaxThreads) void small_stream_kernel(const StreamSmallParams p) {
  extern __shared__ __align__(16) float smem[];
  // the scalars every phase reads.  Each phase starts by passing the ones it uses through an empty asm (SS_PIN): what it derives from them --
  // strides, 64-bit bases, loop bounds -- is then formed inside the phase and dies with it, instead of being hoisted in front of the main
  // loop and kept (or spilled) across all the other phases.  No instruction is emitted for a pin.
#define SS_PIN4(a, b, c, d) asm volatile("" : "+s"(a), "+s"(b), "+s"(c), "+s"(d))
  int n = p.n, f = p.f, fp = p.fp, ld = p.ld, C = p.C, N = p.N, H = p.H, Tc = p.Tc, TB = p.TB, dil = p.dil, rld = p.ring_ld;
  const int nnz = p.nnz;
  const int nthr = blockDim.x, tid = threadIdx.x;
  const int lane = tid & 63;
  int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = nthr >> 6;
  const int r = lane & 15, kq = lane >> 4;
  int ldn = n | 1;
  tgcn_edge* ev = reinterpret_cast<tgcn_edge*>(smem);
  int32_t* rowptr = reinterpret_cast<int32_t*>(smem + 2 * ((nnz + 1) / 2 * 2));
  float* Ld = smem;
  float* Y = DENSE ? smem + (n * ldn + 3) / 4 * 4 : reinterpret_cast<float*>(rowptr) + (n + 1 + 3) / 4 * 4;   // nbuf buffers of n x ld
  constexpr int nbuf = MODE == 0 ? 2 : 3;
  int head = series_ring_head(p.pos, p.head, C);      // once, ahead of any store

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

  // ---- this wave's share of the projection: column group ng (NTW tiles of 16 columns) of the vertex tiles wv, wv + NV, ...; accumulator
  // slot sl holds (vertex tile wv + (sl / TB) * NV, time row sl % TB) x the NTW column tiles.  The slot loops are unrolled (static register
  // indices) and walk (vertex tile, time row) as two running wave-uniform counters behind an empty asm: what a slot derives from them is
  // computed where it is used instead of being kept in registers for all slots at once (which spills).
  constexpr int NSLOT = kSsAcc / NTW;
  int ntv = (n + 15) / 16;
  const int ntn = (N + 15) / 16;
  const int NG = (ntn + NTW - 1) / NTW;
  int NV = nwaves / NG;
  const int wq = wave / NG;
  int cg0 = (wave - wq * NG) * (NTW * 16);            // first column of this wave's group
  int wv = wq < NV ? wq : ntv;                  // a wave beyond the last full row of column groups owns no vertex tile
  // hop: thread = (vertex hv, quad group hg); groups step through the 16-byte quads of the sub-chunk's columns
  const int npad = (n + 63) / 64 * 64;
  int hgroups = nthr / npad;
  const int hv = tid % npad, hg = tid / npad;
  int J = H * f, q4 = 4 / f;             // one k step moves (h, c) by 4 weight rows

  for (int t0 = 0; t0 < Tc; t0 += TB) {
    const int tb = min(TB, Tc - t0);
    const int ncol = tb * fp;
    __syncthreads();      // buffer 0 is free (and the operand staged); the ring stores of the last sub-chunk are behind every wave
    // term 0: the chunk's rows t0 .. t0 + tb - 1, channels padded with zeros; wave = vertex, lane = channel (no division anywhere)
    int so = blockIdx.x;                               // the recording behind an empty asm, phase by phase: the 64-bit global bases are
    asm volatile("" : "+s"(so));                       // formed where they are used and not kept in registers across the other phases
    {
      SS_PIN4(n, ld, f, fp); SS_PIN4(Tc, wave, nwaves, so);
      for (int i = wave; i < n; i += nwaves) {
        const float* crow = p.chunk + (int64_t)so * (n * Tc * f) + (unsigned)((i * Tc + t0) * f);
        for (int j = 0; j < tb; ++j)
          for (int c = lane; c < fp; c += 64) Y[i * ld + j * fp + c] = c < f ? crow[j * f + c] : 0.f;
      }
    }
    f32x4 acc[kSsAcc];
#pragma unroll
    for (int j = 0; j < kSsAcc; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    int bk = 0, b1 = nbuf - 1, b2 = nbuf - 2;          // buffers of term k, k - 1, k - 2 (b2 is read in mode 1 only: three buffers)
    for (int k = 0; k < p.K; ++k) {
      float* Bk = Y + bk * n * ld;
      asm volatile("" : "+s"(so));
      float* ring_k = p.ring + ((int64_t)k * p.S + so) * (n * rld);
      SS_PIN4(n, ld, ldn, hgroups);                    // (in front of the hop's lane-dependent branch: a pin stays wave-uniform)
      if (k > 0 && hv < n && hg < hgroups) {           // ---- hop
        const float* B1 = Y + b1 * n * ld;
        const float* B2 = Y + b2 * n * ld;
        for (int q = hg; q < (ncol >> 2); q += hgroups) {
          float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
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
          if (MODE == 1 && k >= 2) {                 // one rounding, like 2*X - Xt[k-2] of the reference
            const float4 z = reinterpret_cast<const float4*>(B2 + hv * ld)[q];
            a.x = fmaf(2.f, a.x, -z.x); a.y = fmaf(2.f, a.y, -z.y); a.z = fmaf(2.f, a.z, -z.z); a.w = fmaf(2.f, a.w, -z.w);
          }
          reinterpret_cast<float4*>(Bk + hv * ld)[q] = a;
        }
      }
      __syncthreads();    // term k is complete in Bk
      {                   // ---- project
        SS_PIN4(n, ld, f, fp); SS_PIN4(C, N, H, dil); SS_PIN4(J, q4, rld, head); SS_PIN4(ntv, NV, wv, cg0); asm volatile("" : "+s"(TB));
        const float* Wg = p.W + (unsigned)(k * J * N + cg0);     // wave-uniform: this term, this column group
        const int clast = N - 1 - cg0;     // the last column, counted from the group's first (>= 0: the group holds a column)
        const int ksteps = (J + 3) >> 2, r4 = 4 - q4 * f;      // one k step moves (h, c) by 4 weight rows
        const int h0 = kq / f, c0 = kq - h0 * f;       // (h, c) of this lane's weight row jj = 4 ks + kq at ks = 0
        int vt = wv, tl = 0;
#pragma unroll
        for (int sl = 0; sl < NSLOT; ++sl) {           // slot by slot: one short k loop each
          asm volatile("" : "+s"(vt), "+s"(tl));
          if (vt < ntv && tl < tb) {          // wave-uniform
            // branch-free taps, so that the loads of several k steps are in flight at once: a vertex past n reads vertex n - 1 (its
            // output rows are never stored), a weight row past J reads tap H - 1 and counts as zero, and BOTH sources are loaded at an
            // address that is always valid -- the buffer's row start for a tap that lives in the ring, slot 0 for one that does not
            const int vr = min(vt * 16 + r, n - 1);
            const float* Bv = Bk + vr * ld;
            const float* Rv = ring_k + (unsigned)(vr * rld);
            int h = h0, c = c0;
            for (int ks = 0; ks < ksteps; ++ks) {
              const int jj = ks * 4 + kq;
              const int tt = tl - (H - 1 - min(h, H - 1)) * dil;      // the tap's time row, counted from the sub-chunk's first
              const bool inb = tt >= 0;
              int slot = head + tt + C;                               // tt >= -C: the ring's slot head + tt + C (mod C)
              if (slot >= C) slot -= C;
              const float a_buf = Bv[inb ? tt * fp + c : 0];
              const float a_ring = Rv[(unsigned)((inb ? 0 : slot) * f + c)];
              const float av = jj < J ? (inb ? a_buf : a_ring) : 0.f;
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
      __syncthreads();    // every projection read of term k (ring and buffer) is done
      {                   // ---- update the ring, in place: wave = vertex, lane = channel; the slot runs along with the row
        SS_PIN4(n, ld, f, fp); SS_PIN4(C, head, rld, wave); asm volatile("" : "+s"(nwaves));
        const int j0 = tb > C ? tb - C : 0;
        int slot0 = head + j0;                         // < C + tb
        while (slot0 >= C) slot0 -= C;
        for (int i = wave; i < n; i += nwaves) {
          float* rrow = ring_k + (unsigned)(i * rld);
          int slot = slot0;
          for (int j = j0; j < tb; ++j) {
            for (int c = lane; c < f; c += 64) rrow[slot * f + c] = Bk[i * ld + j * fp + c];
            if (++slot == C) slot = 0;
          }
        }
      }
      b2 = b1; b1 = bk; bk = bk + 1 == nbuf ? 0 : bk + 1;
    }
    // ---- epilogue (D: col = lane & 15, row = (lane >> 4) * 4 + reg): bias last, out (S, n, Tc, N)
    {
      SS_PIN4(n, N, Tc, TB); SS_PIN4(ntv, NV, wv, cg0); asm volatile("" : "+s"(so));
      int vt = wv, tl = 0, c0g = cg0;
  #pragma unroll
      for (int sl = 0; sl < NSLOT; ++sl) {
        asm volatile("" : "+s"(vt), "+s"(tl), "+s"(c0g), "+s"(so));
        if (vt < ntv && tl < tb) {
  #pragma unroll
          for (int nl = 0; nl < NTW; ++nl) {
            const int col = c0g + nl * 16 + r;
            if (col < N) {
  #pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int v = vt * 16 + kq * 4 + i;
                if (v < n) {
                  float b = 0.f;
                  if (p.bias_kind == 1) b = p.bias[col];
                  else if (p.bias_kind == 2) b = p.bias[(unsigned)(v * N + col)];
                  (p.out + (int64_t)so * (n * Tc * N))[(unsigned)((v * Tc + t0 + tl) * N + col)] = acc[sl * NTW + nl][i] + b;
                }
              }
            }
          }
        }
        if (++tl == TB) { tl = 0; vt += NV; }
      }
    }
    head += tb;
    while (head >= C) head -= C;
  }
#undef SS_PIN4
}

// The plan: threads, carve-up, floats per buffer row and the sub-chunk length; false where the shape does not fit.
//   ntw      column tiles per wave (4 / 2 / 1 for N > 48 / > 16 / else); ng = ceil(ceil(N/16) / ntw) column groups, at most 16 (N <= 1024)
//   threads  one per vertex at least, and a wave per (vertex tile, column group) where 1024 threads allow it
//   TB       the most time rows (<= Tc) that the accumulators hold -- kSsAcc >= ntw * (vertex tiles per wave) * TB -- and whose buffers fit the
//            LDS next to the operand
//   ld       TB * fp floats, plus 4 where that makes ld / 4 odd: the 16 vertices x 4 k of an A-fragment read fall into 64 different banks
struct StreamSmallPlan { int nthr, dense, tb, ld, lds, ntw; };
inline int stream_small_ld(int tb, int fp) { const int nc = tb * fp; return ((nc >> 2) & 1) ? nc : nc + 4; }
inline bool stream_small_plan(int64_t n, int64_t nnz, int32_t mode, int32_t f, int32_t N, int32_t Tc, StreamSmallPlan* out) {
  if (n < 1 || n > (int64_t)kSmallMaxN || nnz < 0 || nnz > (1 << 20) || (mode != 0 && mode != 1) || f < 1 || N < 1 || Tc < 1) return false;
  if ((int64_t)f > kSsLdsLimit || N > 1024) return false;
  const int fp = (f + 3) / 4 * 4, nbuf = mode == 0 ? 2 : 3;
  const int ntv = (int)((n + 15) / 16), ntn = (N + 15) / 16;
  const int ntw = ntn >= 4 ? 4 : (ntn >= 2 ? 2 : 1), ng = (ntn + ntw - 1) / ntw;
  const int need = (int)((n + 63) / 64 * 64), want = 64 * (ntv * ng < kSsMaxThreads / 64 ? ntv * ng : kSsMaxThreads / 64);
  const int nthr = need > want ? need : want;
  const int nv = (nthr / 64) / ng;                                // waves that share a column group (ng <= 16 <= the waves of `want`)
  if (nv < 1) return false;
  const int most = kSsAcc / (ntw * ((ntv + nv - 1) / nv));        // time rows that the accumulators hold
  if (most < 1) return false;
  const int64_t sparse_f = 2 * ((nnz + 1) / 2 * 2) + (n + 1 + 3) / 4 * 4;
  const int64_t dense_f = n <= 512 ? (n * (n | 1) + 3) / 4 * 4 : INT64_MAX;
  const int64_t graph = sparse_f < dense_f ? sparse_f : dense_f;
  for (int tb = most < Tc ? most : Tc; tb >= 1; --tb) {
    const int ld = stream_small_ld(tb, fp);
    const int64_t bytes = (graph + (int64_t)nbuf * n * ld) * (int64_t)sizeof(float);
    if (bytes <= kSsLdsLimit) {
      out->nthr = nthr; out->dense = dense_f < sparse_f; out->tb = tb; out->ld = ld; out->lds = (int)bytes; out->ntw = ntw;
      return true;
    }
  }
  return false;
}
