// windows_bf16.h -- the streaming time-window kernels of windows.h on bf16 tensors (tgcn_cheb_project_series_conv_bf16 /
// tgcn_cheb_series_conv_backward_bf16): bf16 sources and weights, fp32 accumulators, v_mfma_f32_16x16x32_bf16.
// Part of the single translation unit tgcn_hip.hip (included once, inside its anonymous namespace, after project.h, wgrad.h and windows.h).
#pragma once

// --------------------------------------------------------------------------------------------------
// sliding-window GEMM on bf16 sources: series_gemm_kernel's contract (windows.h), element strides, zeros outside 0 <= t < Tin
// --------------------------------------------------------------------------------------------------
// Workgroup = 4 waves; wave v owns 32 windows of one vertex (two 16-row MFMA tiles sharing their B fragments) x NT*16 columns, fp32
// accumulators.  Fragments as in project_bf16_kernel: lane (r = lane & 15, kq = lane >> 4) holds k = kq*8 .. kq*8 + 7 of row / column r.
// In the window's k index j = h*f + c a lane's 8 consecutive k are 8 contiguous bf16 of the span:
//   VEC8 (f % 8 == 0, 16-byte aligned source): a group of 8 never crosses a time row -- one 16-byte LDS read at (r*lst + h) * fp + c, the
//         rows staged with 16-byte global loads; fp = series_bf16_row_elems(f, lst) elements per span row (the bank rule below).
//   else: the span is the plain element sequence, window r at r*lst*f, j contiguous; eight 2-byte reads, k past the chunk's jn read as zero.
// The weight streams through one LDS tile of kPbKch k x NT*16 columns shared by the four waves, column-major as in project_bf16_kernel (a B
// fragment is one 16-byte read), zeros past the chunk's jn and past N.  A fragments past jn are zeros as well, so nothing outside the
// chunk's own rows ever reaches a product.
// The span keeps only the rows that are read (windows.h): lst = min(stride, HC) span rows per window, span row r*lst + hh <-> time row
// t0 + r*stride + hh (hh < hc).
//
// LDS banks of the 16-byte A read (ds_read_b128: bank = (byte / 4) % 64, i.e. 16 slots of 16 bytes; four groups of 16 lanes, each made of
// the rows {0-3, 12-15} of one kq and the rows {4-11} of the next -- every r once, two neighbouring kq).  A lane reads slot
// r*D + s(kq), D = lst * fp / 8 slots between windows, s(kq + 1) - s(kq) = 1 inside a time row.
//   f >= 16: conflict-free exactly when D = 2 (mod 4): r*D then takes each even slot twice, for r and r + 8, and every such pair has one row
//            in each half of the group, which the odd step between the two kq separates.  fp / 8 is the smallest count >= f / 8 that is
//            2 (mod 4) for an odd lst and odd for lst = 2 (mod 4): at most 3 slots (48 bytes) of padding per time row, none at f = 16, lst odd.
//   f == 8:  a k group is a whole time row, lane (r, kq) reads span row r*lst + h + kq at fp = 8 (no padding): slot = row (mod 16).  lst = 1:
//            15 consecutive rows, the two lanes on row 12 read ONE address (a broadcast): conflict-free; lst = 2: even rows from one half,
//            odd from the other: conflict-free.
//   Residual: lst = 0 (mod 4) leaves D = 0 (mod 4) whatever the padding, 2^(e-1)-way for lst = 2^e * odd as in the fp32 kernel; a pair of kq that
//            straddles a time-row end steps by fp/8 - f/8 + 1 slots, 2-way on that k step when this is even (f/8 odd, f > 8); f == 8 with an
//            odd lst >= 3 has one 2-way slot per group.  The narrow-read form is not padded (2-byte reads, 32 banks: D = lst*f/2 words).
struct SeriesGemmBf16Params {
  const hbf16* src;
  const hbf16* W;       // (nterms, H*f, N) row-major
  const void* bias;     // bias_kind 1: [N]; 2: [n][N]; fp32 or bf16 (bias_bf16)
  void* out;
  int64_t src_ks, src_ss, src_is, src_ts;   // in elements
  int64_t o_ss, o_is, o_ws, o_gs;
  int64_t n, ntiles;
  int64_t blk0;                     // the launch's first workgroup (windows.h)
  int32_t Tin, padl, nwin, H, f, N, nterms, ocg, bias_kind, bias_bf16, tpv, HC;
  int32_t stride, lst, fp;
  int32_t dil, tpp;                 // DILATED only (windows.h)
  const hbf16* ring;                // CARRY only (windows.h): (nterms, S, n, ring_ld), slot j at j * f
  int64_t ring_ks, ring_ss, ring_is;
  int32_t C, head;
  const int64_t* pos;               // CARRY only (windows.h): non-null -> head is read from pos[0], series_ring_head's rule
  int32_t win_off;                  // STRIDED && CARRY only (windows.h): the chunk row at which window 0 ends
};

__host__ __device__ inline int series_bf16_row_elems(int f, int lst) {
  int P = f >> 3;
  if (P <= 1) return 8;
  if (lst & 1) { while ((P & 3) != 2) ++P; }
  else P |= 1;
  return P * 8;
}
__host__ __device__ inline int64_t series_bf16_span_elems(int hc, int f, bool vec, int stride) {
  const int lst = series_span_lst(hc, stride);
  const int64_t rows = (int64_t)(kSgWin - 1) * lst + hc;
  return vec ? rows * series_bf16_row_elems(f, lst) : (rows * f + 7) / 8 * 8;
}

// DILATED: series_gemm_kernel's phase-major tiles (windows.h) -- 32 windows of one phase q = w % dil, staged from the sub-series
// t = (q - padl) + u * dil; span, bank rule and A reads are the step-1 form's.
// CARRY: series_gemm_kernel's ring staging (windows.h) -- a time row t < 0 comes from slot head + t + C (mod C) of the ring; a pure load,
// the bf16 values of the ring reach the span as they are.  head from the struct or, p.pos non-null, from device memory (series_ring_head).
// STRIDED && CARRY: a window step on a chunk (windows.h) -- t0 gains p.win_off, the staging below is shared by every form.
template <int NT, bool VEC8, bool STRIDED, typename OutT, bool DILATED = false, bool CARRY = false>
__global__ __launch_bounds__(kBlock) void series_gemm_bf16_kernel(const SeriesGemmBf16Params p) {
  constexpr int NW = NT * 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char sgb_lds[];
  hbf16* Ws = reinterpret_cast<hbf16*>(sgb_lds);                 // [NW][kPbLd]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const int lst = STRIDED ? p.lst : 1, stride = STRIDED ? p.stride : 1;
  const int fp = VEC8 ? p.fp : p.f;
  hbf16* span = Ws + NW * kPbLd + wave * (int)series_bf16_span_elems(p.HC, p.f, VEC8, stride);
  const uint16_t* span16 = reinterpret_cast<const uint16_t*>(span);
  static_assert(!(STRIDED && DILATED), "a window step with dilated taps is not built");
  const int64_t tile = (p.blk0 + blockIdx.x) * 4 + wave;
  bool live = tile < p.ntiles;
  const int64_t si = live ? tile / p.tpv : 0;
  int w0 = live ? (int)(tile % p.tpv) * kSgWin : 0;      // DILATED: the first window's index v0 inside its phase
  int ph = 0;                                             // DILATED: the phase q
  if constexpr (DILATED) {
    const int rem = live ? (int)(tile % p.tpv) : 0;
    ph = rem / p.tpp;
    w0 = (rem - ph * p.tpp) * kSgWin;
    live = live && ph + w0 * p.dil < p.nwin;
  }
  const int tstep = DILATED ? p.dil : stride;             // time rows between two windows' first span rows
  const int head = CARRY ? series_ring_head(p.pos, p.head, p.C) : 0;
  const int64_t s = si / p.n, iv = si % p.n;
  const int n0 = blockIdx.y * NW;
  const int J = p.H * p.f;
  const int q32 = 32 / p.f, r32 = 32 % p.f;      // one k step of 32 in (time rows, channels)
  f32x4 acc[2][NT];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[rt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int term = 0; term < p.nterms; ++term) {
    const hbf16* __restrict__ base = p.src + term * p.src_ks + s * p.src_ss + iv * p.src_is;
    const hbf16* __restrict__ Wt = p.W + (int64_t)term * J * p.N;
    const hbf16* __restrict__ rbase = CARRY ? p.ring + term * p.ring_ks + s * p.ring_ss + iv * p.ring_is : nullptr;
    for (int hc0 = 0; hc0 < p.H; hc0 += p.HC) {
      const int hcn = min(p.HC, p.H - hc0);
      const int rows = (kSgWin - 1) * lst + hcn, t0 = DILATED ? ph - p.padl + (w0 + hc0) * p.dil : w0 * stride + (STRIDED && CARRY ? p.win_off : 0) + hc0 - p.padl;
      // ---- this wave's span: span row tr = wr * lst + hh holds time row t0 + wr * stride + hh; rows hh >= hcn lie between two windows
      // (lst == HC > hcn), rows outside the series and the span of a wave without a tile are zeros
      const int fq = VEC8 ? p.f >> 3 : p.f;                  // staged units (8 elements / 1 element) per time row
      const int total = rows * fq;
      for (int e = lane; e < total; e += 64) {
        const int tr = e / fq, cu = e - tr * fq;
        const int wr = tr / lst, hh = tr - wr * lst;
        const int t = t0 + wr * tstep + hh;
        const bool ok = live && hh < hcn && t >= 0 && t < p.Tin;
        bool carried = false;
        int slot = 0;
        if constexpr (CARRY) {
          carried = live && hh < hcn && t < 0 && t >= -p.C;
          slot = head + t + p.C;
          if (slot >= p.C) slot -= p.C;
        }
        if constexpr (VEC8) {
          uint4 v = make_uint4(0u, 0u, 0u, 0u);
          if (ok) v = *reinterpret_cast<const uint4*>(base + (int64_t)t * p.src_ts + cu * 8);
          if constexpr (CARRY) { if (carried) v = *reinterpret_cast<const uint4*>(rbase + (int64_t)slot * p.f + cu * 8); }
          *reinterpret_cast<uint4*>(span + tr * fp + cu * 8) = v;
        } else {
          hbf16 v = ok ? base[(int64_t)t * p.src_ts + cu] : (hbf16)0.f;
          if constexpr (CARRY) { if (carried) v = rbase[(int64_t)slot * p.f + cu]; }
          span[e] = v;
        }
      }
      const int jn = hcn * p.f;                   // weight rows of this chunk: W rows hc0 * f + [0, jn)
      int hh = 0, cc = kq * 8;                    // VEC8: (time row, channel) of this lane's k group, kept without a division
      if constexpr (VEC8) { hh = cc / p.f; cc -= hh * p.f; }
      for (int j0 = 0; j0 < jn; j0 += kPbKch) {
        __syncthreads();                          // the previous weight tile has been read by every wave
        for (int idx = tid; idx < kPbKch * NW; idx += kBlock) {
          const int kk = idx / NW, col = idx - kk * NW;
          hbf16 v = (hbf16)0.f;
          if (j0 + kk < jn && n0 + col < p.N) v = Wt[(int64_t)(hc0 * p.f + j0 + kk) * p.N + n0 + col];
          Ws[col * kPbLd + kk] = v;
        }
        __syncthreads();                          // weight tile (and, first time round, the span) visible
#pragma unroll
        for (int ss = 0; ss < kPbKch / 32; ++ss) {
          const int kb = j0 + ss * 32 + kq * 8;   // this lane's first k of the step
          if (j0 + ss * 32 >= jn) break;
          bf16x8 a[2];
          if constexpr (VEC8) {
            uint4 v0 = make_uint4(0u, 0u, 0u, 0u), v1 = v0;
            if (kb < jn) {
              const int aoff = (r * lst + hh) * fp + cc;
              v0 = *reinterpret_cast<const uint4*>(span + aoff);
              v1 = *reinterpret_cast<const uint4*>(span + aoff + 16 * lst * fp);
            }
            a[0] = __builtin_bit_cast(bf16x8, v0);
            a[1] = __builtin_bit_cast(bf16x8, v1);
            hh += q32; cc += r32;
            if (cc >= p.f) { cc -= p.f; ++hh; }
          } else {
            const int aoff = r * lst * p.f + kb;  // + e < 31 * lst * f + jn: inside the staged rows
            using u16x8 = __attribute__((ext_vector_type(8))) unsigned short;
            u16x8 u0, u1;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const bool in = kb + e < jn;
              u0[e] = in ? span16[aoff + e] : (unsigned short)0;
              u1[e] = in ? span16[aoff + 16 * lst * p.f + e] : (unsigned short)0;
            }
            a[0] = __builtin_bit_cast(bf16x8, u0);
            a[1] = __builtin_bit_cast(bf16x8, u1);
          }
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const bf16x8 w = *reinterpret_cast<const bf16x8*>(&Ws[(nt * 16 + r) * kPbLd + ss * 32 + kq * 8]);
            acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], w, acc[0][nt], 0, 0, 0);
            acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], w, acc[1][nt], 0, 0, 0);
          }
        }
      }
      __syncthreads();                            // span and weight tile are free again
    }
  }
  if (!live) return;
  // ---- epilogue (D: col = lane & 15, row = (lane >> 4) * 4 + reg): bias in fp32, column-group addressing, one rounding
  OutT* orow0 = reinterpret_cast<OutT*>(p.out) + s * p.o_ss + iv * p.o_is;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int col = n0 + nt * 16 + r;
    if (col >= p.N) continue;
    const int64_t coff = (int64_t)(col / p.ocg) * p.o_gs + col % p.ocg;
    float b = 0.f;
    if (p.bias_kind) {
      const int64_t bi = (p.bias_kind == 2 ? iv * p.N : 0) + col;
      b = p.bias_bf16 ? bf16_lo(reinterpret_cast<const uint16_t*>(p.bias)[bi]) : reinterpret_cast<const float*>(p.bias)[bi];
    }
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int w = DILATED ? ph + (w0 + rt * 16 + kq * 4 + i) * p.dil : w0 + rt * 16 + kq * 4 + i;
        if (w < p.nwin) orow0[(int64_t)w * p.o_ws + coff] = (OutT)(acc[rt][nt][i] + b);
      }
  }
}

// series_flip_weight_kernel's index map (windows.h) on bf16 values: all phases' flipped, transposed weight.  Moves values only: exact.
__global__ __launch_bounds__(kBlock) void series_flip_weight_bf16_kernel(const hbf16* __restrict__ W, hbf16* __restrict__ Wd, int K, int H, int f, int N,
                                                                         int stride) {
  const int64_t total = (int64_t)K * H * f * N;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {   // index into W: (k, h, c, nn)
    const int nn = (int)(i % N), c = (int)((i / N) % f), h = (int)((i / ((int64_t)N * f)) % H), k = (int)(i / ((int64_t)N * f * H));
    const int ph = h % stride, m = h / stride;
    const int row = series_phase_row0(H, stride, ph) + series_phase_rows(H, stride, ph) - 1 - m;
    Wd[((int64_t)row * N + nn) * ((int64_t)K * f) + (int64_t)k * f + c] = W[i];
  }
}

// --------------------------------------------------------------------------------------------------
// weight gradient on bf16 tensors: dW[k][j][nn] = sum_{s, i, w} stack[k, s, i, tw*f + j] * g[(s, i, w), nn], fp32
// --------------------------------------------------------------------------------------------------
// series_wgrad_partial_kernel's rows and grid (windows.h) on v_mfma_f32_16x16x32_bf16, as wgrad_bf16_partial_kernel is to
// wgrad_partial_kernel: 32 rows m = (s, i, w) per instruction (A fragment: j = lane & 15, m = 8 * (lane >> 4) + e; B fragment: the same m,
// nn = lane & 15), the lane's 8 rows stepped from the first without a division.  The stack's vertex rows are st_is elements apart (>= T*f),
// g is addressed by strides in either layout.  CONV: a weight row contributes only where its own time row lies inside 0 <= t < T.
// fp32 partials per row block, folded in block order by wgrad_reduce_kernel: bit-equal across runs.
struct SeriesWgradBf16Params {
  const hbf16* stack;
  const hbf16* g;
  float* partial;                 // [nblocks][K*J][N]
  int64_t st_ks, st_is, g_ss, g_is, g_ws;
  int64_t M, rows_per_block, n;
  int32_t f, nwin, J, N, K;
  int32_t stride, padl, T;        // CONV only
  int32_t dil;                    // DIL only
};

// DIL (with CONV, step 1): weight row j = h*f + c of window w reads element (tw + h * dil) * f + c, where that time row exists.
template <bool CONV, bool DIL = false>
__global__ __launch_bounds__(64) void series_wgrad_bf16_partial_kernel(const SeriesWgradBf16Params p) {
  const int lane = threadIdx.x;
  const int r = lane & 15, kq = lane >> 4;
  const int64_t m_lo = (int64_t)blockIdx.x * p.rows_per_block;
  const int64_t m_hi = min(p.M, m_lo + p.rows_per_block);
  const int n0 = blockIdx.y * 64;
  const int tgroups = (p.K + kWgTerms - 1) / kWgTerms;
  const int jt = blockIdx.z / tgroups, tg = blockIdx.z % tgroups;
  const int t0 = tg * kWgTerms;
  const int j = jt * 16 + r;
  float* part = p.partial + (size_t)blockIdx.x * p.K * p.J * p.N;
  const int64_t si_lo = m_lo / p.nwin;
  const uint32_t w_lo = (uint32_t)(m_lo % p.nwin);
  const int64_t s_lo = si_lo / p.n;
  const uint32_t i_lo = (uint32_t)(si_lo % p.n);
  const uint32_t nwin = (uint32_t)p.nwin, nv = (uint32_t)p.n;
  const int hj = CONV ? j / p.f : 0;        // the weight time row of this lane's j
  const int hd = DIL ? hj * p.dil : hj;     // its distance from the window's first time row
  const int jd = DIL ? j + (hd - hj) * p.f : j;
  const hbf16 zero = (hbf16)0.f;
  f32x4 acc[kWgTerms][4];
#pragma unroll
  for (int t = 0; t < kWgTerms; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[t][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t m0 = m_lo; m0 < m_hi; m0 += 32) {
    bf16x8 gv[4], av[kWgTerms];
    // (vertex row, window) of the lane's first row by division, its other seven by stepping
    const int64_t mf = m0 + kq * 8;
    const uint32_t d = w_lo + (uint32_t)((mf < m_hi ? mf : m_lo) - m_lo);
    const uint32_t dv = d / nwin;
    uint32_t w = d - dv * nwin;
    const uint32_t ii = i_lo + dv, ds = ii / nv;
    uint32_t i = ii - ds * nv;
    int64_t s = s_lo + ds;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool mok = mf + e < m_hi;
      const hbf16* grow = p.g + s * p.g_ss + (int64_t)i * p.g_is + (int64_t)w * p.g_ws;
      const int tw = CONV ? (int)w * p.stride - p.padl : (int)w;      // first time row of the window
      const hbf16* arow = p.stack + (s * p.n + i) * p.st_is + (int64_t)tw * p.f + jd;
      const bool aok = mok && j < p.J && (!CONV || (tw + hd >= 0 && tw + hd < p.T));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int nn = n0 + q * 16 + r;
        gv[q][e] = (mok && nn < p.N) ? grow[nn] : zero;
      }
#pragma unroll
      for (int t = 0; t < kWgTerms; ++t) av[t][e] = (aok && t0 + t < p.K) ? arow[(int64_t)(t0 + t) * p.st_ks] : zero;
      if (++w == nwin) { w = 0; if (++i == nv) { i = 0; ++s; } }
    }
#pragma unroll
    for (int t = 0; t < kWgTerms; ++t) {
      if (t0 + t >= p.K) break;
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[t][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[t], gv[q], acc[t][q], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < kWgTerms; ++t) {
    if (t0 + t >= p.K) break;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int jj = jt * 16 + kq * 4 + i, nn = n0 + q * 16 + r;
        if (jj < p.J && nn < p.N) part[((size_t)(t0 + t) * p.J + jj) * p.N + nn] = acc[t][q][i];
      }
  }
}
