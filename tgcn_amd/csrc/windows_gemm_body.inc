// windows_gemm_body.inc -- the body of series_gemm_kernel, of series_gemm_pool_dropout_kernel and of series_gemm_chunk_pool_dropout_kernel
// (windows.h), included once in each with TGCN_SERIES_GEMM_DROP 0 / 1 / 2 (2: 1 with the mask's window taken from `at`).  Textual on purpose: behind a shared __forceinline__ function the instantiations without dropout came out
// with other register counts and schedules than before (DESIGN.md 3.10, "dropout in the relu + pool epilogue"); included with 0, the
// compiler sees the tokens the kernel always had.  Names from the including kernel: NT, VEC, STRIDED, DILATED, CARRY, POOLED, p, and -- with
// TGCN_SERIES_GEMM_DROP -- dp.
  constexpr int NW = NT * 16, NS = series_ws_stride(NT), WREG = (kSgKT * NW) / kBlock;
  extern __shared__ __attribute__((aligned(16))) float sg_lds[];
  float* Ws = sg_lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const int fp = STRIDED ? p.fp : (VEC ? p.f + 2 : p.f);
  const int lst = STRIDED ? p.lst : 1;          // span rows between consecutive windows
  float* span = sg_lds + kSgKT * NS + wave * (int)(STRIDED ? series_span_floats(p.HC, p.f, VEC, p.stride) : series_span_floats(p.HC, p.f, VEC));
  static_assert(!(STRIDED && DILATED), "a window step with dilated taps is not built");
  static_assert(!(POOLED && STRIDED && CARRY), "a pooled window step on a chunk is not built");
  const int64_t tile = POOLED ? p.blk0 + blockIdx.x : (p.blk0 + blockIdx.x) * 4 + wave;
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
  const int tstep = DILATED ? p.dil : 1;                  // time rows between two span rows
  const int head = CARRY ? series_ring_head(p.pos, p.head, p.C) : 0;
  const bool wg_live = live;                              // POOLED: the same for the four waves (they share the tile)
  int64_t s, iv;
  if constexpr (POOLED) {
    s = si / p.nq;
    iv = (si % p.nq) * 4 + wave;
    live = live && iv < p.n;
    if (!live) iv = 0;
  } else {
    s = si / p.n;
    iv = si % p.n;
  }
  const int n0 = blockIdx.y * NW;
  const int J = p.H * p.f;
  f32x4 acc[2][NT];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[rt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int term = 0; term < p.nterms; ++term) {
    const float* __restrict__ base = p.src + term * p.src_ks + s * p.src_ss + iv * p.src_is;
    const float* __restrict__ Wt = p.W + (int64_t)term * J * p.N;
    const float* __restrict__ rbase = CARRY ? p.ring + term * p.ring_ks + s * p.ring_ss + iv * p.ring_is : nullptr;
    for (int hc0 = 0; hc0 < p.H; hc0 += p.HC) {
      const int hcn = min(p.HC, p.H - hc0);
      const int rows = (kSgWin - 1) * lst + hcn,
                t0 = DILATED ? ph - p.padl + (w0 + hc0) * p.dil
                             : (STRIDED ? w0 * p.stride + (CARRY ? p.win_off : 0) : w0) + hc0 - p.padl;
      // ---- this wave's span: time rows t0 .. t0 + rows - 1 (zeros outside the series, and for a wave without a tile)
      if constexpr (STRIDED) {
        // span row tr = wr * lst + hh holds time row t0 + wr * stride + hh; rows hh >= hcn lie between two windows (lst == HC > hcn): zeros
        const int fq = VEC ? p.f >> 2 : p.f;                      // staged units (float4 / float) per time row
        const int total = VEC ? rows * fq : ((rows * p.f + 4 + 3) / 4 * 4);
        for (int e = lane; e < total; e += 64) {
          const int tr = e / fq, cu = e - tr * fq;
          const int wr = tr / lst, hh = tr - wr * lst;
          const int t = t0 + wr * p.stride + hh;
          const bool ok = live && tr < rows && hh < hcn && t >= 0 && t < p.Tin;
          bool carried = false;
          int slot = 0;
          if constexpr (CARRY) {
            carried = live && tr < rows && hh < hcn && t < 0 && t >= -p.C;
            slot = head + t + p.C;
            if (slot >= p.C) slot -= p.C;
          }
          if constexpr (VEC) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) v = *reinterpret_cast<const float4*>(base + (int64_t)t * p.src_ts + cu * 4);
            if constexpr (CARRY) { if (carried) v = *reinterpret_cast<const float4*>(rbase + (int64_t)slot * p.f + cu * 4); }
            float* d = span + tr * fp + cu * 4;
            if (fp & 1) { d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }      // odd rows: 4-byte aligned only
            else {
              reinterpret_cast<float2*>(d)[0] = make_float2(v.x, v.y);
              reinterpret_cast<float2*>(d)[1] = make_float2(v.z, v.w);
            }
          } else {
            float v = ok ? base[(int64_t)t * p.src_ts + cu] : 0.f;
            if constexpr (CARRY) { if (carried) v = rbase[(int64_t)slot * p.f + cu]; }
            span[e] = v;
          }
        }
      } else if constexpr (VEC) {
        const int f4 = p.f >> 2, total4 = rows * f4;
        for (int e = lane; e < total4; e += 64) {
          const int tr = e / f4, c = (e - tr * f4) * 4, t = t0 + tr * tstep;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (live && t >= 0 && t < p.Tin) v = *reinterpret_cast<const float4*>(base + (int64_t)t * p.src_ts + c);
          if constexpr (CARRY) {
            if (live && t < 0 && t >= -p.C) {
              int slot = head + t + p.C;
              if (slot >= p.C) slot -= p.C;
              v = *reinterpret_cast<const float4*>(rbase + (int64_t)slot * p.f + c);
            }
          }
          float2* d = reinterpret_cast<float2*>(span + tr * fp + c);
          d[0] = make_float2(v.x, v.y);
          d[1] = make_float2(v.z, v.w);
        }
      } else {
        const int total = (int)series_span_floats(hcn, p.f, false);
        for (int e = lane; e < total; e += 64) {
          const int tr = e / p.f, c = e - tr * p.f, t = t0 + tr * tstep;
          float v = (live && tr < rows && t >= 0 && t < p.Tin) ? base[(int64_t)t * p.src_ts + c] : 0.f;
          if constexpr (CARRY) {
            if (live && tr < rows && t < 0 && t >= -p.C) {
              int slot = head + t + p.C;
              if (slot >= p.C) slot -= p.C;
              v = rbase[(int64_t)slot * p.f + c];
            }
          }
          span[e] = v;
        }
      }
      const int jn = hcn * p.f;                 // weight rows of this chunk: W rows hc0 * f + [0, jn)
      int hh = 0, cc = 0;                       // VEC: (time row, channel) of the current k step, kept without a division
      for (int j0 = 0; j0 < jn; j0 += kSgKT) {
        __syncthreads();                        // the previous weight tile has been read by every wave
#pragma unroll
        for (int h = 0; h < WREG; ++h) {
          const int idx = tid + h * kBlock;
          const int kk = idx / NW, col = idx % NW;
          const bool ok = (j0 + kk < jn) && (n0 + col < p.N);
          Ws[kk * NS + col] = ok ? Wt[(int64_t)(hc0 * p.f + j0 + kk) * p.N + n0 + col] : 0.f;
        }
        __syncthreads();                        // weight tile (and, first time round, the span) visible
        const int ksteps = min(kSgKT, jn - j0 + 3) >> 2;
        // steps whose four k are all weight rows; the scalar-load form has at most one more, the ragged last step of a chunk (jn % 4 != 0).
        // There k >= jn lies in the first floats of time row r + hcn of the span, which belongs to LATER windows; its zero weight row
        // cancels a finite value only (0 * Inf = NaN), so that one step reads zero on the A side as well -- peeled, the loop is untouched
        const int kfull = VEC ? ksteps : min(kSgKT, jn - j0) >> 2;
        auto kstep = [&](const int ks, auto ragged) {
          int aoff;
          bool kin = true;
          if constexpr (VEC) {
            aoff = ((STRIDED ? r * lst : r) + hh) * fp + cc + kq;
            cc += 4;
            if (cc >= p.f) { cc = 0; ++hh; }
          } else {
            aoff = (STRIDED ? r * lst : r) * p.f + j0 + ks * 4 + kq;  // < 31 * lst * f + jn + 3: inside the zero-tailed span
            if constexpr (decltype(ragged)::value) kin = j0 + ks * 4 + kq < jn;
          }
          const float a0 = kin ? span[aoff] : 0.f;
          const float a1 = kin ? span[aoff + (STRIDED ? 16 * lst : 16) * fp] : 0.f;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const float bv = Ws[(ks * 4 + kq) * NS + nt * 16 + r];
            acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv, acc[0][nt], 0, 0, 0);
            acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv, acc[1][nt], 0, 0, 0);
          }
        };
        for (int ks = 0; ks < kfull; ++ks) kstep(ks, std::false_type{});
        if constexpr (!VEC) {
          if (kfull < ksteps) kstep(kfull, std::true_type{});
        }
      }
      __syncthreads();                          // span and weight tile are free again
    }
  }
  if constexpr (POOLED) {
    // ---- pooled epilogue: bias into the scratch [wave][window][col], one barrier, relu + max over the group's waves
    if (!wg_live) return;                       // the whole workgroup: a DILATED block past its phase
    if (live) {
      float* sc = sg_lds + wave * (kSgWin * NW);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int col = n0 + nt * 16 + r;
        float b = 0.f;
        if (col < p.N) {
          if (p.bias_kind == 1) b = p.bias[col];
          else if (p.bias_kind == 2) b = p.bias[iv * p.N + col];
        }
#if TGCN_SERIES_GEMM_DROP      // t = relu(acc + bias) * mask in the scratch (windows.h, DROP)
        const uint64_t seed = (uint64_t)dp.seed[0];
        const bool quad = (p.N & 3) == 0;     // n0 and nt * 16 are multiples of 4: col & 3 == r & 3 == e & 3
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
          uint64_t e[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int wl = rt * 16 + kq * 4 + i;
            const int64_t w = DILATED ? ph + (int64_t)(w0 + wl) * p.dil : w0 + wl;
#if TGCN_SERIES_GEMM_DROP == 2  // a chunk: the window's place in the whole series (windows.h, DROP on a CHUNK)
            e[i] = (uint64_t)(((s * at.nwin + at.w0 + w) * p.n + iv) * p.N + col);
#else
            e[i] = (uint64_t)(((s * p.nwin + w) * p.n + iv) * p.N + col);
#endif
          }
          bool keep[4];
          if (quad) {
            const int j = r & 3;
            uint32_t wd[4];
            dropout_words(seed, (j == 0 ? e[0] : j == 1 ? e[1] : j == 2 ? e[2] : e[3]) >> 2, wd);
            uint32_t x[4][4];                 // x[i][k]: word k of window i's call
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              x[0][k] = series_quad_bcast<0>(wd[k]); x[1][k] = series_quad_bcast<1>(wd[k]);
              x[2][k] = series_quad_bcast<2>(wd[k]); x[3][k] = series_quad_bcast<3>(wd[k]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) keep[i] = (j == 0 ? x[i][0] : j == 1 ? x[i][1] : j == 2 ? x[i][2] : x[i][3]) >= dp.thr;
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) keep[i] = dropout_keep(seed, e[i], dp.thr);
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) sc[(rt * 16 + kq * 4 + i) * NW + nt * 16 + r] = relu_dropout(acc[rt][nt][i] + b, keep[i], dp.scale);
        }
#else
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int i = 0; i < 4; ++i) sc[(rt * 16 + kq * 4 + i) * NW + nt * 16 + r] = acc[rt][nt][i] + b;
#endif
      }
    }
    __syncthreads();                            // all four waves: the scratch is written
    const int pool = p.pool;
    const int64_t v00 = (si % p.nq) * 4;        // first vertex of the quad
    float* orow0 = p.out + s * p.o_ss;
    uint8_t* irow0 = p.idx ? p.idx + s * p.o_ss : nullptr;
    for (int e = tid; e < (4 / pool) * kSgWin * NW; e += kBlock) {
      const int c = e % NW, wl = (e / NW) % kSgWin, grp = e / (NW * kSgWin);
      const int col = n0 + c;
      const int64_t v0 = v00 + grp * pool;
      const int w = DILATED ? ph + (w0 + wl) * p.dil : w0 + wl;
      if (col >= p.N || v0 >= p.n || w >= p.nwin) continue;
      const float* src = sg_lds + (grp * pool) * (kSgWin * NW) + wl * NW + c;
      float best = src[0];
      int bi = 0;
      for (int j = 1; j < pool; ++j) {
        const float v = src[j * (kSgWin * NW)];
        if (v > best || (v != v && best == best)) { best = v; bi = j; }
      }
      const int64_t off = (v0 / pool) * p.o_is + (int64_t)w * p.o_ws + (int64_t)(col / p.ocg) * p.o_gs + col % p.ocg;
      orow0[off] = best > 0.f ? best : (best != best ? best : 0.f);
      if (irow0) irow0[off] = (uint8_t)bi;
    }
    return;
  }
  if (!live) return;
  // ---- epilogue (D: col = lane & 15, row = (lane >> 4) * 4 + reg): bias, column-group addressing, store
  float* orow0 = p.out + s * p.o_ss + iv * p.o_is;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int col = n0 + nt * 16 + r;
    if (col >= p.N) continue;
    const int64_t coff = (int64_t)(col / p.ocg) * p.o_gs + col % p.ocg;
    float b = 0.f;
    if (p.bias_kind == 1) b = p.bias[col];
    else if (p.bias_kind == 2) b = p.bias[iv * p.N + col];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int w = DILATED ? ph + (w0 + rt * 16 + kq * 4 + i) * p.dil : w0 + rt * 16 + kq * 4 + i;
        if (w < p.nwin) orow0[(int64_t)w * p.o_ws + coff] = acc[rt][nt][i] + b;
      }
  }
