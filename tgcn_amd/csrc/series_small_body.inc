// series_small_body.inc -- the body small_series_kernel and small_series_pool_kernel share (series_small.h), included once per kernel
// template like windows_gemm_body.inc: the text up to and including the last term's projection is the same tokens in both, so the kernels
// without a pool keep their code.  TGCN_SERIES_SMALL_POOL selects the epilogue: 0 bias + store of out, 1 bias, relu (+ dropout) and the
// max over POOL consecutive vertices in registers (the includer declares `pp`, POOL and DROP).
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
#if !TGCN_SERIES_SMALL_POOL
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
#else
  // ---- pooled epilogue (series_small.h, small_series_pool_kernel): the lane's f32x4 of a (slot, column tile) is the column `col` of the
  // vertices v0 .. v0 + 3, v0 = vt*16 + kq*4 a multiple of 4 -- 4 / POOL whole pool groups, so the max needs no other lane.
  // p.out is z, (S, n/POOL, nwin, N) as a series, else (S*nwin, n/POOL, N); pp.idx the arg-max bytes in the same layout, nullable.
  {
    SR_PIN4(n, N, nwin, TB); SR_PIN4(ntv, NV, wv, cg0); SR_PIN4(so, w0, tbw, wave);
    const int nout = n / POOL;
    float* zrec = p.out + (int64_t)so * (nout * nwin * N);
    uint8_t* irec = pp.idx ? pp.idx + (int64_t)so * (nout * nwin * N) : nullptr;
    const int vs = p.as_series ? nwin * N : N, ws = p.as_series ? N : nout * N;
    const uint64_t seed = DROP ? (uint64_t)pp.drop.seed[0] : 0;      // one wave-uniform 8-byte load
    const bool quad = (N & 3) == 0;      // cg0 and nl * 16 are multiples of 4: col & 3 == r & 3 == e & 3
    int vt = wv, tl = 0;
#pragma unroll
    for (int sl = 0; sl < NSLOT; ++sl) {
      asm volatile("" : "+s"(vt), "+s"(tl));
      if (vt < ntv && tl < tbw) {
        const int v0 = vt * 16 + kq * 4, w = w0 + tl;
#pragma unroll
        for (int nl = 0; nl < NTW; ++nl) {
          const int col = cg0 + nl * 16 + r;
          bool keep[4] = {true, true, true, true};
          if (DROP) {                                  // dropout.h's element index of vertex v0, in 64 bits; vertex v0 + i is i*N further
            const uint64_t e0 = (uint64_t)((((int64_t)so * nwin + w) * n + v0) * N + col);
            if (quad) {
              // N % 4 == 0: the lanes 4g .. 4g + 3 of a 16-lane row hold the columns col & ~3 .. + 3 of the same four vertices, and one
              // vertex's four columns share the counter e >> 2 (e & 3 == r & 3).  Lane 4g + j runs Philox for vertex j only and the
              // quad exchanges the words by DPP broadcasts, windows.h's series_quad_bcast with vertex i in window i's place.  Every
              // lane of the wave is here (the branches above are wave-uniform): a lane past N or past n computes on a number only.
              const int j = r & 3;
              uint32_t wd[4];
              dropout_words(seed, (e0 + (uint64_t)(j * N)) >> 2, wd);
              uint32_t x[4][4];                // x[i][k]: word k of vertex i's call -- all sixteen exchanged before any lane selects
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                x[0][k] = series_quad_bcast<0>(wd[k]); x[1][k] = series_quad_bcast<1>(wd[k]);
                x[2][k] = series_quad_bcast<2>(wd[k]); x[3][k] = series_quad_bcast<3>(wd[k]);
              }
#pragma unroll
              for (int i = 0; i < 4; ++i) keep[i] = (j == 0 ? x[i][0] : j == 1 ? x[i][1] : j == 2 ? x[i][2] : x[i][3]) >= pp.drop.thr;
            } else {                                   // the plain form: one Philox call per element
#pragma unroll
              for (int i = 0; i < 4; ++i) keep[i] = dropout_keep(seed, e0 + (uint64_t)(i * N), pp.drop.thr);
            }
          }
          if (col < N) {
#pragma unroll
            for (int g = 0; g < 4 / POOL; ++g) {
              const int vg = v0 + g * POOL;            // a group is whole or absent (n % POOL == 0): its first vertex decides
              if (vg < n) {
                float best = 0.f;
                int bi = 0;
#pragma unroll
                for (int j = 0; j < POOL; ++j) {       // members ascending, the first maximum wins, a NaN wins over a number
                  const int v = vg + j;
                  float b = 0.f;
                  if (p.bias_kind == 1) b = p.bias[col];
                  else if (p.bias_kind == 2) b = p.bias[(unsigned)(v * N + col)];
                  float t = acc[sl * NTW + nl][g * POOL + j] + b;
                  if (DROP) t = relu_dropout(t, keep[g * POOL + j], pp.drop.scale);
                  if (j == 0) best = t;
                  else if (t > best || (t != t && best == best)) { best = t; bi = j; }
                }
                const unsigned off = (unsigned)((vg / POOL) * vs + w * ws + col);
                zrec[off] = best > 0.f ? best : (best != best ? best : 0.f);
                if (irec) irec[off] = (uint8_t)bi;
              }
            }
          }
        }
      }
      if (++tl == TB) { tl = 0; vt += NV; }
    }
  }
#endif
#undef SR_PIN4
