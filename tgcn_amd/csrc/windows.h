// windows.h -- streaming time windows of MULTI-CHANNEL series (tgcn_cheb_project_series_f32 / tgcn_cheb_series_backward_f32)
// Part of the single translation unit tgcn_hip.hip (included once, inside its anonymous namespace).
#pragma once

// --------------------------------------------------------------------------------------------------
// sliding-window GEMM:  out[(s, i, w), col] = sum_term sum_{j < H*f} src_term[s, i, w - padl + j / f, j % f] * W[term][j][col]  (+ bias)
// --------------------------------------------------------------------------------------------------
// A series is addressed as src + term * src_ks + s * src_ss + i * src_is + t * src_ts + c with f contiguous channels per time row and
// zeros outside 0 <= t < Tin, so ONE kernel serves
//   the forward       (src = hop stack (K, S, n, T*f), padl = 0, nwin = T - H + 1 windows, columns = output channels) and
//   the input gradient (src = g read as a series of N channels over the windows, in either output layout, padl = H - 1, T "windows",
//                       one term, W = the time-flipped transposed weight, columns = (k, c) written into the (K, S, n, T*f) layout).
// Workgroup = 4 waves; wave v owns 32 consecutive windows of one vertex (two 16-row tiles of v_mfma_f32_16x16x4_f32 sharing their B
// fragments, layouts as in project.h) x NT*16 columns.  Per term (and per chunk of HC weight time rows when the span would not fit) the
// wave stages the (31 + HC) time rows its windows cover ONCE into its own LDS span -- 16-byte loads when VEC -- and feeds the A fragments
// from it at sliding offsets: window w, weight row (h, c) reads span row w + h, so a staged float serves up to HC windows.  The weight
// streams through one 32 x NT*16 LDS tile shared by the four waves.
// LDS banks: VEC spans keep f + 2 floats per time row (f % 4 == 0: (f + 2) / 2 is odd, the 16 windows x 2 k of a half wave fall into 32
// different banks); otherwise the span is the plain float sequence (window stride f).  Ws as in project_kernel.
struct SeriesGemmParams {
  const float* src;
  const float* W;       // (nterms, H*f, N) row-major
  const float* bias;    // bias_kind 1: [N]; 2: [n][N]
  float* out;
  int64_t src_ks, src_ss, src_is, src_ts;
  int64_t o_ss, o_is, o_ws, o_gs;   // output strides: recording, vertex, window, column group (column col lives at (col / ocg) * o_gs + col % ocg)
  int64_t n, ntiles;                // vertices per recording; wave tiles = S * n * tpv
  int64_t blk0;                     // the launch's first workgroup: a grid of 2^32 threads or more is issued in parts (kSeriesGridPart)
  int32_t Tin, padl, nwin, H, f, N, nterms, ocg, bias_kind, tpv, HC;
  int32_t stride, lst, fp;          // STRIDED only: window step in time rows, window distance in span rows, floats per span row
  int32_t dil, tpp;                 // DILATED only: time rows between two taps, tiles of 32 windows per phase
  const float* ring;                // CARRY only: the C = padl time rows before the chunk, (nterms, S, n, ring_ld), slot j at j * f
  int64_t ring_ks, ring_ss, ring_is;
  int32_t C, head;                  // CARRY only: slots of the ring, slot of its oldest row
  const int64_t* pos;               // CARRY only: non-null -> the slot of the oldest row is read from pos[0] in device memory (head is ignored)
  int32_t win_off;                  // STRIDED && CARRY only: the chunk row at which window 0 ends (window r ends at win_off + r * stride)
  uint8_t* idx;                     // POOLED only: arg-max byte per pooled output, in the layout of out; null: not stored
  int64_t nq;                       // POOLED only: vertex quads per recording, ceil(n / 4)
  int32_t pool;                     // POOLED only: 2 or 4 consecutive vertices per output vertex, n % pool == 0
};

constexpr int kSgWin = 32;    // windows per wave
constexpr int kSgKT = 32;     // weight rows per staged tile

// With a window step (STRIDED, stride >= 2) window r of the wave starts stride time rows after window r - 1.  The span keeps the rows that
// are READ: lst = min(stride, hc) span rows per window, span row r * lst + hh <-> time row t0 + r * stride + hh (hh < hc), so from
// stride >= hc on (no two windows of a chunk share a row) it holds the 32 windows back to back, 31 * hc + hc rows, and never the rows
// between them: a larger step costs no LDS and no loads beyond the no-overlap case.
// Bank rule: the 16 windows x 2 k of a half wave (ds_read_b32: 32 banks, lanes (r, kq) at r * D + kq, D = lst * row floats) are
// conflict-free exactly when D / 2 is odd.  VEC rows keep f + 2 floats for an odd lst (stride 1 included: today's layout) and f + 1 for
// an even one -- odd rows make D / 2 odd for lst = 2 (mod 4); they are staged with 4-byte stores instead of 8-byte ones.  Cost: one
// float per time row LESS than the odd case, and on the WRITE side four ds_write_b32 per staged float4 whose lanes sit 4 words apart
// (32 banks, 8 of them hit by a half wave: about 4-way conflicted) -- paid once per staged float, which the conflict-free reads then
// use about HC / lst times for each of the NT column tiles.  Residual: lst = 0 (mod 4) leaves D = 0 (mod 4) whatever the padding, 2^(e-1)-way for
// lst = 2^e * odd (lst 4: 2-way, 8: 4-way).  Scalar-load spans (f % 4 != 0) stay the plain float sequence, D = lst * f, unpadded as at step 1.
__host__ __device__ inline int series_span_lst(int hc, int stride) { return stride < hc ? stride : hc; }
__host__ __device__ inline int series_row_floats(int hc, int f, bool vec, int stride) {
  return !vec ? f : ((series_span_lst(hc, stride) & 1) ? f + 2 : f + 1);
}
// 64-bit: the host tries every hc <= H, and 32 * hc rows of f floats leave 32 bits for shapes the entries admit; what is launched fits the LDS
__host__ __device__ inline int64_t series_span_floats(int hc, int f, bool vec, int stride = 1) {
  const int64_t rows = (int64_t)(kSgWin - 1) * series_span_lst(hc, stride) + hc;
  return vec ? rows * series_row_floats(hc, f, vec, stride) : (rows * f + 4 + 3) / 4 * 4;
}
__host__ __device__ constexpr int series_ws_stride(int NT) { return (NT * 16) % 32 == 0 ? NT * 16 + 16 : NT * 16; }

// DILATED (taps dil >= 2 time rows apart, window step 1): window w reads the time rows w - padl + h * dil, so the windows of one phase
// q = w % dil, w = q + v * dil, are the UNDILATED step-1 windows v of the sub-series t = (q - padl) + u * dil.  A wave owns 32 consecutive
// windows v of one phase; tiles are phase-major inside a vertex: tile -> (recording * vertex, phase q < min(dil, nwin), block of 32
// inside the phase), tpv = min(dil, nwin) * tpp.  Span row tr <-> time row (q - padl) + (v0 + hc0 + tr) * dil -- the phase is taken from the window
// index, which is never negative, so the left padding needs no signed division -- and everything after the staging (span of 31 + HC rows,
// bank layout, sliding A offsets, regimes) is the step-1 kernel's.  Phase q holds ceil((nwin - q) / dil) windows: a wave whose block starts
// past its phase's last window stages zeros, reaches every barrier and writes nothing.
// CARRY (step 1, padl == C, DILATED or not): the src is one CHUNK of a longer series and the C time rows before it live in a ring buffer --
// slot j holds the row whose absolute index is j (mod C), head is the slot of the oldest.  Only the staging differs: a time row t < 0
// (t >= -C always: t0 >= -padl) is loaded from slot head + t + C (mod C; the sum lies in [0, 2C), one conditional subtraction) with the
// ring's own strides, a zeroed ring being the causal zero padding.  Span, banks, A offsets, regimes, tile decode and epilogue are untouched.
// head comes from the parameter struct, or -- p.pos non-null, the form a captured hipGraph step replays -- from device memory: one
// wave-uniform load per workgroup, before any store.  The host cannot check a device value without a synchronisation, so the loaded value is
// used only if 0 <= value < C and 0 is taken otherwise (one compare): whatever that memory holds, head + t + C stays in [0, 2C) and no ring
// access leaves the ring.  Only the source of head differs between the two forms.
// STRIDED && CARRY (a window step on a chunk): window r of the chunk ENDS at chunk row win_off + r * stride, 0 <= win_off < stride -- the
// phase of the chunk's first row in the recording -- so t0 gains win_off and, win_off being >= 0, t >= -C still holds.  The STRIDED staging
// already forms the time row t of every staged element; a row -C <= t < 0 takes the ring's slot head + t + C (mod C) as above.  lst, the
// row padding and its bank rule, the A offsets r * lst, the regimes and the epilogue are the STRIDED form's.
__device__ __forceinline__ int series_ring_head(const int64_t* pos, int head, int C) {
  if (!pos) return head;
  const int64_t v = pos[0];
  return (v >= 0 && v < (int64_t)C) ? (int)v : 0;
}
// POOLED (the forward with relu + max over `pool` consecutive vertices as its epilogue; pool 2 or 4, n % pool == 0): a workgroup owns ONE
// block of 32 windows (in the DILATED form: of one phase) of a vertex QUAD -- tile = blockIdx.x -> (recording, quad vq < nq = ceil(n / 4),
// block), wave v the vertex 4 * vq + v -- so a pool group lies inside one workgroup.  Staging, span, banks, regimes, A offsets and the MFMA
// loop are the form's own: every value acc + bias has the bits the unpooled kernel stores.  After the loop's last barrier the weight tile and
// the spans are free; each wave with a vertex writes its 32 x NT*16 values, bias added (kind 2: its own vertex's), into the scratch
// [wave][window][col] at the start of the LDS, ONE barrier, and the 256 threads walk (group, window, col), col fastest, taking the max by
// relu_pool_kernel's rules -- members ascending, first maximum wins, NaN propagates, then best > 0 ? best : (NaN ? NaN : 0) -- and store one
// float (and, idx non-null, one arg-max byte) at vertex iv / pool through the output strides.
// Barrier rule: the epilogue's barrier is reached by all four waves.  A wave without a vertex (the last quad of n = 2 (mod 4) at pool 2)
// stages zeros, writes no scratch, and stays; no group with a vertex reads its part (n % pool == 0: a group exists whole or not at all).
// Lanes of windows w >= nwin hold sums over zero rows; nothing reads them out.  A DILATED block that starts past its phase is dead for the
// four waves alike and leaves before the barrier, together.
// LDS: max(the GEMM's bytes, 4 * 32 * NT*16 floats <= 32 KB); the scratch never changes the regime (HC).
// DROP (series_gemm_pool_dropout_kernel: POOLED on a whole series; a kernel template of its own around the same body,
// windows_gemm_body.inc, so that the instantiations without dropout keep their names and their code): the value a wave writes into the
// scratch is t = relu(acc + bias) * m, m = keep ? scale : 0 by dropout.h's mask on the element e = ((s * nwin + w) * n + iv) * N + col,
// and the walk pools t by the same rules (its closing relu leaves t >= 0 and NaN as they are).
// The seed is one wave-uniform 8-byte load.  N % 4 == 0: the four lanes r = 4g .. 4g + 3 of a 16-lane row hold four consecutive columns of
// the windows kq * 4 + i, i < 4, which share the counter e >> 2 -- lane 4g + j runs Philox for window i = j only and the quad exchanges the
// words by DPP quad broadcasts (16 v_mov_dpp in place of three more Philox calls per four elements); the wave is whole there (live is
// wave-uniform).  Otherwise one Philox call per element.  No LDS beyond the scratch, no barrier beyond the epilogue's.
template <int I>
__device__ __forceinline__ uint32_t series_quad_bcast(uint32_t v) {      // lane I of each quad of four consecutive lanes, to the four
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, I * 0x55, 0xF, 0xF, true);
}
template <int NT, bool VEC, bool STRIDED = false, bool DILATED = false, bool CARRY = false, bool POOLED = false>
__global__ __launch_bounds__(kBlock) void series_gemm_kernel(const SeriesGemmParams p) {
#define TGCN_SERIES_GEMM_DROP 0
#include "windows_gemm_body.inc"
#undef TGCN_SERIES_GEMM_DROP
}
// the POOLED form of a whole series with dropout between relu and the pool
template <int NT, bool VEC, bool STRIDED, bool DILATED>
__global__ __launch_bounds__(kBlock) void series_gemm_pool_dropout_kernel(const SeriesGemmParams p, const DropoutParams dp) {
  constexpr bool CARRY = false, POOLED = true;
#define TGCN_SERIES_GEMM_DROP 1
#include "windows_gemm_body.inc"
#undef TGCN_SERIES_GEMM_DROP
}
// DROP on a CHUNK (series_gemm_chunk_pool_dropout_kernel: POOLED with the mask on one chunk of a longer series, behind the ring -- CARRY -- or,
// for a one-tap layer, without one; at step 1, DILATED or not): the chunk's window w is window at.w0 + w of the at.nwin windows of the whole
// series, and that is the window the mask counts: e = ((s * at.nwin + at.w0 + w) * n + iv) * N + col.  Nothing else differs from DROP, and
// only this template reads `at`, so every other instantiation keeps its parameters and its code.  e & 3 == col & 3 needs N % 4 == 0 only
// (the window term is a multiple of N), so the quad exchange holds whatever the base.
struct SeriesDropAt {
  int64_t w0, nwin;       // the chunk's first window in the whole series, and the whole series' windows
};
template <int NT, bool VEC, bool DILATED, bool CARRY>
__global__ __launch_bounds__(kBlock) void series_gemm_chunk_pool_dropout_kernel(const SeriesGemmParams p, const DropoutParams dp, const SeriesDropAt at) {
  constexpr bool STRIDED = false, POOLED = true;
#define TGCN_SERIES_GEMM_DROP 2
#include "windows_gemm_body.inc"
#undef TGCN_SERIES_GEMM_DROP
}

// Ring update of the CARRY form, after the projection: the m = min(Tc, C) newest time rows j0 .. j0 + m - 1 (j0 = Tc - m) of every (term,
// recording, vertex) row of the chunk's stack go to the slots (head + j) mod C of the ring's row; the host then moves head by Tc (mod C).
// A grid-stride copy in units U of the widest access f and the two alignments allow (16 bytes: float4 / 8 bf16; else one element); fu units
// per time row, leading dimensions in units.  The slots of one call are m <= C different ones and the source is the stack: in place, and
// values move unchanged in either dtype.  pos non-null: head is read from pos[0] by series_ring_head's rule (0 unless 0 <= pos[0] < C), so
// (head + j) mod C is a slot of the ring whatever that memory holds; the kernel never writes pos.
template <typename U>
__global__ __launch_bounds__(kBlock) void series_ring_update_kernel(const U* __restrict__ stack, U* __restrict__ ring, int64_t nrows, int64_t stack_ld,
                                                                    int64_t ring_ld, int fu, int j0, int m, int C, int head_arg,
                                                                    const int64_t* __restrict__ pos) {
  const int head = series_ring_head(pos, head_arg, C);
  const int64_t per_row = (int64_t)m * fu, total = nrows * per_row;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    const int64_t row = i / per_row;
    const int e = (int)(i - row * per_row);
    const int jj = e / fu, cu = e - jj * fu;
    const int j = j0 + jj;
    const int slot = (int)(((int64_t)head + j) % C);
    ring[row * ring_ld + (int64_t)slot * fu + cu] = stack[row * stack_ld + (int64_t)j * fu + cu];
  }
}

// The position {head, seen} of a ring kept in device memory moves by one chunk: head = (head + Tc) mod C from the value the two kernels above
// used (series_ring_head's rule), seen += Tc; C == 0 (a one-tap layer keeps no ring) leaves head at 0.  One thread, and a launch of its own
// behind the ring update on the same stream: every workgroup of the GEMM and of the update has read the old head before it moves.
__global__ void series_stream_advance_kernel(int64_t* __restrict__ pos, int Tc, int C) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int64_t head = series_ring_head(pos, 0, C);
  pos[0] = C > 0 ? (head + Tc) % C : 0;
  pos[1] += Tc;
}

// Wd[(h', nn), (k, c)] = W[k, H - 1 - h', c, nn]: the weight of the input gradient as a sliding-window GEMM over g.
// With a window step the input gradient is one such GEMM per phase ph = (t + pad_left) % stride over the weight time rows h = ph + m * stride,
// m < Hp = ceil((H - ph) / stride): the phases' weights lie one after the other, phase ph from row series_phase_row0(H, stride, ph) on,
//   Wd_ph[(h', nn), (k, c)] = W[k, ph + (Hp - 1 - h') * stride, c, nn]        (stride 1: the one phase, the line above)
__host__ __device__ inline int series_phase_rows(int H, int stride, int ph) { return ph < H ? (H - ph + stride - 1) / stride : 0; }
__host__ __device__ inline int series_phase_row0(int H, int stride, int ph) { return ph * (H / stride) + (ph < H % stride ? ph : H % stride); }   // ph <= stride

__global__ __launch_bounds__(kBlock) void series_flip_weight_kernel(const float* __restrict__ W, float* __restrict__ Wd, int K, int H, int f, int N,
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
// weight gradient: dW[k][j][nn] = sum_{s, i, w} stack[k, s, i, w*f + j] * g[(s, i, w), nn]         (j = h*f + c < H*f)
// --------------------------------------------------------------------------------------------------
// wgrad_partial_kernel's scheme on window rows: rows m = (s, i, w) in vertex-major order (consecutive rows are consecutive windows of one
// vertex, f floats apart, so the H-fold overlap is served by the caches), one wave per (row block, 64 columns of g, 16 rows j of the
// weight, group of kWgTerms terms), fp32 MFMA with k = 4 rows per instruction; g is addressed by strides, so either output layout is read
// in place.  Partials per row block, folded in block order by wgrad_reduce_kernel: deterministic.
// CONV (a window step and / or zero padding): row (s, i, w) starts at time row w * stride - padl, and weight row j = h*f + c contributes only
// where its OWN time row w * stride - padl + h lies inside 0 <= t < T -- the floats before and after a vertex's row are its neighbours'.
struct SeriesWgradParams {
  const float* stack;
  const float* g;
  float* partial;                 // [nblocks][K*J][N]
  int64_t st_ks, g_ss, g_is, g_ws;
  int64_t M, rows_per_block, n;
  int32_t Tf, f, nwin, J, N, K;
  int32_t stride, padl, T;        // CONV only
  int32_t dil;                    // DIL only
  const float* ring;              // CARRY only: the C = padl time rows before the chunk, (K, S, n, ring_ld), slot j at j * f
  int64_t ring_ks, ring_is;       // CARRY only: term and (recording, vertex) row strides of the ring
  int32_t C, head;                // CARRY only: slots of the ring, slot of its oldest row (the host's: this form is not captured)
};

// DIL (with CONV, step 1): weight row j = h*f + c of window w reads element (tw + h * dil) * f + c, tw = w - padl, where that time row exists.
// CARRY (with CONV, step 1, padl == C): the stack is one CHUNK of a longer series, T = nwin = Tc, and row (s, i, w) is the window that ENDS at
// chunk row w.  A lane's element lies at local time row t = w - C + h * dil, -C <= t <= w: t >= 0 reads the chunk's stack as above, t < 0 the
// ring's slot head + t + C (one conditional subtraction of C: the sum lies in [0, 2C)) with the ring's own term and row strides at channel
// c = j - h*f -- the staging rule of the CARRY GEMM; a zeroed ring is the causal padding, so every element exists.  g is addressed by the
// strides of the WHOLE gradient from the chunk's first row on (the host offsets p.g), in either layout.
template <bool CONV, bool DIL = false, bool CARRY = false>
__global__ __launch_bounds__(64) void series_wgrad_partial_kernel(const SeriesWgradParams p) {
  static_assert(!CARRY || CONV, "a carried chunk is a causal geometry");
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
  // (vertex row, window) of the block's first row once in 64 bits; rows inside the block by 32-bit arithmetic from there
  const int64_t si_lo = m_lo / p.nwin;
  const uint32_t w_lo = (uint32_t)(m_lo % p.nwin);
  const int64_t s_lo = si_lo / p.n;
  const uint32_t i_lo = (uint32_t)(si_lo % p.n);
  const uint32_t nwin = (uint32_t)p.nwin, nv = (uint32_t)p.n;
  const int hj = CONV ? j / p.f : 0;        // the weight time row of this lane's j
  const int hd = DIL ? hj * p.dil : hj;     // its distance from the window's first time row
  const int jd = DIL ? j + (hd - hj) * p.f : j;
  f32x4 acc[kWgTerms][4];
#pragma unroll
  for (int t = 0; t < kWgTerms; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[t][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t m0 = m_lo; m0 < m_hi; m0 += 4 * kWgUnroll) {
    float gv[kWgUnroll][4], av[kWgUnroll][kWgTerms];
#pragma unroll
    for (int u = 0; u < kWgUnroll; ++u) {
      const int64_t m = m0 + u * 4 + kq;
      const bool mok = m < m_hi;
      const uint32_t d = w_lo + (uint32_t)((mok ? m : m_lo) - m_lo);
      const uint32_t dv = d / nwin, w = d - dv * nwin;
      const uint32_t ii = i_lo + dv, ds = ii / nv, i = ii - ds * nv;
      const int64_t s = s_lo + ds;
      const float* grow = p.g + s * p.g_ss + (int64_t)i * p.g_is + (int64_t)w * p.g_ws;
      const int tw = CONV ? (int)w * p.stride - p.padl : (int)w;      // first time row of the window
      const float* arow = p.stack + (s * p.n + i) * (int64_t)p.Tf;
      const bool tok = !CONV || (tw + hd >= 0 && tw + hd < p.T) || (CARRY && tw + hd < 0);     // CARRY: -C <= tw + hd, a slot of the ring
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int nn = n0 + q * 16 + r;
        gv[u][q] = (mok && nn < p.N) ? grow[nn] : 0.f;
      }
      if constexpr (CARRY) {
        const float* ap = arow + (int64_t)tw * p.f + jd;      // the element in term 0, and the distance between two terms
        int64_t aks = p.st_ks;
        if (tw + hd < 0) {
          int slot = p.head + tw + hd + p.C;
          if (slot >= p.C) slot -= p.C;
          ap = p.ring + (s * p.n + i) * p.ring_is + (int64_t)slot * p.f + (j - hj * p.f);
          aks = p.ring_ks;
        }
#pragma unroll
        for (int t = 0; t < kWgTerms; ++t) av[u][t] = (mok && tok && j < p.J && t0 + t < p.K) ? ap[(int64_t)(t0 + t) * aks] : 0.f;
      } else {
#pragma unroll
        for (int t = 0; t < kWgTerms; ++t)
          av[u][t] = (mok && tok && j < p.J && t0 + t < p.K) ? arow[(int64_t)(t0 + t) * p.st_ks + (int64_t)tw * p.f + jd] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < kWgUnroll; ++u)
#pragma unroll
      for (int t = 0; t < kWgTerms; ++t) {
        if (t0 + t >= p.K) break;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[t][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][t], gv[u][q], acc[t][q], 0, 0, 0);
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
