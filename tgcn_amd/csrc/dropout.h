// dropout.h -- the counter-based dropout mask ("dropout in the relu + pool epilogue") and its stand-alone passes
// Part of the single translation unit tgcn_hip.hip (included once, inside its anonymous namespace).
#pragma once

// The mask is a pure function of (seed, element index e): Philox4x32-10 on the counter (lo32(e >> 2), hi32(e >> 2), 0, 0) under the key
// (lo32(seed), hi32(seed)); element e is KEPT iff output word e & 3 is >= thr.  e is 64-bit and counts the layer's output in the caller's
// vertex labels -- streaming layers ((s * nwin + w) * n + v) * N + c, batch layers (q * n + v) * N + c -- so it does not depend on the
// output layout, the tile or the operand's ordering, and no mask is ever stored: the tests restate it in numpy, the backward needs none
// (a positive pooled value was kept).
struct DropoutParams {
  const int64_t* seed;  // device memory, one element: read by the kernel, so a captured step draws a new mask on each replay
  uint32_t thr;         // min(floor(p * 2^32 + 0.5), 2^32 - 1)
  float scale;          // 1 / (1 - p) in fp32
};

inline bool dropout_scale_ok(float scale) { return isfinite(scale) && scale >= 1.f; }      // the entries' rule: 1 / (1 - p), 0 <= p < 1

__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
  // a rolled loop: the key schedule is wave-uniform, and unrolled the compiler keeps all twenty round keys in scalar registers -- enough
  // to spill some in the NT = 4 kernels; rolled it costs two scalar adds and a branch per round of fourteen vector operations
#pragma unroll 1
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four words that decide elements 4 * e4 .. 4 * e4 + 3
__host__ __device__ inline void dropout_words(uint64_t seed, uint64_t e4, uint32_t out[4]) {
  philox4x32_10((uint32_t)e4, (uint32_t)(e4 >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), out);
}
__host__ __device__ inline bool dropout_keep(uint64_t seed, uint64_t e, uint32_t thr) {
  uint32_t w[4];
  dropout_words(seed, e >> 2, w);
  const uint32_t sel = (uint32_t)e & 3u;
  return (sel == 0 ? w[0] : sel == 1 ? w[1] : sel == 2 ? w[2] : w[3]) >= thr;
}
// t = relu(y) * m, m = keep ? scale : 0: NaN stays NaN, a dropped +Inf becomes NaN (0 * Inf), as with torch's multiplicative dropout
__device__ __forceinline__ float relu_dropout(float y, bool keep, float scale) {
  const float r = y > 0.f ? y : (y != y ? y : 0.f);
  return r * (keep ? scale : 0.f);
}

// relu_pool_kernel with the mask: x (q, n, f) with f = nw * N columns per vertex row, column cc = window cc / N, channel cc % N, so element
// (row, v, cc) is e = ((row * nw + cc / N) * n + v) * N + cc % N -- (S*nwin, n, N) with nw = 1, the (S, n, nwin*N) series view, and the batch layers.
// The pool follows relu_pool_kernel's rules on the dropped values: members ascending, first maximum wins, NaN propagates.
__global__ __launch_bounds__(kBlock) void relu_dropout_pool_kernel(const float* __restrict__ x, float* __restrict__ out, uint8_t* __restrict__ idx,
                                                                   int64_t total, int64_t n, int f, int p, int N, const DropoutParams d) {
  const uint64_t seed = (uint64_t)d.seed[0];
  const int64_t nout = n / p;
  const int nw = f / N;
  for (int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x; o < total; o += (int64_t)gridDim.x * kBlock) {
    const int64_t row = o / f;            // (q row, output vertex) flattened
    const int cc = (int)(o % f);
    const int64_t qr = row / nout, v0 = (row - qr * nout) * p;
    const int w = cc / N, c = cc - w * N;
    const uint64_t e0 = (uint64_t)(((qr * nw + w) * n + v0) * N + c);
    const float* src = x + row * p * f + cc;
    float best = relu_dropout(src[0], dropout_keep(seed, e0, d.thr), d.scale);
    int bi = 0;
    for (int j = 1; j < p; ++j) {
      const float v = relu_dropout(src[(int64_t)j * f], dropout_keep(seed, e0 + (uint64_t)j * N, d.thr), d.scale);
      if (v > best || (v != v && best == best)) { best = v; bi = j; }
    }
    out[o] = best > 0.f ? best : (best != best ? best : 0.f);
    if (idx) idx[o] = (uint8_t)bi;
  }
}

// the keep byte of elements e0 .. e0 + count - 1: how a caller reproduces a mask
__global__ __launch_bounds__(kBlock) void dropout_keep_kernel(const int64_t* __restrict__ seed_ptr, uint64_t e0, int64_t count, uint32_t thr,
                                                              uint8_t* __restrict__ out) {
  const uint64_t seed = (uint64_t)seed_ptr[0];
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kBlock)
    out[i] = dropout_keep(seed, e0 + (uint64_t)i, thr) ? 1 : 0;
}
