// Counter-based sampling of zonotopes on the device: the plants [A | B] of Mdata and the disturbances of W that a Monte Carlo over
// the model set draws per trajectory (the sampling idea of reference tzddpc/utils.py:105-129, Mdata.sample(); there only for the
// gain).  A point is  centre + sum_i beta_i gen_i  with beta from Philox4x32-10, so the value of trajectory i (global index) at
// step t is a function of (seed, i, t) alone: every rank fills its own slice in place and the table does not depend on the sharding.
//
// Stream (include/tzddpc.h states it for callers; tzddpc_amd/montecarlo.py is the numpy statement the tests hold this against):
//   key (seed lo, seed hi), counter (i lo, i hi, t, stream * 2^24 + j), stream 0 plants / 1 noise, j the block index;
//   uniform: block j -> coefficients 2j (words 0, 1) and 2j + 1 (words 2, 3), k = (wa >> 5) 2^26 + (wb >> 6), beta = k 2^-52 - 1;
//   vertex:  block j -> coefficients 128 j .. 128 j + 127, coefficient i = bit i mod 32 of word (i mod 128) / 32, set: +1, clear: -1.
//
// One wave per item (a plant, or the disturbance of one step), four items per workgroup.  The coefficients of TZ_SP_CHUNK
// generators at a time are generated ONCE into the wave's LDS slice and then read by every output entry (LDS broadcast); lane e
// carries entries e, e + 64, ... in registers and reads row i of the generator table at [i * nout + e]: coalesced.  The sum runs in
// increasing i.
#pragma once
#include "tz_layout.h"

#define TZ_SP_CHUNK 512                       // coefficients per pass (multiple of 128: whole vertex blocks); 4 KB of LDS per wave
#define TZ_SP_ITEMS 4                         // waves (items) per workgroup
#define TZ_SP_MAXE ((TZ_NMAX * (TZ_NMAX + TZ_MMAX) + 63) / 64)      // output entries per lane: n (n + m) <= 384
#define TZ_SP_MAXGEN (1 << 24)                // the block index has 24 bits of the counter

enum { TZ_SP_UNIFORM = 0, TZ_SP_VERTEX = 1 };

struct SampleParams {
  unsigned key0, key1;
  unsigned long long first;                   // global index of item row 0
  int B, T;                                   // items: B x T (T = 1 for plants), item = b * T + t
  int nout, ngen, mode;
  unsigned stream;                            // 0 plants, 1 noise
  const double* centre;                       // nout
  const double* gen;                          // ngen x nout
  // entry e of item (b, t) goes to out0[b * s0 + t * st0 + e] when e < split (or split == 0), else out1[b * s1 + (e - split)] after
  // the row-wise split e = r * width + c -> c < wA: A[r * wA + c], else B[r * (width - wA) + c - wA]   (plants: [A | B])
  double* out0; size_t s0, st0;
  double* out1; size_t s1;
  int width, wA;                              // plants: width = n + m, wA = n; noise: width = 0 (no split)
};

__device__ inline void tz_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&o)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

__device__ inline double tz_sp_uniform(unsigned wa, unsigned wb) {
  const unsigned long long k = ((unsigned long long)(wa >> 5) << 26) | (unsigned long long)(wb >> 6);      // 53 bits
  return (double)k * 0x1p-52 - 1.0;                                                                      // [-1, 1), exact
}

__global__ __launch_bounds__(64 * TZ_SP_ITEMS) void tz_sample_kernel(SampleParams q) {
  __shared__ double beta_all[TZ_SP_ITEMS][TZ_SP_CHUNK];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double* beta = beta_all[wave];
  const unsigned long long item = (unsigned long long)blockIdx.x * TZ_SP_ITEMS + wave;
  const bool live = item < (unsigned long long)q.B * q.T;          // dead waves only keep the barriers company
  const int b = live ? (int)(item / q.T) : 0, t = live ? (int)(item % q.T) : 0;
  const unsigned long long gi = q.first + (unsigned long long)b;
  const unsigned c0 = (unsigned)gi, c1 = (unsigned)(gi >> 32), c2 = (unsigned)t, c3s = q.stream << 24;
  double acc[TZ_SP_MAXE];
#pragma unroll
  for (int k = 0; k < TZ_SP_MAXE; ++k) { const int e = lane + 64 * k; acc[k] = (e < q.nout) ? q.centre[e] : 0.0; }
  for (int g0 = 0; g0 < q.ngen; g0 += TZ_SP_CHUNK) {
    const int ng = min(TZ_SP_CHUNK, q.ngen - g0);
    __syncthreads();                                               // the previous pass has been read
    if (q.mode == TZ_SP_UNIFORM) {
      for (int jj = lane; 2 * jj < ng; jj += 64) {                 // block g0 / 2 + jj -> coefficients g0 + 2 jj, g0 + 2 jj + 1
        unsigned o[4];
        tz_philox4x32_10(c0, c1, c2, c3s + (unsigned)(g0 / 2 + jj), q.key0, q.key1, o);
        beta[2 * jj] = tz_sp_uniform(o[0], o[1]);
        if (2 * jj + 1 < ng) beta[2 * jj + 1] = tz_sp_uniform(o[2], o[3]);
      }
    } else {
      for (int jj = lane; 32 * jj < ng; jj += 64) {                // word jj of the pass: block g0 / 128 + jj / 4, word jj % 4 (4 lanes share a block)
        unsigned o[4];
        tz_philox4x32_10(c0, c1, c2, c3s + (unsigned)(g0 / 128 + jj / 4), q.key0, q.key1, o);
        const unsigned wsel = (jj & 3) == 0 ? o[0] : ((jj & 3) == 1 ? o[1] : ((jj & 3) == 2 ? o[2] : o[3]));
        for (int bit = 0; bit < 32 && 32 * jj + bit < ng; ++bit) beta[32 * jj + bit] = ((wsel >> bit) & 1u) ? 1.0 : -1.0;
      }
    }
    __syncthreads();
    const double* gr = q.gen + (size_t)g0 * q.nout;
    for (int i = 0; i < ng; ++i) {
      const double bi = beta[i];
#pragma unroll
      for (int k = 0; k < TZ_SP_MAXE; ++k) { const int e = lane + 64 * k; if (e < q.nout) acc[k] += bi * gr[(size_t)i * q.nout + e]; }
    }
  }
  if (!live) return;
#pragma unroll
  for (int k = 0; k < TZ_SP_MAXE; ++k) {
    const int e = lane + 64 * k;
    if (e >= q.nout) continue;
    if (q.width == 0) { q.out0[(size_t)b * q.s0 + (size_t)t * q.st0 + e] = acc[k]; continue; }
    const int r = e / q.width, c = e - r * q.width;
    if (c < q.wA) q.out0[(size_t)b * q.s0 + (size_t)r * q.wA + c] = acc[k];
    else q.out1[(size_t)b * q.s1 + (size_t)r * (q.width - q.wA) + (c - q.wA)] = acc[k];
  }
}
