// The sort-and-match core of the 1024-thread workgroups, shared by draw.hip (the index draw's final sort), sliced.hip and
// palette_sliced.hip (the sliced transports, DESIGN.md sections 21 and 25): ONE statement of the key packing, the bitonic
// network, the quantile-cell matching and the f64 block sum, so that the sorted order -- which decides every rank and every
// sign -- has the same bits in every caller.  Every function is called by ALL 1024 threads of the workgroup (blockDim.x ==
// 1024): each holds barriers.
//   ordered_pack / ordered_value   an order-preserving 32-bit key of a float above a row index: the 64-bit pairs compare as
//                                  (value, row), so equal values keep a total order and the sort is reproducible.
//   bitonic_sort_1024<SIDES>       ascending sort of 1024 pairs a side, one pair per thread and side IN REGISTERS: thread tid
//                                  ends with the tid-th smallest.  The 45 stages whose partner lies within the wave (j < 64)
//                                  exchange the two 32-bit halves by lane shuffles, no barrier.  The 10 cross-wave stages
//                                  (j >= 64) go through LDS, alternating between buf0 and buf1 so that ONE barrier a stage is
//                                  enough; side s uses slots [s * 1024, (s + 1) * 1024) of both (consecutive 8-byte slots,
//                                  partner tid ^ j: conflict-free).  Stages with k > S are skipped: S is a power of two in
//                                  [64, 1024], the same in every thread, and every slot >= S holds ~0 on every side.
//                                  The caller owns the LDS and guarantees
//                                    before: no thread still reads or writes buf0 -- a barrier lies between the last other use
//                                            of buf0 and the call (the first cross-wave stage writes it without one; buf1 is
//                                            first written behind that stage's barrier and may be live up to the call);
//                                    after:  the last cross-wave stage READS a buffer and no barrier follows it, so neither
//                                            buffer is written again before the workgroup's next barrier.
//   quantile_match<Cost>           the exact 1-D transport between n and ns uniform atoms, both sorted: thread tid < n walks
//                                  the cells [j/ns, (j+1)/ns] that overlap its own [tid/n, (tid+1)/n].  Side b's values go
//                                  to `sb` (>= 1024 floats that no thread still reads) behind one barrier.
//   block_sum_f64_1024             the 16 waves' f64 sum: a fixed shuffle tree a wave, the waves in ascending order.
#pragma once
#include "common.h"

namespace {

constexpr int SORT_T = 1024;            // threads of the workgroup = pairs a side

// -0 counts as +0, negative values sort below positive ones; the row index sits in the low word
__device__ __forceinline__ unsigned long long ordered_pack(float v, int idx) {
  unsigned b = __float_as_uint(v);
  if (b == 0x80000000u) b = 0u;
  const unsigned key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((unsigned long long)key << 32) | (unsigned)idx;
}
__device__ __forceinline__ float ordered_value(unsigned long long c) {
  const unsigned key = (unsigned)(c >> 32);
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

template <int SIDES>
__device__ __forceinline__ void bitonic_sort_1024(unsigned long long (&v)[SIDES], unsigned long long* buf0,
                                                  unsigned long long* buf1, int S) {
  const int tid = threadIdx.x;
  int cross = 0;                       // cross-wave stages so far, skipped ones included (they are the last): a constant a stage
#pragma unroll
  for (int k = 2; k <= SORT_T; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      unsigned long long* const buf = (cross & 1) ? buf1 : buf0;
      if (j >= 64) ++cross;
      if (k > S) continue;                               // uniform: every thread skips the stage and its barrier
      unsigned long long pv[SIDES];
      if (j < 64) {
#pragma unroll
        for (int s = 0; s < SIDES; ++s)
          pv[s] = ((unsigned long long)__shfl_xor((unsigned)(v[s] >> 32), j, 64) << 32) | __shfl_xor((unsigned)v[s], j, 64);
      } else {
#pragma unroll
        for (int s = 0; s < SIDES; ++s) buf[s * SORT_T + tid] = v[s];
        __syncthreads();
#pragma unroll
        for (int s = 0; s < SIDES; ++s) pv[s] = buf[s * SORT_T + (tid ^ j)];
      }
      const bool keep_low = ((tid & j) == 0) == ((tid & k) == 0);
#pragma unroll
      for (int s = 0; s < SIDES; ++s) v[s] = (v[s] < pv[s]) == keep_low ? v[s] : pv[s];
    }
  }
}

// Cost::pair(len, diff, g, w) adds one overlap of length len (a whole number of 1 / (n ns)) between a - b = diff to the
// coefficient g and the cost w.
struct SquaredCost {                    // W = sum len diff^2, dW/da / 2 = sum len diff
  static __device__ __forceinline__ void pair(float len, float diff, float& g, float& w) {
    g += len * diff;
    w += len * diff * diff;
  }
};
struct AbsoluteCost {                   // W = sum len |diff|, dW/da = sum len sign(diff): whole numbers, the sum is exact
  static __device__ __forceinline__ void pair(float len, float diff, float& g, float& w) {
    g += diff > 0.f ? len : (diff < 0.f ? -len : 0.f);
    w += len * fabsf(diff);
  }
};

struct QuantileMatch {
  float coef;                           // dW/da of the thread's element (tid < n), scaled by 1 / (n ns)
  int row;                              // the element's original row
  float cost;                           // the thread's share of W, scaled alike; 0 for tid >= n
};

// va, vb: the thread's sorted pairs of the two sides (n and ns atoms).
template <class Cost>
__device__ __forceinline__ QuantileMatch quantile_match(unsigned long long va, unsigned long long vb, int n, int ns,
                                                        float* sb) {
  const int tid = threadIdx.x;
  if (tid < ns) sb[tid] = ordered_value(vb);
  __syncthreads();
  QuantileMatch m = {0.f, 0, 0.f};
  if (tid < n) {
    // the overlap of the quantile cells [i/n, (i+1)/n] and [j/ns, (j+1)/ns], in units of 1 / (n ns): whole numbers
    const float a = ordered_value(va);
    const int lo = tid * ns, hi = lo + ns;
    float g = 0.f, w = 0.f;
    for (int j = lo / n; j < ns && j * n < hi; ++j) {
      const float len = (float)(min(hi, (j + 1) * n) - max(lo, j * n));
      const float diff = a - sb[j];
      Cost::pair(len, diff, g, w);
    }
    const float inv = (float)(1.0 / ((double)n * ns));
    m.coef = g * inv;
    m.row = (int)(unsigned)(va & 0xFFFFFFFFull);
    m.cost = w * inv;
  }
  return m;
}

// `red` holds >= 16 doubles that no thread still reads.  The sum is returned in thread 0 ONLY.
__device__ __forceinline__ double block_sum_f64_1024(double v, double* red) {
  const int tid = threadIdx.x;
  v = wave_sum(v);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < SORT_T / 64; ++i) s += red[i];
  }
  return s;
}

}  // namespace
