// The assignment kernel of spherical k-means, shared by kmeans.hip (strotss_kmeans_assign) and track.hip
// (strotss_kmeans_assign_prior): ONE statement of the dot products, so that s_ij = (x_i . c_j) inv_norm_i
// has the same bits in both entries.
//   kmeans_assign_kernel<KP, PRIOR>  A tile is 32 rows of x, 4 per wave of a 512-thread workgroup: lane l holds columns
//                                    4l..4l+3 of each 256-column half of a 512-column chunk of its 4 rows and KP x 4 partial
//                                    scores; the chunk of the centres lives in LDS (KP x 512 floats, 32 KB at KP = 16: several
//                                    workgroups per CU; all 16 x 2208 floats = 138 KB would leave room for one) and is read once
//                                    per 4 rows of a wave.  x is read once; the centres come from L2 once per tile and chunk.
//                                    PRIOR = false: label = first arg-max of s, best, second (prior and beta are not read).
//                                    PRIOR = true: label = first arg-max of s_ij + (prior_i == j ? beta : 0), one float32 add;
//                                    best = the raw s of that j, second = the largest raw s of the other j.
//                                    SCORES = true (scribble.hip, strotss_kmeans_scores): all k values
//                                    s_ij go to scores[i k + j] (0 for a row with inv_norm_i == 0) instead of the best two;
//                                    label, best and second are not touched.
#pragma once
#include <math.h>

#include "internal.h"

namespace {

#define KM_ASSIGN_THREADS 512
#define KM_ROWS_PER_WAVE 4
#define KM_TILE_ROWS ((KM_ASSIGN_THREADS / WAVE) * KM_ROWS_PER_WAVE)       // 32
#define KM_CHUNK 512                     // columns of the centres in LDS at a time: two float4 per lane
#define KM_MAX_GRID 2048u                // workgroups of an assign launch at most; a workgroup walks the tiles beyond

template <int KP, bool PRIOR, bool SCORES = false>
__global__ __launch_bounds__(KM_ASSIGN_THREADS) void kmeans_assign_kernel(const float* __restrict__ x,
                                                                          const float* __restrict__ inv_norm, int n, int d,
                                                                          int ld, const float* __restrict__ centres, int k,
                                                                          const int* __restrict__ prior, float beta,
                                                                          int* __restrict__ label, float* __restrict__ best,
                                                                          float* __restrict__ second,
                                                                          float* __restrict__ scores) {
  __shared__ __attribute__((aligned(16))) float cs[KP][KM_CHUNK];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const unsigned ntiles = ((unsigned)n + KM_TILE_ROWS - 1) / KM_TILE_ROWS;
  for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int row0 = (int)tile * KM_TILE_ROWS + wave * KM_ROWS_PER_WAVE;
    float acc[KM_ROWS_PER_WAVE][KP];
#pragma unroll
    for (int q = 0; q < KM_ROWS_PER_WAVE; ++q)
#pragma unroll
      for (int j = 0; j < KP; ++j) acc[q][j] = 0.f;
    for (int c0 = 0; c0 < d; c0 += KM_CHUNK) {
      __syncthreads();                                                  // the chunk (or tile) before is read
      for (int i = (int)threadIdx.x; i < KP * (KM_CHUNK / 4); i += KM_ASSIGN_THREADS) {
        const int j = i / (KM_CHUNK / 4), c = c0 + (i % (KM_CHUNK / 4)) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (j < k && c < ld) {                                          // ld % 4 == 0: a float4 is inside ld or outside
          v = *reinterpret_cast<const f32x4*>(centres + (size_t)j * ld + c);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c + e >= d) v[e] = 0.f;                                 // the sum runs over the d columns
        }
        *reinterpret_cast<f32x4*>(&cs[j][(i % (KM_CHUNK / 4)) * 4]) = v;
      }
      __syncthreads();
#pragma unroll
      for (int half = 0; half < KM_CHUNK / 256; ++half) {
        const int col = half * 256 + lane * 4;
        if (c0 + col >= d) continue;
        f32x4 xv[KM_ROWS_PER_WAVE];
#pragma unroll
        for (int q = 0; q < KM_ROWS_PER_WAVE; ++q) {
          xv[q] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (row0 + q < n) xv[q] = *reinterpret_cast<const f32x4*>(x + (size_t)(row0 + q) * ld + c0 + col);
        }
#pragma unroll
        for (int j = 0; j < KP; ++j) {
          const f32x4 cv = *reinterpret_cast<const f32x4*>(&cs[j][col]);
#pragma unroll
          for (int q = 0; q < KM_ROWS_PER_WAVE; ++q)
            acc[q][j] += xv[q][0] * cv[0] + xv[q][1] * cv[1] + xv[q][2] * cv[2] + xv[q][3] * cv[3];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < KM_ROWS_PER_WAVE; ++q)
#pragma unroll
      for (int j = 0; j < KP; ++j) acc[q][j] = wave_sum(acc[q][j]);
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < KM_ROWS_PER_WAVE; ++q) {
        const int row = row0 + q;
        if (row >= n) continue;
        const float inv = inv_norm[row];
        if constexpr (SCORES) {
#pragma unroll
          for (int j = 0; j < KP; ++j)
            if (j < k) scores[(size_t)row * k + j] = inv != 0.f ? acc[q][j] * inv : 0.f;
          continue;
        }
        int bj = 0;
        float b = 0.f, s2 = 0.f;
        if constexpr (!PRIOR) {
          if (inv != 0.f) {
            b = -INFINITY;
            s2 = -INFINITY;
#pragma unroll
            for (int j = 0; j < KP; ++j) {
              if (j >= k) continue;
              const float s = acc[q][j] * inv;
              if (s > b) {                                              // strictly: the lowest j wins on equal values
                s2 = b;
                b = s;
                bj = j;
              } else if (s > s2) {
                s2 = s;
              }
            }
          }
        } else {
          const int p = prior[row];                                     // compared with j < k only, never an index
          if (inv != 0.f) {
            float top = -INFINITY, m1 = -INFINITY, m2 = -INFINITY;      // the best biased score; the two largest raw s
            int i1 = 0;
#pragma unroll
            for (int j = 0; j < KP; ++j) {
              if (j >= k) continue;
              const float s = acc[q][j] * inv;
              const float score = s + (j == p ? beta : 0.f);
              if (score > top) {                                        // strictly: the lowest j wins on equal scores
                top = score;
                b = s;
                bj = j;
              }
              if (s > m1) {
                m2 = m1;
                m1 = s;
                i1 = j;
              } else if (s > m2) {
                m2 = s;
              }
            }
            s2 = bj == i1 ? m2 : m1;                                    // the largest raw s of the others
          } else if (beta > 0.f && (unsigned)p < (unsigned)k) {
            bj = p;                                                     // every s is 0: the prior's beta decides
          }
        }
        label[row] = bj;
        best[row] = b;
        second[row] = s2;
      }
    }
  }
}

inline bool km_rows_ok(int n, int d, int ld) { return n > 0 && d > 0 && d <= ld && (long long)n * ld <= 0x7fffffffLL; }
inline bool km_k_ok(int k) { return k >= 1 && k <= STROTSS_KMEANS_MAX_K; }

// One launch on st; the arguments are checked by the entry.  PRIOR = false: prior may be NULL, beta is ignored.
template <bool PRIOR>
inline void km_launch_assign(const float* x, const float* inv_norm, int n, int d, int ld, const float* centres, int k,
                             const int* prior, float beta, int* label, float* best, float* second, hipStream_t st) {
  const unsigned ntiles = ((unsigned)n + KM_TILE_ROWS - 1) / KM_TILE_ROWS;
  const dim3 grid(min(ntiles, KM_MAX_GRID)), block(KM_ASSIGN_THREADS);
#define KM_LAUNCH(KP)                                                                                                        \
  hipLaunchKernelGGL((kmeans_assign_kernel<KP, PRIOR>), grid, block, 0, st, x, inv_norm, n, d, ld, centres, k, prior, beta, \
                     label, best, second, (float*)nullptr)
  if (k <= 4)
    KM_LAUNCH(4);
  else if (k <= 8)
    KM_LAUNCH(8);
  else
    KM_LAUNCH(16);
#undef KM_LAUNCH
}

// The same launch with SCORES = true: scores is (n, k) float32.
inline void km_launch_scores(const float* x, const float* inv_norm, int n, int d, int ld, const float* centres, int k,
                             float* scores, hipStream_t st) {
  const unsigned ntiles = ((unsigned)n + KM_TILE_ROWS - 1) / KM_TILE_ROWS;
  const dim3 grid(min(ntiles, KM_MAX_GRID)), block(KM_ASSIGN_THREADS);
#define KM_LAUNCH(KP)                                                                                                        \
  hipLaunchKernelGGL((kmeans_assign_kernel<KP, false, true>), grid, block, 0, st, x, inv_norm, n, d, ld, centres, k,        \
                     (const int*)nullptr, 0.f, (int*)nullptr, (float*)nullptr, (float*)nullptr, scores)
  if (k <= 4)
    KM_LAUNCH(4);
  else if (k <= 8)
    KM_LAUNCH(8);
  else
    KM_LAUNCH(16);
#undef KM_LAUNCH
}

}  // namespace
