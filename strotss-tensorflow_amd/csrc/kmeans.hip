// Spherical k-means on sampled feature rows: the two kernels behind --auto_masks.  x is a zero-padded
// (rows, ld) float32 feature buffer as strotss_hypercol_gather writes it, inv_norm its reciprocal row norms
// (strotss_row_inv_norm), centres a (k, ld) float32 matrix of unit (or all-zero) rows, k <= STROTSS_KMEANS_MAX_K.
//   assign   kmeans_assign_kernel<KP>  s_ij = (x_i . c_j) inv_norm_i in float32; label = first arg-max, best, second.  A tile
//                                      is 32 rows of x, 4 per wave of a 512-thread workgroup: lane l holds columns 4l..4l+3 of
//                                      each 256-column half of a 512-column chunk of its 4 rows and KP x 4 partial scores; the
//                                      chunk of the centres lives in LDS (KP x 512 floats, 32 KB at KP = 16: several workgroups
//                                      per CU; all 16 x 2208 floats = 138 KB would leave room for one) and is read once per
//                                      4 rows of a wave.  x is read once; the centres come from L2 once per tile and chunk.
//   update   kmeans_partial_kernel     per (row block, 256-column block): thread t owns column t, walks the rows of its block
//                                      in ascending order and adds x inv_norm (exact in float64) to acc[label][t] in LDS
//                                      (float64, 32 KB; a row's label is uniform, so lane t reads double t + const:
//                                      conflict-free) -> partial[row block][j][column]
//            kmeans_finish_kernel      one workgroup per centre: count[j]; per column the row blocks' partials summed in
//                                      ascending order, the norm by a fixed tree, c / |c| in float64, rounded once at the store
// No float atomics and no order that depends on scheduling: the same bits on every run and stream.  Memory-bound vector
// kernels (at most 16 centres: 8 flops per byte of x at k = 16, no MFMA shape to fill).
#include <math.h>

#include "internal.h"

namespace {

#define KM_ASSIGN_THREADS 512
#define KM_ROWS_PER_WAVE 4
#define KM_TILE_ROWS ((KM_ASSIGN_THREADS / WAVE) * KM_ROWS_PER_WAVE)       // 32
#define KM_CHUNK 512                     // columns of the centres in LDS at a time: two float4 per lane
#define KM_MAX_GRID 2048u                // workgroups of an assign launch at most; a workgroup walks the tiles beyond
#define KM_COLS 256                      // update: columns per workgroup, one per thread
#define KM_MAX_ROW_BLOCKS 32             // update: row blocks at most (the partials are row blocks x k x ld doubles)
#define KM_MIN_BLOCK_ROWS 64             // update: rows per row block at least

template <int KP>
__global__ __launch_bounds__(KM_ASSIGN_THREADS) void kmeans_assign_kernel(const float* __restrict__ x,
                                                                          const float* __restrict__ inv_norm, int n, int d,
                                                                          int ld, const float* __restrict__ centres, int k,
                                                                          int* __restrict__ label, float* __restrict__ best,
                                                                          float* __restrict__ second) {
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
        int bj = 0;
        float b = 0.f, s2 = 0.f;
        if (inv != 0.f) {
          b = -INFINITY;
          s2 = -INFINITY;
#pragma unroll
          for (int j = 0; j < KP; ++j) {
            if (j >= k) continue;
            const float s = acc[q][j] * inv;
            if (s > b) {                                                // strictly: the lowest j wins on equal values
              s2 = b;
              b = s;
              bj = j;
            } else if (s > s2) {
              s2 = s;
            }
          }
        }
        label[row] = bj;
        best[row] = b;
        second[row] = s2;
      }
    }
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(KM_COLS) void kmeans_partial_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ inv_norm,
                                                                 const int* __restrict__ label, int n, int d, int ld, int k,
                                                                 int block_rows, double* __restrict__ partial) {
  __shared__ double acc[STROTSS_KMEANS_MAX_K][KM_COLS];
  const int t = (int)threadIdx.x, c = (int)blockIdx.x * KM_COLS + t;
  if (c >= d) return;                                                   // no barrier below: a thread touches its own column only
  for (int j = 0; j < k; ++j) acc[j][t] = 0.0;
  const int r0 = (int)blockIdx.y * block_rows, r1 = min(n, r0 + block_rows);
#pragma unroll 4
  for (int r = r0; r < r1; ++r) {
    const int l = label[r];
    const double v = (double)x[(size_t)r * ld + c], w = (double)inv_norm[r];
    if ((unsigned)l < (unsigned)k) acc[l][t] = fma(v, w, acc[l][t]);    // v w is exact in float64: one rounding, the sum's
  }
  for (int j = 0; j < k; ++j) partial[((size_t)blockIdx.y * k + j) * ld + c] = acc[j][t];
}

__global__ __launch_bounds__(256) void kmeans_finish_kernel(const int* __restrict__ label, int n, int d, int ld, int k,
                                                            int row_blocks, double* partial,
                                                            float* __restrict__ centres, int* __restrict__ count) {
  __shared__ double red[4];
  __shared__ int redi[4];
  const int j = (int)blockIdx.x, t = (int)threadIdx.x;
  int cnt = 0;
  for (int i = t; i < n; i += 256) cnt += label[i] == j;
  cnt = wave_sum_i32(cnt);
  if ((t & 63) == 0) redi[t >> 6] = cnt;
  __syncthreads();
  cnt = (redi[0] + redi[1]) + (redi[2] + redi[3]);
  if (t == 0) count[j] = cnt;
  if (cnt == 0) return;                                                 // an empty cluster keeps its centre bit for bit
  double* sum = partial + (size_t)j * ld;                               // row block 0's slice of centre j receives the totals
  double sq = 0.0;
  for (int c = t; c < d; c += 256) {
    double s = 0.0;
    for (int b = 0; b < row_blocks; ++b) s += partial[((size_t)b * k + j) * ld + c];
    sum[c] = s;                                                         // read back below by this thread only
    sq = fma(s, s, sq);
  }
  sq = wave_sum_f64(sq);
  if ((t & 63) == 0) red[t >> 6] = sq;
  __syncthreads();
  const double norm = sqrt((red[0] + red[1]) + (red[2] + red[3]));
  for (int c = t; c < ld; c += 256) centres[(size_t)j * ld + c] = (c < d && norm > 0.0) ? (float)(sum[c] / norm) : 0.f;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool rows_ok(int n, int d, int ld) { return n > 0 && d > 0 && d <= ld && (long long)n * ld <= 0x7fffffffLL; }
inline bool k_ok(int k) { return k >= 1 && k <= STROTSS_KMEANS_MAX_K; }
inline int row_blocks(int n) { return min(KM_MAX_ROW_BLOCKS, (n + KM_MIN_BLOCK_ROWS - 1) / KM_MIN_BLOCK_ROWS); }

}  // namespace

int strotss_kmeans_assign(const float* x, const float* inv_norm, int n, int d, int ld, const float* centres, int k, int* label,
                          float* best, float* second, void* stream) {
  ST_CHECK_ARG(x && inv_norm && centres && label && best && second && rows_ok(n, d, ld) && k_ok(k), STROTSS_EINVAL);
  ST_CHECK_ARG(ld % 32 == 0, STROTSS_EALIGN);
  ST_CHECK_ARG(aligned16(x) && aligned16(inv_norm) && aligned16(centres) && aligned16(label) && aligned16(best) &&
                   aligned16(second),
               STROTSS_EALIGN);
  hipStream_t st = (hipStream_t)stream;
  const unsigned ntiles = ((unsigned)n + KM_TILE_ROWS - 1) / KM_TILE_ROWS;
  const dim3 grid(min(ntiles, KM_MAX_GRID)), block(KM_ASSIGN_THREADS);
  if (k <= 4)
    hipLaunchKernelGGL(kmeans_assign_kernel<4>, grid, block, 0, st, x, inv_norm, n, d, ld, centres, k, label, best, second);
  else if (k <= 8)
    hipLaunchKernelGGL(kmeans_assign_kernel<8>, grid, block, 0, st, x, inv_norm, n, d, ld, centres, k, label, best, second);
  else
    hipLaunchKernelGGL(kmeans_assign_kernel<16>, grid, block, 0, st, x, inv_norm, n, d, ld, centres, k, label, best, second);
  ST_LAUNCH_RET();
}

size_t strotss_kmeans_update_workspace_bytes(int n, int ld, int k) {
  if (!rows_ok(n, 1, ld) || ld % 32 != 0 || !k_ok(k)) return 0;
  return (size_t)row_blocks(n) * (size_t)k * (size_t)ld * sizeof(double);
}

int strotss_kmeans_update(const float* x, const float* inv_norm, const int* label, int n, int d, int ld, int k, float* centres,
                          int* count, void* workspace, size_t workspace_bytes, void* stream) {
  ST_CHECK_ARG(x && inv_norm && label && centres && count && workspace && rows_ok(n, d, ld) && k_ok(k), STROTSS_EINVAL);
  ST_CHECK_ARG(ld % 32 == 0, STROTSS_EALIGN);
  ST_CHECK_ARG(workspace_bytes >= strotss_kmeans_update_workspace_bytes(n, ld, k), STROTSS_EINVAL);
  ST_CHECK_ARG(aligned16(x) && aligned16(inv_norm) && aligned16(label) && aligned16(centres) && aligned16(count) &&
                   aligned16(workspace),
               STROTSS_EALIGN);
  hipStream_t st = (hipStream_t)stream;
  const int nb = row_blocks(n), block_rows = (n + nb - 1) / nb;
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(kmeans_partial_kernel, dim3((d + KM_COLS - 1) / KM_COLS, nb), dim3(KM_COLS), 0, st, x, inv_norm, label, n,
                     d, ld, k, block_rows, partial);
  hipLaunchKernelGGL(kmeans_finish_kernel, dim3(k), dim3(256), 0, st, label, n, d, ld, k, nb, partial, centres, count);
  ST_LAUNCH_RET();
}
