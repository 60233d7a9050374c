// Spherical k-means on sampled feature rows: the two kernels behind --auto_masks.  x is a zero-padded
// (rows, ld) float32 feature buffer as strotss_hypercol_gather writes it, inv_norm its reciprocal row norms
// (strotss_row_inv_norm), centres a (k, ld) float32 matrix of unit (or all-zero) rows, k <= STROTSS_KMEANS_MAX_K.
//   assign   kmeans_assign_kernel<KP, false> (kmeans_assign.h, shared with track.hip)  s_ij = (x_i . c_j) inv_norm_i in
//                                      float32; label = first arg-max, best, second.  x is read once, the centres stay in LDS
//                                      a 512-column chunk at a time.
//   update   kmeans_partial_kernel     per (row block, 256-column block): thread t owns column t, walks the rows of its block
//                                      in ascending order and adds x inv_norm (exact in float64) to acc[label][t] in LDS
//                                      (float64, 32 KB; a row's label is uniform, so lane t reads double t + const:
//                                      conflict-free) -> partial[row block][j][column]
//            kmeans_finish_kernel      one workgroup per centre: count[j]; per column the row blocks' partials summed in
//                                      ascending order, the norm by a fixed tree, c / |c| in float64, rounded once at the store
// No float atomics and no order that depends on scheduling: the same bits on every run and stream.  Memory-bound vector
// kernels (at most 16 centres: 8 flops per byte of x at k = 16, no MFMA shape to fill).
#include <math.h>

#include "kmeans_assign.h"

namespace {

#define KM_COLS 256                      // update: columns per workgroup, one per thread
#define KM_MAX_ROW_BLOCKS 32             // update: row blocks at most (the partials are row blocks x k x ld doubles)
#define KM_MIN_BLOCK_ROWS 64             // update: rows per row block at least

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
  sq = wave_sum(sq);
  if ((t & 63) == 0) red[t >> 6] = sq;
  __syncthreads();
  const double norm = sqrt((red[0] + red[1]) + (red[2] + red[3]));
  for (int c = t; c < ld; c += 256) centres[(size_t)j * ld + c] = (c < d && norm > 0.0) ? (float)(sum[c] / norm) : 0.f;
}

inline bool rows_ok(int n, int d, int ld) { return km_rows_ok(n, d, ld); }
inline bool k_ok(int k) { return km_k_ok(k); }
inline int row_blocks(int n) { return min(KM_MAX_ROW_BLOCKS, (n + KM_MIN_BLOCK_ROWS - 1) / KM_MIN_BLOCK_ROWS); }

}  // namespace

int strotss_kmeans_assign(const float* x, const float* inv_norm, int n, int d, int ld, const float* centres, int k, int* label,
                          float* best, float* second, void* stream) {
  ST_CHECK_ARG(x && inv_norm && centres && label && best && second && rows_ok(n, d, ld) && k_ok(k), STROTSS_EINVAL);
  ST_CHECK_ARG(ld % 32 == 0, STROTSS_EALIGN);
  ST_CHECK_ARG(aligned16(x) && aligned16(inv_norm) && aligned16(centres) && aligned16(label) && aligned16(best) &&
                   aligned16(second),
               STROTSS_EALIGN);
  km_launch_assign<false>(x, inv_norm, n, d, ld, centres, k, nullptr, 0.f, label, best, second, (hipStream_t)stream);
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
