// Photo smoothing: the guided filter of He, Sun and Tang (TPAMI 2013) on (h, w, 3) float images, the
// content as colour guide.  Windows are the (2r+1) x (2r+1) boxes clipped to the image, divided by their own pixel count.
// Two stages of the same shape, each a column pass and a row pass of DIRECT sums in float64 (no running sums: the rounding
// error of a window sum depends on the radius alone, never on the image):
//   stage 1  smooth_cols1_kernel   21 column sums per pixel of I, I I^T, p, I p^T (products exact in float64, one fused
//                                  multiply-add each) -> 21 float64 planes
//            smooth_rows_kernel<1> row sums of the planes through LDS, the means, Sigma = cov(I) + eps Id, its LDL^T solve
//                                  against the three cov(I, p_c), a (3 x 3) and b (3) rounded ONCE to 12 float32 planes
//   stage 2  smooth_cols2_kernel   12 column sums of a, b in float64 -> 12 float64 planes (over the first 12 of stage 1's)
//            smooth_rows_kernel<2> row sums, the means rounded to float32, q_c = b_c + a_c0 I_0 + a_c1 I_1 + a_c2 I_2
// No atomics, every sum in ascending order: the same bits on every run.  img is last read by smooth_cols1_kernel and out is
// first written by smooth_rows_kernel<2>, so out may be img; guide is read by that last kernel, so out may not be guide.
#include <math.h>

#include "internal.h"

namespace {

#define SMOOTH_S1 21                     // I (3), I_i I_j for i <= j (6), p (3), I_j p_c (9, c major)
#define SMOOTH_S2 12                     // a_cj (9, c major), b_c (3)
#define SMOOTH_COLS_X 64                 // column pass: 64 x 4 pixels per workgroup, one per thread
#define SMOOTH_COLS_Y 4
#define SMOOTH_ROW_THREADS 256           // row pass: 256 consecutive pixels of one row per workgroup
#define SMOOTH_ROW_SPAN (SMOOTH_ROW_THREADS + 2 * STROTSS_SMOOTH_MAX_RADIUS)
#define SMOOTH_ROW_CHUNK1 7              // planes staged in LDS at a time: 7 x 384 doubles = 21 KB
#define SMOOTH_ROW_CHUNK2 6              //                                 6 x 384 doubles = 18 KB
#define SMOOTH_MAX_GRID (1u << 14)       // workgroups of a launch at most; a workgroup walks the tiles beyond that number
#define SMOOTH_WS_PER_PIXEL (SMOOTH_S1 * sizeof(double) + SMOOTH_S2 * sizeof(float))

// The tiles of an image are numbered row-major and every grid is one-dimensional (an image may be taller than gridDim.y):
// workgroup b does the tiles b, b + gridDim.x, ... below the tile count (one each unless there are more than SMOOTH_MAX_GRID).
__host__ __device__ __forceinline__ unsigned cols_tiles(int h, int w) {
  return (((unsigned)w + SMOOTH_COLS_X - 1) / SMOOTH_COLS_X) * (((unsigned)h + SMOOTH_COLS_Y - 1) / SMOOTH_COLS_Y);
}
__host__ __device__ __forceinline__ unsigned rows_tiles(int h, int w) {
  return (((unsigned)w + SMOOTH_ROW_THREADS - 1) / SMOOTH_ROW_THREADS) * (unsigned)h;
}

// (x, y) of this thread's pixel in tile `tile` of the column passes
__device__ __forceinline__ bool cols_pixel(unsigned tile, int h, int w, int& x, int& y) {
  const unsigned ntx = ((unsigned)w + SMOOTH_COLS_X - 1) / SMOOTH_COLS_X;
  x = (int)(tile % ntx) * SMOOTH_COLS_X + (int)threadIdx.x;
  y = (int)(tile / ntx) * SMOOTH_COLS_Y + (int)threadIdx.y;
  return x < w && y < h;
}

__device__ __forceinline__ void cols1_tile(unsigned tile, const float* __restrict__ img, const float* __restrict__ guide,
                                           int h, int w, int r, double* __restrict__ planes) {
  int x, y;
  if (!cols_pixel(tile, h, w, x, y)) return;
  const int y0 = max(y - r, 0), y1 = min(y + r, h - 1);
  double s[SMOOTH_S1];
#pragma unroll
  for (int k = 0; k < SMOOTH_S1; ++k) s[k] = 0.0;
  for (int yy = y0; yy <= y1; ++yy) {
    const size_t at = 3 * ((size_t)yy * w + x);
    const double i0 = guide[at], i1 = guide[at + 1], i2 = guide[at + 2];
    const double p0 = img[at], p1 = img[at + 1], p2 = img[at + 2];
    s[0] += i0;
    s[1] += i1;
    s[2] += i2;
    s[3] = fma(i0, i0, s[3]);
    s[4] = fma(i0, i1, s[4]);
    s[5] = fma(i0, i2, s[5]);
    s[6] = fma(i1, i1, s[6]);
    s[7] = fma(i1, i2, s[7]);
    s[8] = fma(i2, i2, s[8]);
    s[9] += p0;
    s[10] += p1;
    s[11] += p2;
    s[12] = fma(i0, p0, s[12]);
    s[13] = fma(i1, p0, s[13]);
    s[14] = fma(i2, p0, s[14]);
    s[15] = fma(i0, p1, s[15]);
    s[16] = fma(i1, p1, s[16]);
    s[17] = fma(i2, p1, s[17]);
    s[18] = fma(i0, p2, s[18]);
    s[19] = fma(i1, p2, s[19]);
    s[20] = fma(i2, p2, s[20]);
  }
  const size_t npix = (size_t)h * w, at = (size_t)y * w + x;
#pragma unroll
  for (int k = 0; k < SMOOTH_S1; ++k) planes[k * npix + at] = s[k];
}

__global__ __launch_bounds__(SMOOTH_COLS_X* SMOOTH_COLS_Y) void smooth_cols1_kernel(const float* __restrict__ img,
                                                                                     const float* __restrict__ guide, int h,
                                                                                     int w, int r,
                                                                                     double* __restrict__ planes) {
  const unsigned ntiles = cols_tiles(h, w);
  for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) cols1_tile(tile, img, guide, h, w, r, planes);
}

__device__ __forceinline__ void cols2_tile(unsigned tile, const float* __restrict__ ab, int h, int w, int r,
                                           double* __restrict__ planes) {
  int x, y;
  if (!cols_pixel(tile, h, w, x, y)) return;
  const int y0 = max(y - r, 0), y1 = min(y + r, h - 1);
  const size_t npix = (size_t)h * w;
  double s[SMOOTH_S2];
#pragma unroll
  for (int k = 0; k < SMOOTH_S2; ++k) s[k] = 0.0;
  for (int yy = y0; yy <= y1; ++yy) {
    const size_t at = (size_t)yy * w + x;
#pragma unroll
    for (int k = 0; k < SMOOTH_S2; ++k) s[k] += (double)ab[k * npix + at];
  }
  const size_t at = (size_t)y * w + x;
#pragma unroll
  for (int k = 0; k < SMOOTH_S2; ++k) planes[k * npix + at] = s[k];
}

__global__ __launch_bounds__(SMOOTH_COLS_X* SMOOTH_COLS_Y) void smooth_cols2_kernel(const float* __restrict__ ab, int h, int w,
                                                                                     int r, double* __restrict__ planes) {
  const unsigned ntiles = cols_tiles(h, w);
  for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) cols2_tile(tile, ab, h, w, r, planes);
}

// a = Sigma^{-1} c for the symmetric positive definite Sigma = (s00 s01 s02; . s11 s12; . . s22) by its LDL^T factors,
// written out (elimination without pivoting is backward stable on such a matrix: every pivot is >= eps)
__device__ __forceinline__ void solve_spd3(double s00, double s01, double s02, double s11, double s12, double s22, double c0,
                                           double c1, double c2, double& a0, double& a1, double& a2) {
  const double l10 = s01 / s00, l20 = s02 / s00;
  const double d1 = s11 - l10 * s01;
  const double t12 = s12 - l20 * s01;
  const double l21 = t12 / d1;
  const double d2 = s22 - l20 * s02 - l21 * t12;
  const double z1 = c1 - l10 * c0;
  const double z2 = c2 - l20 * c0 - l21 * z1;
  a2 = z2 / d2;
  a1 = z1 / d1 - l21 * a2;
  a0 = c0 / s00 - l10 * a1 - l20 * a2;
}

// A tile is 256 consecutive pixels of a row, one per thread.  The row sums of NS planes over [x - r, x + r] clipped to the row, CHUNK
// planes at a time through LDS (the span of the workgroup's windows, at most 256 + 2 * 64 doubles per plane; lane t reads
// double t + const: conflict-free 8-byte reads), every sum in ascending x.  Then per pixel:
//   STAGE 1: the means over the N = n_x n_y pixels of the clipped window, Sigma, the three solves, b -> 12 float32 planes;
//   STAGE 2: the means rounded to float32 and the output pixel in float32.
template <int STAGE, int NS, int CHUNK>
__device__ __forceinline__ void rows_tile(unsigned tile, double (&span)[CHUNK][SMOOTH_ROW_SPAN],
                                          const double* __restrict__ planes, const float* __restrict__ guide, int h, int w,
                                          int r, double eps, float* __restrict__ dst) {
  static_assert(NS % CHUNK == 0, "whole chunks");
  const unsigned ntx = ((unsigned)w + SMOOTH_ROW_THREADS - 1) / SMOOTH_ROW_THREADS;
  const int y = (int)(tile / ntx);
  const int xb = (int)(tile % ntx) * SMOOTH_ROW_THREADS;
  const int x = xb + (int)threadIdx.x;
  const int xs = max(xb - r, 0);                                        // the span [xs, xe] of this workgroup's windows
  const int xe = min(xb + SMOOTH_ROW_THREADS - 1 + r, w - 1);
  const int lo = max(x - r, 0) - xs, hi = min(x + r, w - 1) - xs;       // this pixel's window inside the span (x < w)
  const size_t npix = (size_t)h * w, row = (size_t)y * w;
  double s[NS];
#pragma unroll
  for (int c = 0; c < NS / CHUNK; ++c) {
    __syncthreads();                                                    // the span of the chunk or tile before is read
#pragma unroll
    for (int k = 0; k < CHUNK; ++k)
      for (int i = (int)threadIdx.x; i <= xe - xs; i += SMOOTH_ROW_THREADS)
        span[k][i] = planes[(c * CHUNK + k) * npix + row + xs + i];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) s[c * CHUNK + k] = 0.0;
    if (x < w) {
      for (int i = lo; i <= hi; ++i) {
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) s[c * CHUNK + k] += span[k][i];
      }
    }
  }
  if (x >= w) return;
  const double n = (double)(hi - lo + 1) * (double)(min(y + r, h - 1) - max(y - r, 0) + 1);
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] /= n;
  const size_t at = row + x;
  if constexpr (STAGE == 1) {
    const double m0 = s[0], m1 = s[1], m2 = s[2];
    const double s00 = s[3] - m0 * m0 + eps, s01 = s[4] - m0 * m1, s02 = s[5] - m0 * m2;
    const double s11 = s[6] - m1 * m1 + eps, s12 = s[7] - m1 * m2, s22 = s[8] - m2 * m2 + eps;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double pb = s[9 + c];
      double a0, a1, a2;
      solve_spd3(s00, s01, s02, s11, s12, s22, s[12 + 3 * c] - m0 * pb, s[13 + 3 * c] - m1 * pb, s[14 + 3 * c] - m2 * pb, a0,
                 a1, a2);
      dst[(3 * c) * npix + at] = (float)a0;
      dst[(3 * c + 1) * npix + at] = (float)a1;
      dst[(3 * c + 2) * npix + at] = (float)a2;
      dst[(9 + c) * npix + at] = (float)(pb - (a0 * m0 + a1 * m1 + a2 * m2));
    }
  } else {
    const float i0 = guide[3 * at], i1 = guide[3 * at + 1], i2 = guide[3 * at + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      dst[3 * at + c] =
          fmaf((float)s[3 * c + 2], i2, fmaf((float)s[3 * c + 1], i1, fmaf((float)s[3 * c], i0, (float)s[9 + c])));
  }
}

template <int STAGE, int NS, int CHUNK>
__global__ __launch_bounds__(SMOOTH_ROW_THREADS) void smooth_rows_kernel(const double* __restrict__ planes,
                                                                         const float* __restrict__ guide, int h, int w, int r,
                                                                         double eps, float* __restrict__ dst) {
  __shared__ double span[CHUNK][SMOOTH_ROW_SPAN];
  const unsigned ntiles = rows_tiles(h, w);
  for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
    rows_tile<STAGE, NS, CHUNK>(tile, span, planes, guide, h, w, r, eps, dst);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool image_size_ok(int h, int w) { return h > 0 && w > 0 && 3LL * h * w <= 0x7fffffffLL; }
inline bool radius_ok(int r) { return r >= 1 && r <= STROTSS_SMOOTH_MAX_RADIUS; }

}  // namespace

size_t strotss_guided_smooth_workspace_bytes(int h, int w, int radius) {
  if (!image_size_ok(h, w) || !radius_ok(radius)) return 0;
  return SMOOTH_WS_PER_PIXEL * (size_t)h * (size_t)w;
}

int strotss_guided_smooth(const float* img, const float* guide, int h, int w, int radius, float eps, float* out,
                          void* workspace, size_t workspace_bytes, void* stream) {
  ST_CHECK_ARG(img && guide && out && workspace && image_size_ok(h, w) && radius_ok(radius), STROTSS_EINVAL);
  ST_CHECK_ARG(isfinite(eps) && eps >= 1e-4f && eps <= 1.0f, STROTSS_EINVAL);
  ST_CHECK_ARG(workspace_bytes >= strotss_guided_smooth_workspace_bytes(h, w, radius) && out != guide, STROTSS_EINVAL);
  ST_CHECK_ARG(aligned16(img) && aligned16(guide) && aligned16(out) && aligned16(workspace), STROTSS_EALIGN);
  const size_t npix = (size_t)h * w;
  double* planes = (double*)workspace;
  float* ab = (float*)(planes + SMOOTH_S1 * npix);
  hipStream_t st = (hipStream_t)stream;
  const dim3 cols_block(SMOOTH_COLS_X, SMOOTH_COLS_Y);
  // tile counts are below 2^31 for every 3 h w <= INT_MAX; a grid of at most 2^14 workgroups of 256 threads (eight times what
  // the device holds at once) is one that every such size can launch: one workgroup per tile would pass the 2^32 threads
  // of a launch on a narrow, very tall image
  const dim3 cols_grid(min(cols_tiles(h, w), SMOOTH_MAX_GRID));
  const dim3 rows_grid(min(rows_tiles(h, w), SMOOTH_MAX_GRID));
  hipLaunchKernelGGL(smooth_cols1_kernel, cols_grid, cols_block, 0, st, img, guide, h, w, radius, planes);
  hipLaunchKernelGGL((smooth_rows_kernel<1, SMOOTH_S1, SMOOTH_ROW_CHUNK1>), rows_grid, dim3(SMOOTH_ROW_THREADS), 0, st, planes,
                     guide, h, w, radius, (double)eps, ab);
  hipLaunchKernelGGL(smooth_cols2_kernel, cols_grid, cols_block, 0, st, ab, h, w, radius, planes);
  hipLaunchKernelGGL((smooth_rows_kernel<2, SMOOTH_S2, SMOOTH_ROW_CHUNK2>), rows_grid, dim3(SMOOTH_ROW_THREADS), 0, st, planes,
                     guide, h, w, radius, (double)eps, out);
  ST_LAUNCH_RET();
}
