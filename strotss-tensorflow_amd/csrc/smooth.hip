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
//
// Guided upsampling (He and Sun's fast guided filter turned round): the same stage 1 and the same
// column pass of stage 2, then
//            smooth_rows_store_kernel    row sums, the twelve means rounded to float32 and d = p - q (q by stage 2's fma
//                                        chain) as ONE 16-float record per pixel (a 9, b 3, d 3, a zero)
//            upsample_apply_kernel<MODE> one pass over the (H, W) image: the records interpolated with the taps and the
//                                        arithmetic of strotss_resize_bilinear, applied to the full-resolution guide
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
#define UPS_RECORD 16                    // floats of a low-resolution record: a_cj (9, c major), b_c (3), d_c (3), one zero
#define UPS_THREADS 256                  // apply pass: a tile is 1024 consecutive pixels of the flat (H W) image,
#define UPS_PIXELS 4                     //   four consecutive ones per thread (three float4): 768 aligned float4 per tile
#define UPS_TILE (UPS_THREADS * UPS_PIXELS)
#define UPS_MAX_GRID (1u << 12)          // workgroups of the apply launch at most (the device holds 1280 at five per CU)

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
//   STAGE 2: the means rounded to float32 and the output pixel in float32;
//   STAGE 3: stage 2's means and its pixel q, stored as the record (means, img - q, 0) instead of q (guided upsampling).
template <int STAGE, int NS, int CHUNK>
__device__ __forceinline__ void rows_tile(unsigned tile, double (&span)[CHUNK][SMOOTH_ROW_SPAN],
                                          const double* __restrict__ planes, const float* __restrict__ guide, int h, int w,
                                          int r, double eps, float* __restrict__ dst,
                                          const float* __restrict__ img = nullptr) {
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
  } else if constexpr (STAGE == 2) {
    const float i0 = guide[3 * at], i1 = guide[3 * at + 1], i2 = guide[3 * at + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      dst[3 * at + c] =
          fmaf((float)s[3 * c + 2], i2, fmaf((float)s[3 * c + 1], i1, fmaf((float)s[3 * c], i0, (float)s[9 + c])));
  } else {
    const float i0 = guide[3 * at], i1 = guide[3 * at + 1], i2 = guide[3 * at + 2];
    float rec[UPS_RECORD];
#pragma unroll
    for (int k = 0; k < SMOOTH_S2; ++k) rec[k] = (float)s[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float q = fmaf(rec[3 * c + 2], i2, fmaf(rec[3 * c + 1], i1, fmaf(rec[3 * c], i0, rec[9 + c])));
      rec[SMOOTH_S2 + c] = __fsub_rn(img[3 * at + c], q);
    }
    rec[UPS_RECORD - 1] = 0.0f;
    float4* to = (float4*)dst + (UPS_RECORD / 4) * at;                  // dst is 16-byte aligned, a record is 64 bytes
#pragma unroll
    for (int k = 0; k < UPS_RECORD / 4; ++k) to[k] = make_float4(rec[4 * k], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3]);
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

__global__ __launch_bounds__(SMOOTH_ROW_THREADS) void smooth_rows_store_kernel(const double* __restrict__ planes,
                                                                               const float* __restrict__ img,
                                                                               const float* __restrict__ guide, int h, int w,
                                                                               int r, float* __restrict__ records) {
  __shared__ double span[SMOOTH_ROW_CHUNK2][SMOOTH_ROW_SPAN];
  const unsigned ntiles = rows_tiles(h, w);
  for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
    rows_tile<3, SMOOTH_S2, SMOOTH_ROW_CHUNK2>(tile, span, planes, guide, h, w, r, 0.0, records, img);
}

// The taps of strotss_resize_bilinear (image.hip: axis_tap), restated: half-pixel centres, the source coordinate in float32
// without contraction, clamped indices.
struct UpsTap { int lo, hi; float lerp; };
__device__ __forceinline__ UpsTap ups_tap(int i, float scale, int in_size) {
  const float src = __fsub_rn(__fmul_rn(__fadd_rn((float)i, 0.5f), scale), 0.5f);
  const float fl = floorf(src);
  UpsTap t;
  t.lo = min(max((int)fl, 0), in_size - 1);                             // the upper clamp never binds for out >= in sizes
  t.hi = max(min((int)ceilf(src), in_size - 1), 0);                     // nor does the lower one
  t.lerp = __fsub_rn(src, fl);
  return t;
}

// a + (b - a) t, the difference rounded and one fused multiply-add: what `a + (b - a) * t` of the resize kernel compiles to.
// t == 0 returns a.
__device__ __forceinline__ float ups_lerp(float a, float b, float t) { return fmaf(__fsub_rn(b, a), t, a); }
// along x in both rows first, then along y
__device__ __forceinline__ float ups_bilerp(float tl, float tr, float bl, float br, float lx, float ly) {
  return ups_lerp(ups_lerp(tl, tr, lx), ups_lerp(bl, br, lx), ly);
}
__device__ __forceinline__ float4 ups_bilerp4(float4 tl, float4 tr, float4 bl, float4 br, float lx, float ly) {
  return make_float4(ups_bilerp(tl.x, tr.x, bl.x, br.x, lx, ly), ups_bilerp(tl.y, tr.y, bl.y, br.y, lx, ly),
                     ups_bilerp(tl.z, tr.z, bl.z, br.z, lx, ly), ups_bilerp(tl.w, tr.w, bl.w, br.w, lx, ly));
}

// One tile: 1024 consecutive pixels of the flat image = 3072 floats = 768 float4, whatever W is (the image starts 16-byte
// aligned and a tile is 12288 bytes, so every float4 is aligned; a 12-byte pixel never is).  The guide goes through LDS:
// thread t loads float4 t, t + 256, t + 512 (whole cache lines per wave), then owns the four consecutive pixels 4 t .. 4 t + 3
// of the tile (twelve floats = three float4 LDS reads at a 48-byte lane stride), overwrites each with its result, and the
// tile leaves as it came.  The four records of a pixel's taps are read through the cache, four float4 each (three without
// d), and stay in registers from one pixel to the next: a record is loaded only when its tap index changes, and the right
// pair becomes the left pair when the taps move on by one.  The arithmetic per pixel does not depend on what was reused.
template <int MODE>
__device__ __forceinline__ void apply_tile(unsigned tile, float (&px)[3 * UPS_TILE], const float4* __restrict__ records, int h,
                                           int w, const float* __restrict__ guide, int H, int W, float sy, float sx,
                                           float* __restrict__ out) {
  constexpr int NV = MODE == STROTSS_UPSAMPLE_RESIDUAL ? 4 : 3;
  const unsigned npix = (unsigned)H * (unsigned)W;
  const unsigned p0 = tile * UPS_TILE;
  const unsigned n = min(npix - p0, (unsigned)UPS_TILE);               // pixels of this tile
  const float* src = guide + 3 * (size_t)p0;
  float* dst = out + 3 * (size_t)p0;
  __syncthreads();                                                      // the tile before has left px
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const unsigned f = 4 * (j * UPS_THREADS + threadIdx.x);
    if (f + 4 <= 3 * n) {
      *(float4*)&px[f] = *(const float4*)&src[f];
    } else {
      for (unsigned k = f; k < 3 * n; ++k) px[k] = src[k];
    }
  }
  __syncthreads();
  const unsigned q0 = UPS_PIXELS * threadIdx.x;
  if (q0 < n) {
    float i[3 * UPS_PIXELS];                                            // floats past 3 n are stale LDS and go back as they came
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float4 g = *(const float4*)&px[3 * q0 + 4 * k];
      i[4 * k] = g.x;
      i[4 * k + 1] = g.y;
      i[4 * k + 2] = g.z;
      i[4 * k + 3] = g.w;
    }
    const unsigned p = p0 + q0;
    int y = (int)(p / (unsigned)W), x = (int)(p - (unsigned)y * (unsigned)W);
    int cy0 = -1, cy1 = -1, ca = -1, cb = -1;                           // the taps whose records tl, tr, bl, br hold
    float4 tl[NV], tr[NV], bl[NV], br[NV];
#pragma unroll
    for (int j = 0; j < UPS_PIXELS; ++j) {
      if (q0 + j < n) {
        const UpsTap ty = ups_tap(y, sy, h), tx = ups_tap(x, sx, w);
        const float4* r0 = records + (UPS_RECORD / 4) * ((size_t)ty.lo * w);
        const float4* r1 = records + (UPS_RECORD / 4) * ((size_t)ty.hi * w);
        const bool same_rows = ty.lo == cy0 && ty.hi == cy1;
        if (same_rows && tx.lo == cb && tx.lo != ca) {                  // one record to the right: the right pair moves left
#pragma unroll
          for (int k = 0; k < NV; ++k) {
            tl[k] = tr[k];
            bl[k] = br[k];
          }
          ca = cb;
        }
        if (!same_rows || tx.lo != ca) {
#pragma unroll
          for (int k = 0; k < NV; ++k) {
            tl[k] = r0[(UPS_RECORD / 4) * tx.lo + k];
            bl[k] = r1[(UPS_RECORD / 4) * tx.lo + k];
          }
          ca = tx.lo;
        }
        if (!same_rows || tx.hi != cb) {
#pragma unroll
          for (int k = 0; k < NV; ++k) {
            tr[k] = r0[(UPS_RECORD / 4) * tx.hi + k];
            br[k] = r1[(UPS_RECORD / 4) * tx.hi + k];
          }
          cb = tx.hi;
        }
        cy0 = ty.lo;
        cy1 = ty.hi;
        float v[4 * NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          const float4 m = ups_bilerp4(tl[k], tr[k], bl[k], br[k], tx.lerp, ty.lerp);
          v[4 * k] = m.x;
          v[4 * k + 1] = m.y;
          v[4 * k + 2] = m.z;
          v[4 * k + 3] = m.w;
        }
        const float i0 = i[3 * j], i1 = i[3 * j + 1], i2 = i[3 * j + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float g = fmaf(v[3 * c + 2], i2, fmaf(v[3 * c + 1], i1, fmaf(v[3 * c], i0, v[9 + c])));
          if constexpr (MODE == STROTSS_UPSAMPLE_RESIDUAL) {
            i[3 * j + c] = __fadd_rn(g, v[SMOOTH_S2 + c]);
          } else {
            i[3 * j + c] = g;
          }
        }
        if (++x == W) {
          x = 0;
          ++y;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
      *(float4*)&px[3 * q0 + 4 * k] = make_float4(i[4 * k], i[4 * k + 1], i[4 * k + 2], i[4 * k + 3]);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const unsigned f = 4 * (j * UPS_THREADS + threadIdx.x);
    if (f + 4 <= 3 * n) {
      *(float4*)&dst[f] = *(const float4*)&px[f];
    } else {
      for (unsigned k = f; k < 3 * n; ++k) dst[k] = px[k];
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(UPS_THREADS) void upsample_apply_kernel(const float4* __restrict__ records, int h, int w,
                                                                     const float* __restrict__ guide, int H, int W, float sy,
                                                                     float sx, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float px[3 * UPS_TILE];
  const unsigned ntiles = ((unsigned)H * (unsigned)W + UPS_TILE - 1) / UPS_TILE;
  for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
    apply_tile<MODE>(tile, px, records, h, w, guide, H, W, sy, sx, out);
}

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

// two byte ranges share a byte
static inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}

size_t strotss_guided_upsample_workspace_bytes(int h, int w, int radius) {
  if (!image_size_ok(h, w) || !radius_ok(radius)) return 0;
  return (SMOOTH_WS_PER_PIXEL + UPS_RECORD * sizeof(float)) * (size_t)h * (size_t)w;
}

int strotss_guided_upsample(const float* img, const float* guide_lo, int h, int w, const float* guide_hi, int H, int W,
                            int radius, float eps, int mode, float* out, void* workspace, size_t workspace_bytes,
                            void* stream) {
  ST_CHECK_ARG(img && guide_lo && guide_hi && out && workspace, STROTSS_EINVAL);
  ST_CHECK_ARG(image_size_ok(h, w) && image_size_ok(H, W) && H >= h && W >= w && radius_ok(radius), STROTSS_EINVAL);
  ST_CHECK_ARG(isfinite(eps) && eps >= 1e-4f && eps <= 1.0f, STROTSS_EINVAL);
  ST_CHECK_ARG(mode == STROTSS_UPSAMPLE_GUIDED || mode == STROTSS_UPSAMPLE_RESIDUAL, STROTSS_EINVAL);
  ST_CHECK_ARG(workspace_bytes >= strotss_guided_upsample_workspace_bytes(h, w, radius), STROTSS_EINVAL);
  const size_t npix = (size_t)h * w, lo_bytes = 3 * sizeof(float) * npix, hi_bytes = 3 * sizeof(float) * (size_t)H * W;
  ST_CHECK_ARG(!ranges_overlap(out, hi_bytes, guide_hi, hi_bytes) && !ranges_overlap(out, hi_bytes, guide_lo, lo_bytes) &&
                   !ranges_overlap(out, hi_bytes, img, lo_bytes),
               STROTSS_EINVAL);
  ST_CHECK_ARG(aligned16(img) && aligned16(guide_lo) && aligned16(guide_hi) && aligned16(out) && aligned16(workspace),
               STROTSS_EALIGN);
  float* records = (float*)workspace;                                   // first: 64-byte records on a 16-byte aligned base
  double* planes = (double*)(records + UPS_RECORD * npix);
  float* ab = (float*)(planes + SMOOTH_S1 * npix);
  hipStream_t st = (hipStream_t)stream;
  const dim3 cols_block(SMOOTH_COLS_X, SMOOTH_COLS_Y);
  const dim3 cols_grid(min(cols_tiles(h, w), SMOOTH_MAX_GRID));
  const dim3 rows_grid(min(rows_tiles(h, w), SMOOTH_MAX_GRID));
  hipLaunchKernelGGL(smooth_cols1_kernel, cols_grid, cols_block, 0, st, img, guide_lo, h, w, radius, planes);
  hipLaunchKernelGGL((smooth_rows_kernel<1, SMOOTH_S1, SMOOTH_ROW_CHUNK1>), rows_grid, dim3(SMOOTH_ROW_THREADS), 0, st, planes,
                     guide_lo, h, w, radius, (double)eps, ab);
  hipLaunchKernelGGL(smooth_cols2_kernel, cols_grid, cols_block, 0, st, ab, h, w, radius, planes);
  hipLaunchKernelGGL(smooth_rows_store_kernel, rows_grid, dim3(SMOOTH_ROW_THREADS), 0, st, planes, img, guide_lo, h, w, radius,
                     records);
  // the scales of strotss_resize_bilinear from (h, w) to (H, W)
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  const unsigned ntiles = (unsigned)(((size_t)H * W + UPS_TILE - 1) / UPS_TILE);
  const dim3 apply_grid(min(ntiles, UPS_MAX_GRID));
  if (mode == STROTSS_UPSAMPLE_RESIDUAL)
    hipLaunchKernelGGL(upsample_apply_kernel<STROTSS_UPSAMPLE_RESIDUAL>, apply_grid, dim3(UPS_THREADS), 0, st,
                       (const float4*)records, h, w, guide_hi, H, W, sy, sx, out);
  else
    hipLaunchKernelGGL(upsample_apply_kernel<STROTSS_UPSAMPLE_GUIDED>, apply_grid, dim3(UPS_THREADS), 0, st,
                       (const float4*)records, h, w, guide_hi, H, W, sy, sx, out);
  ST_LAUNCH_RET();
}
