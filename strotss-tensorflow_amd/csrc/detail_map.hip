// The detail map of --sample_map auto: where the content has local structure, as an (h, w) float32
// map in [floor, 1] that the importance-sampled draw (section 28) takes in place of a painted one.
//   Y = 0.299 R + 0.587 G + 0.114 B,  e = gx^2 + gy^2 with central differences of Y halved, indices clamped,
//   s(p) = sqrt(mean of e over the (2r+1) x (2r+1) window clipped to the image),  m = mean of s over the image,
//   out(p) = floor + (1 - floor) min(1, s(p) / (gain m));  m == 0: out = 1.
// Three launches:
//   detail_cols_kernel   a tile is 64 columns x 16 rows.  e of the rows [y0 - r, y0 + 15 + r] clipped to the image is
//                        computed ONCE into LDS (float32, every operation rounded on its own: no contraction, so the bits
//                        are those of the float32 statement), then each thread sums the columns of its four pixels in
//                        float64, ascending y -> one float64 plane.  DIRECT sums as in smooth.hip.
//   detail_rows_kernel   a tile is 256 consecutive pixels of a row: the row sums through LDS in float64, ascending x, the
//                        mean and its root in float32 -> out holds s; the threads' sums of s (float64, in tile order) go
//                        through ticket_sum_256 -> m in the workspace.  The grid depends on (h, w) alone: the same bits
//                        on every run.
//   detail_scale_kernel  out = floor + (1 - floor) min(1, s / (gain m)) in place, float4 where whole.
// No float atomics; every store is a vector store from plain C++.
#include <math.h>

#include "internal.h"

namespace {

#define DM_MAX_RADIUS 64
#define DM_COLS_X 64                     // column pass: a tile of 64 x 16 pixels per 64 x 4 workgroup, four rows a thread
#define DM_COLS_TY 4
#define DM_COLS_Y 16
#define DM_COLS_SPAN (DM_COLS_Y + 2 * DM_MAX_RADIUS)      // rows of e staged at most: 144 x 64 floats = 36 KB
#define DM_ROW_THREADS 256               // row pass: 256 consecutive pixels of one row per workgroup
#define DM_ROW_SPAN (DM_ROW_THREADS + 2 * DM_MAX_RADIUS)
#define DM_MAX_GRID (1u << 14)           // workgroups of the column pass at most; a workgroup walks the tiles beyond that number
#define DM_ROWS_MAX_GRID 512u            // ... of the row pass: each takes a ticket on ONE address, and 4096 of them cost 100 us
                                         //   at 1024 x 1024 where 512 (two a compute unit) cost a few
#define DM_SCALE_THREADS 256
#define DM_SCALE_MAX_GRID (1u << 12)
#define DM_WS_HEADER 32                  // {unsigned ticket, 12 bytes, double m, 8 bytes}, then the partials, then the plane

__host__ __device__ __forceinline__ unsigned dm_cols_tiles(int h, int w) {
  return (((unsigned)w + DM_COLS_X - 1) / DM_COLS_X) * (((unsigned)h + DM_COLS_Y - 1) / DM_COLS_Y);
}
__host__ __device__ __forceinline__ unsigned dm_rows_tiles(int h, int w) {
  return (((unsigned)w + DM_ROW_THREADS - 1) / DM_ROW_THREADS) * (unsigned)h;
}
inline unsigned dm_rows_grid(int h, int w) { return min(dm_rows_tiles(h, w), DM_ROWS_MAX_GRID); }
// doubles kept for the partials of the row pass: its grid, rounded up to an even count (the plane stays 16-byte aligned)
inline size_t dm_partial_slots(int h, int w) { return ((size_t)dm_rows_grid(h, w) + 1) & ~(size_t)1; }

__device__ __forceinline__ float dm_luma(const float* __restrict__ img, size_t pixel) {
  const float r = img[3 * pixel], g = img[3 * pixel + 1], b = img[3 * pixel + 2];
  return __fadd_rn(__fadd_rn(__fmul_rn(0.299f, r), __fmul_rn(0.587f, g)), __fmul_rn(0.114f, b));
}

// gradient energy of the luma at (y, x), 0 <= y < h, 0 <= x < w; a clamped axis of one pixel gives a zero difference
__device__ __forceinline__ float dm_energy(const float* __restrict__ img, int h, int w, int y, int x) {
  const size_t row = (size_t)y * w;
  const float xl = dm_luma(img, row + max(x - 1, 0)), xr = dm_luma(img, row + min(x + 1, w - 1));
  const float yu = dm_luma(img, (size_t)max(y - 1, 0) * w + x), yd = dm_luma(img, (size_t)min(y + 1, h - 1) * w + x);
  const float gx = __fmul_rn(__fsub_rn(xr, xl), 0.5f), gy = __fmul_rn(__fsub_rn(yd, yu), 0.5f);
  return __fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy));
}

__global__ __launch_bounds__(DM_COLS_X* DM_COLS_TY) void detail_cols_kernel(const float* __restrict__ img, int h, int w, int r,
                                                                            double* __restrict__ plane) {
  __shared__ float e[DM_COLS_SPAN][DM_COLS_X];
  const unsigned ntx = ((unsigned)w + DM_COLS_X - 1) / DM_COLS_X;
  const unsigned ntiles = dm_cols_tiles(h, w);
  for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int x = (int)(tile % ntx) * DM_COLS_X + (int)threadIdx.x;
    const int yb = (int)(tile / ntx) * DM_COLS_Y;
    const int ys = max(yb - r, 0), ye = min(yb + DM_COLS_Y - 1 + r, h - 1);      // ye - ys < DM_COLS_SPAN for r <= 64
    __syncthreads();                                                    // the tile before has been summed
    if (x < w) {
      for (int i = (int)threadIdx.y; i <= ye - ys; i += DM_COLS_TY) e[i][threadIdx.x] = dm_energy(img, h, w, ys + i, x);
    }
    __syncthreads();
    if (x < w) {
#pragma unroll
      for (int k = 0; k < DM_COLS_Y / DM_COLS_TY; ++k) {
        const int y = yb + k * DM_COLS_TY + (int)threadIdx.y;
        if (y < h) {
          const int lo = max(y - r, 0) - ys, hi = min(y + r, h - 1) - ys;
          double s = 0.0;
          for (int i = lo; i <= hi; ++i) s += (double)e[i][threadIdx.x];
          plane[(size_t)y * w + x] = s;
        }
      }
    }
  }
}

__global__ __launch_bounds__(DM_ROW_THREADS) void detail_rows_kernel(const double* __restrict__ plane, int h, int w, int r,
                                                                     float* __restrict__ out, double inv_npix,
                                                                     double* __restrict__ mean_out,
                                                                     unsigned* __restrict__ ticket,
                                                                     double* __restrict__ partials) {
  __shared__ double span[DM_ROW_SPAN];
  __shared__ double red[4][1];
  __shared__ int is_last;
  const unsigned ntx = ((unsigned)w + DM_ROW_THREADS - 1) / DM_ROW_THREADS;
  const unsigned ntiles = dm_rows_tiles(h, w);
  double acc[1] = {0.0};
  for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int y = (int)(tile / ntx);
    const int xb = (int)(tile % ntx) * DM_ROW_THREADS;
    const int x = xb + (int)threadIdx.x;
    const int xs = max(xb - r, 0), xe = min(xb + DM_ROW_THREADS - 1 + r, w - 1);  // the span of this workgroup's windows
    const size_t row = (size_t)y * w;
    __syncthreads();                                                    // the span of the tile before is read
    for (int i = (int)threadIdx.x; i <= xe - xs; i += DM_ROW_THREADS) span[i] = plane[row + xs + i];
    __syncthreads();
    if (x < w) {
      const int lo = max(x - r, 0) - xs, hi = min(x + r, w - 1) - xs;
      double s = 0.0;
      for (int i = lo; i <= hi; ++i) s += span[i];
      const int n = (hi - lo + 1) * (min(y + r, h - 1) - max(y - r, 0) + 1);      // at most 129^2: exact in float32
      const float d = __fsqrt_rn(__fdiv_rn((float)s, (float)n));
      out[row + x] = d;
      acc[0] += (double)d;
    }
  }
  // every thread of every workgroup arrives here: no thread has returned above
  ticket_sum_256(acc, inv_npix, mean_out, ticket, partials, red, &is_last);
}

__device__ __forceinline__ float dm_scale(float s, float denom, float floor_, float span) {
  if (denom == 0.0f) return 1.0f;                                       // a constant image: m == 0
  const float t = __fdiv_rn(s, denom);
  return t >= 1.0f ? 1.0f : __fadd_rn(floor_, __fmul_rn(span, t));     // the clamp gives 1 itself, not floor + (1 - floor)
}

__global__ __launch_bounds__(DM_SCALE_THREADS) void detail_scale_kernel(float* __restrict__ out, unsigned npix, float gain,
                                                                        float floor_, const double* __restrict__ mean) {
  const float denom = __fmul_rn(gain, (float)*mean);
  const float span = __fsub_rn(1.0f, floor_);
  const unsigned n4 = npix / 4;
  f32x4* out4 = reinterpret_cast<f32x4*>(out);                          // out is 16-byte aligned
  for (unsigned i = blockIdx.x * DM_SCALE_THREADS + threadIdx.x; i < n4; i += gridDim.x * DM_SCALE_THREADS) {
    f32x4 v = out4[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = dm_scale(v[k], denom, floor_, span);
    out4[i] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x < npix - 4 * n4) {
    const unsigned i = 4 * n4 + threadIdx.x;
    out[i] = dm_scale(out[i], denom, floor_, span);
  }
}

inline bool dm_size_ok(int h, int w) { return h > 0 && w > 0 && 3LL * h * w <= 0x7fffffffLL; }

}  // namespace

size_t strotss_detail_map_workspace_bytes(int h, int w) {
  if (!dm_size_ok(h, w)) return 0;
  return DM_WS_HEADER + sizeof(double) * (dm_partial_slots(h, w) + (size_t)h * (size_t)w);
}

int strotss_detail_map(const float* img, int h, int w, int radius, float gain, float floor, float* out, void* workspace,
                       void* stream) {
  ST_CHECK_ARG(img && out && workspace && dm_size_ok(h, w), STROTSS_EINVAL);
  ST_CHECK_ARG(radius >= 1 && radius <= DM_MAX_RADIUS, STROTSS_ERANGE);
  ST_CHECK_ARG(isfinite(gain) && gain > 0.0f && isfinite(floor) && floor >= 0.0f && floor <= 1.0f, STROTSS_ERANGE);
  ST_CHECK_ARG(aligned16(img) && aligned16(out) && aligned16(workspace), STROTSS_EALIGN);
  unsigned* ticket = (unsigned*)workspace;
  double* mean = (double*)((char*)workspace + 16);
  double* partials = (double*)((char*)workspace + DM_WS_HEADER);
  double* plane = partials + dm_partial_slots(h, w);
  const unsigned npix = (unsigned)h * (unsigned)w;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(detail_cols_kernel, dim3(min(dm_cols_tiles(h, w), DM_MAX_GRID)), dim3(DM_COLS_X, DM_COLS_TY), 0, st, img,
                     h, w, radius, plane);
  hipLaunchKernelGGL(detail_rows_kernel, dim3(dm_rows_grid(h, w)), dim3(DM_ROW_THREADS), 0, st, plane, h, w, radius, out,
                     1.0 / (double)npix, mean, ticket, partials);
  const unsigned groups = (npix / 4 + DM_SCALE_THREADS - 1) / DM_SCALE_THREADS;
  hipLaunchKernelGGL(detail_scale_kernel, dim3(min(max(groups, 1u), DM_SCALE_MAX_GRID)), dim3(DM_SCALE_THREADS), 0, st, out,
                     npix, gain, floor, mean);
  ST_LAUNCH_RET();
}
