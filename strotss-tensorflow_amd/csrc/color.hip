// Colour preservation: the two controls of Gatys et al. (2016) on (h, w, 3) float images.
//   - color_stats_kernel: W, S_i, S_ij of an image under an optional weight plane, ten float64 sums in one launch (once per
//     style image and run, once per frame with --video);
//   - color_affine_kernel: s'(p) = A s(p) + b, the recolouring of a style image ("match");
//   - luma_merge_kernel: the luma of the result on the chroma of the content ("luminance").
// All three work on groups of 4 pixels = 12 floats = 3 float4 (+ 1 float4 of the weight plane): a group starts on a 16-byte
// boundary whenever the image does, and every channel of a pixel sits in the thread that needs it.
#include <math.h>

#include "internal.h"

namespace {

#define COLOR_THREADS 256                // ticket_sum_256's workgroup
#define COLOR_PIX_PER_BLOCK (4 * COLOR_THREADS)
#define COLOR_MAX_BLOCKS 2048            // above 2^21 pixels the blocks stride over the groups: the partials stay 160 KB
#define COLOR_SUMS 10                    // W, S_0, S_1, S_2, S_00, S_01, S_02, S_11, S_12, S_22

__device__ __forceinline__ void color_accum(double (&a)[COLOR_SUMS], float m, float x0, float x1, float x2) {
  const double dm = m, d0 = x0, d1 = x1, d2 = x2;      // a product of two float32 values is exact in float64
  a[0] += dm;
  a[1] += dm * d0;
  a[2] += dm * d1;
  a[3] += dm * d2;
  a[4] += dm * (d0 * d0);
  a[5] += dm * (d0 * d1);
  a[6] += dm * (d0 * d2);
  a[7] += dm * (d1 * d1);
  a[8] += dm * (d1 * d2);
  a[9] += dm * (d2 * d2);
}

// Thread t of block b takes the groups (b + i gridDim) 256 + t, i = 0, 1, ... in ascending order, the 4 pixels of a group in
// ascending order: per-thread float64 sums in element order, then ticket_sum_256 (csrc/ticket_sum.h) with scale 1.0, which
// is exact.  No float atomics: the ten doubles are the same bits on every run.
__global__ __launch_bounds__(COLOR_THREADS) void color_stats_kernel(const float* __restrict__ img,
                                                                    const float* __restrict__ weight, int npix,
                                                                    double* __restrict__ out, unsigned* __restrict__ ticket,
                                                                    double* __restrict__ partials) {
  __shared__ double red[4][COLOR_SUMS];
  __shared__ int is_last;
  double a[COLOR_SUMS];
#pragma unroll
  for (int k = 0; k < COLOR_SUMS; ++k) a[k] = 0.0;
  const long long ngroups = ((long long)npix + 3) / 4;
  for (long long g = (long long)blockIdx.x * COLOR_THREADS + threadIdx.x; g < ngroups;
       g += (long long)gridDim.x * COLOR_THREADS) {
    const long long p0 = 4 * g;
    if (p0 + 4 <= npix) {
      const f32x4* x4 = reinterpret_cast<const f32x4*>(img + 3 * p0);
      const f32x4 v0 = x4[0], v1 = x4[1], v2 = x4[2];
      f32x4 m = {1.f, 1.f, 1.f, 1.f};
      if (weight) m = *reinterpret_cast<const f32x4*>(weight + p0);
      color_accum(a, m[0], v0[0], v0[1], v0[2]);
      color_accum(a, m[1], v0[3], v1[0], v1[1]);
      color_accum(a, m[2], v1[2], v1[3], v2[0]);
      color_accum(a, m[3], v2[1], v2[2], v2[3]);
    } else {
      for (long long p = p0; p < npix; ++p)
        color_accum(a, weight ? weight[p] : 1.f, img[3 * p], img[3 * p + 1], img[3 * p + 2]);
    }
  }
  ticket_sum_256(a, 1.0, out, ticket, partials, red, &is_last);
}

// the 12 floats of a group as 3 float4 stores
__device__ __forceinline__ void store_group(float* dst, const float (&y)[12]) {
  f32x4* y4 = reinterpret_cast<f32x4*>(dst);
#pragma unroll
  for (int k = 0; k < 3; ++k) y4[k] = f32x4{y[4 * k], y[4 * k + 1], y[4 * k + 2], y[4 * k + 3]};
}

struct ColorMap { float A[9]; float b[3]; };

// b_i + A_i0 x_0 + A_i1 x_1 + A_i2 x_2, left to right; a pixel whose weight is 0 keeps its bits
__device__ __forceinline__ void color_map_pixel(const ColorMap& t, float m, float x0, float x1, float x2, float& y0, float& y1,
                                                float& y2) {
  const bool on = m != 0.f;
  y0 = on ? fmaf(t.A[2], x2, fmaf(t.A[1], x1, fmaf(t.A[0], x0, t.b[0]))) : x0;
  y1 = on ? fmaf(t.A[5], x2, fmaf(t.A[4], x1, fmaf(t.A[3], x0, t.b[1]))) : x1;
  y2 = on ? fmaf(t.A[8], x2, fmaf(t.A[7], x1, fmaf(t.A[6], x0, t.b[2]))) : x2;
}

// One thread per group of 4 pixels; a thread reads its whole group before it writes (out may be img).
__global__ __launch_bounds__(COLOR_THREADS) void color_affine_kernel(const float* img, const float* __restrict__ weight,
                                                                     int npix, ColorMap t, float* out) {
  const long long p0 = 4 * ((long long)blockIdx.x * COLOR_THREADS + threadIdx.x);
  if (p0 >= npix) return;
  if (p0 + 4 <= npix) {
    const f32x4* x4 = reinterpret_cast<const f32x4*>(img + 3 * p0);
    const f32x4 v0 = x4[0], v1 = x4[1], v2 = x4[2];
    f32x4 m = {1.f, 1.f, 1.f, 1.f};
    if (weight) m = *reinterpret_cast<const f32x4*>(weight + p0);
    float y[12];
    color_map_pixel(t, m[0], v0[0], v0[1], v0[2], y[0], y[1], y[2]);
    color_map_pixel(t, m[1], v0[3], v1[0], v1[1], y[3], y[4], y[5]);
    color_map_pixel(t, m[2], v1[2], v1[3], v2[0], y[6], y[7], y[8]);
    color_map_pixel(t, m[3], v2[1], v2[2], v2[3], y[9], y[10], y[11]);
    store_group(out + 3 * p0, y);
  } else {
    for (long long p = p0; p < npix; ++p) {
      float y0, y1, y2;
      color_map_pixel(t, weight ? weight[p] : 1.f, img[3 * p], img[3 * p + 1], img[3 * p + 2], y0, y1, y2);
      out[3 * p] = y0;
      out[3 * p + 1] = y1;
      out[3 * p + 2] = y2;
    }
  }
}

__device__ __forceinline__ float luma(float r, float g, float b) { return fmaf(0.114f, b, fmaf(0.587f, g, 0.299f * r)); }

// out_ch = c_ch + (Y(r) - Y(c)): the same difference on the three channels of a pixel
__device__ __forceinline__ void luma_merge_pixel(float r0, float r1, float r2, float c0, float c1, float c2, float& y0,
                                                 float& y1, float& y2) {
  const float d = luma(r0, r1, r2) - luma(c0, c1, c2);
  y0 = c0 + d;
  y1 = c1 + d;
  y2 = c2 + d;
}

// One thread per group of 4 pixels, as color_affine_kernel (out may be result or content).
__global__ __launch_bounds__(COLOR_THREADS) void luma_merge_kernel(const float* result, const float* content, int npix,
                                                                   float* out) {
  const long long p0 = 4 * ((long long)blockIdx.x * COLOR_THREADS + threadIdx.x);
  if (p0 >= npix) return;
  if (p0 + 4 <= npix) {
    const f32x4* r4 = reinterpret_cast<const f32x4*>(result + 3 * p0);
    const f32x4* c4 = reinterpret_cast<const f32x4*>(content + 3 * p0);
    const f32x4 r0 = r4[0], r1 = r4[1], r2 = r4[2], c0 = c4[0], c1 = c4[1], c2 = c4[2];
    float y[12];
    luma_merge_pixel(r0[0], r0[1], r0[2], c0[0], c0[1], c0[2], y[0], y[1], y[2]);
    luma_merge_pixel(r0[3], r1[0], r1[1], c0[3], c1[0], c1[1], y[3], y[4], y[5]);
    luma_merge_pixel(r1[2], r1[3], r2[0], c1[2], c1[3], c2[0], y[6], y[7], y[8]);
    luma_merge_pixel(r2[1], r2[2], r2[3], c2[1], c2[2], c2[3], y[9], y[10], y[11]);
    store_group(out + 3 * p0, y);
  } else {
    for (long long p = p0; p < npix; ++p) {
      float y0, y1, y2;
      luma_merge_pixel(result[3 * p], result[3 * p + 1], result[3 * p + 2], content[3 * p], content[3 * p + 1],
                       content[3 * p + 2], y0, y1, y2);
      out[3 * p] = y0;
      out[3 * p + 1] = y1;
      out[3 * p + 2] = y2;
    }
  }
}

inline bool image_size_ok(int h, int w) { return h > 0 && w > 0 && 3LL * h * w <= 0x7fffffffLL; }
inline unsigned stats_blocks(long long npix) {
  const long long b = (npix + COLOR_PIX_PER_BLOCK - 1) / COLOR_PIX_PER_BLOCK;
  return (unsigned)(b < COLOR_MAX_BLOCKS ? b : COLOR_MAX_BLOCKS);
}
inline unsigned group_blocks(long long npix) { return (unsigned)(((npix + 3) / 4 + COLOR_THREADS - 1) / COLOR_THREADS); }

}  // namespace

size_t strotss_color_stats_workspace_bytes(int h, int w) {
  if (!image_size_ok(h, w)) return 0;
  return 16 + sizeof(double) * COLOR_SUMS * (size_t)stats_blocks((long long)h * w);
}

int strotss_color_stats(const float* img, const float* weight, int h, int w, double* out, void* workspace, void* stream) {
  ST_CHECK_ARG(img && out && workspace && image_size_ok(h, w), STROTSS_EINVAL);
  ST_CHECK_ARG(aligned16(img) && aligned16(weight) && aligned16(out) && aligned16(workspace), STROTSS_EALIGN);
  const long long npix = (long long)h * w;
  unsigned* ticket = (unsigned*)workspace;
  double* partials = (double*)((char*)workspace + 16);
  hipLaunchKernelGGL(color_stats_kernel, dim3(stats_blocks(npix)), dim3(COLOR_THREADS), 0, (hipStream_t)stream, img, weight,
                     (int)npix, out, ticket, partials);
  ST_LAUNCH_RET();
}

int strotss_color_affine(const float* img, const float* weight, int h, int w, const float* A, const float* b, float* out,
                         void* stream) {
  ST_CHECK_ARG(img && A && b && out && image_size_ok(h, w), STROTSS_EINVAL);
  ColorMap t;
  for (int k = 0; k < 9; ++k) {
    ST_CHECK_ARG(isfinite(A[k]), STROTSS_EINVAL);
    t.A[k] = A[k];
  }
  for (int k = 0; k < 3; ++k) {
    ST_CHECK_ARG(isfinite(b[k]), STROTSS_EINVAL);
    t.b[k] = b[k];
  }
  ST_CHECK_ARG(aligned16(img) && aligned16(weight) && aligned16(out), STROTSS_EALIGN);
  const long long npix = (long long)h * w;
  hipLaunchKernelGGL(color_affine_kernel, dim3(group_blocks(npix)), dim3(COLOR_THREADS), 0, (hipStream_t)stream, img, weight,
                     (int)npix, t, out);
  ST_LAUNCH_RET();
}

int strotss_luma_merge(const float* result, const float* content, int h, int w, float* out, void* stream) {
  ST_CHECK_ARG(result && content && out && image_size_ok(h, w), STROTSS_EINVAL);
  ST_CHECK_ARG(aligned16(result) && aligned16(content) && aligned16(out), STROTSS_EALIGN);
  const long long npix = (long long)h * w;
  hipLaunchKernelGGL(luma_merge_kernel, dim3(group_blocks(npix)), dim3(COLOR_THREADS), 0, (hipStream_t)stream, result,
                     content, (int)npix, out);
  ST_LAUNCH_RET();
}
