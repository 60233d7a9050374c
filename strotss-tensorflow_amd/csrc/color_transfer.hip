// Colour distribution transfer: the iterative distribution transfer of Pitie, Kokaram and Dahyot
// (2007) on (h, w, 3) float images, "--preserve_color transfer".
//   - color_hist_kernel: the (n_bases, 3, bins) integer histograms of an image's projections on n_bases orthonormal bases,
//     the image read once per group of bases whose histograms fit a workgroup's LDS;
//   - color_table_kernel: the monotone transfer table of one axis per workgroup from two histograms (integer prefix sums);
//   - color_apply_kernel: the three axis displacements of every counted pixel, rotated back, and in the same launch the
//     histogram of the MOVED pixels on the next basis.
// Pixel access as color.hip: groups of 4 pixels = 3 float4 (+ 1 float4 of the weight plane), the last npix mod 4 scalar.
// Counts are uint32 under LDS integer atomics, flushed with integer atomics to global memory: the same bits on every run.
#include <math.h>

#include "internal.h"

namespace {

#define CT_THREADS 256
#define CT_MAX_BLOCKS 256                       // above 2^18 pixels the blocks stride over the groups of 4 pixels
#define CT_LDS_WORDS 15360                      // 60 KiB of LDS counters per workgroup: two workgroups per CU
#define CT_MAX_GROUP 8                          // bases per workgroup at the most (strotss_color_hist_group)
#define CT_MAX_BASES 64
#define CT_MAX_BINS 4096

struct CtBasis { float R[9]; };                 // row-major: R[3 i + k] = component i of axis k
struct CtBasisSet { CtBasis b[CT_MAX_BASES]; };
struct CtAxis { float r0, r1, r2, lo, hi, scale; };

// The range of axis k in double from the float32 basis, on the host and on the device alike: twice the width of the unit
// cube's projection around its middle.  lo, hi and scale are rounded to float32 once.
__host__ __device__ inline void ct_axis_range(const float* R, int k, double& lo, double& hi) {
  double lo0 = 0.0, hi0 = 0.0;
  for (int i = 0; i < 3; ++i) {
    const double r = (double)R[3 * i + k];
    lo0 += r < 0.0 ? r : 0.0;
    hi0 += r > 0.0 ? r : 0.0;
  }
  const double mid = (lo0 + hi0) / 2.0, width = hi0 - lo0;
  lo = mid - width;
  hi = mid + width;
}

__host__ __device__ inline CtAxis ct_axis(const float* R, int k, int bins) {
  double lo, hi;
  ct_axis_range(R, k, lo, hi);
  CtAxis a;
  a.r0 = R[k];
  a.r1 = R[3 + k];
  a.r2 = R[6 + k];
  a.lo = (float)lo;
  a.hi = (float)hi;
  a.scale = (float)((double)bins / (hi - lo));
  return a;
}

// u = R_0k x_0 + R_1k x_1 + R_2k x_2 left to right, clamped to the axis range (a NaN goes to lo); pos >= 0
__device__ __forceinline__ float ct_project(const CtAxis& a, float x0, float x1, float x2, float& pos) {
  const float u = fmaf(a.r2, x2, fmaf(a.r1, x1, a.r0 * x0));
  const float ub = fminf(fmaxf(u, a.lo), a.hi);
  pos = (ub - a.lo) * a.scale;
  return ub;
}

__device__ __forceinline__ int ct_bin(float pos, int bins) {
  const int j = (int)fminf(pos, (float)bins);         // pos is finite and >= 0; the min keeps the conversion in range
  return j < bins - 1 ? (j < 0 ? 0 : j) : bins - 1;
}

__device__ __forceinline__ void ct_count(unsigned* lh, const CtAxis* ax, int n_axes, int bins, float x0, float x1, float x2) {
  for (int a = 0; a < n_axes; ++a) {
    float pos;
    ct_project(ax[a], x0, x1, x2, pos);
    atomicAdd(&lh[a * bins + ct_bin(pos, bins)], 1u);
  }
}

// Block (bx, by) takes the bases by * group .. and the pixel groups bx, bx + gridDim.x, ...: one read of the image per
// group of bases.  hist was cleared before the launch.
__global__ __launch_bounds__(CT_THREADS) void color_hist_kernel(const float* __restrict__ img,
                                                                const float* __restrict__ weight, int npix, CtBasisSet set,
                                                                int n_bases, int group, int bins,
                                                                unsigned* __restrict__ hist) {
  extern __shared__ unsigned lh[];
  __shared__ CtAxis ax[3 * CT_MAX_GROUP];
  const int base0 = blockIdx.y * group;
  const int nb = n_bases - base0 < group ? n_bases - base0 : group;
  const int n_axes = 3 * nb, words = n_axes * bins;
  for (int i = threadIdx.x; i < words; i += CT_THREADS) lh[i] = 0u;
  for (int a = 0; a < n_axes; ++a)                                 // a uniform index into the kernel's arguments
    if ((int)threadIdx.x == a) ax[a] = ct_axis(set.b[base0 + a / 3].R, a % 3, bins);
  __syncthreads();
  const long long ngroups = ((long long)npix + 3) / 4;
  for (long long g = (long long)blockIdx.x * CT_THREADS + threadIdx.x; g < ngroups; g += (long long)gridDim.x * CT_THREADS) {
    const long long p0 = 4 * g;
    if (p0 + 4 <= npix) {
      const f32x4* x4 = reinterpret_cast<const f32x4*>(img + 3 * p0);
      const f32x4 v0 = x4[0], v1 = x4[1], v2 = x4[2];
      f32x4 m = {1.f, 1.f, 1.f, 1.f};
      if (weight) m = *reinterpret_cast<const f32x4*>(weight + p0);
      if (m[0] != 0.f) ct_count(lh, ax, n_axes, bins, v0[0], v0[1], v0[2]);
      if (m[1] != 0.f) ct_count(lh, ax, n_axes, bins, v0[3], v1[0], v1[1]);
      if (m[2] != 0.f) ct_count(lh, ax, n_axes, bins, v1[2], v1[3], v2[0]);
      if (m[3] != 0.f) ct_count(lh, ax, n_axes, bins, v2[1], v2[2], v2[3]);
    } else {
      for (long long p = p0; p < npix; ++p)
        if (!weight || weight[p] != 0.f) ct_count(lh, ax, n_axes, bins, img[3 * p], img[3 * p + 1], img[3 * p + 2]);
    }
  }
  __syncthreads();
  unsigned* dst = hist + (size_t)base0 * 3 * bins;
  for (int i = threadIdx.x; i < words; i += CT_THREADS) {
    const unsigned v = lh[i];
    if (v) atomicAdd(&dst[i], v);
  }
}

// One workgroup per axis.  S and C: the exclusive cumulative counts of the source and target histograms (bins + 1 entries
// each, integers).  Edge j goes to the point of the target axis below which the same share of the target's pixels lies.
__global__ __launch_bounds__(CT_THREADS) void color_table_kernel(const unsigned* __restrict__ hist_src,
                                                                 const unsigned* __restrict__ hist_dst, CtBasis basis,
                                                                 int bins, float* __restrict__ table) {
  __shared__ unsigned S[CT_MAX_BINS + 1], Cc[CT_MAX_BINS + 1];
  __shared__ unsigned part[2][CT_THREADS];
  const int k = blockIdx.x, t = threadIdx.x;
  const unsigned* hs = hist_src + (size_t)k * bins;
  const unsigned* hc = hist_dst + (size_t)k * bins;
  const int chunk = (bins + CT_THREADS - 1) / CT_THREADS;          // <= 16
  const int b0 = t * chunk < bins ? t * chunk : bins, b1 = b0 + chunk < bins ? b0 + chunk : bins;
  unsigned ss = 0u, sc = 0u;
  for (int i = b0; i < b1; ++i) {                                  // exclusive sums inside the thread's chunk
    S[i] = ss;
    Cc[i] = sc;
    ss += hs[i];
    sc += hc[i];
  }
  part[0][t] = ss;
  part[1][t] = sc;
  __syncthreads();
  if (t < 2) {                                                     // the 256 chunk totals, in order
    unsigned run = 0u;
    for (int i = 0; i < CT_THREADS; ++i) {
      const unsigned v = part[t][i];
      part[t][i] = run;
      run += v;
    }
    (t == 0 ? S : Cc)[bins] = run;
  }
  __syncthreads();
  for (int i = b0; i < b1; ++i) {
    S[i] += part[0][t];
    Cc[i] += part[1][t];
  }
  __syncthreads();
  double lo, hi;
  ct_axis_range(basis.R, k, lo, hi);
  const double width = (hi - lo) / (double)bins;
  const unsigned long long Ns = S[bins], Nc = Cc[bins];
  float* out = table + (size_t)k * (bins + 1);
  for (int j = t; j <= bins; j += CT_THREADS) {
    double v = (double)j;                                          // an empty histogram: the identity
    if (Ns != 0ull && Nc != 0ull) {
      const unsigned long long a = (unsigned long long)S[j] * Nc;
      const unsigned long long need = a ? a : 1ull;                // a == 0: the first target bin that is not empty
      int l = 0, r = bins - 1;                                     // the smallest i with C[i + 1] Ns >= need
      while (l < r) {
        const int mid = (l + r) >> 1;
        if ((unsigned long long)Cc[mid + 1] * Ns >= need) r = mid; else l = mid + 1;
      }
      const unsigned long long below = (unsigned long long)Cc[l] * Ns;
      const unsigned long long den = (unsigned long long)(Cc[l + 1] - Cc[l]) * Ns;
      double frac = (den != 0ull && a > below) ? (double)(a - below) / (double)den : 0.0;
      frac = frac < 1.0 ? frac : 1.0;
      v = (double)l + frac;
    }
    out[j] = (float)(lo + v * width);
  }
}

struct CtMap { CtAxis ax[3]; float R[9]; };

// x'_i = x_i + R_i0 d_0 + R_i1 d_1 + R_i2 d_2 with d_k = T_k(pos_k) - clamp(u_k): the table read at the bin position by
// linear interpolation between its two edges.  A pixel whose weight is 0 keeps its bits.
__device__ __forceinline__ void ct_move_pixel(const CtMap& t, const float* __restrict__ table, int bins, bool on, float x0,
                                              float x1, float x2, float& y0, float& y1, float& y2) {
  float d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float pos;
    const float ub = ct_project(t.ax[k], x0, x1, x2, pos);
    const int j = ct_bin(pos, bins);
    const float f = pos - (float)j;
    const float* T = table + (size_t)k * (bins + 1) + j;
    const float t0 = T[0], t1 = T[1];
    d[k] = fmaf(f, t1 - t0, t0) - ub;
  }
  y0 = on ? fmaf(t.R[2], d[2], fmaf(t.R[1], d[1], fmaf(t.R[0], d[0], x0))) : x0;
  y1 = on ? fmaf(t.R[5], d[2], fmaf(t.R[4], d[1], fmaf(t.R[3], d[0], x1))) : x1;
  y2 = on ? fmaf(t.R[8], d[2], fmaf(t.R[7], d[1], fmaf(t.R[6], d[0], x2))) : x2;
}

// A thread reads its whole group before it writes (out may be img).  With next_hist: the stored float32 values of the
// counted pixels are binned on the next basis exactly as color_hist_kernel bins them (LDS counts, flushed at the end).
__global__ __launch_bounds__(CT_THREADS) void color_apply_kernel(const float* img, const float* __restrict__ weight, int npix,
                                                                 CtMap t, const float* __restrict__ table, int bins,
                                                                 float* out, CtBasis next, unsigned* __restrict__ next_hist) {
  extern __shared__ unsigned lh[];
  __shared__ CtAxis ax[3];
  if (next_hist) {
    for (int i = threadIdx.x; i < 3 * bins; i += CT_THREADS) lh[i] = 0u;
    if (threadIdx.x < 3) ax[threadIdx.x] = ct_axis(next.R, threadIdx.x, bins);
    __syncthreads();
  }
  const long long ngroups = ((long long)npix + 3) / 4;
  for (long long g = (long long)blockIdx.x * CT_THREADS + threadIdx.x; g < ngroups; g += (long long)gridDim.x * CT_THREADS) {
    const long long p0 = 4 * g;
    if (p0 + 4 <= npix) {
      const f32x4* x4 = reinterpret_cast<const f32x4*>(img + 3 * p0);
      const f32x4 v0 = x4[0], v1 = x4[1], v2 = x4[2];
      f32x4 m = {1.f, 1.f, 1.f, 1.f};
      if (weight) m = *reinterpret_cast<const f32x4*>(weight + p0);
      float y[12];
      ct_move_pixel(t, table, bins, m[0] != 0.f, v0[0], v0[1], v0[2], y[0], y[1], y[2]);
      ct_move_pixel(t, table, bins, m[1] != 0.f, v0[3], v1[0], v1[1], y[3], y[4], y[5]);
      ct_move_pixel(t, table, bins, m[2] != 0.f, v1[2], v1[3], v2[0], y[6], y[7], y[8]);
      ct_move_pixel(t, table, bins, m[3] != 0.f, v2[1], v2[2], v2[3], y[9], y[10], y[11]);
      f32x4* y4 = reinterpret_cast<f32x4*>(out + 3 * p0);
#pragma unroll
      for (int q = 0; q < 3; ++q) y4[q] = f32x4{y[4 * q], y[4 * q + 1], y[4 * q + 2], y[4 * q + 3]};
      if (next_hist) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (m[q] != 0.f) ct_count(lh, ax, 3, bins, y[3 * q], y[3 * q + 1], y[3 * q + 2]);
      }
    } else {
      for (long long p = p0; p < npix; ++p) {
        const bool on = !weight || weight[p] != 0.f;
        float y0, y1, y2;
        ct_move_pixel(t, table, bins, on, img[3 * p], img[3 * p + 1], img[3 * p + 2], y0, y1, y2);
        out[3 * p] = y0;
        out[3 * p + 1] = y1;
        out[3 * p + 2] = y2;
        if (next_hist && on) ct_count(lh, ax, 3, bins, y0, y1, y2);
      }
    }
  }
  if (next_hist) {
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * bins; i += CT_THREADS) {
      const unsigned v = lh[i];
      if (v) atomicAdd(&next_hist[i], v);
    }
  }
}

inline bool image_size_ok(int h, int w) { return h > 0 && w > 0 && 3LL * h * w <= 0x7fffffffLL; }
inline bool bins_ok(int bins) { return bins >= 2 && bins <= CT_MAX_BINS; }
inline unsigned walk_blocks(long long npix) {
  const long long b = ((npix + 3) / 4 + CT_THREADS - 1) / CT_THREADS;
  return (unsigned)(b < CT_MAX_BLOCKS ? b : CT_MAX_BLOCKS);
}

// finite, and orthonormal to max |R^T R - I| <= 1e-4 (in double)
bool basis_ok(const float* R) {
  for (int i = 0; i < 9; ++i)
    if (!isfinite(R[i])) return false;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double dot = 0.0;
      for (int i = 0; i < 3; ++i) dot += (double)R[3 * i + a] * (double)R[3 * i + b];
      if (!(fabs(dot - (a == b ? 1.0 : 0.0)) <= 1e-4)) return false;
    }
  return true;
}

}  // namespace

int strotss_color_hist_group(int bins) {
  if (!bins_ok(bins)) return 0;
  const int g = CT_LDS_WORDS / (3 * bins);
  return g < 1 ? 1 : g > CT_MAX_GROUP ? CT_MAX_GROUP : g;
}

int strotss_color_hist(const float* img, const float* weight, int h, int w, const float* bases, int n_bases, int bins,
                       unsigned* hist, void* stream) {
  ST_CHECK_ARG(img && bases && hist && image_size_ok(h, w) && bins_ok(bins), STROTSS_EINVAL);
  ST_CHECK_ARG(n_bases >= 1 && n_bases <= CT_MAX_BASES, STROTSS_EINVAL);
  CtBasisSet set = {};
  for (int n = 0; n < n_bases; ++n) {
    ST_CHECK_ARG(basis_ok(bases + 9 * n), STROTSS_EINVAL);
    for (int i = 0; i < 9; ++i) set.b[n].R[i] = bases[9 * n + i];
  }
  ST_CHECK_ARG(aligned16(img) && aligned16(weight) && aligned16(hist), STROTSS_EALIGN);
  const long long npix = (long long)h * w;
  const int group = strotss_color_hist_group(bins);
  const int real = group < n_bases ? group : n_bases;              // a block never holds more bases than there are
  hipError_t e = hipMemsetAsync(hist, 0, sizeof(unsigned) * 3 * (size_t)bins * n_bases, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(color_hist_kernel, dim3(walk_blocks(npix), (n_bases + group - 1) / group), dim3(CT_THREADS),
                     sizeof(unsigned) * 3 * (size_t)bins * real, (hipStream_t)stream, img, weight, (int)npix, set, n_bases,
                     group, bins, hist);
  ST_LAUNCH_RET();
}

int strotss_color_transfer_table(const unsigned* hist_src, const unsigned* hist_dst, const float* basis, int bins,
                                 float* table, void* stream) {
  ST_CHECK_ARG(hist_src && hist_dst && basis && table && bins_ok(bins), STROTSS_EINVAL);
  ST_CHECK_ARG(basis_ok(basis), STROTSS_EINVAL);
  ST_CHECK_ARG(aligned16(hist_src) && aligned16(hist_dst) && aligned16(table), STROTSS_EALIGN);
  CtBasis b;
  for (int i = 0; i < 9; ++i) b.R[i] = basis[i];
  hipLaunchKernelGGL(color_table_kernel, dim3(3), dim3(CT_THREADS), 0, (hipStream_t)stream, hist_src, hist_dst, b, bins,
                     table);
  ST_LAUNCH_RET();
}

int strotss_color_transfer_apply(const float* img, const float* weight, int h, int w, const float* basis, const float* table,
                                 int bins, float* out, const float* next_basis, unsigned* next_hist, void* stream) {
  ST_CHECK_ARG(img && basis && table && out && image_size_ok(h, w) && bins_ok(bins), STROTSS_EINVAL);
  ST_CHECK_ARG((next_basis == nullptr) == (next_hist == nullptr), STROTSS_EINVAL);
  ST_CHECK_ARG(basis_ok(basis) && (!next_basis || basis_ok(next_basis)), STROTSS_EINVAL);
  ST_CHECK_ARG(aligned16(img) && aligned16(weight) && aligned16(table) && aligned16(out) && aligned16(next_hist),
               STROTSS_EALIGN);
  CtMap t;
  CtBasis next = {};
  for (int i = 0; i < 9; ++i) {
    t.R[i] = basis[i];
    if (next_basis) next.R[i] = next_basis[i];
  }
  for (int k = 0; k < 3; ++k) t.ax[k] = ct_axis(basis, k, bins);
  const long long npix = (long long)h * w;
  size_t lds = 0;
  if (next_hist) {
    lds = sizeof(unsigned) * 3 * (size_t)bins;
    hipError_t e = hipMemsetAsync(next_hist, 0, lds, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(color_apply_kernel, dim3(walk_blocks(npix)), dim3(CT_THREADS), lds, (hipStream_t)stream, img, weight,
                     (int)npix, t, table, bins, out, next, next_hist);
  ST_LAUNCH_RET();
}
