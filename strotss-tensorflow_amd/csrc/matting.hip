// The photorealism term of the step: the matting Laplacian of the content (Levin et al. 2008) as the
// regulariser of Luan et al. 2017, windows clipped to the image as section 16 clips them, L p = N (p - q) with q the guided
// filter of the step's image p by the content I.
//   - matting_prepare_kernel: once per scale.  Per pixel k the clipped window's mean mu_k and the inverse of
//     Sigma_k = cov_w(I) + eps Id, in float64 (mean first, then the centred second moments, then the adjugate over the
//     determinant), rounded to float32 once.  stats: 9 planes of (h, w): mu_0..2, then Sigma^{-1} entries 00 01 02 11 12 22.
//   - matting_fwd_bwd_kernel<R>: the step's entry, ONE launch, one workgroup per 16 x 16 pixels.  LDS: I and p on the tile and
//     a 2R halo; a_k (3 x 3) and b_k (3) rebuilt for every window k of the tile and an R halo (0 outside the image, so the
//     unclipped sums below are the clipped ones); their row sums, then their column sums; then the tile's pixels, row by
//     row (coalesced), take v = p - q, add N p v to the scalar and coef N v to gimg.
// All of it float32, the statement of tests/_matting_ref.py (matting_float32) operation by operation: no fused
// multiply-adds.  The covariances are centred: the window is summed once with the data shifted by (mu_k, p_k) -- S_I =
// sum (I - mu_k), S_p = sum (p - p_k), C = sum (I - mu_k) (p - p_k)^T -- and the shift taken out, N cov = C - S_I (S_p / N)^T,
// which is sum (I - mean I)(p - mean p)^T without a second pass over the window.
// The scalar by ticket_sum_256 (csrc/ticket_sum.h): every thread reaches it, no kernel below returns early.  A gradient value
// of exactly 0 is not added: the element of gimg keeps its bits, a -0.0 included.
#include "internal.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

#define MATTING_TILE 16           // pixels per tile side: 256 threads, one per pixel of the tile

__host__ __device__ inline int clip_lo(int x, int r) { return x - r > 0 ? x - r : 0; }
__host__ __device__ inline int clip_hi(int x, int r, int n) { return x + r < n - 1 ? x + r : n - 1; }

__global__ __launch_bounds__(256) void matting_prepare_kernel(const float* __restrict__ guide, int h, int w, int r, double eps,
                                                              float* __restrict__ stats) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long hw = (long long)h * w;
  if (k >= hw) return;
  const int y = (int)(k / w), x = (int)(k - (long long)y * w);
  const int y0 = clip_lo(y, r), y1 = clip_hi(y, r, h), x0 = clip_lo(x, r), x1 = clip_hi(x, r, w);
  const double n = (double)((y1 - y0 + 1) * (x1 - x0 + 1));
  double m0 = 0., m1 = 0., m2 = 0.;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) {
      const float* g = guide + ((size_t)yy * w + xx) * 3;
      m0 += (double)g[0];
      m1 += (double)g[1];
      m2 += (double)g[2];
    }
  m0 /= n;
  m1 /= n;
  m2 /= n;
  double s00 = 0., s01 = 0., s02 = 0., s11 = 0., s12 = 0., s22 = 0.;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) {
      const float* g = guide + ((size_t)yy * w + xx) * 3;
      const double d0 = (double)g[0] - m0, d1 = (double)g[1] - m1, d2 = (double)g[2] - m2;
      s00 += d0 * d0;
      s01 += d0 * d1;
      s02 += d0 * d2;
      s11 += d1 * d1;
      s12 += d1 * d2;
      s22 += d2 * d2;
    }
  s00 = s00 / n + eps;
  s01 = s01 / n;
  s02 = s02 / n;
  s11 = s11 / n + eps;
  s12 = s12 / n;
  s22 = s22 / n + eps;
  const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
  const double c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
  const double det = s00 * c00 + s01 * c01 + s02 * c02;
  float* o = stats + k;
  o[0] = (float)m0;
  o[hw] = (float)m1;
  o[2 * hw] = (float)m2;
  o[3 * hw] = (float)(c00 / det);
  o[4 * hw] = (float)(c01 / det);
  o[5 * hw] = (float)(c02 / det);
  o[6 * hw] = (float)(c11 / det);
  o[7 * hw] = (float)(c12 / det);
  o[8 * hw] = (float)(c22 / det);
}

template <int R>
struct MattingTile {
  static constexpr int T = MATTING_TILE;
  static constexpr int XW = T + 4 * R;            // I, p: the tile and a 2R halo
  static constexpr int AW = T + 2 * R;            // a, b: the tile and an R halo
  static constexpr int X_FLOATS = XW * XW * 3;    // one of I, p
  static constexpr int H_FLOATS = AW * T * 12;    // the row sums of a, b: in the place of I and p
  static constexpr int R0_FLOATS = 2 * X_FLOATS > H_FLOATS ? 2 * X_FLOATS : H_FLOATS;
  static constexpr int AB_FLOATS = AW * AW * 12;  // a (c major: a[c][j] at 3 c + j), b at 9 + c; later the column sums
};

template <int R>
__global__ __launch_bounds__(256) void matting_fwd_bwd_kernel(const float* __restrict__ img, const float* __restrict__ guide,
                                                              const float* __restrict__ stats, int h, int w, int nbx, float coef,
                                                              float inv_n, float* __restrict__ gimg, float* __restrict__ loss_out,
                                                              unsigned* __restrict__ ticket, float* __restrict__ partials) {
  typedef MattingTile<R> M;
  constexpr int T = M::T, XW = M::XW, AW = M::AW;
  __shared__ float region0[M::R0_FLOATS];
  __shared__ float ab[M::AB_FLOATS];
  __shared__ float red[4][1];
  __shared__ int is_last;
  float* Is = region0;
  float* Ps = region0 + M::X_FLOATS;
  float* H = region0;
  const int t = threadIdx.x;
  const int r0 = (int)(blockIdx.x / nbx) * T, s0 = (int)(blockIdx.x % nbx) * T;      // the tile's first pixel
  const size_t hw = (size_t)h * w;
  for (int k = t; k < M::X_FLOATS; k += 256) {
    const int px = k / 3;
    const int ly = px / XW, lx = px - ly * XW;
    const int y = r0 - 2 * R + ly, x = s0 - 2 * R + lx;
    float vi = 0.f, vp = 0.f;
    if (y >= 0 && y < h && x >= 0 && x < w) {
      const size_t o = ((size_t)y * w + x) * 3 + (k - 3 * px);
      vi = guide[o];
      vp = img[o];
    }
    Is[k] = vi;
    Ps[k] = vp;
  }
  __syncthreads();
  for (int k = t; k < AW * AW; k += 256) {
    const int ly = k / AW, lx = k - ly * AW;
    const int y = r0 - R + ly, x = s0 - R + lx;
    float o[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) o[j] = 0.f;
    if (y >= 0 && y < h && x >= 0 && x < w) {
      const float* st = stats + (size_t)y * w + x;
      const float mu0 = st[0], mu1 = st[hw], mu2 = st[2 * hw];
      const float* pk = Ps + ((ly + R) * XW + (lx + R)) * 3;
      const float pk0 = pk[0], pk1 = pk[1], pk2 = pk[2];
      float sI0 = 0.f, sI1 = 0.f, sI2 = 0.f, sp0 = 0.f, sp1 = 0.f, sp2 = 0.f;
      float c00 = 0.f, c01 = 0.f, c02 = 0.f, c10 = 0.f, c11 = 0.f, c12 = 0.f, c20 = 0.f, c21 = 0.f, c22 = 0.f;   // c[j][c]
      for (int dy = 0; dy <= 2 * R; ++dy) {
        const int yy = y - R + dy;
        if (yy < 0 || yy >= h) continue;
#pragma unroll
        for (int dx = 0; dx <= 2 * R; ++dx) {
          const int xx = x - R + dx;
          if (xx < 0 || xx >= w) continue;
          const int q = ((ly + dy) * XW + (lx + dx)) * 3;
          const float d0 = Is[q] - mu0, d1 = Is[q + 1] - mu1, d2 = Is[q + 2] - mu2;
          const float e0 = Ps[q] - pk0, e1 = Ps[q + 1] - pk1, e2 = Ps[q + 2] - pk2;
          sI0 += d0; sI1 += d1; sI2 += d2;
          sp0 += e0; sp1 += e1; sp2 += e2;
          c00 += d0 * e0; c01 += d0 * e1; c02 += d0 * e2;
          c10 += d1 * e0; c11 += d1 * e1; c12 += d1 * e2;
          c20 += d2 * e0; c21 += d2 * e1; c22 += d2 * e2;
        }
      }
      const float n = (float)((clip_hi(y, R, h) - clip_lo(y, R) + 1) * (clip_hi(x, R, w) - clip_lo(x, R) + 1));
      const float mp0 = sp0 / n, mp1 = sp1 / n, mp2 = sp2 / n;
      const float s00 = st[3 * hw], s01 = st[4 * hw], s02 = st[5 * hw], s11 = st[6 * hw], s12 = st[7 * hw], s22 = st[8 * hw];
      const float mp[3] = {mp0, mp1, mp2}, pkc[3] = {pk0, pk1, pk2};
      const float cj0[3] = {c00, c01, c02}, cj1[3] = {c10, c11, c12}, cj2[3] = {c20, c21, c22};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v0 = (cj0[c] - sI0 * mp[c]) / n, v1 = (cj1[c] - sI1 * mp[c]) / n, v2 = (cj2[c] - sI2 * mp[c]) / n;
        const float a0 = (s00 * v0 + s01 * v1) + s02 * v2;
        const float a1 = (s01 * v0 + s11 * v1) + s12 * v2;
        const float a2 = (s02 * v0 + s12 * v1) + s22 * v2;
        o[3 * c] = a0;
        o[3 * c + 1] = a1;
        o[3 * c + 2] = a2;
        o[9 + c] = (pkc[c] + mp[c]) - ((a0 * mu0 + a1 * mu1) + a2 * mu2);
      }
    }
#pragma unroll
    for (int j = 0; j < 12; ++j) ab[k * 12 + j] = o[j];
  }
  __syncthreads();
  // row sums, left to right: (AW rows) x (T columns) x 12, into the place of I and p
  for (int e = t; e < M::H_FLOATS; e += 256) {
    const int comp = e % 12, rest = e / 12;
    const int tx = rest % T, ly = rest / T;
    const float* src = ab + (ly * AW + tx) * 12 + comp;
    float acc = src[0];
#pragma unroll
    for (int d = 1; d <= 2 * R; ++d) acc += src[d * 12];
    H[e] = acc;
  }
  __syncthreads();
  // column sums, top to bottom: (T x T) x 12, into the place of a and b
  for (int e = t; e < T * T * 12; e += 256) {
    const float* src = H + e;                     // e = ((ty T + tx) 12 + comp): row ty + d is d T 12 further
    float acc = src[0];
#pragma unroll
    for (int d = 1; d <= 2 * R; ++d) acc += src[d * (T * 12)];
    ab[e] = acc;
  }
  __syncthreads();
  float lacc = 0.f;
  const int rows = h - r0 < T ? h - r0 : T, cols = w - s0 < T ? w - s0 : T;
  const int cols3 = 3 * cols;
  for (int k = t; k < rows * cols3; k += 256) {
    const int r = k / cols3, c3 = k - r * cols3;
    const int px = c3 / 3, c = c3 - 3 * px;
    const int y = r0 + r, x = s0 + px;
    const float n = (float)((clip_hi(y, R, h) - clip_lo(y, R) + 1) * (clip_hi(x, R, w) - clip_lo(x, R) + 1));
    const float* v = ab + (r * T + px) * 12;
    const size_t o = ((size_t)y * w + x) * 3;
    const float q = (((v[3 * c] / n) * guide[o] + (v[3 * c + 1] / n) * guide[o + 1]) + (v[3 * c + 2] / n) * guide[o + 2]) +
                    v[9 + c] / n;
    const float p = img[o + c];
    const float d = p - q;
    lacc += (n * p) * d;
    if (coef != 0.f) {
      const float g = coef * (n * d);
      if (g != 0.f) gimg[o + c] = gimg[o + c] + g;
    }
  }
  float sum[1] = {lacc};
  ticket_sum_256(sum, inv_n, loss_out, ticket, partials, red, &is_last);
}

inline long long tiles(int n) { return ((long long)n + MATTING_TILE - 1) / MATTING_TILE; }
inline bool matting_size_ok(int h, int w) { return h > 0 && w > 0 && 3LL * h * w <= 0x7fffffffLL; }

template <int R>
int launch_matting(const float* img, const float* guide, const float* stats, int h, int w, float coef, float inv_n, float* gimg,
                   float* loss_out, void* workspace, hipStream_t st) {
  unsigned* ticket = (unsigned*)workspace;
  float* partials = (float*)((char*)workspace + 16);
  const int nbx = (int)tiles(w);                           // a flat grid: tile rows x tile columns, row-major
  hipLaunchKernelGGL(matting_fwd_bwd_kernel<R>, dim3((unsigned)(tiles(h) * nbx)), dim3(256), 0, st, img, guide, stats, h, w, nbx,
                     coef, inv_n, gimg, loss_out, ticket, partials);
  ST_LAUNCH_RET();
}

}  // namespace

size_t strotss_matting_stats_bytes(int h, int w) {
  if (!matting_size_ok(h, w)) return 0;
  return (size_t)36 * (size_t)h * (size_t)w;
}

int strotss_matting_prepare(const float* guide, int h, int w, int r, float eps, float* stats, void* stream) {
  ST_CHECK_ARG(guide && stats && matting_size_ok(h, w), STROTSS_EINVAL);
  ST_CHECK_ARG(r >= 1 && r <= STROTSS_MATTING_MAX_RADIUS, STROTSS_ERANGE);
  ST_CHECK_ARG(isfinite(eps) && eps >= 1e-4f && eps <= 1.0f, STROTSS_ERANGE);
  ST_CHECK_ARG(aligned16(guide) && aligned16(stats), STROTSS_EALIGN);
  const long long n = (long long)h * w;
  hipLaunchKernelGGL(matting_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, guide, h, w, r,
                     (double)eps, stats);
  ST_LAUNCH_RET();
}

size_t strotss_matting_workspace_bytes(int h, int w) {
  if (!matting_size_ok(h, w)) return 0;
  return 16 + (((size_t)4 * (size_t)(tiles(h) * tiles(w)) + 15) & ~(size_t)15);
}

int strotss_matting_fwd_bwd(const float* img, const float* guide, const float* stats, int h, int w, int r, float gscale,
                            float* gimg, float* loss_out, void* workspace, void* stream) {
  ST_CHECK_ARG(img && guide && stats && gimg && loss_out && workspace && matting_size_ok(h, w), STROTSS_EINVAL);
  ST_CHECK_ARG(r >= 1 && r <= STROTSS_MATTING_MAX_RADIUS, STROTSS_ERANGE);
  ST_CHECK_ARG(aligned16(img) && aligned16(guide) && aligned16(stats) && aligned16(gimg) && aligned16(workspace), STROTSS_EALIGN);
  const double n = 3.0 * (double)h * (double)w;
  const float coef = (float)(2.0 * (double)gscale / n), inv_n = (float)(1.0 / n);
  const hipStream_t st = (hipStream_t)stream;
  switch (r) {
    case 1: return launch_matting<1>(img, guide, stats, h, w, coef, inv_n, gimg, loss_out, workspace, st);
    case 2: return launch_matting<2>(img, guide, stats, h, w, coef, inv_n, gimg, loss_out, workspace, st);
    case 3: return launch_matting<3>(img, guide, stats, h, w, coef, inv_n, gimg, loss_out, workspace, st);
    default: return launch_matting<4>(img, guide, stats, h, w, coef, inv_n, gimg, loss_out, workspace, st);
  }
}
