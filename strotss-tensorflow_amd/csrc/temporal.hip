// Temporal consistency of frame sequences: the short-term temporal loss of Ruder et al. (2016).
//   - flow_warp_kernel: once per frame, the previous stylised frame warped along the backward flow + its {0, 1} certainty;
//   - temporal_multi_fwd_bwd_kernel<N>: once per step (inside the captured graph), for each of the N = 1..4 targets
//     L_t = (1/(3hw)) sum_p c(p) |x(p) - w(p)|^2 and gimg += gscale * dL_t/dx, between the trunk's pixel gradient and the
//     fold adjoint.  N = 1 is the short-term term, N >= 2 the long-term terms of several earlier frames.
//   - temporal_long_certainty_kernel: the long-term certainties, once per frame.
#include "internal.h"

namespace {

// Bilinear taps along one axis, pixel centres at integer coordinates, both neighbours clamped to [0, n-1].  Beyond
// [-2, n+1] every tap is the edge pixel already: clamping there first keeps floor() in int range (a NaN lands on -2).
struct Tap64 { int lo, hi; double f; };
__device__ __forceinline__ Tap64 tap64(double s, int n) {
  s = fmin(fmax(s, -2.0), (double)n + 1.0);
  const double fl = floor(s);
  const int i = (int)fl;
  Tap64 t;
  t.lo = min(max(i, 0), n - 1);
  t.hi = min(max(i + 1, 0), n - 1);
  t.f = s - fl;
  return t;
}

__device__ __forceinline__ double bilerp64(const float* __restrict__ p, int w, int c, int ch, const Tap64& ty,
                                           const Tap64& tx) {
  const double a = p[((size_t)ty.lo * w + tx.lo) * c + ch], b = p[((size_t)ty.lo * w + tx.hi) * c + ch];
  const double d = p[((size_t)ty.hi * w + tx.lo) * c + ch], e = p[((size_t)ty.hi * w + tx.hi) * c + ch];
  return (1.0 - ty.f) * ((1.0 - tx.f) * a + tx.f * b) + ty.f * ((1.0 - tx.f) * d + tx.f * e);
}

// One thread per pixel.  Coordinates, samples and the three certainty tests in float64: the tests compare sums of squares
// against thresholds, and float64 keeps them the tests of the float64 statement (an integer shift warps exactly).
__global__ __launch_bounds__(256) void flow_warp_kernel(const float* __restrict__ prev, int h, int w, int c,
                                                        const float* __restrict__ fb, const float* __restrict__ ff,
                                                        float* __restrict__ warped, float* __restrict__ certainty) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)h * w) return;
  const int y = (int)(p / w), x = (int)(p - (long long)y * w);
  const double u = fb[2 * p], v = fb[2 * p + 1];
  const double sx = x + u, sy = y + v;
  const Tap64 tx = tap64(sx, w), ty = tap64(sy, h);
  for (int ch = 0; ch < c; ++ch) warped[p * c + ch] = (float)bilerp64(prev, w, c, ch, ty, tx);
  // out of frame (a NaN coordinate fails both comparisons: out)
  bool ok = sx >= 0.0 && sx <= (double)(w - 1) && sy >= 0.0 && sy <= (double)(h - 1);
  const double fb2 = u * u + v * v;
  // disoccluded: the forward flow at the warped point does not bring the pixel back
  if (ok && ff) {
    const double wu = bilerp64(ff, w, 2, 0, ty, tx), wv = bilerp64(ff, w, 2, 1, ty, tx);
    const double su = u + wu, sv = v + wv;
    if (su * su + sv * sv > 0.01 * (fb2 + wu * wu + wv * wv) + 0.5) ok = false;
  }
  // motion boundary: central differences of the backward flow, indices clamped
  if (ok) {
    const int xm = max(x - 1, 0), xp = min(x + 1, w - 1), ym = max(y - 1, 0), yp = min(y + 1, h - 1);
    const size_t rm = (size_t)y * w, ra = (size_t)ym * w, rb = (size_t)yp * w;
    const double ux = ((double)fb[2 * (rm + xp)] - (double)fb[2 * (rm + xm)]) * 0.5;
    const double vx = ((double)fb[2 * (rm + xp) + 1] - (double)fb[2 * (rm + xm) + 1]) * 0.5;
    const double uy = ((double)fb[2 * (rb + x)] - (double)fb[2 * (ra + x)]) * 0.5;
    const double vy = ((double)fb[2 * (rb + x) + 1] - (double)fb[2 * (ra + x) + 1]) * 0.5;
    if ((ux * ux + uy * uy) + (vx * vx + vy * vy) > 0.01 * fb2 + 0.002) ok = false;
  }
  certainty[p] = ok ? 1.f : 0.f;
}

#define TEMPORAL_PIX_PER_BLOCK 1024

// Long-term certainties, once per frame, one thread per pixel: plane j keeps only what the nearer
// planes k < j do not already cover, the covered amount summed in ascending k in float32.
__global__ __launch_bounds__(256) void temporal_long_certainty_kernel(const float* __restrict__ raw, int count, int npix,
                                                                      float* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  float c[STROTSS_MAX_TEMPORAL];
#pragma unroll
  for (int j = 0; j < STROTSS_MAX_TEMPORAL; ++j) c[j] = j < count ? raw[(size_t)j * npix + p] : 0.f;
  float covered = 0.f;
#pragma unroll
  for (int j = 0; j < STROTSS_MAX_TEMPORAL; ++j) {
    if (j < count) out[(size_t)j * npix + p] = fmaxf(c[j] - covered, 0.f);
    covered += c[j];
  }
}

// The temporal terms of N targets in one launch.  One workgroup per 1024 pixels = 3072 floats = 768 float4 of x, of every
// target and of the gradient: thread t takes float4 t, t + 256 and t + 512 of each (coalesced; every global load of the
// thread in flight at once: a grid of a few waves per SIMD, latency, not bandwidth, bounds it), the block's N x 1024
// certainties staged in LDS first (element e of the block belongs to pixel e / 3), x and gimg read once.  The last block,
// if partial, goes element by element.  Per element the N terms are added to the gradient in ascending j; c_j(p) == 0 or
// gscale_j == 0 adds nothing, and an element that no term touches keeps its bits (the unchanged value is stored back, or
// nothing at all).  The N scalars: per-thread sums in a fixed element order, then ticket_sum_256 (csrc/ticket_sum.h).
template <int N>
struct TemporalSetArgs {
  const float* tgt[N];
  const float* cert[N];
  float coef[N];
};

template <int N>
__global__ __launch_bounds__(256) void temporal_multi_fwd_bwd_kernel(const float* __restrict__ img, TemporalSetArgs<N> s,
                                                                     int npix, float inv_n, float* __restrict__ gimg,
                                                                     float* __restrict__ loss_out,
                                                                     unsigned* __restrict__ ticket,
                                                                     float* __restrict__ partials) {
  __shared__ float cs[N][TEMPORAL_PIX_PER_BLOCK];
  __shared__ float red[4][N];
  __shared__ int is_last;
  const int t = threadIdx.x;
  const int base = blockIdx.x * TEMPORAL_PIX_PER_BLOCK;
  const int count = min(TEMPORAL_PIX_PER_BLOCK, npix - base);
  const bool full = count == TEMPORAL_PIX_PER_BLOCK;
  const size_t f0 = 3 * (size_t)base;
  bool any_coef = false;
#pragma unroll
  for (int j = 0; j < N; ++j) any_coef = any_coef || s.coef[j] != 0.f;
  float acc[N];
#pragma unroll
  for (int j = 0; j < N; ++j) acc[j] = 0.f;
  if (full) {
    const f32x4* x4 = reinterpret_cast<const f32x4*>(img + f0);
    f32x4* g4 = reinterpret_cast<f32x4*>(gimg + f0);
    f32x4 xv[3], yv[N][3], gv[3] = {}, c4[N];
#pragma unroll
    for (int j = 0; j < N; ++j) c4[j] = reinterpret_cast<const f32x4*>(s.cert[j] + base)[t];
#pragma unroll
    for (int k = 0; k < 3; ++k) xv[k] = x4[t + 256 * k];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const f32x4* y4 = reinterpret_cast<const f32x4*>(s.tgt[j] + f0);
#pragma unroll
      for (int k = 0; k < 3; ++k) yv[j][k] = y4[t + 256 * k];
    }
    if (any_coef) {
#pragma unroll
      for (int k = 0; k < 3; ++k) gv[k] = g4[t + 256 * k];
    }
#pragma unroll
    for (int j = 0; j < N; ++j) reinterpret_cast<f32x4*>(cs[j])[t] = c4[j];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const f32x4 d = xv[k] - yv[j][k];
        const float coef = s.coef[j];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float ce = cs[j][(4 * (t + 256 * k) + e) / 3];
          acc[j] += ce * (d[e] * d[e]);
          gv[k][e] = ce != 0.f && coef != 0.f ? gv[k][e] + (coef * ce) * d[e] : gv[k][e];
        }
      }
    }
    if (any_coef) {
#pragma unroll
      for (int k = 0; k < 3; ++k) g4[t + 256 * k] = gv[k];
    }
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j)
      for (int p = t; p < count; p += 256) cs[j][p] = s.cert[j][base + p];
    __syncthreads();
    for (int i = t; i < 3 * count; i += 256) {
      const float x = img[f0 + i];
      float g = any_coef ? gimg[f0 + i] : 0.f;
      bool touched = false;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const float ce = cs[j][i / 3], d = x - s.tgt[j][f0 + i];
        acc[j] += ce * (d * d);
        if (s.coef[j] != 0.f && ce != 0.f) {
          g += (s.coef[j] * ce) * d;
          touched = true;
        }
      }
      if (touched) gimg[f0 + i] = g;
    }
  }
  ticket_sum_256(acc, inv_n, loss_out, ticket, partials, red, &is_last);
}

inline long long temporal_blocks(int h, int w) {
  return ((long long)h * w + TEMPORAL_PIX_PER_BLOCK - 1) / TEMPORAL_PIX_PER_BLOCK;
}

template <int N>
void launch_temporal_multi(const float* img, const strotss_temporal_set_t* set, int h, int w, float* gimg, float* loss_out,
                           void* workspace, hipStream_t stream) {
  const double n = 3.0 * (double)h * (double)w;
  TemporalSetArgs<N> a;
  for (int j = 0; j < N; ++j) {
    a.tgt[j] = set->target[j];
    a.cert[j] = set->certainty[j];
    a.coef[j] = (float)(2.0 * (double)set->gscale[j] / n);
  }
  unsigned* ticket = (unsigned*)workspace;
  float* partials = (float*)((char*)workspace + 16);
  hipLaunchKernelGGL(temporal_multi_fwd_bwd_kernel<N>, dim3((unsigned)temporal_blocks(h, w)), dim3(256), 0, stream, img, a,
                     h * w, (float)(1.0 / n), gimg, loss_out, ticket, partials);
}

// Both entries, their arguments checked: set->count in 1 .. STROTSS_MAX_TEMPORAL picks the instantiation.
int launch_temporal(const float* img, const strotss_temporal_set_t* set, int h, int w, float* gimg, float* loss_out,
                    void* workspace, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  if (set->count == 1) launch_temporal_multi<1>(img, set, h, w, gimg, loss_out, workspace, st);
  else if (set->count == 2) launch_temporal_multi<2>(img, set, h, w, gimg, loss_out, workspace, st);
  else if (set->count == 3) launch_temporal_multi<3>(img, set, h, w, gimg, loss_out, workspace, st);
  else launch_temporal_multi<4>(img, set, h, w, gimg, loss_out, workspace, st);
  ST_LAUNCH_RET();
}

}  // namespace

int strotss_flow_warp(const float* prev, int h, int w, int c, const float* flow_b, const float* flow_f, float* warped,
                      float* certainty, void* stream) {
  ST_CHECK_ARG(prev && flow_b && warped && certainty && h > 0 && w > 0 && c > 0, STROTSS_EINVAL);
  const long long npix = (long long)h * w;
  ST_CHECK_ARG(npix * c <= (1LL << 40), STROTSS_EINVAL);
  hipLaunchKernelGGL(flow_warp_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, prev, h, w,
                     c, flow_b, flow_f, warped, certainty);
  ST_LAUNCH_RET();
}

size_t strotss_temporal_workspace_bytes(int h, int w) { return strotss_temporal_multi_workspace_bytes(h, w, 1); }

int strotss_temporal_fwd_bwd(const float* img, const float* target, const float* certainty, int h, int w, float gscale,
                             float* gimg, float* loss_out, void* workspace, void* stream) {
  ST_CHECK_ARG(img && target && certainty && gimg && loss_out && workspace && h > 0 && w > 0, STROTSS_EINVAL);
  ST_CHECK_ARG(3LL * h * w <= 0x7fffffffLL, STROTSS_EINVAL);
  ST_CHECK_ARG(aligned16(img) && aligned16(target) && aligned16(certainty) && aligned16(gimg) && aligned16(workspace),
               STROTSS_EALIGN);
  strotss_temporal_set_t set = {};
  set.count = 1;
  set.target[0] = target;
  set.certainty[0] = certainty;
  set.gscale[0] = gscale;
  return launch_temporal(img, &set, h, w, gimg, loss_out, workspace, stream);
}

int strotss_temporal_long_certainty(const float* raw, int count, int h, int w, float* out, void* stream) {
  ST_CHECK_ARG(raw && out && h > 0 && w > 0 && count >= 1 && count <= STROTSS_MAX_TEMPORAL, STROTSS_EINVAL);
  const long long npix = (long long)h * w;
  ST_CHECK_ARG(3 * npix <= 0x7fffffffLL, STROTSS_EINVAL);
  ST_CHECK_ARG(aligned16(raw) && aligned16(out), STROTSS_EALIGN);
  hipLaunchKernelGGL(temporal_long_certainty_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, raw, count, (int)npix, out);
  ST_LAUNCH_RET();
}

size_t strotss_temporal_multi_workspace_bytes(int h, int w, int count) {
  if (h <= 0 || w <= 0 || count < 1 || count > STROTSS_MAX_TEMPORAL) return 0;
  return 16 + 4 * (size_t)count * (size_t)temporal_blocks(h, w);
}

int strotss_temporal_multi_fwd_bwd(const float* img, const strotss_temporal_set_t* set, int h, int w, float* gimg,
                                   float* loss_out, void* workspace, void* stream) {
  ST_CHECK_ARG(img && set && gimg && loss_out && workspace && h > 0 && w > 0, STROTSS_EINVAL);
  const int count = set->count;
  ST_CHECK_ARG(count >= 1 && count <= STROTSS_MAX_TEMPORAL, STROTSS_EINVAL);
  for (int j = 0; j < count; ++j) ST_CHECK_ARG(set->target[j] && set->certainty[j], STROTSS_EINVAL);
  ST_CHECK_ARG(3LL * h * w <= 0x7fffffffLL, STROTSS_EINVAL);
  ST_CHECK_ARG(aligned16(img) && aligned16(gimg) && aligned16(workspace), STROTSS_EALIGN);
  for (int j = 0; j < count; ++j) ST_CHECK_ARG(aligned16(set->target[j]) && aligned16(set->certainty[j]), STROTSS_EALIGN);
  return launch_temporal(img, set, h, w, gimg, loss_out, workspace, stream);
}
