// Dense optical flow between two frames: coarse-to-fine Horn-Schunck with warping, solved by Jacobi
// iterations (Meinhardt-Llopis, Sanchez, Kondermann, IPOL 2013, with Jacobi in place of SOR: no sweep order, no atomics,
// the same bits on every run).  The producer of the flows strotss_flow_warp consumes.
//   - flow_blur_kernel: grey + 5 x 5 binomial blur of a frame (level 0), or blur + 2 x 2 decimation of a level;
//   - flow_upsample_kernel: (u, v) of a coarser level at the next finer one (zeros at the coarsest);
//   - flow_coef_kernel: once per warp, B warped along (u, v), its gradients and the linearised data term: Ix, Iy, c, inv;
//   - flow_jacobi_kernel: one Jacobi sweep per launch, one thread per pixel (the plain form);
//   - flow_jacobi_blocked_kernel<K>: K sweeps per launch on a 64 x 32 tile + a halo of K pixels held in LDS;
//   - flow_pack_kernel: (u, v) planes -> (h, w, 2).
// strotss_optical_flow_match adds flow_match.hip's stage between a level's upsample and its warps;
// strotss_optical_flow_robust replaces a warp's sweeps by flow_robust.hip's weight updates and weighted sweeps.
// Both solver forms call hs_update, so they agree bit for bit.
#include <algorithm>
#include <cmath>

#include "internal.h"

namespace {

// Bilinear taps along one axis (tap64 of temporal.hip in float32): pixel centres at integer coordinates, both neighbours
// clamped to [0, n-1]; s clamped to [-2, n+1] first (every tap beyond is the edge pixel already, a NaN lands on -2).
struct Tap { int lo, hi; float f; };
__device__ __forceinline__ Tap tap32(float s, int n) {
  s = fminf(fmaxf(s, -2.f), (float)(n + 1));
  const float fl = floorf(s);
  const int i = (int)fl;
  Tap t;
  t.lo = min(max(i, 0), n - 1);
  t.hi = min(max(i + 1, 0), n - 1);
  t.f = s - fl;
  return t;
}

__device__ __forceinline__ float bilerp32(const float* __restrict__ p, int w, const Tap& ty, const Tap& tx) {
  const float a = p[(size_t)ty.lo * w + tx.lo], b = p[(size_t)ty.lo * w + tx.hi];
  const float d = p[(size_t)ty.hi * w + tx.lo], e = p[(size_t)ty.hi * w + tx.hi];
  return (1.f - ty.f) * ((1.f - tx.f) * a + tx.f * b) + ty.f * ((1.f - tx.f) * d + tx.f * e);
}

__device__ __forceinline__ int clampi(int v, int n) { return min(max(v, 0), n - 1); }

__device__ __forceinline__ float binomial5(float a, float b, float c, float d, float e) {
  return (a + e + 4.f * (b + d) + 6.f * c) * 0.0625f;
}

// out(oy, ox) = blur(src)(oy * stride, ox * stride), blur = [1 4 6 4 1] / 16 along x, then along y, indices clamped; one
// thread per output pixel recomputes the five row sums it needs (25 taps from cache: the pyramids are built once per flow).
// RGB: src is a (h, w, 3) frame and the blurred image is its grey 0.299 R + 0.587 G + 0.114 B.
template <bool RGB>
__global__ __launch_bounds__(256) void flow_blur_kernel(const float* __restrict__ src, int h, int w, float* __restrict__ out,
                                                        int oh, int ow, int stride) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= oh * ow) return;
  const int oy = p / ow, ox = p - oy * ow;
  const int y = oy * stride, x = ox * stride;
  float row[5];
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const size_t r = (size_t)clampi(y + dy, h) * w;
    float g[5];
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const size_t q = r + clampi(x + dx, w);
      g[dx + 2] = RGB ? 0.299f * src[3 * q] + 0.587f * src[3 * q + 1] + 0.114f * src[3 * q + 2] : src[q];
    }
    row[dy + 2] = binomial5(g[0], g[1], g[2], g[3], g[4]);
  }
  out[p] = binomial5(row[0], row[1], row[2], row[3], row[4]);
}

// (u', v')(y, x) = 2 * bilinear((u, v), x / 2, y / 2) at the finer level's size (h, w); u == nullptr: zeros (the coarsest level)
__global__ __launch_bounds__(256) void flow_upsample_kernel(const float* __restrict__ u, const float* __restrict__ v, int ch,
                                                            int cw, float* __restrict__ uo, float* __restrict__ vo, int h,
                                                            int w) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h * w) return;
  if (!u) {
    uo[p] = 0.f;
    vo[p] = 0.f;
    return;
  }
  const int y = p / w, x = p - y * w;
  const Tap tx = tap32(0.5f * (float)x, cw), ty = tap32(0.5f * (float)y, ch);
  uo[p] = 2.f * bilerp32(u, cw, ty, tx);
  vo[p] = 2.f * bilerp32(v, cw, ty, tx);
}

__device__ __forceinline__ float warped_b(const float* __restrict__ b, const float* __restrict__ u,
                                          const float* __restrict__ v, int h, int w, int y, int x) {
  const size_t p = (size_t)y * w + x;
  return bilerp32(b, w, tap32((float)y + v[p], h), tap32((float)x + u[p], w));
}

// One warp's coefficients, one thread per pixel: Bw = B sampled at p + (u, v) (here and at the 4 clamped neighbours: the
// same expression, so the same bits as a stored Bw), Ix, Iy its central differences, c = Bw - A - Ix u - Iy v,
// inv = 1 / (alpha2 + Ix^2 + Iy^2) -> coef(y, x) = {Ix, Iy, c, inv}.
__global__ __launch_bounds__(256) void flow_coef_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        const float* __restrict__ u, const float* __restrict__ v, int h,
                                                        int w, float alpha2, f32x4* __restrict__ coef) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h * w) return;
  const int y = p / w, x = p - y * w;
  const float bw = warped_b(b, u, v, h, w, y, x);
  const float ix = (warped_b(b, u, v, h, w, y, min(x + 1, w - 1)) - warped_b(b, u, v, h, w, y, max(x - 1, 0))) * 0.5f;
  const float iy = (warped_b(b, u, v, h, w, min(y + 1, h - 1), x) - warped_b(b, u, v, h, w, max(y - 1, 0), x)) * 0.5f;
  const float up = u[p], vp = v[p];
  f32x4 c4;
  c4[0] = ix;
  c4[1] = iy;
  c4[2] = bw - a[p] - ix * up - iy * vp;
  c4[3] = 1.f / (alpha2 + ix * ix + iy * iy);
  coef[p] = c4;
}

// The Jacobi update of one pixel from its 8 neighbours (un[0..3] = N, S, W, E; ud[0..3] = NW, NE, SW, SE; v likewise):
//   ub = (N + S + W + E) / 6 + (NW + NE + SW + SE) / 12,  t = (Ix ub + Iy vb + c) inv,  u <- ub - Ix t,  v <- vb - Iy t.
// The one statement of the sweep: both solver kernels call it, so they contract alike and agree bit for bit.
__device__ __forceinline__ void hs_update(const float un[4], const float ud[4], const float vn[4], const float vd[4],
                                          const f32x4 k, float& uo, float& vo) {
  const float ub = (un[0] + un[1] + un[2] + un[3]) / 6.f + (ud[0] + ud[1] + ud[2] + ud[3]) / 12.f;
  const float vb = (vn[0] + vn[1] + vn[2] + vn[3]) / 6.f + (vd[0] + vd[1] + vd[2] + vd[3]) / 12.f;
  const float t = (k[0] * ub + k[1] * vb + k[2]) * k[3];
  uo = ub - k[0] * t;
  vo = vb - k[1] * t;
}

// The plain form: one sweep, one thread per pixel, neighbours from global memory with clamped indices.
__global__ __launch_bounds__(256) void flow_jacobi_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                          const f32x4* __restrict__ coef, int h, int w,
                                                          float* __restrict__ uo, float* __restrict__ vo) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h * w) return;
  const int y = p / w, x = p - y * w;
  const int xm = max(x - 1, 0), xp = min(x + 1, w - 1);
  const size_t rn = (size_t)max(y - 1, 0) * w, rs = (size_t)min(y + 1, h - 1) * w, rc = (size_t)y * w;
  const float un[4] = {u[rn + x], u[rs + x], u[rc + xm], u[rc + xp]};
  const float ud[4] = {u[rn + xm], u[rn + xp], u[rs + xm], u[rs + xp]};
  const float vn[4] = {v[rn + x], v[rs + x], v[rc + xm], v[rc + xp]};
  const float vd[4] = {v[rn + xm], v[rn + xp], v[rs + xm], v[rs + xp]};
  hs_update(un, ud, vn, vd, coef[p], uo[p], vo[p]);
}

// The temporally blocked form: K sweeps per launch.  One workgroup owns FLOW_TW x FLOW_TH output pixels and holds (u, v)
// of the tile + a halo of K pixels in LDS, double-buffered; thread t owns the pixels t, t + 256, ... of that extended
// region and keeps their {Ix, Iy, c, inv} in registers across the sweeps.  Sweep s = 1 .. K updates the pixels at least s
// rings inside the extended region (their neighbours, one ring further out, hold sweep s-1), so after K sweeps the tile
// itself is right.  The image edge is clamped by INDEX inside the region: a pixel outside the image is never loaded,
// computed or read -- its in-image neighbour is read in its place, as flow_jacobi_kernel reads it.
// LDS: 4 * (64 + 2K) * (32 + 2K) floats = 60 KiB at K = 8 (two workgroups per CU); 3840 pixels updated per 2048 written:
// 1.875 x the plain form's arithmetic for 1/8 of its launches and global round trips.
#define FLOW_TW 64
#define FLOW_TH 32
template <int K>
__global__ __launch_bounds__(256) void flow_jacobi_blocked_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                                  const f32x4* __restrict__ coef, int h, int w,
                                                                  float* __restrict__ uo, float* __restrict__ vo) {
  constexpr int EW = FLOW_TW + 2 * K, EH = FLOW_TH + 2 * K, NPIX = EW * EH, PER = (NPIX + 255) / 256;
  __shared__ float su[2][NPIX];
  __shared__ float sv[2][NPIX];
  const int x0 = blockIdx.x * FLOW_TW - K, y0 = blockIdx.y * FLOW_TH - K;      // the extended region's corner in the image
  // per owned pixel: its coefficients and, packed, its ring (0 = outermost; -1 = not in the image or not a pixel) and
  // whether its W / E / N / S neighbour exists in the image
  f32x4 k[PER];
  int meta[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int e = threadIdx.x + 256 * i;
    const int ey = e / EW, ex = e - ey * EW;
    const int gx = x0 + ex, gy = y0 + ey;
    const bool in = e < NPIX && gx >= 0 && gx < w && gy >= 0 && gy < h;
    k[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    meta[i] = -1;
    if (in) {
      const size_t g = (size_t)gy * w + gx;
      k[i] = coef[g];
      su[0][e] = u[g];
      sv[0][e] = v[g];
      const int ring = min(min(ex, EW - 1 - ex), min(ey, EH - 1 - ey));
      meta[i] = ring | (gx > 0 ? 256 : 0) | (gx < w - 1 ? 512 : 0) | (gy > 0 ? 1024 : 0) | (gy < h - 1 ? 2048 : 0);
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int s = 1; s <= K; ++s) {
    const float* __restrict__ ru = su[(s - 1) & 1];
    const float* __restrict__ rv = sv[(s - 1) & 1];
    float* __restrict__ wu = su[s & 1];
    float* __restrict__ wv = sv[s & 1];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int m = meta[i];
      if (m < 0 || (m & 255) < s) continue;
      const int e = threadIdx.x + 256 * i;
      const int xm = e - ((m >> 8) & 1), xp = e + ((m >> 9) & 1);
      const int dn = (m & 1024) ? EW : 0, ds = (m & 2048) ? EW : 0;
      const float un[4] = {ru[e - dn], ru[e + ds], ru[xm], ru[xp]};
      const float ud[4] = {ru[xm - dn], ru[xp - dn], ru[xm + ds], ru[xp + ds]};
      const float vn[4] = {rv[e - dn], rv[e + ds], rv[xm], rv[xp]};
      const float vd[4] = {rv[xm - dn], rv[xp - dn], rv[xm + ds], rv[xp + ds]};
      hs_update(un, ud, vn, vd, k[i], wu[e], wv[e]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int m = meta[i];
    if (m < 0 || (m & 255) < K) continue;           // the tile = the pixels K rings inside
    const int e = threadIdx.x + 256 * i;
    const int ey = e / EW, ex = e - ey * EW;
    const size_t g = (size_t)(y0 + ey) * w + (x0 + ex);
    uo[g] = su[K & 1][e];
    vo[g] = sv[K & 1][e];
  }
}

__global__ __launch_bounds__(256) void flow_pack_kernel(const float* __restrict__ u, const float* __restrict__ v, int npix,
                                                        float* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  out[2 * (size_t)p] = u[p];
  out[2 * (size_t)p + 1] = v[p];
}


const strotss_flow_params_t kFlowDefaults = {0.01f, 5, 32, 12, 8, 8};

// params == NULL: the defaults with the solver form that measured faster at the size (the blocked
// form wins at 48 x 64, 1.35 against 1.55 ms, and loses at 192 x 256 and 768 x 1024, where its few large workgroups leave
// most of the chip idle).  Either choice gives the same bits.
#define FLOW_BLOCKED_MAX_PIXELS 4096
strotss_flow_params_t flow_params_or_default(const strotss_flow_params_t* params, int h, int w) {
  if (params) return *params;
  strotss_flow_params_t p = kFlowDefaults;
  if ((long long)h * w > FLOW_BLOCKED_MAX_PIXELS) p.iters_per_launch = 1;
  return p;
}

bool flow_params_ok(const strotss_flow_params_t& p) {
  const int k = p.iters_per_launch;
  return std::isfinite(p.alpha2) && p.alpha2 > 0.f && p.warps >= 1 && p.iters >= 1 && p.min_side >= 1 &&
         p.max_levels >= 1 && p.max_levels <= STROTSS_MAX_LEVELS && (k == 1 || k == 2 || k == 4 || k == 8) &&
         p.iters % k == 0;
}

struct FlowLevels {
  int n;
  int h[STROTSS_MAX_LEVELS], w[STROTSS_MAX_LEVELS];
};

FlowLevels flow_levels(int h, int w, const strotss_flow_params_t& p) {
  FlowLevels l;
  l.n = 1;
  l.h[0] = h;
  l.w[0] = w;
  while (std::min(l.h[l.n - 1], l.w[l.n - 1]) / 2 >= p.min_side && l.n < p.max_levels) {
    l.h[l.n] = (l.h[l.n - 1] + 1) / 2;
    l.w[l.n] = (l.w[l.n - 1] + 1) / 2;
    ++l.n;
  }
  return l;
}

struct FlowBuffers {
  float* a[STROTSS_MAX_LEVELS];
  float* b[STROTSS_MAX_LEVELS];
  float* u[2];
  float* v[2];
  f32x4* coef;
  float* s;                                             // the robust form's planes (flow_robust.hip): s (h, w), gk (h, w, 2)
  float* gk;
};

// The workspace: both pyramids, the (u, v) ping-pong and the coefficients at the full size (the coarser levels reuse them);
// robust: behind them, the weight planes at the full size.
bool flow_carve(Workspace& ws, const FlowLevels& l, FlowBuffers& f, bool robust = false) {
  for (int k = 0; k < l.n; ++k) {
    f.a[k] = ws.take<float>((size_t)l.h[k] * l.w[k]);
    f.b[k] = ws.take<float>((size_t)l.h[k] * l.w[k]);
  }
  const size_t npix = (size_t)l.h[0] * l.w[0];
  for (int i = 0; i < 2; ++i) {
    f.u[i] = ws.take<float>(npix);
    f.v[i] = ws.take<float>(npix);
  }
  f.coef = ws.take<f32x4>(npix);
  f.s = robust ? ws.take<float>(npix) : nullptr;
  f.gk = robust ? ws.take<float>(2 * npix) : nullptr;
  return ws.ok();
}

inline dim3 per_pixel(int h, int w) { return dim3((unsigned)(((long long)h * w + 255) / 256)); }

template <int K>
void launch_blocked(const FlowBuffers& f, int cur, int h, int w, hipStream_t st) {
  hipLaunchKernelGGL(flow_jacobi_blocked_kernel<K>, dim3((w + FLOW_TW - 1) / FLOW_TW, (h + FLOW_TH - 1) / FLOW_TH), dim3(256),
                     0, st, f.u[cur], f.v[cur], f.coef, h, w, f.u[cur ^ 1], f.v[cur ^ 1]);
}

}  // namespace

void strotss_flow_default_params(strotss_flow_params_t* out) {
  if (out) *out = kFlowDefaults;
}

size_t strotss_flow_workspace_bytes(int h, int w, const strotss_flow_params_t* params) {
  const strotss_flow_params_t p = flow_params_or_default(params, h, w);
  if (h < 2 || w < 2 || (long long)h * w > (1LL << 28) || !flow_params_ok(p)) return 0;
  Workspace plan = Workspace::planner();
  FlowBuffers f;
  flow_carve(plan, flow_levels(h, w, p), f);
  return plan.off;
}

int strotss_optical_flow(const float* frame_a, const float* frame_b, int h, int w, const strotss_flow_params_t* params,
                         float* flow_out, void* workspace, size_t workspace_bytes, void* stream) {
  return strotss_optical_flow_match(frame_a, frame_b, h, w, params, 0, flow_out, workspace, workspace_bytes, stream);
}

int strotss_optical_flow_match(const float* frame_a, const float* frame_b, int h, int w, const strotss_flow_params_t* params,
                               int match_radius, float* flow_out, void* workspace, size_t workspace_bytes, void* stream) {
  return strotss_optical_flow_robust(frame_a, frame_b, h, w, params, nullptr, match_radius, flow_out, workspace,
                                     workspace_bytes, stream);
}

size_t strotss_flow_robust_workspace_bytes(int h, int w, const strotss_flow_params_t* params,
                                           const strotss_flow_robust_params_t* robust) {
  if (!robust) return strotss_flow_workspace_bytes(h, w, params);
  const strotss_flow_params_t p = flow_params_or_default(params, h, w);
  if (h < 2 || w < 2 || (long long)h * w > (1LL << 28) || !flow_params_ok(p) ||
      !st_flow_robust_params_ok(*robust, p.iters, p.iters_per_launch))
    return 0;
  Workspace plan = Workspace::planner();
  FlowBuffers f;
  flow_carve(plan, flow_levels(h, w, p), f, true);
  return plan.off;
}

// The one body.  match_radius R > 0: the patch-matching stage (flow_match.hip) at every level, on the
// level's starting flow and before its warps, into the other half of the (u, v) ping-pong; R = 0 issues no such launch.
// robust != NULL: a warp's `iters` sweeps are `outer` weight updates (flow_robust.hip), each followed
// by iters / outer weighted sweeps in launches of iters_per_launch; NULL issues the launches it always issued.
int strotss_optical_flow_robust(const float* frame_a, const float* frame_b, int h, int w, const strotss_flow_params_t* params,
                                const strotss_flow_robust_params_t* robust, int match_radius, float* flow_out,
                                void* workspace, size_t workspace_bytes, void* stream) {
  ST_CHECK_ARG(frame_a && frame_b && flow_out && workspace, STROTSS_EINVAL);
  ST_CHECK_ARG(match_radius >= 0 && match_radius <= STROTSS_FLOW_MATCH_MAX_RADIUS, STROTSS_EINVAL);
  ST_CHECK_ARG(h >= 2 && w >= 2 && (long long)h * w <= (1LL << 28), STROTSS_EINVAL);
  const strotss_flow_params_t p = flow_params_or_default(params, h, w);
  ST_CHECK_ARG(flow_params_ok(p), STROTSS_EINVAL);
  ST_CHECK_ARG(!robust || st_flow_robust_params_ok(*robust, p.iters, p.iters_per_launch), STROTSS_EINVAL);
  ST_CHECK_ARG(aligned16(frame_a) && aligned16(frame_b) && aligned16(flow_out) && aligned16(workspace), STROTSS_EALIGN);
  const FlowLevels l = flow_levels(h, w, p);
  Workspace ws(workspace, workspace_bytes);
  FlowBuffers f;
  ST_CHECK_ARG(flow_carve(ws, l, f, robust != nullptr), STROTSS_EINVAL);
  const hipStream_t st = (hipStream_t)stream;

  hipLaunchKernelGGL(flow_blur_kernel<true>, per_pixel(h, w), dim3(256), 0, st, frame_a, h, w, f.a[0], h, w, 1);
  hipLaunchKernelGGL(flow_blur_kernel<true>, per_pixel(h, w), dim3(256), 0, st, frame_b, h, w, f.b[0], h, w, 1);
  for (int k = 1; k < l.n; ++k) {
    hipLaunchKernelGGL(flow_blur_kernel<false>, per_pixel(l.h[k], l.w[k]), dim3(256), 0, st, f.a[k - 1], l.h[k - 1],
                       l.w[k - 1], f.a[k], l.h[k], l.w[k], 2);
    hipLaunchKernelGGL(flow_blur_kernel<false>, per_pixel(l.h[k], l.w[k]), dim3(256), 0, st, f.b[k - 1], l.h[k - 1],
                       l.w[k - 1], f.b[k], l.h[k], l.w[k], 2);
  }
  int cur = 0;
  for (int k = l.n - 1; k >= 0; --k) {
    const int hk = l.h[k], wk = l.w[k];
    if (k == l.n - 1) {
      hipLaunchKernelGGL(flow_upsample_kernel, per_pixel(hk, wk), dim3(256), 0, st, (const float*)nullptr,
                         (const float*)nullptr, 0, 0, f.u[cur], f.v[cur], hk, wk);
    } else {
      hipLaunchKernelGGL(flow_upsample_kernel, per_pixel(hk, wk), dim3(256), 0, st, f.u[cur], f.v[cur], l.h[k + 1],
                         l.w[k + 1], f.u[cur ^ 1], f.v[cur ^ 1], hk, wk);
      cur ^= 1;
    }
    if (match_radius > 0) {
      st_flow_match_launch(f.a[k], f.b[k], hk, wk, f.u[cur], f.v[cur], match_radius, f.u[cur ^ 1], f.v[cur ^ 1], st);
      cur ^= 1;
    }
    for (int wi = 0; wi < p.warps; ++wi) {
      hipLaunchKernelGGL(flow_coef_kernel, per_pixel(hk, wk), dim3(256), 0, st, f.a[k], f.b[k], f.u[cur], f.v[cur], hk, wk,
                         p.alpha2, f.coef);
      if (robust) {
        for (int o = 0; o < robust->outer; ++o) {
          st_flow_robust_weights_launch(f.coef, f.u[cur], f.v[cur], hk, wk, *robust, f.s, f.gk, st);
          for (int it = 0; it < p.iters / robust->outer; it += p.iters_per_launch) {
            st_flow_robust_sweeps_launch(f.u[cur], f.v[cur], f.coef, f.s, f.gk, hk, wk, p.iters_per_launch, f.u[cur ^ 1],
                                         f.v[cur ^ 1], st);
            cur ^= 1;
          }
        }
        continue;
      }
      for (int it = 0; it < p.iters; it += p.iters_per_launch) {
        switch (p.iters_per_launch) {
          case 1:
            hipLaunchKernelGGL(flow_jacobi_kernel, per_pixel(hk, wk), dim3(256), 0, st, f.u[cur], f.v[cur], f.coef, hk, wk,
                               f.u[cur ^ 1], f.v[cur ^ 1]);
            break;
          case 2: launch_blocked<2>(f, cur, hk, wk, st); break;
          case 4: launch_blocked<4>(f, cur, hk, wk, st); break;
          default: launch_blocked<8>(f, cur, hk, wk, st); break;
        }
        cur ^= 1;
      }
    }
  }
  hipLaunchKernelGGL(flow_pack_kernel, per_pixel(h, w), dim3(256), 0, st, f.u[cur], f.v[cur], h * w, flow_out);
  ST_LAUNCH_RET();
}
