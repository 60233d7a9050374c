// The optical flow's robust form: Charbonnier penalties on the linearised data term and on the flow's
// gradient, minimised with lagged weights.  Per warp (flow.hip's coefficients Ix, Iy, c), `outer` times: one weight update
// from the current (u, v), then iters / outer Jacobi sweeps with the weights frozen.  tests/_flow_robust_ref.py is the
// statement and fixes the evaluation order; this file is compiled without contraction (the pragma below) and spells every
// sum in that order, 1 / x and sqrt are correctly rounded, so the kernels are the float32 statement's twins.
//   - flow_robust_weight_kernel: once per weight update, one thread per pixel: s = 1 / sqrt(|grad u|^2 + |grad v|^2 + eps_s^2)
//     here and at the 8 clamped neighbours (the same expression, so the same bits as the stored s), from them G = sum g_q,
//     and d = 1 / sqrt(r^2 + eps_d^2) -> s(y, x) and gk(y, x) = {1 / G, d / (alpha G + d (Ix^2 + Iy^2))};
//   - flow_robust_jacobi_kernel: one sweep per launch, one thread per pixel (the plain form);
//   - flow_robust_blocked_kernel<K>: K sweeps per launch on flow.hip's 64 x 32 tile + a halo of K, (u, v) double-buffered
//     and s held once in LDS.
// Both solver forms call robust_update, so they agree bit for bit.  Plain vector stores only, no atomics.
#include <cmath>

#include "internal.h"

#pragma clang fp contract(off)

namespace {

#define FLOW_TW 64
#define FLOW_TH 32
#define W_EDGE (1.f / 12.f)                             // w_q / 2: 1/6 for N, S, W, E
#define W_DIAG (1.f / 24.f)                             //          1/12 for the diagonals

__device__ __forceinline__ float tree8(const float t[8]) {
  return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
}

// g_q of the 8 neighbours (N, S, W, E, NW, NE, SW, SE) from s at the pixel and at them
__device__ __forceinline__ void couplings(float sp, const float sq[8], float g[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) g[i] = (sp + sq[i]) * W_EDGE;
#pragma unroll
  for (int i = 4; i < 8; ++i) g[i] = (sp + sq[i]) * W_DIAG;
}

// s at one pixel: central differences of (u, v) with clamped indices
__device__ __forceinline__ float smooth_weight(const float* __restrict__ u, const float* __restrict__ v, int h, int w, int y,
                                               int x, float eps_s2) {
  const size_t rc = (size_t)y * w, rn = (size_t)max(y - 1, 0) * w, rs = (size_t)min(y + 1, h - 1) * w;
  const int xm = max(x - 1, 0), xp = min(x + 1, w - 1);
  const float ux = (u[rc + xp] - u[rc + xm]) * 0.5f, uy = (u[rs + x] - u[rn + x]) * 0.5f;
  const float vx = (v[rc + xp] - v[rc + xm]) * 0.5f, vy = (v[rs + x] - v[rn + x]) * 0.5f;
  return 1.f / sqrtf(((ux * ux + uy * uy) + (vx * vx + vy * vy)) + eps_s2);
}

__global__ __launch_bounds__(256) void flow_robust_weight_kernel(const f32x4* __restrict__ coef, const float* __restrict__ u,
                                                                 const float* __restrict__ v, int h, int w, float alpha,
                                                                 float eps_d2, float eps_s2, float* __restrict__ s,
                                                                 float2* __restrict__ gk) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h * w) return;
  const int y = p / w, x = p - y * w;
  const int xm = max(x - 1, 0), xp = min(x + 1, w - 1), ym = max(y - 1, 0), yp = min(y + 1, h - 1);
  const float sp = smooth_weight(u, v, h, w, y, x, eps_s2);
  const float sq[8] = {smooth_weight(u, v, h, w, ym, x, eps_s2),  smooth_weight(u, v, h, w, yp, x, eps_s2),
                       smooth_weight(u, v, h, w, y, xm, eps_s2),  smooth_weight(u, v, h, w, y, xp, eps_s2),
                       smooth_weight(u, v, h, w, ym, xm, eps_s2), smooth_weight(u, v, h, w, ym, xp, eps_s2),
                       smooth_weight(u, v, h, w, yp, xm, eps_s2), smooth_weight(u, v, h, w, yp, xp, eps_s2)};
  float g[8];
  couplings(sp, sq, g);
  const float G = tree8(g);
  const f32x4 k = coef[p];
  const float r = (k[0] * u[p] + k[1] * v[p]) + k[2];
  const float d = 1.f / sqrtf(r * r + eps_d2);
  s[p] = sp;
  gk[p] = make_float2(1.f / G, d / (alpha * G + d * (k[0] * k[0] + k[1] * k[1])));
}

// The weighted Jacobi update of one pixel; sq, uq, vq = s, u, v at N, S, W, E, NW, NE, SW, SE.  The one statement of the sweep.
__device__ __forceinline__ void robust_update(float sp, const float sq[8], const float uq[8], const float vq[8], float ix,
                                              float iy, float c, float rg, float k, float& uo, float& vo) {
  float g[8], tu[8], tv[8];
  couplings(sp, sq, g);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    tu[i] = g[i] * uq[i];
    tv[i] = g[i] * vq[i];
  }
  const float ub = tree8(tu) * rg, vb = tree8(tv) * rg;
  const float t = ((ix * ub + iy * vb) + c) * k;
  uo = ub - ix * t;
  vo = vb - iy * t;
}

__global__ __launch_bounds__(256) void flow_robust_jacobi_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                                 const f32x4* __restrict__ coef, const float* __restrict__ s,
                                                                 const float2* __restrict__ gk, int h, int w,
                                                                 float* __restrict__ uo, float* __restrict__ vo) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h * w) return;
  const int y = p / w, x = p - y * w;
  const int xm = max(x - 1, 0), xp = min(x + 1, w - 1);
  const size_t rn = (size_t)max(y - 1, 0) * w, rs = (size_t)min(y + 1, h - 1) * w, rc = (size_t)y * w;
  const size_t q[8] = {rn + x, rs + x, rc + xm, rc + xp, rn + xm, rn + xp, rs + xm, rs + xp};
  float sq[8], uq[8], vq[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sq[i] = s[q[i]];
    uq[i] = u[q[i]];
    vq[i] = v[q[i]];
  }
  const f32x4 k = coef[p];
  const float2 m = gk[p];
  robust_update(s[p], sq, uq, vq, k[0], k[1], k[2], m.x, m.y, uo[p], vo[p]);
}

// flow_jacobi_blocked_kernel's scheme (flow.hip) with the weights: thread t owns the pixels t, t + 256, ... of the tile + a
// halo of K and keeps their {Ix, Iy, c, 1 / G, k} in registers; sweep i updates the pixels at least i rings inside, whose
// neighbours -- one ring further out, at least ring 0 -- hold sweep i - 1 and their s.  G is the weight kernel's, so s is
// needed on those K rings only.  The image edge is clamped by index inside the region.
// LDS: 5 * (64 + 2K) * (32 + 2K) floats = 75 KiB at K = 8: two workgroups in a CU's 160 KiB.
template <int K>
__global__ __launch_bounds__(256) void flow_robust_blocked_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                                  const f32x4* __restrict__ coef, const float* __restrict__ s,
                                                                  const float2* __restrict__ gk, int h, int w,
                                                                  float* __restrict__ uo, float* __restrict__ vo) {
  constexpr int EW = FLOW_TW + 2 * K, EH = FLOW_TH + 2 * K, NPIX = EW * EH, PER = (NPIX + 255) / 256;
  __shared__ float su[2][NPIX];
  __shared__ float sv[2][NPIX];
  __shared__ float ss[NPIX];
  const int x0 = blockIdx.x * FLOW_TW - K, y0 = blockIdx.y * FLOW_TH - K;
  float ix[PER], iy[PER], c[PER], rg[PER], kk[PER];
  int meta[PER];                                        // flow.hip's: ring | W, E, N, S neighbour in the image; -1 = no pixel
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int e = threadIdx.x + 256 * i;
    const int ey = e / EW, ex = e - ey * EW;
    const int gx = x0 + ex, gy = y0 + ey;
    const bool in = e < NPIX && gx >= 0 && gx < w && gy >= 0 && gy < h;
    // every register is assigned once and without a branch (a pixel outside reads the clamped address and is never used):
    // assignments under `if (in)` make the compiler carry the arrays as whole vectors, 446 VGPRs and scratch at K = 8
    const size_t g = (size_t)min(max(gy, 0), h - 1) * w + min(max(gx, 0), w - 1);
    const f32x4 k4 = coef[g];
    const float2 m = gk[g];
    ix[i] = k4[0];
    iy[i] = k4[1];
    c[i] = k4[2];
    rg[i] = m.x;
    kk[i] = m.y;
    const float u0 = u[g], v0 = v[g], s0 = s[g];
    if (in) {
      su[0][e] = u0;
      sv[0][e] = v0;
      ss[e] = s0;
    }
    const int ring = min(min(ex, EW - 1 - ex), min(ey, EH - 1 - ey));
    meta[i] = in ? ring | (gx > 0 ? 256 : 0) | (gx < w - 1 ? 512 : 0) | (gy > 0 ? 1024 : 0) | (gy < h - 1 ? 2048 : 0) : -1;
  }
  __syncthreads();
#pragma unroll 1
  for (int sw = 1; sw <= K; ++sw) {
    const float* __restrict__ ru = su[(sw - 1) & 1];
    const float* __restrict__ rv = sv[(sw - 1) & 1];
    float* __restrict__ wu = su[sw & 1];
    float* __restrict__ wv = sv[sw & 1];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      int m = meta[i];
      asm volatile("" : "+v"(m));                       // opaque per sweep: the 8 neighbour offsets of all PER pixels are
      if (m < 0 || (m & 255) < sw) continue;            // formed again (a few integer operations), not kept in 8 * PER registers
      const int e = threadIdx.x + 256 * i;
      const int xm = e - ((m >> 8) & 1), xp = e + ((m >> 9) & 1);
      const int dn = (m & 1024) ? EW : 0, ds = (m & 2048) ? EW : 0;
      const int q[8] = {e - dn, e + ds, xm, xp, xm - dn, xp - dn, xm + ds, xp + ds};
      float sq[8], uq[8], vq[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sq[j] = ss[q[j]];
        uq[j] = ru[q[j]];
        vq[j] = rv[q[j]];
      }
      robust_update(ss[e], sq, uq, vq, ix[i], iy[i], c[i], rg[i], kk[i], wu[e], wv[e]);
      __builtin_amdgcn_sched_barrier(0);                // one pixel's 25 LDS reads at a time: the registers hold PER pixels' data
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int m = meta[i];
    if (m < 0 || (m & 255) < K) continue;               // the tile = the pixels K rings inside
    const int e = threadIdx.x + 256 * i;
    const int ey = e / EW, ex = e - ey * EW;
    const size_t g = (size_t)(y0 + ey) * w + (x0 + ex);
    uo[g] = su[K & 1][e];
    vo[g] = sv[K & 1][e];
  }
}

template <int K>
void launch_blocked(const float* u, const float* v, const f32x4* coef, const float* s, const float2* gk, int h, int w,
                    float* uo, float* vo, hipStream_t st) {
  hipLaunchKernelGGL(flow_robust_blocked_kernel<K>, dim3((w + FLOW_TW - 1) / FLOW_TW, (h + FLOW_TH - 1) / FLOW_TH), dim3(256),
                     0, st, u, v, coef, s, gk, h, w, uo, vo);
}

inline dim3 per_pixel(int h, int w) { return dim3((unsigned)(((long long)h * w + 255) / 256)); }

const strotss_flow_robust_params_t kRobustDefaults = {0.06f, 1e-3f, 1e-2f, 4};

// finite, > 0, and (the eps) with a square that is: eps^2 = 0 would leave 1 / sqrt(0) at a pixel with r = 0
bool positive(float x) { return std::isfinite(x) && x > 0.f; }

}  // namespace

bool st_flow_robust_params_ok(const strotss_flow_robust_params_t& r, int iters, int iters_per_launch) {
  return positive(r.alpha) && positive(r.eps_d) && positive(r.eps_d * r.eps_d) && positive(r.eps_s) &&
         positive(r.eps_s * r.eps_s) && r.outer >= 1 && r.outer <= STROTSS_FLOW_ROBUST_MAX_OUTER && iters % r.outer == 0 &&
         (iters / r.outer) % iters_per_launch == 0;
}

void st_flow_robust_weights_launch(const f32x4* coef, const float* u, const float* v, int h, int w,
                                   const strotss_flow_robust_params_t& r, float* s, float* gk, hipStream_t st) {
  hipLaunchKernelGGL(flow_robust_weight_kernel, per_pixel(h, w), dim3(256), 0, st, coef, u, v, h, w, r.alpha,
                     r.eps_d * r.eps_d, r.eps_s * r.eps_s, s, (float2*)gk);
}

void st_flow_robust_sweeps_launch(const float* u, const float* v, const f32x4* coef, const float* s, const float* gk, int h,
                                  int w, int sweeps, float* uo, float* vo, hipStream_t st) {
  const float2* m = (const float2*)gk;
  switch (sweeps) {
    case 1:
      hipLaunchKernelGGL(flow_robust_jacobi_kernel, per_pixel(h, w), dim3(256), 0, st, u, v, coef, s, m, h, w, uo, vo);
      break;
    case 2: launch_blocked<2>(u, v, coef, s, m, h, w, uo, vo, st); break;
    case 4: launch_blocked<4>(u, v, coef, s, m, h, w, uo, vo, st); break;
    default: launch_blocked<8>(u, v, coef, s, m, h, w, uo, vo, st); break;
  }
}

void strotss_flow_robust_default_params(strotss_flow_robust_params_t* out) {
  if (out) *out = kRobustDefaults;
}

int strotss_flow_robust_stage(const float* coef, const float* u, const float* v, int h, int w,
                              const strotss_flow_robust_params_t* robust, int sweeps, int iters_per_launch, float* u_out,
                              float* v_out, float* s_out, float* gk_out, float* tmp, void* stream) {
  ST_CHECK_ARG(coef && u && v && u_out && v_out && s_out && gk_out && tmp, STROTSS_EINVAL);
  ST_CHECK_ARG(h >= 2 && w >= 2 && (long long)h * w <= (1LL << 28), STROTSS_EINVAL);
  const int k = iters_per_launch;
  ST_CHECK_ARG((k == 1 || k == 2 || k == 4 || k == 8) && sweeps >= 1 && sweeps <= 1024 && sweeps % k == 0, STROTSS_EINVAL);
  strotss_flow_robust_params_t r = robust ? *robust : kRobustDefaults;
  r.outer = 1;                                          // the stage is one weight update
  ST_CHECK_ARG(st_flow_robust_params_ok(r, sweeps, k), STROTSS_EINVAL);
  const void* ins[3] = {coef, u, v};
  void* outs[5] = {u_out, v_out, s_out, gk_out, tmp};
  for (int i = 0; i < 5; ++i) {
    for (int j = 0; j < 3; ++j) ST_CHECK_ARG(outs[i] != ins[j], STROTSS_EINVAL);
    for (int j = 0; j < i; ++j) ST_CHECK_ARG(outs[i] != outs[j], STROTSS_EINVAL);
  }
  ST_CHECK_ARG(aligned16(coef) && aligned16(u) && aligned16(v) && aligned16(u_out) && aligned16(v_out) && aligned16(s_out) &&
                   aligned16(gk_out) && aligned16(tmp),
               STROTSS_EALIGN);
  const hipStream_t st = (hipStream_t)stream;
  const f32x4* k4 = (const f32x4*)coef;
  st_flow_robust_weights_launch(k4, u, v, h, w, r, s_out, gk_out, st);
  // the launches alternate between (tmp, tmp + h w) and the outputs so that the last one writes the outputs
  const int n = sweeps / k;
  const float *ru = u, *rv = v;
  for (int i = 0; i < n; ++i) {
    const bool to_out = ((n - 1 - i) & 1) == 0;
    float* wu = to_out ? u_out : tmp;
    float* wv = to_out ? v_out : tmp + (size_t)h * w;
    st_flow_robust_sweeps_launch(ru, rv, k4, s_out, gk_out, h, w, k, wu, wv, st);
    ru = wu;
    rv = wv;
  }
  ST_LAUNCH_RET();
}
