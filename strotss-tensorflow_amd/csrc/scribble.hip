// Region labels from a few strokes per image: the kernels behind --content_scribbles /
// --style_scribbles.  img is an (h, w, 3) float32 image, stroke its (h, w) int32 stroke labels (0..k-1 on a stroke, anything
// else elsewhere), scores the (gh gw, k) float32 cosines of the cells of its feature grid to the k region centres
// (strotss_kmeans_scores).  A screened random walker: per region r a plane x_r, started at the unary q_r, held at the
// one-hot of the stroke label on stroke pixels and relaxed by Jacobi sweeps toward
// (lambda q_r + sum w x_r(p')) / (lambda + sum w)  over the 4 neighbours inside the image,
// w = exp(-|I(p) - I(p')|^2 / (2 sigma^2)).
//   scores  kmeans_assign_kernel<KP, false, true> (kmeans_assign.h: the s_ij bits of strotss_kmeans_assign), all k values
//   unary   scribble_unary_kernel        one thread per pixel, in float64, rounded once at the stores: the k score planes
//                                        sampled bilinearly (the 4-neighbour, edge-clamped rule of strotss_flow_warp), their
//                                        softmax at temperature tau -> q (k, h, w); x^0 = q or the stroke's one-hot; the two
//                                        edge weights of the pixel, wE toward (y, x + 1) and wS toward (y + 1, x), 0 where
//                                        that neighbour does not exist.  Workgroup 0 zeroes the k counts.
//   sweeps  scribble_sweep_kernel        the plain form: one sweep, one thread per pixel and plane, ping-pong buffers
//           scribble_sweep_blocked_kernel<T>  T = 2, 4 or 8 sweeps per launch: a workgroup owns a 64 x 32 tile of ONE plane
//                                        and holds x of the tile + a halo of T pixels in LDS, double-buffered (30 KiB at
//                                        T = 8); thread t owns the pixels t, t + 256, .. of that extended region and keeps
//                                        their q, their four weights and their fixed flag in registers across the sweeps
//                                        (15 pixels x 6 values at T = 8), which is what flow_jacobi_blocked_kernel does with
//                                        its coefficients.  grid = (tiles, k): the tiles are numbered row by row in
//                                        grid.x, so that a very tall image does not run into the 65535 limit of grid.y.
//           Both forms call sc_update, so they agree bit for bit.
//   labels  scribble_label_kernel        one thread per pixel: the first arg-max over the planes; counts by a wave ballot per
//                                        label, an integer LDS add per wave, one integer atomic add per label and workgroup.
// No float atomics, no order that depends on scheduling: the same bits on every run and stream.  The sweeps are bound by
// their launches at the sizes the product runs them (DESIGN.md section 24 has the measured times).
#include <math.h>

#include "kmeans_assign.h"

namespace {

#define SC_THREADS 256
#define SC_TW 64
#define SC_TH 32
#define SC_MAX_K 7                       // the colour-coded stroke format: eight corner colours, black is "no stroke"
#define SC_MAX_ITERS 1024
#define SC_T8_MAX_WORK (1 << 20)         // iters_per_launch == 0: T = 8 up to this many pixels x planes, T = 4 beyond

// Bilinear taps along one axis in float64 (tap32 of flow.hip, tap64 of temporal.hip): cell centres at integer coordinates,
// both neighbours clamped to [0, n-1]; s clamped to [-2, n+1] first.
struct ScTap { int lo, hi; double f; };
__device__ __forceinline__ ScTap sc_tap(double s, int n) {
  s = fmin(fmax(s, -2.0), (double)(n + 1));
  const double fl = floor(s);
  const int i = (int)fl;
  ScTap t;
  t.lo = min(max(i, 0), n - 1);
  t.hi = min(max(i + 1, 0), n - 1);
  t.f = s - fl;
  return t;
}

__device__ __forceinline__ double sc_edge_weight(const float* __restrict__ a, const float* __restrict__ b, double two_s2) {
  const double e0 = (double)a[0] - (double)b[0], e1 = (double)a[1] - (double)b[1], e2 = (double)a[2] - (double)b[2];
  return exp(-(e0 * e0 + e1 * e1 + e2 * e2) / two_s2);
}

__global__ __launch_bounds__(SC_THREADS) void scribble_unary_kernel(const float* __restrict__ img,
                                                                    const int* __restrict__ stroke,
                                                                    const float* __restrict__ scores, int h, int w, int gh,
                                                                    int gw, int k, double tau, double two_s2,
                                                                    float* __restrict__ q, float* __restrict__ x0,
                                                                    float* __restrict__ wE, float* __restrict__ wS,
                                                                    int* __restrict__ count) {
  if (blockIdx.x == 0 && (int)threadIdx.x < k) count[threadIdx.x] = 0;
  const size_t plane = (size_t)h * w;
  const size_t p = (size_t)blockIdx.x * SC_THREADS + threadIdx.x;
  if (p >= plane) return;
  const int y = (int)(p / w), x = (int)(p - (size_t)y * w);
  const ScTap ty = sc_tap(((double)y + 0.5) * (double)gh / (double)h - 0.5, gh);
  const ScTap tx = sc_tap(((double)x + 0.5) * (double)gw / (double)w - 0.5, gw);
  const float* __restrict__ c00 = scores + ((size_t)ty.lo * gw + tx.lo) * k;
  const float* __restrict__ c01 = scores + ((size_t)ty.lo * gw + tx.hi) * k;
  const float* __restrict__ c10 = scores + ((size_t)ty.hi * gw + tx.lo) * k;
  const float* __restrict__ c11 = scores + ((size_t)ty.hi * gw + tx.hi) * k;
  double t[SC_MAX_K];
  double top = -INFINITY;
#pragma unroll
  for (int r = 0; r < SC_MAX_K; ++r) {
    t[r] = -INFINITY;
    if (r < k) {
      const double a = (double)c00[r], b = (double)c01[r], d = (double)c10[r], e = (double)c11[r];
      const double s = (1.0 - ty.f) * ((1.0 - tx.f) * a + tx.f * b) + ty.f * ((1.0 - tx.f) * d + tx.f * e);
      t[r] = s / tau;
      top = fmax(top, t[r]);
    }
  }
  double sum = 0.0;
#pragma unroll
  for (int r = 0; r < SC_MAX_K; ++r) {
    if (r < k) {
      t[r] = exp(t[r] - top);
      sum += t[r];
    }
  }
  const int lab = stroke[p];
  const bool fixed = (unsigned)lab < (unsigned)k;                       // compared, never used as an index
#pragma unroll
  for (int r = 0; r < SC_MAX_K; ++r) {
    if (r < k) {
      const float qr = (float)(t[r] / sum);
      q[(size_t)r * plane + p] = qr;
      x0[(size_t)r * plane + p] = fixed ? (lab == r ? 1.f : 0.f) : qr;
    }
  }
  const float* __restrict__ c = img + p * 3;
  wE[p] = x < w - 1 ? (float)sc_edge_weight(c, c + 3, two_s2) : 0.f;
  wS[p] = y < h - 1 ? (float)sc_edge_weight(c, c + (size_t)w * 3, two_s2) : 0.f;
}

// The Jacobi update of one pixel of one plane from its 4 neighbours (wt, xn = N, S, W, E; a neighbour outside the image
// has weight 0 and the pixel's own x in its place):  x <- q + sum w (x' - q) / (lambda + sum w), which is
// (lambda q + sum w x') / (lambda + sum w) with the differences formed first: where every neighbour equals q the result
// is q exactly.  A convex combination up to rounding; the clamp keeps the rounding inside [0, 1].  A stroke pixel keeps
// its value.  The one statement of the sweep: both kernels call it, so they contract alike and agree bit for bit.
__device__ __forceinline__ float sc_update(float q, float xc, bool fixed, const float wt[4], const float xn[4], float lambda) {
  const float s = (wt[0] * (xn[0] - q) + wt[1] * (xn[1] - q)) + (wt[2] * (xn[2] - q) + wt[3] * (xn[3] - q));
  const float den = lambda + ((wt[0] + wt[1]) + (wt[2] + wt[3]));
  const float v = fminf(fmaxf(q + s / den, 0.f), 1.f);
  return fixed ? xc : v;
}

// The plain form: one sweep, one thread per pixel and plane (blockIdx.y), neighbours from global memory.
__global__ __launch_bounds__(SC_THREADS) void scribble_sweep_kernel(const float* __restrict__ xin, const float* __restrict__ q,
                                                                    const float* __restrict__ wE, const float* __restrict__ wS,
                                                                    const int* __restrict__ stroke, int h, int w, int k,
                                                                    float lambda, float* __restrict__ xout) {
  const size_t plane = (size_t)h * w;
  const size_t p = (size_t)blockIdx.x * SC_THREADS + threadIdx.x;
  if (p >= plane) return;
  const int y = (int)(p / w), x = (int)(p - (size_t)y * w);
  const size_t base = (size_t)blockIdx.y * plane;
  const float* __restrict__ xi = xin + base;
  const float wt[4] = {y > 0 ? wS[p - w] : 0.f, wS[p], x > 0 ? wE[p - 1] : 0.f, wE[p]};
  const float xn[4] = {xi[y > 0 ? p - w : p], xi[y < h - 1 ? p + w : p], xi[x > 0 ? p - 1 : p], xi[x < w - 1 ? p + 1 : p]};
  xout[base + p] = sc_update(q[base + p], xi[p], (unsigned)stroke[p] < (unsigned)k, wt, xn, lambda);
}

// The temporally blocked form: T sweeps per launch.  Sweep s = 1 .. T updates the pixels at least s rings inside the
// extended region (their neighbours, one ring further out, hold sweep s-1), so after T sweeps the tile itself is right.
// A pixel outside the image is never loaded, computed or read: toward it the weight is 0 and the pixel's own x is read,
// as scribble_sweep_kernel reads it.  LDS: 2 (64 + 2T)(32 + 2T) floats = 30 KiB at T = 8.
template <int T>
__global__ __launch_bounds__(SC_THREADS) void scribble_sweep_blocked_kernel(const float* __restrict__ xin,
                                                                            const float* __restrict__ q,
                                                                            const float* __restrict__ wE,
                                                                            const float* __restrict__ wS,
                                                                            const int* __restrict__ stroke, int h, int w,
                                                                            int k, float lambda, unsigned tiles_x,
                                                                            float* __restrict__ xout) {
  constexpr int EW = SC_TW + 2 * T, EH = SC_TH + 2 * T, NPIX = EW * EH, PER = (NPIX + SC_THREADS - 1) / SC_THREADS;
  __shared__ float sx[2][NPIX];
  const int x0 = (int)(blockIdx.x % tiles_x) * SC_TW - T;                // the extended region's corner in the image
  const int y0 = (int)(blockIdx.x / tiles_x) * SC_TH - T;
  const size_t base = (size_t)blockIdx.y * (size_t)h * w;
  // per owned pixel: q, the weights toward N, S, W, E and, packed, its ring (0 = outermost; -1 = not in the image or not a
  // pixel), whether its W / E / N / S neighbour exists in the image and whether a stroke fixes it
  float qv[PER];
  float wt[PER][4];
  int meta[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int e = (int)threadIdx.x + SC_THREADS * i;
    const int ey = e / EW, ex = e - ey * EW;
    const int gx = x0 + ex, gy = y0 + ey;
    const bool in = e < NPIX && gx >= 0 && gx < w && gy >= 0 && gy < h;
    qv[i] = 0.f;
    wt[i][0] = wt[i][1] = wt[i][2] = wt[i][3] = 0.f;
    meta[i] = -1;
    if (in) {
      const size_t g = (size_t)gy * w + gx;
      qv[i] = q[base + g];
      wt[i][0] = gy > 0 ? wS[g - w] : 0.f;
      wt[i][1] = wS[g];
      wt[i][2] = gx > 0 ? wE[g - 1] : 0.f;
      wt[i][3] = wE[g];
      sx[0][e] = xin[base + g];
      const int ring = min(min(ex, EW - 1 - ex), min(ey, EH - 1 - ey));
      meta[i] = ring | (gx > 0 ? 256 : 0) | (gx < w - 1 ? 512 : 0) | (gy > 0 ? 1024 : 0) | (gy < h - 1 ? 2048 : 0) |
                ((unsigned)stroke[g] < (unsigned)k ? 4096 : 0);
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int s = 1; s <= T; ++s) {
    const float* __restrict__ rx = sx[(s - 1) & 1];
    float* __restrict__ wx = sx[s & 1];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int m = meta[i];
      if (m < 0 || (m & 255) < s) continue;
      const int e = (int)threadIdx.x + SC_THREADS * i;
      const float xn[4] = {rx[(m & 1024) ? e - EW : e], rx[(m & 2048) ? e + EW : e], rx[e - ((m >> 8) & 1)],
                           rx[e + ((m >> 9) & 1)]};
      wx[e] = sc_update(qv[i], rx[e], (m & 4096) != 0, wt[i], xn, lambda);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int m = meta[i];
    if (m < 0 || (m & 255) < T) continue;            // the tile = the pixels T rings inside
    const int e = (int)threadIdx.x + SC_THREADS * i;
    const int ey = e / EW, ex = e - ey * EW;
    xout[base + (size_t)(y0 + ey) * w + (x0 + ex)] = sx[T & 1][e];
  }
}

__global__ __launch_bounds__(SC_THREADS) void scribble_label_kernel(const float* __restrict__ x, int h, int w, int k,
                                                                    int* __restrict__ label, int* __restrict__ count,
                                                                    float* __restrict__ x_out) {
  __shared__ int cnt[SC_MAX_K + 1];
  const int t = (int)threadIdx.x, lane = t & 63;
  if (t <= SC_MAX_K) cnt[t] = 0;
  __syncthreads();
  const size_t plane = (size_t)h * w;
  const size_t p = (size_t)blockIdx.x * SC_THREADS + threadIdx.x;
  const bool inside = p < plane;
  int bl = 0;
  if (inside) {
    float best = x[p];
    if (x_out) x_out[p] = best;
#pragma unroll
    for (int r = 1; r < SC_MAX_K; ++r) {
      if (r < k) {
        const float v = x[(size_t)r * plane + p];
        if (x_out) x_out[(size_t)r * plane + p] = v;
        if (v > best) {                                                 // strictly: the lowest r wins on equal values
          best = v;
          bl = r;
        }
      }
    }
    label[p] = bl;
  }
#pragma unroll
  for (int l = 0; l < SC_MAX_K; ++l) {
    const unsigned long long m = __ballot(inside && bl == l);
    if (lane == 0 && m) atomicAdd(&cnt[l], __popcll(m));                // integer, in LDS
  }
  __syncthreads();
  if (t < k && cnt[t]) atomicAdd(&count[t], cnt[t]);                    // integer: one per label and workgroup
}

inline bool sc_k_ok(int k) { return k >= 2 && k <= SC_MAX_K; }
inline bool sc_sizes_ok(int h, int w, int k) {
  return h > 0 && w > 0 && sc_k_ok(k) && (long long)k * h * w <= 0x7fffffffLL && 3LL * h * w <= 0x7fffffffLL;
}
inline bool sc_positive(double v) { return isfinite(v) && v > 0.0; }

template <int T>
void sc_launch_blocked(const float* xin, const float* q, const float* wE, const float* wS, const int* stroke, int h, int w,
                       int k, float lambda, float* xout, hipStream_t st) {
  // tiles_x tiles_y <= h w / 2048 + h / 32 + w / 64 + 1 < 2^31 for every k h w <= INT_MAX with k >= 2
  const unsigned tiles_x = ((unsigned)w + SC_TW - 1) / SC_TW, tiles_y = ((unsigned)h + SC_TH - 1) / SC_TH;
  hipLaunchKernelGGL(scribble_sweep_blocked_kernel<T>, dim3(tiles_x * tiles_y, (unsigned)k), dim3(SC_THREADS), 0, st, xin, q,
                     wE, wS, stroke, h, w, k, lambda, tiles_x, xout);
}

}  // namespace

int strotss_kmeans_scores(const float* x, const float* inv_norm, int n, int d, int ld, const float* centres, int k,
                          float* scores, void* stream) {
  ST_CHECK_ARG(x && inv_norm && centres && scores && km_rows_ok(n, d, ld) && km_k_ok(k), STROTSS_EINVAL);
  ST_CHECK_ARG((long long)n * k <= 0x7fffffffLL, STROTSS_EINVAL);
  ST_CHECK_ARG(ld % 32 == 0, STROTSS_EALIGN);
  ST_CHECK_ARG(aligned16(x) && aligned16(inv_norm) && aligned16(centres) && aligned16(scores), STROTSS_EALIGN);
  km_launch_scores(x, inv_norm, n, d, ld, centres, k, scores, (hipStream_t)stream);
  ST_LAUNCH_RET();
}

size_t strotss_scribble_workspace_bytes(int h, int w, int k) {
  if (!sc_sizes_ok(h, w, k)) return 0;
  return (size_t)(3 * k + 2) * ws_slice((size_t)h * (size_t)w, sizeof(float));
}

int strotss_scribble_labels(const float* img, const int* stroke, int h, int w, const float* scores, int gh, int gw, int k,
                            double tau, double lambda, double sigma, int iters, int iters_per_launch, int* label, int* count,
                            float* x, void* workspace, size_t workspace_bytes, void* stream) {
  ST_CHECK_ARG(img && stroke && scores && label && count && workspace && sc_sizes_ok(h, w, k), STROTSS_EINVAL);
  ST_CHECK_ARG(gh > 0 && gw > 0 && (long long)gh * gw * k <= 0x7fffffffLL, STROTSS_EINVAL);
  const double two_s2 = 2.0 * sigma * sigma;
  const float lam = (float)lambda;
  ST_CHECK_ARG(sc_positive(tau) && sc_positive(lambda) && sc_positive(sigma) && sc_positive(1.0 / tau) && sc_positive(two_s2) &&
                   sc_positive(1.0 / two_s2) && isfinite(lam) && lam > 0.f,
               STROTSS_EINVAL);
  ST_CHECK_ARG(iters >= 1 && iters <= SC_MAX_ITERS, STROTSS_EINVAL);
  const int T = iters_per_launch;                                       // 0: the library's choice
  ST_CHECK_ARG(T == 0 || T == 1 || T == 2 || T == 4 || T == 8, STROTSS_EINVAL);
  ST_CHECK_ARG(workspace_bytes >= strotss_scribble_workspace_bytes(h, w, k), STROTSS_EINVAL);
  ST_CHECK_ARG(aligned16(img) && aligned16(stroke) && aligned16(scores) && aligned16(label) && aligned16(count) &&
                   aligned16(x) && aligned16(workspace),
               STROTSS_EALIGN);
  static_assert(STROTSS_SCRIBBLE_MAX_K == SC_MAX_K && STROTSS_SCRIBBLE_MAX_ITERS == SC_MAX_ITERS, "the header's limits");
  const hipStream_t st = (hipStream_t)stream;
  const size_t plane = (size_t)h * (size_t)w;
  Workspace ws(workspace, workspace_bytes);
  // 3 k + 2 planes: q and the two x buffers (k planes each, packed: plane r at r h w), wE, wS.  The size asked for counts a
  // 256-byte slice per plane, which covers the three packed buffers' slices.
  float* q = ws.take<float>((size_t)k * plane);
  float* xb[2] = {ws.take<float>((size_t)k * plane), nullptr};
  xb[1] = ws.take<float>((size_t)k * plane);
  float* wE = ws.take<float>(plane);
  float* wS = ws.take<float>(plane);
  ST_CHECK_ARG(ws.ok(), STROTSS_EINVAL);

  const dim3 block(SC_THREADS), per_pixel((unsigned)((plane + SC_THREADS - 1) / SC_THREADS));
  hipLaunchKernelGGL(scribble_unary_kernel, per_pixel, block, 0, st, img, stroke, scores, h, w, gh, gw, k, tau, two_s2, q,
                     xb[0], wE, wS, count);
  // The library's choice is the form that measured fastest (DESIGN.md section 24, 128 sweeps, eight sizes): T = 8 wherever
  // k h w <= 393216 (384 x 512 x 2: 369 us against 428 at T = 4 and 513 plain), T = 4 wherever k h w >= 1376256
  // (384 x 512 x 7: 610 us against 695 at T = 8 and 851 plain).  Between the two nothing is measured: the switch-over is
  // put at 2^20.  Every form gives the same bits; sweeps that do not fill a blocked launch run in the plain form.
  const int per = T == 0 ? ((long long)k * h * w <= SC_T8_MAX_WORK ? 8 : 4) : T;
  int cur = 0, left = iters;
  for (; per > 1 && left >= per; left -= per, cur ^= 1) {
    switch (per) {
      case 2: sc_launch_blocked<2>(xb[cur], q, wE, wS, stroke, h, w, k, lam, xb[cur ^ 1], st); break;
      case 4: sc_launch_blocked<4>(xb[cur], q, wE, wS, stroke, h, w, k, lam, xb[cur ^ 1], st); break;
      default: sc_launch_blocked<8>(xb[cur], q, wE, wS, stroke, h, w, k, lam, xb[cur ^ 1], st); break;
    }
  }
  for (; left > 0; --left, cur ^= 1)
    hipLaunchKernelGGL(scribble_sweep_kernel, dim3(per_pixel.x, (unsigned)k), block, 0, st, xb[cur], q, wE, wS, stroke, h, w, k,
                       lam, xb[cur ^ 1]);
  hipLaunchKernelGGL(scribble_label_kernel, per_pixel, block, 0, st, xb[cur], h, w, k, label, count, x);
  ST_LAUNCH_RET();
}
