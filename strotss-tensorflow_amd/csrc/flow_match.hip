// The optical flow's patch-matching stage: at one pyramid level, every pixel tries the whole offsets
// d in [-R, R]^2 around its flow and keeps the one whose 5 x 5 window of A matches B best (sum of absolute differences,
// B sampled bilinearly at the window moved by the CENTRE pixel's flow + d).  tests/_flow_match_ref.py is the statement;
// every operation here is rounded on its own (__fadd_rn, __fmul_rn, __fsub_rn: no contraction), in the statement's order,
// so the kernel is its float32 twin.
//   - flow_match_kernel<R>: a 256-thread workgroup owns a FLOW_TW x FLOW_TH = 64 x 32 tile (flow.hip's), 8 pixels per
//     thread; the tile of A + a halo of 2 goes to LDS once (loaded with clamped indices, so the window's clamp is the
//     staging's); B is read through cache with clamped indices: where the window lands depends on the pixel's flow.
// Nothing is indexed by a data value: the flow's whole part enters B's indices only through a clamp to the image.
#include <cmath>

#include "internal.h"

namespace {

#define FLOW_TW 64
#define FLOW_TH 32
#define MATCH_WIN 2                                     // the 5 x 5 window's half width
#define MATCH_LIMIT 1.0e6f                              // |F| clamped there before the split (a NaN lands on -MATCH_LIMIT)

__device__ __forceinline__ int clampi(int v, int n) { return min(max(v, 0), n - 1); }

template <int R>
__global__ __launch_bounds__(256) void flow_match_kernel(const float* __restrict__ a, const float* __restrict__ b, int h, int w,
                                                         const float* __restrict__ u, const float* __restrict__ v,
                                                         float* __restrict__ uo, float* __restrict__ vo) {
  constexpr int EW = FLOW_TW + 2 * MATCH_WIN, EH = FLOW_TH + 2 * MATCH_WIN;
  __shared__ float sa[EH * EW];
  const int x0 = blockIdx.x * FLOW_TW, y0 = blockIdx.y * FLOW_TH;
  for (int e = threadIdx.x; e < EH * EW; e += 256) {
    const int ey = e / EW, ex = e - ey * EW;
    sa[e] = a[(size_t)clampi(y0 + ey - MATCH_WIN, h) * w + clampi(x0 + ex - MATCH_WIN, w)];
  }
  __syncthreads();
  const int lx = threadIdx.x & (FLOW_TW - 1), x = x0 + lx;
  if (x >= w) return;
#pragma unroll 1
  for (int ly = threadIdx.x / FLOW_TW; ly < FLOW_TH; ly += 256 / FLOW_TW) {
    const int y = y0 + ly;
    if (y >= h) return;
    const size_t p = (size_t)y * w + x;
    const float up = u[p], vp = v[p];
    // F = whole part + fraction, once per pixel: the 25 taps and every offset share the weights
    const float uc = fminf(fmaxf(up, -MATCH_LIMIT), MATCH_LIMIT), vc = fminf(fmaxf(vp, -MATCH_LIMIT), MATCH_LIMIT);
    const float ufl = floorf(uc), vfl = floorf(vc);
    const float fx = __fsub_rn(uc, ufl), fy = __fsub_rn(vc, vfl);
    const float gx = __fsub_rn(1.f, fx), gy = __fsub_rn(1.f, fy);
    const int iu = (int)ufl, iv = (int)vfl;
    // the window's pixels in the image (clamped: what the staging put into the halo) and their samples' whole parts
    int qx[5], qy[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      qx[t] = clampi(x + t - MATCH_WIN, w) + iu;
      qy[t] = clampi(y + t - MATCH_WIN, h) + iv;
    }
    const float* __restrict__ win = sa + ly * EW + lx;  // the window's top left corner in the staged tile
    float cbest = INFINITY, czero = INFINITY;
    int bdx = 0, bdy = 0;
#pragma unroll 1
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll 1
      for (int dx = -R; dx <= R; ++dx) {
        float c = 0.f;
#pragma unroll
        for (int ty = 0; ty < 5; ++ty) {
          const float* __restrict__ r0 = b + (size_t)clampi(qy[ty] + dy, h) * w;
          const float* __restrict__ r1 = b + (size_t)clampi(qy[ty] + dy + 1, h) * w;
#pragma unroll
          for (int tx = 0; tx < 5; ++tx) {
            const int c0 = clampi(qx[tx] + dx, w), c1 = clampi(qx[tx] + dx + 1, w);
            const float top = __fadd_rn(__fmul_rn(gx, r0[c0]), __fmul_rn(fx, r0[c1]));
            const float bot = __fadd_rn(__fmul_rn(gx, r1[c0]), __fmul_rn(fx, r1[c1]));
            const float s = __fadd_rn(__fmul_rn(gy, top), __fmul_rn(fy, bot));
            const float term = fabsf(__fsub_rn(win[ty * EW + tx], s));
            c = (ty == 0 && tx == 0) ? term : __fadd_rn(c, term);
          }
        }
        if (dx == 0 && dy == 0) czero = c;
        if (c < cbest) {                                // strict: the first minimiser in scan order stays
          cbest = c;
          bdx = dx;
          bdy = dy;
        }
      }
    }
    const bool move = cbest < czero;                    // strict: d = 0 wins every tie
    uo[p] = move ? __fadd_rn(up, (float)bdx) : up;
    vo[p] = move ? __fadd_rn(vp, (float)bdy) : vp;
  }
}

}  // namespace

void st_flow_match_launch(const float* a, const float* b, int h, int w, const float* u, const float* v, int radius,
                          float* uo, float* vo, hipStream_t st) {
  const dim3 grid((w + FLOW_TW - 1) / FLOW_TW, (h + FLOW_TH - 1) / FLOW_TH);
  switch (radius) {
    case 1: hipLaunchKernelGGL(flow_match_kernel<1>, grid, dim3(256), 0, st, a, b, h, w, u, v, uo, vo); break;
    case 2: hipLaunchKernelGGL(flow_match_kernel<2>, grid, dim3(256), 0, st, a, b, h, w, u, v, uo, vo); break;
    case 3: hipLaunchKernelGGL(flow_match_kernel<3>, grid, dim3(256), 0, st, a, b, h, w, u, v, uo, vo); break;
    default: hipLaunchKernelGGL(flow_match_kernel<4>, grid, dim3(256), 0, st, a, b, h, w, u, v, uo, vo); break;
  }
}

int strotss_flow_match_stage(const float* a, const float* b, int h, int w, const float* u, const float* v, int match_radius,
                             float* u_out, float* v_out, void* stream) {
  ST_CHECK_ARG(a && b && u && v && u_out && v_out, STROTSS_EINVAL);
  ST_CHECK_ARG(h >= 1 && w >= 1 && (long long)h * w <= (1LL << 28), STROTSS_EINVAL);
  ST_CHECK_ARG(match_radius >= 1 && match_radius <= STROTSS_FLOW_MATCH_MAX_RADIUS, STROTSS_EINVAL);
  ST_CHECK_ARG(u_out != u && u_out != v && v_out != u && v_out != v && u_out != v_out, STROTSS_EINVAL);
  ST_CHECK_ARG(aligned16(a) && aligned16(b) && aligned16(u) && aligned16(v) && aligned16(u_out) && aligned16(v_out),
               STROTSS_EALIGN);
  st_flow_match_launch(a, b, h, w, u, v, match_radius, u_out, v_out, (hipStream_t)stream);
  ST_LAUNCH_RET();
}
