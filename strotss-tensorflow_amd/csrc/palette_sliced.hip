// Sliced 1-Wasserstein distance as the step's palette term: the first three columns of the prediction
// and style rows go to YUV, are projected on P fixed unit directions of R^3 (nn/rand.py:palette_directions), each direction's
// two projected sets are sorted, and the exact 1-D transport between the two uniform atom sets (the quantile-cell overlaps
// of section 21) gives the direction's cost and the gradient coefficients.
//
//     match    one workgroup of 1024 threads per direction: thread t converts and projects prediction row t and style row t
//              (D = 3: no GEMM), both sides are sorted by (value, row) on the bitonic network of sort_match.h, then
//              W_p = sum_ij len_ij |a_(i) - b_(j)| and dW_p/da = sum_j len_ij sign(a_(i) - b_(j)) at the element's original row
//     finish   one thread per row: dy_i = (2 / (sqrt(3) P)) sum_p G[p][i] theta_p (p ascending), gpred[i][:3] += gscale M^T dy_i;
//              loss = (2 / (sqrt(3) P)) sum_p W_p in a fixed order
//
// Two launches, no float atomics: every coefficient, every gradient element and the scalar is written by one thread in a
// fixed order.
#include "internal.h"
#include "sort_match.h"

namespace {

constexpr int PS_T = 1024;          // threads of the sort/match workgroup = the largest row count
constexpr int PS_LD = 1024;         // row stride of the coefficient matrix
constexpr int PS_MAX_PROJ = 1024;

struct PaletteSlicedWs {
  float* G;                // (P x PS_LD) dW_p/da at the prediction row, columns >= n never read
  float* Wp;               // (P) the directions' costs
  bool plan(Workspace& w, int n_proj) {
    G = w.take<float>((size_t)n_proj * PS_LD);
    Wp = w.take<float>(n_proj);
    return w.ok();
  }
};

// <theta, yuv(row)>: convert_rgb_to_yuv with the constants of palette_prepare_kernel_body, every product rounded on its own
// and every sum taken left to right (no contraction): the float32 restatement of the tests computes the same bits, so both
// decide every near-tie of a sort and every sign alike
__device__ __forceinline__ float ps_project(const float* __restrict__ row, int convert, float t0, float t1, float t2) {
#pragma clang fp contract(off)
  const float R = row[0], G = row[1], B = row[2];
  float Y = R, U = G, V = B;
  if (convert) {
    Y = R * 0.299f + G * 0.587f + B * 0.114f;
    U = R * -0.14714119f + G * -0.28886916f + B * 0.43601035f;
    V = R * 0.61497538f + G * -0.51496512f + B * -0.10001026f;
  }
  return t0 * Y + t1 * U + t2 * V;
}

// One direction a workgroup.  Thread tid holds one (key, row) pair of each side in registers (~0 past the side's end: sorts
// last); both are sorted at once over the first S = pow2 >= max(n, ns) slots, then matched (sort_match.h): the overlaps are
// whole numbers, so the coefficient's sum is exact (at most ns <= 1024) and only the cost is rounded.  LDS: 32 KB + 4 KB.
__global__ __launch_bounds__(PS_T) void palette_sliced_match_kernel(const float* __restrict__ style, int ns,
                                                                    const float* __restrict__ pred, int n, int ld, int convert,
                                                                    const float* __restrict__ dirs, float* __restrict__ G,
                                                                    float* __restrict__ Wp) {
  __shared__ unsigned long long x[2][2 * PS_T];
  __shared__ float sb[PS_T];
  __shared__ double red[PS_T / 64];
  const int p = blockIdx.x, tid = threadIdx.x;
  const float t0 = dirs[3 * p], t1 = dirs[3 * p + 1], t2 = dirs[3 * p + 2];
  unsigned long long v[2] = {tid < n ? ordered_pack(ps_project(pred + (size_t)tid * ld, convert, t0, t1, t2), tid) : ~0ull,
                             tid < ns ? ordered_pack(ps_project(style + (size_t)tid * ld, convert, t0, t1, t2), tid) : ~0ull};
  int S = 64;
  while (S < max(n, ns)) S <<= 1;
  bitonic_sort_1024<2>(v, x[0], x[1], S);
  const QuantileMatch m = quantile_match<AbsoluteCost>(v[0], v[1], n, ns, sb);
  if (tid < n) G[(size_t)p * PS_LD + m.row] = m.coef;
  const double s = block_sum_f64_1024((double)m.cost, red);
  if (tid == 0) Wp[p] = (float)s;
}

// One row a thread: the directions in ascending order, then M^T (d_rgb = d_yuv @ M^T as palette_bwd_body) and gscale.  The
// added value is rounded before it is added (no contraction with the sum): into a filled gpred the call leaves its contents
// plus the gradient, bit for bit.  Wave 0 of block 0 also adds the directions' costs: lane l takes l, l + 64, .., the lanes a
// fixed shuffle tree.
__global__ __launch_bounds__(256) void palette_sliced_finish_kernel(const float* __restrict__ G, const float* __restrict__ Wp,
                                                                    const float* __restrict__ dirs, int n, int n_proj, int ld,
                                                                    int convert, float gscale, float* __restrict__ gpred,
                                                                    float* __restrict__ loss_out) {
#pragma clang fp contract(off)
  const double scale = 2.0 / (1.7320508075688772 * (double)n_proj);
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    double s = 0.0;
    for (int p = threadIdx.x; p < n_proj; p += 64) s += (double)Wp[p];
    s = wave_sum(s);
    if (threadIdx.x == 0) loss_out[0] = (float)(s * scale);
  }
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float d0 = 0.f, d1 = 0.f, d2 = 0.f;
  for (int p = 0; p < n_proj; ++p) {
    const float g = G[(size_t)p * PS_LD + i];
    d0 += g * dirs[3 * p];
    d1 += g * dirs[3 * p + 1];
    d2 += g * dirs[3 * p + 2];
  }
  const float c = (float)scale;
  d0 *= c; d1 *= c; d2 *= c;
  float r0 = d0, r1 = d1, r2 = d2;
  if (convert) {
    r0 = d0 * 0.299f + d1 * -0.14714119f + d2 * 0.61497538f;
    r1 = d0 * 0.587f + d1 * -0.28886916f + d2 * -0.51496512f;
    r2 = d0 * 0.114f + d1 * 0.43601035f + d2 * -0.10001026f;
  }
  const float v0 = gscale * r0, v1 = gscale * r1, v2 = gscale * r2;
  float* g = gpred + (size_t)i * ld;
  g[0] = g[0] + v0;
  g[1] = g[1] + v1;
  g[2] = g[2] + v2;
}

bool ps_sizes_ok(int ns, int n, int n_proj) {
  return ns > 0 && ns <= PS_T && n > 0 && n <= PS_T && n_proj > 0 && n_proj <= PS_MAX_PROJ;
}

}  // namespace

extern "C" {

size_t strotss_palette_sliced_workspace_bytes(int ns, int n, int n_proj) {
  if (!ps_sizes_ok(ns, n, n_proj)) return 0;
  Workspace w = Workspace::planner();
  PaletteSlicedWs s;
  s.plan(w, n_proj);
  return w.off;
}

int strotss_palette_sliced_fwd_bwd(const float* style, int ns, const float* pred, int n, int ld, int rgb_to_yuv,
                                   const float* dirs, int n_proj, float gscale, float* gpred, float* loss_out,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  ST_CHECK_ARG(style && pred && dirs && gpred && loss_out && workspace && ns > 0 && n > 0 && n_proj > 0 && ld >= 3,
               STROTSS_EINVAL);
  ST_CHECK_ARG(ps_sizes_ok(ns, n, n_proj), STROTSS_ERANGE);
  Workspace w(workspace, workspace_bytes);
  PaletteSlicedWs s;
  ST_CHECK_ARG(s.plan(w, n_proj), STROTSS_EINVAL);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(palette_sliced_match_kernel, dim3(n_proj), dim3(PS_T), 0, st, style, ns, pred, n, ld, rgb_to_yuv, dirs,
                     s.G, s.Wp);
  ST_LAUNCH_OK();
  hipLaunchKernelGGL(palette_sliced_finish_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, s.G, s.Wp, dirs, n, n_proj, ld,
                     rgb_to_yuv, gscale, gpred, loss_out);
  ST_LAUNCH_RET();
}

}  // extern "C"
