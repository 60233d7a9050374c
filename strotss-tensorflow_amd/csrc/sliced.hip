// Sliced Wasserstein distance as the step's style term: the L2-normalised prediction and style rows
// are projected on P Rademacher directions, each direction's two projected sets are sorted, and the exact 1-D transport
// between the two uniform atom sets (quantile-cell overlaps) gives the direction's cost and the gradient coefficients.
//
//     directions   eps[p][k] = +-1 from Philox: bit k & 31 of word (k >> 5) & 3 of philox(ctr = (k >> 7, 2, t, p), key = seed),
//                  1 -> +1, 0 -> -1, columns k >= d zero; t = *counter.  nn/rand.py:sliced_signs is the host twin.
//     projection   a[p][i] = <eps_p, x_i> r_i, b[p][j] = <eps_p, s_j> rs_j on the GEMM cores of gemm.hip (x3 panels or f32 MFMA),
//                  the reciprocal norms in the epilogue, one direction's values contiguous
//     sort, match  one workgroup of 1024 threads per direction: both sides by (value, row) on the bitonic network of sort_match.h,
//                  then W_p = sum_ij len_ij (a_(i) - b_(j))^2 and dloss/da at the element's original row
//     backward     q_i = sum_p G[p][i] a[p][i], then dx += gscale r_i (G^T eps - xhat_i q_i) (st_selfsim_bwd_gemm_tn)
//     finish       loss = sum_p W_p / (2 P) in a fixed order, *counter = t + 1
//
// No float atomics: every coefficient, every gradient element and every scalar is written by one thread in a fixed order.
#include "internal.h"
#include "philox.h"
#include "sort_match.h"

namespace {

constexpr int SL_T = 1024;          // threads of the sort/match workgroup = the largest row count
constexpr int SL_LD = 1024;         // row stride of the per-direction matrices (projections, coefficients)
constexpr int SL_MAX_PROJ = 1024;

struct SlicedWs {
  float* E;                // (kpad x ld) the directions as f32, rows P .. kpad - 1 zero: B operand of the backward product
  unsigned short* Ep;      // x3 panels of the P directions (the h plane holds +-1, the m and l planes zero)
  float* A;                // (P x SL_LD) projections of the prediction rows
  float* B;                // (P x SL_LD) projections of the style rows
  float* Gt;               // (kpad x SL_LD) dloss/da, one direction a row; rows P .. and columns n .. round_up(n, 4) - 1 zero
  float* Wp;               // (P) the directions' costs
  float* q;                // (SL_LD) q_i = <xhat_i, dxhat_i>
  int kpad;
  bool plan(Workspace& w, int ld, int n_proj) {
    kpad = round_up(n_proj, 32);
    E = w.take<float>((size_t)kpad * ld);
    Ep = w.take<unsigned short>((size_t)3 * n_proj * ld);
    A = w.take<float>((size_t)n_proj * SL_LD);
    B = w.take<float>((size_t)n_proj * SL_LD);
    Gt = w.take<float>((size_t)kpad * SL_LD);
    Wp = w.take<float>(n_proj);
    q = w.take<float>(SL_LD);
    return w.ok();
  }
};

// Row p of the direction matrix, 8 consecutive columns a thread: f32 for the f32 products, and the x3 panel image
// (mfma_x3.h: element (kb, plane, row, k) at ((kb * 3 + plane) * rows + row) * 32 + k) whose h plane is the value itself.
__global__ __launch_bounds__(256) void sliced_directions_kernel(const unsigned* __restrict__ counter, unsigned seed_lo,
                                                                 unsigned seed_hi, int n_proj, int d, int ld,
                                                                 float* __restrict__ E, unsigned short* __restrict__ Ep) {
  const int p = blockIdx.x;
  const unsigned t = *counter;
  for (int k0 = threadIdx.x * 8; k0 < ld; k0 += 256 * 8) {
    unsigned bits = 0;
    if (p < n_proj && k0 < d) {
      unsigned o4[4];
      philox4x32_10((unsigned)(k0 >> 7), 2u, t, (unsigned)p, seed_lo, seed_hi, o4);
      bits = (o4[(k0 >> 5) & 3] >> (k0 & 31)) & 0xFFu;
    }
    float v[8];
    unsigned short h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool live = p < n_proj && k0 + e < d, plus = (bits >> e) & 1u;
      v[e] = live ? (plus ? 1.f : -1.f) : 0.f;
      h[e] = live ? (plus ? (unsigned short)0x3F80 : (unsigned short)0xBF80) : (unsigned short)0;    // bf16 of +-1
    }
    float* row = E + (size_t)p * ld + k0;
    *reinterpret_cast<f32x4*>(row) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(row + 4) = f32x4{v[4], v[5], v[6], v[7]};
    if (p < n_proj) {
      const uint4 hv = make_uint4(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16), h[4] | ((unsigned)h[5] << 16),
                                  h[6] | ((unsigned)h[7] << 16));
      const size_t o = ((size_t)(k0 >> 5) * 3 * n_proj + p) * 32 + (k0 & 31);
      *reinterpret_cast<uint4*>(Ep + o) = hv;
      *reinterpret_cast<uint4*>(Ep + o + (size_t)n_proj * 32) = make_uint4(0u, 0u, 0u, 0u);
      *reinterpret_cast<uint4*>(Ep + o + (size_t)2 * n_proj * 32) = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

// One direction a workgroup.  Thread tid holds one (key, row) pair of each side in registers (~0 past the side's end: sorts
// last); both are sorted at once over the first S = pow2 >= max(n, ns) slots, then matched (sort_match.h).  LDS: 32 KB + 4 KB.
__global__ __launch_bounds__(SL_T) void sliced_match_kernel(const float* __restrict__ A, const float* __restrict__ B, int n,
                                                            int ns, int n_proj, float* __restrict__ Gt,
                                                            float* __restrict__ Wp) {
  __shared__ unsigned long long x[2][2 * SL_T];
  __shared__ float sb[SL_T];
  __shared__ double red[SL_T / 64];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n4 = (n + 3) & ~3;
  float* g_row = Gt + (size_t)p * SL_LD;
  if (p >= n_proj) {                                     // the backward product's K padding; uniform, before any barrier
    if (tid < n4) g_row[tid] = 0.f;
    return;
  }
  unsigned long long v[2] = {tid < n ? ordered_pack(A[(size_t)p * SL_LD + tid], tid) : ~0ull,
                             tid < ns ? ordered_pack(B[(size_t)p * SL_LD + tid], tid) : ~0ull};
  int S = 64;
  while (S < max(n, ns)) S <<= 1;
  bitonic_sort_1024<2>(v, x[0], x[1], S);
  const QuantileMatch m = quantile_match<SquaredCost>(v[0], v[1], n, ns, sb);
  if (tid < n) g_row[m.row] = m.coef / (float)n_proj;
  else if (tid < n4) g_row[tid] = 0.f;
  const double s = block_sum_f64_1024((double)m.cost, red);
  if (tid == 0) Wp[p] = (float)s;
}

// q_i = sum_p G[p][i] a[p][i]: 64 rows a workgroup, wave wv takes the directions wv, wv + 16, ..; the 16 partial sums are
// added in wave order.
__global__ __launch_bounds__(SL_T) void sliced_rowdot_kernel(const float* __restrict__ Gt, const float* __restrict__ A, int n,
                                                             int n_proj, float* __restrict__ q) {
  __shared__ double part[SL_T / 64][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  double s = 0.0;
  if (i < n)
    for (int p = wv; p < n_proj; p += SL_T / 64) s += (double)Gt[(size_t)p * SL_LD + i] * (double)A[(size_t)p * SL_LD + i];
  part[wv][lane] = s;
  __syncthreads();
  if (wv == 0 && i < n) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < SL_T / 64; ++k) t += part[k][lane];
    q[i] = (float)t;
  }
}

// loss = sum_p W_p / (2 P): lane l adds the directions l, l + 64, .., the lanes by a fixed shuffle tree; the counter moves on
__global__ __launch_bounds__(64) void sliced_finish_kernel(const float* __restrict__ Wp, int n_proj, float* __restrict__ loss_out,
                                                           unsigned* __restrict__ counter) {
  double s = 0.0;
  for (int p = threadIdx.x; p < n_proj; p += 64) s += (double)Wp[p];
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    loss_out[0] = (float)(s / (2.0 * n_proj));
    *counter = *counter + 1u;
  }
}

}  // namespace

extern "C" {

size_t strotss_sliced_workspace_bytes(int ns, int n, int ld, int n_proj) {
  if (ns <= 0 || ns > SL_T || n <= 0 || n > SL_T || ld <= 0 || ld % 32 != 0 || n_proj < 1 || n_proj > SL_MAX_PROJ) return 0;
  Workspace w = Workspace::planner();
  SlicedWs s;
  s.plan(w, ld, n_proj);
  return w.off;
}

int strotss_sliced_cos_fwd_bwd(const float* style, const float* rs, const void* style_panels, int ns, const float* pred,
                               const float* pred_inv_norm, const void* pred_panels, int n, int d, int ld, int n_proj,
                               unsigned seed_lo, unsigned seed_hi, unsigned* counter, float gscale, float* gpred,
                               float* loss_out, void* workspace, size_t workspace_bytes, void* stream) {
  // the panels come as a pair: both (projections on the bf16x3 core) or neither (f32 MFMA from the rows)
  ST_CHECK_ARG(style && rs && pred && pred_inv_norm && counter && gpred && loss_out && workspace && ns > 0 && n > 0 && d > 0 &&
               ld >= d && n_proj > 0 && (style_panels != nullptr) == (pred_panels != nullptr), STROTSS_EINVAL);
  ST_CHECK_ARG(ld % 32 == 0, STROTSS_EALIGN);
  ST_CHECK_ARG(n <= SL_T && ns <= SL_T && n_proj <= SL_MAX_PROJ, STROTSS_ERANGE);
  Workspace w(workspace, workspace_bytes);
  SlicedWs s;
  ST_CHECK_ARG(s.plan(w, ld, n_proj), STROTSS_EINVAL);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sliced_directions_kernel, dim3(s.kpad), dim3(256), 0, st, counter, seed_lo, seed_hi, n_proj, d, ld, s.E,
                     s.Ep);
  ST_LAUNCH_OK();
  if (pred_panels) {
    ST_TRY(st_rows_project_x3(s.Ep, n_proj, pred_panels, pred_inv_norm, n, ld, s.A, SL_LD, st));
    ST_TRY(st_rows_project_x3(s.Ep, n_proj, style_panels, rs, ns, ld, s.B, SL_LD, st));
  } else {
    ST_TRY(st_rows_project(s.E, n_proj, pred, pred_inv_norm, n, ld, s.A, SL_LD, st));
    ST_TRY(st_rows_project(s.E, n_proj, style, rs, ns, ld, s.B, SL_LD, st));
  }
  hipLaunchKernelGGL(sliced_match_kernel, dim3(s.kpad), dim3(SL_T), 0, st, s.A, s.B, n, ns, n_proj, s.Gt, s.Wp);
  ST_LAUNCH_OK();
  hipLaunchKernelGGL(sliced_rowdot_kernel, dim3(cdiv(n, 64)), dim3(SL_T), 0, st, s.Gt, s.A, n, n_proj, s.q);
  ST_LAUNCH_OK();
  ST_TRY(st_selfsim_bwd_gemm_tn(s.Gt, SL_LD, s.kpad, s.E, pred, pred_inv_norm, s.q, n, ld, gscale, gpred, st));
  hipLaunchKernelGGL(sliced_finish_kernel, dim3(1), dim3(64), 0, st, s.Wp, n_proj, loss_out, counter);
  ST_LAUNCH_RET();
}

}  // extern "C"
