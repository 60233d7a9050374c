// Log-domain Sinkhorn as the step's style term: the scalings of strotss_sinkhorn_cos_fwd_bwd_panels
// kept as their logarithms, phi = log u and psi = log v, so that no kernel matrix exp(-l M) is ever formed and no clamp is
// needed.  M[i][j] is the cosine distance (i < ns style row, j < n prediction row), px = 1 / ns, py = 1 / n, psi_0 = 0:
//
//     phi_t[i] = log px - LSE_j(psi_{t-1}[j] - l M[i][j])          column pass + its reduction   (t = 1 .. T)
//     psi_t[j] = log py - LSE_i(phi_t[i]    - l M[i][j])           one workgroup per prediction row
//     loss     = sum_ij exp(phi_T[i] + psi_T[j] - l M[i][j]) M[i][j]
//
// Every pass reads Mt (pred-major: Mt[j][i], row stride ldm) and forms exp(arg - max) on the fly.  The reverse sweep walks
// the same two reduction shapes: the adjoint of an LSE is its softmax, exp(phi_t[i] + psi_{t-1}[j] - l M) / px over j and
// exp(phi_t[i] + psi_t[j] - l M) / py over i, each at most 1, so its sums need no shift:
//
//     gpsi_T[j]     = cost[j] = sum_i exp(phi_T[i] + psi_T[j] - l M) M
//     gphi_t[i]     = sum_j exp(phi_t[i] + psi_t[j] - l M) ([t == T] M - gpsi_t[j] / py)
//     gpsi_{t-1}[j] = -sum_i exp(phi_t[i] + psi_{t-1}[j] - l M) gphi_t[i] / px
//     dM[i][j]      = exp(phi_T[i] + psi_T[j] - l M) (1 - l M)
//                     + l sum_t (exp(phi_t[i] + psi_t[j] - l M) gpsi_t[j] / py + exp(phi_t[i] + psi_{t-1}[j] - l M) gphi_t[i] / px)
//
// and the chain rule of the cosine distance is the linear form's: W = -dM rs, q[j] = sum_i -dM (1 - M), one product on
// st_selfsim_bwd_gemm.  No float atomics: every value is written by one thread, every reduction has a fixed order.
#include <math.h>

#include "internal.h"

namespace {

#define SKL_CHUNKS 16            // row chunks of the column pass (COL_CHUNKS of losses.hip)
#define SKL_MAX_ITERS 64
#define SKL_MAX_L 1000.0f

struct SinkhornLogWs {
  float *Mt, *W, *PHI, *DA, *PSI, *DB, *pmax, *psum, *q;
  int ldm;
  bool plan(Workspace& w, int ns, int n, int T) {
    ldm = round_up(ns, 32);
    const int rows = round_up(n, 64);
    Mt = w.take<float>((size_t)rows * ldm); W = w.take<float>((size_t)rows * ldm);
    PHI = w.take<float>((size_t)T * ns); DA = w.take<float>((size_t)T * ns);           // phi_t, gphi_t at row t - 1
    PSI = w.take<float>((size_t)(T + 1) * n); DB = w.take<float>((size_t)T * n);       // psi_t at row t, gpsi_t at row t - 1
    pmax = w.take<float>((size_t)SKL_CHUNKS * ns); psum = w.take<float>((size_t)SKL_CHUNKS * ns);
    q = w.take<float>(n);
    return w.ok();
  }
};

// (m, s) <- (m, s) (+) (m2, s2) of two log-sum-exp partials: the sum is s exp(m).  An empty partial is (-inf, 0); two of
// them combine to (-inf, 0) again without forming -inf - (-inf).
__device__ __forceinline__ void lse_combine(float& m, float& s, float m2, float s2) {
  const float mx = fmaxf(m, m2);
  if (mx == -INFINITY) { s = 0.f; return; }
  s = s * __expf(m - mx) + s2 * __expf(m2 - mx);
  m = mx;
}
// one more term a (finite) of an online log-sum-exp
__device__ __forceinline__ void lse_push(float& m, float& s, float a) {
  if (a > m) { s = s * __expf(m - a) + 1.f; m = a; }
  else s += __expf(a - m);
}

// Column pass, stage 1: (max, sum) of psi[j] - l Mt[j][i] over the rows j of chunk blockIdx.y, for 64 columns i a block.
__global__ __launch_bounds__(256) void skl_col_lse_partial_kernel(const float* __restrict__ Mt, int n, int ns, int ldm, float l,
                                                                  const float* __restrict__ psi, float* __restrict__ pmax,
                                                                  float* __restrict__ psum) {
  __shared__ float sm[4][64], ss[4][64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + c;
  const int per = (n + SKL_CHUNKS - 1) / SKL_CHUNKS;
  const int j0 = blockIdx.y * per, j1 = min(n, j0 + per);
  float m = -INFINITY, s = 0.f;
  if (col < ns)
    for (int j = j0 + g; j < j1; j += 4) lse_push(m, s, psi[j] - l * Mt[(size_t)j * ldm + col]);
  sm[g][c] = m; ss[g][c] = s;
  __syncthreads();
  if (g == 0 && col < ns) {
#pragma unroll
    for (int k = 1; k < 4; ++k) lse_combine(m, s, sm[k][c], ss[k][c]);
    pmax[(size_t)blockIdx.y * ns + col] = m;
    psum[(size_t)blockIdx.y * ns + col] = s;
  }
}
// stage 2: the chunks' pairs in the order 0 .. 15, phi[i] = log px - (max + log sum)
__global__ __launch_bounds__(256) void skl_col_lse_final_kernel(const float* __restrict__ pmax, const float* __restrict__ psum,
                                                                int ns, float log_px, float* __restrict__ phi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ns) return;
  float m = pmax[i], s = psum[i];
#pragma unroll
  for (int k = 1; k < SKL_CHUNKS; ++k) lse_combine(m, s, pmax[(size_t)k * ns + i], psum[(size_t)k * ns + i]);
  phi[i] = log_px - (m + logf(s));
}
// psi[j] = log py - LSE_i(phi[i] - l Mt[j][i]), one workgroup per prediction row: one read of the row, every thread an
// online partial, the partials rescaled to the row maximum.
__global__ __launch_bounds__(256) void skl_row_lse_kernel(const float* __restrict__ Mt, int ns, int ldm, float l,
                                                          const float* __restrict__ phi, float log_py,
                                                          float* __restrict__ psi) {
  __shared__ float red[4];
  const int j = blockIdx.x;
  const float* mr = Mt + (size_t)j * ldm;
  float m = -INFINITY, s = 0.f;
  for (int i = threadIdx.x; i < ns; i += 256) lse_push(m, s, phi[i] - l * mr[i]);
  const float mx = block_max_256(m, red);            // finite: ns >= 1
  const float tot = block_sum_256(s * __expf(m - mx), red);      // a thread without terms: 0 * exp(-inf) = 0
  if (threadIdx.x == 0) psi[j] = log_py - (mx + logf(tot));
}
// cost[j] = gpsi_T[j] = sum_i exp(phi_T[i] + psi_T[j] - l M) M; every exponent is <= log px
__global__ __launch_bounds__(256) void skl_cost_kernel(const float* __restrict__ Mt, int ns, int ldm, float l,
                                                       const float* __restrict__ phi, const float* __restrict__ psi,
                                                       float* __restrict__ gpsi) {
  __shared__ float red[4];
  const int j = blockIdx.x;
  const float* mr = Mt + (size_t)j * ldm;
  const float pj = psi[j];
  float a = 0.f;
  for (int i = threadIdx.x; i < ns; i += 256) {
    const float m = mr[i];
    a += __expf(phi[i] + pj - l * m) * m;
  }
  const float b = block_sum_256(a, red);
  if (threadIdx.x == 0) gpsi[j] = b;
}
__global__ __launch_bounds__(256) void skl_reduce_sum_kernel(const float* __restrict__ x, int count, float* __restrict__ out) {
  __shared__ float red[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < count; i += 256) a += x[i];
  a = block_sum_256(a, red);
  if (threadIdx.x == 0) out[0] = a;
}
// Reverse column pass, stage 1: sum_j exp(phi[i] + psi[j] - l M) ((top ? M : 0) - gpsi[j] / py) over the chunk's rows
__global__ __launch_bounds__(256) void skl_col_adj_partial_kernel(const float* __restrict__ Mt, int n, int ns, int ldm, float l,
                                                                  const float* __restrict__ phi, const float* __restrict__ psi,
                                                                  const float* __restrict__ gpsi, float inv_py, int top,
                                                                  float* __restrict__ part) {
  __shared__ float sm[4][64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + c;
  const int per = (n + SKL_CHUNKS - 1) / SKL_CHUNKS;
  const int j0 = blockIdx.y * per, j1 = min(n, j0 + per);
  float a = 0.f;
  if (col < ns) {
    const float pi = phi[col];
    for (int j = j0 + g; j < j1; j += 4) {
      const float m = Mt[(size_t)j * ldm + col];
      a += __expf(pi + psi[j] - l * m) * ((top ? m : 0.f) - gpsi[j] * inv_py);
    }
  }
  sm[g][c] = a;
  __syncthreads();
  if (g == 0 && col < ns) part[(size_t)blockIdx.y * ns + col] = (sm[0][c] + sm[1][c]) + (sm[2][c] + sm[3][c]);
}
// stage 2: gphi[i] = the chunks' sums in the order 0 .. 15
__global__ __launch_bounds__(256) void skl_col_adj_final_kernel(const float* __restrict__ part, int ns, float* __restrict__ gphi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ns) return;
  float a = 0.f;
#pragma unroll
  for (int k = 0; k < SKL_CHUNKS; ++k) a += part[(size_t)k * ns + i];
  gphi[i] = a;
}
// Reverse row pass: gpsi_prev[j] = -sum_i exp(phi[i] + psi_prev[j] - l M) gphi[i] / px   (phi = phi_t, psi_prev = psi_{t-1})
__global__ __launch_bounds__(256) void skl_row_adj_kernel(const float* __restrict__ Mt, int ns, int ldm, float l,
                                                          const float* __restrict__ phi, const float* __restrict__ gphi,
                                                          const float* __restrict__ psi_prev, float inv_px,
                                                          float* __restrict__ gpsi_prev) {
  __shared__ float red[4];
  const int j = blockIdx.x;
  const float* mr = Mt + (size_t)j * ldm;
  const float pj = psi_prev[j];
  float a = 0.f;
  for (int i = threadIdx.x; i < ns; i += 256) a += __expf(phi[i] + pj - l * mr[i]) * gphi[i];
  const float b = block_sum_256(a, red);
  if (threadIdx.x == 0) gpsi_prev[j] = -b * inv_px;
}
// Gradient assembly, one workgroup per prediction row j (dM as in the head of this file):
//   W[j][i] = -dM * rs[i]   (operand of the backward GEMM against the style rows),   q[j] = sum_i -dM (1 - M)
__global__ __launch_bounds__(256) void skl_assemble_kernel(const float* __restrict__ Mt, int ns, int ldm, int T, float l,
                                                           const float* __restrict__ PHI, const float* __restrict__ DA,
                                                           const float* __restrict__ PSI, const float* __restrict__ DB, int n,
                                                           float inv_px, float inv_py, const float* __restrict__ rs,
                                                           float* __restrict__ W, float* __restrict__ q) {
  __shared__ float red[4];
  __shared__ float psj[SKL_MAX_ITERS + 1], gbj[SKL_MAX_ITERS];
  const int j = blockIdx.x;
  for (int t = threadIdx.x; t <= T; t += 256) psj[t] = PSI[(size_t)t * n + j];
  for (int t = threadIdx.x; t < T; t += 256) gbj[t] = DB[(size_t)t * n + j] * inv_py;      // gpsi_{t+1}[j] / py
  __syncthreads();
  float qs = 0.f;
  for (int i = threadIdx.x; i < ldm; i += 256) {
    float w = 0.f;
    if (i < ns) {
      const float m = Mt[(size_t)j * ldm + i];
      const float lm = l * m;
      float s = 0.f;
      for (int t = 0; t < T; ++t) {
        const float a = PHI[(size_t)t * ns + i] - lm;
        s += __expf(a + psj[t + 1]) * gbj[t] + __expf(a + psj[t]) * (DA[(size_t)t * ns + i] * inv_px);
      }
      const float dm = __expf(PHI[(size_t)(T - 1) * ns + i] + psj[T] - lm) * (1.f - lm) + l * s;
      w = -dm;
      qs += w * (1.f - m);
      w *= rs[i];
    }
    W[(size_t)j * ldm + i] = w;
  }
  const float tot = block_sum_256(qs, red);
  if (threadIdx.x == 0) q[j] = tot;
}

// The scalings, the cost and the reverse sweep on the pred-major cost matrix s.Mt: fills PHI, PSI, DA, DB and loss_out.
int sinkhorn_log_iterate(SinkhornLogWs& s, int ns, int n, float l, int T, float* loss_out, hipStream_t st) {
  const int ldm = s.ldm;
  const float inv_px = (float)ns, inv_py = (float)n;
  const float log_px = -logf((float)ns), log_py = -logf((float)n);
  const dim3 gcol(cdiv(ns, 64), SKL_CHUNKS), gfin(cdiv(ns, 256));
  ST_TRY((int)hipMemsetAsync(s.PSI, 0, sizeof(float) * (size_t)n, st));                        // psi_0 = 0
  for (int t = 1; t <= T; ++t) {
    hipLaunchKernelGGL(skl_col_lse_partial_kernel, gcol, dim3(256), 0, st, s.Mt, n, ns, ldm, l, s.PSI + (size_t)(t - 1) * n,
                       s.pmax, s.psum);
    hipLaunchKernelGGL(skl_col_lse_final_kernel, gfin, dim3(256), 0, st, s.pmax, s.psum, ns, log_px,
                       s.PHI + (size_t)(t - 1) * ns);
    hipLaunchKernelGGL(skl_row_lse_kernel, dim3(n), dim3(256), 0, st, s.Mt, ns, ldm, l, s.PHI + (size_t)(t - 1) * ns, log_py,
                       s.PSI + (size_t)t * n);
  }
  ST_LAUNCH_OK();
  const float* phiT = s.PHI + (size_t)(T - 1) * ns;
  const float* psiT = s.PSI + (size_t)T * n;
  hipLaunchKernelGGL(skl_cost_kernel, dim3(n), dim3(256), 0, st, s.Mt, ns, ldm, l, phiT, psiT, s.DB + (size_t)(T - 1) * n);
  hipLaunchKernelGGL(skl_reduce_sum_kernel, dim3(1), dim3(256), 0, st, s.DB + (size_t)(T - 1) * n, n, loss_out);
  for (int t = T; t >= 1; --t) {
    hipLaunchKernelGGL(skl_col_adj_partial_kernel, gcol, dim3(256), 0, st, s.Mt, n, ns, ldm, l, s.PHI + (size_t)(t - 1) * ns,
                       s.PSI + (size_t)t * n, s.DB + (size_t)(t - 1) * n, inv_py, t == T ? 1 : 0, s.pmax);
    hipLaunchKernelGGL(skl_col_adj_final_kernel, gfin, dim3(256), 0, st, s.pmax, ns, s.DA + (size_t)(t - 1) * ns);
    if (t > 1)
      hipLaunchKernelGGL(skl_row_adj_kernel, dim3(n), dim3(256), 0, st, s.Mt, ns, ldm, l, s.PHI + (size_t)(t - 1) * ns,
                         s.DA + (size_t)(t - 1) * ns, s.PSI + (size_t)(t - 1) * n, inv_px, s.DB + (size_t)(t - 2) * n);
  }
  ST_LAUNCH_OK();
  const int rows = round_up(n, 64);
  if (rows > n) ST_TRY((int)hipMemsetAsync(s.W + (size_t)n * ldm, 0, sizeof(float) * (size_t)(rows - n) * ldm, st));
  return 0;
}

}  // namespace

extern "C" {

size_t strotss_sinkhorn_log_step_workspace_bytes(int ns, int n, int n_iter) {
  if (ns <= 0 || n <= 0 || n_iter < 1 || n_iter > SKL_MAX_ITERS) return 0;
  Workspace w = Workspace::planner();
  SinkhornLogWs s;
  s.plan(w, ns, n, n_iter);
  return w.off;
}

int strotss_sinkhorn_log_cos_fwd_bwd_panels(const float* style, const float* rs, const void* style_panels, int ns,
                                            const float* pred, const float* pred_inv_norm, const void* pred_panels, int n,
                                            int d, int ld, float l, int n_iter, float gscale, float* gpred, float* loss_out,
                                            void* workspace, size_t workspace_bytes, void* stream) {
  // the panels come as a pair: both (cost matrix on the bf16x3 core) or neither (f32 MFMA from the rows)
  ST_CHECK_ARG(style && rs && pred && pred_inv_norm && gpred && loss_out && workspace && ns > 0 && n > 0 && d > 0 && ld >= d &&
               (style_panels != nullptr) == (pred_panels != nullptr), STROTSS_EINVAL);
  ST_CHECK_ARG(ld % 32 == 0, STROTSS_EALIGN);
  ST_CHECK_ARG(l > 0.f && l <= SKL_MAX_L && n_iter >= 1 && n_iter <= SKL_MAX_ITERS, STROTSS_ERANGE);
  Workspace w(workspace, workspace_bytes);
  SinkhornLogWs s;
  ST_CHECK_ARG(s.plan(w, ns, n, n_iter), STROTSS_EINVAL);
  hipStream_t st = (hipStream_t)stream;
  const int ldm = s.ldm, T = n_iter;
  if (pred_panels) ST_TRY(st_cosine_distance_x3(pred_panels, pred_inv_norm, n, style_panels, rs, ns, ld, 0, s.Mt, ldm, 1, 0, 0, 0, st));
  else ST_TRY(st_cosine_distance(pred, pred_inv_norm, n, style, rs, ns, ld, s.Mt, ldm, st));     // Mt[j][i] = 1 - <yhat_j, xhat_i>
  ST_TRY(sinkhorn_log_iterate(s, ns, n, l, T, loss_out, st));
  hipLaunchKernelGGL(skl_assemble_kernel, dim3(n), dim3(256), 0, st, s.Mt, ns, ldm, T, l, s.PHI, s.DA, s.PSI, s.DB, n,
                     (float)ns, (float)n, rs, s.W, s.q);
  ST_LAUNCH_OK();
  return st_selfsim_bwd_gemm(s.W, ldm, ldm, style, pred, pred_inv_norm, s.q, n, ld, gscale, gpred, st);
}

}  // extern "C"
