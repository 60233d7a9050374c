// Pixel-space priors of the step, between the trunk's pixel gradient and the fold adjoint:
//   - pool_mean_kernel: P_p of an (h, w, ch) array, cells of p x p pixels, partial cells on the last row / column averaged
//     over the pixels they cover.  Once per scale for the content and the weight map, and once per step and pool size > 1 for
//     the folded image (the same kernel, the same order of additions: x == c gives P_p(x) == P_p(c) bit for bit).
//   - detail_fwd_bwd_kernel: one launch per pool size.  D = L (P_p(x) - P_p(c)) with L the graph Laplacian of the cell grid,
//     loss = (1 / (3 hp wp)) sum m D^2, gimg += (2 gscale / (3 hp wp cnt)) L (m D) at every pixel of the cell.
//   - tv_fwd_bwd_kernel: one launch.  loss = (1 / (3 h w)) sum (sqrt(dx^2 + dy^2 + eps^2) - eps), forward differences that
//     are 0 in the last column / row, gimg += gscale * dloss/dimg.
// Scalars by ticket_sum_256 (csrc/ticket_sum.h): block partials in a fixed tree, summed in a fixed order by the last block,
// no float atomics; every thread reaches it (no kernel below returns early).  A gradient value of exactly 0 is not added: the element of gimg keeps its bits, a -0.0 included.
#include "internal.h"

#include <math.h>

// the arithmetic below is the float32 statement of tests/_pixel_prior_ref.py operation by operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace {

#define PRIOR_TILE_PX 32          // pixels per tile side (TV, and the detail term up to p = 8; p = 16: 4 cells = 64 pixels)
#define PRIOR_MIN_CELLS 4

__host__ __device__ inline int prior_tile_cells(int p) { return PRIOR_TILE_PX / p > PRIOR_MIN_CELLS ? PRIOR_TILE_PX / p : PRIOR_MIN_CELLS; }

// One thread per (cell, channel): every row of the cell summed left to right, the row sums added top to bottom, the total
// divided by the pixel count (rows first: 16 + 16 additions deep at p = 16, not 256).
__global__ __launch_bounds__(256) void pool_mean_kernel(const float* __restrict__ img, int h, int w, int ch, int p, int hp,
                                                        int wp, float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)hp * wp * ch) return;
  const int c = (int)(e % ch);
  const int cell = (int)(e / ch);
  const int i = cell / wp, j = cell - i * wp;
  const int r0 = i * p, s0 = j * p;
  const int r1 = min(r0 + p, h), s1 = min(s0 + p, w);
  float acc = 0.f;
  for (int r = r0; r < r1; ++r) {
    const float* row = img + ((size_t)r * w) * ch + c;
    float racc = 0.f;
    for (int s = s0; s < s1; ++s) racc += row[(size_t)s * ch];
    acc += racc;
  }
  out[e] = acc / (float)((r1 - r0) * (s1 - s0));
}

// One workgroup per tile of tc x tc cells.  LDS: d = X - C on the tile and a 2-cell halo (0 outside the grid), e = m * (L d)
// on the tile and a 1-cell halo (0 outside the grid), g = (coef / cnt) * (L e) on the tile; then the tile's pixels, row by
// row (coalesced), take their cell's g.  X is the pooled image (the image itself at p = 1), C the pooled content, M the cell
// weights or NULL.
__global__ __launch_bounds__(256) void detail_fwd_bwd_kernel(const float* __restrict__ X, const float* __restrict__ Cc,
                                                             const float* __restrict__ M, int h, int w, int hp, int wp, int p,
                                                             int tc, int nbx, float coef, float inv_n, float* __restrict__ gimg,
                                                             float* __restrict__ loss_out, unsigned* __restrict__ ticket,
                                                             float* __restrict__ partials) {
  extern __shared__ float lds[];
  __shared__ float red[4][1];
  __shared__ int is_last;
  const int t = threadIdx.x;
  const int dw = tc + 4, ew = tc + 2;
  float* d = lds;                       // (tc + 4, tc + 4, 3)
  float* e = d + dw * dw * 3;           // (tc + 2, tc + 2, 3)
  float* g = e + ew * ew * 3;           // (tc, tc, 3)
  const int i0 = (int)(blockIdx.x / nbx) * tc, j0 = (int)(blockIdx.x % nbx) * tc;      // the tile's first cell
  for (int k = t; k < dw * dw * 3; k += 256) {
    const int c = k % 3, cell = k / 3;
    const int li = cell / dw, lj = cell - li * dw;
    const int i = i0 - 2 + li, j = j0 - 2 + lj;
    float v = 0.f;
    if (i >= 0 && i < hp && j >= 0 && j < wp) {
      const size_t o = ((size_t)i * wp + j) * 3 + c;
      v = X[o] - Cc[o];
    }
    d[k] = v;
  }
  __syncthreads();
  float acc = 0.f;
  for (int k = t; k < ew * ew * 3; k += 256) {
    const int c = k % 3, cell = k / 3;
    const int li = cell / ew, lj = cell - li * ew;
    const int i = i0 - 1 + li, j = j0 - 1 + lj;
    float v = 0.f;
    if (i >= 0 && i < hp && j >= 0 && j < wp) {
      const float deg = (float)((i > 0) + (i < hp - 1) + (j > 0) + (j < wp - 1));
      const float* q = d + ((li + 1) * dw + (lj + 1)) * 3 + c;
      const float D = deg * q[0] - (((q[-dw * 3] + q[dw * 3]) + q[-3]) + q[3]);
      v = M ? M[(size_t)i * wp + j] * D : D;
      if (li >= 1 && li <= tc && lj >= 1 && lj <= tc) acc += v * D;
    }
    e[k] = v;
  }
  __syncthreads();
  if (coef != 0.f) {
    for (int k = t; k < tc * tc * 3; k += 256) {
      const int c = k % 3, cell = k / 3;
      const int li = cell / tc, lj = cell - li * tc;
      const int i = i0 + li, j = j0 + lj;
      float v = 0.f;
      if (i < hp && j < wp) {
        const float deg = (float)((i > 0) + (i < hp - 1) + (j > 0) + (j < wp - 1));
        const float* q = e + ((li + 1) * ew + (lj + 1)) * 3 + c;
        const float G = deg * q[0] - (((q[-ew * 3] + q[ew * 3]) + q[-3]) + q[3]);
        const int cnt = min(p, h - i * p) * min(p, w - j * p);
        v = G * (coef / (float)cnt);
      }
      g[k] = v;
    }
    __syncthreads();
    const int r0 = i0 * p, s0 = j0 * p;
    const int rows = min(tc * p, h - r0), cols3 = 3 * min(tc * p, w - s0);
    int lp = 0;
    while ((1 << lp) < p) ++lp;
    for (int k = t; k < rows * cols3; k += 256) {
      const int r = k / cols3, c3 = k - r * cols3;
      const int px = c3 / 3, c = c3 - 3 * px;
      const float v = g[((r >> lp) * tc + (px >> lp)) * 3 + c];
      if (v != 0.f) {
        float* o = gimg + ((size_t)(r0 + r) * w + s0) * 3 + c3;
        *o = *o + v;
      }
    }
  }
  float sum[1] = {acc};
  ticket_sum_256(sum, inv_n, loss_out, ticket, partials, red, &is_last);
}

// One workgroup per 32 x 32 pixels.  LDS: x on the tile, one row above / column left of it and one below / right (34 x 34),
// then a = dx / n and b = dy / n on the tile and the row above / column left of it (33 x 33; 0 outside the image).
// dloss/dx(q) = (a(left of q) - a(q)) + (b(above q) - b(q)); the loss term n - eps as (dx^2 + dy^2) / (n + eps), which is
// the same number without the cancellation and exactly 0 on a constant image.
#define TV_XW (PRIOR_TILE_PX + 2)
#define TV_AW (PRIOR_TILE_PX + 1)
__global__ __launch_bounds__(256) void tv_fwd_bwd_kernel(const float* __restrict__ img, int h, int w, int nbx, float eps, float eps2,
                                                         float coef, float inv_n, float* __restrict__ gimg,
                                                         float* __restrict__ loss_out, unsigned* __restrict__ ticket,
                                                         float* __restrict__ partials) {
  __shared__ float xs[TV_XW * TV_XW * 3];
  __shared__ float as[TV_AW * TV_AW * 3];
  __shared__ float bs[TV_AW * TV_AW * 3];
  __shared__ float red[4][1];
  __shared__ int is_last;
  const int t = threadIdx.x;
  const int r0 = (int)(blockIdx.x / nbx) * PRIOR_TILE_PX, s0 = (int)(blockIdx.x % nbx) * PRIOR_TILE_PX;
  for (int k = t; k < TV_XW * TV_XW * 3; k += 256) {
    const int c = k % 3, px = k / 3;
    const int lr = px / TV_XW, ls = px - lr * TV_XW;
    const int r = r0 - 1 + lr, s = s0 - 1 + ls;
    xs[k] = (r >= 0 && r < h && s >= 0 && s < w) ? img[((size_t)r * w + s) * 3 + c] : 0.f;
  }
  __syncthreads();
  float acc = 0.f;
  for (int k = t; k < TV_AW * TV_AW * 3; k += 256) {
    const int c = k % 3, px = k / 3;
    const int lr = px / TV_AW, ls = px - lr * TV_AW;
    const int r = r0 - 1 + lr, s = s0 - 1 + ls;
    float a = 0.f, b = 0.f;
    if (r >= 0 && r < h && s >= 0 && s < w) {
      const float* q = xs + (lr * TV_XW + ls) * 3 + c;
      const float dx = s + 1 < w ? q[3] - q[0] : 0.f;
      const float dy = r + 1 < h ? q[TV_XW * 3] - q[0] : 0.f;
      const float ss = dx * dx + dy * dy;
      const float n = sqrtf(ss + eps2);
      a = dx / n;
      b = dy / n;
      if (lr >= 1 && ls >= 1) acc += ss / (n + eps);
    }
    as[k] = a;
    bs[k] = b;
  }
  __syncthreads();
  if (coef != 0.f) {
    const int rows = min(PRIOR_TILE_PX, h - r0), cols3 = 3 * min(PRIOR_TILE_PX, w - s0);
    for (int k = t; k < rows * cols3; k += 256) {
      const int r = k / cols3, c3 = k - r * cols3;
      const int q = ((r + 1) * TV_AW + 1) * 3 + c3;
      const float v = coef * ((as[q - 3] - as[q]) + (bs[q - TV_AW * 3] - bs[q]));
      if (v != 0.f) {
        float* o = gimg + ((size_t)(r0 + r) * w + s0) * 3 + c3;
        *o = *o + v;
      }
    }
  }
  float sum[1] = {acc};
  ticket_sum_256(sum, inv_n, loss_out, ticket, partials, red, &is_last);
}

inline bool pool_ok(int p) { return p == 1 || p == 2 || p == 4 || p == 8 || p == 16; }
inline long long cells(int n, int p) { return ((long long)n + p - 1) / p; }
inline long long prior_blocks(int h, int w) { return cells(h, PRIOR_TILE_PX) * cells(w, PRIOR_TILE_PX); }
inline size_t detail_partials_bytes(int h, int w) { return ((size_t)4 * (size_t)prior_blocks(h, w) + 15) & ~(size_t)15; }

int launch_pool_mean(const float* img, int h, int w, int ch, int p, float* out, hipStream_t st) {
  const int hp = (int)cells(h, p), wp = (int)cells(w, p);
  const long long n = (long long)hp * wp * ch;
  hipLaunchKernelGGL(pool_mean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, img, h, w, ch, p, hp, wp, out);
  ST_LAUNCH_RET();
}

}  // namespace

int strotss_pool_mean(const float* img, int h, int w, int ch, int p, float* out, void* stream) {
  ST_CHECK_ARG(img && out && h > 0 && w > 0 && (ch == 1 || ch == 3), STROTSS_EINVAL);
  ST_CHECK_ARG(3LL * h * w <= 0x7fffffffLL, STROTSS_EINVAL);
  ST_CHECK_ARG(pool_ok(p), STROTSS_ERANGE);
  ST_CHECK_ARG(aligned16(img) && aligned16(out), STROTSS_EALIGN);
  return launch_pool_mean(img, h, w, ch, p, out, (hipStream_t)stream);
}

size_t strotss_detail_workspace_bytes(int h, int w) {
  if (h <= 0 || w <= 0 || 3LL * h * w > 0x7fffffffLL) return 0;
  return 16 + detail_partials_bytes(h, w) + (size_t)12 * (size_t)(cells(h, 2) * cells(w, 2));
}

int strotss_detail_fwd_bwd(const float* img, int h, int w, const strotss_detail_set_t* set, float* gimg, float* loss_out,
                           void* workspace, void* stream) {
  ST_CHECK_ARG(img && set && gimg && loss_out && workspace && h > 0 && w > 0, STROTSS_EINVAL);
  ST_CHECK_ARG(3LL * h * w <= 0x7fffffffLL, STROTSS_EINVAL);
  const int count = set->count;
  ST_CHECK_ARG(count >= 1 && count <= STROTSS_MAX_DETAIL_POOLS, STROTSS_ERANGE);
  for (int j = 0; j < count; ++j) {
    ST_CHECK_ARG(set->content[j], STROTSS_EINVAL);
    ST_CHECK_ARG(pool_ok(set->pool[j]) && (j == 0 || set->pool[j] > set->pool[j - 1]), STROTSS_ERANGE);
  }
  ST_CHECK_ARG(aligned16(img) && aligned16(gimg) && aligned16(workspace), STROTSS_EALIGN);
  for (int j = 0; j < count; ++j)
    ST_CHECK_ARG(aligned16(set->content[j]) && aligned16(set->weight[j]), STROTSS_EALIGN);
  const hipStream_t st = (hipStream_t)stream;
  unsigned* ticket = (unsigned*)workspace;
  float* partials = (float*)((char*)workspace + 16);
  float* plane = (float*)((char*)workspace + 16 + detail_partials_bytes(h, w));
  for (int j = 0; j < count; ++j) {
    const int p = set->pool[j];
    const int hp = (int)cells(h, p), wp = (int)cells(w, p);
    const float* X = img;                // P_1(x) is x
    if (p > 1) {
      ST_TRY(launch_pool_mean(img, h, w, 3, p, plane, st));
      X = plane;
    }
    const int tc = prior_tile_cells(p);
    const double n = 3.0 * (double)hp * (double)wp;
    const float coef = (float)(2.0 * (double)set->gscale[j] / n), inv_n = (float)(1.0 / n);
    const size_t lds = sizeof(float) * 3 * (size_t)((tc + 4) * (tc + 4) + (tc + 2) * (tc + 2) + tc * tc);
    const int nbx = (int)cells(wp, tc);                    // a flat grid: tile rows x tile columns, row-major
    hipLaunchKernelGGL(detail_fwd_bwd_kernel, dim3((unsigned)(cells(hp, tc) * nbx)), dim3(256), lds, st, X, set->content[j],
                       set->weight[j], h, w, hp, wp, p, tc, nbx, coef, inv_n, gimg, loss_out + j, ticket, partials);
    ST_LAUNCH_OK();
  }
  return 0;
}

size_t strotss_tv_workspace_bytes(int h, int w) {
  if (h <= 0 || w <= 0 || 3LL * h * w > 0x7fffffffLL) return 0;
  return 16 + 4 * (size_t)prior_blocks(h, w);
}

int strotss_tv_fwd_bwd(const float* img, int h, int w, float eps, float gscale, float* gimg, float* loss_out,
                       void* workspace, void* stream) {
  ST_CHECK_ARG(img && gimg && loss_out && workspace && h > 0 && w > 0, STROTSS_EINVAL);
  ST_CHECK_ARG(3LL * h * w <= 0x7fffffffLL, STROTSS_EINVAL);
  ST_CHECK_ARG(isfinite(eps) && eps > 0.f, STROTSS_ERANGE);
  ST_CHECK_ARG(aligned16(img) && aligned16(gimg) && aligned16(workspace), STROTSS_EALIGN);
  const double n = 3.0 * (double)h * (double)w;
  const float coef = (float)((double)gscale / n), inv_n = (float)(1.0 / n);
  unsigned* ticket = (unsigned*)workspace;
  float* partials = (float*)((char*)workspace + 16);
  hipLaunchKernelGGL(tv_fwd_bwd_kernel, dim3((unsigned)prior_blocks(h, w)), dim3(256), 0, (hipStream_t)stream, img, h, w,
                     (int)cells(w, PRIOR_TILE_PX), eps, eps * eps, coef, inv_n, gimg, loss_out, ticket, partials);
  ST_LAUNCH_RET();
}
