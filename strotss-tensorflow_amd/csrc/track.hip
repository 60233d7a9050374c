// Region tracking through frame sequences: the two kernels behind --auto_masks K --video --track_masks.
//   prior    label_warp_kernel             one thread per cell of the (gh, gw) label grid: the cell's probe pixel (the integer
//                                          mean of its first and last owned row and column) is followed along the backward
//                                          flow to the nearest pixel of the earlier frame, and the label of THAT pixel's cell
//                                          in the earlier grid is the prior; -1 where the flow is not finite, the source pixel
//                                          lies outside the image, the certainty at the probe is below 0.5 or the label found
//                                          lies outside 0..k-1.  Integer output, no reduction: 16 bytes read per cell.
//   assign   kmeans_assign_kernel<KP, true> (kmeans_assign.h, shared with kmeans.hip: the same s_ij bits)  label = first
//                                          arg-max of s_ij + (prior_i == j ? beta : 0); best, second on the raw s.
// No atomics at all: the same bits on every run and stream.
#include <math.h>

#include "kmeans_assign.h"

namespace {

#define TR_THREADS 256

// first pixel row (column) of cell i: the smallest y with y g / n >= i (the convention of strotss_refine_labels)
__device__ __forceinline__ int tr_cell_start(int i, int g, int n) { return (int)(((long long)i * n + g - 1) / g); }
// the cell of pixel row (column) y: y g / n < g for every y < n
__device__ __forceinline__ int tr_cell_of(int y, int g, int n) { return (int)(((long long)y * g) / n); }

__global__ __launch_bounds__(TR_THREADS) void label_warp_kernel(const int* __restrict__ prev_grid, int gh, int gw, int k,
                                                                const float* __restrict__ flow,
                                                                const float* __restrict__ certainty, int h, int w,
                                                                int* __restrict__ prior) {
  const size_t cell = (size_t)blockIdx.x * TR_THREADS + threadIdx.x;
  if (cell >= (size_t)gh * gw) return;
  const int i = (int)(cell / gw), j = (int)(cell % gw);
  const int yc = (tr_cell_start(i, gh, h) + tr_cell_start(i + 1, gh, h) - 1) / 2;      // inside [0, h): gh <= h
  const int xc = (tr_cell_start(j, gw, w) + tr_cell_start(j + 1, gw, w) - 1) / 2;
  const size_t pix = (size_t)yc * w + xc;
  const float dx = flow[pix * 2], dy = flow[pix * 2 + 1];
  int out = -1;
  if (isfinite(dx) && isfinite(dy) && !(certainty && certainty[pix] < 0.5f)) {
    const float sy = floorf(((float)yc + dy) + 0.5f), sx = floorf(((float)xc + dx) + 0.5f);
    if (sy >= 0.f && sy < (float)h && sx >= 0.f && sx < (float)w) {   // compared as floats: no cast of a huge value
      const int lab = prev_grid[(size_t)tr_cell_of((int)sy, gh, h) * gw + tr_cell_of((int)sx, gw, w)];
      if ((unsigned)lab < (unsigned)k) out = lab;                       // compared, never used as an index
    }
  }
  prior[cell] = out;
}

inline bool sizes_ok(int h, int w, int gh, int gw) {
  return h > 0 && w > 0 && gh > 0 && gw > 0 && gh <= h && gw <= w && 3LL * h * w <= 0x7fffffffLL;
}

}  // namespace

int strotss_label_warp(const int* prev_grid, int gh, int gw, int k, const float* flow, const float* certainty, int h, int w,
                       int* prior, void* stream) {
  ST_CHECK_ARG(prev_grid && flow && prior && sizes_ok(h, w, gh, gw) && km_k_ok(k), STROTSS_EINVAL);
  ST_CHECK_ARG(aligned16(prev_grid) && aligned16(flow) && aligned16(certainty) && aligned16(prior), STROTSS_EALIGN);
  const size_t cells = (size_t)gh * gw;                                 // <= h w < 2^31: the blocks fit a launch
  hipLaunchKernelGGL(label_warp_kernel, dim3((unsigned)((cells + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0,
                     (hipStream_t)stream, prev_grid, gh, gw, k, flow, certainty, h, w, prior);
  ST_LAUNCH_RET();
}

int strotss_kmeans_assign_prior(const float* x, const float* inv_norm, int n, int d, int ld, const float* centres, int k,
                                const int* prior, float beta, int* label, float* best, float* second, void* stream) {
  ST_CHECK_ARG(x && inv_norm && centres && prior && label && best && second && km_rows_ok(n, d, ld) && km_k_ok(k),
               STROTSS_EINVAL);
  ST_CHECK_ARG(isfinite(beta) && beta >= 0.f && beta <= 2.f, STROTSS_EINVAL);
  ST_CHECK_ARG(ld % 32 == 0, STROTSS_EALIGN);
  ST_CHECK_ARG(aligned16(x) && aligned16(inv_norm) && aligned16(centres) && aligned16(prior) &&
                   aligned16(label) && aligned16(best) && aligned16(second),
               STROTSS_EALIGN);
  km_launch_assign<true>(x, inv_norm, n, d, ld, centres, k, prior, beta, label, best, second, (hipStream_t)stream);
  ST_LAUNCH_RET();
}
