// Joint bilateral upsampling of a label grid: the two kernels behind --refine_masks.  img is an
// (h, w, 3) float32 image, grid_label its (gh, gw) int32 label grid with gh <= h and gw <= w; cell (i, j) owns the pixels
// (y, x) with y gh / h == i and x gw / w == j (integer division: what upsample_labels maps to it).
//   means   refine_cell_mean_kernel    one wave per cell: lane l sums pixels l, l + 64, .. of the cell (row-major inside the
//                                      cell) in float64, the 64 partial sums meet in a fixed xor tree, the mean is divided in
//                                      float64 and rounded ONCE at the store -> (gh, gw, 3) float32 in the workspace.  Workgroup
//                                      0 also zeroes the k counts of the vote kernel (the next launch on the stream).
//   votes   refine_vote_kernel<KP>     a workgroup takes a 32 x 8 tile of pixels, one per thread, and stages the colours and
//                                      labels of the tile's footprint (its own cells plus `radius` on each side, clipped to
//                                      the grid: at most 16 x 40 cells, 10 KB, because gh <= h lets 8 pixel rows meet at most
//                                      8 cell rows) in LDS as (r, g, b, label) quads.  A lane walks its (2 radius + 1)^2
//                                      window row by row, forms one float64 exp per cell and adds it to the accumulator of
//                                      the cell's label: KP float64 accumulators with static indices (a select per label),
//                                      KP = 4, 8 or 16 >= k.  The image is read once, the label written once.  Counts: a wave
//                                      ballot per label, an integer LDS add per wave, one integer atomic add per label and
//                                      workgroup.
// No float atomics, every sum in an order fixed by the shapes alone: the same bits on every run and stream.  The vote kernel
// is bound by its (2 radius + 1)^2 float64 exponentials per pixel, not by its 16 bytes per pixel.
#include <math.h>

#include "internal.h"

namespace {

#define RF_THREADS 256
#define RF_TILE_W 32
#define RF_TILE_H (RF_THREADS / RF_TILE_W)                                  // 8
#define RF_MAX_RADIUS 4
#define RF_FOOT_H (RF_TILE_H + 2 * RF_MAX_RADIUS)                           // 16
#define RF_FOOT_W (RF_TILE_W + 2 * RF_MAX_RADIUS)                           // 40
#define RF_CELLS_PER_BLOCK (RF_THREADS / WAVE)                              // 4
#define RF_MAX_GRID 16384u               // workgroups of a launch at most; a workgroup walks the tiles (cells) beyond

typedef int i32x4 __attribute__((ext_vector_type(4)));

// first pixel row (column) of cell i: the smallest y with y g / n >= i
__device__ __forceinline__ int rf_cell_start(int i, int g, int n) { return (int)(((long long)i * n + g - 1) / g); }
// the cell of pixel row (column) y: y g / n < g for every y < n
__device__ __forceinline__ int rf_cell_of(int y, int g, int n) { return (int)(((long long)y * g) / n); }

__device__ __forceinline__ void refine_cell_mean(const float* __restrict__ img, int h, int w, int gh, int gw, size_t cell,
                                                 int lane, float* __restrict__ mean) {
  const int i = (int)(cell / gw), j = (int)(cell % gw);
  const int y0 = rf_cell_start(i, gh, h), y1 = rf_cell_start(i + 1, gh, h);
  const int x0 = rf_cell_start(j, gw, w), x1 = rf_cell_start(j + 1, gw, w);
  const int cw = x1 - x0;
  const size_t n = (size_t)(y1 - y0) * cw;                             // >= 1: gh <= h and gw <= w
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (size_t p = lane; p < n; p += 64) {
    const size_t at = ((size_t)(y0 + (int)(p / cw)) * w + (size_t)(x0 + (int)(p % cw))) * 3;
    s0 += (double)img[at];
    s1 += (double)img[at + 1];
    s2 += (double)img[at + 2];
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) {
    const double dn = (double)n;
    mean[cell * 3] = (float)(s0 / dn);
    mean[cell * 3 + 1] = (float)(s1 / dn);
    mean[cell * 3 + 2] = (float)(s2 / dn);
  }
}

__global__ __launch_bounds__(RF_THREADS) void refine_cell_mean_kernel(const float* __restrict__ img, int h, int w, int gh,
                                                                      int gw, float* __restrict__ mean, int* __restrict__ count,
                                                                      int k) {
  if (blockIdx.x == 0 && (int)threadIdx.x < k) count[threadIdx.x] = 0;
  const int lane = (int)threadIdx.x & 63;
  const size_t ncells = (size_t)gh * gw, stride = (size_t)gridDim.x * RF_CELLS_PER_BLOCK;
  for (size_t cell = (size_t)blockIdx.x * RF_CELLS_PER_BLOCK + (threadIdx.x >> 6); cell < ncells; cell += stride)
    refine_cell_mean(img, h, w, gh, gw, cell, lane, mean);              // wave-uniform: a whole wave takes a cell or leaves
}

template <int KP>
__global__ __launch_bounds__(RF_THREADS) void refine_vote_kernel(const float* __restrict__ img, int h, int w,
                                                                 const int* __restrict__ grid_label,
                                                                 const float* __restrict__ mean, int gh, int gw, int k,
                                                                 int radius, double inv2s, double inv2r, unsigned tiles_x,
                                                                 unsigned ntiles, int* __restrict__ label,
                                                                 double* __restrict__ best_out, double* __restrict__ second_out,
                                                                 int* __restrict__ count) {
  __shared__ __attribute__((aligned(16))) i32x4 cells[RF_FOOT_H * RF_FOOT_W];
  __shared__ int cnt[KP];
  const int t = (int)threadIdx.x, lane = t & 63;
  if (t < KP) cnt[t] = 0;
  for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int ty0 = (int)(tile / tiles_x) * RF_TILE_H, tx0 = (int)(tile % tiles_x) * RF_TILE_W;
    const int ty1 = min(h, ty0 + RF_TILE_H) - 1, tx1 = min(w, tx0 + RF_TILE_W) - 1;     // the tile's last pixel row, column
    const int i_lo = max(0, rf_cell_of(ty0, gh, h) - radius), i_hi = min(gh - 1, rf_cell_of(ty1, gh, h) + radius);
    const int j_lo = max(0, rf_cell_of(tx0, gw, w) - radius), j_hi = min(gw - 1, rf_cell_of(tx1, gw, w) + radius);
    const int fh = i_hi - i_lo + 1, fw = j_hi - j_lo + 1;              // <= RF_FOOT_H, RF_FOOT_W
    __syncthreads();                                                    // the tile before is read; cnt is zeroed
    for (int c = t; c < fh * fw; c += RF_THREADS) {
      const size_t g = (size_t)(i_lo + c / fw) * gw + (size_t)(j_lo + c % fw);
      i32x4 q;
      q[0] = __float_as_int(mean[g * 3]);
      q[1] = __float_as_int(mean[g * 3 + 1]);
      q[2] = __float_as_int(mean[g * 3 + 2]);
      q[3] = grid_label[g];
      cells[c] = q;
    }
    __syncthreads();

    const int y = ty0 + t / RF_TILE_W, x = tx0 + t % RF_TILE_W;
    const bool inside = y < h && x < w;
    int bl = 0;
    if (inside) {
      const size_t pix = (size_t)y * w + x;
      const double c0 = (double)img[pix * 3], c1 = (double)img[pix * 3 + 1], c2 = (double)img[pix * 3 + 2];
      const double u = ((double)y + 0.5) * (double)gh / (double)h - 0.5;
      const double v = ((double)x + 0.5) * (double)gw / (double)w - 0.5;
      const int i0 = rf_cell_of(y, gh, h), j0 = rf_cell_of(x, gw, w);
      const int wi0 = max(0, i0 - radius), wi1 = min(gh - 1, i0 + radius);             // inside the footprint: i0 lies
      const int wj0 = max(0, j0 - radius), wj1 = min(gw - 1, j0 + radius);             // between the tile's own cells
      double vote[KP];
#pragma unroll
      for (int l = 0; l < KP; ++l) vote[l] = 0.0;
      unsigned present = 0u;
      for (int i = wi0; i <= wi1; ++i) {
        const double du = u - (double)i;
        const int at = (i - i_lo) * fw - j_lo;
        for (int j = wj0; j <= wj1; ++j) {
          const i32x4 q = cells[at + j];
          const double dv = v - (double)j;
          const double e0 = c0 - (double)__int_as_float(q[0]), e1 = c1 - (double)__int_as_float(q[1]),
                       e2 = c2 - (double)__int_as_float(q[2]);
          const double wgt = exp(-((du * du + dv * dv) * inv2s + (e0 * e0 + e1 * e1 + e2 * e2) * inv2r));
          const int lab = q[3];
          if ((unsigned)lab < (unsigned)k) present |= 1u << lab;        // a foreign label: no vote, never an index
#pragma unroll
          for (int l = 0; l < KP; ++l) vote[l] += lab == l ? wgt : 0.0;  // + 0.0 is exact: per label the window's order
        }
      }
      double best = -INFINITY, second = -INFINITY;
#pragma unroll
      for (int l = 0; l < KP; ++l) {
        if (!((present >> l) & 1u)) continue;                           // a label absent from the window cannot win
        if (vote[l] > best) {                                           // strictly: the lowest label wins on equal votes
          second = best;
          best = vote[l];
          bl = l;
        } else if (vote[l] > second) {
          second = vote[l];
        }
      }
      label[pix] = bl;
      if (best_out) best_out[pix] = best;
      if (second_out) second_out[pix] = second;
    }
#pragma unroll
    for (int l = 0; l < KP; ++l) {
      const unsigned long long m = __ballot(inside && bl == l);
      if (lane == 0 && m) atomicAdd(&cnt[l], __popcll(m));              // integer, in LDS
    }
  }
  __syncthreads();
  if (t < k && cnt[t]) atomicAdd(&count[t], cnt[t]);                    // integer: one per label and workgroup
}

inline bool sizes_ok(int h, int w, int gh, int gw) {
  return h > 0 && w > 0 && gh > 0 && gw > 0 && gh <= h && gw <= w && 3LL * h * w <= 0x7fffffffLL;
}
inline bool k_ok(int k) { return k >= 1 && k <= STROTSS_KMEANS_MAX_K; }
inline bool sigma_ok(double s) { return isfinite(s) && s > 0.0; }

}  // namespace

size_t strotss_refine_labels_workspace_bytes(int h, int w, int gh, int gw) {
  if (!sizes_ok(h, w, gh, gw)) return 0;
  return ws_slice((size_t)gh * (size_t)gw * 3, sizeof(float));
}

int strotss_refine_labels(const float* img, int h, int w, const int* grid_label, int gh, int gw, int k, int radius,
                          double sigma_s, double sigma_r, int* label, double* best, double* second, int* count,
                          void* workspace, size_t workspace_bytes, void* stream) {
  ST_CHECK_ARG(img && grid_label && label && count && workspace && sizes_ok(h, w, gh, gw) && k_ok(k), STROTSS_EINVAL);
  ST_CHECK_ARG(radius >= 1 && radius <= STROTSS_REFINE_MAX_RADIUS && sigma_ok(sigma_s) && sigma_ok(sigma_r), STROTSS_EINVAL);
  ST_CHECK_ARG(workspace_bytes >= strotss_refine_labels_workspace_bytes(h, w, gh, gw), STROTSS_EINVAL);
  ST_CHECK_ARG(aligned16(img) && aligned16(grid_label) && aligned16(label) && aligned16(count) && aligned16(workspace) &&
                   aligned16(best) && aligned16(second),
               STROTSS_EALIGN);
  static_assert(STROTSS_REFINE_MAX_RADIUS == RF_MAX_RADIUS, "the LDS footprint is sized for this radius");
  const double inv2s = 1.0 / (2.0 * sigma_s * sigma_s), inv2r = 1.0 / (2.0 * sigma_r * sigma_r);
  ST_CHECK_ARG(isfinite(inv2s) && isfinite(inv2r) && inv2s > 0.0 && inv2r > 0.0, STROTSS_EINVAL);
  hipStream_t st = (hipStream_t)stream;
  float* mean = (float*)workspace;
  // tile and cell counts are below 2^31 for every 3 h w <= INT_MAX (gh gw <= h w); the grids are capped so that a narrow,
  // very tall image stays below the 2^32 threads of a launch
  const size_t mean_blocks = ((size_t)gh * gw + RF_CELLS_PER_BLOCK - 1) / RF_CELLS_PER_BLOCK;
  const unsigned tiles_x = ((unsigned)w + RF_TILE_W - 1) / RF_TILE_W, tiles_y = ((unsigned)h + RF_TILE_H - 1) / RF_TILE_H;
  const unsigned ntiles = tiles_x * tiles_y;
  const dim3 block(RF_THREADS), grid(min(ntiles, RF_MAX_GRID));
  hipLaunchKernelGGL(refine_cell_mean_kernel, dim3((unsigned)min(mean_blocks, (size_t)RF_MAX_GRID)), block, 0, st, img, h, w,
                     gh, gw, mean, count, k);
#define RF_LAUNCH(KP)                                                                                                        \
  hipLaunchKernelGGL(refine_vote_kernel<KP>, grid, block, 0, st, img, h, w, grid_label, mean, gh, gw, k, radius, inv2s, inv2r, \
                     tiles_x, ntiles, label, best, second, count)
  if (k <= 4)
    RF_LAUNCH(4);
  else if (k <= 8)
    RF_LAUNCH(8);
  else
    RF_LAUNCH(16);
#undef RF_LAUNCH
  ST_LAUNCH_RET();
}
