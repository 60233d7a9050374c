/*
 * strotss_hip.h -- C ABI of libstrotss_hip.so: the MI355X (gfx950) kernels behind the
 * STROTSS optimisation inner loop of interaction-lab-uh/STROTSS-tensorflow.
 *
 * The reference has NO native boundary: its hot path is a chain of TensorFlow op calls made
 * from Python (run_strotss.py:131-148).  Each entry point below replaces the TF op(s) at the
 * cited reference call site; the Python package strotss-tensorflow_amd/nn (same module and
 * function names as the reference's nn/) binds them with ctypes (nn/_hip.py).
 *
 * Conventions (all entry points):
 *   - every pointer is a CALLER-OWNED DEVICE pointer (float32 unless stated), never freed or
 *     allocated by the library; workspaces are passed in explicitly;
 *   - `stream` is the hipStream_t the work is enqueued on (as a void*); no call synchronises;
 *   - return 0 on success, a negative STROTSS_E* for a bad argument (nothing is launched), or a
 *     positive hipError_t from the launch;
 *   - images / feature maps are NHWC with batch 1: (H, W, C) row-major, C contiguous;
 *   - sampled feature matrices are (rows, ld) row-major with ld >= D, ld % 32 == 0, columns
 *     [D, ld) and rows [n, rows) ZERO (the library keeps them zero); rows % 32 == 0;
 *   - n-by-n cost matrices are (rows, ldc) row-major, ldc % 4 == 0.
 */
#ifndef STROTSS_HIP_H
#define STROTSS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STROTSS_OK 0
#define STROTSS_EINVAL (-1)   /* bad size / null pointer */
#define STROTSS_EALIGN (-2)   /* leading dimension or K not a multiple of what the kernel needs */
#define STROTSS_ERANGE (-3)   /* too many maps / tensors for the fixed-size descriptor */

#define STROTSS_MAX_MAPS 12
#define STROTSS_MAX_DIVS 8
#define STROTSS_MAX_TENSORS 8

/* library identity; also used by the loader to check the build. */
int strotss_abi_version(void);
const char* strotss_build_info(void);

/* ---------------------------------------------------------------------------------------
 * Images: tf.image.resize(bilinear, half-pixel centres, no antialias)
 *   replaces nn/utils.py:37,41 and nn/strotss_utils.py:142-143,162 (tf.image.resize)
 * --------------------------------------------------------------------------------------- */
/* out(oh,ow,c) = alpha*resize(in(ih,iw,c)) + (add ? add(oh,ow,c) : 0) ; alpha is +1 or -1 in
 * practice: fold uses (add = residual, alpha = 1); make_laplacian uses (add = x, alpha = -1). */
int strotss_resize_bilinear(const float* in, int ih, int iw, int c, float* out, int oh, int ow,
                            float alpha, const float* add, void* stream);
/* fold_laplacian_pyramid (strotss_utils.py:159-163) of a 3-channel pyramid in ONE launch:
 *   img = var[0] + up(var[1] + up(var[2] + ... up(var[n-1]))),   up = TF2 bilinear resize to the next finer level's size.
 * Level k is (h[k], w[k], 3); every level at most as large as the one above it, halving or faster from level 1 on
 * (what make_laplacian_pyramid builds); STROTSS_ERANGE otherwise (use strotss_resize_bilinear level by level).
 * Same taps and arithmetic as n-1 calls of strotss_resize_bilinear(..., alpha = 1, add = var[k]). */
#define STROTSS_MAX_LEVELS 8
typedef struct {
  int n_levels;
  int h[STROTSS_MAX_LEVELS], w[STROTSS_MAX_LEVELS];
  const float* var[STROTSS_MAX_LEVELS];
} strotss_pyramid_t;
int strotss_fold_pyramid(const strotss_pyramid_t* pyr, float* img, void* stream);
/* adjoint of the above w.r.t. `in`: gin(ih,iw,c) = resize^T(gout(oh,ow,c)).  Deterministic
 * gather form (no atomics).  Replaces the TF gradient of strotss_utils.py:162. */
int strotss_resize_bilinear_adjoint(const float* gout, int oh, int ow, int c, float* gin, int ih,
                                    int iw, void* stream);
/* The adjoint of the whole fold (3 channels): var[0] = the gradient of the folded image (input), var[k] for k >= 1 receive
 * var[k] = resize^T(var[k-1]) -- the gradients of the pyramid levels (written through the const pointers of the
 * descriptor).  Two levels per launch where each level halves the one above it to within a pixel (a workgroup recomputes
 * the few middle-level rows its tile reads), strotss_resize_bilinear_adjoint level by level otherwise; bit for bit the
 * same values either way. */
int strotss_fold_pyramid_adjoint(const strotss_pyramid_t* gpyr, void* stream);

/* ---------------------------------------------------------------------------------------
 * VGG16 trunk (frozen): nn/model.py:44-55 -- Keras Conv2D(3x3,'same',relu) / MaxPooling2D(2,2)
 * --------------------------------------------------------------------------------------- */
/* First layer with the ImageNet preprocess fused (model.py:50-51):
 *   out(h,w,cout) = relu(conv3x3((img-mean)/std zero-padded, w_kio) + bias), img(h,w,3) in [0,1].
 *   w_kio: (27, cout) = HWIO kernel flattened, k = (dy*3+dx)*3+ci.
 *   mean3/std3 are the ONLY host pointers of this ABI: 3 floats each, the constants of
 *   model.py:34-35, read at call time and passed to the kernel by value.
 *   relu_bits_out (may be NULL): also writes the sign words of `out`, see strotss_relu_bits. */
int strotss_conv3x3_c3_fwd(const float* img, int h, int w, const float* w_kio, const float* bias,
                           int cout, const float* mean3, const float* std3, float* out,
                           unsigned int* relu_bits_out, void* stream);
/* Sign words of a conv layer's output on the F(4x4,3x3) tile grid: what the data-gradient of the NEXT layer needs of it
 * (the ReLU mask, model.py:44-48 differentiated) in 4 bytes per (4 x 4 tile, channel) instead of 64:
 *   relu_bits[(ty * TW + tx) * c + ch], TW = (w + 3) / 4, byte r (0..3), bit q (0..3) = act[4 ty + r][4 tx + q][ch] > 0
 * (pixels outside the image: unspecified).  strotss_relu_bits_bytes(h, w, c) bytes.  The forward entry points write
 * them from registers (relu_bits_out); strotss_relu_bits derives them from a finished activation tensor (h, w, c). */
size_t strotss_relu_bits_bytes(int h, int w, int c);
int strotss_relu_bits(const float* act, int h, int w, int c, unsigned int* relu_bits, void* stream);
/* Generic layer, cin % 32 == 0, cout % 64 == 0:
 *   out(h,w,cout) = relu(conv3x3(in(h,w,cin)) + bias);  w_tok: (9, cout, cin), tap = dy*3+dx. */
/* workspace (may be NULL; strotss_conv3x3_workspace_bytes(h, w, cin, cout) bytes, 0 for big maps): with it, layers of at
 * most 128 output tiles of 64 x 64 (the small maps of the 64 ... 256 px scales) split K over up to 256 workgroups
 * and a finish kernel adds the partial tiles in a fixed order (same result class, bitwise reproducible).
 * (Round 3 measured the finish INSIDE the split-K kernel -- last workgroup to arrive at a tile, agent-scope release /
 * ticket / acquire: 1.32 ms per 64-px step against 0.835 ms with the finish launch; 256 workgroups each writing back
 * their XCD's L2 cost far more than the 24 kernel boundaries they replace.  Not kept.) */
size_t strotss_conv3x3_workspace_bytes(int h, int w, int cin, int cout);
int strotss_conv3x3_relu_fwd(const float* in, int h, int w, int cin, const float* w_tok,
                             const float* bias, int cout, float* out, void* workspace, size_t workspace_bytes,
                             void* stream);
/* Data gradient of the generic layer (no weight gradient: the net is frozen, model.py:45):
 *   gin(h,w,cin) = conv3x3^T(gout(h,w,cout)) [* (act_in > 0) if act_in != NULL]
 *   gout must already carry the ReLU mask of ITS layer.  w_tik: (9, cin, cout) spatially
 *   flipped kernel, tap' = (2-dy)*3+(2-dx).  act_in = the layer's (post-ReLU) input or NULL
 *   when the input came from a max-pool. */
/* accumulate != 0: gin += the (masked) data gradient instead of being overwritten -- the buffer then already holds the
 * hypercolumn taps' contributions of this layer (scattered in one launch for all maps before the backward pass). */
/* Block ends at the split-K scales (ABI 8): the finish kernel of a split-K layer also does the 2x2/2 max-pool that follows it
 * (forward: out AND pool_out = strotss_maxpool2_fwd(out) with its argmax codes pool_code, may be NULL) or precedes it
 * (data-gradient of a layer whose input came from the pool: gin_full(full_h, full_w, cin) (+)= strotss_maxpool2_bwd's result
 * from the codes, full_h / 2 == h, full_w / 2 == w; the pooled gradient itself is never stored) -- one launch less per block
 * and direction, bit for bit the two-launch results.  Split-K layers only (strotss_conv3x3_workspace_bytes(...) > 0 and that
 * workspace given): STROTSS_EINVAL otherwise. */
int strotss_conv3x3_relu_pool_fwd(const float* in, int h, int w, int cin, const float* w_tok, const float* bias, int cout,
                                  float* out, float* pool_out, unsigned char* pool_code, void* workspace,
                                  size_t workspace_bytes, void* stream);
int strotss_conv3x3_dgrad_unpool(const float* gout, int h, int w, int cout, const float* w_tik, int cin,
                                 const unsigned char* pool_code, float* gin_full, int full_h, int full_w, int accumulate,
                                 void* workspace, size_t workspace_bytes, void* stream);
int strotss_conv3x3_dgrad(const float* gout, int h, int w, int cout, const float* w_tik, int cin,
                          const float* act_in, float* gin, int accumulate, void* workspace, size_t workspace_bytes,
                          void* stream);
/* 1 when strotss_conv3x3_dgrad(..., accumulate = 1, ...) launches for this shape (given its
 * strotss_conv3x3_workspace_bytes(h, w, cout, cin) workspace), 0 where it answers STROTSS_EINVAL or _EALIGN: the one-pass
 * kernel of STROTSS_CONV_VARIANT=1 overwrites, the split-K form adds under every variant.  Host arithmetic, no launch. */
int strotss_conv3x3_dgrad_can_accumulate(int h, int w, int cout, int cin);
/* Data gradient of the first layer down to the pixels, preprocess adjoint fused:
 *   gimg(h,w,3) (+)= conv3x3^T(gout(h,w,cout)) / std.   w_tic: (9, 3, cout) flipped kernel.
 *   accumulate != 0 adds to gimg (the hypercolumn scatter of map 0 lands there first).
 *   std3: HOST pointer, 3 floats. */
int strotss_conv3x3_c3_dgrad(const float* gout, int h, int w, int cout, const float* w_tic,
                             const float* std3, float* gimg, int accumulate, void* stream);
/* Winograd form of the two generic-layer entry points above (same results up to fp32 rounding of the
 * transforms).  tile_m = 2: F(2x2,3x3), P = 16 transform-domain GEMMs, 2.25x fewer MACs than direct;
 * tile_m = 4: F(4x4,3x3), P = 36 GEMMs, 4x fewer MACs (f32 error ~1e-5 of the output range instead of ~5e-7).
 * u_pok: (P, cout, cin) = (G g G^T)[p] of the forward kernel, u_pik: (P, cin, cout) of the spatially flipped
 * kernel; both pre-computed once from the frozen weights.
 * workspace >= strotss_conv3x3_winograd_workspace_bytes(h, w, cin, cout, tile_m).
 * u_packed (tile_m = 4 only, may be NULL): the same weights in the MFMA-fragment order written by
 * strotss_conv3x3_winograd_pack (same number of floats).  With it, layers the three-kernel form would run bound
 * by its transform traffic (few output channels, many tiles) run as ONE persistent kernel that keeps the
 * transforms and the 36 GEMMs on chip (csrc/winograd_fused.hip); the workspace is then not touched.
 * u_x3 (tile_m = 4 only, may be NULL): the same weights as "x3 panels" written by strotss_conv3x3_winograd_x3pack
 * (strotss_conv3x3_winograd_x3_bytes bytes).  With it, the 36 GEMMs of the three-kernel form run on the bf16 MFMA by
 * EXACT 3-way operand splitting (every f32 value = h + m + l in bf16, six exact partial products, f32 accumulation:
 * f32-class results at 6/16 of the f32-MFMA cost, csrc/mfma_x3.h).  Default on (STROTSS_X3_CONV=0 switches it off).
 * (Round 2's two bf16x3 forms of the FUSED kernel, both measured slower than its f32-MFMA form, left the library and
 * this ABI in round 3: tools/experiments/winograd_fused_x3.hip.) */
size_t strotss_conv3x3_winograd_workspace_bytes(int h, int w, int cin, int cout, int tile_m);
/* The Winograd weight transform itself: g_nk33 (n, k, 3, 3) = kernel as [out-row][in-col][r][q] -> u_pnk (P, n, k) with
 * u_pnk[a * (tile_m + 2) + b] = (G g G^T)[a][b], P = (tile_m + 2)^2, computed in float64 and rounded once. */
int strotss_conv3x3_winograd_weights(const float* g_nk33, int n, int k, int tile_m, float* u_pnk, void* stream);
/* u_prk: (36, rows, k) -> x3 panels: per position p, element (r, c) split into bf16 planes h, m, l at
 * ((p * (k/32) + c/32) * 3 + plane) * rows * 32 + r * 32 + c % 32   (bf16 units).  k % 32 == 0. */
size_t strotss_conv3x3_winograd_x3_bytes(int rows, int k);
int strotss_conv3x3_winograd_x3pack(const float* u_prk, int rows, int k, void* u_x3, void* stream);
/* u_prk: (36, rows, k) -> u_packed[p][rows/32][k/8][2][32][4]: element (p, r, c) at
 * ((((p * (rows/32) + r/32) * (k/8) + c/8) * 2 + (c%8)/4) * 32 + r%32) * 4 + c%4.  rows % 32 == 0, k % 8 == 0. */
int strotss_conv3x3_winograd_pack(const float* u_prk, int rows, int k, float* u_packed, void* stream);
/* relu_bits_out (fwd, may be NULL, tile_m == 4 only): also writes the sign words of `out` (strotss_relu_bits).
 * relu_bits (dgrad, may be NULL, tile_m == 4 only): the sign words of the layer's INPUT activation; when given, the ReLU
 * mask comes from them and act_in is not read (same result bit for bit: 4 bytes per tile and channel instead of 64).
 * pool_out (may be NULL): also writes strotss_maxpool2_fwd(out) = the (h/2, w/2, cout) input of the next block --
 * from the registers of the fused kernel's epilogue where that kernel runs, by a pooling launch otherwise;
 * pool_code (may be NULL, needs pool_out): the argmax codes of that pooling, see strotss_maxpool2_fwd.
 * accumulate (dgrad, tile_m == 4 with act_in or relu_bits): gin += the masked data-gradient instead of gin = (round 4, ABI 7:
 * the taps of a tapped layer may be scattered into a zeroed gin before the backward pass -- one scatter launch per step --
 * when every producer of such a gradient adds, like strotss_conv3x3_dgrad and strotss_maxpool2_bwd). */
int strotss_conv3x3_winograd_fwd(const float* in, int h, int w, int cin, const float* u_pok,
                                 const float* u_packed, const void* u_x3, const float* bias,
                                 int cout, int tile_m, float* out,
                                 float* pool_out, unsigned char* pool_code, unsigned int* relu_bits_out,
                                 void* workspace, size_t workspace_bytes, void* stream);
int strotss_conv3x3_winograd_dgrad(const float* gout, int h, int w, int cout, const float* u_pik,
                                   const float* u_packed, const void* u_x3, int cin, int tile_m,
                                   const float* act_in, const unsigned int* relu_bits, float* gin, int accumulate,
                                   void* workspace, size_t workspace_bytes, void* stream);
/* Which kernels strotss_conv3x3_winograd_fwd / _dgrad run for a layer shape (the routing is a size policy with
 * environment switches, read once per process): the very function those two entries dispatch on (csrc/winograd.hip
 * winograd43_route), so the answer cannot differ from what launches.  has_packed / has_x3: whether the caller passes
 * u_packed / u_x3 for this layer; a caller that wants to know whether making the x3 panels is worth it asks with
 * has_x3 = 1 and makes them where the answer is one of the two X3 routes.  Host arithmetic, no GPU needed. */
#define STROTSS_ROUTE_F2_GEMM_F32 0     /* F(2x2,3x3): input transform, 16 f32-MFMA GEMMs, output transform            */
#define STROTSS_ROUTE_F4_FUSED_F32 1    /* F(4x4,3x3), one persistent kernel, f32 MFMA (csrc/winograd_fused.hip)       */
#define STROTSS_ROUTE_F4_GEMM_F32 2     /* F(4x4,3x3), three kernels, 36 f32-MFMA GEMMs                                 */
#define STROTSS_ROUTE_F4_X3_GEMM_128 3  /* three kernels, 36 bf16x3 GEMMs, 128 x 128 tiles (K16 ring, two workgroups/CU)*/
#define STROTSS_ROUTE_F4_X3_GEMM_64 4   /* the same on 64 x 64 tiles                                                    */
int strotss_conv3x3_winograd_route(int h, int w, int cin, int cout, int tile_m, int has_packed, int has_x3);
/* MEASUREMENT HOOK, process-wide and not thread-safe: which stages of the F(4x4,3x3) three-kernel form are launched
 * from now on (bit 0 input transform, bit 1 GEMMs, bit 2 output transform; 7 = all, the default); returns the previous
 * mask.  bench.py times a layer with masks 1, 3, 7 to split its time into transform and GEMM time (results are
 * meaningless under a partial mask). */
int strotss_debug_winograd_stages(int mask);
/* 2x2/2 VALID max-pool: out(h/2, w/2, c).  code (may be NULL): (h/2, w/2, c) bytes, the index 0..3 of the FIRST
 * max of each window in scan order (0,0),(0,1),(1,0),(1,1), or 4 when that max is not positive. */
int strotss_maxpool2_fwd(const float* in, int h, int w, int c, float* out, unsigned char* code, void* stream);
/* gin(h,w,c) = route gout(h/2,w/2,c) to the first max of each window, times (act > 0) where
 * act(h,w,c) is the pooled layer's input (post-ReLU).  Overwrites gin.  With code != NULL (from the forward pass)
 * act is not read (may be NULL): 1 byte instead of 16 per pooled element.  accumulate != 0: gin += instead of gin =. */
int strotss_maxpool2_bwd(const float* act, int h, int w, int c, const float* gout, float* gin,
                         const unsigned char* code, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------
 * Sampling._sample: hypercolumn gather  (nn/strotss_utils.py:25-81) and its adjoint
 * --------------------------------------------------------------------------------------- */
typedef struct {
  int n_maps;
  int h[STROTSS_MAX_MAPS], w[STROTSS_MAX_MAPS], c[STROTSS_MAX_MAPS];
  int n_div[STROTSS_MAX_MAPS];                    /* how many entries of div[] apply to map k */
  float div[STROTSS_MAX_DIVS];                    /* cumulative `indices /= y` chain (float32) */
  const float* map[STROTSS_MAX_MAPS];             /* gather: sources; scatter: activations   */
  float* gmap[STROTSS_MAX_MAPS];                  /* scatter only: gradient buffers           */
  /* Row window (spatially sharded trunk): when rows[k] > 0 the buffers of map k hold only rows
   * [row0[k], row0[k] + rows[k]) of a map whose full height is h[k]; coordinates and clipping stay those of
   * the full map (strotss_utils.py:43-64), the taps are then shifted into the window.  rows[k] == 0: whole map. */
  int row0[STROTSS_MAX_MAPS], rows[STROTSS_MAX_MAPS];
  /* scatter (and its plan) only, windowed maps only: != 0 DROPS a tap whose row lies outside the window instead of
   * clamping it to the window's edge -- halo-exchange strips: every rank scatters ALL samples and keeps what lands in
   * the rows it holds.  The gather always clamps (a rank gathers its own samples, whose taps lie inside). */
  int window_drop;
  /* gather, scatter and plan: NULL, or a DEVICE pointer to two ints {begin, end}: only the samples begin <= s < end of
   * the n given are processed (the launch still spans all n; the gather leaves the other rows of `out` untouched).  The
   * block of samples a rank owns changes every step (parallel.sort_indices_by_strip); read from device memory it can
   * change between replays of a captured graph. */
  const int* sample_range;
} strotss_maps_t;
/* out(rows, ld): row s < n = concat_k sample(map_k, idx[s]); bilinear != 0 -> 4-tap weights of
 * strotss_utils.py:43-70, else truncating nearest (72-75).  idx: (n,2) float32 (row, col). */
int strotss_hypercol_gather(const strotss_maps_t* maps, const float* idx, int n, int bilinear,
                            float* out, int ld, void* stream);
/* strotss_hypercol_gather(maps_a, ..., out_a) and strotss_hypercol_gather(maps_b, ..., out_b) at the same n positions in ONE
 * launch (the content and the prediction features of a train step, run_strotss.py:131-137), and, with zero != NULL, a zero
 * fill of the zero_rows x ld matrix `zero` (the step's gradient rows).  maps_b may carry a sample_range. */
int strotss_hypercol_gather2(const strotss_maps_t* maps_a, const strotss_maps_t* maps_b, const float* idx, int n,
                             int bilinear, float* out_a, float* out_b, int ld, float* zero, int zero_rows,
                             void* stream);
/* strotss_hypercol_gather2 + the content weights of the same n samples in the SAME launch: maps_w holds ONE map of ONE channel
 * (the scale's (h, w) content-weight map, no divisors, no row window), weight_out[s] = strotss_hypercol_gather(maps_w, idx)[s]
 * bit for bit for s < n, weight_out[s] = 0 for n <= s < weight_rows (weight_rows >= n). */
int strotss_hypercol_gather2_cw(const strotss_maps_t* maps_a, const strotss_maps_t* maps_b, const strotss_maps_t* maps_w,
                                const float* idx, int n, int bilinear, float* out_a, float* out_b, int ld, float* zero,
                                int zero_rows, float* weight_out, int weight_rows, void* stream);
/* Adjoint (bilinear only): gmap_k[pixel, c] += w * gfeat[s, off_k + c] * (relu_mask ? map_k>0 : 1)
 * for the maps k in [map_begin, map_end) only (the backward pass of the trunk needs the taps'
 * contributions one layer at a time); gmap[k] may be NULL outside that range.
 * relu_mask_from: maps with index >= relu_mask_from are post-ReLU activations (mask applied).
 * Float atomics, except for maps of at most 64 pixels (the 4 x 4 / 8 x 8 maps of the 64 / 128-px scales, where hundreds of
 * samples share an address): there one workgroup owns a (pixel, channel chunk) and adds its samples in sample order --
 * no atomics, the same bits on every run for those maps (STROTSS_SCATTER_DENSE=0: atomics everywhere). */
int strotss_hypercol_scatter(const strotss_maps_t* maps, const float* idx, int n,
                             const float* gfeat, int ld, int relu_mask_from, int map_begin,
                             int map_end, void* stream);

/* Deterministic form of the same adjoint (no float atomics; bitwise reproducible): strotss_hypercol_scatter_plan orders
 * the (sample, tap) entries of EVERY map by destination pixel once per index set (n <= 1024) into `plan`
 * (strotss_hypercol_scatter_plan_bytes(n_maps) bytes); strotss_hypercol_scatter_sorted then adds, per destination pixel
 * of the maps [map_begin, map_end), the entries' contributions in plan order with one plain read-modify-write. */
size_t strotss_hypercol_scatter_plan_bytes(int n_maps);
int strotss_hypercol_scatter_plan(const strotss_maps_t* maps, const float* idx, int n, void* plan, size_t plan_bytes,
                                  void* stream);
int strotss_hypercol_scatter_sorted(const strotss_maps_t* maps, const void* plan, int n, const float* gfeat, int ld,
                                    int relu_mask_from, int map_begin, int map_end, void* stream);

/* ---------------------------------------------------------------------------------------
 * Box calibration (bench.py only; nothing on the product path calls these).  strotss_calib_mfma: `blocks` workgroups of
 * four waves, each wave 16 * iters register-only v_mfma_f32_32x32x2_f32 (bf16 == 0: 4096 FLOP each) or
 * v_mfma_f32_32x32x16_bf16 (bf16 != 0: 32768 FLOP each); sink: blocks * 256 floats; clocks: per workgroup
 * {s_memtime ticks, s_memrealtime ticks (100 MHz)} of the loop -> the clock the device held.  bf16 == 2: the LOADED loop that
 * tells boxes apart -- 512-thread workgroups, 4 * iters bf16 MFMAs per wave whose operands are re-read from pseudo-random LDS
 * data every trip (sink: blocks * 512 floats).  strotss_calib_copy: a plain
 * 16-byte-per-lane streaming copy of `bytes` (a multiple of 16).
 * --------------------------------------------------------------------------------------- */
int strotss_calib_mfma(int bf16, int blocks, int iters, float* sink, unsigned long long* clocks, void* stream);
int strotss_calib_copy(const void* src, void* dst, size_t bytes, void* stream);
/* dependent-load latency: workgroup b starts at element b * start_stride of `next` (a random cycle over n elements, element i
 * at next[16 * i]: 64-byte stride) and follows `steps` links with one lane; clocks[2b], clocks[2b + 1] = s_memtime /
 * s_memrealtime ticks of its chase */
int strotss_calib_chase(const unsigned* next, unsigned start_stride, int blocks, int steps, unsigned* sink,
                        unsigned long long* clocks, void* stream);

/* ---------------------------------------------------------------------------------------
 * Sample coordinates drawn on the device  (Sampling._make_indices, nn/strotss_utils.py:83-121; the reference draws
 * them inside the traced train_step, run_strotss.py:136 / 115).  Region r (one workgroup each) reads its draw number
 * t = counter[r], draws the grid offsets (k = 0 rows, 1 columns:  philox4x32-10(ctr = (0, 1, t, 0), key = seed)[k] mod
 * step), lists the candidates (off_x + a*step_x, off_y + b*step_y) in tf.meshgrid('xy') order (a fastest), keeps those
 * whose mask byte is nonzero (mask[r] == NULL: all), gives position j of the kept list the shuffle key
 * philox(ctr = (j >> 2, 0, t, 0))[j & 3], writes the min(sample_size, kept) positions with the smallest (key, j) in
 * ascending order as float32 (row, col) pairs to idx[r] (rows beyond that count: zeros) and the count to n_out[r], and
 * stores counter[r] = t + counter_stride.  nn/rand.py:PhiloxStream is the host twin (same numbers through a
 * NumPy-Generator interface), so the oracle's make_indices reproduces every draw.  sample_size <= 1024; the grid has at
 * most 32768 candidates for any image (strotss_index_draw_max_candidates: STROTSS_ERANGE beyond that).
 * --------------------------------------------------------------------------------------- */
#define STROTSS_DRAW_MAX_REGIONS 16
typedef struct strotss_draw_t {
  int h, w;                       /* the scale's image size                                        */
  int step_x, step_y;             /* strotss_utils.py:89-90: max(1, floor / ceil(sqrt(h*w // 128^2))) */
  int sample_size;
  int n_regions;
  unsigned seed_lo, seed_hi;      /* Philox key                                                    */
  unsigned counter_stride;        /* one stream whose draws interleave over the regions: n_regions */
  const unsigned char* mask[STROTSS_DRAW_MAX_REGIONS];   /* (h, w) bytes at THIS scale, or NULL    */
  float* idx[STROTSS_DRAW_MAX_REGIONS];                  /* (sample_size, 2) float32               */
  unsigned* counter;              /* n_regions draw numbers in device memory                       */
  int* n_out;                     /* n_regions counts, or NULL                                     */
  int debug_flags;                /* bit 0: take the kernel's general selection path (tests)       */
} strotss_draw_t;
int strotss_index_draw_max_candidates(int h, int w, int step_x, int step_y);
int strotss_index_draw(const strotss_draw_t* d, void* stream);

/* The same draw with IMPORTANCE LEVELS (--sample_map): region r may carry level[r], (h, w) uint16
 * values at this scale.  Everything up to and including the shuffle keys is strotss_index_draw's statement, unchanged.
 * Position j of the filtered list also draws the acceptance word a_j = philox(ctr = (j >> 2, 3, t, 0), key = seed)[j & 3]
 * (c1 = 3 is used by nothing else: 0 and 1 belong to the index draw, 2 to the sliced transport), and its candidate at
 * (x, y) is ACCEPTED iff  level[r][x*w + y] == 65535  ||  (a_j >> 16) < level[r][x*w + y]:  level 65535 always, level 0
 * never.  Written are the min(sample_size, kept) positions with the smallest (rejected ? 1 : 0, key, j), ascending: the
 * accepted are a uniform draw among themselves, so a candidate's inclusion is proportional to its level; where fewer than
 * sample_size are accepted the rejected fill up in key order, so the count never depends on the levels.  Integer
 * arithmetic only: nn/rand.py:PhiloxStream.permutation_head_weighted is the host twin, element for element.  All levels
 * 65535, or all 0, give strotss_index_draw's bits; so does a region with level[r] == NULL.  n_out and the counters as
 * above; one launch, one workgroup a region.  lv == NULL: STROTSS_EINVAL; every other refusal as strotss_index_draw. */
typedef struct strotss_draw_levels_t {
  const unsigned short* level[STROTSS_DRAW_MAX_REGIONS];   /* (h, w) levels at THIS scale, or NULL: uniform */
} strotss_draw_levels_t;
int strotss_index_draw_weighted(const strotss_draw_t* d, const strotss_draw_levels_t* lv, void* stream);

/* ---------------------------------------------------------------------------------------
 * Pairwise / moment losses  (nn/losses.py:12-80, run_strotss.py:21-40).
 * Every loss entry computes the loss value AND d(loss)/d(pred) scaled by `gscale`, added
 * into gpred (which the caller zero-fills once per step).  Scalars land in a device array.
 * --------------------------------------------------------------------------------------- */
/* r[i] = rsqrt(max(sum_k x[i,k]^2, 1e-12)) for i < n  (tf.nn.l2_normalize, losses.py:13-14) */
int strotss_row_inv_norm(const float* x, int n, int ld, float* r, void* stream);
/* C[i,j] = 1 - <x_i,y_j> * rx[i]*ry[j], i < nx, j < ny   (losses.py:12-15); C (nx, ldc) row-major, ldc >= ny.
 * Output contract of this entry and of strotss_cosine_distance_x3, whatever the tile grid: exactly the elements of
 * [0, nx) x [0, ny) are written, each once per launch (x == y: the entries below the diagonal are the mirrored copies of
 * those above); the pad columns ny .. ldc - 1 of every row and everything past row nx - 1 are NEVER written -- a caller that
 * reads them finds what it put there (tests/test_hip_tilegrid.py asserts it at every grid up to 16 x 33 tiles). */
int strotss_cosine_distance(const float* x, const float* rx, int nx, const float* y,
                            const float* ry, int ny, int ld, float* C, int ldc, void* stream);
/* The same two entry points on the bf16x3 GEMM core (csrc/mfma_x3.h): every f32 value is split EXACTLY into three
 * bf16 values, six exact partial products, f32 accumulation -- f32-class results at 6/16 of the f32-MFMA cost.
 * strotss_row_inv_norm_x3 also writes the rows as "x3 panels" (3 * n * ld bf16; element (i, k), plane p at
 * ((k/32 * 3 + p) * n + i) * 32 + k%32); r may be NULL.  strotss_cosine_distance_x3 takes the panels of x and y;
 * x == y gives an exactly symmetric matrix.  Same output contract as strotss_cosine_distance: [0, nx) x [0, ny) only, the
 * pad columns and further rows untouched.  The loss entry points below use this core unless STROTSS_X3=0. */
/* C[i][j] = sqrt(max(|x_i|^2 + |y_j|^2 - 2 x_i.y_j, 1e-6) / d)   (nn/losses.py:18-24, l2_distance); x (nx, ld), y (ny, ld)
 * row-major with columns >= d zero, ld % 32 == 0; C (nx, ldc); workspace: nx + ny floats. */
int strotss_l2_distance(const float* x, int nx, const float* y, int ny, int d, int ld, float* C, int ldc,
                        float* workspace, void* stream);
int strotss_row_inv_norm_x3(const float* x, int n, int ld, float* r, void* panels, void* stream);
int strotss_cosine_distance_x3(const void* x_panels, const float* rx, int nx, const void* y_panels, const float* ry,
                               int ny, int ld, float* C, int ldc, void* stream);
/* Backward of a pairwise distance matrix w.r.t. one of its row sets (what tape.gradient does to nn/losses.py:12-24):
 *   dx[i, :] += g * r[i] * ( sum_{j < k} W[i, j] * B[j, :]  -  x[i, :] * r[i] * q[i] ),   i < n,
 * W (n rows, ldw >= k floats per row, ldw % 32 == 0), B (>= ldw rows of ld floats), x / dx (n, ld), ld % 32 == 0; r, q: n
 * floats.  THE CALLER ZERO-FILLS: the product runs over all ldw columns of W and the first ldw rows of B (k is only
 * validated, 0 < k <= ldw), so the sum is the one over j < k exactly when W[i, j] = 0 for k <= j < ldw and rows k .. ldw - 1
 * of B are finite (zero or not); anything else in those columns of W is summed too.  cosine_distance(x, y) with upstream gradient G: W = -G * ry[j],
 * B = y, r = the reciprocal norms of x, q[i] = -sum_j G[i, j] (1 - C[i, j]);  l2_distance: W = -2 G' (G' = G / (2 D C) where
 * the clamp passes), B = y, r = 1, q[i] = -2 sum_j G'[i, j].  f32 MFMA (the loss path's own backward GEMMs run on the
 * bf16x3 core from pre-split panels; this entry is the operator surface's). */
int strotss_rows_gemm_bwd(const float* W, int ldw, int k, const float* B, const float* x, const float* r, const float* q,
                          int n, int ld, float g, float* dx, void* stream);
size_t strotss_selfsim_workspace_bytes(int n, int ld);
/* loss_out[0] = self_similarity(pred, content) (losses.py:55-66);
 * gpred += gscale * dloss/dpred.  pred/content: (rows >= n, ld). */
int strotss_selfsim_fwd_bwd(const float* pred, const float* content, int n, int d, int ld,
                            float gscale, float* gpred, float* loss_out, void* workspace,
                            size_t workspace_bytes, void* stream);
/* Content-weighted self-similarity: with Dx, Dy the cosine matrices of pred and content and A, B their column-normalised forms,
 *   loss_out[0] = (1/n) sum_j col_weight[j] sum_i |A[i,j] - B[i,j]|,   gpred += gscale * dloss/dpred.
 * col_weight: n finite values >= 0 on the device (a device pointer), or NULL = strotss_selfsim_fwd_bwd.  All-ones weights give
 * that entry's results bit for bit.  Same workspace (strotss_selfsim_workspace_bytes) and the same contents left in it:
 * strotss_selfsim_pred_panels borrows from it as from the unweighted call. */
int strotss_selfsim_weighted_fwd_bwd(const float* pred, const float* content, const float* col_weight, int n, int d, int ld,
                                     float gscale, float* gpred, float* loss_out, void* workspace, size_t workspace_bytes,
                                     void* stream);
/* Sinkhorn-Knopp transport cost between the style rows (ns) and the prediction rows (n) on the cosine cost matrix.
 * BUILD-DEFINED: the reference's sinkhorn_knopp (losses.py:83-105) is marked untested, is never called and cannot
 * execute (`tf.ones_like` of a Python tuple); this implements its evident intent:
 *   M = cosine_distance(style, pred), K = exp(-l M), v_0 = 1,
 *   n_iter times:  u = (1/ns) / max(K v, 1e-12),  v = (1/n) / max(K^T u, 1e-12),     loss = sum(u * ((K o M) v)),
 * and gpred += gscale * dloss/dpred, differentiated THROUGH the iterations as autodiff would (checked against a
 * float64 autograd restatement, oracle/strotss_oracle.py: sinkhorn_knopp).  n_iter <= 64. */
size_t strotss_sinkhorn_workspace_bytes(int ns, int n, int n_iter);
int strotss_sinkhorn_cos_fwd_bwd(const float* style, const float* rs, int ns, const float* pred, int n, int d,
                                 int ld, float l, int n_iter, float gscale, float* gpred, float* loss_out,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* strotss_sinkhorn_cos_fwd_bwd as the style term of a train step: the same loss and gradient, with the
 * prologue convention of strotss_remd_cos_fwd_bwd_panels -- pred_inv_norm / pred_panels from the content loss's workspace
 * (strotss_selfsim_pred_panels), rs / style_panels made once per scale (strotss_row_inv_norm_x3).  The scalings and their
 * reverse sweep are the entry's above (a fused one-launch-per-scaling form measured 3.5 times slower).
 * Both panels given: the cost matrix on the bf16x3 core; both NULL (what strotss_selfsim_pred_panels hands out under
 * STROTSS_X3=0): on the f32 MFMA from the rows; one of the two: STROTSS_EINVAL.  No float atomics: the same bits on every
 * call and stream.  Refusals before any launch, outputs and workspace untouched: STROTSS_EINVAL (null pointers, sizes, a
 * workspace below strotss_sinkhorn_step_workspace_bytes), STROTSS_EALIGN (ld % 32 != 0), STROTSS_ERANGE (l not finite or
 * <= 0, n_iter outside 1..64). */
size_t strotss_sinkhorn_step_workspace_bytes(int ns, int n, int n_iter);
int strotss_sinkhorn_cos_fwd_bwd_panels(const float* style, const float* rs, const void* style_panels, int ns, const float* pred,
                                        const float* pred_inv_norm, const void* pred_panels, int n, int d, int ld, float l,
                                        int n_iter, float gscale, float* gpred, float* loss_out, void* workspace,
                                        size_t workspace_bytes, void* stream);
/* The Sinkhorn term of a train step in the log domain: strotss_sinkhorn_cos_fwd_bwd_panels with the
 * scalings kept as phi = log u, psi = log v, so that neither exp(-l M) nor a clamp exists and the term stays a transport
 * cost where the plan is sharp.  With M the cosine distance, px = 1 / ns, py = 1 / n, psi_0 = 0 and LSE the max-shifted
 * log-sum-exp, n_iter times:
 *     phi[i] = log px - LSE_j(psi[j] - l M[i][j]),   psi[j] = log py - LSE_i(phi[i] - l M[i][j]),
 *     loss = sum_ij exp(phi[i] + psi[j] - l M[i][j]) M[i][j],
 * and gpred += gscale * dloss/dpred through all the iterations.  Where the linear form engages no clamp the two are the same
 * function.  Arguments, panels and determinism as strotss_sinkhorn_cos_fwd_bwd_panels.  Refusals before any launch, outputs
 * and workspace untouched: STROTSS_EINVAL (null pointers, sizes, one panel of the two, a workspace below
 * strotss_sinkhorn_log_step_workspace_bytes), STROTSS_EALIGN (ld % 32 != 0), STROTSS_ERANGE (l not in (0, 1000]: the f32
 * exponent psi - l M carries about 2 l 2^-24 of absolute error, 1e-4 at 1000; n_iter outside 1..64).  The bytes entry
 * returns 0 for arguments the call would refuse. */
size_t strotss_sinkhorn_log_step_workspace_bytes(int ns, int n, int n_iter);
int strotss_sinkhorn_log_cos_fwd_bwd_panels(const float* style, const float* rs, const void* style_panels, int ns,
                                            const float* pred, const float* pred_inv_norm, const void* pred_panels, int n, int d,
                                            int ld, float l, int n_iter, float gscale, float* gpred, float* loss_out,
                                            void* workspace, size_t workspace_bytes, void* stream);
/* The sliced Wasserstein distance as the style term of a train step, with the prologue convention of
 * strotss_sinkhorn_cos_fwd_bwd_panels (pred_inv_norm / pred_panels from the content loss's workspace, rs / style_panels made
 * once per scale; both panels: projections on the bf16x3 core, both NULL: on the f32 MFMA from the rows, one of the two:
 * STROTSS_EINVAL).  With xhat_i, shat_j the L2-normalised rows and n_proj sign directions eps_p in {-1, +1}^d,
 *     a[p][i] = <eps_p, xhat_i>,  b[p][j] = <eps_p, shat_j>,  both sorted ascending by (value, row; -0 counts as +0),
 *     W_p = sum_ij len_ij (a_(i) - b_(j))^2,  len_ij = max(0, min((i+1) ns, (j+1) n) - max(i ns, j n)) / (n ns),
 *     loss_out[0] = sum_p W_p / (2 n_proj),   gpred += gscale * dloss/dpred (through the sort, piecewise constant, and
 *     through the normalisation); rows >= n of gpred untouched, pad columns d .. ld-1 of rows < n receive +0.
 * The sign of (direction p, feature k, draw t) is bit k & 31 of word (k >> 5) & 3 of
 * philox4x32_10(ctr = (k >> 7, 2, t, p), key = (seed_lo, seed_hi)): 1 -> +1, 0 -> -1 (c1 = 2: disjoint from
 * strotss_index_draw's blocks, c1 = 0, 1); columns k >= d of the direction matrix are zero.  nn/rand.py:sliced_signs is the
 * host twin.  `counter`: one unsigned in device memory; the entry draws with t = *counter and its last kernel stores t + 1,
 * so a captured graph draws fresh directions on every replay.  7 launches, no float atomics: the same bits on every call
 * and stream for the same counter.  Refusals before any launch, outputs, workspace and counter untouched: STROTSS_EINVAL
 * (null pointers, non-positive sizes, d > ld, one panel of the two, a workspace below strotss_sliced_workspace_bytes),
 * STROTSS_EALIGN (ld % 32 != 0), STROTSS_ERANGE (n or ns above 1024, n_proj above 1024).  The query returns 0 for
 * arguments the entry refuses. */
size_t strotss_sliced_workspace_bytes(int ns, int n, int ld, int n_proj);
int strotss_sliced_cos_fwd_bwd(const float* style, const float* rs, const void* style_panels, int ns, const float* pred,
                               const float* pred_inv_norm, const void* pred_panels, int n, int d, int ld, int n_proj,
                               unsigned seed_lo, unsigned seed_hi, unsigned* counter, float gscale, float* gpred,
                               float* loss_out, void* workspace, size_t workspace_bytes, void* stream);
/* ld = row stride of the feature matrices (strotss_remd_cos_fwd_bwd), 0 for strotss_palette_remd_fwd_bwd */
/* The same with dist_metrics 'l2' (STROTSS_METRIC_L2) or 'both' (STROTSS_METRIC_BOTH) as the cost (losses.py:27-28): cost matrix
 * on the f32 MFMA with the distance in its epilogue, the scalings and their reverse sweep as above, the clamp of l2_distance
 * passing gradient where m >= 1e-6. */
size_t strotss_sinkhorn_metric_workspace_bytes(int ns, int n, int n_iter);
int strotss_sinkhorn_metric_fwd_bwd(const float* style, int ns, const float* pred, int n, int d, int ld, int metric, float l,
                                    int n_iter, float gscale, float* gpred, float* loss_out, void* workspace,
                                    size_t workspace_bytes, void* stream);
size_t strotss_remd_workspace_bytes(int ns, int n, int ld);
/* loss_out[0] = relaxed_emd(style, pred, 'cosine') (losses.py:69-80); gpred += gscale*dloss/dpred.
 * rs = row_inv_norm(style) (constant per scale). */
/* flags (this entry, strotss_remd_metric_fwd_bwd, strotss_palette_remd_fwd_bwd): STROTSS_REMD_SWAPPED = the caller wants the
 * gradient w.r.t. the reference's FIRST argument x and therefore passed x as `pred` and y as `style` (every metric is symmetric,
 * the value is the same); tf.maximum(R_X, R_Y) sends an exact tie to R_X, which is then the kernel's column branch. */
#define STROTSS_REMD_SWAPPED 1
int strotss_remd_cos_fwd_bwd(const float* style, const float* rs, int ns, const float* pred, int n,
                             int d, int ld, float gscale, float* gpred, float* loss_out, int flags,
                             void* workspace, size_t workspace_bytes, void* stream);
/* The same with its prologue already done (a train step computes the prediction rows' reciprocal norms and x3 panels for
 * the content loss anyway, and the style rows' panels do not change within a scale): pred_inv_norm / pred_panels as
 * strotss_row_inv_norm_x3(pred) writes them -- e.g. the ones strotss_selfsim_fwd_bwd left in ITS workspace
 * (strotss_selfsim_pred_panels: pointers into that workspace, valid until it is reused; *panels == NULL when the cost
 * matrices run on the f32 MFMA, STROTSS_X3=0) -- and style_panels = strotss_row_inv_norm_x3(style).  Same result bit for
 * bit, one launch and two passes over the rows less. */
int strotss_selfsim_pred_panels(void* workspace, size_t workspace_bytes, int n, int ld, const float** inv_norm,
                                const void** panels);
int strotss_remd_cos_fwd_bwd_panels(const float* style, const float* rs, const void* style_panels, int ns,
                                    const float* pred, const float* pred_inv_norm, const void* pred_panels, int n,
                                    int d, int ld, float gscale, float* gpred, float* loss_out, void* workspace,
                                    size_t workspace_bytes, void* stream);
/* loss_out[0] = relaxed_emd(yuv(style[:, :3]), yuv(pred[:, :3]), 'both') (run_strotss.py:37-39);
 * gpred[:, :3] += gscale*dloss/dpred[:, :3].  style/pred are the full (rows, ld) matrices, of
 * which only the first three columns are read.  rgb_to_yuv != 0 applies convert_rgb_to_yuv
 * (strotss_utils.py:166-167) to them first; 0 takes them as they are (losses.relaxed_emd 'both').
 * Workspace: strotss_remd_workspace_bytes(ns, n, 0). */
int strotss_palette_remd_fwd_bwd(const float* style, int ns, const float* pred, int n, int ld,
                                 int rgb_to_yuv, float gscale, float* gpred, float* loss_out, int flags,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* The sliced 1-Wasserstein distance in the place of the palette relaxed EMD.  With
 * y_i = yuv(pred_i[:3]), s_j = yuv(style_j[:3]) (rgb_to_yuv as in strotss_palette_remd_fwd_bwd) and n_proj unit directions
 * theta_p of R^3 (dirs: n_proj x 3 floats in device memory; nn/rand.py:palette_directions makes the engine's),
 *     a[p][i] = <theta_p, y_i>,  b[p][j] = <theta_p, s_j>,  both sorted ascending by (value, row; -0 counts as +0),
 *     W_p = sum_ij len_ij |a_(i) - b_(j)|,  len_ij = max(0, min((i+1) ns, (j+1) n) - max(i ns, j n)) / (n ns),
 *     loss_out[0] = (2 / (sqrt(3) n_proj)) sum_p W_p,
 *     gpred[i][:3] += gscale * dloss/dpred_i[:3] (through the sort, piecewise constant; sign(0) = 0), each added value
 *     rounded on its own; rows >= n and columns >= 3 of gpred are not written.
 * 2 launches, no float atomics: the same bits on every call and stream.  Refusals before any launch, outputs and workspace
 * untouched: STROTSS_EINVAL (null pointers, non-positive sizes, ld < 3, a workspace below
 * strotss_palette_sliced_workspace_bytes), STROTSS_ERANGE (n or ns above 1024, n_proj above 1024).  As
 * strotss_palette_remd_fwd_bwd, the entry reads three scalars a row and takes every ld >= 3 (no STROTSS_EALIGN).  The query
 * returns 0 for arguments the entry refuses. */
size_t strotss_palette_sliced_workspace_bytes(int ns, int n, int n_proj);
int strotss_palette_sliced_fwd_bwd(const float* style, int ns, const float* pred, int n, int ld, int rgb_to_yuv,
                                   const float* dirs, int n_proj, float gscale, float* gpred, float* loss_out,
                                   void* workspace, size_t workspace_bytes, void* stream);
/* relaxed_emd(style, pred, distance) for the other two entries of dist_metrics (losses.py:27-28) at ANY width d:
 * metric STROTSS_METRIC_L2 -> l2_distance (losses.py:18-24), STROTSS_METRIC_BOTH -> cosine + l2.  Same reductions and
 * tie rules as strotss_remd_cos_fwd_bwd (tf.reduce_min splits among ties, tf.maximum -> first argument);
 * tf.maximum(m, 1e-6) inside l2_distance passes gradient where m >= 1e-6.  gpred += gscale*dloss/dpred. */
#define STROTSS_METRIC_L2 1
#define STROTSS_METRIC_BOTH 2
size_t strotss_remd_metric_workspace_bytes(int ns, int n);
int strotss_remd_metric_fwd_bwd(const float* style, int ns, const float* pred, int n, int d, int ld, int metric,
                                float gscale, float* gpred, float* loss_out, int flags, void* workspace,
                                size_t workspace_bytes, void* stream);
/* The four loss terms of one train step on the same prediction rows (run_strotss.py:131-142, 33-40) in ONE call:
 * loss_content[0] = self_similarity(pred, content), loss_moment[0] = moment_matching(style, pred) (style side given by
 * strotss_moment_stats), loss_remd[0] = relaxed_emd(style, pred) (cosine; style_inv_norm / style_panels =
 * strotss_row_inv_norm_x3(style)), loss_palette[0] = relaxed_emd(yuv(style[:, :3]), yuv(pred[:, :3]), 'both'),
 * gpred += g_content * d(content)/d(pred) + g_moment * ... + g_remd * ... + g_palette * ....  Bit for bit
 * strotss_selfsim_fwd_bwd, strotss_moment_fwd_bwd, strotss_remd_cos_fwd_bwd_panels and strotss_palette_remd_fwd_bwd called in
 * this order; the three forward GEMMs (two symmetric cost matrices, covariance, prediction x style cost matrix) share ONE
 * launch, the prologues of all four terms another, every statistic of the forward products (self-similarity rows, moment
 * scalars, REMD and palette minima) a third, the two branch selections + the self-similarity gradient matrix a fourth:
 * 9 launches instead of 21.
 * bf16x3 core only: STROTSS_EINVAL when STROTSS_X3 / _COST / _MOMENT switch it off (take the separate entry points).
 * strotss_step_losses_available() is 1 exactly when the switches (read once per process) do NOT make this entry and the
 * blend / cw entries below refuse that way: the caller asks instead of parsing the switches itself. */
int strotss_step_losses_available(void);
size_t strotss_step_losses_workspace_bytes(int ns, int n, int ld);
int strotss_step_losses_fwd_bwd(const float* pred, const float* content, int n, int d, int ld, const float* style,
                                const float* style_inv_norm, const void* style_panels, int ns, const float* style_mean,
                                const float* style_cov, float g_content, float g_moment, float g_remd, float g_palette,
                                float* gpred, float* loss_content, float* loss_moment, float* loss_remd, float* loss_palette,
                                void* workspace, size_t workspace_bytes, void* stream);
/* Style blending: the same step against a weighted set of 1 .. STROTSS_MAX_STYLES style targets.  Style k is what
 * strotss_step_losses_fwd_bwd takes for one style (feats[k] = its ns[k] sampled rows, inv_norm / panels =
 * strotss_row_inv_norm_x3(feats[k]), mean / cov = strotss_moment_stats(feats[k])); weight[k] >= 0, finite (the caller
 * normalises them).  loss_content[0] as above; loss_moment[k], loss_remd[k], loss_palette[k] = the UNWEIGHTED terms of
 * style k;  gpred += g_content * dLc + sum_k weight[k] * (g_moment * dLm_k + g_remd * dLr_k + g_palette * dLp_k).
 * n_styles == 1 is strotss_step_losses_fwd_bwd itself (g_moment, g_remd, g_palette times weight[0]).  n_styles > 1: the
 * same 9 launches whatever the count -- one covariance of the prediction rows compared with every style's, one
 * prediction x style cost matrix per style in the grouped forward launch, statistics, selections and sparse backward
 * passes segmented per style, ONE moment backward product on the weighted sign matrix.
 * STROTSS_EINVAL: null pointers, bad sizes or weights, bf16x3 core switched off; STROTSS_ERANGE: n_styles outside
 * 1 .. STROTSS_MAX_STYLES or a style with more rows than the tie lists hold (2048); STROTSS_EALIGN: ld % 32 != 0. */
#define STROTSS_MAX_STYLES 4
typedef struct {
  int n_styles;
  const float* feats[STROTSS_MAX_STYLES];      /* (ns[k], ld) rows */
  const float* inv_norm[STROTSS_MAX_STYLES];   /* (ns[k]) */
  const void* panels[STROTSS_MAX_STYLES];      /* x3 panels of feats[k] */
  int ns[STROTSS_MAX_STYLES];
  const float* mean[STROTSS_MAX_STYLES];       /* (ld) */
  const float* cov[STROTSS_MAX_STYLES];        /* (ld, ld) */
  float weight[STROTSS_MAX_STYLES];
} strotss_style_set_t;
size_t strotss_step_losses_blend_workspace_bytes(const strotss_style_set_t* styles, int n, int ld);
int strotss_step_losses_blend_fwd_bwd(const float* pred, const float* content, int n, int d, int ld,
                                      const strotss_style_set_t* styles, float g_content, float g_moment, float g_remd,
                                      float g_palette, float* gpred, float* loss_content, float* loss_moment,
                                      float* loss_remd, float* loss_palette, void* workspace, size_t workspace_bytes,
                                      void* stream);
/* strotss_step_losses_blend_fwd_bwd with the content term weighted per sampled column as strotss_selfsim_weighted_fwd_bwd
 * (col_weight: n device floats, finite, >= 0; NULL = that entry).  Same workspace (strotss_step_losses_blend_workspace_bytes),
 * same launches: n_styles == 1 the single-style structure, n_styles > 1 the blended one.  All-ones weights: bit for bit. */
int strotss_step_losses_cw_fwd_bwd(const float* pred, const float* content, int n, int d, int ld, const float* col_weight,
                                   const strotss_style_set_t* styles, float g_content, float g_moment, float g_remd,
                                   float g_palette, float* gpred, float* loss_content, float* loss_moment, float* loss_remd,
                                   float* loss_palette, void* workspace, size_t workspace_bytes, void* stream);
size_t strotss_moment_workspace_bytes(int n, int ld);
/* style side of moment_matching, once per scale: mean_out(ld), cov_out(ld,ld) = biased covariance */
int strotss_moment_stats(const float* x, int n, int d, int ld, float* mean_out, float* cov_out,
                         void* workspace, size_t workspace_bytes, void* stream);
/* loss_out[0] = moment_matching(style, pred) (losses.py:39-52) with the style statistics
 * cached; gpred += gscale*dloss/dpred. */
int strotss_moment_fwd_bwd(const float* style_mean, const float* style_cov, const float* pred,
                           int n, int d, int ld, float gscale, float* gpred, float* loss_out,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Temporal consistency of frame sequences: the short-term temporal loss of Ruder et al. (2016)
 * --------------------------------------------------------------------------------------- */
/* Once per frame, in ONE launch: the previous stylised frame prev(h, w, c) warped along the backward flow and its
 * certainty.  flow_b, flow_f: (h, w, 2) = (u, v) displacements in pixels (frame t -> t-1 and t-1 -> t); flow_f may be NULL.
 *   warped(y, x, :) = prev sampled at (x + u_b, y + v_b): pixel centres at integer coordinates, bilinear over the 4
 *                     neighbours, indices clamped to the edge;
 *   certainty(y, x) = 0 where the sample point lies outside [0, w-1] x [0, h-1], where it is disoccluded (flow_f given:
 *                     |f_b + f_f(p + f_b)|^2 > 0.01 (|f_b|^2 + |f_f(p + f_b)|^2) + 0.5, f_f sampled by the same rule) or on
 *                     a motion boundary (|grad u_b|^2 + |grad v_b|^2 > 0.01 |f_b|^2 + 0.002, central differences with
 *                     clamped indices); 1 elsewhere.  Coordinates and tests in float64.
 * Out-of-range and non-finite coordinates, per axis (n = w or h): the coordinate s = x + u is clamped to [-2, n + 1] before
 * its floor, a NaN taken as -2; both taps are then clamped to [0, n - 1].  So s < 0, -inf and NaN sample the edge pixel 0,
 * s > n - 1 and +inf the edge pixel n - 1: warped is finite wherever prev is, whatever the flows hold.  s == n - 1 is inside
 * the frame (certainty by the other tests, the sample exact); the next float32 u beyond it, +-inf and NaN are outside:
 * certainty 0, and flow_f is not consulted.  The threshold tests are IEEE `>` comparisons: a NaN on the left (a NaN in a
 * neighbour's flow_b or in a tap of flow_f, zero-weight taps included, or inf - inf) removes nothing, +inf against a finite
 * right side removes the pixel.  Pixels whose own tests read only finite values are unaffected by non-finite ones elsewhere. */
int strotss_flow_warp(const float* prev, int h, int w, int c, const float* flow_b, const float* flow_f, float* warped,
                      float* certainty, void* stream);
/* bytes of the workspace of strotss_temporal_fwd_bwd (0 for h, w <= 0) */
size_t strotss_temporal_workspace_bytes(int h, int w);
/* The temporal term of one step, in ONE launch (img, target, gimg: (h, w, 3); certainty: (h, w); all 16-byte aligned):
 *   loss_out[0] = (1 / (3 h w)) sum_p certainty(p) sum_ch (img - target)^2,   gimg += gscale * dloss/dimg.
 * gscale == 0 or certainty(p) == 0 leaves gimg (at p) bit for bit.  The scalar is a fixed-order reduction (block partials,
 * summed in a fixed order by the last block to finish; no float atomics).  workspace: strotss_temporal_workspace_bytes(h, w)
 * bytes, 16-byte aligned, ZEROED before its first use; every call leaves it ready for the next (one call at a time). */
int strotss_temporal_fwd_bwd(const float* img, const float* target, const float* certainty, int h, int w, float gscale,
                             float* gimg, float* loss_out, void* workspace, void* stream);

/* Long-term temporal consistency: 1 .. STROTSS_MAX_TEMPORAL warped earlier results at once, nearest
 * frame first.  Once per frame, in ONE launch, one thread per pixel: raw, out (count, h, w), plane j = certainty of the
 * j-th nearest frame;  out_j(p) = max(raw_j(p) - sum_{k < j} raw_k(p), 0), the sum in ascending k in float32 (out may equal
 * raw).  STROTSS_EINVAL: null pointers, h, w <= 0, count outside 1 .. STROTSS_MAX_TEMPORAL, 3 h w > INT_MAX;
 * STROTSS_EALIGN: a pointer not 16-byte aligned. */
#define STROTSS_MAX_TEMPORAL 4
int strotss_temporal_long_certainty(const float* raw, int count, int h, int w, float* out, void* stream);
typedef struct {
  int count;                                     /* 1 .. STROTSS_MAX_TEMPORAL */
  const float* target[STROTSS_MAX_TEMPORAL];     /* (h, w, 3) */
  const float* certainty[STROTSS_MAX_TEMPORAL];  /* (h, w), already combined */
  float gscale[STROTSS_MAX_TEMPORAL];
} strotss_temporal_set_t;
/* bytes of the workspace of strotss_temporal_multi_fwd_bwd (0 for h, w <= 0 or count outside 1 .. STROTSS_MAX_TEMPORAL) */
size_t strotss_temporal_multi_workspace_bytes(int h, int w, int count);
/* The temporal terms of several targets in ONE launch, each read once (img, gimg, every target and certainty 16-byte
 * aligned):  loss_out[j] = (1 / (3 h w)) sum_p certainty_j(p) sum_ch (img - target_j)^2 for j < count,
 * gimg += sum_j gscale_j * dloss_j/dimg, added in ascending j per element.  count == 1 is strotss_temporal_fwd_bwd (the
 * same kernel).  Every gscale_j == 0, or certainty_j(p) == 0 for every j, leaves gimg (at p) bit for bit.  Fixed-order
 * reductions per j, no float atomics.  workspace: strotss_temporal_multi_workspace_bytes(h, w, set->count) bytes, ZEROED
 * before its first use (one call at a time).  STROTSS_EINVAL: null pointers, h, w <= 0, count outside
 * 1 .. STROTSS_MAX_TEMPORAL, 3 h w > INT_MAX; STROTSS_EALIGN: a pointer not 16-byte aligned. */
int strotss_temporal_multi_fwd_bwd(const float* img, const strotss_temporal_set_t* set, int h, int w, float* gimg,
                                   float* loss_out, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------
 * Pixel-space priors of the step: a Laplacian detail term against the content and a total variation
 * --------------------------------------------------------------------------------------- */
/* P_p of an (h, w, ch) array, ch 1 or 3, p in {1, 2, 4, 8, 16}: out (ceil(h / p), ceil(w / p), ch), cell (i, j) the mean of
 * the pixels [i p, min((i+1) p, h)) x [j p, min((j+1) p, w)) it covers: every row summed left to right, the row sums added top
 * to bottom, in float32, the total divided by their count.  ONE launch.  STROTSS_EINVAL: null pointers, h, w <= 0, ch not 1 or 3, 3 h w > INT_MAX;
 * STROTSS_ERANGE: p not in the set; STROTSS_EALIGN: a pointer not 16-byte aligned. */
int strotss_pool_mean(const float* img, int h, int w, int ch, int p, float* out, void* stream);
#define STROTSS_MAX_DETAIL_POOLS 3
typedef struct {
  int count;                                       /* 1 .. STROTSS_MAX_DETAIL_POOLS */
  int pool[STROTSS_MAX_DETAIL_POOLS];              /* distinct values of {1, 2, 4, 8, 16}, ascending */
  const float* content[STROTSS_MAX_DETAIL_POOLS];  /* P_p(content): (hp, wp, 3), from strotss_pool_mean */
  const float* weight[STROTSS_MAX_DETAIL_POOLS];   /* cell weights m_p >= 0: (hp, wp), or NULL for 1 */
  float gscale[STROTSS_MAX_DETAIL_POOLS];
} strotss_detail_set_t;
/* bytes of the workspace of strotss_detail_fwd_bwd for any set (0 for h, w <= 0 or 3 h w > INT_MAX) */
size_t strotss_detail_workspace_bytes(int h, int w);
/* The Laplacian detail term of one step (img, gimg: (h, w, 3)).  Per pool size p = pool[j], hp = ceil(h / p),
 * wp = ceil(w / p), L the graph Laplacian of the hp x wp 4-neighbour grid ((L u)(k) = deg(k) u(k) - sum of the neighbours
 * inside the grid), D = L (P_p(img) - content[j]) per channel:
 *   loss_out[j] = (1 / (3 hp wp)) sum_k m(k) sum_ch D(k, ch)^2,
 *   gimg(q, ch) += (2 gscale[j] / (3 hp wp cnt(k))) (L (m D))(k, ch) for every pixel q of cell k, cnt(k) its pixel count,
 * the pool sizes in ascending order.  Per pool size ONE launch, after one strotss_pool_mean launch of img into the workspace
 * when p > 1.  A gradient value that is exactly 0 is not added: gscale[j] == 0 for every j stores nothing, a cell whose own
 * and whose neighbours' weights are 0 leaves its pixels' gimg bit for bit, and img == content pixel for pixel gives
 * loss_out[j] == 0 and leaves gimg bit for bit.  Fixed-order reductions, no float atomics.  workspace:
 * strotss_detail_workspace_bytes(h, w) bytes, 16-byte aligned, ZEROED before its first use (one call at a time).
 * Refused before anything is launched: STROTSS_EINVAL (null img, set, gimg, loss_out, workspace or content[j], h, w <= 0,
 * 3 h w > INT_MAX), STROTSS_ERANGE (count outside 1 .. STROTSS_MAX_DETAIL_POOLS, a pool size not in the set or not
 * ascending), STROTSS_EALIGN (a pointer not 16-byte aligned). */
int strotss_detail_fwd_bwd(const float* img, int h, int w, const strotss_detail_set_t* set, float* gimg, float* loss_out,
                           void* workspace, void* stream);
/* bytes of the workspace of strotss_tv_fwd_bwd (0 for h, w <= 0 or 3 h w > INT_MAX) */
size_t strotss_tv_workspace_bytes(int h, int w);
/* The total variation of one step in ONE launch (img, gimg: (h, w, 3)): dx(r, s) = img(r, s+1) - img(r, s), 0 in the last
 * column, dy likewise, 0 in the last row, per channel;
 *   loss_out[0] = (1 / (3 h w)) sum_q sum_ch (sqrt(dx^2 + dy^2 + eps^2) - eps),   gimg += gscale * dloss/dimg.
 * gscale == 0 stores nothing; a gradient value that is exactly 0 is not added (a constant image: loss 0, gimg bit for bit).
 * Fixed-order reduction, no float atomics.  workspace: strotss_tv_workspace_bytes(h, w) bytes, 16-byte aligned, ZEROED before
 * its first use.  Refused before anything is launched: STROTSS_EINVAL (null pointers, h, w <= 0, 3 h w > INT_MAX),
 * STROTSS_ERANGE (eps not finite or <= 0), STROTSS_EALIGN (a pointer not 16-byte aligned). */
int strotss_tv_fwd_bwd(const float* img, int h, int w, float eps, float gscale, float* gimg, float* loss_out,
                       void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------
 * The photorealism term of the step: the matting Laplacian of the content, L p = N (p - q)
 * --------------------------------------------------------------------------------------- */
#define STROTSS_MATTING_MAX_RADIUS 4
/* bytes of the window statistics of strotss_matting_prepare: 36 per pixel (0 for h, w <= 0 or 3 h w > INT_MAX) */
size_t strotss_matting_stats_bytes(int h, int w);
/* The guide's window statistics, once per scale, ONE launch.  guide (h, w, 3) float32; window w_k the (2r+1) x (2r+1) box
 * around pixel k clipped to the image (the windows of strotss_guided_smooth); eps at its float32 value.  stats: 9 planes of
 * (h, w) float32: planes 0..2 mu_k = mean_w guide, planes 3..8 the entries 00, 01, 02, 11, 12, 22 of the inverse of
 * Sigma_k = cov_w(guide) + eps Id, computed in float64 and rounded once.  Refused before the launch: STROTSS_EINVAL (null
 * pointers, h, w <= 0, 3 h w > INT_MAX), STROTSS_ERANGE (r outside 1 .. STROTSS_MATTING_MAX_RADIUS, eps not finite or outside
 * [1e-4, 1]), STROTSS_EALIGN (a pointer not 16-byte aligned). */
int strotss_matting_prepare(const float* guide, int h, int w, int r, float eps, float* stats, void* stream);
/* bytes of the workspace of strotss_matting_fwd_bwd (0 for h, w <= 0 or 3 h w > INT_MAX) */
size_t strotss_matting_workspace_bytes(int h, int w);
/* The photorealism term of one step in ONE launch (img, guide, gimg: (h, w, 3); stats from strotss_matting_prepare with the
 * same guide, h, w and r).  Per window k and channel c: pbar = mean_w img_c, a = Sigma_k^{-1} cov_w(guide, img_c),
 * b = pbar - a . mu_k; q_c(i) = abar_c(i) . guide(i) + bbar_c(i) with abar, bbar the means of a, b over the clipped window
 * around i, N_i its pixel count:
 *   loss_out[0] = (1 / (3 h w)) sum_i N_i sum_c img_c(i) (img_c(i) - q_c(i)),
 *   gimg_c(i) += gscale (2 / (3 h w)) N_i (img_c(i) - q_c(i)).
 * float32 throughout, covariances centred.  gscale == 0 stores nothing; a gradient value that is exactly 0 is not added (a
 * 1 x 1 image: loss 0, gimg bit for bit).  Fixed-order reduction, no float atomics.  workspace:
 * strotss_matting_workspace_bytes(h, w) bytes, 16-byte aligned, ZEROED before its first use (one call at a time).  Refused
 * before the launch: STROTSS_EINVAL (null pointers, h, w <= 0, 3 h w > INT_MAX), STROTSS_ERANGE (r outside
 * 1 .. STROTSS_MATTING_MAX_RADIUS), STROTSS_EALIGN (a pointer not 16-byte aligned). */
int strotss_matting_fwd_bwd(const float* img, const float* guide, const float* stats, int h, int w, int r, float gscale,
                            float* gimg, float* loss_out, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------
 * Optical flow between two frames: what strotss_flow_warp consumes, computed by the library
 * --------------------------------------------------------------------------------------- */
/* Coarse-to-fine Horn-Schunck with warping, solved by Jacobi iterations (Meinhardt-Llopis, Sanchez, Kondermann, IPOL 2013,
 * Jacobi in place of SOR: no sweep order, no atomics, the same bits on every run).  frame_a, frame_b: (h, w, 3) RGB in
 * [0, 1]; flow_out: (h, w, 2) = (u, v), x and y displacement in pixels with frame_a(p) ~ frame_b(p + flow(p)) -- flow_b of
 * strotss_flow_warp for frame t is (frame_t, frame_{t-j}), flow_f is (frame_{t-j}, frame_t).
 *   1. grey g = 0.299 R + 0.587 G + 0.114 B;  2. level 0 of each pyramid = blur(g), blur = separable [1 4 6 4 1] / 16, along
 *   the rows then the columns, indices clamped;  3. level k+1 = blur(level k)[::2, ::2] (ceil(h/2) x ceil(w/2)) while
 *   min(h_k, w_k) / 2 >= min_side and fewer than max_levels levels;  4. u = v = 0 at the coarsest level; to a finer level:
 *   u'(y, x) = 2 bilinear(u, x/2, y/2), v' likewise (the 4-neighbour, edge-clamped rule of strotss_flow_warp);  5. per level,
 *   `warps` times: Bw = bilinear(B_k, x + u, y + v), Ix, Iy = central differences of Bw with clamped indices,
 *   c = Bw - A_k - Ix u - Iy v, inv = 1 / (alpha2 + Ix^2 + Iy^2), then `iters` times for all pixels at once:
 *   ub = (N + S + W + E of u) / 6 + (the four diagonals of u) / 12 with clamped indices, vb likewise,
 *   t = (Ix ub + Iy vb + c) inv, u <- ub - Ix t, v <- vb - Iy t;  6. flow = (u, v) of level 0.  float32 throughout.
 * iters_per_launch: 1 = one sweep per launch; 2, 4, 8 = that many sweeps per launch on LDS-resident tiles with a halo
 * (bit for bit the results of 1).  alpha2 is the smoothness weight for greys in [0, 1]. */
typedef struct { float alpha2; int warps, iters, min_side, max_levels, iters_per_launch; } strotss_flow_params_t;
/* the defaults: alpha2 0.01, warps 5, iters 32, min_side 12, max_levels 8, iters_per_launch 8 */
void strotss_flow_default_params(strotss_flow_params_t* out);
/* bytes of the workspace of strotss_optical_flow (both pyramids, the (u, v) ping-pong, the coefficients); 0 on bad
 * arguments (see below).  params == NULL: the defaults. */
size_t strotss_flow_workspace_bytes(int h, int w, const strotss_flow_params_t* params);
/* The whole flow on `stream` from this one call.  params == NULL: the defaults, with iters_per_launch = 1 above 4096
 * pixels, where the one-sweep form measured faster (the same bits either way).  STROTSS_EINVAL (nothing is launched or
 * written): a null pointer, h or w < 2, h w > 2^28, alpha2 not finite or <= 0, warps or iters < 1, min_side < 1, max_levels
 * outside 1 .. STROTSS_MAX_LEVELS, iters_per_launch not in {1, 2, 4, 8} or not dividing iters, workspace_bytes below
 * strotss_flow_workspace_bytes(h, w, params); STROTSS_EALIGN: frame_a, frame_b, flow_out or workspace not 16-byte aligned. */
int strotss_optical_flow(const float* frame_a, const float* frame_b, int h, int w, const strotss_flow_params_t* params,
                         float* flow_out, void* workspace, size_t workspace_bytes, void* stream);

/* The patch-matching stage (tests/_flow_match_ref.py is the statement): what the coarse-to-fine flow
 * misses, an object that moves against its background and that the coarse levels no longer see.  At one level, with grey
 * planes a, b (h, w) and the level's flow (u, v): for each pixel p and each whole offset d = (dx, dy) in [-R, R]^2,
 *   C(p, d) = sum over the 5 x 5 window q around p (indices clamped, row-major) of |a(q) - bilinear(b, q + F(p) + d)|,
 * the flow of the CENTRE pixel for all 25 taps, the 4-neighbour edge-clamped rule, F(p) split once into whole part and
 * fraction (|F| clamped to 1e6 first).  d* = the first minimiser in scan order (dy outer, dx inner, ascending);
 * F'(p) = F(p) + d* if C(p, d*) < C(p, 0) strictly, else F(p) itself: d = 0 wins every tie.  Every float32 operation is
 * rounded on its own.
 * strotss_flow_match_stage: the stage alone, (u, v) -> (u_out, v_out), all planes (h, w) and distinct.  Refused before
 * anything is launched, the outputs untouched: STROTSS_EINVAL for a null pointer, h or w < 1, h w > 2^28, match_radius
 * outside 1 .. STROTSS_FLOW_MATCH_MAX_RADIUS, an output that is an input or the other output; STROTSS_EALIGN for a pointer
 * that is not 16-byte aligned. */
#define STROTSS_FLOW_MATCH_MAX_RADIUS 4
int strotss_flow_match_stage(const float* a, const float* b, int h, int w, const float* u, const float* v, int match_radius,
                             float* u_out, float* v_out, void* stream);
/* strotss_optical_flow with the stage at every level, on the level's starting flow (the upsampled one; zeros at the
 * coarsest) and before its warps, written to the other half of the (u, v) ping-pong: the workspace is that of
 * strotss_flow_workspace_bytes.  match_radius = 0 IS strotss_optical_flow: the same launches, the same bits.  Refusals as
 * there, and STROTSS_EINVAL for a match_radius outside 0 .. STROTSS_FLOW_MATCH_MAX_RADIUS. */
int strotss_optical_flow_match(const float* frame_a, const float* frame_b, int h, int w, const strotss_flow_params_t* params,
                               int match_radius, float* flow_out, void* workspace, size_t workspace_bytes, void* stream);

/* The robust form (tests/_flow_robust_ref.py is the statement and fixes the evaluation order):
 * Charbonnier penalties on the data term and on the flow's gradient, minimised with lagged weights, so that a motion
 * boundary is not smoothed away.  The pyramid, the upsampling, the warp and Ix, Iy, c are strotss_optical_flow's; alpha2 and
 * inv are not used.  Per warp, `outer` times:  1. weights from the current (u, v), indices clamped: r = Ix u + Iy v + c,
 *   d = 1 / sqrt(r^2 + eps_d^2), s = 1 / sqrt(|grad u|^2 + |grad v|^2 + eps_s^2) with central differences, for the 8
 *   neighbours q of p g_q = w_q (s_p + s_q) / 2 (w_q = 1/6 for N, S, W, E and 1/12 for the diagonals), G = sum g_q,
 *   k = d / (alpha G + d (Ix^2 + Iy^2));  2. iters / outer sweeps with s, 1 / G and k frozen: ub = (sum g_q u_q) / G, vb
 *   likewise, t = (Ix ub + Iy vb + c) k, u <- ub - Ix t, v <- vb - Iy t.  Every float32 operation is rounded on its own. */
typedef struct { float alpha, eps_d, eps_s; int outer; } strotss_flow_robust_params_t;
#define STROTSS_FLOW_ROBUST_MAX_OUTER 8
/* the defaults: alpha 0.06, eps_d 1e-3, eps_s 1e-2, outer 4 */
void strotss_flow_robust_default_params(strotss_flow_robust_params_t* out);
/* bytes of the workspace of strotss_optical_flow_robust: that of strotss_flow_workspace_bytes and, behind it, the planes s
 * (h, w) and {1 / G, k} (h, w, 2) at the full size; 0 on bad arguments (see below).  robust == NULL: exactly
 * strotss_flow_workspace_bytes(h, w, params). */
size_t strotss_flow_robust_workspace_bytes(int h, int w, const strotss_flow_params_t* params,
                                           const strotss_flow_robust_params_t* robust);
/* strotss_optical_flow_match with the robust solver: one weight-update launch and (iters / outer) / iters_per_launch sweep
 * launches, `outer` times per warp; iters_per_launch = 1 is one weighted sweep per launch, 2, 4, 8 the LDS-blocked form (bit
 * for bit the results of 1).  robust == NULL IS strotss_optical_flow_match: the same launches, the same bits, the workspace
 * of strotss_flow_workspace_bytes.  Refusals as there (nothing is launched or written), and STROTSS_EINVAL for alpha, eps_d
 * or eps_s not finite or <= 0 (or an eps whose square is 0 in float32), outer outside 1 .. STROTSS_FLOW_ROBUST_MAX_OUTER or
 * not dividing iters, iters_per_launch not dividing iters / outer, workspace_bytes below
 * strotss_flow_robust_workspace_bytes(h, w, params, robust). */
int strotss_optical_flow_robust(const float* frame_a, const float* frame_b, int h, int w, const strotss_flow_params_t* params,
                                const strotss_flow_robust_params_t* robust, int match_radius, float* flow_out,
                                void* workspace, size_t workspace_bytes, void* stream);
/* One weight update on its own, for tests: coef (h, w, 4) = {Ix, Iy, c, unused} and the flow planes u, v (h, w) -> s_out
 * (h, w), gk_out (h, w, 2) = {1 / G, k} and, after `sweeps` sweeps in launches of iters_per_launch, u_out, v_out (h, w).
 * tmp: 2 h w floats of scratch.  robust == NULL: the defaults; its `outer` is not used.  Refused before anything is
 * launched, the outputs untouched: STROTSS_EINVAL for a null pointer, h or w < 2, h w > 2^28, the parameters as above,
 * iters_per_launch not in {1, 2, 4, 8} or not dividing sweeps, sweeps outside 1..1024, an output that is an input or
 * another output; STROTSS_EALIGN for a pointer that is not 16-byte aligned. */
int strotss_flow_robust_stage(const float* coef, const float* u, const float* v, int h, int w,
                              const strotss_flow_robust_params_t* robust, int sweeps, int iters_per_launch, float* u_out,
                              float* v_out, float* s_out, float* gk_out, float* tmp, void* stream);

/* ---------------------------------------------------------------------------------------
 * Colour preservation: keep the content's colours, after Gatys et al. (2016)
 * --------------------------------------------------------------------------------------- */
/* Images are (h, w, 3) float32 RGB, a weight plane is (h, w) float32 >= 0 (NULL = all ones); every pointer 16-byte aligned.
 * The three entries refuse, before anything is launched: STROTSS_EINVAL for a null required pointer, h or w <= 0,
 * 3 h w > INT_MAX; STROTSS_EALIGN for a pointer that is not 16-byte aligned. */
/* bytes of the workspace of strotss_color_stats (0 for h, w <= 0 or 3 h w > INT_MAX): a 16-byte ticket header and ten doubles
 * per block of 1024 pixels, at most 2048 blocks (COLOR_MAX_BLOCKS of csrc/color.hip) -- from h w > 2^21 on the size stays at
 * 16 + 163840 bytes and the blocks stride over the image; the layout holds for every size the entry accepts only because of
 * that cap (tests/test_hip_launch_caps.py runs the strided form). */
size_t strotss_color_stats_workspace_bytes(int h, int w);
/* The colour statistics of an image, in ONE launch:  out[0] = W = sum_p m(p),  out[1..3] = S_i = sum_p m(p) x_i(p),
 * out[4..9] = S_ij = sum_p m(p) x_i(p) x_j(p) for (i, j) = (0,0) (0,1) (0,2) (1,1) (1,2) (2,2), m = weight (NULL: 1).
 * Accumulated in float64 (the products of two float32 values are exact there): per-thread sums in element order, a fixed
 * tree per block, the block partials summed in a fixed order by the last block to finish (integer ticket, no float
 * atomics) -- the same ten doubles, bit for bit, on every run.  out: ten doubles in DEVICE memory.  workspace:
 * strotss_color_stats_workspace_bytes(h, w) bytes, ZEROED before its first use; every call leaves it ready for the next
 * (one call at a time).  Mean and covariance are formed by the caller: mu = S / W, Sigma = S_ij / W - mu mu^T. */
int strotss_color_stats(const float* img, const float* weight, int h, int w, double* out, void* workspace, void* stream);
/* out(p) = A img(p) + b where weight(p) != 0 (NULL: everywhere), img(p) bit for bit elsewhere.  A (row-major 3 x 3) and
 * b (3) are HOST arrays, read during the call; a value that is not finite: STROTSS_EINVAL.  Per output channel
 * b_i + A_i0 x_0 + A_i1 x_1 + A_i2 x_2 in float32, evaluated left to right, NOT clamped to [0, 1].  out may equal img. */
int strotss_color_affine(const float* img, const float* weight, int h, int w, const float* A, const float* b, float* out,
                         void* stream);
/* "The luma of the result on the chroma of the content":  out_ch(p) = content_ch(p) + (Y(result(p)) - Y(content(p))),
 * Y = 0.299 R + 0.587 G + 0.114 B in float32 (the inverse of the RGB -> YUV matrix sends Y to (1, 1, 1)).  result == content
 * returns the content bit for bit.  out may equal result or content. */
int strotss_luma_merge(const float* result, const float* content, int h, int w, float* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Colour distribution transfer: iterative distribution transfer after Pitie, Kokaram and Dahyot (2007)
 * --------------------------------------------------------------------------------------- */
/* Images and weight planes as above; a pixel COUNTS when its weight is != 0 (NULL: every pixel).  A basis is a row-major
 * 3 x 3 float32 matrix R whose COLUMNS are the axes, in HOST memory, read during the call; a set of bases is n_bases of them
 * back to back.  Axis k of R has the range [lo, hi], computed in double from the float32 R: with lo0 = sum_i min(R_ik, 0) and
 * hi0 = sum_i max(R_ik, 0) (the unit cube's projection), lo = (lo0 + hi0)/2 - (hi0 - lo0), hi = (lo0 + hi0)/2 + (hi0 - lo0);
 * lo, hi and scale = bins / (hi - lo) are rounded to float32 once.  A pixel x has, in float32,
 *   u_k = R_0k x_0 + R_1k x_1 + R_2k x_2 (three fused multiply-adds, left to right),  ub = clamp(u_k, lo, hi) (NaN -> lo),
 *   pos = (ub - lo) * scale,  bin j = min(int(pos), bins - 1).
 * Counts are uint32 under integer atomics (LDS, then global memory): the same bits on every run.
 * The three entries refuse, before anything is launched: STROTSS_EINVAL for a null required pointer, h or w <= 0,
 * 3 h w > INT_MAX, bins outside 2..4096, n_bases outside 1..64, a basis that is not finite or not orthonormal to
 * max |R^T R - I| <= 1e-4, exactly one of next_basis / next_hist being NULL; STROTSS_EALIGN for a device pointer that is not
 * 16-byte aligned. */
/* the number of bases whose histograms one workgroup of strotss_color_hist holds in LDS: clamp(15360 / (3 bins), 1, 8),
 * 60 KiB of counters at the most (two workgroups per CU); 0 for bins outside 2..4096 */
int strotss_color_hist_group(int bins);
/* hist (n_bases, 3, bins) uint32 = the histograms of the counted pixels' projections on every axis of every basis, in ONE
 * kernel launch behind a memset of hist on the same stream (the call clears hist itself).  The image is read once per
 * group of strotss_color_hist_group(bins) bases. */
int strotss_color_hist(const float* img, const float* weight, int h, int w, const float* bases, int n_bases, int bins,
                       unsigned* hist, void* stream);
/* table (3, bins + 1) float32, one entry per bin edge of each axis, from the (3, bins) histograms of the source and of
 * the target on `basis`; one workgroup per axis, prefix sums in integers.  With S_j, C_i the exclusive cumulative counts
 * and N_s, N_c the totals (each <= INT_MAX / 3, so that the 64-bit products are exact): a = S_j N_c; i = the smallest
 * target bin with hist_dst[i] > 0 and C_{i+1} N_s >= a (a == 0: the first target bin that is not empty);
 * frac = double(a - C_i N_s) / double(hist_dst[i] N_s); table[j] = lo + (i + frac) (hi - lo) / bins in double with the
 * unrounded lo and hi, rounded to float32 once.  Non-decreasing.  Either histogram all zero: the identity
 * table[j] = lo + j (hi - lo) / bins.  Totals above INT_MAX / 3 give unspecified finite-or-not VALUES, never a division by
 * zero or an index out of range. */
int strotss_color_transfer_table(const unsigned* hist_src, const unsigned* hist_dst, const float* basis, int bins,
                                 float* table, void* stream);
/* For every counted pixel and axis k: ub, pos, j as above, f = pos - j, d_k = table_k[j] + f (table_k[j+1] - table_k[j]) - ub;
 * out_i = img_i + R_i0 d_0 + R_i1 d_1 + R_i2 d_2 (three fused multiply-adds, left to right), NOT clamped to [0, 1].  A pixel
 * that does not count is copied bit for bit.  out may equal img.  next_basis / next_hist (both or neither): the same launch
 * also bins the stored float32 values of the counted pixels on next_basis into next_hist (3, bins), which the call clears
 * (a memset on the same stream) -- bit for bit strotss_color_hist of out with the same weight plane on next_basis. */
int strotss_color_transfer_apply(const float* img, const float* weight, int h, int w, const float* basis, const float* table,
                                 int bins, float* out, const float* next_basis, unsigned* next_hist, void* stream);

/* ---------------------------------------------------------------------------------------
 * Photo smoothing: the guided filter of He, Sun and Tang (2013), the content as colour guide
 * --------------------------------------------------------------------------------------- */
#define STROTSS_SMOOTH_MAX_RADIUS 64
/* bytes of the workspace of strotss_guided_smooth: 216 per pixel (21 float64 planes of window sums + 12 float32 planes of
 * a, b); 0 for h, w <= 0, 3 h w > INT_MAX or a radius outside 1..STROTSS_SMOOTH_MAX_RADIUS */
size_t strotss_guided_smooth_workspace_bytes(int h, int w, int radius);
/* out = the guided filter of img with guide as colour guide, both (h, w, 3) float32.  The window of a pixel is the
 * (2 radius + 1)^2 box around it CLIPPED to the image and divided by its own pixel count (no padding).  Per window k:
 * mu = mean(I), Sigma = mean(I I^T) - mu mu^T + eps Id, and per channel c  a_c = Sigma^{-1} (mean(I p_c) - mu mean(p_c)),
 * b_c = mean(p_c) - a_c . mu;  out_c(i) = mean_i(a_c) . I(i) + mean_i(b_c), the means over the clipped window around i.
 * Window sums and the 3 x 3 solves in float64 (direct sums, a column pass and a row pass: no running sums), a and b stored
 * as float32, the output pixel in float32; NOT clamped.  eps is used at its float32 value.  No atomics: the same bits on
 * every run.  Four launches on `stream`; the workspace needs no initialisation and is the only scratch.  out may equal
 * img; it may not equal guide.
 * Refused before anything is launched: STROTSS_EINVAL for a null pointer, h or w <= 0, 3 h w > INT_MAX, a radius outside
 * 1..STROTSS_SMOOTH_MAX_RADIUS, eps not finite or outside [1e-4, 1], workspace_bytes below
 * strotss_guided_smooth_workspace_bytes(h, w, radius), out == guide; STROTSS_EALIGN for a pointer that is not 16-byte
 * aligned. */
int strotss_guided_smooth(const float* img, const float* guide, int h, int w, int radius, float eps, float* out,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Guided upsampling: the result at the content's own resolution, after He and Sun's fast guided filter
 * --------------------------------------------------------------------------------------- */
#define STROTSS_UPSAMPLE_GUIDED 0
#define STROTSS_UPSAMPLE_RESIDUAL 1
/* bytes of the workspace of strotss_guided_upsample: 280 per LOW-resolution pixel (the 216 of strotss_guided_smooth + one
 * 16-float record); 0 where strotss_guided_smooth_workspace_bytes is 0 */
size_t strotss_guided_upsample_workspace_bytes(int h, int w, int radius);
/* out (H, W, 3) = img (h, w, 3) brought to the size of guide_hi (H, W, 3), H >= h, W >= w; guide_lo (h, w, 3) is the same
 * guide at img's size.  The window means abar (3 x 3) and bbar (3) of strotss_guided_smooth(img, guide_lo) at (h, w),
 * rounded to float32 as there, and d = img - q with q that entry's output; up() is strotss_resize_bilinear from (h, w) to
 * (H, W) (half-pixel centres, clamped taps, along x then along y, a + (b - a) t with the difference rounded and one fused
 * multiply-add: a weight of 0 returns the sample).  Per pixel and channel c, in float32, not clamped:
 *   STROTSS_UPSAMPLE_GUIDED    out_c = fma(A_c2, I_2, fma(A_c1, I_1, fma(A_c0, I_0, B_c))), A = up(abar), B = up(bbar),
 *                              I = guide_hi: at H == h, W == w, guide_hi == guide_lo the bits of strotss_guided_smooth
 *   STROTSS_UPSAMPLE_RESIDUAL  that + up(d): the texture of img that the guide does not explain is kept
 * Five launches on `stream`, no atomics, the same bits on every run; the workspace needs no initialisation.
 * Refused before anything is launched: STROTSS_EINVAL for a null pointer, h, w, H or W <= 0, H < h, W < w,
 * 3 H W > INT_MAX, a radius outside 1..STROTSS_SMOOTH_MAX_RADIUS, eps not finite or outside [1e-4, 1], an unknown mode,
 * workspace_bytes below strotss_guided_upsample_workspace_bytes(h, w, radius), out overlapping guide_hi, guide_lo or img;
 * STROTSS_EALIGN for a pointer that is not 16-byte aligned. */
int strotss_guided_upsample(const float* img, const float* guide_lo, int h, int w, const float* guide_hi, int H, int W,
                            int radius, float eps, int mode, float* out, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ---------------------------------------------------------------------------------------
 * Region clustering: spherical k-means on sampled feature rows, the kernels of --auto_masks
 * --------------------------------------------------------------------------------------- */
#define STROTSS_KMEANS_MAX_K 16
/* x: a zero-padded (rows, ld) float32 feature matrix (strotss_hypercol_gather's layout, ld % 32 == 0), n rows of d columns
 * in use; inv_norm: strotss_row_inv_norm(x); centres: (k, ld) float32, every row of unit length or all zero (an empty
 * cluster), columns d..ld-1 zero; 1 <= k <= STROTSS_KMEANS_MAX_K.  Both entries refuse, before anything is launched and with
 * their outputs untouched: STROTSS_EINVAL for a null pointer, n <= 0, d <= 0, d > ld, n ld > INT_MAX, k outside
 * 1..STROTSS_KMEANS_MAX_K, a workspace below strotss_kmeans_update_workspace_bytes(n, ld, k); STROTSS_EALIGN for
 * ld % 32 != 0 or a pointer that is not 16-byte aligned. */
/* For every row i < n:  s_ij = (x_i . c_j) inv_norm_i, the dot product accumulated in float32 over the d columns;
 * label[i] (int32) = the j with the largest s_ij, the lowest j on equal values; best[i] = that value; second[i] = the largest
 * of the other k - 1 values (-inf for k == 1).  A row with inv_norm_i == 0 gets label 0 and best = second = 0.  One launch;
 * x is read once, the centres stay in LDS a 512-column chunk at a time.  The same bits on every run and stream. */
int strotss_kmeans_assign(const float* x, const float* inv_norm, int n, int d, int ld, const float* centres, int k, int* label,
                          float* best, float* second, void* stream);
/* bytes of the workspace of strotss_kmeans_update (the row blocks' float64 partial sums: at most 32 k ld doubles); 0 for
 * n <= 0, ld <= 0, ld % 32 != 0, n ld > INT_MAX or k outside 1..STROTSS_KMEANS_MAX_K */
size_t strotss_kmeans_update_workspace_bytes(int n, int ld, int k);
/* count[j] (int32) = the number of rows i < n with label[i] == j;  centres[j] = S_j / |S_j| with
 * S_j = sum_{label[i] == j} x_i inv_norm_i: the products (exact) and the sums in float64, in an order fixed by (n, d, k)
 * alone (rows ascending inside a row block, row blocks ascending, a fixed tree for the norm; no float atomics), the norm
 * and the division in float64, ONE rounding to float32 at the store; columns d..ld-1 are written as zero.  A cluster with
 * count[j] == 0 keeps its centre bit for bit; one whose S_j is all zero becomes the zero centre.  Labels outside 0..k-1
 * are skipped (counted nowhere, never used as an index).  Two launches; x is read once; the workspace needs no
 * initialisation.  The same bits on every run and stream. */
int strotss_kmeans_update(const float* x, const float* inv_norm, const int* label, int n, int d, int ld, int k, float* centres,
                          int* count, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Mask refinement: joint bilateral upsampling of a label grid, the kernels of --refine_masks
 * --------------------------------------------------------------------------------------- */
#define STROTSS_REFINE_MAX_RADIUS 4
/* bytes of the workspace of strotss_refine_labels (the (gh, gw, 3) float32 cell colours); 0 for h, w, gh or gw <= 0,
 * gh > h, gw > w or 3 h w > INT_MAX */
size_t strotss_refine_labels_workspace_bytes(int h, int w, int gh, int gw);
/* img: an (h, w, 3) float32 image; grid_label: its (gh, gw) int32 label grid over the labels 0..k-1, gh <= h, gw <= w,
 * 1 <= k <= STROTSS_KMEANS_MAX_K.  Cell (i, j) owns the pixels (y, x) with y gh / h == i and x gw / w == j (integer
 * division); m(i, j) is the mean of img over them, summed and divided in float64 in a fixed order and rounded once to
 * float32.  For every pixel, with u = (y + 0.5) gh / h - 0.5, v = (x + 0.5) gw / w - 0.5 and (i0, j0) its own cell, over the
 * cells |i - i0| <= radius, |j - j0| <= radius inside the grid (no padding), row by row, in float64:
 *   vote[l] = sum over the cells with label l of
 *             exp(-(((u - i)^2 + (v - j)^2) / (2 sigma_s^2) + |img(y, x) - m(i, j)|^2 / (2 sigma_r^2)))
 * label[y w + x] (int32) = the l with the largest vote among the labels that occur in the window, the lowest l on equal
 * votes; best / second (float64, each may be NULL) = that vote and the largest of the other occurring labels' votes
 * (-inf when only one occurs).  A cell whose label lies outside 0..k-1 casts no vote (compared, never used as an index);
 * a window without any label in 0..k-1 gives label 0 and best = second = -inf.  count[l] (int32, l < k) = the number of
 * pixels with label l, by integer atomics.  Two launches; the image is read once per launch; the workspace needs no
 * initialisation; no float atomics: the same bits on every run and stream.
 * Refused before anything is launched: STROTSS_EINVAL for a null img, grid_label, label, count or workspace, a size <= 0,
 * gh > h, gw > w, 3 h w > INT_MAX, k outside 1..STROTSS_KMEANS_MAX_K, a radius outside 1..STROTSS_REFINE_MAX_RADIUS, a sigma
 * that is not finite or not positive (or so small that 1 / (2 sigma^2) overflows), workspace_bytes below
 * strotss_refine_labels_workspace_bytes(h, w, gh, gw); STROTSS_EALIGN for a pointer that is not 16-byte aligned. */
int strotss_refine_labels(const float* img, int h, int w, const int* grid_label, int gh, int gw, int k, int radius,
                          double sigma_s, double sigma_r, int* label, double* best, double* second, int* count,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Region tracking: the regions of --auto_masks through a frame sequence, the kernels of --track_masks
 * --------------------------------------------------------------------------------------- */
/* The prior label of every cell of frame t's (gh, gw) label grid, from the grid of an earlier frame, in ONE launch.
 * prev_grid: (gh, gw) int32, the earlier frame's labels; flow: (h, w, 2) float32 = (dx, dy) per pixel, the backward flow of
 * frame t against the earlier frame as .flo files and strotss_flow_warp have it; certainty: (h, w) float32 or NULL (no
 * test); prior: (gh gw) int32; gh <= h, gw <= w, 1 <= k <= STROTSS_KMEANS_MAX_K.  Cell (i, j) owns the pixels (y, x) with
 * y gh / h == i and x gw / w == j (integer division, the convention of strotss_refine_labels).  Its probe pixel is
 * y_c = (y_lo + y_hi) / 2, x_c = (x_lo + x_hi) / 2, the integer mean of its first and last owned row and column; the source
 * pixel is sy = floor(y_c + dy + 0.5f), sx = floor(x_c + dx + 0.5f) with (dx, dy) = flow(y_c, x_c), two float32 additions each.
 *   prior(i, j) = prev_grid[sy gh / h, sx gw / w],
 * and -1 where a flow component is not finite, (sy, sx) lies outside the image, certainty(y_c, x_c) < 0.5 (an IEEE `<`: a NaN
 * removes nothing) or the label found lies outside 0..k-1 (compared, never used as an index).  No atomics: the same bits
 * on every run and stream.  Refused before anything is launched, prior untouched: STROTSS_EINVAL for a null prev_grid, flow
 * or prior, a size <= 0, gh > h, gw > w, 3 h w > INT_MAX, k outside 1..STROTSS_KMEANS_MAX_K; STROTSS_EALIGN for a pointer
 * that is not 16-byte aligned. */
int strotss_label_warp(const int* prev_grid, int gh, int gw, int k, const float* flow, const float* certainty, int h, int w,
                       int* prior, void* stream);
/* strotss_kmeans_assign with a bias toward a prior label.  x, inv_norm, n, d, ld, centres, k as there, and s_ij the same
 * bits as there (one kernel source); prior: (n) int32; 0 <= beta <= 2.
 *   score_ij = s_ij + (prior_i == j ? beta : 0), ONE float32 addition; a prior outside 0..k-1 adds nothing and is never used
 *   as an index;  label[i] = the j with the largest score, the lowest j on equal scores;  best[i] = the raw s of that j;
 *   second[i] = the largest raw s of the other j (-inf for k == 1; it may exceed best).
 * A row with inv_norm_i == 0 has every s = 0: it takes its prior when that is valid and beta > 0, else label 0, and
 * best = second = 0.  With beta == 0, or without a valid prior, label, best and second are strotss_kmeans_assign's bit for
 * bit.  Cosines lie in [-1, 1], so beta == 2 never changes a label that has a prior.  One launch; x is read once, the centres
 * stay in LDS a 512-column chunk at a time; no atomics: the same bits on every run and stream.  Refused before anything is
 * launched, the outputs untouched: STROTSS_EINVAL for a null pointer, n <= 0, d <= 0, d > ld, n ld > INT_MAX, k outside
 * 1..STROTSS_KMEANS_MAX_K, a beta that is not finite or outside [0, 2]; STROTSS_EALIGN for ld % 32 != 0 or a pointer that
 * is not 16-byte aligned. */
int strotss_kmeans_assign_prior(const float* x, const float* inv_norm, int n, int d, int ld, const float* centres, int k,
                                const int* prior, float beta, int* label, float* best, float* second, void* stream);

/* ---------------------------------------------------------------------------------------
 * Scribble masks: region labels from a few strokes per image, the kernels of --content_scribbles /
 * --style_scribbles
 * --------------------------------------------------------------------------------------- */
#define STROTSS_SCRIBBLE_MAX_K 7
#define STROTSS_SCRIBBLE_MAX_ITERS 1024
/* scores[i k + j] (float32, (n, k)) = s_ij of strotss_kmeans_assign for every row i < n and centre j < k, the same bits (one
 * kernel source); x, inv_norm, n, d, ld, centres, k as there.  A row with inv_norm_i == 0 gets k zeros.  One launch; the same
 * bits on every run and stream.  Refused before anything is launched, scores untouched: STROTSS_EINVAL for a null pointer,
 * n <= 0, d <= 0, d > ld, n ld > INT_MAX, n k > INT_MAX, k outside 1..STROTSS_KMEANS_MAX_K; STROTSS_EALIGN for ld % 32 != 0 or
 * a pointer that is not 16-byte aligned. */
int strotss_kmeans_scores(const float* x, const float* inv_norm, int n, int d, int ld, const float* centres, int k,
                          float* scores, void* stream);
/* bytes of the workspace of strotss_scribble_labels: 3 k + 2 float32 planes of h w values (the unary q, two buffers of x, the
 * two edge weights), each in 256-byte slices; 0 for h or w <= 0, k outside 2..STROTSS_SCRIBBLE_MAX_K, k h w > INT_MAX or
 * 3 h w > INT_MAX */
size_t strotss_scribble_workspace_bytes(int h, int w, int k);
/* img: an (h, w, 3) float32 image; stroke: (h, w) int32, a label 0..k-1 on a stroke pixel and any other value elsewhere
 * (compared, never used as an index); scores: the (gh, gw, k) float32 scores of the cells of the image's feature grid
 * (strotss_kmeans_scores), 2 <= k <= STROTSS_SCRIBBLE_MAX_K.
 *   unary    s_r(y, x) = scores plane r sampled bilinearly at u = (y + 0.5) gh / h - 0.5, v = (x + 0.5) gw / w - 0.5 (the
 *            4-neighbour, edge-clamped rule of strotss_flow_warp);  q_r = softmax_r(s_r / tau), the maximum subtracted first;
 *            all of it in float64, q rounded once to float32
 *   weights  w(p, p') = exp(-|img(p) - img(p')|^2 / (2 sigma^2)) for the 4 neighbours inside the image (float64, rounded
 *            once); a neighbour outside the image is omitted
 *   sweeps   x^0 = q; on a stroke pixel x is the one-hot of its label, before and after every sweep; every other pixel, in
 *            each of `iters` Jacobi sweeps (float32):  x_r(p) <- (lambda q_r(p) + sum w x_r(p')) / (lambda + sum w), evaluated as
 *            q_r(p) + sum w (x_r(p') - q_r(p)) / (lambda + sum w) and clamped to [0, 1]
 *   labels   label[y w + x] (int32) = the r with the largest x_r, the lowest r on equal values; count[r] (int32, r < k) = the
 *            number of pixels with label r, by integer atomics; x (k, h, w) float32 or NULL = the planes after the last sweep
 * iters_per_launch: 1 = one sweep per launch; 2, 4 or 8 = that many sweeps per launch of the blocked kernel (sweeps that do
 * not fill a launch run one by one); 0 = the library's choice.  Every choice gives the same bits.  No float atomics: the
 * same bits on every run and stream.  The workspace needs no initialisation.
 * Refused before anything is launched, the outputs untouched: STROTSS_EINVAL for a null img, stroke, scores, label, count or
 * workspace, a size <= 0, k outside 2..STROTSS_SCRIBBLE_MAX_K, k h w, 3 h w or gh gw k > INT_MAX, a tau, lambda or sigma that
 * is not finite or not positive (or so small that its reciprocal overflows, or a lambda that is 0 as float32), iters outside
 * 1..STROTSS_SCRIBBLE_MAX_ITERS, iters_per_launch not in {0, 1, 2, 4, 8}, workspace_bytes below
 * strotss_scribble_workspace_bytes(h, w, k); STROTSS_EALIGN for a pointer that is not 16-byte aligned. */
int strotss_scribble_labels(const float* img, const int* stroke, int h, int w, const float* scores, int gh, int gw, int k,
                            double tau, double lambda, double sigma, int iters, int iters_per_launch, int* label, int* count,
                            float* x, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Detail map (--sample_map auto): where an image has local structure
 * --------------------------------------------------------------------------------------- */
/* bytes of the workspace of strotss_detail_map: 32 + 8 per workgroup of its row pass + 8 per pixel (one float64 plane of
 * column sums); 0 for h, w <= 0 or 3 h w > INT_MAX */
size_t strotss_detail_map_workspace_bytes(int h, int w);
/* out (h, w) = the detail map of img (h, w, 3), float32 RGB in [0, 1]:
 *   Y = 0.299 R + 0.587 G + 0.114 B                                        (the grey of strotss_flow)
 *   e = gx^2 + gy^2,  gx = (Y(y, x+1) - Y(y, x-1)) / 2, gy likewise, indices clamped to the image (a 1-pixel axis gives 0)
 *   s(p) = sqrt(mean of e over the window [y-r, y+r] x [x-r, x+r] clipped to the image), the divisor the count of pixels
 *          inside the clipped window; the window sums in float64, a column pass and a row pass of direct sums
 *   m = mean of s over the image, in float64, a fixed-order reduction (no float atomics)
 *   out(p) = floor + (1 - floor) * min(1, s(p) / (gain * m));  m == 0 (a constant image): out = 1 everywhere, and where
 *            the minimum is 1 out is 1 itself.
 * Y, e, the mean's division, the root and the last line are float32 operations, each rounded on its own (no contraction).
 * Three launches on `stream`; the same bits on every run.  The workspace is 16-byte aligned and zero before its first use
 * (one call at a time; a call leaves it ready for the next).  Refused before anything is launched: STROTSS_EINVAL for a
 * null pointer, h or w <= 0, 3 h w > INT_MAX; STROTSS_ERANGE for a radius outside 1..64, a gain that is not finite or
 * <= 0, a floor that is not finite or outside [0, 1]; STROTSS_EALIGN for a pointer that is not 16-byte aligned. */
int strotss_detail_map(const float* img, int h, int w, int radius, float gain, float floor, float* out, void* workspace,
                       void* stream);

/* ---------------------------------------------------------------------------------------
 * Optimiser + output
 * --------------------------------------------------------------------------------------- */
typedef struct {
  int n_tensors;
  float* var[STROTSS_MAX_TENSORS];
  float* rms[STROTSS_MAX_TENSORS];
  const float* grad[STROTSS_MAX_TENSORS];
  int64_t numel[STROTSS_MAX_TENSORS];
} strotss_tensors_t;
/* Keras RMSprop (momentum 0, not centred), run_strotss.py:63,148, all tensors in ONE launch:
 *   rms = rho*rms + (1-rho)*g*g ;  var -= lr * g / (sqrt(rms) + eps) */
int strotss_rmsprop_step(const strotss_tensors_t* t, float lr, float rho, float eps, void* stream);
/* postprocess (strotss_utils.py:170-175): clip[0,1], -min, /max, *255, truncate to uint8.
 * workspace: >= 2*1024 floats. */
int strotss_postprocess(const float* img, int64_t numel, uint8_t* out, float* workspace,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STROTSS_HIP_H */
