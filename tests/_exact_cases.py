"""Convolution and distance-GEMM cases whose float64 result is the bit-exact float32 answer of every route, and the
conditions that make that so.  A plain module (not a conftest): tests/test_exact_cases_cpu.py checks the conditions and
float32 stand-ins of every pipeline on the CPU, tests/test_hip_exact_conv.py runs the kernels.

Integer family (every route, both directions).  The transformed input `a` (the activation, or the output gradient of a
data-gradient) holds small integers, about half of them zero; the kernel is g = 576 k with small sparse integers k; bias and
the accumulate base are integers.  The Winograd matrices are Lavin & Gray's: B^T and A^T are integer, G has 1/4, 1/6, 1/12,
1/24, so U = G g G^T = (24 G) k (24 G)^T is an integer, V = B^T d B is an integer, and so is every product and partial sum.
While all of them stay below 2^24 float32 arithmetic is exact in any order, fused or not, on the f32 MFMA and on the
six-product bf16x3 core (which keeps hh, hm, mh, hl, mm, lh: exact when both operands have at most 16 significant bits).
Conditions, computed from the reference data alone in float64 (`winograd_conditions`, `direct_conditions`):
  1. U read back from the library equals the exact (24 G) k (24 G)^T               (GPU file; the CPU file restates the kernel)
  2. max |V| < 2^24
  3. max over (position, tile, output channel) of sum_c |U| |V| < 2^24; on the bf16x3 routes with |x| replaced by
     |h| + |m| + |l| of split3, which bounds every partial sum of the six plane products
  4. max sum |A^T| |M| |A| + max |bias| + max |base| < 2^24
  5. every U and V has at most 16 significant bits
  6. direct routes: max sum over the 9 K terms of |a| |g| + max |bias| + max |base| < 2^24
  7. at least FLOOR of the outputs strictly positive and at least FLOOR strictly negative before the ReLU / the mask.

Wide family (the bf16x3 routes only).  One operand carries 9 .. 18 significant bits so that the m and l planes of split3 are
used; K is sparse (1 .. 3 non-zero input channels per output channel) so that M is still exact (condition 3).  The output
transform of such an M rounds, so the comparison is element by element under WINO4_OUT_ROUNDINGS u (sum |A^T| |M| |A| +
|bias|), u = 2^-24.  The count follows winograd43_out_kernel's operation sequence: a column sum s[i][q] is at most five
terms (row 3: m1 - m2 + 8 m3 - 8 m4 + m5; the factors are powers of two) = 4 additions, an output is at most five such s
plus the bias = 5 additions, each addition rounds once whether or not it is contracted with its factor: 4 + 5 = 9.

Distance GEMM (strotss_cosine_distance_x3 with unit norms): integer rows with sum |x|_3 |y|_3 < 2^24, C = 1 - x.y exact."""
import zlib

import numpy as np
import torch

import _route_cases as RC
from _conv_ref import conv64, sign_words          # (shared with the float64 route tests)

LIMIT = 2.0 ** 24
U_RND = 2.0 ** -24
FLOOR = 0.2                    # condition 7: share of strictly positive and of strictly negative reference outputs
WINO4_OUT_ROUNDINGS = 9        # derived above
GAMMA9 = WINO4_OUT_ROUNDINGS * U_RND / (1 - WINO4_OUT_ROUNDINGS * U_RND)
WIDE_M_HEADROOM = 0.9          # wide family: condition 3 with the split3 planes' magnitudes must stay below this of 2^24

BT4 = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
       [0, 4, 0, -5, 0, 1]]
AT4 = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]
G4_24 = [[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]]          # 24 G
BT2 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
AT2 = [[1, 1, 1, 0], [0, 1, -1, -1]]
G2_24 = [[24, 0, 0], [12, 12, 12], [12, -12, 12], [0, 0, 24]]
MATS = {4: (BT4, AT4, G4_24), 2: (BT2, AT2, G2_24)}

IMAGES = ((683, 1024), (1024, 683), (1024, 1024))


def scale_sizes(h, w):
    """The sizes an h x w image takes through the schedule: long side 64, 128, ... 1024."""
    long = max(h, w)
    return [(h * s // long, w * s // long) for s in (64, 128, 256, 512, 1024)]


def schedule_layers():
    """(h, w, cin, cout) of every generic layer at every scale of IMAGES."""
    M = RC._model()
    out = []
    for ih, iw in IMAGES:
        for h, w in scale_sizes(ih, iw):
            for it in M.vgg_config("16"):
                if it == "pool":
                    h, w = h // 2, w // 2
                    continue
                _, cin, cout = it
                if cin != 3 and (h, w, cin, cout) not in out:
                    out.append((h, w, cin, cout))
    return out


def class_key(case):
    """Cases with one key run the same code on the same tile-remainder pattern: route, direction, channels, h % 4, w % 4,
    whether h * w fills whole 64-pixel tiles (direct kernels), and for the fused kernel whether its work items (16 x 32 pixels
    x 32 output channels) exceed the 256 workgroups and whether they split evenly over the 8 XCDs."""
    route, direction, h, w, cin, cout = case
    n_out = cin if direction == "dgrad" else cout
    items = -(-h // 16) * -(-w // 32) * (n_out // 32)
    fused = (items > 256, items % 8 != 0) if route == "F4_fused_f32" else ()
    return (route, direction, cin, cout, h % 4, w % 4, (h * w) % 64 == 0, fused)


def dedup(cases):
    """One case per class_key: the one with the most pixels (the first of those in list order)."""
    best = {}
    for c in cases:
        k = class_key(c)
        if k not in best or c[2] * c[3] > best[k][2] * best[k][3]:
            best[k] = c
    return sorted(best.values(), key=lambda c: (RC.ROUTES.index(c[0]), c[1], c[2] * c[3], c[2], c[4], c[5]))


def enumerate_default_cases():
    """The schedule's layers, both directions, labelled by the policy of this process, plus _route_cases' ragged shapes."""
    cases = []
    for h, w, cin, cout in schedule_layers():
        for direction in ("fwd", "dgrad"):
            cases.append((RC.route_of((None, direction, h, w, cin, cout)), direction, h, w, cin, cout))
    return dedup(cases + list(RC.DEFAULT_CASES))


# enumerate_default_cases() under the default policy, written out so that a policy change fails
# test_exact_cases_cpu.py::test_case_list_is_the_schedule_under_the_default_policy instead of silently moving the cases
DEFAULT_CASES = [
    ('direct', 'dgrad', 31, 41, 512, 128),
    ('direct', 'dgrad', 21, 64, 512, 64),
    ('direct', 'dgrad', 85, 128, 64, 64),
    ('direct', 'dgrad', 128, 85, 64, 64),
    ('direct', 'dgrad', 128, 128, 64, 64),
    ('direct', 'fwd', 85, 128, 64, 64),
    ('direct', 'fwd', 128, 85, 64, 64),
    ('direct', 'fwd', 128, 128, 64, 64),
    ('direct_splitk', 'dgrad', 4, 4, 512, 512),
    ('direct_splitk', 'dgrad', 5, 8, 256, 512),
    ('direct_splitk', 'dgrad', 5, 8, 512, 512),
    ('direct_splitk', 'dgrad', 8, 5, 256, 512),
    ('direct_splitk', 'dgrad', 8, 5, 512, 512),
    ('direct_splitk', 'dgrad', 10, 16, 128, 256),
    ('direct_splitk', 'dgrad', 10, 16, 256, 256),
    ('direct_splitk', 'dgrad', 10, 16, 256, 512),
    ('direct_splitk', 'dgrad', 10, 16, 512, 512),
    ('direct_splitk', 'dgrad', 16, 10, 128, 256),
    ('direct_splitk', 'dgrad', 16, 10, 256, 256),
    ('direct_splitk', 'dgrad', 16, 10, 256, 512),
    ('direct_splitk', 'dgrad', 16, 10, 512, 512),
    ('direct_splitk', 'dgrad', 13, 17, 256, 256),
    ('direct_splitk', 'dgrad', 16, 16, 256, 512),
    ('direct_splitk', 'dgrad', 16, 16, 512, 512),
    ('direct_splitk', 'dgrad', 33, 20, 64, 64),
    ('direct_splitk', 'dgrad', 21, 32, 64, 128),
    ('direct_splitk', 'dgrad', 21, 32, 128, 128),
    ('direct_splitk', 'dgrad', 21, 32, 128, 256),
    ('direct_splitk', 'dgrad', 21, 32, 256, 256),
    ('direct_splitk', 'dgrad', 32, 21, 64, 128),
    ('direct_splitk', 'dgrad', 32, 21, 128, 128),
    ('direct_splitk', 'dgrad', 32, 21, 128, 256),
    ('direct_splitk', 'dgrad', 32, 21, 256, 256),
    ('direct_splitk', 'dgrad', 32, 32, 128, 256),
    ('direct_splitk', 'dgrad', 32, 32, 256, 256),
    ('direct_splitk', 'dgrad', 42, 64, 64, 64),
    ('direct_splitk', 'dgrad', 42, 64, 64, 128),
    ('direct_splitk', 'dgrad', 42, 64, 128, 128),
    ('direct_splitk', 'dgrad', 64, 42, 64, 64),
    ('direct_splitk', 'dgrad', 64, 42, 64, 128),
    ('direct_splitk', 'dgrad', 64, 42, 128, 128),
    ('direct_splitk', 'dgrad', 64, 64, 64, 64),
    ('direct_splitk', 'dgrad', 64, 64, 64, 128),
    ('direct_splitk', 'dgrad', 64, 64, 128, 128),
    ('direct_splitk', 'fwd', 4, 4, 512, 512),
    ('direct_splitk', 'fwd', 5, 8, 256, 512),
    ('direct_splitk', 'fwd', 5, 8, 512, 512),
    ('direct_splitk', 'fwd', 8, 5, 256, 512),
    ('direct_splitk', 'fwd', 8, 5, 512, 512),
    ('direct_splitk', 'fwd', 10, 16, 128, 256),
    ('direct_splitk', 'fwd', 10, 16, 256, 256),
    ('direct_splitk', 'fwd', 10, 16, 256, 512),
    ('direct_splitk', 'fwd', 10, 16, 512, 512),
    ('direct_splitk', 'fwd', 16, 10, 128, 256),
    ('direct_splitk', 'fwd', 16, 10, 256, 256),
    ('direct_splitk', 'fwd', 16, 10, 256, 512),
    ('direct_splitk', 'fwd', 16, 10, 512, 512),
    ('direct_splitk', 'fwd', 13, 17, 256, 256),
    ('direct_splitk', 'fwd', 16, 16, 256, 512),
    ('direct_splitk', 'fwd', 16, 16, 512, 512),
    ('direct_splitk', 'fwd', 33, 20, 64, 64),
    ('direct_splitk', 'fwd', 21, 32, 64, 128),
    ('direct_splitk', 'fwd', 21, 32, 128, 128),
    ('direct_splitk', 'fwd', 21, 32, 128, 256),
    ('direct_splitk', 'fwd', 21, 32, 256, 256),
    ('direct_splitk', 'fwd', 32, 21, 64, 128),
    ('direct_splitk', 'fwd', 32, 21, 128, 128),
    ('direct_splitk', 'fwd', 32, 21, 128, 256),
    ('direct_splitk', 'fwd', 32, 21, 256, 256),
    ('direct_splitk', 'fwd', 32, 32, 128, 256),
    ('direct_splitk', 'fwd', 32, 32, 256, 256),
    ('direct_splitk', 'fwd', 42, 64, 64, 64),
    ('direct_splitk', 'fwd', 42, 64, 64, 128),
    ('direct_splitk', 'fwd', 42, 64, 128, 128),
    ('direct_splitk', 'fwd', 64, 42, 64, 64),
    ('direct_splitk', 'fwd', 64, 42, 64, 128),
    ('direct_splitk', 'fwd', 64, 42, 128, 128),
    ('direct_splitk', 'fwd', 64, 64, 64, 64),
    ('direct_splitk', 'fwd', 64, 64, 64, 128),
    ('direct_splitk', 'fwd', 64, 64, 128, 128),
    ('F2_gemm_f32', 'dgrad', 23, 29, 256, 512),
    ('F2_gemm_f32', 'dgrad', 21, 32, 256, 512),
    ('F2_gemm_f32', 'dgrad', 21, 32, 512, 512),
    ('F2_gemm_f32', 'dgrad', 32, 21, 256, 512),
    ('F2_gemm_f32', 'dgrad', 32, 21, 512, 512),
    ('F2_gemm_f32', 'dgrad', 21, 33, 512, 512),
    ('F2_gemm_f32', 'fwd', 23, 29, 256, 512),
    ('F2_gemm_f32', 'fwd', 21, 32, 256, 512),
    ('F2_gemm_f32', 'fwd', 21, 32, 512, 512),
    ('F2_gemm_f32', 'fwd', 32, 21, 256, 512),
    ('F2_gemm_f32', 'fwd', 32, 21, 512, 512),
    ('F2_gemm_f32', 'fwd', 21, 33, 512, 512),
    ('F4_fused_f32', 'dgrad', 85, 128, 256, 256),
    ('F4_fused_f32', 'dgrad', 85, 128, 256, 512),
    ('F4_fused_f32', 'dgrad', 128, 85, 256, 256),
    ('F4_fused_f32', 'dgrad', 128, 85, 256, 512),
    ('F4_fused_f32', 'dgrad', 128, 128, 128, 128),
    ('F4_fused_f32', 'dgrad', 128, 128, 128, 256),
    ('F4_fused_f32', 'dgrad', 128, 128, 256, 256),
    ('F4_fused_f32', 'dgrad', 128, 128, 256, 512),
    ('F4_fused_f32', 'dgrad', 170, 256, 64, 64),
    ('F4_fused_f32', 'dgrad', 170, 256, 64, 128),
    ('F4_fused_f32', 'dgrad', 170, 256, 128, 128),
    ('F4_fused_f32', 'dgrad', 170, 256, 128, 256),
    ('F4_fused_f32', 'dgrad', 256, 170, 64, 64),
    ('F4_fused_f32', 'dgrad', 256, 170, 64, 128),
    ('F4_fused_f32', 'dgrad', 256, 170, 128, 128),
    ('F4_fused_f32', 'dgrad', 256, 170, 128, 256),
    ('F4_fused_f32', 'dgrad', 171, 259, 128, 128),
    ('F4_fused_f32', 'dgrad', 256, 256, 64, 64),
    ('F4_fused_f32', 'dgrad', 256, 256, 64, 128),
    ('F4_fused_f32', 'dgrad', 256, 256, 128, 256),
    ('F4_fused_f32', 'dgrad', 170, 520, 64, 64),
    ('F4_fused_f32', 'dgrad', 341, 512, 64, 64),
    ('F4_fused_f32', 'dgrad', 341, 512, 64, 128),
    ('F4_fused_f32', 'dgrad', 341, 512, 128, 128),
    ('F4_fused_f32', 'dgrad', 512, 341, 64, 64),
    ('F4_fused_f32', 'dgrad', 512, 341, 64, 128),
    ('F4_fused_f32', 'dgrad', 512, 341, 128, 128),
    ('F4_fused_f32', 'dgrad', 512, 512, 64, 128),
    ('F4_fused_f32', 'dgrad', 512, 512, 128, 128),
    ('F4_fused_f32', 'dgrad', 683, 1024, 64, 64),
    ('F4_fused_f32', 'dgrad', 1024, 683, 64, 64),
    ('F4_fused_f32', 'dgrad', 1024, 1024, 64, 64),
    ('F4_fused_f32', 'fwd', 85, 128, 128, 256),
    ('F4_fused_f32', 'fwd', 85, 128, 256, 256),
    ('F4_fused_f32', 'fwd', 128, 85, 128, 256),
    ('F4_fused_f32', 'fwd', 128, 85, 256, 256),
    ('F4_fused_f32', 'fwd', 128, 128, 64, 128),
    ('F4_fused_f32', 'fwd', 128, 128, 128, 128),
    ('F4_fused_f32', 'fwd', 128, 128, 128, 256),
    ('F4_fused_f32', 'fwd', 128, 128, 256, 256),
    ('F4_fused_f32', 'fwd', 170, 256, 64, 64),
    ('F4_fused_f32', 'fwd', 170, 256, 64, 128),
    ('F4_fused_f32', 'fwd', 170, 256, 128, 128),
    ('F4_fused_f32', 'fwd', 256, 170, 64, 64),
    ('F4_fused_f32', 'fwd', 256, 170, 64, 128),
    ('F4_fused_f32', 'fwd', 256, 170, 128, 128),
    ('F4_fused_f32', 'fwd', 171, 259, 64, 128),
    ('F4_fused_f32', 'fwd', 256, 256, 64, 64),
    ('F4_fused_f32', 'fwd', 170, 520, 64, 64),
    ('F4_fused_f32', 'fwd', 341, 512, 64, 64),
    ('F4_fused_f32', 'fwd', 341, 512, 64, 128),
    ('F4_fused_f32', 'fwd', 341, 512, 128, 128),
    ('F4_fused_f32', 'fwd', 512, 341, 64, 64),
    ('F4_fused_f32', 'fwd', 512, 341, 64, 128),
    ('F4_fused_f32', 'fwd', 512, 341, 128, 128),
    ('F4_fused_f32', 'fwd', 512, 512, 64, 128),
    ('F4_fused_f32', 'fwd', 512, 512, 128, 128),
    ('F4_fused_f32', 'fwd', 683, 1024, 64, 64),
    ('F4_fused_f32', 'fwd', 1024, 683, 64, 64),
    ('F4_fused_f32', 'fwd', 1024, 1024, 64, 64),
    ('F4_gemm_f32', 'dgrad', 32, 32, 512, 512),
    ('F4_gemm_f32', 'dgrad', 43, 61, 256, 512),
    ('F4_gemm_f32', 'dgrad', 41, 65, 256, 512),
    ('F4_gemm_f32', 'dgrad', 42, 64, 128, 256),
    ('F4_gemm_f32', 'dgrad', 42, 64, 256, 256),
    ('F4_gemm_f32', 'dgrad', 42, 64, 256, 512),
    ('F4_gemm_f32', 'dgrad', 42, 64, 512, 512),
    ('F4_gemm_f32', 'dgrad', 64, 42, 128, 256),
    ('F4_gemm_f32', 'dgrad', 64, 42, 256, 256),
    ('F4_gemm_f32', 'dgrad', 64, 42, 256, 512),
    ('F4_gemm_f32', 'dgrad', 64, 42, 512, 512),
    ('F4_gemm_f32', 'dgrad', 64, 64, 128, 256),
    ('F4_gemm_f32', 'dgrad', 64, 64, 256, 256),
    ('F4_gemm_f32', 'dgrad', 64, 64, 256, 512),
    ('F4_gemm_f32', 'dgrad', 85, 128, 64, 128),
    ('F4_gemm_f32', 'dgrad', 85, 128, 128, 128),
    ('F4_gemm_f32', 'dgrad', 85, 128, 128, 256),
    ('F4_gemm_f32', 'dgrad', 128, 85, 64, 128),
    ('F4_gemm_f32', 'dgrad', 128, 85, 128, 128),
    ('F4_gemm_f32', 'dgrad', 128, 85, 128, 256),
    ('F4_gemm_f32', 'dgrad', 128, 128, 64, 128),
    ('F4_gemm_f32', 'fwd', 32, 32, 256, 512),
    ('F4_gemm_f32', 'fwd', 32, 32, 512, 512),
    ('F4_gemm_f32', 'fwd', 43, 61, 256, 512),
    ('F4_gemm_f32', 'fwd', 41, 65, 256, 512),
    ('F4_gemm_f32', 'fwd', 42, 64, 128, 256),
    ('F4_gemm_f32', 'fwd', 42, 64, 256, 256),
    ('F4_gemm_f32', 'fwd', 42, 64, 256, 512),
    ('F4_gemm_f32', 'fwd', 42, 64, 512, 512),
    ('F4_gemm_f32', 'fwd', 64, 42, 128, 256),
    ('F4_gemm_f32', 'fwd', 64, 42, 256, 256),
    ('F4_gemm_f32', 'fwd', 64, 42, 256, 512),
    ('F4_gemm_f32', 'fwd', 64, 42, 512, 512),
    ('F4_gemm_f32', 'fwd', 64, 64, 128, 256),
    ('F4_gemm_f32', 'fwd', 64, 64, 256, 256),
    ('F4_gemm_f32', 'fwd', 85, 128, 64, 128),
    ('F4_gemm_f32', 'fwd', 85, 128, 128, 128),
    ('F4_gemm_f32', 'fwd', 128, 85, 64, 128),
    ('F4_gemm_f32', 'fwd', 128, 85, 128, 128),
    ('F4_x3_gemm_128', 'dgrad', 128, 128, 512, 512),
    ('F4_x3_gemm_128', 'dgrad', 170, 255, 256, 256),
    ('F4_x3_gemm_128', 'dgrad', 169, 257, 256, 256),
    ('F4_x3_gemm_128', 'dgrad', 170, 256, 256, 256),
    ('F4_x3_gemm_128', 'dgrad', 256, 170, 256, 256),
    ('F4_x3_gemm_128', 'dgrad', 256, 256, 256, 256),
    ('F4_x3_gemm_128', 'fwd', 128, 128, 256, 512),
    ('F4_x3_gemm_128', 'fwd', 128, 128, 512, 512),
    ('F4_x3_gemm_128', 'fwd', 170, 255, 256, 256),
    ('F4_x3_gemm_128', 'fwd', 169, 257, 256, 256),
    ('F4_x3_gemm_128', 'fwd', 170, 256, 128, 256),
    ('F4_x3_gemm_128', 'fwd', 170, 256, 256, 256),
    ('F4_x3_gemm_128', 'fwd', 256, 170, 128, 256),
    ('F4_x3_gemm_128', 'fwd', 256, 170, 256, 256),
    ('F4_x3_gemm_128', 'fwd', 256, 256, 128, 256),
    ('F4_x3_gemm_128', 'fwd', 256, 256, 256, 256),
    ('F4_x3_gemm_64', 'dgrad', 61, 67, 512, 512),
    ('F4_x3_gemm_64', 'dgrad', 64, 64, 512, 512),
    ('F4_x3_gemm_64', 'dgrad', 65, 65, 512, 512),
    ('F4_x3_gemm_64', 'dgrad', 85, 128, 512, 512),
    ('F4_x3_gemm_64', 'dgrad', 128, 85, 512, 512),
    ('F4_x3_gemm_64', 'fwd', 61, 67, 512, 512),
    ('F4_x3_gemm_64', 'fwd', 64, 64, 256, 512),
    ('F4_x3_gemm_64', 'fwd', 64, 64, 512, 512),
    ('F4_x3_gemm_64', 'fwd', 65, 65, 512, 512),
    ('F4_x3_gemm_64', 'fwd', 85, 128, 256, 512),
    ('F4_x3_gemm_64', 'fwd', 85, 128, 512, 512),
    ('F4_x3_gemm_64', 'fwd', 128, 85, 256, 512),
    ('F4_x3_gemm_64', 'fwd', 128, 85, 512, 512),
]

SWITCH_CASES = RC.SWITCH_CASES

# the bf16x3 routes' shapes for the wide family: (group or None, route, h, w, cin, cout)
WIDE_SHAPES = [
    (None, "F4_x3_gemm_128", 170, 256, 256, 256),
    (None, "F4_x3_gemm_128", 170, 255, 256, 256),
    (None, "F4_x3_gemm_64", 85, 128, 512, 512),
    (None, "F4_x3_gemm_64", 61, 67, 512, 512),
    ("x3_64_channels", "F4_x3_gemm_64", 64, 64, 64, 64),
    ("x3_64_channels", "F4_x3_gemm_64", 42, 64, 64, 64),
]
WIDE_KINDS = ("v12", "v17", "u17")
# floors on the share of non-zero products U V whose wide factor has a non-zero m / l plane.  v12: V = B^T d B of 8-bit
# pixels has up to 15 bits and mostly more than 8 (m != 0), hardly ever more than 16 (l == 0).  v17: 12-bit pixels give V of
# 14 .. 19 bits; more than 16 significant bits needs |V| >= 2^16 and set low bits, which the four positions with the largest
# B^T rows reach in a few per cent of their tiles (split3 rounds to nearest, so l != 0 needs a residual of more than 8 bits
# below the 8 of h: |V| >= 2^17).  u17: every U has more than 8 bits.  An l plane of U is out of reach while M stays exact: the
# wide entries of U = k v x v carry the factors 4 .. 36 of v x v as trailing zeros or sit next to an entry 16 .. 36 times
# larger, whose product with |V| <= 50 passes 2^24; the B operand's l plane is exercised by the distance GEMM's y_wide rows.
WIDE_FLOORS = {"v12": (0.5, 0.0), "v17": (0.8, 0.005), "u17": (0.5, 0.0)}


def case_id(case):
    return RC.case_id(case)


def wide_id(shape, direction, kind):
    return f"wide-{kind}-{shape[1]}-{direction}-{shape[2]}x{shape[3]}x{shape[4]}to{shape[5]}"


def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def _relu_ints(g, shape, vmax, signed=False):
    """Integers 0 .. vmax (signed: -vmax .. vmax) with about half of them zero, as float32."""
    v = torch.randint(1, vmax + 1, shape, generator=g, dtype=torch.int16)
    keep = torch.rand(shape, generator=g) < 0.5
    if signed:
        v = torch.where(torch.rand(shape, generator=g) < 0.5, -v, v)
    return (v * keep).float()


def int_params(route, K):
    """(largest |a|, density of non-zero k over (tap, input channel)) of the integer family per reduction width K.  The
    output transform's condition 4 binds (its |A^T| rows sum to 19): denser or larger data leaves it at large K."""
    if route.startswith("direct"):
        return 3, 0.5              # worst case 9 * 512 * 3 * 576 = 7.96e6 < 2^24 whatever the data
    return {64: (3, 0.5), 128: (3, 0.25), 256: (2, 0.25), 512: (2, 0.125)}[K]


class Problem:
    """One layer problem in the kernel's terms: out (h, w, N) = conv3x3(a (h, w, K), 576 k_eff (3, 3, K, N)) [+ bias].
    fwd: a = x, K = cin, N = cout, wt = 576 k_eff.  dgrad: a = gy, K = cout, N = cin and the layer's HWIO kernel is
    wt = 576 k_eff.flip(0, 1).transpose(2, 3); x is the layer's input activation (the mask), pre the accumulate base."""

    def __init__(self, ident, route, direction, h, w, cin, cout):
        self.id, self.route, self.direction, self.h, self.w, self.cin, self.cout = ident, route, direction, h, w, cin, cout
        self.K, self.N = (cin, cout) if direction == "fwd" else (cout, cin)
        self.tile = 0 if route.startswith("direct") else 2 if route == "F2_gemm_f32" else 4
        self.x3 = "x3" in route
        self.bias = None

    @property
    def wt(self):
        g = 576.0 * self.k_eff
        return g if self.direction == "fwd" else g.flip(0, 1).transpose(2, 3).contiguous()

    def mask_input(self):
        """dgrad: the layer's input activation x (1, h, w, cin), ReLU-like integers; made on demand (it is only a mask)."""
        return _relu_ints(_gen(self.id + ":x"), (1, self.h, self.w, self.cin), 3)

    def base(self):
        """dgrad: the integer tensor an accumulating data-gradient adds onto."""
        return torch.randint(-PRE_MAX, PRE_MAX + 1, (1, self.h, self.w, self.cin), generator=_gen(self.id + ":pre")).float()


PRE_MAX = 1000
BIAS_MAX = 4


def make_int_problem(case):
    route, direction, h, w, cin, cout = case
    p = Problem(case_id(case), route, direction, h, w, cin, cout)
    amax, density = int_params(route, p.K)
    p.a = _relu_ints(_gen(p.id + ":a"), (1, h, w, p.K), amax, signed=direction == "dgrad")
    g = _gen(p.id + ":k")
    sign = torch.where(torch.rand((3, 3, p.K, p.N), generator=g) < 0.5, -1.0, 1.0)
    p.k_eff = sign * (torch.rand((3, 3, p.K, p.N), generator=g) < density)
    if direction == "fwd":
        p.bias = torch.randint(-BIAS_MAX, BIAS_MAX + 1, (cout,), generator=_gen(p.id + ":b")).float()
    return p


def make_wide_problem(shape, direction, kind):
    _, route, h, w, cin, cout = shape
    p = Problem(wide_id(shape, direction, kind), route, direction, h, w, cin, cout)
    p.kind = kind
    g = _gen(p.id + ":k")
    nnz = torch.randint(1, 4, (p.N,), generator=g)                     # 1 .. 3 non-zero input channels per output channel
    chans = torch.stack([torch.randperm(p.K, generator=g)[:3] for _ in range(p.N)])          # (N, 3)
    sel = torch.zeros(p.K, p.N)
    for j in range(3):
        sel[chans[:, j], torch.arange(p.N)] = (nnz > j).float()
    p.k_eff = torch.zeros(3, 3, p.K, p.N)
    sign = torch.where(torch.rand((p.K, p.N), generator=g) < 0.5, -1.0, 1.0)
    one = torch.zeros(p.K, p.N)
    one[chans[:, 0], torch.arange(p.N)] = 1.0                         # a single input channel per output channel
    if kind == "v12":
        # V of 9 .. 15 bits from 8-bit pixels; a tap at (0, 0) with k = +-1: U = +-(6, -4, -4, 1, 1, 0) x (6, -4, -4, 1, 1, 0)
        p.a = _relu_ints(_gen(p.id + ":a"), (1, h, w, p.K), 255, signed=direction == "dgrad")
        p.k_eff[0, 0] = sel * sign
    elif kind == "v17":
        # V of up to 19 bits from pixels up to 10000; the centre tap with k = +-1 (U = +-(0, -4, 4, 2, -2, 0) x the same, at
        # most 16) on one channel, so that U V stays below 2^24
        p.a = _relu_ints(_gen(p.id + ":a"), (1, h, w, p.K), 10000, signed=direction == "dgrad")
        p.k_eff[1, 1] = one * sign
    else:
        # U wide, V narrow: pixels 0 / 1 (|V| <= 50) and a tap at (0, 0) with 4096 <= |k| <= 8000 on one channel:
        # U = k (36, 24, 16, 6, 4, 1), i.e. 9 k, 3 k and k up to bits: 13 .. 17 significant bits, 36 * 8000 * 50 = 0.86 * 2^24
        p.a = _relu_ints(_gen(p.id + ":a"), (1, h, w, p.K), 1)
        p.k_eff[0, 0] = one * sign * torch.randint(4096, 8001, (p.K, p.N), generator=g).float()
    if direction == "fwd":
        p.bias = torch.randint(-BIAS_MAX, BIAS_MAX + 1, (cout,), generator=_gen(p.id + ":b")).float()
    return p


# ---------------------------------------------------------------------------------------------------------- references
def pool_reference(pre, last=False):
    """strotss_maxpool2_fwd by its header, from the float64 pre-activation (1, h, w, c): (max(window, 0), code) with code the
    FIRST maximum in scan order (0,0), (0,1), (1,0), (1,1), or 4 where the maximum is not positive.  last=True: the planted
    variant that names the last maximum."""
    _, h, w, c = pre.shape
    ph, pw = h // 2, w // 2
    win = pre[0, :2 * ph, :2 * pw].reshape(ph, 2, pw, 2, c).permute(0, 2, 1, 3, 4).reshape(ph, pw, 4, c)
    mx = win.max(2).values
    eq = win == mx[:, :, None]
    order = (3, 2, 1, 0) if last else (0, 1, 2, 3)
    code = torch.full(mx.shape, order[3], dtype=torch.uint8, device=pre.device)
    for k in reversed(order[:3]):
        code = torch.where(eq[:, :, k], torch.tensor(k, dtype=torch.uint8, device=pre.device), code)
    code = torch.where(mx > 0, code, torch.tensor(4, dtype=torch.uint8, device=pre.device))
    return torch.relu(mx)[None], code[None]


def tied_windows(pre):
    """Share of the pooling windows of the float64 pre-activation whose positive maximum occurs more than once."""
    _, h, w, c = pre.shape
    ph, pw = h // 2, w // 2
    win = pre[0, :2 * ph, :2 * pw].reshape(ph, 2, pw, 2, c).permute(0, 2, 1, 3, 4).reshape(ph, pw, 4, c)
    mx = win.max(2).values
    return float((((win == mx[:, :, None]).sum(2) > 1) & (mx > 0)).double().mean())


def unpool_reference(d, code):
    """strotss_maxpool2_bwd from the codes: d (1, h, w, c) routed to (1, 2h, 2w, c), element (2y + dy, 2x + dx) = d[y, x] where
    code == 2 dy + dx, else 0."""
    _, h, w, c = d.shape
    out = torch.zeros(1, 2 * h, 2 * w, c, dtype=d.dtype, device=d.device)
    for k in range(4):
        out[0, k // 2::2, k % 2::2] = torch.where(code[0] == k, d[0], torch.zeros_like(d[0]))
    return out


# ---------------------------------------------------------------------------------------------------------- conditions
def sig_bits(v):
    """Largest number of significant bits (highest set bit to lowest set bit) over the integers in v (float64 tensor)."""
    n = v.abs().long()
    n = n[n != 0]
    if n.numel() == 0:
        return 0
    low = n & -n
    return int((torch.frexp(n.double())[1] - torch.frexp(low.double())[1] + 1).max())


def split3_t(x):
    """split3 of csrc/mfma_x3.h on a float32 tensor (torch's bfloat16 conversion rounds to nearest even)."""
    h = x.bfloat16().float()
    r1 = x - h
    m = r1.bfloat16().float()
    r2 = r1 - m
    return h, m, r2.bfloat16().float()


def abs3(v):
    """|h| + |m| + |l| of split3 for float64 values that are exact in float32."""
    h, m, l = split3_t(v.float())
    return (h.abs() + m.abs() + l.abs()).double()


def exact_u(k_eff, tile):
    """(P, P, K, N) float64: U = G (576 k) G^T = (24 G) k (24 G)^T, an integer."""
    G = torch.tensor(MATS[tile][2], dtype=torch.float64, device=k_eff.device)
    return torch.einsum("ar,rqcn,bq->abcn", G, k_eff.double(), G)


G_DOUBLE = {4: [[1.0 / 4, 0, 0], [-1.0 / 6, -1.0 / 6, -1.0 / 6], [-1.0 / 6, 1.0 / 6, -1.0 / 6], [1.0 / 24, 1.0 / 12, 1.0 / 6],
                [1.0 / 24, -1.0 / 12, 1.0 / 6], [0, 0, 1.0]],
            2: [[1.0, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1.0]]}


def _gggt(G, g):
    """G g G^T in float64 in winograd_weights_kernel's order (sums from 0.0, r and q ascending): (P, P, K, N)."""
    P = len(G)
    out = np.zeros((P, P) + g.shape[2:])
    for a in range(P):
        t = []
        for q in range(3):
            acc = np.zeros(g.shape[2:])
            for r in range(3):
                acc = acc + float(G[a][r]) * g[r, q]
            t.append(acc)
        for b in range(P):
            acc = np.zeros(g.shape[2:])
            for q in range(3):
                acc = acc + t[q] * float(G[b][q])
            out[a, b] = acc
    return out


def kernel_u(k_eff, tile, residue=0.0):
    """winograd_weights_kernel restated: G g G^T in float64 with G's fractions as doubles, rounded once to float32, and 0
    where the numerator (24 G) g (24 G)^T is 0.  numpy does not contract a product with its addition as the device compiler
    does, so the 1e-14 a contracted, cancelling sum leaves is modelled by `residue`: it is added to every entry before the
    zero test (the test file shows that the zero test is what removes it).  (P, P, K, N) float32."""
    g = 576.0 * k_eff.double().numpy()
    u = _gggt(G_DOUBLE[tile], g) + residue
    num = _gggt(MATS[tile][2], g)
    return torch.from_numpy(np.where(num == 0.0, 0.0, u).astype(np.float32))


def tile_patches(a, tile, rows):
    """d (P, P, len(rows) * TW, K): the (tile + 2)^2 input patch of every tile in tile rows `rows` of a (h, w, K)."""
    h, w, K = a.shape
    P = tile + 2
    TH, TW = -(-h // tile), -(-w // tile)
    ap = torch.zeros(TH * tile + 2, TW * tile + 2, K, dtype=a.dtype, device=a.device)
    ap[1:h + 1, 1:w + 1] = a
    rows = torch.as_tensor(rows, device=a.device)
    d = torch.stack([torch.stack([ap[tile * rows + r][:, q:q + tile * TW:tile] for q in range(P)]) for r in range(P)])
    return d.reshape(P, P, -1, K)


def winograd_conditions(p, rows=None, extra=0.0, chunk_rows=32):
    """Conditions 2 .. 5 of problem p over tile rows `rows` (default: all), in float64 on p.a's device.  Returns the figures
    (each a share of 2^24 or a bit count) and, for the rows given, the float64 Winograd-domain result Y (m, m, tiles, N)
    without bias.  `extra`: max |base| of an accumulating data-gradient."""
    m = p.tile
    BT, AT, _ = (torch.tensor(t, dtype=torch.float64, device=p.a.device) for t in MATS[m])
    U = exact_u(p.k_eff.to(p.a.device), m)
    P = m + 2
    Uf = U.reshape(P * P, p.K, p.N)
    Ua = abs3(Uf) if p.x3 else Uf.abs()
    TH = -(-p.h // m)
    rows = list(range(TH)) if rows is None else list(rows)
    a = p.a[0].double()
    fig = {"v": 0.0, "m": 0.0, "out": 0.0, "bits_v": 0, "bits_u": sig_bits(U)}
    ys = []
    for i in range(0, len(rows), chunk_rows):
        d = tile_patches(a, m, rows[i:i + chunk_rows])
        V = torch.einsum("ar,rqtc,bq->abtc", BT, d, BT).reshape(P * P, -1, p.K)
        M = torch.bmm(V, Uf)
        fig["v"] = max(fig["v"], float(V.abs().max()) / LIMIT)
        fig["bits_v"] = max(fig["bits_v"], sig_bits(V))
        fig["m"] = max(fig["m"], float(torch.bmm(abs3(V) if p.x3 else V.abs(), Ua).max()) / LIMIT)
        Mv = M.reshape(P, P, -1, p.N)
        S = torch.einsum("ia,abtn,jb->ijtn", AT.abs(), Mv.abs(), AT.abs())
        fig["out"] = max(fig["out"], float(S.max()))
        ys.append((torch.einsum("ia,abtn,jb->ijtn", AT, Mv, AT), S))
    fig["out"] = (fig["out"] + (float(p.bias.abs().max()) if p.bias is not None else 0.0) + extra) / LIMIT
    return fig, torch.cat([y for y, _ in ys], 2), torch.cat([s for _, s in ys], 2)


def assert_winograd_conditions(fig, ident, wide=False):
    lim_m = WIDE_M_HEADROOM if wide else 1.0
    assert fig["v"] < 1.0, (ident, "condition 2: |V|", fig)
    assert fig["m"] < lim_m, (ident, "condition 3: sum |U||V|", fig)
    if not wide:
        assert fig["out"] < 1.0, (ident, "condition 4: sum |A^T||M||A| + |bias| + |base|", fig)
        assert fig["bits_u"] <= 16 and fig["bits_v"] <= 16, (ident, "condition 5: significant bits", fig)


def direct_conditions(p, extra=0.0):
    """Condition 6: max over outputs of the sum of |a| |g| over the 9 K terms, + max |bias| + max |base|, as a share of 2^24."""
    s = float(conv64(p.a.abs(), 576.0 * p.k_eff.to(p.a.device).abs()).max())
    return {"sum": (s + (float(p.bias.abs().max()) if p.bias is not None else 0.0) + extra) / LIMIT}


def untile(Y, p, rows):
    """(m, m, len(rows) * TW, N) tile outputs -> (len(rows) * m, w, N) rows of the image (columns cropped to w)."""
    m = p.tile
    TW = -(-p.w // m)
    n = len(rows)
    return Y.reshape(m, m, n, TW, p.N).permute(2, 0, 3, 1, 4).reshape(n * m, TW * m, p.N)[:, :p.w]


def shares(ref):
    """(share strictly positive, share strictly negative) of a float64 tensor."""
    return float((ref > 0).double().mean()), float((ref < 0).double().mean())


def assert_nontrivial(ref, ident):
    pos, neg = shares(ref)
    assert pos >= FLOOR and neg >= FLOOR, (ident, "condition 7: shares of positive / negative outputs", pos, neg)
    return pos, neg


def plane_shares(p, rows=None):
    """Wide family: among the non-zero products U V of the rows given, the share whose wide factor (V for v12 / v17, U for
    u17) has a non-zero m plane, and a non-zero l plane."""
    m = p.tile
    P = m + 2
    BT = torch.tensor(MATS[m][0], dtype=torch.float64, device=p.a.device)
    U = exact_u(p.k_eff.to(p.a.device), m).reshape(P * P, p.K, p.N)
    TH = -(-p.h // m)
    rows = list(range(TH)) if rows is None else list(rows)
    V = torch.einsum("ar,rqtc,bq->abtc", BT, tile_patches(p.a[0].double(), m, rows), BT).reshape(P * P, -1, p.K)
    nzu, nzv = (U != 0).double(), (V != 0).double()
    total = float(torch.bmm(nzv, nzu).sum())
    out = []
    for plane in (1, 2):
        if p.kind == "u17":
            has = (split3_t(U.float())[plane] != 0).double()
            out.append(float(torch.bmm(nzv, has).sum()) / total)
        else:
            has = (split3_t(V.float())[plane] != 0).double()
            out.append(float(torch.bmm(has, nzu).sum()) / total)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------- comparisons
def check_bitwise(got, ref64, what):
    """got (float32) must hold exactly the float64 reference's values, and no -0.0.  Raises with the mismatch pattern."""
    got = torch.as_tensor(got)
    ref64 = torch.as_tensor(ref64).to(got.device)
    assert got.dtype == torch.float32 and got.shape == ref64.shape, (what, got.dtype, got.shape, ref64.shape)
    bad = ~(got.double() == ref64)                      # (NaN compares unequal: an unwritten entry fails)
    if bool(bad.any()):
        idx = bad.nonzero()
        first = tuple(int(v) for v in idx[0])
        raise AssertionError((what, "not bit for bit", int(bad.sum()), "of", bad.numel(), "first at", first,
                              float(got[first]), float(ref64[first]),
                              "rows", sorted(set(idx[:, -3].tolist()))[:8], "cols", sorted(set(idx[:, -2].tolist()))[:8],
                              "channels", sorted(set(idx[:, -1].tolist()))[:8]) if got.dim() >= 3 else (what, int(bad.sum())))
    negzero = (got == 0) & torch.signbit(got)
    assert not bool(negzero.any()), (what, "holds -0.0", int(negzero.sum()))


def check_bound(got, ref64, bound, what):
    """|got - ref| <= bound element by element; returns the largest error / bound (0 / 0 counts as 0)."""
    got = torch.as_tensor(got)
    ref64 = torch.as_tensor(ref64).to(got.device)
    bound = torch.as_tensor(bound).to(got.device)
    err = (got.double() - ref64).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max())
    assert worst <= 1.0, (what, "error / bound", worst, "at", tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0]))
    return worst


def check_codes(got, want, what):
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    bad = got != want.to(got.device)
    assert not bool(bad.any()), (what, int(bad.sum()), "codes differ, first at", tuple(int(v) for v in bad.nonzero()[0]))


def check_sign_words(bits, pre64, what):
    """The sign words a kernel wrote equal `pre64 > 0` on every bit inside the image."""
    words, valid = sign_words(pre64)
    bits = torch.as_tensor(bits).long().to(words.device) & 0xFFFFFFFF
    bad = (bits & valid) != words
    assert not bool(bad.any()), (what, int(bad.sum()), "sign words differ, first (tile, channel)",
                                 tuple(int(v) for v in bad.nonzero()[0]))


# ---------------------------------------------------------------------------------------------------------- distance GEMM
# (label, n, ns): the n x ns x d shapes of _loss_cases.py, d = 2179 in rows of 2208 floats
DIST_SHAPES = [("step", 1024, 1024), ("n1000_ns777", 1000, 777), ("n777_ns1000", 777, 1000), ("n37_ns1500", 37, 1500),
               ("n1_ns64", 1, 64), ("n2_ns64", 2, 64)]
DIST_D = 2179
DIST_KINDS = ("dense", "x_wide", "y_wide", "both_mid")


def make_dist_rows(label, n, ns, kind):
    """Integer rows x (n, d), y (ns, d).  dense: x in 0 .. 2 (half zeros), y in -1 .. 1: every index, only h planes.
    x_wide / y_wide: eight entries per row of up to 19 bits against dense -1 .. 1: the m and l planes of one operand.
    both_mid: eight entries per row of up to 10 bits against dense entries of up to 10 bits: the m x m product."""
    d = DIST_D
    tag = f"dist-{label}-{kind}"

    def sparse(g, rows, vmax, nnz=8):
        v = torch.zeros(rows, d)
        for i in range(rows):
            cols = torch.randperm(d, generator=g)[:nnz]
            v[i, cols] = torch.randint(-vmax, vmax + 1, (nnz,), generator=g).float()
        return v

    def dense(g, rows, vmax):
        return torch.randint(-vmax, vmax + 1, (rows, d), generator=g).float()

    gx, gy = _gen(tag + ":x"), _gen(tag + ":y")
    if kind == "dense":
        return _relu_ints(gx, (n, d), 2), dense(gy, ns, 1)
    if kind == "x_wide":
        return sparse(gx, n, 2 ** 19 - 1), dense(gy, ns, 1)
    if kind == "y_wide":
        return dense(gx, n, 1), sparse(gy, ns, 2 ** 19 - 1)
    return sparse(gx, n, 1023), dense(gy, ns, 1023)


def dist_self_operand(x, y, kind):
    """The rows whose self-distance matrix is asked for: x, except where x is the wide operand (x . x would pass 2^24)."""
    return y if kind == "x_wide" else x


def dist_conditions(x, y):
    """max sum_k |x|_3 |y|_3 as a share of 2^24 (every partial sum of the six plane products is then an exact integer), and
    the shares of non-zero products with a non-zero m / l plane in either factor."""
    x, y = x.double(), y.double()
    s = float((abs3(x) @ abs3(y).T).max()) / LIMIT
    nzx, nzy = (x != 0).double(), (y != 0).double()
    total = float((nzx @ nzy.T).sum())
    sh = []
    for plane in (1, 2):
        hx, hy = (split3_t(x.float())[plane] != 0).double(), (split3_t(y.float())[plane] != 0).double()
        both = (hx @ nzy.T + nzx @ hy.T - hx @ hy.T).sum()
        sh.append(float(both) / total)
    return s, tuple(sh)
