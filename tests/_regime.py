"""Seeded data shaped like a pretrained trunk's, for the tests that ask whether a kernel depends on its values: dead
channels, mostly-zero maps, heavy tails, channel scales spread over orders of magnitude, sparse and tiny data-gradients.
A plain module (not a conftest), everything is built on the CPU: tests/test_regime_cpu.py asserts the properties stated
here, tests/test_hip_regime.py runs the convolution routes on this data, tests/_loss_cases.py draws its "regime" rows from
`loss_rows`, tests/test_hip_engine.py runs one step on `trunk_weights`.

Channel gains are powers of two with a real exponent, 2^u: u uniform on [-6, 6] for activations and gradients, on [-3, 3]
for a kernel's output channels.  A kernel's input channels get 2^-u_in with u_in uniform on [-3, 3] drawn from the
kernel's own seed: it is independent of the gains of the activation it meets, so the products x_c w_c keep a spread of
their own (up to 2^18 between channels) instead of cancelling back to one scale."""
import math
import os

import numpy as np
import torch

import _route_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEAD_SHARE = 0.10            # of channels (activations), output channels (kernels), columns (loss rows)
DEAD_BIAS = -2.0 ** 30       # below any pre-activation these tests can produce: the channel is 0 after the ReLU
GRAD_LEVEL = 2.0 ** -27      # median magnitude of a data-gradient entry before its channel gain
GRAD_PIXELS = 4096           # 4 index sets x 1024 samples: the most pixels a tap adjoint touches in one map
TAP_CHANNELS = (64, 64, 128, 128, 256, 256, 256, 512, 512)      # the nine tapped layers behind the 3 RGB columns


def _rng(seed, stream):
    return np.random.default_rng([int(seed), int(stream)])


def _dead(rng, c):
    """About DEAD_SHARE of c channels, at least one: a boolean mask."""
    out = np.zeros(c, dtype=bool)
    out[rng.permutation(c)[:max(1, int(round(DEAD_SHARE * c)))]] = True
    return out


def _activations(h, w, c, seed):
    rng = _rng(seed, 1)
    gain = 2.0 ** rng.uniform(-6.0, 6.0, c)
    dead = _dead(rng, c)
    p_zero = rng.uniform(0.5, 0.9, c)
    x = rng.lognormal(0.0, 1.0, (h, w, c)) * gain
    x *= rng.random((h, w, c)) >= p_zero
    x[:, :, dead] = 0.0
    single = int(np.flatnonzero(~dead)[rng.integers(0, int((~dead).sum()))])
    x[:, :, single] = 0.0
    x[rng.integers(0, h), rng.integers(0, w), single] = gain[single] * rng.lognormal(0.0, 1.0)
    return torch.from_numpy(x.astype(np.float32))[None], dead, single


def activations(h, w, c, seed):
    """(1, h, w, c) float32, non-negative.  Channel gain 2^u, u ~ U[-6, 6]; about 10 % of the channels zero everywhere; a
    live channel has a share of zeros of its own, U[0.5, 0.9]; non-zero entries are log-normal (sigma 1) times the gain;
    one live channel holds a single non-zero pixel."""
    return _activations(h, w, c, seed)[0]


def activation_info(h, w, c, seed):
    """(dead-channel mask, index of the single-pixel channel) of `activations(h, w, c, seed)`."""
    return _activations(h, w, c, seed)[1:]


def gradients(h, w, c, seed):
    """(1, h, w, c) float32, signed: zero except on a seeded set of min(GRAD_PIXELS, h w / 32) pixels (so that windows
    without any exist at every size), where every channel
    holds +- a log-normal (sigma 1) around GRAD_LEVEL times the channel gain 2^u, u ~ U[-6, 6]."""
    rng = _rng(seed, 2)
    gain = 2.0 ** rng.uniform(-6.0, 6.0, c)
    n = min(GRAD_PIXELS, max(1, (h * w) // 32))
    pix = rng.permutation(h * w)[:n]
    g = np.zeros((h * w, c))
    g[pix] = rng.lognormal(math.log(GRAD_LEVEL), 1.0, (n, c)) * gain * rng.choice((-1.0, 1.0), (n, c))
    return torch.from_numpy(g.reshape(h, w, c).astype(np.float32))[None]


def weights(cin, cout, seed, scale=1.0):
    """(w (3, 3, cin, cout), b (cout,)) float32: He-normal times 2^u per output channel (u ~ U[-3, 3]) times 2^-u_in per input
    channel (u_in ~ U[-3, 3], see the module text) times `scale`; biases N(0, 0.5) times `scale`, about 10 % of the output
    channels DEAD_BIAS instead."""
    rng = _rng(seed, 3)
    w = rng.standard_normal((3, 3, cin, cout)) * math.sqrt(2.0 / (9 * cin))
    w *= 2.0 ** rng.uniform(-3.0, 3.0, cout)
    w *= (2.0 ** -rng.uniform(-3.0, 3.0, cin))[:, None]
    b = rng.normal(0.0, 0.5, cout)
    dead = _dead(rng, cout)
    w, b = w * scale, b * scale
    b[dead] = DEAD_BIAS
    return torch.from_numpy(w.astype(np.float32)), torch.from_numpy(b.astype(np.float32))


def dead_outputs(cin, cout, seed):
    """The output channels `weights(cin, cout, seed)` kills (boolean mask)."""
    return (weights(cin, cout, seed)[1] == DEAD_BIAS).numpy()


# ------------------------------------------------------------------------------------------------------------ the trunk
TRUNK_SEED = 0
# log2 of each layer's `scale`, fixed on the CPU with the float64 oracle on tests/golden/content_im.jpg at 64 px so that the
# 99th percentile of the layer's non-zero activations walks from about 2 (block1) to about 100 (block5): without it the two
# gains multiply the variance by E[4^u]^2 = 59 per layer.  tests/test_regime_cpu.py asserts the outcome:
# block5_conv3's 99th percentile (all entries) within [10, 1000], at least 5 % dead channels in every tapped layer.
TRUNK_LOG2_SCALE = (-2, -3, -2, -3, -1, -3, -3, -1, -2, -2, -2, -2, -3)


def trunk_layers():
    from oracle import strotss_oracle as O
    return [it for it in O.VGG16_CFG if it != "pool"]


def trunk_weights(seed=TRUNK_SEED, log2_scale=TRUNK_LOG2_SCALE):
    """[(w (3, 3, cin, cout), b (cout,)), ...] float32 in layer order, the list format of make_synthetic_vgg16_weights: layer l
    is `weights(cin, cout, 7919 (seed + 1) + l, 2^log2_scale[l])`."""
    return [weights(cin, cout, 7919 * (int(seed) + 1) + l, 2.0 ** log2_scale[l]) for l, (_, cin, cout) in enumerate(trunk_layers())]


def golden_content_64():
    """tests/golden/content_im.jpg at the schedule's 64 px scale (42 x 64), float64 (1, h, w, 3) in [0, 1]."""
    from PIL import Image
    from oracle import strotss_oracle as O
    img = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "content_im.jpg")).convert("RGB"), dtype=np.float64) / 255.0
    return O.resize(torch.from_numpy(img)[None], 64)


# ------------------------------------------------------------------------------------------------------------ loss rows
def _columns(d):
    """The column structure of d-wide hypercolumn rows, a function of d alone (it is the network, not the sample): per
    column its scale (RGB 1; nine tap blocks growing geometrically from 1 to 100, times a gain 2^U[-3, 3] of the column's
    own), its share of zeros U[0.65, 0.85], the texture phase U[0, 1) it responds to, and whether it is dead (about 10 % of
    the tap columns)."""
    rng = _rng(d, 4)
    if d - 3 == sum(TAP_CHANNELS):
        widths = list(TAP_CHANNELS)
    else:
        widths = [(d - 3) // 9 + (k < (d - 3) % 9) for k in range(9)]
    scale = np.concatenate([np.ones(3)] + [np.full(wd, 100.0 ** (k / 8.0)) for k, wd in enumerate(widths)])
    scale[3:] *= 2.0 ** rng.uniform(-3.0, 3.0, d - 3)
    p_zero = rng.uniform(0.65, 0.85, d)
    dead = np.zeros(d, dtype=bool)
    dead[3:] = _dead(rng, d - 3)
    return scale, p_zero, dead, rng.random(d)


def loss_rows(rng, m, d):
    """A drop-in for _loss_cases.hyper_rows: (m, d) float64 rows, RGB in [0, 1] in columns 0..2, behind them log-normal
    (sigma 0.5) entries times their column's scale (`_columns`) and a level 2^U[-1, 1] of the row's own.  A row has a texture
    phase t of its own; an entry is non-zero with probability (1 - p_zero_j) (1 + cos 2 pi (t - t_j))^2 / 1.5 times the row's density U[0.4, 1.6], so rows of like
    texture share their live columns and the cosine distances spread as an image's do, while a column keeps its 65-85 %
    of zeros over the rows; dead columns are zero in every row of every call."""
    scale, p_zero, dead, phase = _columns(d)
    x = rng.lognormal(0.0, 0.5, (m, d)) * scale * 2.0 ** rng.uniform(-1.0, 1.0, (m, 1))
    x *= rng.random((m, d)) < (1.0 - p_zero) * (1.0 + np.cos(2.0 * np.pi * (rng.random((m, 1)) - phase))) ** 2 / 1.5 * rng.uniform(0.4, 1.6, (m, 1))
    x[:, dead] = 0.0
    x[:, :3] = rng.random((m, 3))
    return x


# ------------------------------------------------------------------------------------------------------------ conv cases
def smallest_cases():
    """For every (route, direction) the default policy reaches: the DEFAULT_CASES entry with the fewest multiply-adds."""
    best = {}
    for c in RC.DEFAULT_CASES:
        key = c[:2]
        macs = c[2] * c[3] * c[4] * c[5]
        if key not in best or macs < best[key][0]:
            best[key] = (macs, c)
    return [best[k][1] for k in sorted(best, key=lambda k: (RC.ROUTES.index(k[0]), k[1] != "fwd"))]


CASES = smallest_cases()


def case_seed(case):
    import zlib
    return zlib.crc32(RC.case_id(case).encode())


def tile_of(route):
    return 0 if route.startswith("direct") else 2 if route == "F2_gemm_f32" else 4


class Problem:
    """One case's regime data on the CPU (float32): the layer's kernel and bias, and for a forward the input activation, for
    a data-gradient the output gradient `gy`, the input activation `x` that masks it and the base `pre` it accumulates on.
    `a` is the tensor the route transforms and `k` the (3, 3, K, N) kernel it meets (the data-gradient's flipped and
    transposed), so that ref = conv64(a, k) (+ bias) in both directions."""

    def __init__(self, case):
        self.case = case
        self.route, self.direction, self.h, self.w, self.cin, self.cout = case
        s = case_seed(case)
        self.wt, self.bias = weights(self.cin, self.cout, s)
        self.x = activations(self.h, self.w, self.cin, s)
        if self.direction == "fwd":
            self.a, self.k, self.b = self.x, self.wt, self.bias
        else:
            self.gy = gradients(self.h, self.w, self.cout, s)
            self.pre = gradients(self.h, self.w, self.cin, s + 1)
            self.a, self.k, self.b = self.gy, self.wt.flip(0, 1).transpose(2, 3).contiguous(), None


def scale_problem(case):
    """Section-4 data of a case (float32, CPU): relu(randn) activations and randn gradients quantised to multiples of 2^-20,
    He-normal kernel, N(0, 0.1) bias quantised alike -> dict(x, wt, b, gy)."""
    _, _, h, w, cin, cout = case
    g = torch.Generator().manual_seed(case_seed(case) ^ 0x5CA1E)
    q = lambda t: torch.round(t * 2.0 ** 20) / 2.0 ** 20
    x = q(torch.relu(torch.randn(1, h, w, cin, generator=g)))
    wt = torch.randn(3, 3, cin, cout, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = q(torch.randn(cout, generator=g) * 0.1)
    gy = q(torch.randn(1, h, w, cout, generator=g))
    return dict(x=x, wt=wt, b=b, gy=gy)


SCALE_EXPONENTS = (-40, 40)


# ------------------------------------------------------------------------------------------------------------ normalisers
def window_max(a, size):
    """(1, h, w, c) -> the maximum of |a| over the size x size window centred on each pixel (zero outside the map)."""
    return torch.nn.functional.max_pool2d(a.abs().permute(0, 3, 1, 2), size, 1, size // 2).permute(0, 2, 3, 1)


def normaliser(a, k, b, tile, conv64):
    """What one output element's rounding error is measured against, float64 (1, h, w, N), on a's device.
    tile 0 (direct): |a| (*) |k| + |b|, the same convolution of absolute values: every term the element sums.
    tile 2 / 4 (Winograd): 9 sum_c winmax(|a|)_c maxtap|k|_{c,n} + |b| with a 5 x 5 / 9 x 9 window maximum: the transforms mix
    the (tile + 2)^2 input patch of the element's tile, and every patch of a tile that contains the pixel lies inside
    that window."""
    if tile == 0:
        out = conv64(a.abs(), k.abs())
    else:
        win = window_max(a.double(), 2 * tile + 1)
        out = 9.0 * torch.matmul(win, k.abs().double().amax(dim=(0, 1)))
    return out + (b.abs().double() if b is not None else 0.0)


def element_error(got, ref, norm):
    """max over the elements with norm > 0 of |got - ref| / norm, and whether every element with norm == 0 is exactly 0."""
    live = norm > 0
    e = ((got.double() - ref).abs() / torch.where(live, norm, torch.ones_like(norm)))[live]
    return float(e.max()) if e.numel() else 0.0, bool((got[~live] == 0).all())


def yardstick_f32(a, k, b, tile, relu):
    """The float32 CPU restatement of the route's algorithm on the same data: conv2d for the direct routes, Lavin & Gray's
    F(2x2,3x3) / F(4x4,3x3) in NumPy (tests/_conv_ref.py) for the Winograd ones (the bf16x3 routes claim f32-exact products,
    so they are held to the same F(4x4,3x3) yardstick)."""
    from _conv_ref import winograd_f32
    if tile == 0:
        out = torch.nn.functional.conv2d(a.permute(0, 3, 1, 2), k.permute(3, 2, 0, 1).contiguous(), padding=1).permute(0, 2, 3, 1)
    else:
        out = winograd_f32(a.numpy(), k.numpy(), tile)
    if b is not None:
        out = out + b
    return torch.relu(out) if relu else out
