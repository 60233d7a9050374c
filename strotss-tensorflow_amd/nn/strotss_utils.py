"""Sampling (hypercolumn gather), Laplacian pyramid, YUV, postprocess, masks -- mirrors the
reference's nn/strotss_utils.py:12-201 on torch HIP tensors and the kernels of libstrotss_hip.so.

The optimisation loop itself goes through `nn.engine` (pre-allocated buffers, fused backward);
the functions here are the reference's operator surface, differentiable where the reference's are
(`fold_laplacian_pyramid`, `Sampling.bilinear`) through small `torch.autograd.Function` bridges."""
from __future__ import annotations

import math
import os
from functools import partialmethod
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _ops, rand, utils

RGB2YUV = ((0.299, -0.14714119, 0.61497538),       # tf.image.rgb_to_yuv kernel, rgb @ M
           (0.587, -0.28886916, -0.51496512),
           (0.114, 0.43601035, -0.10001026))


# ----------------------------------------------------------------------------- autograd bridges
class _ResizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, oh, ow):
        ctx.in_hw = (int(x.shape[-3]), int(x.shape[-2]))
        return _ops.resize_bilinear(x.detach().contiguous(), oh, ow)

    @staticmethod
    def backward(ctx, g):
        return _ops.resize_bilinear_adjoint(g.contiguous(), *ctx.in_hw), None, None


def _resize(x: torch.Tensor, oh: int, ow: int) -> torch.Tensor:
    if x.requires_grad:
        return _ResizeFn.apply(x, oh, ow)
    return _ops.resize_bilinear(x.contiguous(), oh, ow)


class _GatherFn(torch.autograd.Function):
    """feats(n, D) = bilinear hypercolumns of the maps at idx; gradient to every map that needs it."""

    @staticmethod
    def forward(ctx, idx, n_maps, *maps):
        maps_c = [m.detach().contiguous() for m in maps]
        out = _ops.hypercol_gather(maps_c, idx, True)
        ctx.maps = maps_c
        ctx.idx = idx
        d = sum(int(m.shape[-1]) for m in maps_c)
        ctx.nd = (idx.shape[0], d)
        return out[:idx.shape[0], :d]

    @staticmethod
    def backward(ctx, g):
        n, d = ctx.nd
        gbuf = torch.zeros((_ops.pad32(n), _ops.pad32(d)), dtype=torch.float32, device=g.device)
        gbuf[:n, :d] = g
        gm = [torch.zeros_like(m) for m in ctx.maps]
        # the maps are plain inputs here (any ReLU mask belongs to whoever produced them)
        _ops.hypercol_scatter(ctx.maps, gm, ctx.idx, gbuf, relu_mask_from=len(gm))
        return (None, None, *gm)


# ----------------------------------------------------------------------------- Sampling
def sampling_steps(h: int, w: int) -> Tuple[int, int]:
    """reference strotss_utils.py:89-90"""
    area = math.sqrt((h * w) // (128 ** 2))
    return max(1, math.floor(area)), max(1, math.ceil(area))


def make_indices_np(h: int, w: int, bilinear_sampling: bool, sample_size: int, rng: np.random.Generator,
                    mask_hw: Optional[np.ndarray] = None) -> np.ndarray:
    """reference strotss_utils.py:83-121 given the ALREADY resized+thresholded boolean mask (h,w).
    Strided grid with random offsets (bilinear mode) or every pixel, optional mask filter, joint
    shuffle of the (row, col) pairs, first `sample_size`, float32."""
    if bilinear_sampling:
        step_x, step_y = sampling_steps(h, w)
        off_x = int(rng.integers(0, step_x))
        off_y = int(rng.integers(0, step_y))
        X = np.arange(h)[off_x::step_x]
        Y = np.arange(w)[off_y::step_y]
    else:
        X, Y = np.arange(h), np.arange(w)
    XX, YY = np.meshgrid(X, Y)                      # tf.meshgrid default 'xy'
    ret = np.stack([XX.reshape(-1), YY.reshape(-1)], axis=1)
    if mask_hw is not None:
        ret = ret[mask_hw[ret[:, 0], ret[:, 1]]]
    if hasattr(rng, "permutation_head"):                # PhiloxStream: the same first `sample_size` entries, without the full sort
        ret = ret[rng.permutation_head(ret.shape[0], sample_size)]
    else:
        ret = ret[rng.permutation(ret.shape[0])][:sample_size]
    return ret.astype(np.float32)


def make_indices_weighted_np(h: int, w: int, sample_size: int, rng, levels_hw: np.ndarray,
                             mask_hw: Optional[np.ndarray] = None) -> np.ndarray:
    """make_indices_np's bilinear branch with the weighted head (--sample_map): the host twin of
    strotss_index_draw_weighted.  levels_hw: (h, w) uint16 levels at this scale (sample_levels_at_scale); rng: a
    rand.PhiloxStream, consumed exactly as make_indices_np consumes it (one draw number per call)."""
    levels_hw = np.asarray(levels_hw)
    if levels_hw.dtype != np.uint16 or levels_hw.shape != (h, w):
        raise ValueError(f"sample levels of dtype {levels_hw.dtype} and shape {levels_hw.shape}: expected uint16 ({h}, {w})")
    step_x, step_y = sampling_steps(h, w)
    off_x = int(rng.integers(0, step_x))
    off_y = int(rng.integers(0, step_y))
    XX, YY = np.meshgrid(np.arange(h)[off_x::step_x], np.arange(w)[off_y::step_y])
    ret = np.stack([XX.reshape(-1), YY.reshape(-1)], axis=1)
    if mask_hw is not None:
        ret = ret[mask_hw[ret[:, 0], ret[:, 1]]]
    ret = ret[rng.permutation_head_weighted(ret.shape[0], sample_size, levels_hw[ret[:, 0], ret[:, 1]])]
    return ret.astype(np.float32)


def load_sample_map(path: str) -> torch.Tensor:
    """--sample_map: the image read as greyscale, divided by 255 -> (H, W) float32 host tensor in [0, 1]."""
    return load_content_weight_map(path)


SAMPLE_MAX_RADIUS = 64                   # strotss_detail_map's window radius, 1..64
DEFAULT_SAMPLE_GAIN = 2.0                # detail at `gain` times the image's mean detail saturates the map; not tuned
DEFAULT_SAMPLE_FLOOR = 0.25              # the level of a flat region: it is still sampled, four times less densely; not tuned


def default_sample_radius(h: int, w: int) -> int:
    """max(1, longer side // 64), at most 64 (a documented choice, not a tuned value)"""
    return max(1, min(SAMPLE_MAX_RADIUS, max(int(h), int(w)) // 64))


def check_sample_parameters(radius, gain, floor) -> None:
    """ValueError for a radius that is not an integer in 1..64, a gain that is not finite or <= 0, a floor that is not
    finite or outside [0, 1] (None: not given)"""
    if radius is not None and (int(radius) != radius or not 1 <= int(radius) <= SAMPLE_MAX_RADIUS):
        raise ValueError(f"sample radius {radius!r}: expected an integer in 1..{SAMPLE_MAX_RADIUS}")
    if gain is not None and not (math.isfinite(gain) and gain > 0):
        raise ValueError(f"sample gain {gain!r}: expected a finite value above 0")
    if floor is not None and not (math.isfinite(floor) and 0 <= floor <= 1):
        raise ValueError(f"sample floor {floor!r}: expected a finite value in [0, 1]")


def auto_sample_map(content, radius=None, gain=None, floor=None) -> torch.Tensor:
    """--sample_map auto: the detail map of the content as utils.load_image returns it ((1, h, w, 3)
    or (h, w, 3)) -> (h, w) float32 host tensor in [floor, 1], what load_sample_map returns for a painted map
    (strotss_detail_map on the device).  None: default_sample_radius(h, w), DEFAULT_SAMPLE_GAIN, DEFAULT_SAMPLE_FLOOR.
    ValueError as check_sample_parameters."""
    check_sample_parameters(radius, gain, floor)
    c = _rgb(content, "content")
    if radius is None:
        radius = default_sample_radius(int(c.shape[0]), int(c.shape[1]))
    out = _ops.detail_map(c, int(radius), DEFAULT_SAMPLE_GAIN if gain is None else float(gain),
                          DEFAULT_SAMPLE_FLOOR if floor is None else float(floor))
    return out.cpu()


def save_sample_map(path: str, sample_map) -> None:
    """--save_sample_map: the (h, w) map in [0, 1] as an 8-bit greyscale PNG, rint(255 v), which load_sample_map reads"""
    from PIL import Image
    m = sample_map.detach().cpu().numpy() if torch.is_tensor(sample_map) else np.asarray(sample_map)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(np.rint(np.clip(m.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8), "L").save(path, format="PNG")


def sample_levels_at_scale(sample_map, h: int, w: int) -> np.ndarray:
    """The levels of a scale: the user's (H, W) map, finite (ValueError otherwise), resized
    bilinearly to (h, w) as content_weight_at_scale resizes, clipped to [0, 1], rint(v * 65535) -> (h, w) uint16 host array.
    The rounding runs on the host, once per scale; an all-zero result is a ValueError (such a map says nothing)."""
    m = sample_map if torch.is_tensor(sample_map) else torch.as_tensor(np.asarray(sample_map))
    if m.dim() == 3 and m.shape[-1] == 1:
        m = m[..., 0]
    if m.dim() != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError(f"sample map of shape {tuple(m.shape)}: expected (H, W) or (H, W, 1)")
    m = m.float()
    if not bool(torch.isfinite(m).all()):
        raise ValueError("sample map: values must be finite")
    if not bool((m > 0).any()):                  # (nothing positive stays so under a bilinear resize: refused before it runs)
        raise ValueError("sample map: every level is zero")
    m = _ops.resize_bilinear(m.reshape(1, *m.shape, 1).to(utils.device()).contiguous(), int(h), int(w))[0, ..., 0]
    v =np.clip(m.detach().cpu().numpy().astype(np.float64), 0.0, 1.0)
    levels = np.rint(v * 65535.0).astype(np.uint16)
    if not levels.any():
        raise ValueError("sample map: every level is zero at this scale")
    return np.ascontiguousarray(levels)


def mask_at_scale(mask: torch.Tensor, h: int, w: int) -> np.ndarray:
    """reference strotss_utils.py:105-110: bilinear resize of the (H,W,1) float mask to the scale,
    `> 0.5` (or all-true if the resized mask is all < 0.1).  Boolean (h,w) host array."""
    m = mask.to(utils.device()).float()
    if m.dim() == 2:
        m = m[..., None]
    m = _ops.resize_bilinear(m.contiguous(), h, w)[..., 0]
    if float(m.max()) < 0.1:
        keep = (m + 1) > 0.5
    else:
        keep = m > 0.5
    return keep.cpu().numpy()


def check_content_weight(weight, h: int, w: int) -> torch.Tensor:
    """A content-weight map at a scale of (h, w): an (h, w) or (1, h, w, 1) array, every value finite and >= 0 -> the
    (1, h, w, 1) float32 tensor on the map's device (ValueError otherwise).  Values above 1 are allowed."""
    t = weight if torch.is_tensor(weight) else torch.as_tensor(np.asarray(weight))
    if tuple(t.shape) not in ((h, w), (1, h, w, 1)):
        raise ValueError(f"content-weight map of shape {tuple(t.shape)}: expected ({h}, {w}) or (1, {h}, {w}, 1)")
    t = t.float()
    if not bool(torch.isfinite(t).all()):
        raise ValueError("content-weight map: values must be finite")
    if bool((t < 0).any()):
        raise ValueError("content-weight map: values must be >= 0")
    return t.reshape(1, h, w, 1).contiguous()


def content_weight_at_scale(weight_map, h: int, w: int) -> torch.Tensor:
    """W_s of a scale: the user's (H, W), (H, W, 1) or (1, H, W, 1) weight map, checked (finite,
    >= 0; ValueError otherwise, before anything runs on the device), resized bilinearly to (h, w) the way mask_at_scale
    resizes a mask, without its threshold.  -> (1, h, w, 1) float32 on the device, checked again."""
    m = weight_map if torch.is_tensor(weight_map) else torch.as_tensor(np.asarray(weight_map))
    if m.dim() == 4 and m.shape[0] == 1 and m.shape[-1] == 1:
        m = m[0, ..., 0]
    elif m.dim() == 3 and m.shape[-1] == 1:
        m = m[..., 0]
    if m.dim() != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError(f"content-weight map of shape {tuple(weight_map.shape)}: expected (H, W), (H, W, 1) or (1, H, W, 1)")
    big_h, big_w = int(m.shape[0]), int(m.shape[1])
    m = check_content_weight(m, big_h, big_w)
    m = _ops.resize_bilinear(m.to(utils.device()).contiguous(), int(h), int(w))
    return check_content_weight(m, int(h), int(w))


def load_content_weight_map(path: str) -> torch.Tensor:
    """--content_weight_map: the image read as greyscale, divided by 255 -> (H, W) float32 host tensor in [0, 1]."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"File not found: {path}")
    from PIL import Image
    with Image.open(path) as im:
        grey = np.asarray(im.convert("L"), dtype=np.float32)
    return torch.from_numpy(grey / np.float32(255.0))


# ----------------------------------------------------------------------------- frame sequences
FLO_MAGIC = 202021.25


def read_flo(path: str) -> torch.Tensor:
    """A Middlebury .flo file -> (h, w, 2) float32 host tensor, (u, v) = (x, y) displacement in pixels.  ValueError on a bad
    magic number or a file whose size is not that of its header's (w, h)."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"File not found: {path}")
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 12 or float(np.frombuffer(raw[:4], dtype="<f4")[0]) != FLO_MAGIC:
        raise ValueError(f"{path}: not a .flo file (magic number {FLO_MAGIC} missing)")
    w, h = (int(v) for v in np.frombuffer(raw[4:12], dtype="<i4"))
    if w <= 0 or h <= 0 or len(raw) != 12 + 8 * w * h:
        raise ValueError(f"{path}: a {w} x {h} flow needs {12 + 8 * max(w, 0) * max(h, 0)} bytes, the file has {len(raw)}")
    return torch.from_numpy(np.frombuffer(raw[12:], dtype="<f4").astype(np.float32).reshape(h, w, 2))


def write_flo(path: str, flow) -> None:
    """The inverse of read_flo: a (h, w, 2) flow (tensor on any device, or array) as a Middlebury .flo file -- the magic
    number as float32, (w, h) as little-endian int32, then the (u, v) pairs row by row as little-endian float32."""
    if isinstance(flow, torch.Tensor):
        flow = flow.detach().cpu().numpy()
    flow = np.asarray(flow, dtype=np.float32)
    if flow.ndim != 3 or flow.shape[-1] != 2:
        raise ValueError(f"flow of shape {tuple(flow.shape)}: expected (h, w, 2)")
    h, w = flow.shape[:2]
    with open(path, "wb") as f:
        f.write(np.array([FLO_MAGIC], dtype="<f4").tobytes())
        f.write(np.array([w, h], dtype="<i4").tobytes())
        f.write(np.ascontiguousarray(flow).astype("<f4").tobytes())


def resize_flow(flow: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """A (H, W, 2) flow field at the size (h, w) of resized frames: both components resized bilinearly (the kernel of
    utils.resize), u multiplied by w / W and v by h / H.  The same size: an unchanged copy.  -> (h, w, 2) float32 on the
    flow's device (a host flow is resized on the device and comes back to the host)."""
    if flow.dim() != 3 or flow.shape[-1] != 2:
        raise ValueError(f"flow of shape {tuple(flow.shape)}: expected (H, W, 2)")
    big_h, big_w = int(flow.shape[0]), int(flow.shape[1])
    if (big_h, big_w) == (int(h), int(w)):
        return flow.float().clone()
    out = _ops.resize_bilinear(flow.float().to(utils.device()).contiguous(), int(h), int(w))
    out = out * torch.tensor([w / big_w, h / big_h], dtype=torch.float32, device=out.device)
    return out.to(flow.device)


def temporal_target_at_scale(warped: torch.Tensor, certainty: torch.Tensor, h: int, w: int):
    """(omega_s, c_s) of a scale: the warped previous frame (1, H, W, 3) and its certainty (H, W), resized bilinearly to
    (h, w) as content_weight_at_scale resizes its map (no threshold) -> ((h, w, 3), (h, w)) float32 on the device."""
    big_h, big_w = int(warped.shape[-3]), int(warped.shape[-2])
    if tuple(certainty.shape[-2:]) != (big_h, big_w) or int(warped.shape[-1]) != 3 or certainty.numel() != big_h * big_w:
        raise ValueError(f"warped frame {tuple(warped.shape)} and certainty {tuple(certainty.shape)} do not match")
    dev = utils.device()
    x = warped.float().to(dev).reshape(big_h, big_w, 3).contiguous()
    c = certainty.float().to(dev).reshape(big_h, big_w, 1).contiguous()
    if (big_h, big_w) == (int(h), int(w)):
        return x.clone(), c.reshape(h, w).clone()
    return _ops.resize_bilinear(x, int(h), int(w)), _ops.resize_bilinear(c, int(h), int(w)).reshape(int(h), int(w))



def temporal_targets_at_scale(temporal, h: int, w: int):
    """the long-term targets of a scale: [(warped_j, combined certainty_j)] nearest frame first, each
    resized as temporal_target_at_scale resizes the one target -> [((h, w, 3), (h, w))]"""
    return [temporal_target_at_scale(warped, certainty, h, w) for warped, certainty in temporal]

class Sampling:
    """reference strotss_utils.py:20-136.  `rng` defaults to nn.rand.index_rng."""

    def __init__(self, sample_size: int, rng: Optional[np.random.Generator] = None, **kwargs):
        self.sample_size = sample_size
        self.rng = rng

    def _rng(self):
        return self.rng if self.rng is not None else rand.index_rng

    def _sample(self, xs: List[torch.Tensor], indices: torch.Tensor, bilinear_sampling: bool) -> torch.Tensor:
        n = indices.shape[0]
        d = sum(int(x.shape[-1]) for x in xs)
        if bilinear_sampling and any(x.requires_grad for x in xs):
            return _GatherFn.apply(indices, len(xs), *xs)
        out = _ops.hypercol_gather([x.detach().contiguous() for x in xs], indices, bilinear_sampling)
        return out[:n, :d]

    def _make_indices(self, base_tensor: torch.Tensor, bilinear_sampling: bool,
                      mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        _, h, w, *_ = base_tensor.shape
        mk = mask_at_scale(mask, int(h), int(w)) if mask is not None else None
        idx = make_indices_np(int(h), int(w), bilinear_sampling, self.sample_size, self._rng(), mk)
        return torch.from_numpy(idx).to(base_tensor.device)

    def __call__(self, xs: List[torch.Tensor], ys: Optional[List[torch.Tensor]] = None,
                 mask: Optional[torch.Tensor] = None, bilinear_sampling: bool = False,
                 indices: Optional[torch.Tensor] = None
                 ) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        if indices is None:
            indices = self._make_indices(xs[0], bilinear_sampling, mask)
        ret = self._sample(xs, indices, bilinear_sampling)
        if ys:
            ret_y = self._sample(ys, indices, bilinear_sampling)
            return ret, ret_y
        return ret

    bilinear = partialmethod(__call__, bilinear_sampling=True)


# ----------------------------------------------------------------------------- Laplacian pyramid
def make_laplacian(x: torch.Tensor, return_downscale: bool = False):
    """reference strotss_utils.py:139-146"""
    h, w = int(x.shape[1]), int(x.shape[2])
    hd, wd = max(h // 2, 1), max(w // 2, 1)
    xc = x.contiguous()
    temp = _ops.resize_bilinear(xc, hd, wd)
    pyr = _ops.resize_bilinear(temp, h, w, -1.0, xc)          # x - up(down(x)) in one kernel
    if return_downscale:
        return pyr, temp
    return pyr


def make_laplacian_pyramid(x: torch.Tensor, levels: int = 5) -> List[torch.Tensor]:
    """reference strotss_utils.py:149-156"""
    xs = []
    curx = x
    for _ in range(levels):
        pyr, curx = make_laplacian(curx, return_downscale=True)
        xs.append(pyr)
    xs.append(curx)
    return xs


def fold_laplacian_pyramid(xs: Sequence[torch.Tensor]) -> torch.Tensor:
    """reference strotss_utils.py:159-163 (differentiable w.r.t. every level)."""
    ret = xs[-1]
    needs_grad = any(x.requires_grad for x in xs)
    for x in reversed(xs[:-1]):
        h, w = int(x.shape[1]), int(x.shape[2])
        if needs_grad:
            ret = x + _resize(ret, h, w)
        else:
            ret = _ops.resize_bilinear(ret.contiguous(), h, w, 1.0, x.contiguous())
    return ret


def convert_rgb_to_yuv(x: torch.Tensor) -> torch.Tensor:
    """reference strotss_utils.py:166-167"""
    # three axpys per output channel instead of a (N, 3) x (3, 3) library GEMM
    r, g, b = x[:, 0:1], x[:, 1:2], x[:, 2:3]
    return torch.cat([r * RGB2YUV[0][k] + g * RGB2YUV[1][k] + b * RGB2YUV[2][k] for k in range(3)], dim=1)


def postprocess(final: torch.Tensor) -> torch.Tensor:
    """reference strotss_utils.py:170-175 -> uint8 (H,W,3)"""
    return _ops.postprocess(final.detach().float().contiguous())[0]


# ----------------------------------------------------------------------------- colour preservation
COLOUR_EPS = (1.0 / 255.0) ** 2          # a channel whose spread is below one 8-bit step counts as flat


def _rgb(image, name: str) -> torch.Tensor:
    """an (h, w, 3) or (1, h, w, 3) image -> the (h, w, 3) float32 view on the device; ValueError for another shape"""
    if not torch.is_tensor(image):
        image = torch.as_tensor(np.asarray(image))
    if image.dim() == 4 and image.shape[0] == 1:
        image = image[0]
    if image.dim() != 3 or image.shape[-1] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError(f"{name} of shape {tuple(image.shape)}: expected (h, w, 3) or (1, h, w, 3)")
    return image.float().to(utils.device()).contiguous()


def _plane(mask, h: int, w: int, name: str) -> Optional[torch.Tensor]:
    """an (h, w), (h, w, 1) or (1, h, w, 1) weight plane -> (h, w) float32 on the device; ValueError for another shape"""
    if mask is None:
        return None
    if not torch.is_tensor(mask):
        mask = torch.as_tensor(np.asarray(mask))
    if tuple(mask.shape) not in ((h, w), (h, w, 1), (1, h, w, 1)):
        raise ValueError(f"{name} of shape {tuple(mask.shape)}: expected ({h}, {w}) for an image of that size")
    return mask.float().to(utils.device()).reshape(h, w).contiguous()


def colour_statistics(image, mask=None) -> Tuple[np.ndarray, np.ndarray]:
    """(mu, Sigma) of an (h, w, 3) image, float64 numpy: the weighted mean colour and the biased covariance under the
    optional weight plane `mask` ((h, w), >= 0; None = all ones).  The ten sums come from strotss_color_stats in float64;
    mu = S / W and Sigma = S_ij / W - mu mu^T are formed here.  ValueError: shapes that do not match, W == 0 (an empty
    mask region), statistics that are not finite."""
    x = _rgb(image, "image")
    h, w = int(x.shape[0]), int(x.shape[1])
    sums = _ops.color_stats(x, _plane(mask, h, w, "mask")).cpu().numpy()
    if not np.isfinite(sums).all():
        raise ValueError("colour statistics: the image or the mask holds values that are not finite")
    if sums[0] == 0:
        raise ValueError("colour statistics: the mask selects no pixel (W == 0)")
    if sums[0] < 0:
        raise ValueError("colour statistics: the mask's weights must be >= 0")
    mu = sums[1:4] / sums[0]
    second = np.empty((3, 3))
    second[np.triu_indices(3)] = sums[4:10]
    second = np.triu(second) + np.triu(second, 1).T
    return mu, second / sums[0] - np.outer(mu, mu)


def _sym_power(sigma: np.ndarray, power: float) -> np.ndarray:
    """(sigma + eps I)^power of a symmetric 3 x 3 matrix through its float64 eigendecomposition"""
    lam, vec = np.linalg.eigh(sigma)
    lam = lam + COLOUR_EPS
    if not (lam > 0).all():
        raise ValueError(f"colour covariance is not positive semi-definite (eigenvalues {lam - COLOUR_EPS})")
    return (vec * lam ** power) @ vec.T


def colour_transform(mu_s, sigma_s, mu_c, sigma_c) -> Tuple[np.ndarray, np.ndarray]:
    """(A, b), float64, of the affine map that gives the style's colours the content's mean and covariance (Gatys et al.
    2016): A = (Sigma_c + eps I)^(1/2) (Sigma_s + eps I)^(-1/2), b = mu_c - A mu_s, eps = (1/255)^2, symmetric roots.
    Then mean(A s + b) = mu_c and cov(A s + b) = Sigma_c + eps (I - A A^T) exactly.  Pure host.  ValueError: shapes other
    than (3,) and (3, 3), values that are not finite."""
    mu_s, mu_c = np.asarray(mu_s, dtype=np.float64), np.asarray(mu_c, dtype=np.float64)
    sigma_s, sigma_c = np.asarray(sigma_s, dtype=np.float64), np.asarray(sigma_c, dtype=np.float64)
    if mu_s.shape != (3,) or mu_c.shape != (3,) or sigma_s.shape != (3, 3) or sigma_c.shape != (3, 3):
        raise ValueError(f"colour statistics of shapes {mu_s.shape}, {sigma_s.shape}, {mu_c.shape}, {sigma_c.shape}: "
                         f"expected (3,), (3, 3), (3,), (3, 3)")
    if not all(np.isfinite(v).all() for v in (mu_s, mu_c, sigma_s, sigma_c)):
        raise ValueError("colour statistics must be finite")
    A = _sym_power((sigma_c + sigma_c.T) / 2, 0.5) @ _sym_power((sigma_s + sigma_s.T) / 2, -0.5)
    b = mu_c - A @ mu_s
    if not (np.isfinite(A).all() and np.isfinite(b).all()):
        raise ValueError("colour transform is not finite")
    return A, b


def match_colour(style, content, style_mask=None, content_mask=None) -> torch.Tensor:
    """--preserve_color match: the style image recoloured with the affine map of colour_transform, so that its colour mean
    and covariance are the content's (strotss_color_stats on both, strotss_color_affine on the style; not clamped).  With
    masks ((h, w) planes at each image's size): the statistics of the style pixels in style_mask and of the content pixels
    in content_mask, the map applied where style_mask != 0, the other pixels copied.  -> an image of the style's shape."""
    s = _rgb(style, "style image")
    h, w = int(s.shape[0]), int(s.shape[1])
    sm = _plane(style_mask, h, w, "style mask")
    A, b = colour_transform(*colour_statistics(s, sm), *colour_statistics(content, content_mask))
    out = _ops.color_affine(s, A, b, sm)
    return out.reshape(tuple(style.shape)) if torch.is_tensor(style) else out


# ----------------------------------------------------------------------------- colour transfer
DEFAULT_TRANSFER_ITERS = 10
TRANSFER_ITERS_RANGE = (1, 64)           # the bases of one strotss_color_hist call
TRANSFER_BINS = 1024                     # not tuned: 256 bins land within 20 % of the same distance
_TRANSFER_SEED = 1000                    # basis t >= 1 is drawn from seed 1000 + t, whatever --seed is


def transfer_bases(iters: int) -> np.ndarray:
    """(iters, 3, 3) float32: the orthonormal colour bases of a transfer, their COLUMNS the axes.  Made in float64 and rounded
    once: R_0 = I (the channels themselves), R_t for t >= 1 the Q factor of a 3 x 3 normal draw of a fixed seed with the
    signs chosen so that diag(R) of the factorisation is positive.  The sequence is a prefix of itself for every iters and
    does not depend on --seed."""
    lo, hi = TRANSFER_ITERS_RANGE
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not lo <= iters <= hi:
        raise ValueError(f"transfer iterations {iters!r}: expected a whole number in {lo}..{hi}")
    out = [np.eye(3)]
    for t in range(1, int(iters)):
        q, r = np.linalg.qr(np.random.default_rng(_TRANSFER_SEED + t).standard_normal((3, 3)))
        out.append(q * np.sign(np.diag(r)))
    return np.stack(out).astype(np.float32)


def transfer_colour(style, content, style_mask=None, content_mask=None, iters: int = DEFAULT_TRANSFER_ITERS,
                    bins: int = TRANSFER_BINS) -> torch.Tensor:
    """--preserve_color transfer: the style image with the content's whole colour distribution, by the iterative
    distribution transfer of Pitie, Kokaram and Dahyot (2007): `iters` times, the style's pixels are projected on an
    orthonormal basis (transfer_bases) and each of the three axes is histogram-matched to the content's projection on it.
    2 iters + 2 kernel launches: the content's histograms on every basis (one strotss_color_hist), the style's on the first,
    then per iteration strotss_color_transfer_table and strotss_color_transfer_apply, which also bins the moved pixels on
    the next basis.  Not clamped.  With masks ((h, w) planes at each image's size): the pixels with a weight != 0 count,
    the others of the style are copied.  -> an image of the style's shape.  ValueError, before any launch: shapes that do
    not match, an image that is not finite, a mask that counts no pixel, iters outside 1..64, bins that are not a multiple
    of 4 in 4..4096 (iteration t's target is the slice t of the content's (iters, 3, bins) histograms, 12 bins t bytes into
    them, and strotss_color_transfer_table takes 16-byte aligned pointers; the entries themselves take any bins in 2..4096)."""
    s, c = _rgb(style, "style image"), _rgb(content, "content image")
    sm = _plane(style_mask, int(s.shape[0]), int(s.shape[1]), "style mask")
    cm = _plane(content_mask, int(c.shape[0]), int(c.shape[1]), "content mask")
    bases = transfer_bases(iters)
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 4 <= bins <= 4096 or bins % 4:
        raise ValueError(f"transfer bins {bins!r}: expected a multiple of 4 in 4..4096")
    if not (bool(torch.isfinite(s).all()) and bool(torch.isfinite(c).all())):
        raise ValueError("colour transfer: the style or the content holds values that are not finite")
    for m, name in ((sm, "style"), (cm, "content")):
        if m is not None and not bool((m != 0).any()):
            raise ValueError(f"colour transfer: the {name} mask counts no pixel")
    target = _ops.color_hist(c, bases, bins, cm)             # the content never moves: every iteration's target at once
    hist, table = _ops.color_transfer_workspace(s.device, bins)
    _ops.color_hist(s, bases[:1], bins, sm, out=hist[None])
    out = torch.empty_like(s)
    for t in range(len(bases)):
        _ops.color_transfer_table(hist, target[t], bases[t], bins, out=table)
        following = bases[t + 1] if t + 1 < len(bases) else None
        _ops.color_transfer_apply(s if t == 0 else out, bases[t], table, bins, sm, out=out, next_basis=following,
                                  next_hist=None if following is None else hist)
    return out.reshape(tuple(style.shape)) if torch.is_tensor(style) else out


def luminance_merge(result, content) -> torch.Tensor:
    """--preserve_color luminance: the luma of `result` on the chroma of `content`, out = content + (Y(result) - Y(content))
    on every channel with Y = 0.299 R + 0.587 G + 0.114 B (strotss_luma_merge).  Two images of one size -> the result's
    shape.  ValueError when the sizes differ."""
    r, c = _rgb(result, "result"), _rgb(content, "content")
    if tuple(r.shape) != tuple(c.shape):
        raise ValueError(f"result of shape {tuple(r.shape)} and content of shape {tuple(c.shape)} differ in size")
    out = _ops.luma_merge(r, c)
    return out.reshape(tuple(result.shape)) if torch.is_tensor(result) else out


# ----------------------------------------------------------------------------- photo smoothing
SMOOTH_MAX_RADIUS = 64                   # STROTSS_SMOOTH_MAX_RADIUS
SMOOTH_EPS_RANGE = (1e-4, 1.0)
DEFAULT_SMOOTH_EPS = 1e-2                # 0.1^2 on [0, 1] images: the middle of He's usual range; a documented choice


def default_smooth_radius(h: int, w: int) -> int:
    """1/64 of the longer side, within 1..64 (a documented choice, not a tuned value)"""
    return max(1, min(SMOOTH_MAX_RADIUS, round(max(int(h), int(w)) / 64)))


def check_smooth_parameters(radius, eps) -> None:
    """ValueError for a radius that is not an integer in 1..64 or an eps that is not finite in [1e-4, 1] (None: not given)"""
    if radius is not None and (int(radius) != radius or not 1 <= int(radius) <= SMOOTH_MAX_RADIUS):
        raise ValueError(f"smoothing radius {radius!r}: expected an integer in 1..{SMOOTH_MAX_RADIUS}")
    if eps is not None and not (math.isfinite(eps) and SMOOTH_EPS_RANGE[0] <= eps <= SMOOTH_EPS_RANGE[1]):
        raise ValueError(f"smoothing eps {eps!r}: expected a finite value in [{SMOOTH_EPS_RANGE[0]}, {SMOOTH_EPS_RANGE[1]}]")


def guided_smooth(result, content, radius=None, eps=DEFAULT_SMOOTH_EPS) -> torch.Tensor:
    """--photo_smooth: the guided filter (He, Sun, Tang 2013) of `result` with `content` as colour guide, which puts the
    content's edges back into the result (strotss_guided_smooth; not clamped).  Two images of one size, (h, w, 3) or
    (1, h, w, 3) -> the result's shape.  radius None: default_smooth_radius(h, w).  ValueError when the sizes differ, for a
    radius outside 1..64, for an eps that is not finite or outside [1e-4, 1]."""
    check_smooth_parameters(radius, eps)
    r, c = _rgb(result, "result"), _rgb(content, "content")
    if tuple(r.shape) != tuple(c.shape):
        raise ValueError(f"result of shape {tuple(r.shape)} and content of shape {tuple(c.shape)} differ in size")
    if radius is None:
        radius = default_smooth_radius(int(r.shape[0]), int(r.shape[1]))
    out = _ops.guided_smooth(r, c, int(radius), float(eps))
    return out.reshape(tuple(result.shape)) if torch.is_tensor(result) else out


# ----------------------------------------------------------------------------- guided upsampling
UPSAMPLE_MODES = ("residual", "guided")
DEFAULT_UPSAMPLE_EPS = 1e-3              # residual: about 0.03^2, the guide explains weaker edges and less is left to the
#                                          interpolated residual; a documented choice, not tuned.  guided: DEFAULT_SMOOTH_EPS
UPSAMPLE_SIZE_RANGE = (64, 16384)        # --output_size in pixels


def default_upsample_eps(mode: str) -> float:
    return DEFAULT_UPSAMPLE_EPS if mode == "residual" else DEFAULT_SMOOTH_EPS


def check_upsample_sizes(h: int, w: int, H: int, W: int) -> None:
    """ValueError for a target (H, W) smaller than the result (h, w) in either dimension or with 3 H W > INT_MAX"""
    if H < h or W < w:
        raise ValueError(f"upsampling target {H} x {W} is smaller than the result {h} x {w}")
    if 3 * H * W > 2 ** 31 - 1:
        raise ValueError(f"upsampling target {H} x {W}: 3 H W exceeds {2 ** 31 - 1}")


def guided_upsample(result, content_lo, content_hi, radius=None, eps=None, mode="residual") -> torch.Tensor:
    """--output_size: `result` (h, w, 3) or (1, h, w, 3) brought to the size of `content_hi` (H, W, 3) or (1, H, W, 3) by
    joint upsampling with the content as guide (He and Sun 2015; strotss_guided_upsample; not clamped): the guided
    filter's coefficients of (result, content_lo) at the result's size, interpolated and applied to content_hi; mode
    "residual" adds the interpolated result - filter(result), which keeps the optimiser's texture, "guided" does not.
    -> (H, W, 3), with the leading 1 when the result has one.  radius None: default_smooth_radius(h, w); eps None: 1e-3 for
    residual, DEFAULT_SMOOTH_EPS for guided.  ValueError for an unknown mode, result and content_lo of different sizes, a
    content_hi smaller than the result in either dimension, 3 H W > INT_MAX, a radius outside 1..64, an eps that is not
    finite or outside [1e-4, 1]."""
    if mode not in UPSAMPLE_MODES:
        raise ValueError(f"upsampling mode {mode!r}: expected one of {UPSAMPLE_MODES}")
    check_smooth_parameters(radius, eps)
    r, lo, hi = _rgb(result, "result"), _rgb(content_lo, "content at the result's size"), _rgb(content_hi, "content")
    if tuple(r.shape) != tuple(lo.shape):
        raise ValueError(f"result of shape {tuple(r.shape)} and content of shape {tuple(lo.shape)} differ in size")
    check_upsample_sizes(int(r.shape[0]), int(r.shape[1]), int(hi.shape[0]), int(hi.shape[1]))
    if radius is None:
        radius = default_smooth_radius(int(r.shape[0]), int(r.shape[1]))
    if eps is None:
        eps = default_upsample_eps(mode)
    out = _ops.guided_upsample(r, lo, hi, int(radius), float(eps), mode)
    return out[None] if torch.is_tensor(result) and result.dim() == 4 else out


# ----------------------------------------------------------------------------- automatic region masks
AUTO_MASK_ITERS = 16                     # k-means iterations, fixed (no convergence test: no host synchronisation)
AUTO_MASK_SIZE = 256                     # long side at which the two images are clustered
AUTO_MASK_GRID = 64                      # grid points per image along its long side at most
AUTO_MASK_MIN_SHARE = 1.0 / 32.0         # a cluster is a region when it holds this share of BOTH images' grid points
AUTO_MASK_RANGE = (2, 8)                 # --auto_masks K: the colour-coded mask format tells eight colours apart
MASK_COLOURS = tuple((r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255))      # ascending (r, g, b)


def farthest_first(x: torch.Tensor, inv_norm: torch.Tensor, n: int, d: int, k: int) -> torch.Tensor:
    """(k, ld) initial centres, deterministic, on the device: centre 0 is the unit row with the largest cosine to the
    normalised sum of all unit rows (strotss_kmeans_update with one cluster, strotss_kmeans_assign against it), centre j the
    unit row whose largest cosine to centres 0..j-1 (the `best` of strotss_kmeans_assign) is smallest.  torch.argmax /
    argmin return the lowest index among equal values (tests/test_hip_cluster.py asserts it on the device)."""
    centres = torch.zeros((k, int(x.shape[1])), dtype=torch.float32, device=x.device)
    everyone = torch.zeros(n, dtype=torch.int32, device=x.device)
    _ops.kmeans_update(x, inv_norm, everyone, n, d, 1, centres)
    _, best, _ = _ops.kmeans_assign(x, inv_norm, n, d, centres, 1)
    row = torch.argmax(best).reshape(1)
    for j in range(k):                                       # index_select: the row number never leaves the device
        centres[j] = (x.index_select(0, row) * inv_norm.index_select(0, row))[0]
        if j + 1 < k:
            _, best, _ = _ops.kmeans_assign(x, inv_norm, n, d, centres, j + 1)
            row = torch.argmin(best).reshape(1)
    return centres


def label_counts(label: torch.Tensor, k: int) -> torch.Tensor:
    """(k,) int32 on the device: how many labels equal 0, 1, .., k-1 (torch.bincount would read the largest label back)"""
    return (label[:, None] == torch.arange(k, dtype=label.dtype, device=label.device)).sum(dim=0).to(torch.int32)


def spherical_kmeans(x: torch.Tensor, n: int, d: int, k: int, iters: int = AUTO_MASK_ITERS,
                     inv_norm: Optional[torch.Tensor] = None):
    """Spherical k-means of the first n rows (d columns) of a zero-padded (rows, ld) feature buffer, in the cosine metric of
    the style term: farthest_first centres, one assignment, then `iters` times (centre update, assignment) -- a fixed
    count, nothing is read back.  -> (label (n,) int32, centres (k, ld) unit or zero rows, count (k,) int32 of the labels
    returned, objective (iters,) = the mean of each assignment's best cosine, never decreasing), all on the device.  The
    labels are the assignment against the centres returned."""
    if not 1 <= int(k) <= _ops._hip.KMEANS_MAX_K:
        raise ValueError(f"{k} clusters: expected 1..{_ops._hip.KMEANS_MAX_K}")
    if inv_norm is None:
        inv_norm = _ops.row_inv_norm(x, n)
    centres = farthest_first(x, inv_norm, n, d, k)
    label, best, _ = _ops.kmeans_assign(x, inv_norm, n, d, centres, k)
    objective = torch.empty(iters, dtype=torch.float32, device=x.device)
    for it in range(iters):
        _ops.kmeans_update(x, inv_norm, label, n, d, k, centres)
        label, best, _ = _ops.kmeans_assign(x, inv_norm, n, d, centres, k)
        objective[it] = best.mean()
    count = label_counts(label, k)
    return label, centres, count, objective


def auto_mask_grid(h: int, w: int) -> Tuple[np.ndarray, np.ndarray]:
    """(rows, columns) of the clustering grid of an (h, w) image: stride g = ceil(long side / 64), from g // 2"""
    g = -(-max(int(h), int(w)) // AUTO_MASK_GRID)
    return np.arange(g // 2, int(h), g), np.arange(g // 2, int(w), g)


def upsample_labels(grid: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """a (gh, gw) label grid at (H, W) by nearest neighbour: pixel (y, x) takes cell (min(y gh // H, gh-1), min(x gw // W, gw-1))"""
    gh, gw = int(grid.shape[0]), int(grid.shape[1])
    ys = torch.clamp(torch.arange(H, device=grid.device) * gh // H, max=gh - 1)
    xs = torch.clamp(torch.arange(W, device=grid.device) * gw // W, max=gw - 1)
    return grid[ys][:, xs]


def _joint_rows(params, content: torch.Tensor, style: torch.Tensor):
    """The hypercolumn rows of both images' clustering grids: each image resized to AUTO_MASK_SIZE, one trunk forward, one
    gather -> (rows = the zero-padded (pad32(n_c + n_s), ld) buffer, content rows first, inv_norm, n_c, n_s, d,
    grids = [(gh, gw)] * 2, sizes = [(h, w) of the resized image] * 2)"""
    from . import engine
    grids, sizes, blocks, d = [], [], [], 0
    for image in (content, style):
        small = utils.resize(image, min(AUTO_MASK_SIZE, max(int(image.shape[-3]), int(image.shape[-2]))))
        if small.dim() == 3:
            small = small[None]
        feats = engine.extract_features(params, small.contiguous())
        ys, xs = auto_mask_grid(int(small.shape[1]), int(small.shape[2]))
        idx = np.stack(np.meshgrid(ys, xs, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float32)      # (row, col), row-major
        grids.append((len(ys), len(xs)))
        sizes.append((int(small.shape[1]), int(small.shape[2])))
        blocks.append((feats, torch.from_numpy(idx).to(small.device)))
        d = sum(int(m.shape[-1]) for m in feats)
    n_c, n_s = (g[0] * g[1] for g in grids)
    rows = torch.zeros((_ops.pad32(n_c + n_s), _ops.pad32(d)), dtype=torch.float32, device=blocks[0][1].device)
    _ops.hypercol_gather(blocks[0][0], blocks[0][1], False, out=rows)
    _ops.hypercol_gather(blocks[1][0], blocks[1][1], False, out=rows[n_c:])
    return rows, _ops.row_inv_norm(rows, n_c + n_s), n_c, n_s, d, grids, sizes


def auto_mask_regions(params, content: torch.Tensor, style: torch.Tensor, k: int, min_share: float = AUTO_MASK_MIN_SHARE):
    """The clustering behind auto_masks, with everything the tests look at: dict(kept = number of regions (0: fewer than
    two clusters hold min_share of both images' grid points), content_grid / style_grid = (gh, gw) int32 label grids over the
    kept clusters, centres (kept, ld), rows = the (n_c + n_s, ld) hypercolumn buffer (content rows first), inv_norm, n_c,
    n_s, d, shares (kept, 2) of the two images' points per region).  One device-to-host read: the (2, k) counts."""
    lo, hi = 1, _ops._hip.KMEANS_MAX_K
    if not lo <= int(k) <= hi:
        raise ValueError(f"{k} clusters: expected {lo}..{hi}")
    rows, inv_norm, n_c, n_s, d, grids, _ = _joint_rows(params, content, style)
    n = n_c + n_s
    label, centres, _, _ = spherical_kmeans(rows, n, d, int(k), inv_norm=inv_norm)
    counts = torch.stack([label_counts(label[:n_c], k), label_counts(label[n_c:], k)]).cpu().numpy()
    keep = np.flatnonzero((counts[0] >= min_share * n_c) & (counts[1] >= min_share * n_s))
    out = dict(kept=0, rows=rows, inv_norm=inv_norm, n_c=n_c, n_s=n_s, d=d, counts=counts)
    if keep.size < 2:
        return out
    if keep.size < k:                                        # every point into a kept cluster (ascending cluster order)
        centres = centres[torch.from_numpy(keep).to(centres.device)].contiguous()
        label, _, _ = _ops.kmeans_assign(rows, inv_norm, n, d, centres, int(keep.size))
    out.update(kept=int(keep.size), centres=centres, content_grid=label[:n_c].reshape(grids[0]),
               style_grid=label[n_c:].reshape(grids[1]))
    return out


# mask refinement: three documented choices, none tuned
REFINE_RADIUS = 2                        # a 5 x 5 window of cells around the pixel's own
REFINE_SIGMA_S = 1.0                     # in cells
REFINE_SIGMA_R = 0.1                     # on [0, 1] colours: the 0.1 behind DEFAULT_SMOOTH_EPS = 0.1^2
REFINE_SIGMA_RANGE = (0.01, 1.0)         # --refine_sigma


def check_refine_sigma(sigma_r) -> None:
    """ValueError for a colour sigma that is not finite or outside [0.01, 1] (None: not given)"""
    lo, hi = REFINE_SIGMA_RANGE
    if sigma_r is not None and not (math.isfinite(sigma_r) and lo <= sigma_r <= hi):
        raise ValueError(f"refinement sigma {sigma_r!r}: expected a finite value in [{lo}, {hi}]")


def refine_labels(image, grid: torch.Tensor, k: int, sigma_r: float = REFINE_SIGMA_R):
    """--refine_masks for one image: its (gh, gw) int32 label grid over the regions 0..k-1 brought to the image's size by
    joint bilateral upsampling with the image itself as guide (strotss_refine_labels at REFINE_RADIUS and REFINE_SIGMA_S):
    every pixel takes the label with the largest vote among the 5 x 5 cells around its own, a cell counting for more when
    it is near and when its mean colour is like the pixel's.  image: (H, W, 3) or (1, H, W, 3) in [0, 1] -> (labels (H, W)
    int32, count (k,) int32 pixels per label), both on the device.  ValueError: a sigma outside [0.01, 1], k outside 1..16,
    a grid that is not two-dimensional or larger than the image."""
    check_refine_sigma(sigma_r)
    if not 1 <= int(k) <= _ops._hip.KMEANS_MAX_K:
        raise ValueError(f"{k} regions: expected 1..{_ops._hip.KMEANS_MAX_K}")
    x = _rgb(image, "image")
    if grid.dim() != 2 or int(grid.shape[0]) > int(x.shape[0]) or int(grid.shape[1]) > int(x.shape[1]):
        raise ValueError(f"a label grid of shape {tuple(grid.shape)} for an image of {tuple(x.shape[:2])}: expected (gh, gw), "
                         f"not larger than the image")
    label, count, _, _, _ = _ops.refine_labels(x, grid.to(device=x.device, dtype=torch.int32).contiguous(), int(k),
                                               REFINE_RADIUS, REFINE_SIGMA_S, float(sigma_r))
    return label, count


def masks_from_grids(content, style, content_grid: torch.Tensor, style_grid: torch.Tensor, kept: int, refine=None,
                     min_share: float = AUTO_MASK_MIN_SHARE):
    """(content_masks, style_masks): `kept` (H, W, 1) float 0/1 masks per image in ascending region order, a partition of
    each image, from the two label grids.  refine None: nearest neighbour (upsample_labels).  refine = sigma_r: each grid is
    refined against its own image (refine_labels) and the two (kept,) pixel counts are read back; when a region then holds
    fewer than min_share of either image's pixels -- an emptied region must never reach the masked draw -- a warning is
    logged and both images keep their unrefined masks."""
    pairs = ((content, content_grid), (style, style_grid))
    labels = [upsample_labels(grid, int(image.shape[-3]), int(image.shape[-2])) for image, grid in pairs]
    if refine is not None:
        refined = [refine_labels(image, grid, kept, refine) for image, grid in pairs]
        counts = torch.stack([count for _, count in refined]).cpu().numpy()
        pixels = [int(image.shape[-3]) * int(image.shape[-2]) for image, _ in pairs]
        if all((counts[i] >= min_share * pixels[i]).all() for i in range(2)):
            labels = [label for label, _ in refined]
        else:
            utils.logger.warning(f"--refine_masks: a region would hold fewer than {min_share:.3f} of an image's pixels "
                                 f"(content {counts[0].tolist()} of {pixels[0]}, style {counts[1].tolist()} of {pixels[1]}); "
                                 f"keeping the unrefined masks")
    return tuple([(lab == j).float()[..., None] for j in range(kept)] for lab in labels)


def auto_masks(params, content: torch.Tensor, style: torch.Tensor, k: int, min_share: float = AUTO_MASK_MIN_SHARE,
               refine=None):
    """--auto_masks K: (content_masks, style_masks) as load_mask returns them -- lists of (H, W, 1) float 0/1 tensors at the
    two images' own sizes, one pair per region, each list a partition of its image -- from a joint spherical k-means of both
    images' hypercolumns (auto_mask_regions): cluster j is content region j and the style region it draws from.  Fewer than
    two clusters with min_share of both images: ([None], [None]) and a warning (the run proceeds unmasked).  refine: None
    brings the label grids to the images by nearest neighbour; a colour sigma (--refine_masks) by
    joint bilateral upsampling against each image itself (masks_from_grids)."""
    check_refine_sigma(refine)
    found = auto_mask_regions(params, content, style, k, min_share)
    if not found["kept"]:
        utils.logger.warning(f"--auto_masks {k}: fewer than two clusters hold {min_share:.3f} of both images "
                             f"(content {found['counts'][0].tolist()}, style {found['counts'][1].tolist()} of "
                             f"{found['n_c']}, {found['n_s']} points); running unmasked")
        return [None], [None]
    return masks_from_grids(content, style, found["content_grid"], found["style_grid"], found["kept"], refine, min_share)


def save_masks(directory: str, content_masks, style_masks) -> None:
    """--save_masks: content_mask.png and style_mask.png in `directory`, region r painted in MASK_COLOURS[r] -- the format
    load_mask reads, in the order it returns them (ascending (r, g, b)).  The masks of auto_masks are a partition, so every
    pixel gets the colour of its one region."""
    from PIL import Image
    if len(content_masks) > len(MASK_COLOURS):
        raise ValueError(f"{len(content_masks)} regions: the colour-coded format tells {len(MASK_COLOURS)} apart")
    os.makedirs(directory, exist_ok=True)
    palette = torch.tensor(MASK_COLOURS, dtype=torch.uint8)
    for name, masks in (("content_mask.png", content_masks), ("style_mask.png", style_masks)):
        region = torch.stack([m.reshape(m.shape[0], m.shape[1]) for m in masks]).argmax(dim=0).cpu()
        Image.fromarray(palette[region].numpy(), "RGB").save(os.path.join(directory, name), format="PNG")


# ----------------------------------------------------------------------------- scribble masks
# four documented choices, none tuned
SCRIBBLE_TAU = 0.05                      # temperature of the unary's softmax over the cosines
SCRIBBLE_LAMBDA = 0.05                   # the pull toward the unary, against edge weights of at most 1 per neighbour
SCRIBBLE_ITERS = 128                     # Jacobi sweeps
SCRIBBLE_SIGMA = REFINE_SIGMA_R          # on [0, 1] colours
SCRIBBLE_SIGMA_RANGE = (0.01, 1.0)       # --scribble_sigma
SCRIBBLE_ITERS_RANGE = (1, 1024)         # --scribble_iters (STROTSS_SCRIBBLE_MAX_ITERS)
SCRIBBLE_RANGE = (2, 7)                  # regions: the eight corner colours without black ("no stroke")


def check_scribble_parameters(sigma, iters) -> None:
    """ValueError for a colour sigma that is not finite or outside [0.01, 1], or a sweep count that is no integer in
    1..1024 (None: not given)"""
    lo, hi = SCRIBBLE_SIGMA_RANGE
    if sigma is not None and not (math.isfinite(sigma) and lo <= sigma <= hi):
        raise ValueError(f"scribble sigma {sigma!r}: expected a finite value in [{lo}, {hi}]")
    lo, hi = SCRIBBLE_ITERS_RANGE
    if iters is not None and not (int(iters) == iters and lo <= int(iters) <= hi):
        raise ValueError(f"{iters!r} scribble sweeps: expected {lo}..{hi}")


def _stroke_colours(path: str) -> np.ndarray:
    """(h, w) int64 per pixel of a stroke image: the index into MASK_COLOURS of its colour under the mask loader's
    threshold rule (a channel counts when it is 255); 0 is black, "no stroke".  Host only."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"File not found: {path}")
    from PIL import Image
    with Image.open(path) as im:
        q = (np.array(im.convert("RGB")) // 255).astype(np.int64)
    return q[..., 0] * 4 + q[..., 1] * 2 + q[..., 2]


def load_scribbles(content_path: str, style_path: str):
    """--content_scribbles / --style_scribbles: two RGB images in the corner-colour format of MASK_COLOURS, black meaning
    "no stroke" -> (content strokes, style strokes, colours): (h, w) int32 host arrays at the files' own sizes, region r
    (the r-th non-black colour present, ascending (r, g, b)) on its strokes and -1 elsewhere, and the regions' colours.
    ValueError: a colour present in one file only, fewer than two colours."""
    found = [_stroke_colours(content_path), _stroke_colours(style_path)]
    present = [sorted(set(np.unique(f).tolist()) - {0}) for f in found]
    if present[0] != present[1]:
        only = sorted(set(present[0]) ^ set(present[1]))
        raise ValueError(f"scribbles: the colours {[MASK_COLOURS[c] for c in only]} are present in one file only "
                         f"({content_path}, {style_path}); every region needs a stroke in both images")
    if len(present[0]) < SCRIBBLE_RANGE[0]:
        raise ValueError(f"scribbles: {len(present[0])} stroke colours in {content_path}; expected {SCRIBBLE_RANGE[0]}.."
                         f"{SCRIBBLE_RANGE[1]} of the corner colours {MASK_COLOURS[1:]}")
    lut = np.full(len(MASK_COLOURS), -1, dtype=np.int32)
    lut[present[0]] = np.arange(len(present[0]), dtype=np.int32)
    return lut[found[0]], lut[found[1]], [MASK_COLOURS[c] for c in present[0]]


def resize_strokes(strokes: np.ndarray, H: int, W: int) -> np.ndarray:
    """(h, w) stroke labels at (H, W) by nearest neighbour: pixel (y, x) takes (y h // H, x w // W)"""
    h, w = strokes.shape
    return np.ascontiguousarray(strokes[np.arange(H) * h // H][:, np.arange(W) * w // W])


def scribble_seeds(strokes: np.ndarray, k: int) -> np.ndarray:
    """(gh, gw) int32 seed labels of the clustering grid (auto_mask_grid) of a small image from its (h, w) stroke labels:
    per cell the majority label among the stroke pixels of its g x g block (rows i g .. i g + g - 1), the lowest label on a
    tie, -1 without a stroke pixel.  Host only: at most 256 x 256 pixels."""
    h, w = strokes.shape
    g = -(-max(h, w) // AUTO_MASK_GRID)
    ys, xs = auto_mask_grid(h, w)
    gh, gw = len(ys), len(xs)
    yy, xx = np.nonzero((strokes >= 0) & (strokes < k))
    inside = (yy // g < gh) & (xx // g < gw)
    yy, xx = yy[inside], xx[inside]
    votes = np.zeros((gh, gw, k), dtype=np.int64)
    np.add.at(votes, (yy // g, xx // g, strokes[yy, xx]), 1)
    return np.where(votes.sum(axis=2) > 0, votes.argmax(axis=2), -1).astype(np.int32)        # argmax: the first of equal counts


def scribble_regions(params, content: torch.Tensor, style: torch.Tensor, content_strokes: np.ndarray,
                     style_strokes: np.ndarray, k: int, sigma: float = SCRIBBLE_SIGMA, iters: int = SCRIBBLE_ITERS,
                     tau: float = SCRIBBLE_TAU, lam: float = SCRIBBLE_LAMBDA, iters_per_launch: int = 0, planes: bool = False):
    """The propagation behind scribble_masks, with everything the tests look at.  The strokes (host label arrays of any
    size, load_scribbles) are brought to each image's size and to its AUTO_MASK_SIZE copy by nearest neighbour; the cells of
    the two clustering grids that a stroke crosses seed k centres (one strotss_kmeans_update over both images' rows); every
    cell's cosines to the centres (strotss_kmeans_scores) are the unary of a screened random walker on each image, whose
    strokes are fixed (strotss_scribble_labels).  -> dict(k, rows, inv_norm, n_c, n_s, d, seeds = [(gh, gw) int32] * 2 on
    the host, centres (k, ld), scores (n_c + n_s, k), grid_scores / strokes / labels / x = [content's, style's] on the
    device ((gh, gw, k), (H, W) int32, (H, W) int32, (k, H, W) or None), counts (2, k) pixels per region, read back).
    ValueError: k outside 2..7, bad parameters, a region that seeds no cell in either image -- nearest-neighbour sampling
    of the stroke file keeps every stroke that is at least (file's longer side) / AUTO_MASK_SIZE pixels wide; a thinner one
    may fall between the samples."""
    lo, hi = SCRIBBLE_RANGE
    if not lo <= int(k) <= hi:
        raise ValueError(f"{k} regions: expected {lo}..{hi}")
    check_scribble_parameters(sigma, iters)
    k = int(k)
    rows, inv_norm, n_c, n_s, d, grids, sizes = _joint_rows(params, content, style)
    n = n_c + n_s
    seeds = [scribble_seeds(resize_strokes(strokes, *size), k) for strokes, size in zip((content_strokes, style_strokes), sizes)]
    joint = np.concatenate([seed.reshape(-1) for seed in seeds])
    missing = [r for r in range(k) if not (joint == r).any()]
    if missing:
        raise ValueError(f"scribbles: the strokes of region(s) {missing} cover no cell of either image's {AUTO_MASK_GRID}-cell "
                         f"grid (stroke too thin at {AUTO_MASK_SIZE} px: the stroke file is sampled by nearest neighbour at "
                         f"the image's size and at its {AUTO_MASK_SIZE}-px copy, so draw strokes at least 1/{AUTO_MASK_SIZE} of "
                         f"the file's longer side wide, e.g. 8 pixels on a 2048-pixel file)")
    centres = torch.zeros((k, int(rows.shape[1])), dtype=torch.float32, device=rows.device)
    _ops.kmeans_update(rows, inv_norm, torch.from_numpy(joint).to(rows.device), n, d, k, centres)      # -1: skipped
    scores = _ops.kmeans_scores(rows, inv_norm, n, d, centres, k)
    out = dict(k=k, rows=rows, inv_norm=inv_norm, n_c=n_c, n_s=n_s, d=d, seeds=seeds, centres=centres, scores=scores,
               grid_scores=[], strokes=[], labels=[], x=[])
    counts = []
    for image, strokes, part, grid in ((content, content_strokes, scores[:n_c], grids[0]),
                                       (style, style_strokes, scores[n_c:], grids[1])):
        img = _rgb(image, "image")
        grid_scores = part.reshape(grid[0], grid[1], k).clone()              # its own allocation: 16-byte aligned
        on_image = torch.from_numpy(resize_strokes(strokes, int(img.shape[0]), int(img.shape[1]))).to(img.device)
        label, count, x = _ops.scribble_labels(img, on_image, grid_scores, tau, lam, sigma, int(iters), iters_per_launch, planes)
        out["grid_scores"].append(grid_scores)
        out["strokes"].append(on_image)
        out["labels"].append(label)
        out["x"].append(x)
        counts.append(count)
    out["counts"] = torch.stack(counts).cpu().numpy()
    return out


def scribble_masks(params, content: torch.Tensor, style: torch.Tensor, content_strokes: np.ndarray, style_strokes: np.ndarray,
                   k: int, colours=None, sigma: float = SCRIBBLE_SIGMA, iters: int = SCRIBBLE_ITERS,
                   min_share: float = AUTO_MASK_MIN_SHARE):
    """--content_scribbles / --style_scribbles: (content_masks, style_masks) as load_mask returns them -- k (H, W, 1) float
    0/1 masks per image in ascending colour order, a partition of each image -- from a few strokes per image
    (scribble_regions).  The strokes are the user's statement: a region left with fewer than min_share of either image's
    pixels is a ValueError that names its colour (colours: the regions' (r, g, b), load_scribbles), never a fallback."""
    found = scribble_regions(params, content, style, content_strokes, style_strokes, k, sigma, iters)
    for i, (name, label) in enumerate(zip(("content", "style"), found["labels"])):
        pixels = int(label.numel())
        for r in np.flatnonzero(found["counts"][i] < min_share * pixels):
            colour = f"region {r}" if colours is None else f"the region of colour {tuple(colours[r])}"
            raise ValueError(f"scribbles: {colour} holds {int(found['counts'][i][r])} of the {name} image's {pixels} pixels, "
                             f"fewer than {min_share:.3f} of them; draw a longer stroke or drop the colour")
    return tuple([(label == r).float()[..., None] for r in range(k)] for label in found["labels"])


# ----------------------------------------------------------------------------- region tracking
MASK_INERTIA = 0.05                      # beta of --track_masks: a documented choice, not tuned
MASK_INERTIA_RANGE = (0.0, 2.0)          # cosines lie in [-1, 1]: 2 never changes a label that has a prior


def check_mask_inertia(beta) -> None:
    """ValueError for an inertia that is not finite or outside [0, 2] (None: not given)"""
    lo, hi = MASK_INERTIA_RANGE
    if beta is not None and not (math.isfinite(beta) and lo <= beta <= hi):
        raise ValueError(f"mask inertia {beta!r}: expected a finite value in [{lo}, {hi}]")


def frame_rows(params, frame: torch.Tensor):
    """The content half of what auto_mask_regions gathers, for one frame: dict(rows = the zero-padded (pad32(n), ld)
    hypercolumn buffer of the frame's clustering grid, inv_norm, n, d, grid = (gh, gw), size = (h, w) of the image the grid
    lies on).  One trunk forward at
    AUTO_MASK_SIZE; the rows are bit for bit the content rows of auto_mask_regions on the same image."""
    from . import engine
    small = utils.resize(frame, min(AUTO_MASK_SIZE, max(int(frame.shape[-3]), int(frame.shape[-2]))))
    if small.dim() == 3:
        small = small[None]
    feats = engine.extract_features(params, small.contiguous())
    ys, xs = auto_mask_grid(int(small.shape[1]), int(small.shape[2]))
    idx = np.stack(np.meshgrid(ys, xs, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float32)          # (row, col), row-major
    n, d = len(ys) * len(xs), sum(int(m.shape[-1]) for m in feats)
    rows = torch.zeros((_ops.pad32(n), _ops.pad32(d)), dtype=torch.float32, device=small.device)
    _ops.hypercol_gather(feats, torch.from_numpy(idx).to(small.device), False, out=rows)
    return dict(rows=rows, inv_norm=_ops.row_inv_norm(rows, n), n=n, d=d, grid=(len(ys), len(xs)),
                size=(int(small.shape[1]), int(small.shape[2])))


def tracking_state(found) -> dict:
    """The state of frame 1 from its auto_mask_regions result (kept >= 2): dict(kept, centres (kept, ld), grid = G_1 over all
    kept regions, present = the regions of this frame (all of them), mask_grid = the grid over the present regions)"""
    kept = int(found["kept"])
    grid = found["content_grid"].clone()                     # its own allocation: the library wants it 16-byte aligned
    return dict(kept=kept, centres=found["centres"], grid=grid, present=list(range(kept)), mask_grid=grid)


def track_regions(state: dict, params, frame: torch.Tensor, flow: Optional[torch.Tensor], certainty: Optional[torch.Tensor],
                  beta: float = MASK_INERTIA, min_share: float = AUTO_MASK_MIN_SHARE) -> dict:
    """The regions of one frame after the first.  state: the state of the earlier frame the prior is
    taken from (tracking_state for frame 1, or what this function returned); flow (h, w, 2), certainty (h, w) or None: the
    backward flow of this frame against that one and its certainty, at the results' size (brought to the clustering
    image's size when the grid has more points than they have pixels); flow None: no prior (every cell -1).  Every cell of the
    frame's clustering grid is assigned to one of the fixed centres of frame 1, `beta` added to the cosine of the label its
    scene point had in the earlier frame (strotss_label_warp, strotss_kmeans_assign_prior) -> grid = G_t over all kept
    regions.  The counts of G_t are read back (the one device-to-host read): a region below min_share of the grid points
    is absent from this frame and its cells are reassigned among the present ones (a second biased assignment against the
    present centres) -> mask_grid over the labels 0..len(present)-1.  Returns the new state; fewer than two present
    regions: present = [] and mask_grid = None (the frame runs unmasked)."""
    check_mask_inertia(beta)
    kept, centres = int(state["kept"]), state["centres"]
    got = frame_rows(params, frame)
    shape, n, d = got["grid"], got["n"], got["d"]
    if shape != tuple(state["grid"].shape):
        raise ValueError(f"a clustering grid of {shape} after one of {tuple(state['grid'].shape)}: the frames differ in size")
    if flow is None:
        prior = torch.full(shape, -1, dtype=torch.int32, device=centres.device)
    else:
        if int(flow.shape[0]) < shape[0] or int(flow.shape[1]) < shape[1]:      # results smaller than the clustering image
            hs, ws = got["size"]                                                # (the coarse levels): the grid fits that one
            if certainty is not None:
                certainty = _ops.resize_bilinear(certainty.float().reshape(int(flow.shape[0]), int(flow.shape[1]), 1)
                                                 .contiguous(), hs, ws).reshape(hs, ws)
            flow = resize_flow(flow, hs, ws).contiguous()
        prior = _ops.label_warp(state["grid"].contiguous(), kept, flow, certainty)
    label, _, _ = _ops.kmeans_assign_prior(got["rows"], got["inv_norm"], n, d, centres, kept, prior.reshape(-1), float(beta))
    counts = label_counts(label, kept).cpu().numpy()
    present = [int(r) for r in np.flatnonzero(counts >= min_share * n)]
    out = dict(kept=kept, centres=centres, grid=label.reshape(shape), present=present, mask_grid=label.reshape(shape),
               prior=prior, counts=counts)
    if len(present) < 2:
        out.update(present=[], mask_grid=None)
    elif len(present) < kept:                                # the absent regions' cells go to a present one
        lut = torch.full((kept + 1,), -1, dtype=torch.int32)
        lut[torch.tensor(present) + 1] = torch.arange(len(present), dtype=torch.int32)
        sub_prior = lut.to(prior.device)[(prior.reshape(-1) + 1).long()].contiguous()
        sub_centres = centres[torch.tensor(present, device=centres.device)].contiguous()
        sub, _, _ = _ops.kmeans_assign_prior(got["rows"], got["inv_norm"], n, d, sub_centres, len(present), sub_prior,
                                             float(beta))
        out["mask_grid"] = sub.reshape(shape)
    return out


def masks_from_grid(image, grid: torch.Tensor, kept: int, refine=None, min_share: float = AUTO_MASK_MIN_SHARE):
    """masks_from_grids for one image: `kept` (H, W, 1) float 0/1 masks in ascending label order from its label grid, by
    nearest neighbour (refine None) or refined against the image itself (refine = sigma_r) with the same fallback: a
    region left with fewer than min_share of the pixels logs a warning and the unrefined masks are kept."""
    H, W = int(image.shape[-3]), int(image.shape[-2])
    label = upsample_labels(grid, H, W)
    if refine is not None:
        refined, count = refine_labels(image, grid, kept, refine)
        count = count.cpu().numpy()
        if (count >= min_share * H * W).all():
            label = refined
        else:
            utils.logger.warning(f"--refine_masks: a region would hold fewer than {min_share:.3f} of the frame's pixels "
                                 f"({count.tolist()} of {H * W}); keeping the unrefined masks")
    return [(label == j).float()[..., None] for j in range(kept)]


def save_region_image(path: str, masks, regions=None) -> None:
    """One colour-coded region image in the format of save_masks: the pixels of masks[i] painted in MASK_COLOURS[regions[i]]
    (regions None: 0, 1, ..), so that a region keeps its colour across the frames of a sequence while an absent one's colour
    does not occur."""
    from PIL import Image
    regions = list(range(len(masks))) if regions is None else [int(r) for r in regions]
    if len(regions) != len(masks) or any(not 0 <= r < len(MASK_COLOURS) for r in regions):
        raise ValueError(f"{len(masks)} masks for the regions {regions}: the colour-coded format tells {len(MASK_COLOURS)} apart")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    palette = torch.tensor(MASK_COLOURS, dtype=torch.uint8)[torch.tensor(regions)]
    region = torch.stack([m.reshape(m.shape[0], m.shape[1]) for m in masks]).argmax(dim=0).cpu()
    Image.fromarray(palette[region].numpy(), "RGB").save(path, format="PNG")


def _colour_keys(path: str, max_size: Optional[int], pixel_threth: int) -> np.ndarray:
    """(H, W) int64 key per pixel of a colour-coded region image: its channels floored to multiples of `pixel_threth`
    (uint8 as decoded, or float32 when `max_size` made load_image resize it) and packed so that ascending keys are
    ascending (r, g, b) triples."""
    img = utils.load_image(path, max_size, dtype=torch.uint8, batch_expand=False).cpu().numpy()
    q = (np.floor_divide(img, pixel_threth) * pixel_threth).astype(np.int64)
    return (q[..., 0] << 32) | (q[..., 1] << 16) | q[..., 2]


def load_mask(content_path: str, style_path: str, max_size: Optional[int],
              pixel_threth: int = 255, sample_threth: int = 10000):
    """reference strotss_utils.py:178-201: paired (H, W, 1) float 0/1 region masks from two colour-coded images -- one
    pair per colour that covers at least `sample_threth` content pixels and occurs in the style image too, in ascending
    (r, g, b) order; bare Exception('No mask found') when there is none."""
    c_keys = _colour_keys(content_path, max_size, pixel_threth)
    s_keys = _colour_keys(style_path, max_size, pixel_threth)
    colours, counts = np.unique(c_keys, return_counts=True)
    chosen = colours[(counts >= sample_threth) & np.isin(colours, s_keys)]
    if chosen.size == 0:
        raise Exception('No mask found')

    def region(keys: np.ndarray, colour) -> torch.Tensor:
        return torch.from_numpy((keys == colour).astype(np.float32))[..., None]
    return [region(c_keys, c) for c in chosen], [region(s_keys, c) for c in chosen]
