"""STROTSS on MI355X -- the reference's command line and coarse-to-fine schedule on the HIP step engine.

    python run_strotss.py content_im.jpg style_im.jpg -o output.jpg
    python run_strotss.py c.jpg s.jpg -o out.jpg --content_mask cm.jpg --style_mask sm.jpg

Every reference flag is kept (run_strotss.py:165-178 there).  Additions:
  --start_level K   run only scales K..level-1 (0 = reference behaviour); the first executed scale is
                    initialised like the reference's first one and alpha starts at 16/2^K
  --seed, --weights PATH (.npz; the reference downloads vgg16_norm.h5, impossible offline -- without
                    --weights a seeded synthetic VGG is used)
  --log_every N     read the three scalars back every N steps (the reference formats them every step,
                    i.e. one device->host sync per step; default 10, 1 restores that)
  --no_graph        launch kernels one by one instead of replaying one hipGraph per step
  --style_mix P [P ...], --style_weights W [W ...]
                    style blending: stylise toward a weighted mix of style_path and the --style_mix images (1 + len(mix)
                    weights, default equal; normalised to sum to 1; zero-weight styles are dropped before they are loaded).
                    Not combined with masks or --strips.
  --content_weight_map PATH
                    per-pixel content strength: a greyscale image (white = keep the content, black = let it go), divided
                    by 255 and resized to every scale; weights each sample's column of the content term (DESIGN.md
                    section 11).  Combines with masks and --style_mix; not with --strips or a multi-process run.
  --sample_map PATH
                    where the step looks: a greyscale image, white samples densely and black is sampled only when nothing
                    else is left.  Divided by 255, resized to every scale and rounded to 16-bit levels; every step's 1024
                    sample coordinates are drawn with inclusion proportional to the level, inside the step's graph
                    (strotss_index_draw_weighted).  The sample count does not change.  Combines with
                    masks, --auto_masks, the scribble files, --style_mix, --content_weight_map, every transport and --video
                    (one map for every frame); not with --strips or a multi-process run.  The style's samples stay uniform.
                    --sample_map auto (the word in place of a path) computes the map from the content instead: a detail
                    map, the root of the windowed mean gradient energy of the content's luma over --sample_gain times its
                    image mean, clamped at 1 and lifted to --sample_floor (strotss_detail_map), at
                    the content's loaded size, once per image; with --video once per frame, so it follows what moves.
  --sample_radius R with --sample_map auto: the window radius in pixels, 1..64 (default: the longer side // 64, at least 1)
  --sample_gain G   with --sample_map auto: detail at G times the image's mean detail reaches level 1 (default 2, > 0; not
                    tuned for image quality)
  --sample_floor F  with --sample_map auto: the level of a flat region, 0..1 (default 0.25; not tuned for image quality)
  --save_sample_map DIR
                    with --sample_map auto: write the map to DIR as the 8-bit sample_map.png (with --video
                    sample_map_<frame stem>.png), which --sample_map PATH reads back
  --video           content_path is a directory of frames (sorted by name, all of one size) and -o an output directory:
                    frame <stem> is written as <stem>.jpg.  With --flow_dir DIR (backward_{t}_{t-1}.flo, optional
                    forward_{t-1}_{t}.flo and reliable_{t}_{t-1}.pgm, t the 1-based position of the frame: the naming of
                    the artistic-videos tools) every frame after the first is pulled toward the previous result warped
                    along the flow, weight --temporal_weight; --temporal_init starts a frame's
                    first executed scale from that warped result.  One GPU; not with --strips.
  --temporal_frames J [J ...]
                    with --video: long-term consistency, 1 to 4 distinct positive frame offsets
                    (default 1, the short-term term alone; Ruder et al. use 1 10 20 40).  Frame t is also pulled toward the
                    results of frames t-j, warped along backward_{t}_{t-j}.flo (forward_{t-j}_{t}.flo, reliable_{t}_{t-j}.pgm
                    as above), each only where no nearer frame covers the pixel; --temporal_init starts from the nearest.
  --compute_flow    with --video, instead of --flow_dir: the flows are computed on the GPU from the content frames at the
                    results' size (strotss_optical_flow, coarse-to-fine Horn-Schunck), backward and
                    forward for every --temporal_frames offset; no reliable_*.pgm is involved.  --flow_dir stays the way to
                    bring better flow from elsewhere.
  --flow_match [R]  with --compute_flow: a patch-matching stage in every computed flow: at each
                    pyramid level every pixel may move its flow by a whole offset of up to R pixels (1..4, 2 when R is
                    left out) if its 5 x 5 window matches better there -- for objects that move against their background
  --flow_robust     with --compute_flow: every computed flow is solved with robust (Charbonnier) penalties on the data and
                    the smoothness term (strotss_optical_flow_robust), so that an object moving against
                    its background keeps its motion; combines with --flow_match
  --flow_alpha A    with --flow_robust: its smoothness weight (finite, > 0; default 0.06)
  --flow_outer N    with --flow_robust: weight updates per warp (1..8, a divisor of the 32 sweeps; default 4)
  --save_flow DIR   with --compute_flow: also write the computed flows to DIR as backward_{t}_{t-j}.flo and
                    forward_{t-j}_{t}.flo (a later run with --flow_dir DIR reads the same floats back)
  --preserve_color {match,luminance,transfer}
                    keep the content's colours (Gatys et al. 2016).  match: every style image is
                    recoloured, before anything is sampled from it, with the affine map that gives it the content's colour
                    mean and covariance (each --style_mix image on its own; with masks region by region; with --video
                    against every frame's own colours).  luminance: the written image keeps the luma of the result and takes
                    the chroma of the content; with --video the temporal targets stay the unmerged results.  transfer:
                    where match recolours with one affine map, every style image is given the content's whole colour
                    distribution by iterative distribution transfer (Pitie, Kokaram and Dahyot 2007):
                    its pixels are rotated into an orthonormal colour basis, each axis is histogram-matched to the content,
                    and the loop repeats on the next basis; it runs where and as match runs (per --style_mix image, region by
                    region, per --video frame).  One GPU; not with --strips.
  --transfer_iters T
                    with --preserve_color transfer: the number of bases, 1..64 (default 10; the bases do not depend on --seed)
  --photo_smooth    keep the content's edges: the result is passed through the guided filter of He, Sun and Tang (2013) with
                    the content at the result's size as colour guide before --preserve_color
                    luminance's merge and before it is written; with --video the temporal targets stay the unfiltered
                    results.  One GPU; not with --strips.
  --smooth_radius R with --photo_smooth: the window radius in pixels, 1..64 (default: 1/64 of the result's longer side)
  --smooth_eps E    with --photo_smooth: the regulariser on [0, 1] colours, 1e-4..1 (default 1e-2); smaller keeps weaker edges
  --output_size SIZE
                    write the result at the content's own resolution: SIZE is `full` (the content
                    file as decoded) or a long side in pixels, 64..16384.  The guided filter's coefficients of the result
                    against the content are computed at the result's size, interpolated and applied to the content at the
                    target size (He and Sun 2015); after --photo_smooth, before --preserve_color luminance's merge, which
                    then runs at the target size.  In --video only what is written is upsampled.  One GPU; not with --strips.
  --upsample_mode {residual,guided}
                    with --output_size: residual (default) adds the interpolated difference between the result and its
                    filter, which keeps the optimiser's texture; guided is the filter alone
  --upsample_radius R, --upsample_eps E
                    with --output_size: the window radius at the result's size, 1..64 (default 1/64 of its longer side),
                    and the regulariser, 1e-4..1 (default 1e-3 for residual, 1e-2 for guided)
  --auto_masks K    region guidance without painted masks: the hypercolumns of the content and of
                    style_path on a regular grid are clustered jointly into K groups (2..8) by spherical k-means on the GPU;
                    every cluster that holds 1/32 of both images' grid points is a content region and the style region it
                    draws from, exactly as a pair of --content_mask / --style_mask colours is.  Computed on the images as
                    loaded (before --preserve_color match recolours the style, which then runs region by region).  Fewer
                    than two such clusters: a warning and an unmasked run.  Combines with --content_weight_map,
                    --preserve_color and --photo_smooth; not with --content_mask / --style_mask, --style_mix, --strips or a
                    multi-process run; with --video only together with --track_masks.
  --refine_masks    with --auto_masks: edge-aligned regions.  The label grid of each image is brought to
                    the image by joint bilateral upsampling with the image itself as guide instead of by nearest neighbour:
                    every pixel votes among the 5 x 5 grid cells around its own, a cell counting for more when it is near
                    and when its mean colour is like the pixel's.  The borders then follow the image's edges, not the
                    grid's blocks.  A region left with less than 1/32 of either image: a warning and the unrefined masks.
  --refine_sigma S  with --refine_masks: the colour scale of the vote on [0, 1] colours, 0.01..1 (default 0.1); smaller
                    follows weaker edges
  --save_masks DIR  with --auto_masks (or the scribble files): write the regions to DIR as content_mask.png and
                    style_mask.png in the colour-coded format of --content_mask / --style_mask (region r in the r-th of
                    the eight colours with channels in {0, 255}, ascending (r, g, b)), to be edited and handed back through
                    those two flags
  --content_scribbles C.png --style_scribbles S.png
                    region guidance from a few strokes per image.  Both files are RGB images in the
                    colour-coded format of --content_mask / --style_mask, of any size (they are brought to their image's
                    size by nearest neighbour, so a stroke should be at least 1/256 of the file's longer side wide, or it
                    may fall between the samples: an error then says so): black means "no stroke", each of the other seven corner colours is a region,
                    drawn as a short stroke on the content and one of the same colour on the style.  The cells of both
                    images' feature grids under the strokes give one centre per colour; every pixel's likeness to the
                    centres and the image's own edges then carry the strokes over the whole image (a screened random walker,
                    128 Jacobi sweeps on the GPU).  2..7 colours, every colour in both files.  A region left with less than
                    1/32 of either image is an error that names its colour.  --save_masks DIR writes the regions found.
                    Combines and excludes as --auto_masks does; not with --auto_masks or --video.
  --scribble_sigma S
                    with the scribble files: the colour scale of the edge weights on [0, 1] colours, 0.01..1 (default 0.1, not
                    tuned); smaller stops the strokes at weaker edges
  --scribble_iters T
                    with the scribble files: the number of sweeps, 1..1024 (default 128, not tuned)
  --track_masks     with --auto_masks K --video: the regions of the first frame followed through the sequence (DESIGN.md
                    section 19).  Frame 1 is clustered jointly with style_path as a single image is; its regions, their
                    centres and the style masks then stay.  Every later frame's grid cells are assigned to those centres,
                    the label that the same scene point had in the nearest earlier frame of --temporal_frames (followed
                    along the backward flow of --flow_dir / --compute_flow, where that flow is certain) preferred by
                    --mask_inertia.  A region below 1/32 of a frame's grid points is absent from that frame (its cells go
                    to the others) and may come back later.  --save_masks DIR then writes style_mask.png once and
                    content_mask_<frame stem>.png per frame, a region keeping its colour.
  --mask_inertia B  with --track_masks: what is added to the cosine of the prior label, 0..2 (default 0.05, not tuned); 0 is
                    the plain assignment to frame 1's centres, 2 never changes a label that has a prior
  --style_transport {remd,sinkhorn,sliced}
                    the transport term of the style loss.  remd (default): the relaxed EMD, every
                    row matched to its nearest neighbour on each side.  sinkhorn: the entropic transport cost between the
                    style's and the result's hypercolumns (cosine cost, uniform marginals, differentiated through the
                    scalings), which conserves mass -- the style's features are matched in proportion -- and costs about
                    60 more kernel launches per region and step.  Combines with masks, --style_mix, --content_weight_map
                    and --video; one GPU, not with --strips.
  --sinkhorn_reg L  with --style_transport sinkhorn: K = exp(-L * cost), finite and > 0 (default 10); larger is closer to
                    the unregularised plan and needs more scalings
  --sinkhorn_iters T
                    with --style_transport sinkhorn: the number of scalings, 1..64 (default 30)
  --sinkhorn_log    with --style_transport sinkhorn: the scalings in the log domain, for sharp plans:
                    the linear form is guaranteed free of its clamps only to --sinkhorn_reg 13.8, above it exp(-L * cost)
                    underflows and rows lose their gradient silently; this form has neither, for --sinkhorn_reg in (0, 1000]
                    sliced: the sliced Wasserstein distance -- both sets of L2-normalised
                    hypercolumns projected on P random sign directions (drawn on the device from --seed, fresh every step),
                    sorted and matched by rank, which is the exact transport in one dimension: mass-conserving like
                    sinkhorn, without a regulariser or an iteration count, in 7 launches per region and step.  Combines
                    and excludes as sinkhorn does.
  --sliced_projections P
                    with --style_transport sliced: the number of directions, 1..1024 (default 256, not tuned)
  --palette_transport {remd,sliced}
                    the palette term of the style loss.  remd (default): the relaxed EMD between the
                    YUV colours of the style's and the result's samples, every colour matched to its nearest neighbour: a
                    result with one blue sample among red ones matches a style that is half red and half blue at no
                    cost.  sliced: the sliced
                    Wasserstein distance between the two colour sets -- projected on P fixed directions, sorted and matched
                    by rank -- which conserves mass: the style's colours are matched in proportion.  2 launches per region
                    and step; with --style_transport remd the step then runs its separate loss launches, not the grouped 13.
                    Combines with masks, --auto_masks, the scribble files, --style_mix, --video, --content_weight_map and
                    every --style_transport; one GPU, not with --strips.
  --palette_projections P
                    with --palette_transport sliced: the number of directions, 1..1024 (default 64, not tuned for image
                    quality; a Fibonacci lattice on the hemisphere, the same on every step, independent of --seed)
  --strips          under torchrun (one process per GPU): ONE image on all GPUs -- every rank runs the trunk on its strip
                    of the image (+ halo) at the scales where that pays, two all-reduces per step (nn/parallel.py);
                    rank 0 writes the output
  --detail_weight W
                    a Laplacian detail term against the content: the result and the content are
                    average-pooled at every size of --detail_pool, the graph Laplacian of the pooled difference is
                    penalised, and its gradient joins the pixel gradient of every step -- edges, lettering and thin lines
                    finer than the sample spacing stay where the content has them.  Off unless given (finite, >= 0).  With
                    --content_weight_map the pooled map weighs the cells: white keeps the content's detail, black lets it
                    go.  Combines with masks, --auto_masks, the scribble files, --track_masks, --style_mix, every transport
                    flag, --preserve_color, --photo_smooth and --video (the target is the current frame's content); one
                    GPU, not with --strips.
  --detail_pool P [P ...]
                    with --detail_weight: 1..3 distinct pool sizes of {1, 2, 4, 8, 16}, ascending (default 1 4, not tuned)
  --tv_weight W     the total variation of the result, sqrt(dx^2 + dy^2 + (1/255)^2) per pixel and channel, as a term of
                    every step: penalises pixel-level grain.  Off unless given (finite, >= 0).
                    Combines as --detail_weight; one GPU, not with --strips.
  --photo_weight W  the photorealism term of Luan et al. (2017) in every step: the matting Laplacian of
                    the content (Levin et al. 2008) applied to the result -- the result may take any colours, but over every
                    (2R+1) x (2R+1) window it should be an affine function of the content's colours, so straight edges stay
                    straight and flat areas stay flat.  Off unless given (finite, >= 0).  Combines as --detail_weight,
                    --photo_smooth included (that filters the written result, this shapes every step); with --video the
                    guide is the current frame's content; one GPU, not with --strips.
  --photo_radius R  with --photo_weight: the window radius, 1..4 (default 1: the 3 x 3 windows of Luan et al.)
  --photo_eps E     with --photo_weight: the regulariser of the window covariances, 1e-4..1 (default 1e-4; a convention,
                    not tuned)
Under torchrun WITH masks (region-guided run, BASELINE config 4) the mask regions are dealt round-robin to the ranks:
every rank runs the replicated trunk forward, its own regions' samples + losses and their data-gradient, ONE RCCL
all-reduce sums the pixel gradient, every rank applies the identical update; rank 0 writes the output.
`--level` is coerced to int (the reference declares type=float, which breaks `range(args.level)`).
"""
import argparse
import os

import numpy as np
import torch

from nn import engine as strotss_engine
from nn import rand, utils
from nn import strotss_utils as strotss
from nn.losses import moment_matching, relaxed_emd, self_similarity, weighted_self_similarity
from nn.model import VGG

utils.make_logger('STROTSS')
tqdm = __import__('tqdm.notebook' if utils.is_jupyter_env() else 'tqdm', fromlist=['tqdm']).tqdm

SAMPLE_SIZE = 1024          # Sampling(1024), run_strotss.py:68 of the reference


class ContentLoss:
    """ContentLoss()(target, prediction) = self_similarity(prediction, target)"""

    def __call__(self, target: torch.Tensor, prediction: torch.Tensor) -> torch.Tensor:
        return self_similarity(prediction, target)


class WeightedContentLoss:
    """WeightedContentLoss(weight)(target, prediction) = weighted_self_similarity(prediction, target, weight): the content
    loss with one weight per sample (the content-weight map at the samples); all ones is ContentLoss"""

    def __init__(self, weight):
        self.weight = weight

    def __call__(self, target: torch.Tensor, prediction: torch.Tensor) -> torch.Tensor:
        return weighted_self_similarity(prediction, target, self.weight)


class StyleLoss:
    """StyleLoss(target, alpha)(prediction) = moment + REMD + palette REMD / max(alpha, 1)"""

    def __init__(self, target: torch.Tensor, alpha: float, **kwargs):
        self.target = target
        self.inv_alpha = 1 / max(alpha, 1)

    def __call__(self, prediction: torch.Tensor) -> torch.Tensor:
        yuv = strotss.convert_rgb_to_yuv
        return (moment_matching(self.target, prediction) + relaxed_emd(self.target, prediction)
                + self.inv_alpha * relaxed_emd(yuv(self.target), yuv(prediction), distance='both'))


class BlendedStyleLoss:
    """Style blending: BlendedStyleLoss(targets, weights, alpha)(prediction) = sum_k w_k * StyleLoss(targets[k], alpha)(prediction),
    the weights normalised to sum to 1"""

    def __init__(self, targets, weights, alpha: float, **kwargs):
        if len(targets) != len(weights):
            raise ValueError(f"{len(targets)} style targets but {len(weights)} weights")
        self.weights = strotss_engine.normalise_style_weights(weights)
        self.losses = [StyleLoss(t, alpha) for t in targets]

    def __call__(self, prediction: torch.Tensor) -> torch.Tensor:
        total = None
        for w, loss in zip(self.weights, self.losses):
            term = w * loss(prediction)
            total = term if total is None else total + term
        return total


# --------------------------------------------------------------------------------------------------
def _one_gpu(args, what: str, verb: str = "runs"):
    """the refusal every one-GPU flag family shares: ValueError for `what` with --strips, then under torchrun with
    WORLD_SIZE > 1.  Where a validator calls it decides which of its refusals wins."""
    if getattr(args, "strips", False):
        raise ValueError(f"{what} cannot be combined with --strips")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError(f"{what} {verb} on one GPU: not under torchrun with WORLD_SIZE > 1")


def _style_inputs(args):
    """(style paths, normalised weights) of the run: style_path alone, or style_path + --style_mix with --style_weights
    (1 + len(style_mix) values, default equal).  Zero-weight styles are dropped here, before anything is loaded or sampled,
    so `--style_weights 1 0` is the single-style run.  Blends with masks or --strips: ValueError."""
    mix = list(getattr(args, "style_mix", None) or [])
    weights = getattr(args, "style_weights", None)
    paths = [args.style_path] + mix
    if weights is None:
        weights = [1.0] * len(paths)
    weights = [float(w) for w in weights]
    if len(weights) != len(paths):
        raise ValueError(f"--style_weights takes {len(paths)} values (style_path + {len(mix)} --style_mix images), "
                         f"got {len(weights)}")
    if len(paths) > strotss_engine._hip.MAX_STYLES:
        raise ValueError(f"style blending takes at most {strotss_engine._hip.MAX_STYLES} styles, got {len(paths)}")
    weights = strotss_engine.normalise_style_weights(weights)        # finite, >= 0, not all zero
    if mix and (getattr(args, "content_mask", None) or getattr(args, "style_mask", None)):
        raise ValueError("style blending (--style_mix) cannot be combined with masks")
    if mix and getattr(args, "strips", False):
        raise ValueError("style blending (--style_mix) cannot be combined with --strips")
    kept = [(p, w) for p, w in zip(paths, weights) if w > 0]
    paths, weights = [p for p, _ in kept], [w for _, w in kept]
    return paths, strotss_engine.normalise_style_weights(weights)


def _content_weight_input(args):
    """--content_weight_map: its path, or None.  One GPU only: with --strips or under torchrun with WORLD_SIZE > 1 a
    ValueError (checked before anything is loaded)."""
    path = getattr(args, "content_weight_map", None)
    if not path:
        return None
    _one_gpu(args, "--content_weight_map")
    return path


def _sample_map_input(args):
    """--sample_map: its path, the word "auto" (the map is computed from the content, _auto_sample_input), or None.  One
    GPU only: with --strips, under torchrun with WORLD_SIZE > 1 or for a file that does not exist a ValueError (checked
    before anything is loaded)."""
    path = getattr(args, "sample_map", None)
    if not path:
        return None
    _one_gpu(args, "--sample_map")
    if path == SAMPLE_MAP_AUTO:
        return path
    if not os.path.isfile(path):
        raise ValueError(f"--sample_map: no such file: {path}")
    return path


SAMPLE_MAP_AUTO = "auto"


def _auto_sample_input(args):
    """--sample_map auto: (radius or None, gain or None, floor or None, --save_sample_map's DIR or None), or None without
    it.  ValueError, before anything is loaded: one of --sample_radius, --sample_gain, --sample_floor, --save_sample_map
    without --sample_map auto, or a value out of range (strotss.check_sample_parameters)."""
    given = {f: getattr(args, f, None) for f in ("sample_radius", "sample_gain", "sample_floor", "save_sample_map")}
    if _sample_map_input(args) != SAMPLE_MAP_AUTO:
        for flag, value in given.items():
            if value is not None:
                raise ValueError(f"--{flag} needs --sample_map auto (the map computed from the content)")
        return None
    strotss.check_sample_parameters(given["sample_radius"], given["sample_gain"], given["sample_floor"])
    return given["sample_radius"], given["sample_gain"], given["sample_floor"], given["save_sample_map"]


PRESERVE_COLOR_MODES = ("match", "luminance", "transfer")


def _preserve_color_input(args):
    """--preserve_color: "match", "luminance", "transfer" or None.  One GPU only: with --strips or under torchrun with
    WORLD_SIZE > 1 a ValueError (checked before anything is loaded), as is --transfer_iters without the mode transfer or
    outside 1..64."""
    mode = getattr(args, "preserve_color", None)
    iters = getattr(args, "transfer_iters", None)
    if iters is not None:
        if mode != "transfer":
            raise ValueError("--transfer_iters needs --preserve_color transfer")
        lo, hi = strotss.TRANSFER_ITERS_RANGE
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not lo <= iters <= hi:
            raise ValueError(f"--transfer_iters must be a whole number in {lo}..{hi}, got {iters!r}")
    if mode is None:
        return None
    if mode not in PRESERVE_COLOR_MODES:
        raise ValueError(f"--preserve_color takes one of {PRESERVE_COLOR_MODES}, got {mode!r}")
    _one_gpu(args, "--preserve_color")
    return mode


def _style_transport_input(args) -> dict:
    """--style_transport, --sinkhorn_reg, --sinkhorn_iters, --sinkhorn_log, --sliced_projections: StepEngine's keywords for
    them (sinkhorn_log only where the flag is given).  ValueError, before anything is loaded: an unknown transport, a
    regulariser, an iteration count or --sinkhorn_log without --style_transport sinkhorn or out of range (--sinkhorn_log:
    --sinkhorn_reg above 1000), a projection count without --style_transport sliced or out of range, and with sinkhorn or
    sliced --strips or WORLD_SIZE > 1."""
    transport = getattr(args, "style_transport", None) or "remd"
    reg, iters = getattr(args, "sinkhorn_reg", None), getattr(args, "sinkhorn_iters", None)
    proj = getattr(args, "sliced_projections", None)
    if transport != "sinkhorn" and (reg is not None or iters is not None):
        raise ValueError("--sinkhorn_reg and --sinkhorn_iters need --style_transport sinkhorn")
    log = bool(getattr(args, "sinkhorn_log", False))
    if log and transport != "sinkhorn":
        raise ValueError("--sinkhorn_log needs --style_transport sinkhorn")
    if transport != "sliced" and proj is not None:
        raise ValueError("--sliced_projections needs --style_transport sliced")
    reg = strotss_engine.DEFAULT_SINKHORN_L if reg is None else reg
    iters = strotss_engine.DEFAULT_SINKHORN_ITERS if iters is None else iters
    proj = strotss_engine.DEFAULT_SLICED_PROJECTIONS if proj is None else proj
    strotss_engine.check_style_transport(transport, reg, iters, sinkhorn_log=log)
    if isinstance(proj, bool) or not isinstance(proj, (int, np.integer)) or \
            not 1 <= proj <= strotss_engine.SLICED_MAX_PROJECTIONS:
        raise ValueError(f"--sliced_projections must be a whole number in 1..{strotss_engine.SLICED_MAX_PROJECTIONS}, "
                         f"got {proj!r}")
    if transport in ("sliced", "sinkhorn"):
        _one_gpu(args, f"--style_transport {transport}")
    if transport == "sliced":
        return dict(style_transport=transport, sinkhorn_l=float(reg), sinkhorn_iters=int(iters),
                    sliced_projections=int(proj), sliced_seed=int(getattr(args, "seed", 0) or 0))
    kw =dict(style_transport=transport, sinkhorn_l=float(reg), sinkhorn_iters=int(iters))
    return dict(kw, sinkhorn_log=True) if log else kw


def _palette_transport_input(args) -> dict:
    """--palette_transport, --palette_projections: StepEngine's keywords for them, none for remd (the engine is then built as
    it always was).  ValueError, before anything is loaded: an unknown transport, a direction count without
    --palette_transport sliced or out of range, and with sliced --strips or WORLD_SIZE > 1."""
    transport = getattr(args, "palette_transport", None) or "remd"
    proj = getattr(args, "palette_projections", None)
    if transport not in strotss_engine.PALETTE_TRANSPORTS:
        raise ValueError(f"--palette_transport takes one of {strotss_engine.PALETTE_TRANSPORTS}, got {transport!r}")
    if transport != "sliced":
        if proj is not None:
            raise ValueError("--palette_projections needs --palette_transport sliced")
        return {}
    proj = strotss_engine.DEFAULT_PALETTE_PROJECTIONS if proj is None else proj
    if isinstance(proj, bool) or not isinstance(proj, (int, np.integer)) or \
            not 1 <= proj <= strotss_engine.PALETTE_MAX_PROJECTIONS:
        raise ValueError(f"--palette_projections must be a whole number in 1..{strotss_engine.PALETTE_MAX_PROJECTIONS}, "
                         f"got {proj!r}")
    _one_gpu(args, "--palette_transport sliced")
    return dict(palette_transport=transport, palette_projections=int(proj))


DEFAULT_DETAIL_POOLS = (1, 4)             # pixel-level edges and 4-pixel structure; a convention, not tuned


def _pixel_prior_input(args) -> dict:
    """--detail_weight, --detail_pool, --tv_weight: {"detail": (weight, pools) or None, "tv": weight},
    both off unless given.  ValueError, before anything is loaded, for a weight that is not finite or negative,
    --detail_pool without --detail_weight or not 1..3 distinct ascending values of {1, 2, 4, 8, 16}, and for either flag
    with --strips or under torchrun with WORLD_SIZE > 1."""
    dw, pools, tv = (getattr(args, k, None) for k in ("detail_weight", "detail_pool", "tv_weight"))
    for flag, val in (("--detail_weight", dw), ("--tv_weight", tv)):
        if val is not None and (not np.isfinite(val) or val < 0):
            raise ValueError(f"{flag} must be finite and >= 0, got {val}")
    if pools is not None and dw is None:
        raise ValueError("--detail_pool needs --detail_weight")
    if dw is None and tv is None:
        return dict(detail=None, tv=0.0)
    from nn import _ops
    if dw is not None:
        pools = _ops.check_detail_pools(list(DEFAULT_DETAIL_POOLS) if pools is None else list(pools))
    _one_gpu(args, " / ".join(f for f, v in (("--detail_weight", dw), ("--tv_weight", tv)) if v is not None))
    return dict(detail=None if dw is None else (float(dw), pools), tv=0.0 if tv is None else float(tv))


DEFAULT_PHOTO_RADIUS, DEFAULT_PHOTO_EPS = 1, 1e-4      # the 3 x 3 windows of Luan et al.; conventions, not tuned


def _photo_term_input(args):
    """--photo_weight, --photo_radius, --photo_eps: (weight, radius, eps), or None when --photo_weight
    is absent.  ValueError, before anything is loaded: a radius or an eps without the weight, a weight that is not finite or
    negative, a radius outside 1..4, an eps outside [1e-4, 1], --strips, WORLD_SIZE > 1."""
    weight, radius, eps = (getattr(args, k, None) for k in ("photo_weight", "photo_radius", "photo_eps"))
    if weight is None:
        if radius is not None or eps is not None:
            raise ValueError("--photo_radius and --photo_eps need --photo_weight")
        return None
    if not np.isfinite(weight) or weight < 0:
        raise ValueError(f"--photo_weight must be finite and >= 0, got {weight}")
    radius = DEFAULT_PHOTO_RADIUS if radius is None else radius
    eps = DEFAULT_PHOTO_EPS if eps is None else eps
    strotss_engine.check_photo(radius, eps)
    _one_gpu(args, "--photo_weight")
    return float(weight), int(radius), float(eps)


def _photo_smooth_input(args):
    """--photo_smooth: (radius or None, eps) or None when the flag is absent.  ValueError, before anything is loaded: a
    radius or an eps without the flag, a radius outside 1..64, an eps outside [1e-4, 1], --strips, WORLD_SIZE > 1."""
    radius, eps = getattr(args, "smooth_radius", None), getattr(args, "smooth_eps", None)
    if not getattr(args, "photo_smooth", False):
        if radius is not None or eps is not None:
            raise ValueError("--smooth_radius and --smooth_eps need --photo_smooth")
        return None
    strotss.check_smooth_parameters(radius, eps)
    _one_gpu(args, "--photo_smooth")
    return (None if radius is None else int(radius)), (strotss.DEFAULT_SMOOTH_EPS if eps is None else float(eps))


def _output_size_input(args):
    """--output_size: dict(size="full" or the long side in pixels, mode, radius or None, eps or None), or None when the
    flag is absent.  ValueError, before anything is loaded: --upsample_mode, --upsample_radius or --upsample_eps without
    the flag, a size that is neither "full" nor a whole number in 64..16384, an unknown mode, a radius outside 1..64, an eps
    outside [1e-4, 1], --strips, WORLD_SIZE > 1."""
    size = getattr(args, "output_size", None)
    mode, radius, eps = (getattr(args, "upsample_" + k, None) for k in ("mode", "radius", "eps"))
    if size is None:
        if mode is not None or radius is not None or eps is not None:
            raise ValueError("--upsample_mode, --upsample_radius and --upsample_eps need --output_size")
        return None
    if size != "full":
        lo, hi = strotss.UPSAMPLE_SIZE_RANGE
        try:
            pixels = int(str(size), 10)
        except ValueError:
            pixels = None
        if pixels is None or not lo <= pixels <= hi:
            raise ValueError(f"--output_size {size!r}: expected 'full' or a whole number in {lo}..{hi}")
        size = pixels
    mode = "residual" if mode is None else mode
    if mode not in strotss.UPSAMPLE_MODES:
        raise ValueError(f"--upsample_mode takes one of {strotss.UPSAMPLE_MODES}, got {mode!r}")
    for flag, kw in (("--upsample_radius", dict(radius=radius, eps=None)), ("--upsample_eps", dict(radius=None, eps=eps))):
        try:
            strotss.check_smooth_parameters(**kw)
        except ValueError as e:
            raise ValueError(f"{flag}: {e}") from None
    _one_gpu(args, "--output_size")
    return dict(size=size, mode=mode, radius=None if radius is None else int(radius), eps=None if eps is None else float(eps))


def _refine_masks_input(args):
    """--refine_masks, --refine_sigma S: the colour sigma of the refinement (S, or the default), or None without
    --refine_masks.  ValueError: --refine_masks without --auto_masks, --refine_sigma without --refine_masks or outside
    0.01..1."""
    refine, sigma = getattr(args, "refine_masks", False), getattr(args, "refine_sigma", None)
    if sigma is not None and not refine:
        raise ValueError("--refine_sigma needs --refine_masks")
    if not refine:
        return None
    if getattr(args, "auto_masks", None) is None:
        raise ValueError("--refine_masks needs --auto_masks (it refines the regions the run finds)")
    if sigma is None:
        return strotss.REFINE_SIGMA_R
    try:
        strotss.check_refine_sigma(float(sigma))
    except ValueError:
        lo, hi = strotss.REFINE_SIGMA_RANGE
        raise ValueError(f"--refine_sigma takes a colour scale in {lo}..{hi}, got {sigma!r}") from None
    return float(sigma)


def _track_masks_input(args):
    """--track_masks, --mask_inertia B: the inertia of the tracking (B, or the default), or None without --track_masks.
    ValueError: --track_masks without --auto_masks or without --video, --mask_inertia without --track_masks, not finite or
    outside 0..2."""
    track, beta = getattr(args, "track_masks", False), getattr(args, "mask_inertia", None)
    if beta is not None and not track:
        raise ValueError("--mask_inertia needs --track_masks")
    if not track:
        return None
    if getattr(args, "auto_masks", None) is None:
        raise ValueError("--track_masks needs --auto_masks (it follows the regions the run finds)")
    if not getattr(args, "video", False):
        raise ValueError("--track_masks needs --video (it follows the regions through a frame sequence)")
    if beta is None:
        return strotss.MASK_INERTIA
    try:
        strotss.check_mask_inertia(float(beta))
    except ValueError:
        lo, hi = strotss.MASK_INERTIA_RANGE
        raise ValueError(f"--mask_inertia takes a value in {lo:g}..{hi:g}, got {beta!r}") from None
    return float(beta)


def _scribble_masks_input(args):
    """--content_scribbles C --style_scribbles S, --scribble_sigma, --scribble_iters: (C, S, sigma, iters) with the defaults
    filled in, or None without the two files.  ValueError, before anything is loaded: one file without the other,
    --scribble_sigma / --scribble_iters without the files or outside 0.01..1 / 1..1024, the files together with
    --content_mask / --style_mask, --auto_masks, --style_mix, --video, --strips or under torchrun with WORLD_SIZE > 1."""
    c, s_ = getattr(args, "content_scribbles", None), getattr(args, "style_scribbles", None)
    sigma, iters = getattr(args, "scribble_sigma", None), getattr(args, "scribble_iters", None)
    if bool(c) != bool(s_):
        raise ValueError("--content_scribbles and --style_scribbles go together: every region needs a stroke in both images")
    if not c:
        for flag, value in (("--scribble_sigma", sigma), ("--scribble_iters", iters)):
            if value is not None:
                raise ValueError(f"{flag} needs --content_scribbles and --style_scribbles")
        return None
    try:
        strotss.check_scribble_parameters(None if sigma is None else float(sigma), None)
    except (TypeError, ValueError):
        lo, hi = strotss.SCRIBBLE_SIGMA_RANGE
        raise ValueError(f"--scribble_sigma takes a colour scale in {lo}..{hi:g}, got {sigma!r}") from None
    try:
        strotss.check_scribble_parameters(None, iters)
    except (TypeError, ValueError):
        lo, hi = strotss.SCRIBBLE_ITERS_RANGE
        raise ValueError(f"--scribble_iters takes a number of sweeps in {lo}..{hi}, got {iters!r}") from None
    if getattr(args, "content_mask", None) or getattr(args, "style_mask", None):
        raise ValueError("scribbles cannot be combined with --content_mask / --style_mask: the regions are grown or given")
    if getattr(args, "auto_masks", None) is not None:
        raise ValueError("scribbles cannot be combined with --auto_masks: the regions are grown from strokes or clustered")
    if getattr(args, "style_mix", None):
        raise ValueError("scribbles cannot be combined with --style_mix: masks and blends exclude each other")
    if getattr(args, "video", False):
        raise ValueError("scribbles cannot be combined with --video: the strokes belong to one image")
    _one_gpu(args, "scribbles", verb="run")
    return (c, s_, strotss.SCRIBBLE_SIGMA if sigma is None else float(sigma),
            strotss.SCRIBBLE_ITERS if iters is None else int(iters))


def _auto_masks_input(args, found=None):
    """--auto_masks K, --save_masks DIR: (K, DIR or None), or None without --auto_masks.  ValueError, before anything is
    loaded: K outside 2..8, --save_masks without --auto_masks, --auto_masks with --content_mask / --style_mask, --style_mix,
    --video without --track_masks, --strips or under torchrun with WORLD_SIZE > 1, and the refusals of --refine_masks /
    --refine_sigma (_refine_masks_input), of --track_masks / --mask_inertia (_track_masks_input) and of the scribble flags
    (_scribble_masks_input, with which --save_masks is allowed too).  found: a dict that receives what those three
    returned, as refine, inertia and scribbles (_resolve's way to them: they are entered here and nowhere else)."""
    k, save = getattr(args, "auto_masks", None), getattr(args, "save_masks", None)
    refine = _refine_masks_input(args)
    track = _track_masks_input(args)
    scribbles = _scribble_masks_input(args)
    if found is not None:
        found.update(refine=refine, inertia=track, scribbles=scribbles)
    if k is None:
        if save and scribbles is None:
            raise ValueError("--save_masks needs --auto_masks (it writes the regions the run finds)")
        return None
    lo, hi = strotss.AUTO_MASK_RANGE
    if int(k) != k or not lo <= int(k) <= hi:
        raise ValueError(f"--auto_masks takes a number of clusters in {lo}..{hi}, got {k!r}")
    if getattr(args, "content_mask", None) or getattr(args, "style_mask", None):
        raise ValueError("--auto_masks cannot be combined with --content_mask / --style_mask: the regions are found or given")
    if getattr(args, "style_mix", None):
        raise ValueError("--auto_masks cannot be combined with --style_mix: masks and blends exclude each other")
    if getattr(args, "video", False) and track is None:
        raise ValueError("--auto_masks cannot be combined with --video: clustering every frame on its own would flicker "
                         "(--track_masks follows the first frame's regions through the sequence)")
    _one_gpu(args, "--auto_masks")
    return int(k), (save or None)


DEFAULT_TEMPORAL_WEIGHT = 1000.0          # chosen on the MI355X with the consistency error
MAX_TEMPORAL_FRAMES = 4                   # STROTSS_MAX_TEMPORAL: the targets of one strotss_temporal_multi_fwd_bwd launch
IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png", ".bmp", ".ppm", ".pgm", ".tif", ".tiff", ".webp")


def _temporal_frames(args):
    """--temporal_frames as an ascending tuple of 1..4 distinct positive frame offsets ((1,) when not given); ValueError
    for a non-positive, repeated or fifth offset"""
    raw = getattr(args, "temporal_frames", None)
    if raw is None:
        return (1,)
    offsets = [int(j) for j in raw]
    if not offsets or any(j < 1 for j in offsets):
        raise ValueError(f"--temporal_frames takes positive frame offsets, got {raw}")
    if len(set(offsets)) != len(offsets):
        raise ValueError(f"--temporal_frames: repeated offset in {raw}")
    if len(offsets) > MAX_TEMPORAL_FRAMES:
        raise ValueError(f"--temporal_frames takes at most {MAX_TEMPORAL_FRAMES} offsets, got {len(offsets)}")
    return tuple(sorted(offsets))


def _video_inputs(args, found=None):
    """--video: (sorted frame paths, temporal weight); None without --video.  Refused with a ValueError before anything is
    optimised: --temporal_weight / --flow_dir / --temporal_init / --temporal_frames without --video, a negative weight, bad
    --temporal_frames offsets (_temporal_frames), --video with --strips or under torchrun with WORLD_SIZE > 1, neither
    --flow_dir nor --compute_flow, a content_path that is not a directory of frames, frames of different sizes, a missing
    backward flow of any frame and offset (--flow_dir only); --compute_flow without --video or together with --flow_dir,
    --save_flow without --compute_flow, --flow_match without --compute_flow or outside 1..4, --flow_robust without
    --compute_flow, --flow_alpha / --flow_outer without --flow_robust or out of range (_flow_robust).  found: a dict that
    receives what _flow_match_radius, _flow_robust and (with --video) _temporal_frames returned, as match_radius, robust and
    offsets (_resolve's way to them: they are entered here and nowhere else)."""
    video = bool(getattr(args, "video", False))
    lam = getattr(args, "temporal_weight", None)
    flow_dir = getattr(args, "flow_dir", None)
    compute_flow = bool(getattr(args, "compute_flow", False))
    if not video:
        for flag, val in (("--temporal_weight", lam), ("--flow_dir", flow_dir),
                          ("--temporal_init", getattr(args, "temporal_init", False) or None),
                          ("--temporal_frames", getattr(args, "temporal_frames", None)),
                          ("--compute_flow", compute_flow or None)):
            if val is not None:
                raise ValueError(f"{flag} needs --video")
    if getattr(args, "save_flow", None) and not compute_flow:
        raise ValueError("--save_flow needs --compute_flow (it writes the flows the run computes)")
    if compute_flow and flow_dir:
        raise ValueError("--compute_flow and --flow_dir exclude each other: the flows are computed or read, not both")
    match_radius, robust = _flow_match_radius(args), _flow_robust(args)
    offsets = _temporal_frames(args) if video else None
    if found is not None:
        found.update(match_radius=match_radius, robust=robust, offsets=offsets)
    if not video:
        return None
    lam = DEFAULT_TEMPORAL_WEIGHT if lam is None else float(lam)
    if not np.isfinite(lam) or lam < 0:
        raise ValueError(f"--temporal_weight must be finite and >= 0, got {lam}")
    _one_gpu(args, "--video")
    if not flow_dir and not compute_flow:
        raise ValueError("--video needs --flow_dir (the optical flow between consecutive frames)")
    if not os.path.isdir(args.content_path):
        raise ValueError(f"--video: content_path {args.content_path} is not a directory of frames")
    frames = sorted(os.path.join(args.content_path, f) for f in os.listdir(args.content_path)
                    if f.lower().endswith(IMAGE_SUFFIXES) and os.path.isfile(os.path.join(args.content_path, f)))
    if not frames:
        raise ValueError(f"--video: no frames in {args.content_path}")
    from PIL import Image
    sizes = set()
    for f in frames:
        with Image.open(f) as im:
            sizes.add(im.size)
    if len(sizes) != 1:
        raise ValueError(f"--video: the frames differ in size: {sorted(sizes)}")
    for t in range(2, len(frames) + 1):
        for j in offsets:
            if t - j < 1 or compute_flow:               # computed flows: no file to look for
                continue
            path = os.path.join(flow_dir, f"backward_{t}_{t - j}.flo")
            if not os.path.exists(path):
                raise ValueError(f"--video: backward flow {path} of frame {t} is missing")
    return frames, lam


FLOW_MATCH_RADII = (1, 4)           # --flow_match: strotss_optical_flow_match's radii (0 = no stage is the flag's absence)


def _flow_match_radius(args) -> int:
    """--flow_match [R]: the patch-matching radius of every computed flow, 0 without the flag.
    ValueError without --compute_flow (there is no flow to match) or outside 1..4."""
    r = getattr(args, "flow_match", None)
    if r is None:
        return 0
    if not getattr(args, "compute_flow", False):
        raise ValueError("--flow_match needs --compute_flow (it is a stage of the flows the run computes)")
    if isinstance(r, bool) or int(r) != r or not FLOW_MATCH_RADII[0] <= int(r) <= FLOW_MATCH_RADII[1]:
        raise ValueError(f"--flow_match must be a whole radius in {FLOW_MATCH_RADII[0]}..{FLOW_MATCH_RADII[1]}, got {r}")
    return int(r)


FLOW_ROBUST_OUTER = (1, 8)          # --flow_outer: strotss_flow_robust_params_t.outer, a divisor of the default 32 sweeps
FLOW_SWEEPS = 32                    # strotss_flow_default_params' iters


def _flow_robust(args):
    """--flow_robust [--flow_alpha A] [--flow_outer N]: the `robust` argument of every computed flow:
    None without the flag, else a dict of the values given (the others stay at the library's defaults).  ValueError for
    --flow_robust without --compute_flow, a sub-flag without --flow_robust, an alpha that is not finite and > 0, an outer
    outside 1..8 or not dividing the 32 sweeps of a warp."""
    alpha, outer = getattr(args, "flow_alpha", None), getattr(args, "flow_outer", None)
    if not getattr(args, "flow_robust", False):
        for flag, val in (("--flow_alpha", alpha), ("--flow_outer", outer)):
            if val is not None:
                raise ValueError(f"{flag} needs --flow_robust (it is a parameter of the robust flow)")
        return None
    if not getattr(args, "compute_flow", False):
        raise ValueError("--flow_robust needs --compute_flow (it is the solver of the flows the run computes)")
    robust = {}
    if alpha is not None:
        if isinstance(alpha, bool) or not np.isfinite(alpha) or alpha <= 0:
            raise ValueError(f"--flow_alpha must be finite and > 0, got {alpha}")
        robust["alpha"] = float(alpha)
    if outer is not None:
        if (isinstance(outer, bool) or int(outer) != outer or not FLOW_ROBUST_OUTER[0] <= int(outer) <= FLOW_ROBUST_OUTER[1]
                or FLOW_SWEEPS % int(outer)):
            raise ValueError(f"--flow_outer must be a whole number in {FLOW_ROBUST_OUTER[0]}..{FLOW_ROBUST_OUTER[1]} that "
                             f"divides the {FLOW_SWEEPS} sweeps of a warp, got {outer}")
        robust["outer"] = int(outer)
    return robust


def _resolve(args) -> argparse.Namespace:
    """The job of a run, made once: the namespace as given (the parser's, or a partial one) completed with the parser's own
    defaults, plus what every validator above returns.  Each validator is entered once, in the order in which run() and
    run_video() have always reached them -- of two wrong flags the same one is reported -- and before a device or an image
    is touched.  Everything below this function reads the job; nothing below validates or asks whether a flag is there.
        auto, refine, inertia, scribbles    _auto_masks_input and the three validators it enters
        engine_terms                        StepEngine's keywords of --style_transport and of --palette_transport, merged
        prior, photo, auto_sample           _pixel_prior_input, _photo_term_input, _auto_sample_input
        content_weight                      _content_weight_input: the map's path or None
        preserve, smooth, upsample          _preserve_color_input, _photo_smooth_input, _output_size_input
        frames, temporal_weight             _video_inputs; frames is None without --video
        offsets, match_radius, robust       the three validators _video_inputs enters; offsets is None without --video
        styles                              _style_inputs: (paths, weights)
    sample_map stays the flag (_sample_map_input has passed it); transfer_iters has its default with --preserve_color
    transfer."""
    job = argparse.Namespace(**{**vars(build_parser().parse_args(["", ""])), **vars(args)})
    found = {}
    job.auto = _auto_masks_input(job, found)
    job.engine_terms = dict(_style_transport_input(job), **_palette_transport_input(job))
    job.prior = _pixel_prior_input(job)
    job.photo = _photo_term_input(job)
    job.auto_sample = _auto_sample_input(job)
    if not job.video:                                        # a sequence reaches this one after _video_inputs
        job.content_weight = _content_weight_input(job)
    job.preserve = _preserve_color_input(job)
    job.smooth = _photo_smooth_input(job)
    job.upsample = _output_size_input(job)
    job.frames, job.temporal_weight = _video_inputs(job, found) or (None, job.temporal_weight)
    if job.video:
        job.content_weight = _content_weight_input(job)
    vars(job).update(found)
    if job.preserve == "transfer":
        job.transfer_iters = strotss.DEFAULT_TRANSFER_ITERS if job.transfer_iters is None else int(job.transfer_iters)
    job.styles = _style_inputs(job)
    if bool(job.content_mask) != bool(job.style_mask):
        raise ValueError('Either both content and style masks must be provided or neither.')
    return job


def _written_guides(job, content_path: str, frame_lo=None):
    """The guides of _written, loaded before the image's first step: (the content at the result's size, the content at
    --output_size's target size), both (h, w, 3) on the device, each None where nothing needs it.  frame_lo: the content at
    the result's size where the caller holds it already (a --compute_flow frame).  ValueError for a target smaller than the
    result in either dimension or with 3 H W > INT_MAX -- here, not after the optimisation."""
    upsample = job.upsample
    if not (upsample or job.smooth or job.preserve == "luminance"):
        return None, None
    lo = _frame_at_result_size(job, content_path) if frame_lo is None else frame_lo
    if not upsample:
        return lo, None
    hi = utils.load_image(content_path, max_size=None if upsample["size"] == "full" else upsample["size"])[0].contiguous()
    strotss.check_upsample_sizes(int(lo.shape[0]), int(lo.shape[1]), int(hi.shape[0]), int(hi.shape[1]))
    return lo, hi


def _written(stylized: torch.Tensor, job, guides) -> torch.Tensor:
    """The uint8 image that is written for an optimiser's result, of a single image and of every frame of a sequence:
    --photo_smooth's filter, then --output_size's upsampling, then --preserve_color luminance's merge at the written size,
    then postprocess.  `stylized` itself stays as it is: the temporal targets and --temporal_init keep seeing it."""
    upsample, (guide, guide_hi) = job.upsample, guides
    if job.smooth:                                           # the content's edges back into the result, then its colours
        stylized = strotss.guided_smooth(stylized, guide, *job.smooth)
    if upsample:                                             # to the target size, the content there as guide from here on
        stylized = strotss.guided_upsample(stylized, guide, guide_hi, upsample["radius"], upsample["eps"], upsample["mode"])
        guide = guide_hi
    if job.preserve == "luminance":                          # the result's luma on the content's chroma
        stylized = strotss.luminance_merge(stylized, guide)
    return strotss.postprocess(stylized)


def _match_styles(styles, content, content_masks, style_masks, recolour=None):
    """--preserve_color match: every style image recoloured toward the content's colour mean and covariance
    (strotss_utils.match_colour), each style on its own.  With masks region by region: the statistics of the style pixels
    in style mask r and of the content pixels in content mask r, the map applied to style mask r's pixels only (the masks
    resized to the images as mask_at_scale resizes them to a scale); pixels in no region stay.  recolour: another
    (style, content, style_mask, content_mask) -> style in match_colour's place (_recolour_styles)."""
    recolour = recolour or strotss.match_colour
    if list(content_masks) == [None]:
        return [recolour(s_k, content) for s_k in styles]
    ch, cw = int(content.shape[1]), int(content.shape[2])
    out = []
    for s_k in styles:
        sh, sw = int(s_k.shape[1]), int(s_k.shape[2])
        for c_mask, s_mask in zip(content_masks, style_masks):
            cm = torch.from_numpy(strotss.mask_at_scale(c_mask, ch, cw).astype(np.float32))
            sm = torch.from_numpy(strotss.mask_at_scale(s_mask, sh, sw).astype(np.float32))
            s_k = recolour(s_k, content, sm, cm)
        out.append(s_k)
    return out


def _recolour_styles(job, styles, content, content_masks, style_masks):
    """the styles as --preserve_color leaves them before anything is sampled: recoloured by match or by transfer
    (--transfer_iters bases) exactly where and as _match_styles recolours them, untouched otherwise"""
    if job.preserve == "match":
        return _match_styles(styles, content, content_masks, style_masks)
    if job.preserve == "transfer":
        def transfer(style, content, style_mask=None, content_mask=None):
            return strotss.transfer_colour(style, content, style_mask, content_mask, iters=job.transfer_iters)
        return _match_styles(styles, content, content_masks, style_masks, recolour=transfer)
    return styles


def _frame_at_result_size(job, path: str) -> torch.Tensor:
    """a content frame (h, w, 3) on the device at the size of a frame's final result: resized as _stylise makes the content
    of its last executed scale"""
    scl = 2 << (5 + int(job.level) - 1)
    return utils.resize(utils.load_image(path, max_size=job.max_size), scl)[0].contiguous()


def _computed_flows(job, t: int, j: int, frames, h: int, w: int):
    """--compute_flow: (backward, forward) flow of frame t against frame t-j, both (h, w, 2), by strotss_optical_flow on the
    content frames at the results' size (with --flow_match R: strotss_optical_flow_match; with --flow_robust:
    strotss_optical_flow_robust).  frames: {1-based position: (h, w, 3) frame on the device}.  --save_flow DIR
    writes them as backward_{t}_{t-j}.flo and forward_{t-j}_{t}.flo."""
    cur, old = frames[t], frames[t - j]
    if tuple(cur.shape) != (h, w, 3) or tuple(old.shape) != (h, w, 3):
        raise ValueError(f"--compute_flow: frames of {tuple(cur.shape)} and {tuple(old.shape)}, the results are {h} x {w}")
    fb = strotss_engine._ops.optical_flow(cur, old, match_radius=job.match_radius, robust=job.robust)
    ff = strotss_engine._ops.optical_flow(old, cur, match_radius=job.match_radius, robust=job.robust)
    if job.save_flow:
        os.makedirs(job.save_flow, exist_ok=True)
        strotss.write_flo(os.path.join(job.save_flow, f"backward_{t}_{t - j}.flo"), fb)
        strotss.write_flo(os.path.join(job.save_flow, f"forward_{t - j}_{t}.flo"), ff)
    return fb, ff


def _flow_warp_for_frame(job, t: int, previous: torch.Tensor, j: int = 1, frames=None):
    """(backward flow (h, w, 2), warped result of frame t-j, certainty) of frame t (1-based, t > j) at that result's size:
    the flows of --flow_dir resized to that size (strotss_utils.resize_flow), the warp and certainty in one launch; a
    reliable_{t}_{t-j}.pgm, when there is one, replaces the certainty (its value / 255, resized).  `previous`: the final
    result of frame t-j.  --compute_flow: both flows come from _computed_flows(frames) at that size instead; no file is
    read."""
    h, w = int(previous.shape[1]), int(previous.shape[2])
    dev = previous.device
    if job.compute_flow:
        fb, ff = _computed_flows(job, t, j, frames, h, w)
        return (fb,) + tuple(strotss_engine._ops.flow_warp(previous.contiguous(), fb, ff))
    flow_b = strotss.read_flo(os.path.join(job.flow_dir, f"backward_{t}_{t - j}.flo"))
    big = tuple(flow_b.shape[:2])
    fwd_path = os.path.join(job.flow_dir, f"forward_{t - j}_{t}.flo")
    flow_f = strotss.read_flo(fwd_path) if os.path.exists(fwd_path) else None
    if flow_f is not None and tuple(flow_f.shape[:2]) != big:
        raise ValueError(f"{fwd_path}: a {tuple(flow_f.shape[:2])} flow, the backward one is {big}")
    fb = strotss.resize_flow(flow_b.to(dev), h, w).contiguous()
    ff = None if flow_f is None else strotss.resize_flow(flow_f.to(dev), h, w).contiguous()
    warped, certainty = strotss_engine._ops.flow_warp(previous.contiguous(), fb, ff)
    rel = os.path.join(job.flow_dir, f"reliable_{t}_{t - j}.pgm")
    if os.path.exists(rel):
        certainty = _resized_reliable(rel, h, w)
    return fb, warped, certainty


def _pairs_for_frame(job, t: int, results, frames=None) -> dict:
    """{j: (backward flow, warped result of frame t-j, raw certainty)} of frame t for the offsets j of job.offsets (ascending)
    with t - j >= 1: one _flow_warp_for_frame call per pair, so each flow is read or computed -- and with --save_flow
    written -- once per frame.  results[k]: the final result of frame t-1-k.  {} for the first frame.  The tracking
    (entry offsets[0]) and the temporal list (_temporal_targets_for_frame) both take their pairs from this map; the flows
    are the same bits on every run, so sharing an entry gives what computing it again gave."""
    return {j: _flow_warp_for_frame(job, t, results[j - 1], j, frames) for j in job.offsets if t - j >= 1 and j <= len(results)}


def _temporal_targets_for_frame(job, t: int, results, frames=None, pairs=None):
    """[(warped result of frame t-j, combined certainty)] of frame t, nearest frame first, 0..4 of them: the one temporal
    shape between the flows and _stylise.  pairs: the frame's _pairs_for_frame map where the caller
    holds it already, built here otherwise.  With two pairs or more the certainties are combined once, at the frame's size
    (strotss_temporal_long_certainty), so that a pixel a nearer frame covers does not pull toward an older one; one pair
    keeps its raw certainty.  [] for the first frame."""
    if pairs is None:
        pairs = _pairs_for_frame(job, t, results, frames)
    found = [pairs[j][1:] for j in sorted(pairs)]
    if len(found) <= 1:                     # nothing nearer to subtract: the raw certainty is the combined one
        return found
    combined = strotss_engine._ops.temporal_long_certainty(torch.stack([c.float().contiguous() for _, c in found]))
    return [(warped, combined[k]) for k, (warped, _) in enumerate(found)]


def _resized_reliable(path: str, h: int, w: int) -> torch.Tensor:
    """reliable_{t}_{t-1}.pgm / 255 at (h, w) on the device (bilinear, no threshold): read as a content-weight map is"""
    c = strotss.load_content_weight_map(path).to(utils.device())
    if tuple(c.shape) != (h, w):
        c = strotss_engine._ops.resize_bilinear(c[:, :, None].contiguous(), h, w).reshape(h, w)
    return c.contiguous()


def _load_masks(job):
    """(content_masks, style_masks) or ([None], [None]); one of the two flags alone was refused by _resolve."""
    if not job.content_mask:
        return [None], [None]
    c_masks, s_masks = strotss.load_mask(job.content_mask, job.style_mask, max_size=job.max_size)
    utils.logger.info(f'Loaded {len(c_masks)} masks.')
    return c_masks, s_masks


def _initial_image(position: int, is_last: bool, previous, content, style, base_lr: float, weights=None):
    """The image a scale starts from and its learning rate (reference run_strotss.py:78-88):
    first executed scale: Laplacian of the content + mean style colour; middle scales: upsampled previous
    result + Laplacian; last scale (when more than one runs): upsampled previous result, lr halved.
    Style blending: `style` a list of images with `weights`, the mean colour is sum_k w_k * mean(style_k)."""
    laplacian = strotss.make_laplacian(content)
    if position == 0:
        if isinstance(style, (list, tuple)):
            if len(style) == 1:
                style = style[0]
            else:
                mix = None
                for w, s_k in zip(weights, style):
                    term = w * s_k.mean(dim=(1, 2), keepdim=True)
                    mix = term if mix is None else mix + term
                return laplacian + mix, base_lr
        return laplacian + style.mean(dim=(1, 2), keepdim=True), base_lr
    if not is_last:
        return utils.resize_like(previous, content) + laplacian, base_lr
    return utils.resize_like(previous, content), base_lr / 2


def _style_targets(params, style, style_masks, sampling, weights=None):
    """One StyleTarget per region: <= 1024 nearest-sampled hypercolumns of the style image (fixed for the
    scale), their inverse norms and first/second moments.  Style blending (`style` a list of images, `weights`): one
    StyleBlend of one target per style, drawn in style order (one style: exactly the single-style draws)."""
    if isinstance(style, (list, tuple)):
        if len(style) == 1:
            return _style_targets(params, style[0], style_masks, sampling)
        if list(style_masks) != [None]:
            raise ValueError("style blending cannot be combined with masks")
        targets = [_style_targets(params, s_k, [None], sampling)[0] for s_k in style]
        return [strotss_engine.StyleBlend(targets, list(weights))]
    feats = strotss_engine.extract_features(params, style)
    width = sum(int(m.shape[-1]) for m in feats)
    targets = []
    for mask in style_masks:
        idx = sampling._make_indices(feats[0], False, mask)
        rows = strotss_engine._ops.hypercol_gather(feats, idx, False)
        targets.append(strotss_engine.StyleTarget.build(rows, int(idx.shape[0]), width))
    return targets


def _optimise_scale(eng, scl: int, content_masks, args, dev, quiet: bool = False, step_trace=None, sample_levels=None):
    """`max_iter` RMSprop steps; fresh sample coordinates every step (they are drawn inside the reference's
    traced train_step as well).  `step_trace`: a list receiving every step's loss dict (one host sync per step).
    sample_levels: the scale's (h, w) uint16 importance levels (--sample_map) or None; the device draw and the host loop
    below then draw the same weighted sequence."""
    from nn import parallel
    masks_here = [None if m is None else strotss.mask_at_scale(m, eng.h, eng.w) for m in content_masks]
    log_every = max(1, int(args.log_every))
    # The index sets are drawn on the host (as make_indices does in the reference's step).  Uploading them from pageable
    # memory would block the host until the previous step has drained, leaving the GPU idle while the next draw is
    # computed (~0.3 ms per step, a quarter of a 64-px step): a small ring of pinned buffers + asynchronous copies lets
    # the host draw step k+1 while the GPU runs step k.
    # Round 4: the draw itself runs on the device, as the first kernel of the captured step (csrc/draw.hip; counter-based
    # Philox stream whose host twin is rand.index_rng, so the sequence is the one the host loop below would draw) -- wherever
    # the sample count cannot vary from step to step.  No upload, no ring, nothing for the host to do per step.
    stream = rand.index_rng
    if (dev.type == "cuda" and not args.host_draw and isinstance(stream, rand.PhiloxStream)
            and (eng.enable_device_draw(stream.seed, stream.t, masks_here) if sample_levels is None else
                 eng.enable_device_draw(stream.seed, stream.t, masks_here, sample_levels=sample_levels))):
        with tqdm(range(args.max_iter), disable=quiet) as bar:
            for it in bar:
                if it == 0 and not args.no_graph:
                    eng.capture_graph()
                eng.step()
                if step_trace is not None:
                    step_trace.append(eng.losses())
                if (it + 1) % log_every == 0 or it + 1 == args.max_iter:
                    r = eng.losses()
                    bar.set_description(f"Scale: {scl:4d} - It: {it+1:4d}")
                    bar.set_postfix({k: f'{r[_LOGGED.get(k, k)]:.3f}' for k in _logged_terms(eng)})
        stream.skip(args.max_iter * len(masks_here))          # the host twin moves past the draws the device made
        return
    ring, slots = 8, {}
    with tqdm(range(args.max_iter), disable=quiet) as bar:
        for it in bar:
            if sample_levels is None:
                idx_np = [strotss.make_indices_np(eng.h, eng.w, True, SAMPLE_SIZE, rand.index_rng, mk) for mk in masks_here]
            else:
                idx_np = [strotss.make_indices_weighted_np(eng.h, eng.w, SAMPLE_SIZE, rand.index_rng, sample_levels, mk)
                          for mk in masks_here]
            offsets = None
            if eng.strips is not None:            # same seed on every rank: identical draws, every region's set ordered by owner
                offsets = []
                for r in range(len(idx_np)):
                    idx_np[r], off = parallel.sort_indices_by_strip(idx_np[r], eng.strips)
                    offsets.append(off)
            idx = []
            for r, a in enumerate(idx_np):
                if dev.type != "cuda":
                    idx.append(torch.from_numpy(a).to(dev))
                    continue
                buf, ev = slots.get((r, it % ring), (None, None))
                if buf is None:
                    buf = torch.empty((SAMPLE_SIZE, 2), dtype=torch.float32).pin_memory()
                if ev is not None:
                    ev.synchronize()              # the copy that last used this slot has run
                host = buf[:a.shape[0]]
                host.copy_(torch.from_numpy(a))
                idx.append(host.to(dev, non_blocking=True))
                ev = torch.cuda.Event()
                ev.record()
                slots[(r, it % ring)] = (buf, ev)
            if it == 0 and not args.no_graph:
                eng.capture_graph(idx, offsets)
            eng.step(idx, offsets)
            if step_trace is not None:
                step_trace.append(eng.losses())
            if (it + 1) % log_every == 0 or it + 1 == args.max_iter:
                r = eng.losses()
                bar.set_description(f"Scale: {scl:4d} - It: {it+1:4d}")
                bar.set_postfix({k: f'{r[_LOGGED.get(k, k)]:.3f}' for k in _logged_terms(eng)})


_LOGGED = {"sinkhorn": "l_sinkhorn", "sliced": "l_sliced"}      # the log line's name of a term -> its key in StepEngine.losses()


def _logged_terms(eng):
    """the scalars of the log line: with --style_transport sinkhorn or sliced also the transport term, under its name"""
    terms = ('loss', 'loss_c', 'loss_s')
    return terms + (eng.style_transport,) if eng.style_transport in _LOGGED else terms


def run(args: argparse.Namespace, trace=None):
    """The reference's run(args) (run_strotss.py:43-161).  `trace` (a list) receives one dict per executed scale:
    scale index and size, lr, alpha, loss_denom, the image the scale starts from, every step's losses and the
    result -- what the parity test of the schedule compares with the oracle's run_scales.  The command line is resolved
    once (_resolve); with --video the job goes to run_video's frame loop."""
    job = _resolve(args)                                     # every refusal, before anything is loaded
    if job.video:
        return _run_frames(job, trace)
    timer = utils.Timer()
    timer.start()
    rand.seed_everything(job.seed)
    from nn import parallel
    rank, world = 0, 1
    if (job.strips or job.content_mask) and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count()))
        rank, world = parallel.init_from_env(torch.cuda.current_device())
    dev = utils.device()

    vgg = VGG(use_keras_weight=job.use_keras_weight, weights=job.weights, seed=job.seed, device=dev)
    guides = _written_guides(job, job.content_path)          # --output_size: the target's size is refused before the first step
    final = _written(_stylise(job, vgg, job.content_path, dev, rank, world, trace), job, guides)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    timer.stop()
    if rank == 0:
        utils.logger.info(f"Done in {timer.elapsed_time:.2f}s.")
        utils.write_image(final, job.output_path)
    return final


def _region_masks(job, vgg, content, style, strokes=None, masks=None):
    """(content_masks, style_masks) of an image as loaded, from the first source there is: `masks` from the caller
    (--track_masks), --auto_masks (the regions found), the scribble files (`strokes`: what load_scribbles read; the regions
    grown from them), --content_mask / --style_mask (or [None], [None]).  --save_masks writes what was found or grown."""
    if masks is not None:
        return masks
    if job.auto:
        k, save = job.auto                                   # without --refine_masks the call carries no such keyword
        content_masks, style_masks = strotss.auto_masks(vgg.params, content, style, k,
                                                        **({} if job.refine is None else dict(refine=job.refine)))
        if content_masks[0] is not None:
            utils.logger.info(f'Found {len(content_masks)} regions.')
            if save:
                strotss.save_masks(save, content_masks, style_masks)
        return content_masks, style_masks
    if strokes:
        _, _, sigma, iters = job.scribbles
        content_masks, style_masks = strotss.scribble_masks(vgg.params, content, style, strokes[0], strokes[1],
                                                            len(strokes[2]), strokes[2], sigma, iters)
        utils.logger.info(f'Grew {len(content_masks)} regions from the strokes.')
        if job.save_masks:
            strotss.save_masks(job.save_masks, content_masks, style_masks)
        return content_masks, style_masks
    return _load_masks(job)


def _sample_map(job, content, content_path: str, rank: int = 0):
    """--sample_map: the map read from its path; with `auto` this image's own detail map (with --video every frame's), which
    --save_sample_map DIR writes as sample_map.png (with --video sample_map_<frame stem>.png); None without the flag"""
    auto = job.auto_sample
    if not auto:
        return strotss.load_sample_map(job.sample_map) if job.sample_map else None
    sm_map = strotss.auto_sample_map(content, *auto[:3])
    if auto[3] and rank == 0:
        stem = os.path.splitext(os.path.basename(content_path))[0]
        name = f"sample_map_{stem}.png" if job.video else "sample_map.png"
        strotss.save_sample_map(os.path.join(auto[3], name), sm_map)
    return sm_map


def _stylise(job, vgg, content_path: str, dev, rank: int = 0, world: int = 1, trace=None, temporal=None, masks=None):
    """The coarse-to-fine schedule on one content image -> the final image of the finest scale (1, h, w, 3).
    temporal: _temporal_targets_for_frame's list of 0..4 (warped earlier result, certainty) pairs at that result's size,
    nearest frame first; None and [] mean no term.  Every scale carries one temporal term per pair, all with weight
    job.temporal_weight, and --temporal_init starts the first executed scale from the nearest pair's warped result.
    masks: (content_masks, style_masks) of this frame from the caller (--track_masks), in place of those of _region_masks."""
    from nn import parallel
    level, first = int(job.level), int(job.start_level)
    strokes = strotss.load_scribbles(*job.scribbles[:2]) if job.scribbles else None
    content = utils.load_image(content_path, max_size=job.max_size)
    style_paths, style_weights = job.styles
    styles = [utils.load_image(p, max_size=job.max_size) for p in style_paths]
    content_masks, style_masks = _region_masks(job, vgg, content, styles[0], strokes, masks)
    # --preserve_color match / transfer, before any resize: every scale samples the recoloured styles
    styles = _recolour_styles(job, styles, content, content_masks, style_masks)
    cw_map = strotss.load_content_weight_map(job.content_weight) if job.content_weight else None
    sm_map = _sample_map(job, content, content_path, rank)
    sampling = strotss.Sampling(SAMPLE_SIZE)
    prior, photo = job.prior, job.photo

    # alpha = 16 (x3500 with Keras weights), halved after every scale -- also after skipped ones
    alpha = job.alpha * 16.0 * (3500 if job.use_keras_weight else 1) / 2.0 ** first
    stylized = None
    for position, i in enumerate(range(first, level)):
        scl = 2 << (5 + i)                                   # long side 64, 128, 256, ...
        scl_content = utils.resize(content, scl)
        scl_style = [utils.resize(s_k, scl) for s_k in styles]
        if len(scl_style) == 1:
            scl_style = scl_style[0]
        stylized, lr = _initial_image(position, position > 0 and i == level - 1, stylized, scl_content, scl_style,
                                      job.lr, style_weights)
        hs, ws = int(scl_content.shape[1]), int(scl_content.shape[2])
        terms = dict(job.engine_terms)                       # the engine's keywords of this scale, built afresh
        if temporal:
            scaled = strotss.temporal_targets_at_scale(temporal, hs, ws)
            terms["temporal"] = [strotss_engine.TemporalTarget(target, cert, job.temporal_weight) for target, cert in scaled]
            if position == 0 and job.temporal_init:
                stylized = scaled[0][0][None].contiguous()   # the nearest frame's warp instead of Laplacian + mean style colour
        # --strips: ONE image sharded by rows (the only sharding that cuts trunk work), with or without mask regions; where
        # a scale is too small for strips to pay (strip_plan -> None) a masked run falls back to dealing its regions out
        plan = (parallel.strip_plan(int(scl_content.shape[1]), world, rank, halo=bool(job.halo))
                if world > 1 and job.strips else None)
        cw_scaled = None if cw_map is None else strotss.content_weight_at_scale(cw_map, hs, ws)
        if prior["detail"] is not None:                      # the detail target: this image's content at this scale
            terms["detail"] = strotss_engine.DetailTarget(scl_content, prior["detail"][1], prior["detail"][0], cw_scaled)
        if prior["tv"] > 0:
            terms["tv_weight"] = prior["tv"]
        if photo is not None:                                # the photorealism term: this image's content as the guide
            terms["photo"] = strotss_engine.PhotoTarget(scl_content, photo[1], photo[2], photo[0])
        eng = strotss_engine.StepEngine(
            vgg.params, strotss_engine.extract_features(vgg.params, scl_content),
            _style_targets(vgg.params, scl_style, style_masks, sampling, style_weights), stylized, alpha,
            loss_denom=2. + alpha + 1. / max(alpha, 1.), lr=lr, sample_size=SAMPLE_SIZE, strips=plan,
            dist_group=parallel.WORLD if (world > 1 and job.content_mask and plan is None) else None,
            content_weight=cw_scaled, **terms)
        rec = None
        if trace is not None:
            rec = dict(i=i, scl=scl, lr=lr, alpha=alpha, loss_denom=eng.loss_denom, init=stylized.clone(), steps=[],
                       hw=(eng.h, eng.w))
            trace.append(rec)
        # --sample_map: the levels of this scale, rounded once
        _optimise_scale(eng, scl, content_masks, job, dev, quiet=rank != 0, step_trace=None if rec is None else rec["steps"],
                        sample_levels=None if sm_map is None else strotss.sample_levels_at_scale(sm_map, hs, ws))
        stylized = eng.stylized()
        if rec is not None:
            rec["final"] = stylized.clone()
        del eng
        alpha /= 2.
    return stylized


def _tracked_masks(job, vgg, tracking: dict, t: int, frame: str, nearest):
    """--track_masks: (content_masks, style_masks) of frame t.  tracking: {frame position: state} of the
    last j frames (j = job.offsets[0], the nearest offset) plus the sequence's constants under "style" (the style masks of
    all kept regions) -- or {"off": True} once frame 1 gave fewer than two regions (the whole sequence then runs unmasked).
    Frame 1: auto_mask_regions jointly with style_path, the masks of both images as a single-image run makes them.
    Frame t > 1: strotss_utils.track_regions against the state of frame t-j along `nearest` = (backward flow, warped
    result, certainty) of that pair (None for t <= j: no prior), then the content masks of the present regions with the
    matching style masks.  --save_masks DIR: style_mask.png once, content_mask_<frame stem>.png per frame (of a frame that
    runs unmasked: its label grid)."""
    if tracking.get("off"):
        return [None], [None]
    (k, save), refine, j = job.auto, job.refine, job.offsets[0]
    content = utils.load_image(frame, max_size=job.max_size)
    stem = os.path.splitext(os.path.basename(frame))[0]
    if t == 1:
        style = utils.load_image(job.style_path, max_size=job.max_size)
        found = strotss.auto_mask_regions(vgg.params, content, style, k)
        if not found["kept"]:
            utils.logger.warning(f"--auto_masks {k}: fewer than two clusters hold {strotss.AUTO_MASK_MIN_SHARE:.3f} of both "
                                 f"images (content {found['counts'][0].tolist()}, style {found['counts'][1].tolist()} of "
                                 f"{found['n_c']}, {found['n_s']} points); running the sequence unmasked")
            tracking["off"] = True
            return [None], [None]
        content_masks, style_masks = strotss.masks_from_grids(content, style, found["content_grid"], found["style_grid"],
                                                              found["kept"], refine)
        utils.logger.info(f'Found {len(content_masks)} regions.')
        tracking["style"], tracking[1] = style_masks, strotss.tracking_state(found)
        if save:
            strotss.save_region_image(os.path.join(save, "style_mask.png"), style_masks)
            strotss.save_region_image(os.path.join(save, f"content_mask_{stem}.png"), content_masks)
        return content_masks, style_masks
    source = tracking[t - j] if nearest is not None else tracking[1]      # t <= j: frame 1's state is still held
    flow, certainty = (nearest[0], nearest[2].float().contiguous()) if nearest is not None else (None, None)
    state = strotss.track_regions(source, vgg.params, content, flow, certainty, job.inertia)
    tracking[t] = state
    tracking.pop(t - j, None)
    present = state["present"]
    if not present:
        utils.logger.warning(f"--track_masks: fewer than two regions hold {strotss.AUTO_MASK_MIN_SHARE:.3f} of frame {t}'s grid "
                             f"points ({state['counts'].tolist()}); running this frame unmasked")
        if save:                            # what the frame was given: its grid over all regions, by nearest neighbour
            strotss.save_region_image(os.path.join(save, f"content_mask_{stem}.png"),
                                      strotss.masks_from_grid(content, state["grid"], state["kept"]))
        return [None], [None]
    content_masks = strotss.masks_from_grid(content, state["mask_grid"], len(present), refine)
    if save:
        strotss.save_region_image(os.path.join(save, f"content_mask_{stem}.png"), content_masks, present)
    return content_masks, [tracking["style"][r] for r in present]


def run_video(args: argparse.Namespace, trace=None):
    """--video: every frame of the directory content_path through the schedule of run(), one VGG for the sequence, the
    seeds reset for every frame (each frame draws the index stream a single-image run draws).  Per frame: the
    (frame, offset) pairs of --temporal_frames, each read or computed once (_pairs_for_frame; the last max(J) results and,
    with --compute_flow, the last max(J) + 1 content frames at the results' size stay on the device); with --track_masks
    the frame's regions from the nearest pair (_tracked_masks); the temporal list from the same pairs
    (_temporal_targets_for_frame); then the frame path of run(): _written_guides, _stylise, _written.  Only what is written
    is filtered, upsampled or merged: the temporal targets and --temporal_init keep the optimiser's own results.  Writes
    <output dir>/<frame stem>.jpg; returns the list of the frames' uint8 results.  `trace`: one list per frame."""
    return _run_frames(_resolve(args), trace)


def _run_frames(job, trace=None):
    """run_video on the resolved job: run() hands over its own, so a sequence is resolved once as well"""
    dev = utils.device()
    os.makedirs(job.output_path, exist_ok=True)
    vgg = VGG(use_keras_weight=job.use_keras_weight, weights=job.weights, seed=job.seed, device=dev)
    offsets = job.offsets
    tracking = {} if job.auto else None     # --track_masks: the states of the last offsets[0] frames, by frame position
    outs, results = [], []                  # results[k]: the final image of frame t-1-k, the last max(offsets) of them
    flow_frames = {} if job.compute_flow else None      # --compute_flow: the last max(offsets) + 1 frames
    for t, frame in enumerate(job.frames, start=1):
        timer = utils.Timer()
        timer.start()
        rand.seed_everything(job.seed)
        if flow_frames is not None:
            flow_frames[t] = _frame_at_result_size(job, frame)
            flow_frames.pop(t - offsets[-1] - 1, None)
        pairs = _pairs_for_frame(job, t, results, flow_frames)
        temporal = _temporal_targets_for_frame(job, t, results, flow_frames, pairs)
        rec = None
        if trace is not None:
            rec = []
            trace.append(rec)
        masks = None
        if tracking is not None:            # pairs.get: no prior for t <= offsets[0]
            masks = _tracked_masks(job, vgg, tracking, t, frame, pairs.get(offsets[0]))
        guides = _written_guides(job, frame, None if flow_frames is None else flow_frames[t])
        stylized = _stylise(job, vgg, frame, dev, trace=rec, temporal=temporal, masks=masks)
        results = [stylized] + results[:offsets[-1] - 1]
        final = _written(stylized, job, guides)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        timer.stop()
        out = os.path.join(job.output_path, os.path.splitext(os.path.basename(frame))[0] + ".jpg")
        utils.logger.info(f"Frame {t}/{len(job.frames)} done in {timer.elapsed_time:.2f}s.")
        utils.write_image(final, out)
        outs.append(final)
    return outs


# (flag, kwargs): the reference's flags first, then this build's additions
_FLAGS = (
    (("content_path",), dict(type=str)), (("style_path",), dict(type=str)),
    (("--content_mask",), dict(type=str, default=None)), (("--style_mask",), dict(type=str, default=None)),
    (("--max_size",), dict(type=int, default=None)), (("--lr",), dict(type=float, default=2e-3)),
    (("--level",), dict(type=float, default=4)), (("--max_iter",), dict(type=int, default=200)),
    (("--alpha",), dict(type=float, default=1.0)), (("--use_keras_weight",), dict(action='store_true')),
    (("--gpu_id",), dict(type=int, default=0)), (("--output_path", "-o"), dict(type=str, default="output.jpg")),
    (("--start_level",), dict(type=int, default=0)), (("--seed",), dict(type=int, default=0)),
    (("--weights",), dict(type=str, default=None)), (("--log_every",), dict(type=int, default=10)),
    (("--no_graph",), dict(action='store_true', help="eager kernel launches instead of one hipGraph per step")),
    (("--host_draw",), dict(action='store_true', help="draw the sample coordinates on the host every step (the same sequence; "
                                                      "the default draws them on the device inside the step)")),
    (("--style_mix",), dict(type=str, nargs='+', default=None, metavar='PATH',
                            help="style blending: further style images mixed with style_path")),
    (("--style_weights",), dict(type=float, nargs='+', default=None, metavar='W',
                                help="style blending: one weight per style (style_path first), default equal")),
    (("--content_weight_map",), dict(type=str, default=None, metavar='PATH',
                                     help="greyscale image: per-pixel content strength (white keeps the content, black lets "
                                          "it go), resized to every scale")),
    (("--video",), dict(action='store_true', help="content_path is a directory of frames, -o an output directory")),
    (("--flow_dir",), dict(type=str, default=None, metavar='DIR',
                           help="with --video: backward_{t}_{t-1}.flo, forward_{t-1}_{t}.flo, reliable_{t}_{t-1}.pgm")),
    (("--temporal_weight",), dict(type=float, default=None, metavar='LAMBDA',
                                  help=f"with --video: weight of the temporal term (default {DEFAULT_TEMPORAL_WEIGHT:g})")),
    (("--temporal_init",), dict(action='store_true', help="with --video: frames after the first start their first executed "
                                                          "scale from the warped previous result")),
    (("--temporal_frames",), dict(type=int, nargs='+', default=None, metavar='J',
                                  help="with --video: 1 to 4 distinct positive frame offsets of the long-term temporal term "
                                       "(default 1; Ruder et al. use 1 10 20 40): frame t is also pulled toward frame t-j's "
                                       "result along backward_{t}_{t-j}.flo where no nearer frame covers the pixel")),
    (("--compute_flow",), dict(action='store_true', help="with --video, instead of --flow_dir: compute the optical flows between "
                                                         "the frames on the GPU (both directions, every --temporal_frames offset)")),
    (("--flow_match",), dict(type=int, nargs='?', const=2, default=None, metavar='R',
                             help="with --compute_flow: patch-matching stage of radius R (1..4, default 2) at every level of "
                                  "the computed flows (DESIGN.md section 31)")),
    (("--flow_robust",), dict(action='store_true', help="with --compute_flow: robust (Charbonnier) penalties in every computed "
                                                        "flow, for objects that move against their background (DESIGN.md "
                                                        "section 32); combines with --flow_match")),
    (("--flow_alpha",), dict(type=float, default=None, metavar='A',
                             help="with --flow_robust: the smoothness weight (finite, > 0; default 0.06)")),
    (("--flow_outer",), dict(type=int, default=None, metavar='N',
                             help="with --flow_robust: weight updates per warp (1..8, a divisor of 32; default 4)")),
    (("--save_flow",), dict(type=str, default=None, metavar='DIR',
                            help="with --compute_flow: write the computed flows there as backward_{t}_{t-j}.flo and "
                                 "forward_{t-j}_{t}.flo")),
    (("--preserve_color",), dict(type=str, default=None, choices=PRESERVE_COLOR_MODES,
                                 help="keep the content's colours: 'match' recolours the style images to the content's colour "
                                      "mean and covariance before anything is sampled, 'luminance' writes the result's luma on "
                                      "the content's chroma, 'transfer' gives the style images the content's whole colour "
                                      "distribution (iterative distribution transfer)")),
    (("--transfer_iters",), dict(type=int, default=None, metavar='T',
                                 help="with --preserve_color transfer: the number of colour bases, 1..64 (default 10)")),
    (("--photo_smooth",), dict(action='store_true', help="keep the content's edges: pass the result through the guided filter "
                                                         "with the content as colour guide before it is written")),
    (("--smooth_radius",), dict(type=int, default=None, metavar='R',
                                help="with --photo_smooth: window radius in pixels, 1..64 (default: 1/64 of the longer side)")),
    (("--smooth_eps",), dict(type=float, default=None, metavar='E',
                             help="with --photo_smooth: regulariser on [0, 1] colours, 1e-4..1 (default 1e-2)")),
    (("--output_size",), dict(type=str, default=None, metavar='SIZE',
                              help="write the result at the content's resolution: 'full' (the content file as decoded) or a "
                                   "long side in pixels, 64..16384; joint upsampling with the content as guide")),
    (("--upsample_mode",), dict(type=str, default=None, choices=strotss.UPSAMPLE_MODES,
                                help="with --output_size: 'residual' (default) keeps the optimiser's texture, 'guided' is the "
                                     "guided filter alone (photorealistic; goes with --photo_smooth)")),
    (("--upsample_radius",), dict(type=int, default=None, metavar='R',
                                  help="with --output_size: window radius at the result's size, 1..64 (default: 1/64 of its "
                                       "longer side)")),
    (("--upsample_eps",), dict(type=float, default=None, metavar='E',
                               help="with --output_size: regulariser on [0, 1] colours, 1e-4..1 (default 1e-3 for residual, "
                                    "1e-2 for guided)")),
    (("--auto_masks",), dict(type=int, default=None, metavar='K',
                             help="region guidance without painted masks: cluster the hypercolumns of content and style "
                                  "jointly into K groups (2..8); every cluster found in both images is a region")),
    (("--refine_masks",), dict(action='store_true', help="with --auto_masks: bring the label grids to the images by joint "
                                                         "bilateral upsampling, so that the regions follow the images' edges")),
    (("--refine_sigma",), dict(type=float, default=None, metavar='S',
                               help="with --refine_masks: colour scale of the vote on [0, 1] colours, 0.01..1 (default 0.1)")),
    (("--save_masks",), dict(type=str, default=None, metavar='DIR',
                             help="with --auto_masks: write content_mask.png and style_mask.png there, in the colour-coded "
                                  "format of --content_mask / --style_mask")),
    (("--content_scribbles",), dict(type=str, default=None, metavar='PATH',
                                    help="region guidance from strokes: an image with a stroke per region on the content, in "
                                         "the corner colours of --content_mask (black: no stroke)")),
    (("--style_scribbles",), dict(type=str, default=None, metavar='PATH',
                                  help="with --content_scribbles: strokes of the same colours on the style")),
    (("--scribble_sigma",), dict(type=float, default=None, metavar='S',
                                 help=f"with the scribble files: colour scale of the edge weights on [0, 1] colours, 0.01..1 "
                                      f"(default {strotss.SCRIBBLE_SIGMA:g}, not tuned)")),
    (("--scribble_iters",), dict(type=int, default=None, metavar='T',
                                 help=f"with the scribble files: sweeps, 1..1024 (default {strotss.SCRIBBLE_ITERS}, not tuned)")),
    (("--track_masks",), dict(action='store_true', help="with --auto_masks K --video: follow the first frame's regions through "
                                                        "the sequence along the backward flow instead of refusing the pair")),
    (("--mask_inertia",), dict(type=float, default=None, metavar='B',
                               help=f"with --track_masks: added to the cosine of a cell's prior label, 0..2 (default "
                                    f"{strotss.MASK_INERTIA:g})")),
    (("--style_transport",), dict(type=str, default="remd", choices=strotss_engine.STYLE_TRANSPORTS,
                                  help="the transport term of the style loss: the relaxed EMD, the Sinkhorn transport cost "
                                       "(mass-conserving, about 60 more launches per region and step) or the sliced "
                                       "Wasserstein distance (mass-conserving, sort and match on random sign directions)")),
    (("--sinkhorn_reg",), dict(type=float, default=None, metavar='L',
                               help=f"with --style_transport sinkhorn: K = exp(-L cost), > 0 (default "
                                    f"{strotss_engine.DEFAULT_SINKHORN_L:g})")),
    (("--sinkhorn_iters",), dict(type=int, default=None, metavar='T',
                                 help=f"with --style_transport sinkhorn: scalings, 1..{strotss_engine.SINKHORN_MAX_ITERS} (default "
                                      f"{strotss_engine.DEFAULT_SINKHORN_ITERS})")),
    (("--sinkhorn_log",), dict(action='store_true',
                               help=f"with --style_transport sinkhorn: the scalings in the log domain, for sharp plans; "
                                    f"--sinkhorn_reg in (0, {strotss_engine.SINKHORN_LOG_MAX_L:g}] (the linear form is "
                                    f"clamp-free only to 13.8)")),
    (("--sliced_projections",), dict(type=int, default=None, metavar='P',
                                     help=f"with --style_transport sliced: directions, 1..{strotss_engine.SLICED_MAX_PROJECTIONS} "
                                          f"(default {strotss_engine.DEFAULT_SLICED_PROJECTIONS}, not tuned)")),
    (("--palette_transport",), dict(type=str, default="remd", choices=strotss_engine.PALETTE_TRANSPORTS,
                                    help="the palette term of the style loss: the relaxed EMD between the samples' YUV "
                                         "colours, or their sliced Wasserstein distance (mass-conserving: the style's "
                                         "colours are matched in proportion)")),
    (("--palette_projections",), dict(type=int, default=None, metavar='P',
                                      help=f"with --palette_transport sliced: directions, "
                                           f"1..{strotss_engine.PALETTE_MAX_PROJECTIONS} (default "
                                           f"{strotss_engine.DEFAULT_PALETTE_PROJECTIONS}, not tuned for image quality)")),
    (("--strips",), dict(action='store_true', help="under torchrun: shard ONE image over the GPUs by image strips")),
    (("--halo",), dict(action='store_true', help="with --strips: per-layer halo EXCHANGE with the neighbouring ranks (16-row "
                                                 "windows margins, one row per layer and direction) instead of a 128-row recompute margin")),
    (("--photo_weight",), dict(type=float, default=None, metavar='W',
                               help="weight of the photorealism term: over every window the result should be an affine "
                                    "function of the content's colours (off unless given; finite, >= 0)")),
    (("--photo_radius",), dict(type=int, default=None, metavar='R',
                               help=f"with --photo_weight: the window radius, 1..4 (default {DEFAULT_PHOTO_RADIUS})")),
    (("--photo_eps",), dict(type=float, default=None, metavar='E',
                            help=f"with --photo_weight: the covariance regulariser, 1e-4..1 (default {DEFAULT_PHOTO_EPS:g}, "
                                 "not tuned)")),
    (("--sample_map",), dict(type=str, default=None, metavar='PATH',
                             help="greyscale image: where the step's sample coordinates are drawn (white densely, black only "
                                  "when nothing else is left), resized to every scale; or the word auto: a detail map "
                                  "computed from the content (with --video from every frame)")),
    (("--sample_radius",), dict(type=int, default=None, metavar='R',
                                help="with --sample_map auto: window radius in pixels, 1..64 (default: the longer side // 64, "
                                     "at least 1)")),
    (("--sample_gain",), dict(type=float, default=None, metavar='G',
                              help="with --sample_map auto: detail at G times the image's mean detail reaches level 1 "
                                   f"(default {strotss.DEFAULT_SAMPLE_GAIN:g}, > 0; not tuned for image quality)")),
    (("--sample_floor",), dict(type=float, default=None, metavar='F',
                               help="with --sample_map auto: the level of a flat region, 0..1 "
                                    f"(default {strotss.DEFAULT_SAMPLE_FLOOR:g}; not tuned for image quality)")),
    (("--save_sample_map",), dict(type=str, default=None, metavar='DIR',
                                  help="with --sample_map auto: write the map to DIR as sample_map.png (with --video "
                                       "sample_map_<frame stem>.png), readable through --sample_map PATH")),
    (("--detail_weight",), dict(type=float, default=None, metavar='W',
                                help="weight of the Laplacian detail term: keeps the content's edges at the pool sizes of "
                                     "--detail_pool (off unless given; finite, >= 0)")),
    (("--detail_pool",), dict(type=int, nargs='+', default=None, metavar='P',
                              help="with --detail_weight: 1..3 distinct pool sizes of {1, 2, 4, 8, 16}, ascending (default "
                                   "1 4, not tuned)")),
    (("--tv_weight",), dict(type=float, default=None, metavar='W',
                            help="weight of the total variation of the result: penalises pixel-level grain (off unless "
                                 "given; finite, >= 0)")),
)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    for names, kw in _FLAGS:
        parser.add_argument(*names, **kw)
    return parser


if __name__ == "__main__":
    cli = build_parser().parse_args()
    utils.set_gpu(cli.gpu_id)
    run(cli)
