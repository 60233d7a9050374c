"""Scribble-mask timings.  One JSON line per measurement; device events around `iters` back-to-back calls after
a warm-up, the sweep forms alternated, three repeats.
  - strotss_scribble_labels as the product calls it (unary, 128 sweeps, labels; no copy of the planes; the wrapper's two
    output allocations included) at 48 x 64, 192 x 256, 384 x 512 and 768 x 1024 with k = 2 and 7 regions and
    iters_per_launch 1 (one sweep per launch), 2, 4 and 8 (blocked).
  - `--golden`: on the golden pair at 64 px, the share of pixels whose label differs between two-stroke scribbles and
    --auto_masks 2 --refine_masks (regions matched by the better of the two pairings)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

from nn import _ops as ops

DEV = "cuda"
SWEEPS = 128


def _time(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters        # us per call


def launches(per):
    return 1 + SWEEPS // per + SWEEPS % per + 1


def sweeps(iters):
    import _scribble_cases as S
    for h, w in ((48, 64), (192, 256), (384, 512), (768, 1024)):
        for k in (2, 7):
            img, stroke, scores = (torch.from_numpy(a).to(DEV) for a in S.make(h, w, k))
            call = lambda per, planes=False: ops.scribble_labels(img, stroke, scores, 0.05, 0.05, 0.1, SWEEPS, per, planes)
            plain = call(1, True)
            for per in (2, 4, 8):
                assert all(torch.equal(a, b) for a, b in zip(plain, call(per, True)))
            for rep in range(3):                      # alternated: plain, blocked
                for per in (1, 2, 4, 8):
                    us = _time(lambda: call(per), iters)
                    print(json.dumps({"what": "scribble_labels", "h": h, "w": w, "k": k, "sweeps": SWEEPS,
                                      "iters_per_launch": per, "rep": rep, "launches": launches(per), "us": round(us, 1)}),
                          flush=True)


def golden():
    from nn import strotss_utils as U
    from nn import utils
    from nn.model import VGG
    golden = os.path.join(ROOT, "tests", "golden")
    vgg = VGG(use_keras_weight=False, weights=None, seed=0, device=utils.device())
    content = utils.load_image(os.path.join(golden, "content_im.jpg"), max_size=64)
    style = utils.load_image(os.path.join(golden, "style_im.jpg"), max_size=64)
    strokes = []
    for im in (content, style):
        h, w = int(im.shape[1]), int(im.shape[2])
        s = np.full((h, w), -1, dtype=np.int32)
        s[2:5, 2:w // 3] = 0
        s[h - 5:h - 2, w - w // 3:w - 2] = 1
        strokes.append(s)
    grown = U.scribble_masks(vgg.params, content, style, strokes[0], strokes[1], 2)
    auto = U.auto_masks(vgg.params, content, style, 2, refine=U.REFINE_SIGMA_R)
    res = {"what": "golden_pair_64px", "auto_regions": 0 if auto[0][0] is None else len(auto[0])}
    if auto[0][0] is not None:
        for name, a, b in (("content", grown[0], auto[0]), ("style", grown[1], auto[1])):
            same = float((a[1] == b[1]).float().mean())
            res[f"{name}_share_differing"] = round(1.0 - same, 4)
            res[f"{name}_share_differing_swapped"] = round(same, 4)
    return res


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--golden":
        print(json.dumps(golden()), flush=True)
        return
    sweeps(int(os.environ.get("ITERS", "50")))


if __name__ == "__main__":
    main()
