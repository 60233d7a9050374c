"""What DESIGN.md section 19 records about --track_masks.

    python tools/track_time.py CONTENT STYLE [--k 3] [--size 256] [--calls 5]
        1. label-change rates: on the occluder sequence of the tests (exact flows) and on three frames cut from CONTENT with
           a shift of 4 px per frame (constant flow), the share of the grid cells with a prior (a certain flow that stays
           inside the frame and meets a valid label) whose label differs from that prior, at --mask_inertia 0, 0.05 and 2
        2. wall clock per frame of the tracking steps 1-5 (track_regions + masks_from_grid) next to frame 1's path
           (auto_mask_regions + masks_from_grids) on the same frame, median of --calls after two warm-ups
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BETAS = (0.0, 0.05, 2.0)


def change_rates(U, params, frames, style, flows, k, what):
    """frames: [(1, h, w, 3)]; flows[t] = (backward flow, certainty or None) of frames[t] against frames[t - 1], t >= 1"""
    found = U.auto_mask_regions(params, frames[0], style, k)
    if not found["kept"]:
        print(f"{what}: frame 1 gives fewer than two regions (counts {found['counts'].tolist()}); nothing to track")
        return
    for beta in BETAS:
        state, changed, certain, present = U.tracking_state(found), 0, 0, []
        for t in range(1, len(frames)):
            state = U.track_regions(state, params, frames[t], flows[t][0], flows[t][1], beta)
            has = state["prior"] >= 0
            certain += int(has.sum())
            changed += int((has & (state["grid"] != state["prior"])).sum())
            present.append(state["present"])
        print(f"{what}: kept {found['kept']}, --mask_inertia {beta:g}: {changed} of {certain} cells with a prior changed their "
              f"label = {100.0 * changed / max(certain, 1):.2f} %; present regions per frame {present}")


def wall(torch, fn, calls):
    for _ in range(2):
        fn()
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times), min(times)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("content")
    ap.add_argument("style")
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    import _temporal_long_ref as TL
    from nn import _ops, utils
    from nn import strotss_utils as U
    from nn.model import VGG
    dev = utils.device()
    vgg = VGG(use_keras_weight=False, weights=None, seed=0, device=dev)
    style = utils.load_image(a.style, max_size=a.size)

    # 1a. the occluder sequence, its exact flows, the certainty of strotss_flow_warp
    tmp = tempfile.mkdtemp()
    frames_dir, flow_dir = os.path.join(tmp, "frames"), os.path.join(tmp, "flows")
    paths, _ = TL.occluder_sequence(frames_dir, flow_dir, n_frames=3, offsets=(1,))
    frames = [utils.load_image(p) for p in paths]
    flows = [None]
    for t in (2, 3):
        fb = U.read_flo(os.path.join(flow_dir, f"backward_{t}_{t - 1}.flo")).to(dev).contiguous()
        ff = U.read_flo(os.path.join(flow_dir, f"forward_{t - 1}_{t}.flo")).to(dev).contiguous()
        _, cert = _ops.flow_warp(frames[t - 2].contiguous(), fb, ff)
        flows.append((fb, cert))
    change_rates(U, vgg.params, frames, style, flows, 2, "occluder sequence 48 x 64, K = 2")

    # 1b. the content moved by 4 px per frame: frame t shows columns 4 t .. 4 t + W - 8, so its backward flow is (+4, 0)
    content = utils.load_image(a.content, max_size=a.size)
    h, w = int(content.shape[1]), int(content.shape[2]) - 8
    frames = [content[:, :, 4 * t:4 * t + w].contiguous() for t in range(3)]
    fb = torch.from_numpy(np.broadcast_to(np.float32([4.0, 0.0]), (h, w, 2)).copy()).to(dev)
    change_rates(U, vgg.params, frames, style, [None, (fb, None), (fb, None)], a.k,
                 f"content {h} x {w} shifted by 4 px per frame, K = {a.k}")

    # 2. wall clock per frame
    found = U.auto_mask_regions(vgg.params, frames[0], style, a.k)
    if not found["kept"]:
        raise SystemExit("no regions on this pair: nothing to time")
    state = U.tracking_state(found)

    def first():
        f = U.auto_mask_regions(vgg.params, frames[1], style, a.k)
        if f["kept"]:
            U.masks_from_grids(frames[1], style, f["content_grid"], f["style_grid"], f["kept"])

    def tracked():
        s = U.track_regions(state, vgg.params, frames[1], fb, None, U.MASK_INERTIA)
        if s["present"]:
            U.masks_from_grid(frames[1], s["mask_grid"], len(s["present"]))

    for name, fn in (("auto_mask_regions + masks_from_grids", first), ("track_regions + masks_from_grid", tracked)):
        med, low = wall(torch, fn, a.calls)
        print(f"{name} on a {h} x {w} frame, K = {a.k}: median {med:.2f} ms (min {low:.2f}, {a.calls} calls)")


if __name__ == "__main__":
    main()
