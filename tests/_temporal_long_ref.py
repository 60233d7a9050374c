"""Restatements of the long-term temporal term, shared by test_temporal_long_cpu.py and
test_hip_temporal_long.py: the combined certainties in float32 (the kernel's order, for a bit-exact comparison) and in
float64, the terms L_j and their summed gradient in float64, and a synthetic sequence of a static textured background
crossed by a square occluder, with its exact flows and reliable_*.pgm files for every frame offset."""
import os

import numpy as np

import _temporal_ref as T


def long_certainty32(stack):
    """stack (count, h, w), nearest frame first -> plane j = max(c_j - sum_{k<j} c_k, 0), the sum in ascending k in
    float32 starting from 0 (the order of strotss_temporal_long_certainty)"""
    stack = np.asarray(stack, dtype=np.float32)
    out = np.empty_like(stack)
    covered = np.zeros(stack.shape[1:], dtype=np.float32)
    for j in range(stack.shape[0]):
        out[j] = np.maximum(stack[j] - covered, np.float32(0))
        covered = covered + stack[j]
    return out


def long_certainty64(stack):
    """the same combination in float64"""
    stack = np.asarray(stack, dtype=np.float64)
    csum = np.concatenate([np.zeros((1,) + stack.shape[1:]), np.cumsum(stack, axis=0)[:-1]])
    return np.maximum(stack - csum, 0.0)


def multi_loss64(x, targets, certs, gscales):
    """([L_j], sum_j gscale_j dL_j/dx) in float64, L_j = (1/(3hw)) sum_p c_j(p) |x(p) - target_j(p)|^2"""
    losses, grad = [], np.zeros(np.shape(x), dtype=np.float64)
    for tgt, c, g in zip(targets, certs, gscales):
        l, d = T.temporal_loss64(x, tgt, c)
        losses.append(l)
        grad = grad + g * d
    return losses, grad


def write_pgm(path, img):
    """img (h, w) uint8 as a binary PGM"""
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape
    with open(path, "wb") as f:
        f.write(f"P5\n{w} {h}\n255\n".encode())
        f.write(img.tobytes())


def occluder_box(t, x0, y0, size, vx):
    """(y0, y1, x0, x1) of the occluder in frame t (1-based): it moves vx pixels to the right per frame"""
    x = x0 + (t - 1) * vx
    return y0, y0 + size, x, x + size


def occluder_sequence(dirpath, flow_dir, n_frames=4, h=48, w=64, size=12, vx=10, x0=2, y0=18, offsets=(1, 2), seed=0):
    """n_frames frames of a static textured background with a square occluder (its own texture) moving vx pixels to the
    right per frame, written as frame_{t}.png; for every frame t and offset j with t - j >= 1 the exact flows
    backward_{t}_{t-j}.flo (occluder pixels -(j vx, 0), background 0), forward_{t-j}_{t}.flo (+(j vx, 0) on the occluder of
    frame t-j) and reliable_{t}_{t-j}.pgm (255, except 0 on the background that the occluder covers in frame t-j).
    -> (frame paths, occluder(t): the (h, w) bool mask of the occluder in frame t)."""
    from PIL import Image
    bg = T.texture(h, w, seed)
    occ = T.texture(size, size, seed + 100)[..., ::-1] * 0.5 + 0.5
    os.makedirs(dirpath, exist_ok=True)
    os.makedirs(flow_dir, exist_ok=True)

    def mask(t):
        m = np.zeros((h, w), dtype=bool)
        ya, yb, xa, xb = occluder_box(t, x0, y0, size, vx)
        m[max(ya, 0):min(yb, h), max(xa, 0):min(xb, w)] = True
        return m

    paths = []
    for t in range(1, n_frames + 1):
        frame = bg.copy()
        ya, yb, xa, xb = occluder_box(t, x0, y0, size, vx)
        ox0, ox1 = max(xa, 0), min(xb, w)
        if ox0 < ox1:
            frame[ya:yb, ox0:ox1] = occ[:, ox0 - xa:ox1 - xa]
        p = os.path.join(dirpath, f"frame_{t:02d}.png")
        Image.fromarray((frame * 255).round().astype(np.uint8)).save(p)
        paths.append(p)

    def covered(t, j):
        return mask(t - j) & ~mask(t)

    for t in range(2, n_frames + 1):
        for j in offsets:
            if t - j < 1:
                continue
            fb = np.zeros((h, w, 2), np.float32)
            fb[mask(t), 0] = -j * vx
            ff = np.zeros((h, w, 2), np.float32)
            ff[mask(t - j), 0] = j * vx
            T.write_flo(os.path.join(flow_dir, f"backward_{t}_{t - j}.flo"), fb)
            T.write_flo(os.path.join(flow_dir, f"forward_{t - j}_{t}.flo"), ff)
            rel = np.full((h, w), 255, np.uint8)
            rel[covered(t, j)] = 0
            write_pgm(os.path.join(flow_dir, f"reliable_{t}_{t - j}.pgm"), rel)
    return paths, mask
