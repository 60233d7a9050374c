"""float64 restatement of the temporal term of frame sequences, shared by test_temporal_cpu.py and
test_hip_temporal.py: the warp along the backward flow, its certainty, L_t and its gradient, .flo writing, and a synthetic
sequence of a texture translated by a whole number of pixels per frame with its exact flows."""
import os

import numpy as np


def _taps(s, n):
    s = np.clip(s, -2.0, n + 1.0)
    fl = np.floor(s)
    i = fl.astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), s - fl


def bilinear(img, sx, sy):
    """img (h, w, c) sampled at (sx, sy) (each (h, w)): pixel centres at integer coordinates, 4 neighbours clamped"""
    h, w = img.shape[:2]
    x0, x1, fx = _taps(sx, w)
    y0, y1, fy = _taps(sy, h)
    fx, fy = fx[..., None], fy[..., None]
    img = img.astype(np.float64)
    return ((1 - fy) * ((1 - fx) * img[y0, x0] + fx * img[y0, x1]) + fy * ((1 - fx) * img[y1, x0] + fx * img[y1, x1]))


def warp64(prev, flow_b):
    h, w = flow_b.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    fb = flow_b.astype(np.float64)
    return bilinear(prev, xs + fb[..., 0], ys + fb[..., 1])


def certainty64(flow_b, flow_f=None):
    h, w = flow_b.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    fb = flow_b.astype(np.float64)
    u, v = fb[..., 0], fb[..., 1]
    sx, sy = xs + u, ys + v
    ok = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    fb2 = u * u + v * v
    if flow_f is not None:
        wf = bilinear(flow_f, sx, sy)
        su, sv = u + wf[..., 0], v + wf[..., 1]
        ok &= ~(su * su + sv * sv > 0.01 * (fb2 + wf[..., 0] ** 2 + wf[..., 1] ** 2) + 0.5)
    xm, xp = np.clip(np.arange(w) - 1, 0, w - 1), np.clip(np.arange(w) + 1, 0, w - 1)
    ym, yp = np.clip(np.arange(h) - 1, 0, h - 1), np.clip(np.arange(h) + 1, 0, h - 1)
    ux, vx = (u[:, xp] - u[:, xm]) * 0.5, (v[:, xp] - v[:, xm]) * 0.5
    uy, vy = (u[yp] - u[ym]) * 0.5, (v[yp] - v[ym]) * 0.5
    ok &= ~((ux * ux + uy * uy) + (vx * vx + vy * vy) > 0.01 * fb2 + 0.002)
    return ok.astype(np.float64)


def temporal_loss64(x, target, cert):
    """(L_t, dL_t/dx) = ((1/(3hw)) sum_p c(p) |x(p) - target(p)|^2, its gradient), x / target (h, w, 3), cert (h, w)"""
    h, w = cert.shape
    d = x.astype(np.float64) - target.astype(np.float64)
    c = cert.astype(np.float64)[..., None]
    return float((c * d * d).sum() / (3 * h * w)), 2.0 * c * d / (3 * h * w)


def write_flo(path, flow):
    flow = np.asarray(flow, dtype=np.float32)
    h, w = flow.shape[:2]
    with open(path, "wb") as f:
        f.write(np.float32(202021.25).tobytes())
        f.write(np.array([w, h], dtype="<i4").tobytes())
        f.write(flow.astype("<f4").tobytes())


def texture(h, w, seed):
    """a smooth random RGB texture (h, w, 3) in [0, 1]"""
    rng = np.random.default_rng(seed)
    coarse = rng.random((h // 6 + 2, w // 6 + 2, 3))
    ys = np.linspace(0, coarse.shape[0] - 1.001, h)
    xs = np.linspace(0, coarse.shape[1] - 1.001, w)
    sx, sy = np.meshgrid(xs, ys)
    return np.clip(bilinear(coarse, sx, sy) * 0.8 + 0.1 * rng.random((h, w, 3)), 0.0, 1.0)


def translated_sequence(dirpath, flow_dir, n_frames=3, h=60, w=80, shift=(3, 2), seed=0):
    """n_frames frames of one texture moved by shift = (dx, dy) pixels per frame (frame t shows the texture at offset
    t * shift: content at p in frame t came from p - shift in frame t-1), written as frame_{t}.png, with the exact flows
    backward_{t}_{t-1}.flo = -shift and forward_{t-1}_{t}.flo = +shift.  -> list of frame paths."""
    from PIL import Image
    dx, dy = shift
    big = texture(h + n_frames * dy + 8, w + n_frames * dx + 8, seed)
    os.makedirs(dirpath, exist_ok=True)
    os.makedirs(flow_dir, exist_ok=True)
    paths = []
    for t in range(n_frames):
        oy, ox = (n_frames - t) * dy, (n_frames - t) * dx
        frame = big[oy:oy + h, ox:ox + w]
        p = os.path.join(dirpath, f"frame_{t + 1:02d}.png")
        Image.fromarray((frame * 255).round().astype(np.uint8)).save(p)
        paths.append(p)
    for t in range(2, n_frames + 1):
        write_flo(os.path.join(flow_dir, f"backward_{t}_{t - 1}.flo"), np.broadcast_to(np.float32([-dx, -dy]), (h, w, 2)))
        write_flo(os.path.join(flow_dir, f"forward_{t - 1}_{t}.flo"), np.broadcast_to(np.float32([dx, dy]), (h, w, 2)))
    return paths


def consistency_error(outs, flow_b, flow_f=None):
    """E = mean over the frames t > 1 and the pixels with c = 1 of (out_t - warp(out_{t-1}))^2, outs (h, w, 3) in [0, 1]"""
    cert = certainty64(flow_b, flow_f).astype(bool)
    errs = []
    for prev, cur in zip(outs[:-1], outs[1:]):
        d = cur.astype(np.float64) - warp64(prev, flow_b)
        errs.append((d[cert] ** 2).mean())
    return float(np.mean(errs))
