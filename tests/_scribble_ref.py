"""numpy restatement of strotss_scribble_labels, shared by test_scribble_cpu.py and
test_hip_scribble.py: the unary (score planes sampled bilinearly, softmax at temperature tau), the edge weights and the
Jacobi sweeps of the screened random walker that spreads a few strokes over an image, then the labels.  Every array is of
`dtype` (float64: the statement the kernels are tested against; float32: the yardstick of what the number format itself
costs), so the two runs differ only in their rounding.  Plus the seeds of the cell grid (the host code of
nn.strotss_utils.scribble_seeds restated with loops)."""
import numpy as np

TAU, LAMBDA, ITERS, SIGMA = 0.05, 0.05, 128, 0.1
MAX_K, MAX_ITERS = 7, 1024
CORNER_COLOURS = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]     # ascending (r, g, b); 0 = no stroke


def planes_in_workspace(k: int) -> int:
    """q, two buffers of x (k planes each), the weights toward the east and the south neighbour"""
    return 3 * k + 2


def _taps(s, n, dt):
    """the 4-neighbour rule of strotss_flow_warp along one axis: s clamped to [-2, n + 1], both neighbours clamped"""
    s = np.clip(s, dt(-2), dt(n + 1))
    fl = np.floor(s)
    i = fl.astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), s - fl


def sample_scores(scores, H, W, dtype=np.float64):
    """(gh, gw, k) -> (k, H, W): every plane at u = (y + 0.5) gh / H - 0.5, v = (x + 0.5) gw / W - 0.5, bilinearly"""
    dt = dtype
    g = np.asarray(scores).astype(dt)
    gh, gw, _ = g.shape
    y0, y1, fy = _taps((np.arange(H).astype(dt) + dt(0.5)) * dt(gh) / dt(H) - dt(0.5), gh, dt)
    x0, x1, fx = _taps((np.arange(W).astype(dt) + dt(0.5)) * dt(gw) / dt(W) - dt(0.5), gw, dt)
    fy, fx, one = fy[:, None, None], fx[None, :, None], dt(1)
    a, b = g[y0][:, x0], g[y0][:, x1]
    d, e = g[y1][:, x0], g[y1][:, x1]
    s = (one - fy) * ((one - fx) * a + fx * b) + fy * ((one - fx) * d + fx * e)
    return np.ascontiguousarray(np.moveaxis(s, 2, 0))


def unary(scores, H, W, tau=TAU, dtype=np.float64):
    """q (k, H, W) = softmax over the planes of sample_scores / tau, the maximum subtracted first"""
    t = sample_scores(scores, H, W, dtype) / dtype(tau)
    e = np.exp(t - t.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True)


def edge_weights(img, sigma=SIGMA, dtype=np.float64):
    """(wE, wS), each (H, W): exp(-|I(p) - I(p')|^2 / (2 sigma^2)) toward (y, x + 1) and (y + 1, x); 0 where that neighbour
    does not exist"""
    x = np.asarray(img).astype(dtype)
    two_s2 = dtype(2) * dtype(sigma) * dtype(sigma)
    wE, wS = np.zeros(x.shape[:2], dtype=dtype), np.zeros(x.shape[:2], dtype=dtype)
    wE[:, :-1] = np.exp(-((x[:, :-1] - x[:, 1:]) ** 2).sum(axis=2) / two_s2)
    wS[:-1] = np.exp(-((x[:-1] - x[1:]) ** 2).sum(axis=2) / two_s2)
    return wE, wS


def _shifted(a, dy, dx):
    """a (.., H, W) read at (y + dy, x + dx), 0 where that lies outside"""
    out = np.zeros_like(a)
    H, W = a.shape[-2:]
    ys, yd = (slice(1, H), slice(0, H - 1)) if dy > 0 else (slice(0, H - 1), slice(1, H)) if dy < 0 else (slice(None),) * 2
    xs, xd = (slice(1, W), slice(0, W - 1)) if dx > 0 else (slice(0, W - 1), slice(1, W)) if dx < 0 else (slice(None),) * 2
    out[..., yd, xd] = a[..., ys, xs]
    return out


def sweep(x, q, wE, wS, fixed, onehot, lam, dtype=np.float64):
    """one Jacobi sweep: (lambda q + sum w x(p')) / (lambda + sum w) over the neighbours inside the image; stroke pixels
    keep their one-hot"""
    wn, ws, ww, we = _shifted(wS, -1, 0), wS, _shifted(wE, 0, -1), wE
    num = dtype(lam) * q + wn * _shifted(x, -1, 0) + ws * _shifted(x, 1, 0) + ww * _shifted(x, 0, -1) + we * _shifted(x, 0, 1)
    den = dtype(lam) + wn + ws + ww + we
    return np.where(fixed[None], onehot, num / den)


def labels_of(x):
    """(label (H, W) int32 = the first arg-max over the planes, count (k,), margin (H, W) = largest - second largest)"""
    label = np.argmax(x, axis=0).astype(np.int32)
    top = np.sort(x, axis=0)
    return label, np.bincount(label.reshape(-1), minlength=x.shape[0]), top[-1] - top[-2]


def diffuse(img, stroke, scores, tau=TAU, lam=LAMBDA, sigma=SIGMA, iters=ITERS, dtype=np.float64):
    """The whole statement.  stroke: (H, W) ints, a label 0..k-1 or anything else.  iters: a count or an ascending tuple of
    counts.  -> dict(q, wE, wS, fixed) and, per count n, out[n] = dict(x (k, H, W), label, count, margin)."""
    H, W = stroke.shape
    k = int(np.asarray(scores).shape[2])
    q = unary(scores, H, W, tau, dtype)
    wE, wS = edge_weights(img, sigma, dtype)
    fixed = (stroke >= 0) & (stroke < k)
    onehot = (np.arange(k)[:, None, None] == stroke[None]).astype(dtype)
    x = np.where(fixed[None], onehot, q)
    out = dict(q=q, wE=wE, wS=wS, fixed=fixed)
    wanted = (iters,) if np.isscalar(iters) else tuple(iters)
    for n in range(1, max(wanted) + 1):
        x = sweep(x, q, wE, wS, fixed, onehot, lam, dtype)
        if n in wanted:
            label, count, margin = labels_of(x)
            out[n] = dict(x=x, label=label, count=count, margin=margin)
    return out


def seeds(stroke_small, g: int, gh: int, gw: int, k: int):
    """(gh, gw) int32: per cell the majority label among the stroke pixels of its g x g block of the small image, the lowest
    label on a tie, -1 without a stroke pixel"""
    out = np.full((gh, gw), -1, dtype=np.int32)
    for i in range(gh):
        for j in range(gw):
            block = stroke_small[i * g:(i + 1) * g, j * g:(j + 1) * g].reshape(-1)
            block = block[(block >= 0) & (block < k)]
            if block.size:
                out[i, j] = int(np.argmax(np.bincount(block, minlength=k)))
    return out


def nearest(a, H, W):
    """a (h, w) at (H, W) by nearest neighbour: pixel (y, x) takes (y h // H, x w // W)"""
    h, w = a.shape[:2]
    return a[(np.arange(H) * h // H)][:, (np.arange(W) * w // W)]
