"""References the convolution tests share: the float64 3x3 convolution as nine shifted GEMMs (none of the project's
kernels; tests/test_hip_conv_routes.py checks it against torch.nn.functional.conv2d), the sign words of
include/strotss_hip.h, and a float32 NumPy restatement of Lavin & Gray's F(2x2,3x3) / F(4x4,3x3) that serves as the
yardstick of what the Winograd algorithm itself costs in float32 (tests/test_hip_regime.py).  A plain module."""
import numpy as np
import torch

BT4 = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
       [0, 4, 0, -5, 0, 1]]
AT4 = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]
G4 = [[1.0 / 4, 0, 0], [-1.0 / 6, -1.0 / 6, -1.0 / 6], [-1.0 / 6, 1.0 / 6, -1.0 / 6], [1.0 / 24, 1.0 / 12, 1.0 / 6],
      [1.0 / 24, -1.0 / 12, 1.0 / 6], [0, 0, 1.0]]
BT2 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
AT2 = [[1, 1, 1, 0], [0, 1, -1, -1]]
G2 = [[1.0, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1.0]]
LAVIN_GRAY = {4: (BT4, AT4, G4), 2: (BT2, AT2, G2)}


def conv64(x, w):
    """float64 3x3 convolution with zero padding 1 as nine shifted GEMMs: x (1, h, w, ci), w (3, 3, ci, co) -> (1, h, w, co)."""
    h, wd = int(x.shape[1]), int(x.shape[2])
    xp = torch.nn.functional.pad(x[0].double(), (0, 0, 1, 1, 1, 1))
    w = w.double()
    out = torch.zeros(h, wd, int(w.shape[3]), dtype=torch.float64, device=x.device)
    for r in range(3):
        for q in range(3):
            out += torch.matmul(xp[r:r + h, q:q + wd], w[r, q])
    return out[None]


def sign_words(act):
    """relu_bits of include/strotss_hip.h for a (1, h, w, c) tensor: word (tile, ch), byte r, bit q = act[4ty+r, 4tx+q, ch] > 0;
    and the mask of the bits that lie inside the image (the others are unspecified)."""
    _, h, w, c = act.shape
    th, tw = (h + 3) // 4, (w + 3) // 4
    pos = torch.zeros(th * 4, tw * 4, c, dtype=torch.bool, device=act.device)
    inside = torch.zeros_like(pos)
    pos[:h, :w] = act[0] > 0
    inside[:h, :w] = True
    words = torch.zeros(th * tw, c, dtype=torch.int64, device=act.device)
    valid = torch.zeros_like(words)
    for r in range(4):
        for q in range(4):
            words |= pos[r::4, q::4].reshape(th * tw, c).long() << (8 * r + q)
            valid |= inside[r::4, q::4].reshape(th * tw, c).long() << (8 * r + q)
    return words, valid


def winograd_f32(x, w, tile):
    """Lavin & Gray's F(tile x tile, 3x3) in float32 NumPy: x (1, h, w, ci) float32, w (3, 3, ci, co) float32 ->
    (1, h, w, co) float32 without bias.  U = G g G^T is made in float64 and rounded once (as the library's weight
    transform states it); V = B^T d B, the (tile + 2)^2 GEMMs M = V U and Y = A^T M A are float32 throughout."""
    BT, AT, G = (np.asarray(m, dtype=np.float64) for m in LAVIN_GRAY[tile])
    x = np.asarray(x, dtype=np.float32)[0]
    h, wd, ci = x.shape
    co = w.shape[3]
    P = tile + 2
    th, tw = -(-h // tile), -(-wd // tile)
    U = np.einsum("ar,rqcn,bq->abcn", G, np.asarray(w, dtype=np.float64), G).astype(np.float32)
    xp = np.zeros((th * tile + 2, tw * tile + 2, ci), dtype=np.float32)
    xp[1:h + 1, 1:wd + 1] = x
    d = np.empty((P, P, th, tw, ci), dtype=np.float32)
    for r in range(P):
        for q in range(P):
            d[r, q] = xp[r:r + th * tile:tile, q:q + tw * tile:tile]
    BT32, AT32 = BT.astype(np.float32), AT.astype(np.float32)

    def sandwich(T, v):                  # T v T^T over the two leading axes, one float32 rounding per operation
        t1 = np.zeros((T.shape[0],) + v.shape[1:], dtype=np.float32)
        for a in range(T.shape[0]):
            for r in range(T.shape[1]):
                if T[a, r]:
                    t1[a] += T[a, r] * v[r]
        t2 = np.zeros((T.shape[0], T.shape[0]) + v.shape[2:], dtype=np.float32)
        for b in range(T.shape[0]):
            for q in range(T.shape[1]):
                if T[b, q]:
                    t2[:, b] += T[b, q] * t1[:, q]
        return t2

    V = sandwich(BT32, d).reshape(P, P, th * tw, ci)
    M = np.matmul(V, U)                  # (P, P, tiles, co), float32
    Y = sandwich(AT32, M).reshape(tile, tile, th, tw, co)
    out = Y.transpose(2, 0, 3, 1, 4).reshape(th * tile, tw * tile, co)[:h, :wd]
    return torch.from_numpy(np.ascontiguousarray(out))[None]
