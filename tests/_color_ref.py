"""Float64 numpy restatement of colour preservation: the ten colour sums, mean and covariance, the
affine colour transform of Gatys et al. (2016), its application, and the luminance merge.  Nothing here touches the
product's code; the tests compare the kernels and the operator surface with it."""
import math

import numpy as np

EPS = (1.0 / 255.0) ** 2
LUMA = np.array([0.299, 0.587, 0.114])
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def sums64(img, mask=None, exact=False):
    """(W, S_0, S_1, S_2, S_00, S_01, S_02, S_11, S_12, S_22) of an (h, w, 3) image under an (h, w) weight plane.  The
    terms are formed in float64 (a product of two float32 values is exact there); exact=True sums them with math.fsum (the
    correctly rounded sum), otherwise numpy's pairwise sum."""
    x = np.asarray(img, dtype=np.float64).reshape(-1, 3)
    m = np.ones(x.shape[0]) if mask is None else np.asarray(mask, dtype=np.float64).reshape(-1)
    assert m.shape[0] == x.shape[0]
    terms = [m] + [m * x[:, i] for i in range(3)] + [m * (x[:, i] * x[:, j]) for i, j in PAIRS]
    total = math.fsum if exact else np.sum
    return np.array([float(total(t)) for t in terms])


def stats_from_sums(s):
    """mu = S / W, Sigma = S_ij / W - mu mu^T"""
    s = np.asarray(s, dtype=np.float64)
    if s[0] == 0:
        raise ValueError("W == 0")
    mu = s[1:4] / s[0]
    second = np.zeros((3, 3))
    for k, (i, j) in enumerate(PAIRS):
        second[i, j] = second[j, i] = s[4 + k]
    return mu, second / s[0] - np.outer(mu, mu)


def stats64(img, mask=None, exact=False):
    return stats_from_sums(sums64(img, mask, exact))


def sym_power(sigma, power, eps=EPS):
    """(sigma + eps I)^power, symmetric, by a float64 eigh"""
    lam, vec = np.linalg.eigh(np.asarray(sigma, dtype=np.float64))
    return (vec * (lam + eps) ** power) @ vec.T


def transform64(mu_s, sigma_s, mu_c, sigma_c, eps=EPS):
    """A = (Sigma_c + eps I)^(1/2) (Sigma_s + eps I)^(-1/2), b = mu_c - A mu_s"""
    A = sym_power(sigma_c, 0.5, eps) @ sym_power(sigma_s, -0.5, eps)
    return A, np.asarray(mu_c, dtype=np.float64) - A @ np.asarray(mu_s, dtype=np.float64)


def expected_cov(sigma_c, A, eps=EPS):
    """cov(A s + b) = Sigma_c + eps (I - A A^T), exactly"""
    return np.asarray(sigma_c) + eps * (np.eye(3) - A @ A.T)


def affine64(img, A, b, mask=None):
    """s'(p) = A s(p) + b where mask(p) != 0 (None: everywhere), s(p) elsewhere; float64"""
    x = np.asarray(img, dtype=np.float64)
    y = x @ np.asarray(A, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
    if mask is None:
        return y
    return np.where(np.asarray(mask).reshape(x.shape[:-1] + (1,)) != 0, y, x)


def affine_bound(img, A, b):
    """per element |b_i| + sum_j |A_ij| |x_j|: what the float32 roundings of the kernel are relative to"""
    x = np.abs(np.asarray(img, dtype=np.float64))
    return x @ np.abs(np.asarray(A, dtype=np.float64)).T + np.abs(np.asarray(b, dtype=np.float64))


def match64(style, content, style_mask=None, content_mask=None):
    """the recoloured style in float64, and (A, b)"""
    A, b = transform64(*stats64(style, style_mask), *stats64(content, content_mask))
    return affine64(style, A, b, style_mask), A, b


def luma64(img):
    return np.asarray(img, dtype=np.float64) @ LUMA


def luma_merge64(result, content):
    """out_ch = c_ch + (Y(r) - Y(c))"""
    c = np.asarray(content, dtype=np.float64)
    return c + (luma64(result) - luma64(c))[..., None]


def colour_distance(img, content):
    """D(img) = |mean(img) - mean(c)|_2 + |cov(img) - cov(c)|_F"""
    mu, cov = stats64(img)
    mu_c, cov_c = stats64(content)
    return float(np.linalg.norm(mu - mu_c) + np.linalg.norm(cov - cov_c))


RGB2YUV = np.array(((0.299, -0.14714119, 0.61497538), (0.587, -0.28886916, -0.51496512), (0.114, 0.43601035, -0.10001026)))


def chroma_distance(img, content):
    """C(img) = mean over the pixels of the Euclidean (U, V) distance to the content"""
    d = (np.asarray(img, dtype=np.float64) - np.asarray(content, dtype=np.float64)) @ RGB2YUV[:, 1:]
    return float(np.sqrt((d ** 2).sum(-1)).mean())
