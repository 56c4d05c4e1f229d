"""Numpy restatement of the signed distance maps (include/ustrun.h: ustrun_signed_dist2, ustrun_sdf_from_dist2) the GPU tests
compare against: exact integer signed squared distances, the flags, and the float64 map of the reference's compute_sdf
(utils/util.py:219-239) -- `bool` where the reference writes `np.bool`, and its inner boundary
(skimage find_boundaries(posmask, mode="inner")) written as the rule it amounts to on a binary plane: a foreground pixel with a
background 4-neighbour inside the image.  tests/test_distmap_ref_host.py pins this file to a brute force, to scipy and to the
g20 fixture."""
import os

import numpy as np

DIST_NONE = 0x7fffffff
EMPTY, MIXED, FULL = 0, 1, 2
_INF = 1 << 20                    # > any column distance; its square stays far inside int64


def planes(mask, by_class=False, K=None):
    """the boolean planes [N,K,H,W] ustrun_signed_dist2 reads: (x != 0) of [N,(K,)H,W], or (x == c + 1) of a class map [N,H,W]"""
    mask = np.asarray(mask)
    if by_class:
        return np.stack([mask == c + 1 for c in range(K)], axis=1)
    return (mask if mask.ndim == 4 else mask[:, None]) != 0


def _col_dist(seed):
    """distance along each column to the nearest True of `seed` [H,W], _INF where the column has none"""
    H = seed.shape[0]
    g = np.where(seed, 0, _INF).astype(np.int64)
    for y in range(1, H):
        g[y] = np.minimum(g[y], g[y - 1] + 1)
    for y in range(H - 2, -1, -1):
        g[y] = np.minimum(g[y], g[y + 1] + 1)
    return np.minimum(g, _INF)


def dist2_to(seed):
    """exact squared Euclidean distance from every pixel to the nearest True pixel of `seed` [H,W] (inside the image only);
    None when seed has no True pixel.  Separable: column distances, then the minimum over the row of g^2 + dx^2."""
    if not seed.any():
        return None
    W = seed.shape[1]
    g2 = _col_dist(seed) ** 2                                   # [H,W']
    dx2 = (np.arange(W)[:, None] - np.arange(W)[None, :]) ** 2  # [W,W']
    return np.stack([(row[None, :] + dx2).min(axis=1) for row in g2])


def signed_dist2(p):
    """one boolean plane -> (s2 int32 [H,W], flag)"""
    p = np.asarray(p, bool)
    to_fg, to_bg = dist2_to(p), dist2_to(~p)
    if to_fg is None:
        return np.full(p.shape, DIST_NONE, np.int32), EMPTY
    if to_bg is None:
        return np.full(p.shape, -DIST_NONE, np.int32), FULL
    return np.where(p, -to_bg, to_fg).astype(np.int32), MIXED


def signed_dist2_batch(mask, by_class=False, K=None):
    """-> (s2 int32 [N,K,H,W], flags int32 [N,K])"""
    pl = planes(mask, by_class, K)
    res = [[signed_dist2(p) for p in row] for row in pl]
    return (np.stack([np.stack([s for s, _ in row]) for row in res]),
            np.array([[f for _, f in row] for row in res], np.int32))


def inner_boundary(p):
    """foreground pixels with a background 4-neighbour inside the image"""
    p = np.asarray(p, bool)
    bg = ~p
    nb = np.zeros_like(p)
    nb[1:] |= bg[:-1]
    nb[:-1] |= bg[1:]
    nb[:, 1:] |= bg[:, :-1]
    nb[:, :-1] |= bg[:, 1:]
    return p & nb


def sdf_from_dist2(s2, flag):
    """utils/util.py:224-235 in float64 from the integer distances: zeros unless the plane is mixed (the reference skips the empty
    plane and divides 0 / 0 on the full one)"""
    out = np.zeros(s2.shape, np.float64)
    if flag != MIXED:
        return out
    s = s2.astype(np.int64)
    posdis, negdis = np.sqrt(np.maximum(-s, 0).astype(np.float64)), np.sqrt(np.maximum(s, 0).astype(np.float64))
    out = (negdis - negdis.min()) / (negdis.max() - negdis.min()) - (posdis - posdis.min()) / (posdis.max() - posdis.min())
    out[s == -1] = 0.0
    return out


def sdf(p):
    """one boolean plane -> float64 [H,W]"""
    s2, flag = signed_dist2(p)
    return sdf_from_dist2(s2, flag)


def sdf_batch(mask, by_class=False, K=None):
    s2, flags = signed_dist2_batch(mask, by_class, K)
    return np.stack([np.stack([sdf_from_dist2(a, f) for a, f in zip(ra, rf)]) for ra, rf in zip(s2, flags)]), flags


def blobs(rng, H, W, n=3, flip=0.0):
    """a few discs and rings, optionally with pixel noise: objects with an inside, as labels have"""
    yy, xx = np.mgrid[:H, :W]
    p = np.zeros((H, W), bool)
    for _ in range(n):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(1, max(2, max(H, W) // 3))
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        p |= (d2 <= r * r) & (d2 >= (r // 3) ** 2)
    return p ^ (rng.random((H, W)) < flip)


def load_golden(path):
    """tests/golden/g20_sdf.npz -> list of (mask bool [H,W], to_fg int64, to_bg int64, sdf float64)"""
    z = np.load(path, allow_pickle=False)
    n = int(z["count"])
    return [(z[f"mask_{i}"].astype(bool), z[f"to_fg_{i}"], z[f"to_bg_{i}"], z[f"sdf_{i}"]) for i in range(n)]


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_sdf.npz")
