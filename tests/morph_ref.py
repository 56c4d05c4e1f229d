"""numpy-only restatement of what csrc/morph.hip computes (include/ustrun.h: ustrun_chamfer_dist, ustrun_morph): the exact integer
distance to a set under the city-block (metric 0, scipy's cross) or chessboard (metric 1, scipy's full structure) metric, and the
binary morphology that is a threshold of it:

    binary_dilation(a, iterations=w, border_value=b)  ==  dist(a, outside=(b == 1)) <= w
    binary_erosion(a, iterations=w, border_value=b)   ==  dist(~a, outside=(b == 0)) > w

`outside=True` counts everything outside the box as part of the set: a pixel at index i of an axis of extent n is min(i + 1, n - i)
from it.  The box is the last `rank` axes of an array; leading axes are a batch.  Two forms of the distance: a brute force over all
pairs in int64 (small boxes) and a separable one (any box); tests/test_morph_ref_host.py pins both to scipy.ndimage and to each
other, the GPU tests compare the kernels with the separable form only.  get_boundary restates the reference's GetBoundary
(dataloaders/custom_transforms.py:630-647)."""
import numpy as np

INF = 1 << 20                   # "no source": larger than any distance in a box the kernels accept
DIST_NONE = 0x7fffffff          # USTRUN_DIST_NONE
L1, LINF = 0, 1
DILATE, ERODE, OPEN, CLOSE, BAND = range(5)


def _outside_dist(shape, rank):
    """min over the box's axes of min(i + 1, n - i), shape = the box"""
    out = np.full(shape, INF, np.int64)
    for ax in range(rank):
        n = shape[ax]
        i = np.arange(n, dtype=np.int64)
        d = np.minimum(i + 1, n - i).reshape([n if k == ax else 1 for k in range(rank)])
        out = np.minimum(out, d)
    return out


def dist_brute(a, metric, rank, outside=False):
    """int64 distance of every pixel to the set `a` (bool), all pairs; INF where there is no source"""
    a = np.asarray(a, bool)
    box = a.shape[a.ndim - rank:]
    flat = a.reshape((-1,) + box)
    out = np.empty(flat.shape, np.int64)
    pts = np.stack(np.meshgrid(*[np.arange(n, dtype=np.int64) for n in box], indexing="ij"), -1).reshape(-1, rank)
    for b in range(flat.shape[0]):
        src = pts[flat[b].reshape(-1)]
        if len(src):
            diff = np.abs(pts[:, None, :] - src[None, :, :])
            d = (diff.sum(-1) if metric == L1 else diff.max(-1)).min(1)
        else:
            d = np.full(len(pts), INF, np.int64)
        out[b] = d.reshape(box)
        if outside:
            out[b] = np.minimum(out[b], _outside_dist(box, rank))
    return out.reshape(a.shape)


def _op_l1(v, outside):
    """v'(i) = min over i' of v(i') + |i - i'| along the last axis; the outside is a 0 before index 0 and past the last one"""
    n = v.shape[-1]
    v = v.copy()
    d = np.full(v.shape[:-1], 0 if outside else INF, np.int64)
    for i in range(n):
        d = np.minimum(v[..., i], d + 1)
        v[..., i] = d
    d = np.full(v.shape[:-1], 0 if outside else INF, np.int64)
    for i in range(n - 1, -1, -1):
        d = np.minimum(v[..., i], d + 1)
        v[..., i] = d
    return np.minimum(v, INF)


def _op_linf(v, outside):
    """v'(i) = min over i' of max(v(i'), |i - i'|) along the last axis; the outside adds the candidates i + 1 and n - i"""
    n = v.shape[-1]
    j = np.arange(n, dtype=np.int64)
    out = np.empty_like(v)
    for i in range(n):
        out[..., i] = np.maximum(v, np.abs(j - i)).min(-1)
        if outside:
            out[..., i] = np.minimum(out[..., i], min(i + 1, n - i))
    return out


def dist_sep(a, metric, rank, outside=False):
    """the same distance, one 1-D operator per axis of the box"""
    a = np.asarray(a, bool)
    v = np.where(a, 0, INF).astype(np.int64)
    op = _op_l1 if metric == L1 else _op_linf
    for ax in range(a.ndim - rank, a.ndim):
        v = np.moveaxis(op(np.ascontiguousarray(np.moveaxis(v, ax, -1)), outside), -1, ax)
    return v


def dist(a, metric, rank, outside=False, brute=False):
    return (dist_brute if brute else dist_sep)(a, metric, rank, outside)


def chamfer(a, metric, rank, outside=0, brute=False):
    """(sd int64, flags) of ustrun_chamfer_dist: + d to the foreground on the background, - d to the background on the foreground;
    outside 0 / 1 / 2 = neither kind / background / foreground; flags 0 / 1 / 2 = empty / mixed / full box"""
    a = np.asarray(a, bool)
    d_fg = dist(a, metric, rank, outside == 2, brute)
    d_bg = dist(~a, metric, rank, outside == 1, brute)
    d_fg = np.where(d_fg >= INF, DIST_NONE, d_fg)
    d_bg = np.where(d_bg >= INF, DIST_NONE, d_bg)
    axes = tuple(range(a.ndim - rank, a.ndim))
    flags = np.where(a.any(axes), np.where((~a).any(axes), 1, 2), 0)
    return np.where(a, -d_bg, d_fg), flags


def binary_dilation(a, metric, rank, iterations=1, border_value=0, brute=False):
    return dist(np.asarray(a, bool), metric, rank, border_value == 1, brute) <= iterations


def binary_erosion(a, metric, rank, iterations=1, border_value=0, brute=False):
    return dist(~np.asarray(a, bool), metric, rank, border_value == 0, brute) > iterations


def binary_opening(a, metric, rank, iterations=1, border_value=0, brute=False):
    """scipy hands border_value to both halves"""
    return binary_dilation(binary_erosion(a, metric, rank, iterations, border_value, brute), metric, rank, iterations, border_value, brute)


def binary_closing(a, metric, rank, iterations=1, border_value=0, brute=False):
    return binary_erosion(binary_dilation(a, metric, rank, iterations, border_value, brute), metric, rank, iterations, border_value, brute)


def band(a, metric, rank, width, border_value=0, brute=False):
    return binary_dilation(a, metric, rank, width, border_value, brute) & ~binary_erosion(a, metric, rank, width, border_value, brute)


def morph(a, metric, rank, op, width, border_value=0, brute=False):
    return (binary_dilation, binary_erosion, binary_opening, binary_closing, band)[op](a, metric, rank, width, border_value, brute)


def distance_transform_cdt(a, metric, rank, brute=False):
    """scipy.ndimage.distance_transform_cdt of ONE box (a.ndim == rank): the distance to the nearest background on the foreground,
    0 on the background; -1 everywhere on an input without background"""
    a = np.asarray(a, bool)
    if a.all():
        return np.full(a.shape, -1, np.int64)
    return np.where(a, dist(~a, metric, rank, False, brute), 0)


def decode(mask, by_class, K):
    """the boolean parts [N, K, ...] the kernels read: planes binarised as != 0, or part c of a class map [N, ...] as == c + 1"""
    mask = np.asarray(mask)
    if by_class:
        return np.stack([mask == c + 1 for c in range(K)], 1)
    return mask != 0


def get_boundary(mask, width=5):
    """GetBoundary.__call__ (custom_transforms.py:633-647) on an H x W x 2 mask: per part, the pixels where the dilation and the
    erosion by `width` steps of the cross differ (their sum with the 2s zeroed), the two parts ORed, as uint8"""
    parts = []
    for c in range(2):
        part = np.asarray(mask)[:, :, c] != 0
        s = binary_dilation(part, L1, 2, width).astype(np.int64) + binary_erosion(part, L1, 2, width).astype(np.int64)
        s[s == 2] = 0
        parts.append(s)
    return ((parts[0] + parts[1]) > 0).astype(np.uint8)
