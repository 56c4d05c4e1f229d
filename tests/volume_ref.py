"""Numpy / scipy restatement of the volume kernels (include/ustrun.h: ustrun_signed_dist2_3d, ustrun_sdf_from_dist2_3d,
ustrun_surface_metrics_3d) and of the host functions on top of them, shared by tests/test_volume_ref_host.py (which pins this file
to an O(n^2) brute force and to the 2-D restatements) and tests/test_gpu_volumes.py.

    d2(p, q)   = wz^2 dz^2 + wy^2 dy^2 + wx^2 dx^2 with integer weights: rint(distance_transform_edt(sampling=weights)^2)
    border(A)  = A & ~erode(A), 6-neighbour cross, one iteration, background outside the volume
    record     = int32[10]: {|border(P)|, |border(G)|, d2[k], d2[k+1], max d2 over border(P), max d2 over border(G)},
                 f64 sum of sqrt(d2) over border(P), f64 the same over border(G)
    medpy      = medpy.metric.binary.__surface_distances restated with sampling=voxelspacing, and hd / hd95 / asd / assd on it
"""
import numpy as np
from scipy import ndimage as ndi

import distmap_ref as R2

DIST_NONE = 0x7fffffff
EMPTY, MIXED, FULL = 0, 1, 2


def volumes(mask, by_class=False, K=None):
    """the boolean volumes [N,K,D,H,W] the entries read: (x != 0) of [N,(K,)D,H,W], or (x == c + 1) of a class map [N,D,H,W]"""
    mask = np.asarray(mask)
    if by_class:
        return np.stack([mask == c + 1 for c in range(K)], axis=1)
    return (mask if mask.ndim == 5 else mask[:, None]) != 0


def dist2_to(seed, weights=(1, 1, 1)):
    """exact weighted squared distance from every voxel to the nearest True voxel of `seed` [D,H,W], int64; None without one"""
    if not seed.any():
        return None
    d = ndi.distance_transform_edt(~seed, sampling=[float(w) for w in weights])
    return np.rint(d * d).astype(np.int64)


def signed_dist2(p, weights=(1, 1, 1)):
    """one boolean volume -> (s2 int32 [D,H,W], flag)"""
    p = np.asarray(p, bool)
    to_fg, to_bg = dist2_to(p, weights), dist2_to(~p, weights)
    if to_fg is None:
        return np.full(p.shape, DIST_NONE, np.int32), EMPTY
    if to_bg is None:
        return np.full(p.shape, -DIST_NONE, np.int32), FULL
    return np.where(p, -to_bg, to_fg).astype(np.int32), MIXED


def signed_dist2_batch(mask, by_class=False, K=None, weights=(1, 1, 1)):
    """-> (s2 int32 [N,K,D,H,W], flags int32 [N,K])"""
    vol = volumes(mask, by_class, K)
    res = [[signed_dist2(p, weights) for p in row] for row in vol]
    return (np.stack([np.stack([s for s, _ in row]) for row in res]),
            np.array([[f for _, f in row] for row in res], np.int32))


def inner_boundary(p):
    """foreground voxels with a background 6-neighbour inside the volume"""
    p = np.asarray(p, bool)
    bg = ~p
    nb = np.zeros_like(p)
    nb[1:] |= bg[:-1]
    nb[:-1] |= bg[1:]
    nb[:, 1:] |= bg[:, :-1]
    nb[:, :-1] |= bg[:, 1:]
    nb[:, :, 1:] |= bg[:, :, :-1]
    nb[:, :, :-1] |= bg[:, :, 1:]
    return p & nb


def sdf_batch(mask, by_class=False, K=None):
    """utils/util.py:224-235 per volume in float64 (distmap_ref.sdf_from_dist2 takes any shape) -> (sdf [N,K,D,H,W], flags)"""
    s2, flags = signed_dist2_batch(mask, by_class, K)
    return np.stack([np.stack([R2.sdf_from_dist2(a, f) for a, f in zip(ra, rf)]) for ra, rf in zip(s2, flags)]), flags


def border(a):
    a = np.asarray(a, dtype=bool)
    p = np.pad(a, 1)
    c = slice(1, -1)
    return a & ~(p[:-2, c, c] & p[2:, c, c] & p[c, :-2, c] & p[c, 2:, c] & p[c, c, :-2] & p[c, c, 2:])


def d2_to(a, b, weights=(1, 1, 1)):
    """int64 weighted squared distance from each border(a) voxel (C order) to the nearest border(b) voxel"""
    return dist2_to(border(b), weights)[border(a)]


def record(p, g, weights=(1, 1, 1)):
    """the device record of one (case, part) as int32[10]; an empty border leaves everything but the two counts 0"""
    p, g = np.asarray(p, dtype=bool), np.asarray(g, dtype=bool)
    rec = np.zeros(10, dtype=np.int32)
    rec[0], rec[1] = border(p).sum(), border(g).sum()
    if rec[0] and rec[1]:
        dp, dg = d2_to(p, g, weights), d2_to(g, p, weights)
        u = np.sort(np.concatenate([dp, dg]))
        k = int(np.floor(0.95 * np.float64(len(u) - 1)))
        rec[2], rec[3], rec[4], rec[5] = u[k], u[min(k + 1, len(u) - 1)], dp.max(), dg.max()
        rec[6:10] = np.array([np.sqrt(dp.astype(np.float64)).sum(), np.sqrt(dg.astype(np.float64)).sum()]).view(np.int32)
    return rec


def records(pred, gt, by_class=False, n_classes=1, weights=(1, 1, 1)):
    """-> (records int32 [N,K,10], counts int64 [N,K,3] = {|P|, |G|, |P & G|})"""
    P, G = volumes(pred, by_class, n_classes), volumes(gt, by_class, n_classes)
    N, K = P.shape[:2]
    rec = np.stack([np.stack([record(P[n, k], G[n, k], weights) for k in range(K)]) for n in range(N)])
    cnt = np.array([[[P[n, k].sum(), G[n, k].sum(), (P[n, k] & G[n, k]).sum()] for k in range(K)] for n in range(N)], np.int64)
    return rec, cnt


def record_sums(rec):
    """the two f64 fields of records [...,10] -> [...,2]"""
    return np.ascontiguousarray(np.asarray(rec, dtype=np.int32)[..., 6:10]).view(np.float64)


def metrics_from_record(rec, cnt, unit=1.0):
    """dict of the six metrics of ONE (case, part) from its record and counts, in float64 (the arithmetic volume_metrics documents)"""
    s, g, i = (int(v) for v in cnt)
    if g == 0:
        raise RuntimeError("empty ground truth")
    out = {"dc": 2.0 * i / (s + g), "jc": i / float(s + g - i)}
    if s == 0:
        out.update(hd=100.0, hd95=100.0, asd=100.0, assd=100.0)
        return out
    n = int(rec[0]) + int(rec[1])
    pos = 0.95 * np.float64(n - 1)
    t = pos - np.floor(pos)
    a, b = unit * np.sqrt(np.float64(rec[2])), unit * np.sqrt(np.float64(rec[3]))
    sums = record_sums(rec)
    asd = unit * sums[0] / rec[0]
    out.update(hd=unit * np.sqrt(np.float64(max(rec[4], rec[5]))), hd95=b - (b - a) * (1 - t) if t >= 0.5 else a + (b - a) * t,
               asd=asd, assd=(asd + unit * sums[1] / rec[1]) / 2.0)
    return out


def medpy_surface_distances(result, reference, voxelspacing=None):
    """medpy.metric.binary.__surface_distances, restated: the distances from the result's border voxels to the reference's
    border, from a float distance transform with sampling=voxelspacing"""
    result, reference = np.asarray(result, bool), np.asarray(reference, bool)
    if not result.any() or not reference.any():
        raise RuntimeError("empty object")
    fp = ndi.generate_binary_structure(result.ndim, 1)
    rb = result ^ ndi.binary_erosion(result, structure=fp, iterations=1)
    fb = reference ^ ndi.binary_erosion(reference, structure=fp, iterations=1)
    return ndi.distance_transform_edt(~fb, sampling=voxelspacing)[rb]


def medpy_metrics(p, g, voxelspacing=None):
    """medpy's dc, jc, hd, hd95, asd, assd of one pair of masks, with the reference's rule for an empty prediction"""
    p, g = np.asarray(p, bool), np.asarray(g, bool)
    if not g.any():
        raise RuntimeError("empty ground truth")
    i, s, t = float((p & g).sum()), float(p.sum()), float(g.sum())
    out = {"dc": 2.0 * i / (s + t), "jc": i / (s + t - i)}
    if not p.any():
        out.update(hd=100.0, hd95=100.0, asd=100.0, assd=100.0)
        return out
    a, b = medpy_surface_distances(p, g, voxelspacing), medpy_surface_distances(g, p, voxelspacing)
    out.update(hd=max(a.max(), b.max()), hd95=np.percentile(np.hstack((a, b)), 95), asd=a.mean(), assd=np.mean((a.mean(), b.mean())))
    return out


def ball(shape, centre, radius, weights=(1, 1, 1)):
    zz, yy, xx = np.mgrid[:shape[0], :shape[1], :shape[2]]
    return (weights[0] * (zz - centre[0])) ** 2 + (weights[1] * (yy - centre[1])) ** 2 + (weights[2] * (xx - centre[2])) ** 2 <= radius ** 2


def blobs(rng, D, H, W, n=3, flip=0.0):
    """a few balls and shells, optionally with voxel noise: objects with an inside, as labels have"""
    p = np.zeros((D, H, W), bool)
    zz, yy, xx = np.mgrid[:D, :H, :W]
    for _ in range(n):
        cz, cy, cx = rng.integers(0, D), rng.integers(0, H), rng.integers(0, W)
        r = rng.integers(1, max(2, max(D, H, W) // 3))
        d2 = (zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2
        p |= (d2 <= r * r) & (d2 >= (r // 3) ** 2)
    return p ^ (rng.random((D, H, W)) < flip)
