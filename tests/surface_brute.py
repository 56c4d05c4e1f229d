"""Brute-force numpy restatement of the surface-distance metrics (the contract of ustrun_surface_metrics), shared by
tests/test_surface_metrics_host.py and tests/test_gpu_surface_metrics.py, and the reader of the g15 fixture.

    border(A) = A & ~erode(A): 4-neighbour cross, one iteration, background outside the image
    sds(A, B) = Euclidean distance from every border(A) pixel to the nearest border(B) pixel (all pairs, exact integers d2)
    hd95      = numpy.percentile(hstack(sds(P,G), sds(G,P)), 95);  asd = mean(sds(P,G));  |P| = 0 -> both 100
"""
import numpy as np


def border(a):
    a = np.asarray(a, dtype=bool)
    p = np.pad(a, 1)
    return a & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def d2_to(a, b, chunk=512):
    """int64 squared distance from each border(a) pixel (row-major order) to the nearest border(b) pixel."""
    ya, xa = np.nonzero(border(a))
    yb, xb = np.nonzero(border(b))
    out = np.empty(len(ya), dtype=np.int64)
    for o in range(0, len(ya), chunk):
        dy = ya[o:o + chunk, None].astype(np.int64) - yb[None]
        dx = xa[o:o + chunk, None].astype(np.int64) - xb[None]
        out[o:o + chunk] = (dy * dy + dx * dx).min(axis=1)
    return out


def record(p, g):
    """The device record of one (sample, part) as int32[6]: {|border(P)|, |border(G)|, d2[k], d2[k+1]}, f64 sum of sqrt(d2)
    over border(P) in the last two words; an empty mask leaves everything but the border counts 0."""
    p, g = np.asarray(p, dtype=bool), np.asarray(g, dtype=bool)
    rec = np.zeros(6, dtype=np.int32)
    rec[0], rec[1] = border(p).sum(), border(g).sum()
    if rec[0] and rec[1]:
        dp = d2_to(p, g)
        u = np.sort(np.concatenate([dp, d2_to(g, p)]))
        k = int(np.floor(0.95 * np.float64(len(u) - 1)))
        rec[2], rec[3] = u[k], u[min(k + 1, len(u) - 1)]
        rec[4:6] = np.array([np.sqrt(dp.astype(np.float64)).sum()]).view(np.int32)
    return rec


def counts(p, g):
    p, g = np.asarray(p, dtype=bool), np.asarray(g, dtype=bool)
    return np.array([p.sum(), g.sum(), (p & g).sum()], dtype=np.int64)


def metrics(p, g):
    """(dc, jc, hd95, asd) of one (sample, part) straight from the definitions (numpy.percentile, numpy.mean)."""
    p, g = np.asarray(p, dtype=bool), np.asarray(g, dtype=bool)
    s, t, i = counts(p, g)
    if t == 0:
        raise RuntimeError("empty ground truth")
    dc = 2.0 * i / float(s + t)
    jc = float(i) / float(s + t - i)
    if s == 0:
        return dc, jc, 100.0, 100.0
    dp = np.sqrt(d2_to(p, g).astype(np.float64))
    dg = np.sqrt(d2_to(g, p).astype(np.float64))
    return dc, jc, float(np.percentile(np.hstack((dp, dg)), 95)), float(dp.mean())


def planes(pred, gt, by_class=False, n_classes=1):
    """boolean [N, K, H, W] views of inputs given the way ustrun_dice_counts takes them"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    if by_class:
        cls = np.arange(1, n_classes + 1)[None, :, None, None]
        return pred[:, None] == cls, gt[:, None] == cls
    if pred.ndim == 3:
        pred, gt = pred[:, None], gt[:, None]
    return pred != 0, gt != 0


def records(pred, gt, by_class=False, n_classes=1):
    """-> (records int32 [N,K,6], counts int64 [N,K,3])"""
    P, G = planes(pred, gt, by_class, n_classes)
    N, K = P.shape[:2]
    rec = np.stack([np.stack([record(P[n, k], G[n, k]) for k in range(K)]) for n in range(N)])
    cnt = np.stack([np.stack([counts(P[n, k], G[n, k]) for k in range(K)]) for n in range(N)])
    return rec, cnt


def record_sum(rec):
    """the f64 field of records [...,6]"""
    return np.ascontiguousarray(np.asarray(rec, dtype=np.int32)[..., 4:6]).view(np.float64)[..., 0]


# ---- the g15 fixture (tools/gen_surface_goldens.py): bit-packed boolean planes + float64 expectations per case ----
def fixture_cases(z):
    return [str(n) for n in z["cases"]]


def fixture_inputs(z, name):
    """-> (pred, gt, by_class, n_classes) as numpy arrays in the dtype / layout the case is meant for:
    kind 0: float32 {0,1} planes [N,K,H,W];  kind 1: int64 class maps [N,H,W] whose part k is class k+1 (by_class)."""
    N, K, H, W = (int(v) for v in z[name + "_shape"])
    unpack = lambda a: np.unpackbits(a)[:N * K * H * W].reshape(N, K, H, W).astype(bool)
    P, G = unpack(z[name + "_pred"]), unpack(z[name + "_gt"])
    if int(z[name + "_kind"]) == 0:
        return P.astype(np.float32), G.astype(np.float32), False, K
    cls = np.arange(1, K + 1, dtype=np.int64)[None, :, None, None]
    return (P * cls).sum(1), (G * cls).sum(1), True, K
