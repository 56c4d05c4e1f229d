#!/usr/bin/env python3
"""Writes tests/golden/g15_surface_metrics.npz: masks and the float64 dc / jc / hd95 / asd the reference's test() would print
for them (train.py:306-320: medpy.metric.binary.dc / jc / hd95 / asd), restated here with scipy.ndimage from their definitions:

    border(A) = A & ~binary_erosion(A, generate_binary_structure(2, 1), iterations=1, border_value=0)
    sds(A, B) = distance_transform_edt(~border(B))[border(A)]
    hd95 = numpy.percentile(hstack(sds(P,G), sds(G,P)), 95);  asd = sds(P,G).mean();  |P| = 0 -> hd95 = asd = 100
    dc = 2|P&G| / (|P|+|G|);  jc = |P&G| / |P|G|

Also stored: the border sizes and the two integer order statistics d2[k], d2[min(k+1, n-1)], k = floor(0.95 (n-1)), of the
squared distances (exact: edt's distances are square roots of integers).  Masks are bit-packed boolean planes [N,K,H,W];
kind 1 cases are meant to be fed as int64 class maps (part k = class k+1, the M&Ms convention).  Needs scipy; the tests do not.

    python tools/gen_surface_goldens.py
"""
import os

import numpy as np
from scipy import ndimage

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CROSS = ndimage.generate_binary_structure(2, 1)


def border(a):
    return a & ~ndimage.binary_erosion(a, structure=CROSS, iterations=1, border_value=0)


def sds(a, b):
    return ndimage.distance_transform_edt(~border(b))[border(a)]


def expect(p, g):
    """-> (dc, jc, hd95, asd, |border(P)|, |border(G)|, d2[k], d2[k+1])"""
    s, t, i = int(p.sum()), int(g.sum()), int((p & g).sum())
    assert t > 0, "the fixture holds no empty ground truth (the reference cannot score one)"
    dc, jc = 2.0 * i / float(s + t), float(i) / float(s + t - i)
    nb = (int(border(p).sum()), int(border(g).sum()))
    if s == 0:
        return (dc, jc, 100.0, 100.0) + nb + (0, 0)
    dp, dg = sds(p, g), sds(g, p)
    u = np.hstack((dp, dg))
    d2 = np.sort(np.rint(u * u).astype(np.int64))
    assert np.array_equal(np.sqrt(d2.astype(np.float64)), np.sort(u))          # the distances are exact roots of integers
    k = int(np.floor(0.95 * np.float64(len(u) - 1)))
    return (dc, jc, float(np.percentile(u, 95)), float(dp.mean())) + nb + (int(d2[k]), int(d2[min(k + 1, len(u) - 1)]))


def disc(H, W, cy, cx, r):
    yy, xx = np.mgrid[:H, :W]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def rand_disc(rng, H, W, rmin=0.15, rspan=0.15):
    """centre and radius drawn as ustrun.synthetic._discs does"""
    return (0.3 + 0.4 * rng.random()) * H, (0.3 + 0.4 * rng.random()) * W, (rmin + rspan * rng.random()) * min(H, W)


def blobs(rng, H, W, n, smax=7):
    """many small components: n random rectangles of 1..smax pixels a side"""
    a = np.zeros((H, W), bool)
    for _ in range(n):
        y, x, h, w = rng.integers(0, H), rng.integers(0, W), rng.integers(1, smax + 1), rng.integers(1, smax + 1)
        a[y:y + h, x:x + w] = True
    return a


def fundus_like(rng, N, H, W):
    """[N,2,H,W]: cup inside disc, the prediction a displaced / rescaled copy (discs and rings like synthetic.labels)"""
    P, G = np.zeros((N, 2, H, W), bool), np.zeros((N, 2, H, W), bool)
    for n in range(N):
        cy, cx, r = rand_disc(rng, H, W)
        G[n, 1], G[n, 0] = disc(H, W, cy, cx, r), disc(H, W, cy, cx, 0.5 * r)
        dy, dx, f = rng.normal(0, 0.03 * H), rng.normal(0, 0.03 * W), 1 + rng.normal(0, 0.1)
        P[n, 1], P[n, 0] = disc(H, W, cy + dy, cx + dx, r * f), disc(H, W, cy + dy, cx + dx, 0.5 * r * f)
    return P, G


def rings(rng, N, H, W):
    """[N,3,H,W] disjoint rings (class k+1 = part k), the prediction displaced: the M&Ms class-map convention"""
    P, G = np.zeros((N, 3, H, W), bool), np.zeros((N, 3, H, W), bool)
    for n in range(N):
        cy, cx, r = rand_disc(rng, H, W)
        for M, (oy, ox, f) in ((G, (0, 0, 1)), (P, (rng.normal(0, 0.02 * H), rng.normal(0, 0.02 * W), 1 + rng.normal(0, 0.08)))):
            a, b, c = (disc(H, W, cy + oy, cx + ox, r * f * q) for q in (1.0, 0.7, 0.4))
            M[n, 0], M[n, 1], M[n, 2] = a & ~b, b & ~c, c
    return P, G


def speckle(rng, N, H, W):
    """[N,1,H,W] many small components; sample 0: the prediction is noise inside a disc, sample 1: identical masks"""
    P, G = np.zeros((N, 1, H, W), bool), np.zeros((N, 1, H, W), bool)
    for n in range(N):
        G[n, 0], P[n, 0] = blobs(rng, H, W, 250), blobs(rng, H, W, 250)
    cy, cx, r = rand_disc(rng, H, W)
    P[0, 0] = disc(H, W, cy, cx, r) & (rng.random((H, W)) < 0.5)
    P[1, 0] = G[1, 0]
    return P, G


def frame(rng, N, H, W):
    """[N,1,H,W], N >= 6: foreground touching and filling the image frame, a single pixel, far-apart masks, an empty prediction"""
    assert N >= 6
    P, G = np.zeros((N, 1, H, W), bool), np.zeros((N, 1, H, W), bool)
    G[0, 0], P[0, 0] = True, disc(H, W, H / 2, W / 2, 0.3 * min(H, W))                       # ground truth fills the frame
    G[1, 0, :H // 3], P[1, 0, :, :W // 4] = True, True                                        # both touch the frame
    G[2, 0, H // 2, W // 2], P[2, 0, 1, W - 2] = True, True                                   # single pixels
    G[3, 0], P[3, 0] = disc(H, W, 0.1 * H, 0.1 * W, 0.08 * min(H, W)), disc(H, W, 0.9 * H, 0.9 * W, 0.08 * min(H, W))   # far apart
    G[4, 0] = disc(H, W, H / 2, W / 2, 0.2 * min(H, W))                                       # empty prediction: the 100 rule
    G[5, 0, 0, 0], P[5, 0, H - 1, W - 1] = True, True                                         # opposite corners: the largest d2
    for n in range(6, N):
        G[n, 0], P[n, 0] = disc(H, W, *rand_disc(rng, H, W)), True                            # the prediction fills the frame
    return P, G


CASES = [  # name, kind (0: f32 planes, 1: int64 class map), generator, N, H, W
    ("discs_256", 0, fundus_like, 4, 256, 256),
    ("rings_288_i64", 1, rings, 4, 288, 288),
    ("speckle_384", 0, speckle, 4, 384, 384),
    ("frame_512", 0, frame, 7, 512, 512),
    ("discs_512", 0, fundus_like, 4, 512, 512),
    ("frame_40x72", 0, frame, 7, 40, 72),
    ("speckle_40x72", 0, speckle, 4, 40, 72),
    ("rings_40x72_i64", 1, rings, 4, 40, 72),
]


def main():
    out = {"cases": np.array([c[0] for c in CASES])}
    for ci, (name, kind, gen, N, H, W) in enumerate(CASES):
        P, G = gen(np.random.default_rng(1500 + ci), N, H, W)
        K = P.shape[1]
        e = np.array([[expect(P[n, k], G[n, k]) for k in range(K)] for n in range(N)])
        out[name + "_shape"] = np.array([N, K, H, W], dtype=np.int32)
        out[name + "_kind"] = np.int32(kind)
        out[name + "_pred"], out[name + "_gt"] = np.packbits(P), np.packbits(G)
        for j, key in enumerate(("dc", "jc", "hd95", "asd")):
            out[f"{name}_{key}"] = e[..., j].astype(np.float64)
        out[name + "_nborder"] = e[..., 4:6].astype(np.int32)
        out[name + "_d2"] = e[..., 6:8].astype(np.int32)
        print(f"{name}: N {N} K {K} {H}x{W}  hd95 {e[..., 2].min():.3f}..{e[..., 2].max():.3f}  asd {e[..., 3].min():.3f}..{e[..., 3].max():.3f}")
    path = os.path.join(ROOT, "tests", "golden", "g15_surface_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
