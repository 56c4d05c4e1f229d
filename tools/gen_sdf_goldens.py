#!/usr/bin/env python3
"""Writes tests/golden/g20_sdf.npz: a handful of masks (at most 64 x 64) with their integer squared distances and the float64
signed distance map of the reference's compute_sdf (utils/util.py:208-239), computed with scipy -- the library the reference
calls.

The reference's own function cannot execute as written: it uses `np.bool`, which current numpy no longer has, and its
`skimage.segmentation` import is commented out (and skimage is not a dependency here).  So this file RESTATES lines 219-239:
`bool` for `np.bool`, scipy.ndimage.distance_transform_edt for `distance`, and for find_boundaries(posmask, mode="inner")
the rule it amounts to on a binary plane, posmask & ~binary_erosion(posmask, cross, border_value=1): a foreground pixel with a
background 4-neighbour inside the image.  Everything else is the reference's text.

Per mask i:  mask_i uint8;  to_fg_i / to_bg_i int64 = round(edt^2) of ~mask / mask (0 on the pixels of the kind itself, all -1
when the kind is absent);  sdf_i float64.  With the fixture committed, no test on the GPU needs scipy.

    python tools/gen_sdf_goldens.py
"""
import os
import sys

import numpy as np
from scipy import ndimage
from scipy.ndimage import distance_transform_edt as distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import distmap_ref as R  # noqa: E402  (only for the blob generator: the masks, none of the results)


CROSS = ndimage.generate_binary_structure(2, 1)


def minmax(d):
    return (d - d.min()) / (d.max() - d.min())


def sdf_of(mask):
    """utils/util.py:223-235 for one sample, step by step in the reference's order and float64 operations"""
    fg = mask.astype(np.uint8).astype(bool)                               # :219, :223
    if not fg.any():                                                      # :224 -- the sample keeps the zeros of :220
        return np.zeros(fg.shape)
    inside, outside = distance(fg), distance(~fg)                         # :226-227
    inner = fg & ~ndimage.binary_erosion(fg, CROSS, border_value=1)       # :228
    out = minmax(outside) - minmax(inside)                                # :231-233
    out[inner] = 0                                                        # :234
    return out


def masks():
    rng = np.random.default_rng(20)
    out = [R.blobs(rng, 64, 64), R.blobs(rng, 33, 47, flip=0.02), R.blobs(rng, 48, 20, n=2), R.blobs(rng, 17, 64, flip=0.2)]
    one = np.zeros((5, 5), bool)
    one[1, 3] = True
    out += [one, ~one, np.zeros((6, 9), bool)]
    yy, xx = np.mgrid[:31, :40]
    out.append((yy + xx) % 2 == 0)
    out.append(((yy - 15) ** 2 + (xx - 20) ** 2 <= 14 ** 2) & ((yy - 15) ** 2 + (xx - 20) ** 2 >= 6 ** 2))
    return out


def main():
    arrays = {}
    ms = masks()
    for i, m in enumerate(ms):
        assert max(m.shape) <= 64 and not m.all()          # (the reference divides 0 / 0 on a full mask: nothing to record)
        sq = lambda d: np.rint(d * d).astype(np.int64)      # noqa: E731
        arrays[f"mask_{i}"] = m.astype(np.uint8)
        arrays[f"to_fg_{i}"] = sq(distance(~m)) if m.any() else np.full(m.shape, -1, np.int64)
        arrays[f"to_bg_{i}"] = sq(distance(m))
        arrays[f"sdf_{i}"] = sdf_of(m)
    arrays["count"] = np.int64(len(ms))
    path = os.path.join(ROOT, "tests", "golden", "g20_sdf.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(ms), "masks")


if __name__ == "__main__":
    main()
