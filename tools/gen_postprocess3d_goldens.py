#!/usr/bin/env python3
"""Writes tests/golden/g22_postprocess3d.npz: binary VOLUMES and what the reference's `post_processing`
(dataloaders/utils.py:193-204) returns for them -- its scipy / skimage calls are n-dimensional and take a volume as they take a plane.

The reference's file is loaded IN PLACE by its path (`--reference DIR`, the directory that holds dataloaders/), as
tools/gen_postprocess_goldens.py loads it, with stand-in modules of this tool's own in sys.modules:

    skimage.measure.label       = scipy.ndimage.label with the full 3^ndim structure (skimage's default: connectivity = ndim)
    skimage.measure.regionprops = nothing (the reference discards its result)
    matplotlib.pyplot           = an empty module, only where matplotlib does not import

What the fixture pins is the reference's own: the hole filling (its call of scipy.ndimage.binary_fill_holes with the default
structure, on a volume the 6-neighbour cross), the total counted after filling, the `single_vol / total_cc < 0.2` rule in float64
and the loop that clears the components; the labelling is the stand-in's (26-connectivity, from skimage's documentation).
The tool asserts that tests/postprocess3d_ref.py (the numpy restatement the tests compare against) equals the reference's result
at every voxel of every volume, and that the fixture holds volumes that gain voxels by filling, lose a component, keep several
components, and come out empty: the four counts are stored as `counts` and none may be zero.

Volumes are stored per size as np.packbits of [n, D, H, W] (`in_<D>x<H>x<W>`, `out_<D>x<H>x<W>`) beside `sizes` [groups, 4] =
(n, D, H, W).

    python tools/gen_postprocess3d_goldens.py --reference /path/to/reference
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import postprocess3d_ref as R  # noqa: E402


def stand_ins():
    from scipy import ndimage
    measure = types.ModuleType("skimage.measure")

    def label(a, return_num=False):
        lab, n = ndimage.label(a, structure=np.ones((3,) * np.ndim(a)))
        return (lab, n) if return_num else lab

    measure.label = label
    measure.regionprops = lambda lab: None
    sk = types.ModuleType("skimage")
    sk.measure = measure
    sys.modules["skimage"], sys.modules["skimage.measure"] = sk, measure
    try:
        import matplotlib.pyplot  # noqa: F401
    except ImportError:
        mpl = types.ModuleType("matplotlib")
        mpl.pyplot = types.ModuleType("matplotlib.pyplot")
        sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, mpl.pyplot


def load_reference(root):
    path = os.path.join(os.path.abspath(root), "dataloaders", "utils.py")
    spec = importlib.util.spec_from_file_location("reference_dataloaders_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def blob_volume(rng, D, H, W, flip):
    """balls and shells (cavities, nested ones too), a few stray specks, then a share of flipped voxels"""
    zz, yy, xx = np.mgrid[:D, :H, :W]
    p = np.zeros((D, H, W), bool)
    for _ in range(rng.integers(1, 4)):
        cz, cy, cx = rng.integers(0, D), rng.integers(0, H), rng.integers(0, W)
        r = rng.integers(2, max(3, min(D, H, W) // 2 + 1))
        d2 = (zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2
        kind = rng.integers(0, 3)
        p |= d2 <= r * r if kind == 0 else (d2 <= r * r) & (d2 >= (r - 1) ** 2)
        if kind == 2:
            p |= d2 <= (r // 3) ** 2
    for _ in range(rng.integers(0, 4)):
        p[rng.integers(0, D), rng.integers(0, H), rng.integers(0, W)] = True
    return p ^ (rng.random((D, H, W)) < flip)


def hand_volumes(D, H, W):
    """the named cases of the issue, at 7 x 9 x 11"""
    blank = lambda: np.zeros((D, H, W), bool)
    out = []
    tube = blank()
    tube[:, 2:7, 2:7] = True
    tube[:, 3:6, 3:6] = False
    out.append(tube)                                    # a ring in every slice: open at both ends, nothing gained
    box = blank()
    box[1:6, 1:6, 1:6] = True
    box[2:5, 2:5, 2:5] = False
    out.append(box)                                     # the closed box gains its 27 voxels
    octa = blank()
    for dz, dy, dx in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        octa[3 + dz, 4 + dy, 5 + dx] = True
    out.append(octa)                                    # six voxels touching by edges enclose their centre
    corner = blank()
    corner[1:3, 1:3, 1:3] = corner[3:5, 3:5, 3:5] = True
    out.append(corner)                                  # two cubes touching by a corner: one component
    five = blank()
    for k in range(5):
        five[1:3, 1:3, 2 * k:2 * k + 1] = True
    out.append(five)                                    # five equal components: ratio exactly 0.2, all stay
    more = five.copy()
    more[D - 1, H - 1, W - 1] = True
    out.append(more)                                    # ... plus one voxel: every ratio below 0.2, the empty volume
    out.append(blank())
    stray = blank()
    stray[1:6, 1:6, 1:6] = True
    stray[3, 3, 3] = False
    stray[5, 7, 8:10] = True
    out.append(stray)                                   # a cube with a cavity and a stray blob that goes
    two = blank()
    two[0:3, 0:4, 0:4] = two[4:7, 5:9, 6:10] = True
    out.append(two)                                     # two kept components
    specks = blank()
    specks[::3, ::3, ::3] = True
    out.append(specks)                                  # many equal specks: all below a fifth, the empty volume
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's root directory (holds dataloaders/utils.py)")
    args = ap.parse_args()
    stand_ins()
    ref = load_reference(args.reference)
    rng = np.random.default_rng(22)
    z, sizes = {}, []
    gained = lost = several = empty = 0
    for D, H, W, n in ((7, 9, 11, 16), (5, 19, 70, 10), (2, 17, 65, 4), (9, 20, 33, 8), (1, 12, 13, 4)):
        vs = hand_volumes(D, H, W) if (D, H, W) == (7, 9, 11) else []
        while len(vs) < n:
            vs.append(blob_volume(rng, D, H, W, (0.0, 0.01, 0.3)[len(vs) % 3]))
        outs = []
        for p in vs:
            got = ref.post_processing(p.copy())
            assert got.dtype == bool and got.shape == p.shape
            mine = R.process(p)
            assert np.array_equal(got, mine), ("postprocess3d_ref differs from the reference", D, H, W, int((got != mine).sum()))
            f = R.fill(p)
            gained += int(f.sum() > p.sum())
            lost += int(got.sum() < f.sum())
            several += int(len(R.components(got)) > 1)
            empty += int(not got.any())
            outs.append(got)
        z["in_%dx%dx%d" % (D, H, W)] = np.packbits(np.stack(vs))
        z["out_%dx%dx%d" % (D, H, W)] = np.packbits(np.stack(outs))
        sizes.append((n, D, H, W))
    z["sizes"] = np.array(sizes, np.int32)
    z["counts"] = np.array([gained, lost, several, empty], np.int32)
    print("volumes %d: gained voxels %d, lost components %d, kept several %d, empty %d"
          % (sum(s[0] for s in sizes), gained, lost, several, empty))
    assert min(gained, lost, several, empty) > 0, "every count must be non-zero: choose other inputs"
    path = os.path.join(ROOT, "tests", "golden", "g22_postprocess3d.npz")
    np.savez_compressed(path, **z)
    print("wrote", os.path.normpath(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
