#!/usr/bin/env python3
"""Writes tests/golden/g18_postprocess.npz: binary planes and what the reference's `post_processing`
(dataloaders/utils.py:193-204) returns for them.

The reference's file is loaded IN PLACE by its path (`--reference DIR`, the directory that holds dataloaders/), not through its
package, whose __init__ imports cv2.  The file imports skimage.measure and matplotlib.pyplot, which need not be installed:
stand-in modules of this tool's own sit in sys.modules,

    skimage.measure.label       = scipy.ndimage.label with the full 3x3 structure (skimage's default connectivity for a plane)
    skimage.measure.regionprops = nothing (the reference discards its result)
    matplotlib.pyplot           = an empty module, only where matplotlib does not import

What the fixture pins:
  * the reference's own: the hole filling (its call of scipy.ndimage.binary_fill_holes with the default structure), the total
    counted after filling, the `single_vol / total_cc < 0.2` rule in float64 and the loop that clears the components;
  * the stand-in's: the labelling, i.e. which pixels form one component (8-connectivity, taken from skimage's documentation,
    not from a run of skimage).
The tool asserts that tests/postprocess_ref.py (the numpy restatement the tests compare against) equals the reference's result
at every pixel of every plane, and that the fixture holds at least three planes each that gain pixels by filling, lose a
component, keep several components, and come out empty.

Planes are stored per size as np.packbits of [n, H, W] (`in_<H>x<W>`, `out_<H>x<W>`) beside `sizes` [groups, 3] = (n, H, W).

    python tools/gen_postprocess_goldens.py --reference /path/to/reference
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import postprocess_ref as R  # noqa: E402


def stand_ins():
    from scipy import ndimage
    measure = types.ModuleType("skimage.measure")

    def label(a, return_num=False):
        lab, n = ndimage.label(a, structure=np.ones((3, 3)))
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


def blob_plane(rng, H, W, flip):
    """discs and rings (holes, nested ones too), a few stray specks, then a share of flipped pixels"""
    yy, xx = np.mgrid[:H, :W]
    p = np.zeros((H, W), bool)
    for _ in range(rng.integers(1, 4)):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(2, max(3, min(H, W) // 2))
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        kind = rng.integers(0, 3)
        p |= d2 <= r * r if kind == 0 else (d2 <= r * r) & (d2 >= (r - 2) ** 2)
        if kind == 2:
            p |= d2 <= (r // 3) ** 2
    for _ in range(rng.integers(0, 4)):
        p[rng.integers(0, H), rng.integers(0, W)] = True
    return p ^ (rng.random((H, W)) < flip)


def hand_planes(H, W):
    out = []
    five = np.zeros((H, W), bool)
    for k in range(5):
        five[1:3, 1 + 3 * k:3 + 3 * k] = True
    out.append(five)                                    # five equal components: ratio exactly 0.2, all stay
    more = five.copy()
    more[H - 1, W - 1] = True
    out.append(more)                                    # ... plus one pixel: every ratio below 0.2, the empty plane
    dia = np.zeros((H, W), bool)
    dia[4, 5] = dia[6, 5] = dia[5, 4] = dia[5, 6] = True
    out.append(dia)                                     # the diamond encloses its centre
    frame = np.zeros((H, W), bool)
    frame[0] = frame[-1] = True
    frame[:, 0] = frame[:, -1] = True
    out.append(frame)                                   # a frame along the border: the full plane
    out.append(np.zeros((H, W), bool))
    two = np.zeros((H, W), bool)
    two[2:8, 2:8] = two[9:15, 10:16] = True
    two[4, 4] = False
    out.append(two)                                     # two kept components, one with a hole
    specks = np.zeros((H, W), bool)
    specks[::4, ::4] = True
    out.append(specks)                                  # many equal specks: all below a fifth, the empty plane
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's root directory (holds dataloaders/utils.py)")
    args = ap.parse_args()
    stand_ins()
    ref = load_reference(args.reference)
    rng = np.random.default_rng(18)
    z, sizes = {}, []
    gained = lost = several = empty = 0
    for H, W, n in ((17, 23, 24), (33, 65, 20), (64, 64, 20), (96, 136, 10), (130, 70, 10)):
        ps = hand_planes(H, W) if (H, W) == (17, 23) else []
        while len(ps) < n:
            ps.append(blob_plane(rng, H, W, (0.0, 0.02, 0.3)[len(ps) % 3]))
        outs = []
        for p in ps:
            got = ref.post_processing(p.copy())
            assert got.dtype == bool and got.shape == p.shape
            mine = R.process(p)
            assert np.array_equal(got, mine), ("postprocess_ref differs from the reference", H, W, int((got != mine).sum()))
            f = R.fill(p)
            gained += int(f.sum() > p.sum())
            lost += int(got.sum() < f.sum())
            several += int(len(R.components(got)) > 1)
            empty += int(not got.any())
            outs.append(got)
        z["in_%dx%d" % (H, W)] = np.packbits(np.stack(ps))
        z["out_%dx%d" % (H, W)] = np.packbits(np.stack(outs))
        sizes.append((n, H, W))
    z["sizes"] = np.array(sizes, np.int32)
    print("planes %d: gained pixels %d, lost components %d, kept several %d, empty %d"
          % (sum(s[0] for s in sizes), gained, lost, several, empty))
    assert min(gained, lost, several, empty) >= 3
    path = os.path.join(ROOT, "tests", "golden", "g18_postprocess.npz")
    np.savez_compressed(path, **z)
    print("wrote", os.path.normpath(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
