#!/usr/bin/env python3
"""Writes tests/golden/g23_morph.npz: a handful of cup / disc masks and the reference's own GetBoundary outputs for them at widths
1, 3 and 5 (tests/test_morph_ref_host.py, tests/test_gpu_morph.py).

Runs only where the reference tree is on disk:

    python tools/gen_morph_goldens.py /path/to/reference

It imports the reference's dataloaders/custom_transforms.py in place and calls its GetBoundary class; `torchvision.transforms` and
`cv2`, which that module imports and this environment may lack, are the throw-away stubs of tools/gen_augment_goldens.py.  The file
holds data only: the masks (uint8 H x W x 2, channel 0 the cup, channel 1 the disc, as the reference's to_multilabel lays them out)
and the uint8 H x W maps GetBoundary returned for them as float64 arrays, which is what its pipeline hands it.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g23_morph.npz")
WIDTHS = (1, 3, 5)


def ellipse(h, w, cy, cx, ry, rx):
    y, x = np.mgrid[0:h, 0:w]
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0


def masks():
    rs = np.random.RandomState(23)
    m = {}
    disc, cup = ellipse(96, 96, 48, 50, 30, 26), ellipse(96, 96, 50, 52, 14, 11)
    m["nested_96"] = np.stack([cup, disc], -1)
    disc, cup = ellipse(96, 96, 20, 80, 28, 24), ellipse(96, 96, 14, 86, 12, 13)
    m["edge_96"] = np.stack([cup, disc], -1)                               # both parts run into the top and right edges
    m["no_cup_96"] = np.stack([np.zeros((96, 96), bool), ellipse(96, 96, 40, 40, 22, 33)], -1)
    disc = ellipse(96, 96, 48, 48, 34, 34) & ~ellipse(96, 96, 44, 56, 3, 3)       # a hole narrower than two widths, and speckle
    cup = (ellipse(96, 96, 48, 48, 12, 16) | (rs.rand(96, 96) < 0.01)) & disc
    m["hole_speckle_96"] = np.stack([cup, disc], -1)
    m["thin_96"] = np.stack([ellipse(96, 96, 60, 30, 2, 20), ellipse(96, 96, 60, 30, 4, 40)], -1)   # thinner than the band: erodes away
    disc, cup = ellipse(40, 56, 19, 30, 15, 22), ellipse(40, 56, 21, 27, 6, 9)
    m["nested_40x56"] = np.stack([cup, disc], -1)
    m["full_disc_40x56"] = np.stack([ellipse(40, 56, 10, 10, 5, 7), np.ones((40, 56), bool)], -1)
    return {k: v.astype(np.uint8) for k, v in m.items()}


def main():
    ref = sys.argv[1]
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from gen_augment_goldens import install_stubs
    install_stubs()
    warnings.simplefilter("ignore")
    from dataloaders import custom_transforms as tr
    out = {"names": np.array(sorted(masks())), "widths": np.array(WIDTHS, np.int32)}
    for name, mask in masks().items():
        out[f"{name}_mask"] = mask
        for w in WIDTHS:
            got = tr.GetBoundary(width=w)(mask.astype(np.float64))
            assert got.dtype == np.uint8 and got.shape == mask.shape[:2]
            out[f"{name}_w{w}"] = got
            print(name, mask.shape, "width", w, "band pixels", int(got.sum()))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
