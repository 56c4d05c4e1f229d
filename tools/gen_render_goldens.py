#!/usr/bin/env python3
"""Writes tests/golden/g17_render.npz: inputs and the pictures the reference's utils/util.py draws for them
(draw_mask_and_save :367-390, draw_contour_and_save :299-365).

The reference's module is imported IN PLACE (`--reference DIR`, the directory that holds its utils/) and run unchanged; it imports
cv2, which need not be installed: a stand-in module of this tool's own sits in sys.modules,

    cvtColor = channel reversal,  imwrite = capture the array,
    dilate   = scipy.ndimage.grey_dilation(size of the kernel, mode="constant", cval=0)  (cv2's default border: background outside)

What the fixture pins:
  * mask overlay: every number is the REFERENCE'S OWN arithmetic (torch f32 for the range rule, numpy float64 for colour and
    halving, numpy's uint8 cast); the stand-in only reverses channels twice.  `<case>_out` is the captured picture.
  * contour overlay: the scaling and the drawing order are the reference's; the dilation and the final float -> uint8 step are
    the stand-in's.  `<case>_float` is the captured FLOAT image (what cv2.imwrite would be given; stored channel-first, [N,3,H,W], which
    packs better), `<case>_out` its rounding by
    the rule cv2 documents for saturate_cast<uchar> (round half to even, clamp) -- a rule this tool takes from the
    documentation, not from a run of cv2.
The tool asserts that tests/render_ref.py (the numpy restatement the GPU tests compare against) equals both at every pixel, and
that at most 0.5 % of a contour case's pixels lie within 1e-4 of a half-integer (the pixels the tests allow to differ by one level).

Images are stored as uint16 sources with a rule per image (render_ref.decode_image): [-1, 1], [0, 1] or raw [0, 256) -- the three
branches of the mask overlay's range rule; part planes as uint8 {0, 1, 2} (2: not 1, yet > 0), label maps as uint8 0..3.

    python tools/gen_render_goldens.py --reference /path/to/reference
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_ref as R  # noqa: E402

CAPTURED = []


def stand_in_cv2():
    from scipy import ndimage
    m = types.ModuleType("cv2")
    m.COLOR_RGB2BGR = 4
    m.cvtColor = lambda a, code: np.ascontiguousarray(a[..., ::-1])
    m.dilate = lambda a, k, iterations=1: ndimage.grey_dilation(a, size=k.shape, mode="constant", cval=0)
    m.imwrite = lambda path, a: CAPTURED.append(np.ascontiguousarray(a[..., ::-1]).copy()) or True     # BGR file order -> RGB
    return m


def blobs(rng, N, P, H, W, odd):
    """overlapping discs and frames, some touching all four borders; `odd`: a few pixels hold 2 (not 1, yet > 0)"""
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((N, P, H, W), np.uint8)
    for n in range(N):
        for i in range(P):
            for _ in range(2):
                cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(4, max(H, W) // 2)
                out[n, i] |= ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.uint8)
            if (n + i) % 2 == 0:                       # a frame along the border: its contour must stay inside the image
                out[n, i, :2] = out[n, i, -2:] = 1
                out[n, i, :, :2] = out[n, i, :, -2:] = 1
            if odd:
                out[n, i][rng.random((H, W)) < 0.02] = 2
    return out


def label_map(rng, N, H, W, top):
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((N, H, W), np.uint8)
    for n in range(N):
        for lab in range(1, top + 1):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(5, max(H, W) // 2)
            out[n][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = lab
        out[n, 0, :] = top
        out[n, :, -1] = 1
    return out


def as_planes(m, kind, parts):
    """the reference's argument for one image: [P,H,W] planes (labels as test.py's to_3d / unsqueeze gives them)"""
    import torch
    if kind == 1:
        return torch.stack([torch.from_numpy((m == i + 1).astype(np.float32)) for i in range(parts)])
    return torch.from_numpy(m.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's root directory (holds utils/util.py)")
    args = ap.parse_args()
    import torch
    sys.modules["cv2"] = stand_in_cv2()
    sys.path.insert(0, os.path.abspath(args.reference))
    from utils import util as ref_util
    assert os.path.abspath(ref_util.__file__).startswith(os.path.abspath(args.reference)), ref_util.__file__

    rng = np.random.default_rng(17)
    z = {}
    # name: (kind, N, C, P, H, W, rules)
    mask_cases = {
        "m_two_rules_c3": (0, 2, 3, 2, 40, 56, (0, 1)),          # one batch, two branches of the per-image rule
        "m_raw_c1_p3": (0, 2, 1, 3, 37, 41, (1, 2)),
        "m_labels_c1": (1, 1, 1, 3, 37, 41, (0,)),               # int64 labels 0..3, N = 1
        "m_five_parts_c1": (0, 2, 1, 5, 37, 41, (2, 0)),
        "m_labels_c1_p1": (1, 2, 1, 1, 40, 56, (1, 2)),          # labels through the 16-byte path
    }
    contour_cases = {
        "c_planes_c3": (0, 1, 3, 2, 40, 56, (0,)),
        "c_labels_c1": (1, 2, 1, 3, 40, 56, (1, 2)),
        "c_four_parts_c1": (0, 2, 1, 4, 37, 41, (2, 0)),
    }
    for group, cases in (("mask", mask_cases), ("contour", contour_cases)):
        z["cases_" + group] = np.array(list(cases))
        for name, (kind, N, C, P, H, W, rules) in cases.items():
            q = rng.integers(0, 65536, (N, C, H, W), dtype=np.uint16)
            z[name + "_q"], z[name + "_rule"] = q, np.array(rules, np.int32)
            z[name + "_kind"], z[name + "_parts"] = np.int32(kind), np.int32(P)
            make = (lambda: label_map(rng, N, H, W, min(P, 3))) if kind == 1 else (lambda: blobs(rng, N, P, H, W, odd=True))
            z[name + "_pred"] = make()
            if group == "contour":
                z[name + "_gt"] = make()
            img, pred, gt, parts = R.fixture_inputs(_View(z), name)
            del CAPTURED[:]
            for n in range(N):
                t = torch.from_numpy(img[n].copy())
                if group == "mask":
                    ref_util.draw_mask_and_save(t, as_planes(z[name + "_pred"][n], kind, P), "unused.png")
                else:
                    ref_util.draw_contour_and_save(t, as_planes(z[name + "_pred"][n], kind, P), as_planes(z[name + "_gt"][n], kind, P),
                                                   "unused.png")
            got = np.stack(CAPTURED)
            if group == "mask":
                assert got.dtype == np.uint8
                assert np.array_equal(got, R.mask_overlay(img, pred, parts)), name
                z[name + "_out"] = got
            else:
                assert got.dtype == np.float32, got.dtype
                assert np.array_equal(got, R.contour_float(img, pred, gt, parts)), name
                share = R.near_half(R.contour_value64(img, pred, gt, parts)).mean()
                assert share <= 0.005, (name, share)
                z[name + "_float"], z[name + "_out"] = np.ascontiguousarray(got.transpose(0, 3, 1, 2)), R.saturate(got)
                print(name, "pixels within 1e-4 of a half-integer: %.2e" % share)
    path = os.path.join(ROOT, "tests", "golden", "g17_render.npz")
    np.savez_compressed(path, **z)
    print("wrote", os.path.normpath(path), os.path.getsize(path), "bytes")


class _View:
    """the dict under construction, read the way render_ref reads the loaded file"""

    def __init__(self, d):
        self.d = d

    files = property(lambda self: list(self.d))

    def __getitem__(self, k):
        return self.d[k]


if __name__ == "__main__":
    main()
