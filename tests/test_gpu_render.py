"""The overlay kernels (csrc/render.hip) against the fixture g17, which the reference's own utils/util.py drew
(tools/gen_render_goldens.py), and against its numpy restatement tests/render_ref.py.

Bars.  Mask overlay: equal at EVERY pixel -- the range rule is two f32 steps rounded one by one, the colour sum and the halving
are exact in float64, the cast truncates; nothing is left to differ.  Per-image range: equal to torch.amin / amax (min and max
are exact in any order).  Contour overlay: equal at every pixel except that a pixel whose value, evaluated in float64 by
render_ref, lies within 1e-4 of a half-integer may differ by one level (the f32 quotient is correctly rounded on both sides, so
none is expected to; the allowance covers a last-place difference of the scaling steps deciding a tie) -- such pixels are at
most 0.5 % of a case, asserted here and by the generator on the CPU."""
import numpy as np
import pytest
import torch

import render_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
CAP = 0.005


@pytest.fixture(scope="module")
def Z():
    return load_golden("g17_render")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cases(kind):
    return R.fixture_cases(load_golden("g17_render"), kind)


@pytest.mark.parametrize("name", _cases("mask"))
def test_mask_overlay_equals_the_reference_at_every_pixel(Z, name):
    """the three range branches (two of them inside one batch: the rule is per image), overlapping parts (lowest index wins),
    planes holding values other than 0 and 1, both prediction forms, C = 1 and 3, 40 x 56 (16-byte path) and 37 x 41 (scalar)"""
    from ustrun import render
    img, pred, _, parts = R.fixture_inputs(Z, name)
    got = render.render_mask(dev(img), dev(pred), parts=parts)
    assert got.dtype == torch.uint8 and tuple(got.shape) == img.shape[:1] + img.shape[2:] + (3,)
    got = got.cpu().numpy()
    print(name, "pixels that differ:", int((got != Z[name + "_out"]).any(-1).sum()))
    assert np.array_equal(got, Z[name + "_out"])
    if pred.dtype == np.int64:                                 # without a part count every colour is tried: the same picture
        assert np.array_equal(render.render_mask(dev(img), dev(pred)).cpu().numpy(), got)
    if len(img) > 1:                                           # N = 1, and an image's picture does not depend on its batch
        one = render.render_mask(dev(img[1:]), dev(pred[1:]), parts=parts).cpu().numpy()
        assert np.array_equal(one[0], got[1])


def test_range_equals_torch_on_a_multi_wave_reduction():
    from ustrun import render
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 1, 256, 256, generator=g).cuda()
    x[1] = x[1] * 40 + 3
    got = render.image_range(x)
    assert torch.equal(got[:, 0], torch.amin(x, dim=(1, 2, 3))) and torch.equal(got[:, 1], torch.amax(x, dim=(1, 2, 3)))
    y = torch.rand(3, 3, 37, 41, generator=g).cuda()           # 3 * 37 * 41 is no multiple of 4: the scalar tail
    got = render.image_range(y)
    assert torch.equal(got[:, 0], torch.amin(y, dim=(1, 2, 3))) and torch.equal(got[:, 1], torch.amax(y, dim=(1, 2, 3)))


def _check_contour(got, img, pred, gt, parts, want, what):
    near = R.near_half(R.contour_value64(img, pred, gt, parts))
    assert near.mean() <= CAP, f"{what}: {near.mean():.4f} of the pixels sit near a half-integer"
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print(f"{what}: max |d| {d.max()}, differing {int((d != 0).sum())}, near a half-integer {int(near.sum())}")
    assert (d[~near] == 0).all() and d.max() <= 1, what


@pytest.mark.parametrize("name", _cases("contour"))
def test_contour_overlay_equals_the_fixture(Z, name):
    from ustrun import render
    img, pred, gt, parts = R.fixture_inputs(Z, name)
    want = Z[name + "_out"]
    assert np.array_equal(want, R.contour_overlay(img, pred, gt, parts))
    got = render.render_contour(dev(img), dev(pred), dev(gt), parts=parts).cpu().numpy()
    _check_contour(got, img, pred, gt, parts, want, name)
    one = render.render_contour(dev(img[-1:]), dev(pred[-1:]), dev(gt[-1:]), parts=parts).cpu().numpy()      # N = 1
    assert np.array_equal(one[0], got[-1])


@pytest.mark.parametrize("H,W", [(12, 16), (11, 13)])
def test_contour_drawing_order_borders_and_constant_image(H, W):
    """a prediction contour and a ground-truth contour on the same pixels: red wins; parts touching all four borders draw inside
    the image only; a constant image is 0 outside the contours (the reference has 0 / 0 there)"""
    from ustrun import render
    g = np.random.default_rng(5)
    img = g.random((2, 1, H, W), dtype=np.float32)
    img[1] = 0.25                                              # constant
    pred = np.zeros((2, 2, H, W), np.float32)
    gt = np.zeros_like(pred)
    pred[:, 0, 4:7, 4:8] = 1
    gt[:, 0, 4:7, 4:8] = 1                                     # the same region: every contour pixel is drawn twice
    pred[:, 1, 0, :] = pred[:, 1, -1, :] = 1                   # a frame on the border
    pred[:, 1, :, 0] = pred[:, 1, :, -1] = 1
    gt[:, 1, :2, :2] = gt[:, 1, -2:, -2:] = gt[:, 1, :2, -2:] = gt[:, 1, -2:, :2] = 1      # the four corners
    want = R.contour_overlay(img, pred, gt)
    got = render.render_contour(dev(img), dev(pred), dev(gt)).cpu().numpy()
    _check_contour(got, img, pred, gt, None, want, f"{H}x{W}")
    ring = R.dilate3(pred[0, 0] > 0) & ~(pred[0, 0] > 0)
    assert ring.sum() > 0 and (got[:, ring] == np.array([255, 0, 0], np.uint8)).all()                       # red over green
    inner = R.dilate3(pred[0, 1] > 0) & ~(pred[0, 1] > 0) & ~(R.dilate3(gt[0, 1] > 0) & ~(gt[0, 1] > 0))
    assert inner.sum() > 0 and (got[:, inner] == np.array([0, 0, 255], np.uint8)).all()                     # part 1 of pred: blue
    drawn = np.zeros((H, W), bool)
    for i in range(2):
        for m in (pred[0, i] > 0, gt[0, i] > 0):
            drawn |= R.dilate3(m) & ~m
    assert (~drawn).sum() > 0 and (got[1][~drawn] == 0).all()                                              # the constant image


def test_labels_form_in_contour_mode_reads_part_i_as_label_i_plus_1():
    from ustrun import render
    g = np.random.default_rng(9)
    img = g.random((1, 3, 9, 10), dtype=np.float32)
    pred = g.integers(0, 5, (1, 9, 10)).astype(np.int64)       # label 4 is beyond the three parts: background
    gt = g.integers(0, 4, (1, 9, 10)).astype(np.int64)
    want = R.contour_overlay(img, pred, gt, 3)
    got = render.render_contour(dev(img), dev(pred), dev(gt), parts=3).cpu().numpy()
    _check_contour(got, img, pred, gt, 3, want, "labels 9x10")


def test_errors_carry_a_message():
    from ustrun import render
    img = torch.zeros(1, 3, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="parts"):
        render.render_mask(img, torch.zeros(1, 6, 8, 8, device="cuda"))
    with pytest.raises(RuntimeError, match="channels"):
        render.render_mask(torch.zeros(1, 2, 8, 8, device="cuda"), torch.zeros(1, 2, 8, 8, device="cuda"))
    with pytest.raises(RuntimeError, match="parts"):
        render.render_contour(img, torch.zeros(1, 5, 8, 8, device="cuda"), torch.zeros(1, 5, 8, 8, device="cuda"))
    with pytest.raises(RuntimeError, match="differ in form"):
        render.render_contour(img, torch.zeros(1, 2, 8, 8, device="cuda"), torch.zeros(1, 8, 8, dtype=torch.int64, device="cuda"))
