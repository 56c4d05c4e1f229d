"""tests/distmap_ref.py, the numpy restatement the GPU tests of ustrun_signed_dist2 / ustrun_sdf_from_dist2 compare against, is
itself pinned: to an O((HW)^2) brute force, to scipy (the library the reference's compute_sdf calls) and to the g20 fixture
(tools/gen_sdf_goldens.py).  Also checked here, without the library: the reference's names and parameters on the Python surface,
and that 3-D volumes are refused before anything touches the device."""
import inspect

import numpy as np
import pytest

import distmap_ref as R


def brute(p):
    """signed squared distances by looking at every pair of pixels"""
    H, W = p.shape
    yy, xx = np.mgrid[:H, :W]
    y, x = yy.ravel(), xx.ravel()
    d2 = (y[:, None] - y[None, :]) ** 2 + (x[:, None] - x[None, :]) ** 2         # [HW,HW]
    f = p.ravel()
    big = 1 << 40
    to_fg = np.where(f[None, :], d2, big).min(axis=1)
    to_bg = np.where(~f[None, :], d2, big).min(axis=1)
    if not f.any():
        return np.full((H, W), R.DIST_NONE, np.int64), R.EMPTY
    if f.all():
        return np.full((H, W), -R.DIST_NONE, np.int64), R.FULL
    return np.where(f, -to_bg, to_fg).reshape(H, W), R.MIXED


def small_planes():
    rng = np.random.default_rng(7)
    out = [np.zeros((1, 1), bool), np.ones((1, 1), bool), np.zeros((4, 6), bool), np.ones((5, 3), bool)]
    for H, W in ((1, 7), (7, 1), (5, 5), (24, 24), (13, 24), (24, 9)):
        out += [R.blobs(rng, H, W), R.blobs(rng, H, W, flip=0.1), rng.random((H, W)) < 0.5]
        one = np.zeros((H, W), bool)
        one[rng.integers(0, H), rng.integers(0, W)] = True
        out += [one, ~one]
    return out


def test_signed_dist2_equals_the_brute_force():
    for p in small_planes():
        s2, flag = R.signed_dist2(p)
        want, wflag = brute(p)
        assert flag == wflag and s2.dtype == np.int32 and np.array_equal(s2, want), p.shape


def test_inner_boundary_is_minus_one():
    for p in small_planes():
        s2, _ = R.signed_dist2(p)
        assert np.array_equal(R.inner_boundary(p), s2 == -1), p.shape


def test_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    cross = ndi.generate_binary_structure(2, 1)
    for H, W in ((33, 47), (64, 130), (9, 200), (120, 3), (40, 40)):
        for p in (R.blobs(rng, H, W), R.blobs(rng, H, W, flip=0.05)):
            assert p.any() and not p.all()
            s2, flag = R.signed_dist2(p)
            inside, outside = ndi.distance_transform_edt(p), ndi.distance_transform_edt(~p)
            assert flag == R.MIXED and np.array_equal(s2, np.rint(outside ** 2 - inside ** 2).astype(np.int64))
            assert np.array_equal(R.inner_boundary(p), p & ~ndi.binary_erosion(p, cross, border_value=1))
            want = outside / outside.max() - inside / inside.max()
            want[R.inner_boundary(p)] = 0
            assert np.array_equal(R.sdf(p), want)            # the same float64 operations on the same integers' roots


def test_against_the_g20_fixture():
    cases = R.load_golden(R.GOLDEN)
    assert len(cases) >= 6 and all(max(m.shape) <= 64 for m, *_ in cases)
    kinds = set()
    for m, to_fg, to_bg, sdf in cases:
        s2, flag = R.signed_dist2(m)
        kinds.add(flag)
        if flag == R.EMPTY:
            assert (to_fg == -1).all() and (s2 == R.DIST_NONE).all() and not sdf.any()
        else:
            assert np.array_equal(s2, to_fg - to_bg)
        assert np.array_equal(R.sdf(m), sdf)
    assert kinds == {R.EMPTY, R.MIXED}                       # (a full mask has no reference result: 0 / 0)


def test_sdf_range_and_degenerate_planes():
    rng = np.random.default_rng(3)
    p = R.blobs(rng, 33, 47)
    s = R.sdf(p)
    assert s.min() == -1.0 and s.max() == 1.0 and (s[p] <= 0).all() and (s[~p] > 0).all()
    assert not R.sdf(np.zeros((4, 5), bool)).any() and not R.sdf(np.ones((4, 5), bool)).any()
    m = np.zeros((2, 6, 7), np.int64)
    m[0, 1:3, 1:4] = 1
    m[1, 2:5, 2:6] = 2
    s2, flags = R.signed_dist2_batch(m, by_class=True, K=2)
    assert s2.shape == (2, 2, 6, 7) and flags.tolist() == [[R.MIXED, R.EMPTY], [R.EMPTY, R.MIXED]]


def test_the_reference_names_and_parameters_exist():
    from utils import metrics, util
    assert list(inspect.signature(util.compute_sdf).parameters) == ["img_gt", "out_shape"]
    assert list(inspect.signature(metrics.distance_transform).parameters) == ["bitmap"]


def test_volumes_are_refused_before_any_device_call():
    from utils import util
    with pytest.raises(NotImplementedError, match="2-D planes"):
        util.compute_sdf(np.zeros((2, 8, 8, 8), np.uint8), (2, 8, 8, 8))
    with pytest.raises(NotImplementedError, match="2-D planes"):
        util.compute_sdf(np.zeros((2, 8, 8), np.uint8), (2, 2, 8, 8))
    with pytest.raises(ValueError, match="out_shape"):
        util.compute_sdf(np.zeros((2, 8, 8), np.uint8), (2, 8, 9))
