"""tests/volume_ref.py, the numpy / scipy restatement the GPU tests of the volume kernels compare against, is itself pinned: to an
O(n^2) brute force in exact integers on volumes of at most 6 x 7 x 9, and, for D = 1, to the 2-D restatements (distmap_ref,
surface_brute).  Also checked here, without the library: utils.metrics.spacing_weights, the names and parameters of the new Python
surface, and that compute_sdf_volume refuses a wrong out_shape before anything touches the device."""
import inspect

import numpy as np
import pytest

import distmap_ref as R2
import surface_brute as B2
import volume_ref as R

WEIGHTS = [(1, 1, 1), (8, 1, 1), (5, 2, 2), (16, 5, 5), (1, 3, 2)]
SHAPES = [(5, 7, 9), (1, 7, 7), (7, 1, 5), (3, 6, 1), (6, 7, 9), (1, 1, 1), (2, 2, 2)]


def pair_d2(shape, weights):
    """[n,n] int64 weighted squared distances between all voxels of the volume (C order)"""
    zz, yy, xx = (a.ravel().astype(np.int64) for a in np.mgrid[:shape[0], :shape[1], :shape[2]])
    wz, wy, wx = weights
    return (wz * (zz[:, None] - zz[None])) ** 2 + (wy * (yy[:, None] - yy[None])) ** 2 + (wx * (xx[:, None] - xx[None])) ** 2


def brute_to(seed, weights):
    """int64 squared distance from every voxel to the nearest True voxel of seed, by looking at every pair; None without one"""
    if not seed.any():
        return None
    d2 = pair_d2(seed.shape, weights)
    return np.where(seed.ravel()[None, :], d2, 1 << 60).min(axis=1).reshape(seed.shape)


def small_volumes():
    rng = np.random.default_rng(7)
    out = []
    for shape in SHAPES:
        assert np.prod(shape) <= 6 * 7 * 9
        out += [np.zeros(shape, bool), np.ones(shape, bool), rng.random(shape) < 0.5, rng.random(shape) < 0.1,
                R.blobs(rng, *shape), R.blobs(rng, *shape, flip=0.1)]
        one = np.zeros(shape, bool)
        one[tuple(rng.integers(0, s) for s in shape)] = True
        out += [one, ~one]
    return out


def test_signed_dist2_equals_the_brute_force_for_every_weight():
    for p in small_volumes():
        for w in WEIGHTS:
            s2, flag = R.signed_dist2(p, w)
            to_fg, to_bg = brute_to(p, w), brute_to(~p, w)
            if to_fg is None:
                assert flag == R.EMPTY and (s2 == R.DIST_NONE).all()
            elif to_bg is None:
                assert flag == R.FULL and (s2 == -R.DIST_NONE).all()
            else:
                assert flag == R.MIXED and s2.dtype == np.int32 and np.array_equal(s2, np.where(p, -to_bg, to_fg)), (p.shape, w)


def test_scipy_stays_next_to_an_integer_at_the_largest_distances():
    """one source voxel in a corner of a 1024-voxel column with weight 40: distances up to 40 * 1023"""
    p = np.zeros((1024, 1, 2), bool)
    p[0, 0, 0] = True
    from scipy import ndimage as ndi
    d = ndi.distance_transform_edt(~p, sampling=(40.0, 1.0, 1.0))
    want = (40 * np.arange(1024)[:, None, None]) ** 2 + np.arange(2)[None, None, :] ** 2
    assert np.abs(d * d - want).max() <= 1e-6
    assert np.array_equal(R.dist2_to(p, (40, 1, 1)), want)


def test_inner_boundary_is_minus_one_with_unit_weights():
    for p in small_volumes():
        s2, _ = R.signed_dist2(p)
        assert np.array_equal(R.inner_boundary(p), s2 == -1), p.shape


def _thin(p):
    """the fixed point of the plane's border operator: a mask that is its own border"""
    while not np.array_equal(B2.border(p), p):
        p = B2.border(p)
    return p


def test_a_single_slice_equals_the_plane():
    rng = np.random.default_rng(3)
    for H, W in ((7, 9), (13, 24), (1, 7)):
        for p in (R2.blobs(rng, H, W), rng.random((H, W)) < 0.4, np.zeros((H, W), bool), np.ones((H, W), bool)):
            s2, flag = R.signed_dist2(p[None])
            w2, wflag = R2.signed_dist2(p)
            assert flag == wflag and np.array_equal(s2[0], w2)
            assert np.array_equal(R.sdf_batch(p[None, None].astype(np.float32))[0][0, 0, 0], R2.sdf(p))
            # outside the volume is background, so every voxel of a single slice is a border voxel: the plane's record is that
            # of masks that are their own 4-neighbour border
            q, g = _thin(p), _thin(R2.blobs(rng, H, W))
            assert np.array_equal(R.border(q[None])[0], q) and np.array_equal(B2.border(q), q)
            rec3, rec2 = R.record(q[None], g[None]), B2.record(q, g)
            assert np.array_equal(rec3[:4], rec2[:4]) and np.array_equal(rec3[6:8], rec2[4:6])


def test_borders_and_records_equal_the_brute_force():
    from scipy import ndimage as ndi
    rng = np.random.default_rng(11)
    cross = ndi.generate_binary_structure(3, 1)
    for shape in SHAPES:
        for w in WEIGHTS:
            p, g = R.blobs(rng, *shape, flip=0.05), R.blobs(rng, *shape, flip=0.05)
            assert np.array_equal(R.border(p), p & ~ndi.binary_erosion(p, cross))
            rec = R.record(p, g, w)
            bp, bg = R.border(p), R.border(g)
            assert rec[0] == bp.sum() and rec[1] == bg.sum()
            if not rec[0] or not rec[1]:
                assert not rec[2:].any()
                continue
            dp, dg = brute_to(bg, w)[bp], brute_to(bp, w)[bg]
            u = np.sort(np.concatenate([dp, dg]))
            k = int(np.floor(0.95 * (len(u) - 1)))
            assert rec[2:6].tolist() == [u[k], u[min(k + 1, len(u) - 1)], dp.max(), dg.max()]
            assert np.array_equal(R.record_sums(rec), [np.sqrt(dp.astype(np.float64)).sum(), np.sqrt(dg.astype(np.float64)).sum()])


def test_metrics_from_records_against_the_medpy_restatement():
    rng = np.random.default_rng(5)
    p, g = R.ball((6, 7, 9), (3, 3, 4), 2.5), R.ball((6, 7, 9), (2, 4, 5), 2.5)
    for spacing, w, unit in ((None, (1, 1, 1), 1.0), ((10, 1.25, 1.25), (8, 1, 1), 1.25), ((2.5, 1, 1), (5, 2, 2), 0.5)):
        rec, cnt = R.records(p[None].astype(np.float32), g[None].astype(np.float32), weights=w)
        got, want = R.metrics_from_record(rec[0, 0], cnt[0, 0], unit), R.medpy_metrics(p, g, spacing)
        assert sorted(got) == sorted(want) == ["asd", "assd", "dc", "hd", "hd95", "jc"]
        for name in want:
            assert np.isclose(got[name], want[name], rtol=1e-12, atol=0), (name, got[name], want[name])
    empty = np.zeros_like(p)
    rec, cnt = R.records(empty[None].astype(np.float32), g[None].astype(np.float32))
    assert R.metrics_from_record(rec[0, 0], cnt[0, 0]) == R.medpy_metrics(empty, g) and R.medpy_metrics(empty, g)["hd95"] == 100.0
    with pytest.raises(RuntimeError):
        R.medpy_metrics(p, empty)


def test_spacing_weights_table_and_refusals():
    from utils.metrics import spacing_weights
    for spacing, weights, unit in (((10, 1.25, 1.25), (8, 1, 1), 1.25), ((2.5, 1, 1), (5, 2, 2), 0.5),
                                   ((3.0, 0.9375, 0.9375), (16, 5, 5), 0.1875), ((3.6, 0.625, 0.625), (144, 25, 25), 0.025),
                                   ((1, 1, 1), (1, 1, 1), 1.0), ((0.5, 0.5, 0.5), (1, 1, 1), 0.5)):
        w, u = spacing_weights(spacing)
        assert w == weights and all(isinstance(v, int) for v in w) and np.isclose(u, unit, rtol=1e-15), (spacing, w, u)
        assert np.allclose(np.array(w) * u, spacing, rtol=1e-6)
    with pytest.raises(ValueError, match="no scale"):
        spacing_weights((np.pi, 1.0, 1.0))
    with pytest.raises(ValueError, match="255"):
        spacing_weights((300.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="no scale"):
        spacing_weights((2.5, 1, 1), max_scale=1)


def test_the_new_names_and_parameters_exist():
    from ustrun import functional as F
    from utils import metrics, util
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert sig(F.signed_dist2_3d) == [("mask", E), ("by_class", False), ("num_classes", None), ("weights", (1, 1, 1))]
    assert sig(F.signed_distance_map_3d) == [("mask", E), ("by_class", False), ("num_classes", None)]
    assert sig(F.surface_metrics_3d) == [("pred", E), ("gt", E), ("by_class", False), ("n_classes", 1), ("weights", (1, 1, 1))]
    assert sig(util.compute_sdf_volume) == [("img_gt", E), ("out_shape", E)]
    assert sig(metrics.spacing_weights) == [("voxelspacing", E), ("max_scale", 64), ("rtol", 1e-6)]
    assert sig(metrics.volume_metrics) == [("pred", E), ("gt", E), ("voxelspacing", None), ("by_class", False), ("n_classes", 1)]
    for f in (F.signed_dist2_3d, F.signed_distance_map_3d, F.surface_metrics_3d, util.compute_sdf_volume, metrics.volume_metrics):
        assert ".py:" in f.__doc__                                 # each cites the reference's lines


def test_compute_sdf_volume_refuses_a_wrong_out_shape_before_any_device_call():
    from utils import util
    for in_shape, out_shape in (((2, 4, 8, 8), (2, 4, 8, 9)), ((2, 4, 8, 8), (2, 2, 4, 8, 8)), ((2, 8, 8), (2, 8, 8)),
                                ((2, 4, 8, 8), (2, 4, 64))):
        with pytest.raises(ValueError, match="compute_sdf_volume.*out_shape"):
            util.compute_sdf_volume(np.zeros(in_shape, np.uint8), out_shape)


def test_case_groups_and_the_driver_flags():
    from ustrun.evaluate import case_groups
    names = ["p01_s00.png", "p02_s00.png", "p01_s01.png", "p02_s01.png", "p01_s02.png"]
    assert case_groups(names, r"(p\d+)_") == [("p01", [0, 2, 4]), ("p02", [1, 3])]          # listing order, cases and slices
    with pytest.raises(ValueError, match="does not match"):
        case_groups(names + ["readme.txt"], r"(p\d+)_")
    with pytest.raises(ValueError, match="one group"):
        case_groups(names, r"p\d+_")
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ust-run_amd", "test.py")
    spec = importlib.util.spec_from_file_location("ust_test_driver", path)
    driver = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(driver)
    off = driver.parser.parse_args([])
    assert (off.volume_metrics, off.case_pattern, off.voxelspacing) == (0, "", "")             # everything is off by default
    on = driver.parser.parse_args(["--volume_metrics", "1", "--case_pattern", r"(p\d+)_", "--voxelspacing", "10,1.25,1.25"])
    assert on.volume_metrics == 1 and on.case_pattern == r"(p\d+)_" and on.voxelspacing == "10,1.25,1.25"
