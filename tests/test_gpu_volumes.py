"""The volume kernels (csrc/edt3d.hip: ustrun_signed_dist2_3d, ustrun_sdf_from_dist2_3d, ustrun_surface_metrics_3d) and the Python
surface on top of them (ustrun.functional.*_3d, utils.util.compute_sdf_volume, utils.metrics.volume_metrics) against
tests/volume_ref.py, which tests/test_volume_ref_host.py pins to a brute force.

Squared distances, counts, order statistics and maxima are integers: every comparison of them is bit equality.
The normalised map holds the bar of tests/test_gpu_distmap.py, 2^-24 absolute: one quotient of at most 1 formed in float64 and
rounded to float32 once (2^-25) next to the float64 restatement's own few 2^-53.
The two f64 sums of sqrt(d2): every term is non-negative and correctly rounded in both (IEEE sqrt), so any summation order of n
terms stays within n * 2^-52 relative of any other (each of at most n - 1 additions errs by at most 2^-53 of a partial sum that
is at most the total, on either side)."""
import functools

import numpy as np
import pytest
import torch

import distmap_ref as R2
import volume_ref as R

pytestmark = pytest.mark.gpu

SDF_TOL = 2.0 ** -24


def _one(shape, at):
    p = np.zeros(shape, bool)
    p[at] = True
    return p


def _dev(p):
    return torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).cuda()


@functools.lru_cache(maxsize=None)
def dist_cases():
    """name -> (volumes bool [N,K,D,H,W], weights): the inputs of the signed-distance cases"""
    rng = np.random.default_rng(2028)
    one_slice = np.zeros((9, 12, 20), bool)
    one_slice[6] = R2.blobs(rng, 12, 20)
    c = {
        "1x1x1_foreground": (np.ones((1, 1, 1), bool), (1, 1, 1)),
        "1x1x1_background": (np.zeros((1, 1, 1), bool), (1, 1, 1)),
        "1x7x9_plane": (R2.blobs(rng, 7, 9)[None], (1, 1, 1)),
        "5x1x1": (np.array([0, 1, 1, 0, 0], bool).reshape(5, 1, 1), (1, 1, 1)),
        "3x5x1": (rng.random((3, 5, 1)) < 0.4, (1, 1, 1)),
        "6x10x13_blobs": (R.blobs(rng, 6, 10, 13), (1, 1, 1)),
        "9x33x70_blobs": (R.blobs(rng, 9, 33, 70), (1, 1, 1)),                 # W > 64, H no multiple of 4
        "70x9x5_blobs": (R.blobs(rng, 70, 9, 5), (1, 1, 1)),                   # D > 64
        "17x40x67_w811": (R.blobs(rng, 17, 40, 67), (8, 1, 1)),
        "17x40x67_w522": (R.blobs(rng, 17, 40, 67, flip=0.01), (5, 2, 2)),
        "17x40x67_w132": (R.blobs(rng, 17, 40, 67), (1, 3, 2)),
        "40x64x64_corner_voxel": (_one((40, 64, 64), (39, 63, 63)), (1, 1, 1)),   # the longest z search: 39 slices from the far corner
        "9x12x20_one_slice_of_sources": (one_slice, (1, 1, 1)),                # all other slices carry the sentinel
        "9x12x20_all_but_one_slice": (~one_slice, (2, 1, 1)),
        "4x5x6_empty": (np.zeros((4, 5, 6), bool), (1, 1, 1)),
        "4x5x6_full": (np.ones((4, 5, 6), bool), (3, 1, 2)),
    }
    return {k: (v[None, None], w) for k, (v, w) in c.items()}


DIST_NAMES = ["1x1x1_foreground", "1x1x1_background", "1x7x9_plane", "5x1x1", "3x5x1", "6x10x13_blobs", "9x33x70_blobs",
              "70x9x5_blobs", "17x40x67_w811", "17x40x67_w522", "17x40x67_w132", "40x64x64_corner_voxel",
              "9x12x20_one_slice_of_sources", "9x12x20_all_but_one_slice", "4x5x6_empty", "4x5x6_full"]


@functools.lru_cache(maxsize=None)
def dist_want(name):
    p, w = dist_cases()[name]
    return R.signed_dist2_batch(p.astype(np.float32), weights=w)


def _report(name, got, want):
    bad = int((got != want).sum())
    print(name, tuple(want.shape), "differing voxels", bad, "of", want.size)
    return bad


@pytest.mark.parametrize("name", DIST_NAMES)
def test_signed_dist2_3d_is_bit_equal(name):
    from ustrun import functional as F
    p, w = dist_cases()[name]
    s2, flags = dist_want(name)
    got, gflags = F.signed_dist2_3d(_dev(p), weights=w)
    assert got.dtype == torch.int32 and gflags.dtype == torch.int32 and got.is_cuda and gflags.is_cuda
    assert got.shape == p.shape and gflags.shape == p.shape[:2]
    assert np.array_equal(gflags.cpu().numpy(), flags), (gflags.cpu().numpy(), flags)
    assert _report(name, got.cpu().numpy(), s2) == 0


def test_fixed_values_flags_and_the_plane_twin():
    from ustrun import functional as F
    s2, flags = F.signed_dist2_3d(_dev(dist_cases()["1x1x1_foreground"][0]))
    assert flags.item() == F.PLANE_FULL and s2.item() == -F.DIST_NONE
    s2, flags = F.signed_dist2_3d(_dev(dist_cases()["1x1x1_background"][0]))
    assert flags.item() == F.PLANE_EMPTY and s2.item() == F.DIST_NONE
    s2, flags = F.signed_dist2_3d(_dev(dist_cases()["4x5x6_full"][0]), weights=(3, 1, 2))
    assert flags.item() == F.PLANE_FULL and (s2 == -F.DIST_NONE).all()
    s2, flags = F.signed_dist2_3d(_dev(dist_cases()["40x64x64_corner_voxel"][0]))
    assert flags.item() == F.PLANE_MIXED and s2[0, 0, 0, 0, 0].item() == 39 * 39 + 2 * 63 * 63 and s2[0, 0, 39, 63, 63].item() == -1
    s2, _ = F.signed_dist2_3d(_dev(dist_cases()["5x1x1"][0]), weights=(3, 1, 1))
    assert s2.flatten().tolist() == [9, -9, -9, 9, 36]
    p = dist_cases()["1x7x9_plane"][0]
    s3, f3 = F.signed_dist2_3d(_dev(p))
    s2, f2 = F.signed_dist2(_dev(p[:, :, 0]))                                   # a single slice is the plane
    assert torch.equal(s3[:, :, 0], s2) and torch.equal(f3, f2)


@functools.lru_cache(maxsize=None)
def batch_case():
    rng = np.random.default_rng(6)
    m = np.zeros((2, 7, 11, 13), np.int64)
    for c in (1, 2, 3, 4):                               # 4 is a value above K: it belongs to no volume
        m[0][R.blobs(rng, 7, 11, 13, n=1)] = c
    m[1][R.blobs(rng, 7, 11, 13, n=2)] = 2               # sample 1: classes 1 and 3 are empty
    return m, R.signed_dist2_batch(m, by_class=True, K=3, weights=(2, 1, 1))


@pytest.mark.parametrize("dtype", [torch.int64, torch.float32])
def test_batched_class_maps_from_an_offset_view(dtype):
    from ustrun import functional as F
    m, (want, wflags) = batch_case()
    buf = torch.zeros(m.size + 1, dtype=dtype, device="cuda")
    buf[0] = 1
    buf[1:] = torch.from_numpy(m).to(dtype).cuda().flatten()
    view = buf[1:].view(m.shape)
    assert view.data_ptr() == buf.data_ptr() + buf.element_size() and view.is_contiguous()
    got, gflags = F.signed_dist2_3d(view, by_class=True, num_classes=3, weights=(2, 1, 1))
    assert got.shape == (2, 3, 7, 11, 13) and (wflags[1] == [R.EMPTY, R.MIXED, R.EMPTY]).all() and (wflags[0] == R.MIXED).all()
    assert np.array_equal(gflags.cpu().numpy(), wflags) and _report("by_class", got.cpu().numpy(), want) == 0
    if dtype == torch.float32:                           # the same volumes as float32 planes [N,K,D,H,W], from an offset view too
        vol = R.volumes(m, True, 3).astype(np.float32)
        buf = torch.zeros(vol.size + 1, device="cuda")
        buf[1:] = torch.from_numpy(vol).cuda().flatten()
        got, gflags = F.signed_dist2_3d(buf[1:].view(vol.shape), weights=(2, 1, 1))
        assert np.array_equal(gflags.cpu().numpy(), wflags) and np.array_equal(got.cpu().numpy(), want)


def test_more_maps_than_a_grid_extent_holds():
    """[33, 1, 1000, 2, 2]: 66 000 slice maps, past 65 535"""
    from ustrun import functional as F
    rng = np.random.default_rng(9)
    p = rng.random((33, 1, 1000, 2, 2)) < 0.01
    p[5] = False
    p[6] = True
    want, wflags = R.signed_dist2_batch(p.astype(np.float32), weights=(1, 2, 3))
    got, gflags = F.signed_dist2_3d(_dev(p), weights=(1, 2, 3))
    assert wflags[5, 0] == R.EMPTY and wflags[6, 0] == R.FULL and (wflags == R.MIXED).sum() == 31
    assert np.array_equal(gflags.cpu().numpy(), wflags) and _report("66000 maps", got.cpu().numpy(), want) == 0


def test_two_calls_give_identical_bits():
    from ustrun import functional as F
    x = _dev(dist_cases()["17x40x67_w522"][0])
    a, fa = F.signed_dist2_3d(x, weights=(5, 2, 2))
    b, fb = F.signed_dist2_3d(x, weights=(5, 2, 2))
    sa, _ = F.signed_distance_map_3d(x)
    sb, _ = F.signed_distance_map_3d(x)
    assert torch.equal(a, b) and torch.equal(fa, fb) and torch.equal(sa, sb)


# ---- the normalised map ----
SDF_NAMES = ["1x1x1_foreground", "1x7x9_plane", "3x5x1", "6x10x13_blobs", "9x33x70_blobs", "70x9x5_blobs",
             "9x12x20_one_slice_of_sources", "4x5x6_empty", "4x5x6_full"]


@pytest.mark.parametrize("name", SDF_NAMES)
def test_signed_distance_map_3d_against_float64(name):
    from ustrun import functional as F
    p = dist_cases()[name][0]
    s2, flags = R.signed_dist2_batch(p.astype(np.float32))
    sdf, _ = R.sdf_batch(p.astype(np.float32))
    got, gflags = F.signed_distance_map_3d(_dev(p))
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == p.shape and not got.requires_grad
    got = got.cpu().numpy()
    assert np.array_equal(gflags.cpu().numpy(), flags)
    err = float(np.abs(got.astype(np.float64) - sdf).max())
    print(name, "max |sdf - float64|", err, "bound", SDF_TOL)
    assert err <= SDF_TOL
    assert np.array_equal(got, sdf.astype(np.float32))                       # the float64 value rounded once
    assert (got[s2 == -1] == 0).all() and np.array_equal(s2 == -1, R.inner_boundary(p[0, 0])[None, None])
    if flags[0, 0] == R.MIXED:                                               # the deepest voxels, exactly
        assert got.max() == 1.0 and np.array_equal(got == 1.0, s2 == s2.max())
        assert got.min() == -1.0 or (s2[p] == -1).all()
        if s2.min() < -1:
            assert np.array_equal(got == -1.0, s2 == s2.min())
        assert (got[p] <= 0).all() and (got[~p] > 0).all()
    else:
        assert not got.any()


def test_the_maxima_are_taken_over_the_whole_volume():
    from ustrun import functional as F
    p = np.zeros((1, 1, 6, 9, 9), bool)
    p[0, 0, 1:5, 2:7, 2:7] = True                        # slices differ in depth: per-slice maxima would give other values
    got, _ = F.signed_distance_map_3d(_dev(p))
    want, _ = R.sdf_batch(p.astype(np.float32))
    assert np.array_equal(got.cpu().numpy(), want.astype(np.float32)) and (got[0, 0, 2].min() == -1.0) and got[0, 0, 1].min() > -1.0


def test_compute_sdf_volume_wrapper():
    from utils.util import compute_sdf_volume
    rng = np.random.default_rng(4)
    gt = np.stack([R.blobs(rng, 5, 9, 11), np.zeros((5, 9, 11), bool), R.blobs(rng, 5, 9, 11, flip=0.02)])
    want, flags = R.sdf_batch(gt.astype(np.float32))
    assert flags[:, 0].tolist() == [R.MIXED, R.EMPTY, R.MIXED]
    for shape in ((3, 5, 9, 11), (3, 1, 5, 9, 11)):
        out = compute_sdf_volume((gt * 7).astype(np.int16), shape)
        assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == shape
        assert np.array_equal(out.reshape(3, 5, 9, 11), want[:, 0])          # float64 of the exact integers: the restatement's values
        dev = compute_sdf_volume(torch.from_numpy(gt).cuda(), shape)
        assert torch.is_tensor(dev) and dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == shape
        assert float(np.abs(dev.cpu().numpy().reshape(3, 5, 9, 11) - want[:, 0]).max()) <= SDF_TOL
    assert not out.reshape(3, 5, 9, 11)[1].any()
    full = gt.copy()
    full[1] = True
    with pytest.raises(ValueError, match="sample 1"):
        compute_sdf_volume(full, (3, 5, 9, 11))
    assert not compute_sdf_volume(torch.from_numpy(full[1:2]).cuda(), (1, 5, 9, 11)).any()       # tensor route: zeros, no exception


# ---- surface records ----
@functools.lru_cache(maxsize=None)
def surf_cases():
    """name -> (pred bool [N,K,D,H,W], gt, weights)"""
    rng = np.random.default_rng(31)
    ball = R.ball((20, 24, 70), (10, 12, 30), 8)
    low, high = np.zeros((40, 12, 12), bool), np.zeros((40, 12, 12), bool)
    rng40 = np.random.default_rng(40)
    low[0], high[38], high[39] = R2.blobs(rng40, 12, 12), R2.blobs(rng40, 12, 12), R2.blobs(rng40, 12, 12)
    far = np.zeros((129, 4, 5), bool)
    far[128, 3, 4] = True
    c = {
        "ball_against_shifted_ball": (ball, R.ball((20, 24, 70), (11, 10, 35), 7), (1, 1, 1)),
        "ball_weights_522": (ball, R.ball((20, 24, 70), (11, 10, 35), 7), (5, 2, 2)),
        "single_voxels": (_one((5, 6, 7), (0, 0, 0)), _one((5, 6, 7), (4, 5, 6)), (2, 1, 3)),
        "identical_masks": (ball, ball, (1, 1, 1)),
        "noisy_blobs": (R.blobs(rng, 9, 33, 70, flip=0.02), R.blobs(rng, 9, 33, 70, flip=0.02), (3, 1, 1)),
        "empty_prediction": (np.zeros_like(ball), ball, (1, 1, 1)),
        "empty_ground_truth": (ball, np.zeros_like(ball), (1, 1, 1)),
        "both_empty": (np.zeros((3, 4, 5), bool), np.zeros((3, 4, 5), bool), (1, 1, 1)),
        "weights_40_at_D40": (low, high, (40, 1, 1)),                            # every d2 >= 38^2 40^2 > 2^21
        # the largest weight at D = 129: d2 up to 255^2 128^2 + 25 = 1 065 369 625, 0.8 % short of 2^30 (no volume of this depth
        # and weight reaches 2^30: 2 x 1023^2 more is the most the plane adds); one slice more passes it
        "weights_255_at_D129": (_one((129, 4, 5), (0, 0, 0)) | _one((129, 4, 5), (3, 1, 1)), far, (255, 1, 1)),
        "weights_255_at_D130": (_one((130, 4, 5), (0, 0, 0)) | _one((130, 4, 5), (3, 1, 1)), _one((130, 4, 5), (129, 3, 4)), (255, 1, 1)),
    }
    return {k: (p[None, None], g[None, None], w) for k, (p, g, w) in c.items()}


SURF_NAMES = ["ball_against_shifted_ball", "ball_weights_522", "single_voxels", "identical_masks", "noisy_blobs", "empty_prediction",
              "empty_ground_truth", "both_empty", "weights_40_at_D40", "weights_255_at_D129", "weights_255_at_D130"]


def _check_records(name, got, want):
    assert got.shape == want.shape and got.dtype == np.int32
    print(name, "integers", got[..., :6].tolist(), "want", want[..., :6].tolist())
    assert np.array_equal(got[..., :6], want[..., :6])
    gs, ws = R.record_sums(got), R.record_sums(want)
    n = want[..., :2].astype(np.float64)
    print(name, "sums", gs.tolist(), "want", ws.tolist(), "terms", n.tolist())
    assert (np.abs(gs - ws) <= n * 2.0 ** -52 * ws).all()


@pytest.mark.parametrize("name", SURF_NAMES)
def test_surface_metrics_3d_records(name):
    from ustrun import functional as F
    p, g, w = surf_cases()[name]
    want, _ = R.records(p.astype(np.float32), g.astype(np.float32), weights=w)
    rec = F.surface_metrics_3d(_dev(p), _dev(g), weights=w)
    assert rec.dtype == torch.int32 and rec.is_cuda and tuple(rec.shape) == (1, 1, 10)
    _check_records(name, rec.cpu().numpy(), want)
    again = F.surface_metrics_3d(_dev(p), _dev(g), weights=w)
    assert torch.equal(rec, again)                                           # a repeated call, bit-identical


def test_surface_records_fixed_values():
    from ustrun import functional as F
    p, g, w = surf_cases()["weights_40_at_D40"]
    rec = F.surface_metrics_3d(_dev(p), _dev(g), weights=w).cpu().numpy()[0, 0]
    assert rec[0] > 8 and rec[1] > 8 and rec[2] > 1 << 21 and rec[2] <= rec[3] <= max(rec[4], rec[5])
    p, g, w = surf_cases()["weights_255_at_D129"]
    rec = F.surface_metrics_3d(_dev(p), _dev(g), weights=w).cpu().numpy()[0, 0]
    d_far, d_near = 255 * 255 * 128 * 128 + 9 + 16, 255 * 255 * 125 * 125 + 4 + 9
    assert d_far > 0.99 * 2 ** 30 and rec[:6].tolist() == [2, 1, d_near, d_far, d_far, d_near]
    assert R.record_sums(rec).tolist() == [np.sqrt(np.float64(d_far)) + np.sqrt(np.float64(d_near)), np.sqrt(np.float64(d_near))]
    p, g, w = surf_cases()["weights_255_at_D130"]
    rec = F.surface_metrics_3d(_dev(p), _dev(g), weights=w).cpu().numpy()[0, 0]
    d_far, d_near = 255 * 255 * 129 * 129 + 9 + 16, 255 * 255 * 126 * 126 + 4 + 9
    assert d_far > 1 << 30 and rec[:6].tolist() == [2, 1, d_near, d_far, d_far, d_near]             # a value past 2^30
    p, g, w = surf_cases()["identical_masks"]
    rec = F.surface_metrics_3d(_dev(p), _dev(g)).cpu().numpy()[0, 0]
    assert rec[0] == rec[1] > 0 and not rec[2:].any()
    rec = F.surface_metrics_3d(_dev(surf_cases()["empty_ground_truth"][0]), _dev(surf_cases()["empty_ground_truth"][1])).cpu().numpy()
    assert rec[0, 0, 0] > 0 and not rec[0, 0, 1:].any()


def test_surface_metrics_3d_batched_class_maps():
    from ustrun import functional as F
    m, _ = batch_case()
    rng = np.random.default_rng(8)
    g = m.copy()
    g[0][R.blobs(rng, 7, 11, 13, n=1)] = 1
    g[1] = np.roll(m[1], 2, axis=2)
    want, _ = R.records(m, g, by_class=True, n_classes=3, weights=(2, 1, 1))
    got = F.surface_metrics_3d(torch.from_numpy(m).cuda(), torch.from_numpy(g).float().cuda(), by_class=True, n_classes=3,
                               weights=(2, 1, 1))
    _check_records("by_class", got.cpu().numpy(), want)


def test_volume_metrics_with_voxelspacing():
    from utils import metrics
    p, g, _ = surf_cases()["ball_against_shifted_ball"]
    pred = np.concatenate([p, np.zeros_like(p)])                             # case 1: an empty prediction
    gt = np.concatenate([g, g])
    for spacing in ((10, 1.25, 1.25), None, (2.5, 1, 1)):
        got = metrics.volume_metrics(_dev(pred), _dev(gt), voxelspacing=spacing)
        assert sorted(got) == ["asd", "assd", "dc", "hd", "hd95", "jc"]
        for n in range(2):
            want = R.medpy_metrics(pred[n, 0], gt[n, 0], spacing)
            for name, v in want.items():
                assert got[name].dtype == np.float64 and got[name].shape == (2, 1)
                print(spacing, n, name, got[name][n, 0], v)
                assert np.isclose(got[name][n, 0], v, rtol=1e-12, atol=0), (spacing, n, name)
        assert got["hd95"][1, 0] == 100.0 and got["assd"][1, 0] == 100.0
        if spacing is None:                                                  # float32 volumes without the part axis: [N,D,H,W]
            flat = metrics.volume_metrics(_dev(pred[:, 0]), _dev(gt[:, 0]))
            assert all(np.array_equal(flat[name], got[name]) for name in got)
    with pytest.raises(metrics.EmptyGroundTruth) as e:
        metrics.volume_metrics(_dev(gt), _dev(pred))
    assert e.value.sample == 1 and e.value.part == 0
    m, _ = batch_case()
    cls = metrics.volume_metrics(torch.from_numpy(m[:1]).cuda(), torch.from_numpy(np.roll(m[:1], 1, axis=3)).cuda(), by_class=True,
                                 n_classes=3, voxelspacing=(2.5, 1, 1))
    for k in range(3):
        want = R.medpy_metrics(m[0] == k + 1, np.roll(m[0], 1, axis=2) == k + 1, (2.5, 1, 1))
        for name, v in want.items():
            assert np.isclose(cls[name][0, k], v, rtol=1e-12, atol=0), (k, name)


class _Pool:
    """what validate_volumes reads of a ustrun.datasets.ResidentDataset: images / labels uint8 [n,H,W,C] on the device, names"""

    def __init__(self, images, labels, names):
        self.images, self.labels, self.names = torch.from_numpy(images).cuda(), torch.from_numpy(labels).cuda(), names


class _ByIntensity(torch.nn.Module):
    """a stand-in network whose class follows the image's intensity (per image, so coalescing cannot matter): logit c is highest
    where the intensity, scaled to the image's own range, is nearest to c / (k - 1).  What is under test is the grouping, the stacking and the metrics"""

    def __init__(self, k):
        super().__init__()
        self.k, self.dummy = k, torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        lo, hi = x.amin(dim=(1, 2, 3), keepdim=True), x.amax(dim=(1, 2, 3), keepdim=True)
        levels = torch.linspace(0.0, 1.0, self.k, device=x.device).view(1, self.k, 1, 1)
        return -((x - lo) / (hi - lo) - levels) ** 2


@pytest.mark.parametrize("dataset,k,spacing", [("prostate", 2, (2.5, 1, 1)), ("MNMS", 4, None)])
def test_validate_volumes_groups_slices_into_cases(dataset, k, spacing):
    from ustrun import datasets
    from ustrun.evaluate import PARTS, case_groups, predict, validate_volumes
    from ustrun.trainer import decode_labels
    rng = np.random.default_rng(12)
    names = ["caseA_s0.png", "caseB_s0.png", "caseA_s1.png", "caseB_s1.png", "caseB_s2.png", "caseA_s2.png", "caseA_s3.png"]
    n, H, parts = len(names), 48, len(PARTS[dataset])
    truth = np.zeros((n, H, H), np.int64)                                   # nested discs per slice: classes 1..parts
    yy, xx = np.mgrid[:H, :H]
    for i in range(n):
        cy, cx, r = rng.integers(18, 30), rng.integers(18, 30), rng.integers(10, 16)
        for c in range(parts):
            truth[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= (r * (1 - c / (parts + 0.5))) ** 2] = c + 1
    seen = np.roll(truth, (2, -3), axis=(1, 2))                              # the image shows the structure moved: the prediction errs
    images = (seen * (200 // parts) + 20 + rng.integers(0, 12, seen.shape)).astype(np.uint8)[..., None]
    if dataset == "prostate":
        labels = np.where(truth == 1, 0, 255).astype(np.uint8)[..., None]    # foreground is 0 (train.py:590-608)
    else:
        labels = np.stack([np.where(truth == c + 1, 255, 0) for c in range(3)], axis=-1).astype(np.uint8)
    model = _ByIntensity(k).cuda()
    pool = _Pool(images, labels, names)
    lines = []
    got = validate_volumes(dataset, model, [pool], r"(case[A-Z])_", voxelspacing=spacing, log=lines.append, coalesce=3)
    assert model.training and len(got) == 1 and sorted(got[0]) == ["asd", "assd", "dc", "hd95", "jc"]
    assert len(lines) == 1 and all(f"vol_{p}_{m}: " in lines[0] for p in PARTS[dataset] for m in ("dc", "jc", "hd95", "asd", "assd"))
    model.eval()
    with torch.no_grad():
        x, _, y = datasets.stage_finish(pool.images, None, pool.labels)
        pred, mask = predict(dataset, model(x)).cpu().numpy(), decode_labels(dataset, y).cpu().numpy()
    assert np.array_equal(mask, truth)
    want = {m: np.zeros(parts) for m in got[0]}
    groups = case_groups(names, r"(case[A-Z])_")
    assert groups == [("caseA", [0, 2, 5, 6]), ("caseB", [1, 3, 4])]
    for _, idx in groups:
        for c in range(parts):
            p, g = pred[idx] == c + 1, mask[idx] == c + 1
            assert 0 < (p & g).sum() < min(p.sum(), g.sum())                 # a prediction that overlaps and errs
            one = R.medpy_metrics(p, g, spacing)
            for m in want:
                want[m][c] += one[m] / len(groups)
    for m in want:
        print(dataset, m, got[0][m], want[m].tolist())
        assert np.allclose(got[0][m], want[m], rtol=1e-12, atol=0), m


# ---- refusals: the message names the entry and the values, and nothing is launched (the outputs keep their fill) ----
def _raw():
    from ustrun import _lib as L
    lib = L.lib()
    dev = "cuda"
    t = dict(mask=torch.ones(4096, device=dev), work=torch.zeros(1 << 20, dtype=torch.uint8, device=dev),
             s2=torch.full((4096,), 77, dtype=torch.int32, device=dev), flags=torch.full((8,), 77, dtype=torch.int32, device=dev),
             sdf=torch.full((4096,), 77.0, device=dev), out=torch.full((16,), 77, dtype=torch.int32, device=dev))
    return lib, t


def _err(lib):
    return lib.ustrun_last_error().decode()


def _untouched(t):
    torch.cuda.synchronize()
    return bool((t["s2"] == 77).all() and (t["flags"] == 77).all() and (t["sdf"] == 77.0).all() and (t["out"] == 77).all())


ENTRIES = ("signed_dist2_3d", "sdf_from_dist2_3d", "surface_metrics_3d")


def _calls(lib, t, D, H, W, wz=1, wy=1, wx=1, N=1, K=1, work_bytes=1 << 20, which=ENTRIES, **ptr):
    """the entries named in `which` with one set of sizes -> {name: rc}; only a call that must be refused is made with sizes its
    buffers do not hold"""
    a = {k: v.data_ptr() for k, v in t.items()}
    a.update(ptr)
    rc = {}
    if "signed_dist2_3d" in which:
        rc["signed_dist2_3d"] = lib.ustrun_signed_dist2_3d(a["mask"], 0, N, K, 0, D, H, W, wz, wy, wx, a["work"], work_bytes, a["s2"],
                                                           a["flags"], None)
    if "sdf_from_dist2_3d" in which:
        rc["sdf_from_dist2_3d"] = lib.ustrun_sdf_from_dist2_3d(a["s2"], a["flags"], N, K, D, H, W, a["work"], work_bytes, a["sdf"], None)
    if "surface_metrics_3d" in which:
        rc["surface_metrics_3d"] = lib.ustrun_surface_metrics_3d(a["mask"], a["mask"], 0, 0, N, K, 0, D, H, W, wz, wy, wx, a["work"],
                                                                 work_bytes, a["out"], None)
    return rc


WEIGHTED = ("signed_dist2_3d", "surface_metrics_3d")          # (the normalisation takes no weights)


@pytest.mark.parametrize("D,H,W", [(0, 8, 8), (8, 0, 8), (8, 8, 0), (1025, 8, 8), (8, 1025, 8), (8, 8, 1025)])
def test_sizes_out_of_range_are_refused(D, H, W):
    from ustrun import functional as F
    lib, t = _raw()
    for name in ("signed_dist2_3d", "sdf_from_dist2_3d", "surface_metrics_3d"):
        assert getattr(lib, f"ustrun_{name}_work_bytes")(1, 1, D, H, W) == -1
        assert _err(lib).startswith(f"{name}_work_bytes:") and "1024" in _err(lib) and f"D {D} H {H} W {W}" in _err(lib)
    for name in ENTRIES:
        assert _calls(lib, t, D, H, W, which=(name,))[name] != 0
        assert _err(lib).startswith(name + ":") and "1024" in _err(lib) and f"D {D} H {H} W {W}" in _err(lib)
    assert _untouched(t)
    if D and H and W:
        with pytest.raises(RuntimeError, match="ustrun_signed_dist2_3d_work_bytes.*1024"):
            F.signed_dist2_3d(torch.zeros(1, 1, D, H, W, device="cuda"))
        with pytest.raises(RuntimeError, match="ustrun_surface_metrics_3d_work_bytes.*1024"):
            F.surface_metrics_3d(torch.zeros(1, 1, D, H, W, device="cuda"), torch.zeros(1, 1, D, H, W, device="cuda"))


def test_too_many_voxels_and_too_many_volumes_are_refused():
    lib, t = _raw()
    for name in ENTRIES:                                                     # 2^27 + 2^20 voxels, over dummy buffers
        assert _calls(lib, t, 1024, 1024, 129, which=(name,))[name] != 0
        assert _err(lib).startswith(name + ":") and "2^27" in _err(lib) and "D 1024 H 1024 W 129" in _err(lib)
    assert lib.ustrun_signed_dist2_3d_work_bytes(1, 1, 1024, 1024, 129) == -1 and "2^27" in _err(lib)
    assert lib.ustrun_signed_dist2_3d_work_bytes(1, 1, 1024, 1024, 128) > 0
    for name in ENTRIES:
        assert _calls(lib, t, 2, 2, 2, N=2, K=16384, which=(name,))[name] != 0
        assert _err(lib).startswith(name + ":") and "32767" in _err(lib) and "N 2 K 16384" in _err(lib)
    assert _untouched(t)


@pytest.mark.parametrize("w", [(0, 1, 1), (1, 256, 1), (1, 1, -3), (256, 256, 256)])
def test_weights_out_of_range_are_refused(w):
    from ustrun import functional as F
    lib, t = _raw()
    for name in WEIGHTED:
        assert _calls(lib, t, 4, 4, 4, *w, which=(name,))[name] != 0
        assert _err(lib).startswith(name + ": axis weights") and f"wz {w[0]} wy {w[1]} wx {w[2]}" in _err(lib)
    assert _untouched(t)
    with pytest.raises(RuntimeError, match="signed_dist2_3d: axis weights"):
        F.signed_dist2_3d(torch.zeros(1, 1, 4, 4, 4, device="cuda"), weights=w)


def test_the_overflow_bound_is_refused():
    lib, t = _raw()
    bound = 46 * 46 * 1023 * 1023 + 1023 * 1023 + 127 * 127
    assert bound > 2 ** 31 - 2 >= 45 * 45 * 1023 * 1023
    for name in WEIGHTED:                                                    # D = H = 1024, W = 128, wz = 46, over dummy buffers
        assert _calls(lib, t, 1024, 1024, 128, wz=46, which=(name,))[name] != 0
        assert _err(lib).startswith(name + ": the largest squared distance") and str(bound) in _err(lib)
        assert "D 1024 H 1024 W 128 wz 46 wy 1 wx 1" in _err(lib)
    assert _untouched(t)


def test_null_pointers_short_work_and_misaligned_out_are_refused():
    lib, t = _raw()
    for name, keys in (("signed_dist2_3d", ("mask", "work", "s2", "flags")), ("sdf_from_dist2_3d", ("s2", "flags", "work", "sdf")),
                       ("surface_metrics_3d", ("mask", "work", "out"))):
        for key in keys:
            assert _calls(lib, t, 4, 4, 4, which=(name,), **{key: None})[name] != 0 and f"{name}: null pointer" in _err(lib)
        need = getattr(lib, f"ustrun_{name}_work_bytes")(1, 1, 4, 4, 4)
        assert 0 < need <= 1 << 20
        assert _calls(lib, t, 4, 4, 4, work_bytes=need - 1, which=(name,))[name] != 0
        assert _err(lib) == f"{name}: work buffer of {need - 1} bytes, needs {need}"
        assert _calls(lib, t, 4, 4, 4, which=(name,), work=t["work"].data_ptr() + 8)[name] != 0 and "16-byte" in _err(lib)
    assert lib.ustrun_signed_dist2_3d_work_bytes(1, 1, 4, 4, 4) == 16 + 2 * 64 * 2 + 64 * 4
    assert lib.ustrun_sdf_from_dist2_3d_work_bytes(1, 1, 4, 4, 4) == 16
    assert _calls(lib, t, 4, 4, 4, which=ENTRIES[2:], out=t["out"].data_ptr() + 4)[ENTRIES[2]] != 0 and "out 8-byte aligned" in _err(lib)
    assert _untouched(t)
    # with exactly the bytes asked for, all three run
    for name, rc in _calls(lib, t, 4, 4, 4, work_bytes=lib.ustrun_surface_metrics_3d_work_bytes(1, 1, 4, 4, 4)).items():
        assert rc == 0, (name, _err(lib))
    torch.cuda.synchronize()
    assert t["flags"][0].item() == 2 and (t["s2"][:64] == -0x7fffffff).all() and (t["s2"][64:] == 77).all()
    assert t["out"][:2].tolist() == [56, 56] and not t["out"][2:10].any() and (t["out"][10:] == 77).all()


def test_python_surface_refuses_what_it_cannot_read():
    from ustrun import functional as F
    with pytest.raises(RuntimeError, match="signed_dist2_3d: mask must be"):
        F.signed_dist2_3d(torch.zeros(1, 1, 4, 8, 8))
    with pytest.raises(RuntimeError, match="signed_dist2_3d: mask must be"):
        F.signed_dist2_3d(torch.zeros(1, 8, 8, device="cuda"))
    with pytest.raises(RuntimeError, match="by_class"):
        F.signed_dist2_3d(torch.zeros(1, 4, 8, 8, dtype=torch.int64, device="cuda"))
    with pytest.raises(RuntimeError, match="weights"):
        F.signed_dist2_3d(torch.zeros(1, 4, 8, 8, device="cuda"), weights=(1.5, 1, 1))
    with pytest.raises(RuntimeError, match="surface_metrics_3d: pred"):
        F.surface_metrics_3d(torch.zeros(1, 8, 8, device="cuda"), torch.zeros(1, 8, 8, device="cuda"))
