"""Host side of the surface-distance metrics (dc / jc / hd95 / asd of the reference's test(), train.py:306-325): the numpy
finish of the device records (utils.metrics.surface_from_records) against the scipy-generated fixture g15, its empty-mask
rules, and the two C-ABI symbols of the device part."""
import os
import re
import subprocess

import numpy as np
import pytest

import surface_brute as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "g15_surface_metrics.npz"), allow_pickle=False)
SYMBOLS = ("ustrun_surface_metrics_work_bytes", "ustrun_surface_metrics")


def test_fixture_has_the_sizes_and_contents_the_feature_is_specified_on():
    shapes = {tuple(int(v) for v in Z[n + "_shape"][2:]) for n in B.fixture_cases(Z)}
    assert {(256, 256), (288, 288), (384, 384), (512, 512), (40, 72)} <= shapes
    assert all(int(Z[n + "_shape"][0]) >= 4 for n in B.fixture_cases(Z))
    assert any(int(Z[n + "_kind"]) == 1 and int(Z[n + "_shape"][1]) == 3 for n in B.fixture_cases(Z))      # M&Ms class maps
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g15_surface_metrics.npz")) < 1 << 20


@pytest.mark.parametrize("name", B.fixture_cases(Z))
def test_records_from_brute_force_reproduce_the_fixture(name):
    """all-pairs distances between the border pixel lists -> records -> surface_from_records == the scipy restatement:
    integers, dc and jc exactly; hd95 and asd to 1e-9 relative (everything before the square roots is exact, what is left is
    f64 rounding of <= 1e5-term sums and the one-ulp variants of numpy's lerp)."""
    from utils import metrics
    pred, gt, by_class, K = B.fixture_inputs(Z, name)
    rec, cnt = B.records(pred, gt, by_class, K)
    assert np.array_equal(rec[..., 0:2], Z[name + "_nborder"])
    assert np.array_equal(rec[..., 2:4], Z[name + "_d2"])
    dc, jc, hd, asd = metrics.surface_from_records(rec, cnt)
    assert all(a.dtype == np.float64 and a.shape == rec.shape[:2] for a in (dc, jc, hd, asd))
    assert np.array_equal(dc, Z[name + "_dc"]) and np.array_equal(jc, Z[name + "_jc"])
    np.testing.assert_allclose(hd, Z[name + "_hd95"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(asd, Z[name + "_asd"], rtol=1e-9, atol=0)


def test_brute_force_metrics_agree_with_the_fixture():
    """the second, records-free restatement the end-to-end GPU test averages (numpy.percentile / mean on the distances)"""
    for name in ("frame_40x72", "speckle_40x72", "rings_40x72_i64", "discs_256"):
        pred, gt, by_class, K = B.fixture_inputs(Z, name)
        P, G = B.planes(pred, gt, by_class, K)
        got = np.array([[B.metrics(P[n, k], G[n, k]) for k in range(P.shape[1])] for n in range(P.shape[0])])
        for j, key in enumerate(("dc", "jc")):
            assert np.array_equal(got[..., j], Z[f"{name}_{key}"])
        for j, key in ((2, "hd95"), (3, "asd")):
            np.testing.assert_allclose(got[..., j], Z[f"{name}_{key}"], rtol=1e-9, atol=0)


def test_percentile_position_and_lerp_are_numpys():
    """n values with known roots: the two order statistics at k = floor(0.95 (n-1)) and the linear weight give numpy.percentile"""
    from utils import metrics
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 20, 21, 41, 101, 1000, 4097):
        d2 = np.sort(rng.integers(0, 2 ** 21, n))
        k = int(np.floor(0.95 * np.float64(n - 1)))
        rec = np.zeros((1, 1, 6), np.int32)
        n0 = (n + 1) // 2
        rec[0, 0, :4] = n0, n - n0, d2[k], d2[min(k + 1, n - 1)]
        cnt = np.array([[[max(n0, 1), max(n - n0, 1), 0]]])
        hd = metrics.surface_from_records(rec, cnt)[2]
        np.testing.assert_allclose(hd[0, 0], np.percentile(np.sqrt(d2.astype(np.float64)), 95), rtol=1e-12, atol=0)


def test_empty_prediction_scores_100_and_empty_ground_truth_raises():
    from utils import metrics
    g = np.zeros((2, 1, 9, 9), bool)
    g[:, 0, 3:6, 3:6] = True
    p = g.copy()
    p[1] = False                                            # sample 1: the empty prediction of train.py:313-315
    rec, cnt = B.records(p.astype(np.float32), g.astype(np.float32))
    dc, jc, hd, asd = metrics.surface_from_records(rec, cnt)
    assert (dc[0, 0], jc[0, 0], hd[0, 0], asd[0, 0]) == (1.0, 1.0, 0.0, 0.0)
    assert (dc[1, 0], jc[1, 0], hd[1, 0], asd[1, 0]) == (0.0, 0.0, 100.0, 100.0)
    rec, cnt = B.records(g.astype(np.float32), p.astype(np.float32))       # roles swapped: sample 1 has no ground truth
    with pytest.raises(RuntimeError, match=r"batch 7, sample 1, part 0"):
        metrics.surface_from_records(rec, cnt, where="batch 7, ")


def test_abi_declares_binds_and_exports_the_two_entry_points():
    header = open(os.path.join(ROOT, "include", "ustrun.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    from ustrun import _lib
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.SIGNATURES, s
    if not os.path.exists(_lib.LIB_PATH):
        import sys
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (ustrun_\w+)", out))
    assert set(SYMBOLS) <= exported


def test_sizes_outside_1_to_1024_are_refused_before_any_launch():
    from ustrun import _lib
    h = _lib.lib()
    assert h.ustrun_surface_metrics_work_bytes(4, 2, 384, 384) >= 4 * 2 * 384 * 384 * 12
    for H, W in ((1025, 64), (64, 1025), (0, 64), (64, 0)):
        assert h.ustrun_surface_metrics_work_bytes(1, 1, H, W) == -1
        assert b"surface_metrics" in h.ustrun_last_error()
        rc = h.ustrun_surface_metrics(1, 1, 0, 0, 1, 1, 0, H, W, 16, 1 << 40, 8, None)     # argument check precedes any launch
        assert rc != 0 and b"1..1024" in h.ustrun_last_error()
