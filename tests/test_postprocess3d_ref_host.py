"""tests/postprocess3d_ref.py, the numpy restatement the GPU tests of ustrun_post_process_3d compare against, is itself pinned: to
scipy.ndimage.binary_fill_holes and scipy.ndimage.label with the full 3 x 3 x 3 structure, to the plane restatement
(postprocess_ref.py) where the two must agree, to the reference's post_processing through the g22 fixture
(tools/gen_postprocess3d_goldens.py), and to hand cases stated literally."""
import os

import numpy as np
import pytest
from scipy import ndimage

import postprocess3d_ref as R
import postprocess_ref as R2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_postprocess3d.npz")


def _random(seed, shape, density):
    return np.random.default_rng(seed).random(shape) < density


@pytest.mark.parametrize("shape", [(5, 19, 70), (4, 7, 7), (1, 9, 9), (2, 6, 8), (7, 3, 5)])
@pytest.mark.parametrize("density", [0.15, 0.3, 0.5, 0.7])
def test_fill_and_labels_equal_scipy(shape, density):
    p = _random(100 * sum(shape) + int(100 * density), shape, density)
    f = R.fill(p)
    assert np.array_equal(f, ndimage.binary_fill_holes(p))
    lab, n = ndimage.label(f, structure=np.ones((3, 3, 3)))
    comps = R.components(f)
    assert len(comps) == n
    mine = np.zeros(f.size, np.int64)
    for k, c in enumerate(comps):
        mine[c] = k + 1
    assert np.array_equal(mine.reshape(shape), lab)        # scipy numbers components by their first voxel in raster order too
    for share in ((1, 5), (1, 2)):
        want = f.copy()
        for k in range(1, n + 1):
            if share[1] * int((lab == k).sum()) < share[0] * int(f.sum()):
                want[lab == k] = False
        assert np.array_equal(R.process(p, True, share), want)


def test_ref_equals_the_reference_fixture_at_every_voxel():
    groups = R.load_golden(GOLDEN)
    assert sum(len(i) for i, _ in groups) >= 40
    for inp, out in groups:
        for p, want in zip(inp, out):
            assert np.array_equal(R.process(p), want)
    assert (np.load(GOLDEN)["counts"] > 0).all()           # gained voxels, lost components, kept several, came out empty


def test_one_slice_without_filling_is_the_plane():
    for seed, density in enumerate((0.15, 0.3, 0.5)):
        p = _random(seed, (17, 23), density)
        for share in ((1, 5), (1, 2), None):
            assert np.array_equal(R.process(p[None], False, share)[0], R2.process(p, False, share))


def test_a_tube_gains_nothing_where_the_planes_gain_36():
    p = np.zeros((4, 7, 7), bool)
    p[:, 1:6, 1:6] = True
    p[:, 2:5, 2:5] = False
    assert np.array_equal(R.fill(p), p)
    assert sum(int(R2.fill(s).sum() - s.sum()) for s in p) == 36
    for axis in (1, 2):                                    # along y and along x
        q = np.moveaxis(p, 0, axis)
        assert np.array_equal(R.fill(q), q)


def test_the_closed_box_gains_its_27_voxels():
    p = np.zeros((7, 7, 7), bool)
    p[1:6, 1:6, 1:6] = True
    p[2:5, 2:5, 2:5] = False
    f = R.fill(p)
    assert f.sum() - p.sum() == 27 and f[1:6, 1:6, 1:6].all()


def test_the_octahedron_centre_is_filled():
    p = np.zeros((5, 5, 5), bool)
    for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        p[2 + d[0], 2 + d[1], 2 + d[2]] = True
    f = R.fill(p)
    assert f.sum() == 7 and f[2, 2, 2]
    assert len(R.components(p)) == 1                       # the six touch by edges: one component under 26-connectivity


def test_a_corner_touch_is_one_component():
    p = np.zeros((4, 4, 4), bool)
    p[0:2, 0:2, 0:2] = p[2:4, 2:4, 2:4] = True
    assert len(R.components(p)) == 1
    assert np.array_equal(R.process(p, share=(1, 1)), p)


@pytest.mark.parametrize("D", [1, 2])
def test_thin_volumes_gain_nothing(D):
    p = np.zeros((D, 9, 9), bool)
    p[:, 2:7, 2:7] = True
    p[:, 3:6, 3:6] = False
    assert np.array_equal(R.fill(p), p)
    assert np.array_equal(R.fill(_random(D, (D, 19, 21), 0.6)), _random(D, (D, 19, 21), 0.6))


def _five():
    p = np.zeros((3, 4, 11), bool)
    for k in range(5):
        p[0:2, 1:3, 2 * k] = True
    return p


def test_five_equal_components_all_stay_and_one_voxel_more_empties_the_volume():
    p = _five()
    assert p.sum() == 20 and len(R.components(p)) == 5 and np.array_equal(R.process(p), p)
    p[2, 3, 10] = True
    assert not R.process(p).any()
    assert not R.process(p, largest=True).any()            # emptied by the share rule: stays empty


def test_largest_only_tie_keeps_the_lower_index():
    p = _five()
    want = np.zeros_like(p)
    want[0:2, 1:3, 0] = True
    assert np.array_equal(R.process(p, share=None, largest=True), want)
    assert np.array_equal(R.process(p, share=(1, 5), largest=True), want)
    p[2, 1, 8] = True                                      # the last component now leads by one voxel
    want = np.zeros_like(p)
    want[0:2, 1:3, 8] = want[2, 1, 8] = True
    assert np.array_equal(R.process(p, share=None, largest=True), want)


def test_switches_and_volumes():
    m = np.zeros((1, 5, 6, 8), np.int64)
    m[0, 1:4, 1:5, 1:5] = 1
    m[0, 2, 2, 2] = 0
    m[0, 0, 0, 7] = 3                                      # a value above K belongs to no part
    v = R.volumes(m, by_class=True, K=2)
    assert v.shape == (1, 2, 5, 6, 8) and v[0, 0].sum() == 47 and not v[0, 1].any()
    assert np.array_equal(R.process(v[0, 0], fill_holes=False, share=None), v[0, 0])
    assert R.process(v[0, 0], share=None).sum() == 48
    out = R.process_batch(m, True, 2)
    assert out.dtype == np.float32 and out.shape == (1, 2, 5, 6, 8) and out.sum() == 48
    assert not R.process(np.zeros((3, 4, 5), bool), largest=True).any()
