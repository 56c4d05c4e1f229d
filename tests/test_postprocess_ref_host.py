"""tests/postprocess_ref.py, the numpy restatement the GPU tests of ustrun_post_process compare against, is itself pinned: to the
reference's post_processing through the g18 fixture (tools/gen_postprocess_goldens.py), and to hand cases stated literally."""
import os

import numpy as np

import postprocess_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_postprocess.npz")


def test_ref_equals_the_reference_fixture_at_every_pixel():
    groups = R.load_golden(GOLDEN)
    assert sum(len(i) for i, _ in groups) >= 80
    for inp, out in groups:
        for p, want in zip(inp, out):
            assert np.array_equal(R.process(p), want)


def _squares():
    p = np.zeros((8, 20), bool)
    for k in range(5):
        p[2:4, 1 + 3 * k:3 + 3 * k] = True
    return p


def test_five_equal_squares_all_stay():
    p = _squares()
    assert p.sum() == 20 and np.array_equal(R.process(p), p)


def test_five_squares_and_one_pixel_leave_the_empty_plane():
    p = _squares()
    p[7, 19] = True
    assert not R.process(p).any()


def test_diamond_encloses_its_centre():
    p = np.zeros((7, 7), bool)
    p[2, 3] = p[4, 3] = p[3, 2] = p[3, 4] = True
    want = p.copy()
    want[3, 3] = True
    got = R.process(p)
    assert got.sum() == 5 and np.array_equal(got, want)


def test_frame_along_the_border_gives_the_full_plane():
    p = np.zeros((9, 11), bool)
    p[0] = p[-1] = True
    p[:, 0] = p[:, -1] = True
    assert R.process(p).all()


def test_ring_inside_the_hole_of_a_ring_gives_a_solid_disc():
    yy, xx = np.mgrid[:41, :41]
    d2 = (yy - 20) ** 2 + (xx - 20) ** 2
    p = ((d2 <= 18 ** 2) & (d2 >= 15 ** 2)) | ((d2 <= 8 ** 2) & (d2 >= 5 ** 2))
    assert np.array_equal(R.process(p), d2 <= 18 ** 2)


def test_empty_plane_stays_empty():
    assert not R.process(np.zeros((5, 6), bool)).any()


def test_switches_and_planes():
    p = np.zeros((1, 6, 8), np.int64)
    p[0, 1:5, 1:5] = 1
    p[0, 2, 2] = 0
    p[0, 0, 7] = 3                                       # a value above K belongs to no part
    pl = R.planes(p, by_class=True, K=2)
    assert pl.shape == (1, 2, 6, 8) and pl[0, 0].sum() == 15 and not pl[0, 1].any()
    assert np.array_equal(R.process(pl[0, 0], fill_holes=False, share=None), pl[0, 0])
    assert R.process(pl[0, 0], share=None).sum() == 16
    both = pl[0, 0].copy()
    both[0, 7] = True
    assert R.process(both, fill_holes=False).sum() == 15 and R.process(both, share=(1, 1)).sum() == 0
