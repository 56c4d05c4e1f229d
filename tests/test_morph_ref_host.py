"""tests/morph_ref.py -- the numpy restatement the GPU tests of csrc/morph.hip compare against -- is pinned to scipy.ndimage on the
host: binary_dilation / erosion / opening / closing with both structures, both border values and iterations 1, 2, 3, 5 and one
count past the box's extent, distance_transform_cdt in both metrics, on planes and volumes from empty to full; the separable form
is pinned to the brute force over all pairs; get_boundary to the reference's own GetBoundary outputs (tests/golden/g23_morph.npz,
written by tools/gen_morph_goldens.py)."""
import numpy as np
import pytest

import morph_ref as M

DENSITIES = (0.0, 0.03, 0.3, 0.9, 1.0)
BOXES = ((2, (9, 13)), (2, (1, 7)), (2, (16, 5)), (3, (5, 6, 7)), (3, (1, 5, 6)), (3, (2, 9, 4)))


def boxes():
    rs = np.random.RandomState(23)
    for rank, shape in BOXES:
        for dens in DENSITIES:
            yield rank, shape, dens, rs.rand(*shape) < dens


def test_separable_form_equals_the_brute_force():
    for rank, shape, dens, a in boxes():
        for metric in (M.L1, M.LINF):
            for outside in (False, True):
                assert np.array_equal(M.dist_sep(a, metric, rank, outside), M.dist_brute(a, metric, rank, outside)), (shape, dens, metric, outside)
    a = np.random.RandomState(1).rand(3, 2, 6, 7) < 0.2           # leading axes are a batch
    for metric in (M.L1, M.LINF):
        both = M.dist_sep(a, metric, 2, True)
        for n in range(3):
            for k in range(2):
                assert np.array_equal(both[n, k], M.dist_brute(a[n, k], metric, 2, True))


def test_morphology_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    ops = ((M.DILATE, ndi.binary_dilation), (M.ERODE, ndi.binary_erosion), (M.OPEN, ndi.binary_opening), (M.CLOSE, ndi.binary_closing))
    checked = 0
    for rank, shape, dens, a in boxes():
        for metric in (M.L1, M.LINF):
            st = ndi.generate_binary_structure(rank, 1 if metric == M.L1 else rank)
            for it in (1, 2, 3, 5, sum(shape) + 2):
                for b in (0, 1):
                    for op, fn in ops:
                        want = fn(a, structure=st, iterations=it, border_value=b)
                        for brute in (False, True):
                            assert np.array_equal(M.morph(a, metric, rank, op, it, b, brute), want), (shape, dens, metric, it, b, op, brute)
                        checked += 1
    assert checked == len(BOXES) * len(DENSITIES) * 2 * 5 * 2 * 4


def test_cdt_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rs = np.random.RandomState(5)
    cases = [a for _, _, _, a in boxes()]
    for shape in ((9, 13), (5, 6, 7)):                   # a mixed box with exactly one background pixel, in a corner and inside
        for at in (tuple(0 for _ in shape), tuple(n // 2 for n in shape), tuple(n - 1 for n in shape)):
            a = np.ones(shape, bool)
            a[at] = False
            cases.append(a)
        a = rs.rand(*shape) < 0.5
        cases.append(a)
    for a in cases:
        for metric, name in ((M.L1, "taxicab"), (M.LINF, "chessboard")):
            want = ndi.distance_transform_cdt(a, metric=name)
            got = M.distance_transform_cdt(a, metric, a.ndim)
            assert np.array_equal(got, want), (a.shape, name, int(a.sum()))
            sd, flags = M.chamfer(a, metric, a.ndim, 0)
            if not a.all():
                assert np.array_equal(np.where(sd < 0, -sd, 0), want)
            assert int(flags) == (0 if not a.any() else (2 if a.all() else 1))


def test_chamfer_signs_sentinels_and_outside_codes():
    a = np.zeros((4, 5), bool)
    a[1, 2] = True
    for metric in (M.L1, M.LINF):
        sd, flags = M.chamfer(a, metric, 2, 0)
        assert sd[1, 2] == -1 and sd[1, 3] == 1 and flags == 1
        assert sd[3, 4] == (4 if metric == M.L1 else 2)
        sd, flags = M.chamfer(np.zeros((4, 5), bool), metric, 2, 0)
        assert (sd == M.DIST_NONE).all() and flags == 0
        sd, flags = M.chamfer(np.ones((4, 5), bool), metric, 2, 0)
        assert (sd == -M.DIST_NONE).all() and flags == 2
        sd, flags = M.chamfer(np.ones((4, 5), bool), metric, 2, 1)       # the outside is background
        assert sd[0, 0] == -1 and sd[2, 2] == -2 and flags == 2
        sd, flags = M.chamfer(np.zeros((4, 5), bool), metric, 2, 2)      # the outside is foreground
        assert sd[0, 0] == 1 and sd[1, 2] == 2 and flags == 0
        sd, _ = M.chamfer(np.ones((1, 3, 3), bool), metric, 3, 1)        # a one-slice volume: 1 from the outside along z
        assert (sd == -1).all()


def test_get_boundary_equals_the_reference_goldens(golden):
    g = golden("g23_morph")
    names = [str(n) for n in g["names"]]
    assert len(names) >= 5 and [int(w) for w in g["widths"]] == [1, 3, 5]
    for name in names:
        mask = g[f"{name}_mask"]
        assert mask.ndim == 3 and mask.shape[2] == 2
        for w in (1, 3, 5):
            want = g[f"{name}_w{w}"]
            got = M.get_boundary(mask, w)
            assert got.dtype == np.uint8 and want.dtype == np.uint8 and np.array_equal(got, want), (name, w)
