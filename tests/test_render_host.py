"""Host side of the `--save_img` overlays (csrc/render.hip, ustrun/render.py): the numpy restatement against the fixture g17 that
the reference's own functions drew (tools/gen_render_goldens.py), which pins the fixture without a GPU; the three C-ABI entries in
the header, the binding table and the built library; the script's flags."""
import os
import re
import subprocess

import numpy as np
import pytest

import render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "g17_render.npz")
Z = np.load(PATH, allow_pickle=False)
SYMBOLS = ("ustrun_render_range", "ustrun_render_mask", "ustrun_render_contour")


def test_fixture_has_the_cases_the_feature_is_specified_on():
    shapes, rules, kinds = set(), set(), set()
    for name in R.fixture_cases(Z, "mask"):
        img, pred, _, parts = R.fixture_inputs(Z, name)
        shapes.add(img.shape[1:])
        kinds.add(pred.dtype.type)
        rules.add(tuple(int(r) for r in Z[name + "_rule"]))
    assert {(3, 40, 56), (1, 37, 41), (1, 40, 56)} <= shapes
    assert kinds == {np.float32, np.int64}
    assert {r for t in rules for r in t} == {0, 1, 2} and any(len(set(t)) == 2 for t in rules)      # a batch with two branches
    assert any(int(Z[n + "_kind"]) == 1 and int(Z[n + "_pred"].max()) == 3 for n in R.fixture_cases(Z, "mask"))
    assert len(R.fixture_cases(Z, "contour")) >= 3
    assert os.path.getsize(PATH) < 1 << 20


@pytest.mark.parametrize("name", R.fixture_cases(Z, "mask"))
def test_mask_restatement_equals_the_reference_at_every_pixel(name):
    img, pred, _, parts = R.fixture_inputs(Z, name)
    on = R.planes_eq1(pred, parts)
    assert pred.dtype == np.int64 or (on.sum(1) > 1).any()     # plane cases overlap: the lowest index decides
    got = R.mask_overlay(img, pred, parts)
    assert got.dtype == np.uint8 and np.array_equal(got, Z[name + "_out"])


@pytest.mark.parametrize("name", R.fixture_cases(Z, "contour"))
def test_contour_restatement_equals_the_captured_float_image(name):
    img, pred, gt, parts = R.fixture_inputs(Z, name)
    f = R.contour_float(img, pred, gt, parts)
    assert f.dtype == np.float32 and np.array_equal(f, Z[name + "_float"].transpose(0, 2, 3, 1))
    assert np.array_equal(R.saturate(f), Z[name + "_out"])
    assert R.near_half(R.contour_value64(img, pred, gt, parts)).mean() <= 0.005


def test_rounding_rule_and_contour_definition():
    assert R.saturate(np.array([0.5, 1.5, 2.5, 254.5, 255.5, 300.0, -3.0, 2.4999])).tolist() == [0, 2, 2, 254, 255, 255, 0, 2]
    b = np.zeros((5, 6), bool)
    b[0, 0] = b[2, 3] = True
    ring = R.dilate3(b) & ~b
    assert ring.sum() == 3 + 8 and ring[1, 1] and ring[1, 2] and not ring[4, 5] and not ring[2, 3]


def test_header_declares_and_binding_lists_the_render_entries():
    from ustrun import _lib
    src = open(os.path.join(ROOT, "include", "ustrun.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, src), s
        assert s in _lib.SIGNATURES, s
    assert len(_lib.SIGNATURES["ustrun_render_mask"][1]) == 11 and len(_lib.SIGNATURES["ustrun_render_contour"][1]) == 12


def test_library_exports_the_render_entries():
    from ustrun import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import sys
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (ustrun_\w+)", out))
    assert set(SYMBOLS) <= exported


def test_render_argument_errors_need_no_gpu_work():
    from ustrun import _lib
    h = _lib.lib()
    assert h.ustrun_render_mask(None, None, None, 0, 1, 1, 1, 8, 8, None, None) != 0
    assert b"render_mask" in h.ustrun_last_error()


def test_script_accepts_the_save_img_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ustrun_test_script", os.path.join(ROOT, "ust-run_amd", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parser.parse_args(["--save_img", "--save_img_mode", "contour", "--save_dir", "X"])
    assert (a.save_img, a.save_img_mode, a.save_dir) == (True, "contour", "X")
    d = mod.parser.parse_args([])
    assert (d.save_img, d.save_img_mode, d.save_dir) == (False, "mask", "./img/save")        # the reference's path, test.py:113
    with pytest.raises(SystemExit):
        mod.parser.parse_args(["--save_img_mode", "sketch"])
