"""CPU checks of the label-map feature: tests/labelmap_ref.py (the restatement the GPU tests compare against) pinned to the
reference's own results (g21_labelmap.npz, tools/gen_labelmap_goldens.py), the palette quotient in float32, the confusion-matrix
identities behind get_iou / get_dice / cal_dice against direct loops, and the names utils.metrics / dataloaders.utils must carry."""
import inspect

import numpy as np
import pytest
import torch

import labelmap_ref as R
from conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("g21_labelmap")


def close32(mine, ref):
    """a float32 restatement against the reference's float32 result: a few roundings of the largest value"""
    return float(np.abs(np.asarray(mine, np.float64) - ref).max()) <= 2e-6 * float(np.abs(ref).max())


def close64(mine, ref32):
    """the float64 restatement against a float32 result of the reference: f32 sums of a few hundred terms"""
    return float(np.abs(np.asarray(mine) - ref32).max()) <= 2e-5 * float(np.abs(ref32).max())


@pytest.mark.parametrize("K", [2, 21])
def test_cross_entropy_restatement_matches_the_reference(gold, K):
    x, tn, t255, w = (torch.from_numpy(gold[f"ce{K}_{n}"]) for n in ("logits", "t_neg", "t_255", "weight"))
    N, H, W = tn.shape
    checked = 0
    for dtype, close in ((torch.float32, close32), (torch.float64, close64)):
        for wt in (0, 1):
            for sa in (0, 1):
                m = R.ce_map(x, tn, w if wt else None, None, True, 1.0, True, bool(sa), dtype=dtype)
                assert close(m["out"][0].item(), gold[f"ce{K}_metrics_w{wt}_sa{sa}"])
                if f"ce{K}_metrics_w{wt}_sa{sa}_grad" in gold:
                    assert close(m["grad"].numpy(), gold[f"ce{K}_metrics_w{wt}_sa{sa}_grad"])
                    checked += 1
        for sa in (0, 1):
            for ba in (0, 1):
                m = R.ce_map(x, t255, None, 255, False, 1.0 / ((H * W if sa else 1) * (N if ba else 1)), dtype=dtype)
                assert close(m["out"][0].item(), gold[f"ce{K}_utils_s{sa}_b{ba}"])
                if f"ce{K}_utils_s{sa}_b{ba}_grad" in gold:
                    assert close(m["grad"].numpy(), gold[f"ce{K}_utils_s{sa}_b{ba}_grad"])
                    checked += 1
        m = R.ce_map(x, t255, w, 255, False, 1.0 / (H * W * N), dtype=dtype)
        assert close(m["out"][0].item(), gold[f"ce{K}_utils_weighted"]) and close(m["grad"].numpy(), gold[f"ce{K}_utils_weighted_grad"])
    assert checked >= 6
    assert int(m["out"][3]) == int((t255 != 255).sum()) and int(m["out"][4]) == 0


def test_cross_entropy_edge_rules():
    """no valid pixel: nan with a divisor, 0 without, gradient 0; out-of-range targets add nothing and are counted"""
    x = torch.randn(1, 3, 2, 2)
    t = torch.full((1, 2, 2), 255)
    m = R.ce_map(x, t, None, 255, False, 1.0, True, False)
    assert torch.isnan(m["out"][0]) and not m["grad"].any()
    m = R.ce_map(x, t, None, 255, False, 1.0, False, False)
    assert m["out"][0] == 0 and not m["grad"].any()
    t = torch.tensor([[[0, 7], [-3, 255]]])
    m = R.ce_map(x, t, None, 255, False)
    assert m["out"][3] == 1 and m["out"][4] == 2 and not m["grad"][0, :, 0, 1].any() and not m["grad"][0, :, 1].any()
    m = R.ce_map(x, t, None, 255, True)
    assert m["out"][3] == 1 and m["out"][4] == 1
    want = torch.nn.functional.cross_entropy(x.double(), torch.tensor([[[0, 255], [255, 255]]]), ignore_index=255, reduction="sum")
    assert abs(float(m["out"][0]) - float(want)) < 1e-12


def test_sigmoid_map_losses_match_the_reference(gold):
    x, t, tig = (torch.from_numpy(gold[n]) for n in ("map_logits", "map_target", "map_target_ignore"))
    p = torch.sigmoid(x)
    for name, fn, arg, tt, kw in (("DiceLoss", R.DiceLoss, p, t, {}), ("Balanced_DiceLoss", R.Balanced_DiceLoss, x, t, {}), ("dice", R.dice, p, t, {}),
                                  ("dice_ignore", R.dice, p, tig, {"ignore_index": 255.0}),
                                  ("WatershedCrossEntropy", R.WatershedCrossEntropy, x, t, {})):
        for dtype, close in ((torch.float32, close32), (torch.float64, close64)):
            v, g = R.value_and_grad(fn, arg, tt, dtype=dtype, **kw)
            assert close(v.item(), gold[name]), name
            assert close(g.numpy(), gold[name + "_grad"]), name
    empty = t.clone()
    empty[:, 1] = 0          # the reference's weight is nan over an empty plane; the target + 1 form stays finite
    assert torch.isfinite(R.WatershedCrossEntropy(x, empty))


def test_plane_sums_restatement_against_plain_sums(gold):
    x, t = torch.from_numpy(gold["map_logits"]).double(), torch.from_numpy(gold["map_target_ignore"]).double()
    s = R.plane_sums(x, t, "sigmoid", 255.0)
    keep = t != 255
    for k in range(2):
        sk, tk, m = torch.sigmoid(x[:, k]), t[:, k], keep[:, k]
        bce = torch.clamp(x[:, k], min=0) - x[:, k] * tk + torch.log1p(torch.exp(-x[:, k].abs()))
        want = torch.stack([(sk * tk)[m].sum(), sk[m].sum(), tk[m].sum(), ((1 + tk) * bce)[m].sum()])
        assert torch.allclose(s[k], want, rtol=1e-12, atol=0)
    assert not R.plane_sums(x, t, "none")[:, 3].any()


def test_confusion_identities_against_direct_loops(gold):
    pred, gt = gold["lab_pred"], gold["lab_gt"]
    c, skipped = R.confusion(pred, gt, 21)
    assert c.dtype == np.int32 and c.shape == (2, 21, 21) and not skipped.any() and c.sum() == pred.size
    for n in range(2):
        for a in range(21):
            for b in range(21):
                assert c[n, a, b] == int(((gt[n] == a) & (pred[n] == b)).sum())
    assert abs(R.iou_from_counts(c) - R.iou_direct(pred, gt, 21)) < 1e-12
    assert abs(R.iou_from_counts(c) - float(gold["iou_intended"])) < 1e-12 and float(gold["iou_reference"]) == 0.0
    assert R.get_dice_from_counts(c) == R.get_dice_direct(pred, gt) == float(gold["get_dice"])
    c32, _ = R.confusion(pred, gt, 32)                     # get_dice counts 32 classes whatever the labels are
    assert R.get_dice_from_counts(c32) == float(gold["get_dice"])
    c5, _ = R.confusion((pred % 5).reshape(1, -1), (gt % 5).reshape(1, -1), 5)
    assert np.array_equal(R.cal_dice_from_counts(c5), R.cal_dice_direct(pred % 5, gt % 5, 5))
    assert np.allclose(R.cal_dice_from_counts(c5), gold["cal_dice_5"], rtol=1e-15, atol=0)
    # ignored and out-of-range pixels leave the counts and are skipped; a float label that is no integer is out of range
    g2 = gt.copy()
    g2[0, 0, :3] = 255
    g2[1, 0, 0] = -1
    p2 = pred.astype(np.float32)
    p2[1, 1, 1] = 2.5
    c2, s2 = R.confusion(p2, g2, 21, ignore_index=255)
    assert list(s2) == [3, 2] and c2.sum() == pred.size - 5


def test_palette_quotients_in_float32():
    """byte / 255 divided in float32 is the float64 quotient rounded to float32, for all 256 bytes"""
    c = np.arange(256)
    assert np.array_equal(c.astype(np.float32) / np.float32(255.0), (c / 255.0).astype(np.float32))
    assert np.array_equal(np.rint((c / 255.0).astype(np.float32).astype(np.float64) * 255.0), c)      # and the byte comes back


def test_colour_restatement_matches_the_reference(gold):
    assert np.array_equal(R.pascal_palette(), gold["pascal_labels"])
    for ds in ("pascal", "cityscapes"):
        assert np.array_equal(R.colorize(gold["colour_labels"], gold[f"{ds}_labels"]), gold[f"decode_{ds}"])
    assert np.array_equal(R.encode_segmap(gold["encode_image"]), gold["encode_labels"])


def test_added_names_exist_with_the_reference_signatures(gold):
    """every tensor-arithmetic name of the reference's utils/metrics.py and dataloaders/utils.py, with its parameters and defaults"""
    import dataloaders.utils as U
    from utils import metrics as M
    for mod, key in ((M, "metrics_signatures"), (U, "utils_signatures")):
        for rec in gold[key]:
            name = str(rec).split("(")[0]
            assert hasattr(mod, name), (mod.__name__, name)
            assert name + str(inspect.signature(getattr(mod, name))) == str(rec), (mod.__name__, name)


def test_host_helpers_match_the_reference(gold):
    import dataloaders.utils as U
    assert np.array_equal(U.get_pascal_labels(), gold["pascal_labels"]) and np.array_equal(U.get_cityscapes_labels(), gold["cityscapes_labels"])
    assert U.get_pascal_labels().shape == (21, 3) and U.get_cityscapes_labels().shape == (19, 3)
    got = U.encode_segmap(gold["encode_image"])
    assert got.dtype == gold["encode_labels"].dtype and np.array_equal(got, gold["encode_labels"])
    assert U.lr_poly(0.1, 25) == 0.1 * ((1 - 25.0 / 100) ** 0.9) and U.lr_poly(1.0, 3, max_iter=10, power=2) == (1 - 0.3) ** 2
    img, lt = U.untransform(np.array([-1.0, 0.0, 1.0]), np.array([0.5, 1.0]))
    assert np.array_equal(img, [0.0, 127.5, 255.0]) and np.array_equal(lt, [64.0, 128.0])
    from utils.metrics import dice_coeff, dice_loss
    a, b = (np.arange(24).reshape(2, 3, 4) % 3 == 0), (np.arange(24).reshape(2, 3, 4) % 2 == 0)
    assert dice_loss(a[0], b[0]) == 1 - dice_coeff(a[0], b[0])
    assert dice_loss(a, b) == [1 - v for v in dice_coeff(a, b)]       # the reference raises TypeError here
