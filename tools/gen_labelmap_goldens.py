#!/usr/bin/env python3
"""Writes tests/golden/g21_labelmap.npz: small inputs (N = 2, 9 x 13, K in {2, 21}) and what the reference's own label-map losses,
metrics and colour decoders return for them on the CPU, values and gradients.

The reference's utils/metrics.py and dataloaders/utils.py are loaded IN PLACE by path (`--reference DIR`), not through their
packages; dataloaders/utils.py imports skimage.measure and matplotlib.pyplot, which need not be installed: empty stand-in modules
sit in sys.modules (none of the functions recorded here touches them).

Run as written, from the reference: metrics.cross_entropy2d (with weight, both size_average values), utils.cross_entropy2d with
weight=None (all four flag pairs), get_dice, get_iou, decode_segmap, decode_seg_map_sequence, encode_segmap, get_pascal_labels,
get_cityscapes_labels, DiceLoss, Balanced_DiceLoss, dice.

Restated here over torch's own operators, because the reference's lines cannot run on this CPU:
  * cal_dice: it calls np.float, which numpy no longer has -- the same lines with np.float64;
  * WatershedCrossEntropy and the weighted branch of utils.cross_entropy2d: both call .cuda() -- the same lines without it (the
    former with the reference's own distance_transform and bce).
get_iou: the reference's result (0.0 for every input under today's torch, where bool + bool is a logical OR) is recorded as
`iou_reference` beside the intended value `iou_intended` (tests/labelmap_ref.py: iou_direct).

The names and signatures of the functions the project adds are read from the reference with inspect and recorded as strings.

    python tools/gen_labelmap_goldens.py --reference /path/to/reference
"""
import argparse
import importlib.util
import inspect
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import labelmap_ref as R  # noqa: E402

METRICS_NAMES = ["cal_dice", "dice", "WatershedCrossEntropy", "cross_entropy2d", "dice_loss", "DiceLoss", "Balanced_DiceLoss"]
UTILS_NAMES = ["cross_entropy2d", "get_iou", "get_dice", "decode_segmap", "decode_seg_map_sequence", "encode_segmap", "get_pascal_labels",
               "get_cityscapes_labels", "lr_poly", "untransform"]


def stand_ins():
    for name in ("skimage", "skimage.measure", "matplotlib", "matplotlib.pyplot"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
            if "." in name:
                setattr(sys.modules[name.split(".")[0]], name.split(".")[1], sys.modules[name])


def load(root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.abspath(root), *rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def vg(fn, x):
    """float32 value and gradient of UP * fn(x), as the reference computes them"""
    xx = x.clone().requires_grad_(True)
    v = fn(xx)
    g, = torch.autograd.grad(v * R.UP, xx)
    return np.float32(v.item()), g.numpy()


def close(mine, ref):
    """a float32 restatement against the reference's float32 result: a few roundings of the largest value"""
    return float(np.abs(mine - ref).max()) <= 2e-6 * float(np.abs(ref).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's root directory (holds utils/ and dataloaders/)")
    a = ap.parse_args()
    warnings.filterwarnings("ignore")
    stand_ins()
    M = load(a.reference, ("utils", "metrics.py"), "reference_utils_metrics")
    U = load(a.reference, ("dataloaders", "utils.py"), "reference_dataloaders_utils")
    g = torch.Generator().manual_seed(21)
    N, H, W = 2, 9, 13
    z = {}
    z["metrics_signatures"] = np.array(["%s%s" % (n, inspect.signature(getattr(M, n))) for n in METRICS_NAMES])
    z["utils_signatures"] = np.array(["%s%s" % (n, inspect.signature(getattr(U, n))) for n in UTILS_NAMES])

    # ---- cross-entropy over a label map, K = 21 and K = 2
    for K in (2, 21):
        x = 3 * torch.randn(N, K, H, W, generator=g)
        t = torch.randint(0, K, (N, H, W), generator=g)
        hole = torch.rand(N, H, W, generator=g) < 0.15
        t_neg, t_255 = torch.where(hole, -1, t), torch.where(hole, 255, t)
        w = 0.5 + torch.rand(K, generator=g)
        z[f"ce{K}_logits"], z[f"ce{K}_t_neg"], z[f"ce{K}_t_255"], z[f"ce{K}_weight"] = x.numpy(), t_neg.numpy(), t_255.numpy(), w.numpy()
        for wt in (0, 1):
            for sa in (0, 1):
                v, gr = vg(lambda xx: M.cross_entropy2d(xx, t_neg, weight=w if wt else None, size_average=bool(sa)), x)
                z[f"ce{K}_metrics_w{wt}_sa{sa}"] = v
                if K == 2 or wt:
                    z[f"ce{K}_metrics_w{wt}_sa{sa}_grad"] = gr
                mine = R.ce_map(x, t_neg, w if wt else None, None, True, 1.0, True, bool(sa), dtype=torch.float32)
                assert np.allclose(mine["out"][0].item(), v, rtol=1e-5), (K, wt, sa)
                assert close(mine["grad"].numpy(), gr), (K, wt, sa)
        for sa in (0, 1):
            for ba in (0, 1):
                v, gr = vg(lambda xx: U.cross_entropy2d(xx, t_255[:, None], size_average=bool(sa), batch_average=bool(ba)), x)
                z[f"ce{K}_utils_s{sa}_b{ba}"] = v
                if K == 2 or (sa and ba):
                    z[f"ce{K}_utils_s{sa}_b{ba}_grad"] = gr
                mine = R.ce_map(x, t_255, None, 255, False, 1.0 / ((H * W if sa else 1) * (N if ba else 1)), dtype=torch.float32)
                assert np.allclose(mine["out"][0].item(), v, rtol=1e-5) and close(mine["grad"].numpy(), gr)

        def weighted(xx):            # dataloaders/utils.py:135-144 without .cuda()
            crit = torch.nn.CrossEntropyLoss(weight=torch.from_numpy(np.array(w.tolist())).float(), ignore_index=255, size_average=False)
            return crit(xx, t_255.long()) / (H * W) / N
        z[f"ce{K}_utils_weighted"], z[f"ce{K}_utils_weighted_grad"] = vg(weighted, x)

    # ---- label maps: get_dice, get_iou, cal_dice, colours
    pred = torch.randint(0, 21, (N, H, W), generator=g)
    gt = torch.where(torch.rand(N, H, W, generator=g) < 0.6, pred, torch.randint(0, 21, (N, H, W), generator=g))
    gt[1, :, :6] = 3
    z["lab_pred"], z["lab_gt"] = pred.numpy(), gt.numpy()
    z["get_dice"] = np.float64(U.get_dice(pred, gt))
    z["iou_reference"] = np.float64(U.get_iou(pred, gt, 21))
    z["iou_intended"] = np.float64(R.iou_direct(pred.numpy(), gt.numpy(), 21))
    assert z["iou_reference"] == 0.0 and z["iou_intended"] > 0.5
    assert z["get_dice"] == R.get_dice_direct(pred.numpy(), gt.numpy())

    def cal_dice(prediction, label, num):          # utils/metrics.py:13-24 with np.float64 for np.float
        total = np.zeros(num - 1)
        for i in range(1, num):
            p, l = (prediction == i).astype(np.float64), (label == i).astype(np.float64)
            total[i - 1] += 2 * np.sum(p * l) / (np.sum(p) + np.sum(l))
        return total
    z["cal_dice_5"] = cal_dice(pred.numpy() % 5, gt.numpy() % 5, 5)
    assert np.array_equal(z["cal_dice_5"], R.cal_dice_direct(pred.numpy() % 5, gt.numpy() % 5, 5))

    z["pascal_labels"], z["cityscapes_labels"] = U.get_pascal_labels().astype(np.uint8), U.get_cityscapes_labels().astype(np.uint8)
    assert np.array_equal(z["pascal_labels"], R.pascal_palette())
    odd = pred.numpy().copy()
    odd[0, 0, :4] = (21, 255, 300, 19)           # outside one palette or both: the reference leaves label / 255 there
    z["colour_labels"] = odd
    for ds in ("pascal", "cityscapes"):
        z[f"decode_{ds}"] = np.stack([U.decode_segmap(m, ds) for m in odd])
        assert np.array_equal(z[f"decode_{ds}"], R.colorize(odd, z[f"{ds}_labels"]))
        assert np.array_equal(U.decode_seg_map_sequence(odd, ds).numpy(), z[f"decode_{ds}"].transpose(0, 3, 1, 2))
    img = np.rint(U.decode_segmap(pred.numpy()[0], "pascal") * 255).astype(np.uint8)
    img[0, 0] = (1, 2, 3)                         # no Pascal colour: class 0
    z["encode_image"], z["encode_labels"] = img, U.encode_segmap(img)
    assert np.array_equal(z["encode_labels"], R.encode_segmap(img))

    # ---- sigmoid-map losses on [N,2,H,W]
    x = 2 * torch.randn(N, 2, H, W, generator=g)
    yy, xx_ = np.mgrid[:H, :W]
    disc = ((yy - 4) ** 2 + (xx_ - 6) ** 2 <= 16).astype(np.float32)
    cup = ((yy - 4) ** 2 + (xx_ - 6) ** 2 <= 4).astype(np.float32)
    t = torch.from_numpy(np.stack([np.stack([disc, cup]), np.stack([np.roll(disc, 2, 1), np.roll(cup, 1, 0)])]))
    p = torch.sigmoid(x)
    tig = t.clone()
    tig[0, 0, :2] = 255.0
    z["map_logits"], z["map_target"], z["map_target_ignore"] = x.numpy(), t.numpy(), tig.numpy()
    z["DiceLoss"], z["DiceLoss_grad"] = vg(lambda q: M.DiceLoss(q, t), p)
    z["Balanced_DiceLoss"], z["Balanced_DiceLoss_grad"] = vg(lambda q: M.Balanced_DiceLoss(q, t), x)
    z["dice"], z["dice_grad"] = vg(lambda q: M.dice(q, t), p)
    z["dice_ignore"], z["dice_ignore_grad"] = vg(lambda q: M.dice(q, tig, ignore_index=255), p)

    def watershed(inp):            # utils/metrics.py:72-91 without .cuda()
        discmap, cupmap = t[:, 0], t[:, 1]
        disc_dt = torch.from_numpy(M.distance_transform(discmap)).float()
        cup_dt = torch.from_numpy(M.distance_transform(cupmap)).float()
        disc_dt = discmap * (1.0 - disc_dt / torch.max(disc_dt)) + 1.0
        cup_dt = cupmap * (1.0 - cup_dt / torch.max(cup_dt)) + 1.0
        ce = M.bce(inp, t)
        return torch.mean(disc_dt * ce[:, 0] + cup_dt * ce[:, 1])
    z["WatershedCrossEntropy"], z["WatershedCrossEntropy_grad"] = vg(watershed, x)
    for name, fn, arg, kw in (("DiceLoss", R.DiceLoss, p, {}), ("Balanced_DiceLoss", R.Balanced_DiceLoss, x, {}), ("dice", R.dice, p, {}),
                              ("dice_ignore", R.dice, p, {"ignore_index": 255.0}), ("WatershedCrossEntropy", R.WatershedCrossEntropy, x, {})):
        tt = tig if name == "dice_ignore" else t
        v, gr = R.value_and_grad(fn, arg, tt, dtype=torch.float32, **kw)
        assert np.allclose(v.item(), z[name], rtol=1e-5), name
        assert close(gr.numpy(), z[name + "_grad"]), name

    path = os.path.join(ROOT, "tests", "golden", "g21_labelmap.npz")
    np.savez_compressed(path, **z)
    print("wrote", os.path.normpath(path), os.path.getsize(path), "bytes,", len(z), "arrays")


if __name__ == "__main__":
    main()
