"""Binary Dice metrics (host side) -- same surface as the reference's utils/metrics.py:114-231.

`dice_coefficient_numpy` is (2I+1)/(1.001+S+G), 0.0 when both masks are empty.  The per-sample
overlap counts can also come from the device (ustrun.functional.dice_counts): `dice_from_counts`
applies the same formula to them, so the training step needs one small D2H copy instead of moving
whole masks to the host.

`surface_from_records` is the host part of the medpy metrics the reference's test() prints beside the Dice
(binary.dc / jc / hd95 / asd, train.py:306-325): the device (ustrun.functional.surface_metrics) delivers, per sample and
part, the border sizes, the two integer order statistics of the squared surface distances and the sum of the
prediction's distances; the square roots, numpy's linear percentile and the reference's empty-mask rules are applied here.

`spacing_weights` and `volume_metrics` are the per-case form of the same metrics on volumes with `voxelspacing`
(ustrun.functional.surface_metrics_3d), adding medpy's hd and assd.

`distance_transform` is the Euclidean distance transform utils/metrics.py:52-70 means to be, computed on the device.

`cal_dice`, `dice`, `WatershedCrossEntropy`, `cross_entropy2d`, `dice_loss`, `DiceLoss` and `Balanced_DiceLoss` keep the reference's
signatures and defaults; their arithmetic over tensors runs on the device (ustrun.functional: ce_map, confusion, plane_sums).
"""
import numpy as np


def _np(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def dice_from_counts(s, g, i):
    """Dice from |pred|, |gt|, |pred & gt| (scalars or arrays)."""
    s, g, i = np.asarray(s, dtype=np.float64), np.asarray(g, dtype=np.float64), np.asarray(i, dtype=np.float64)
    d = (2.0 * i + 1.0) / (1.001 + s + g)
    return np.where((s == 0) & (g == 0), 0.0, d)


EMPTY_PRED_VALUE = 100.0          # train.py:313-315: hd and asd of a sample whose prediction is empty


class EmptyGroundTruth(RuntimeError):
    """hd95 / asd asked for a (sample, part) whose ground truth is empty; `.sample`, `.part` index the arrays given."""

    def __init__(self, sample, part, where=""):
        super().__init__(f"surface metrics: {where}sample {sample}, part {part}: the ground truth is empty "
                         "(hd95 / asd are undefined; the reference's medpy raises here)")
        self.sample, self.part = int(sample), int(part)


def surface_from_records(records, counts, where=""):
    """records: int32 [N, parts, 6] of ustrun.functional.surface_metrics; counts: [N, parts, 3] = {|P|, |G|, |P & G|}
    (dice_counts).  -> (dc, jc, hd95, asd), float64 [N, parts] each:
      dc = 2|P&G| / (|P|+|G|), 0.0 on 0/0;  jc = |P&G| / |P|G|;
      hd95 = numpy.percentile(both directions' distances, 95): linear between sqrt(d2[k]) and sqrt(d2[k+1]) at 0.95 (n-1);
      asd = sum of the prediction's distances / |border(P)|;  |P| = 0 -> hd95 = asd = 100;
      |G| = 0 -> EmptyGroundTruth, a RuntimeError (medpy raises on an empty reference object), naming `where` (the caller's
      words for the batch), the sample and the part."""
    rec = np.ascontiguousarray(_np(records), dtype=np.int32)
    cnt = np.asarray(_np(counts), dtype=np.int64)
    if rec.ndim != 3 or rec.shape[2] != 6 or cnt.shape != rec.shape[:2] + (3,):
        raise ValueError(f"surface_from_records: records {rec.shape} / counts {cnt.shape} are not [N,parts,6] / [N,parts,3]")
    s, g, i = cnt[..., 0], cnt[..., 1], cnt[..., 2]
    if (g == 0).any():
        raise EmptyGroundTruth(*np.argwhere(g == 0)[0], where)
    dc = np.where(s + g > 0, 2.0 * i / np.maximum(s + g, 1), 0.0)
    jc = i / (s + g - i).astype(np.float64)
    nbp, nbg = rec[..., 0].astype(np.int64), rec[..., 1].astype(np.int64)
    total = np.ascontiguousarray(rec[..., 4:6]).view(np.float64)[..., 0]
    n = nbp + nbg
    pos = 0.95 * (n - 1).astype(np.float64)
    t = pos - np.floor(pos)
    a, b = np.sqrt(rec[..., 2].astype(np.float64)), np.sqrt(rec[..., 3].astype(np.float64))
    # numpy's _lerp: a + (b-a) t, and b - (b-a)(1-t) from t = 0.5 on
    hd = np.where(t >= 0.5, b - (b - a) * (1 - t), a + (b - a) * t)
    asd = total / np.maximum(nbp, 1)
    empty = s == 0
    return dc, jc, np.where(empty, EMPTY_PRED_VALUE, hd), np.where(empty, EMPTY_PRED_VALUE, asd)


def spacing_weights(voxelspacing, max_scale=64, rtol=1e-6):
    """medpy's `voxelspacing` (z, y, x) as the integer axis weights of the device's exact metric (ustrun_surface_metrics_3d):
    -> ((wz, wy, wx), unit) with spacing_i = weight_i * unit up to `rtol`, so that a distance is unit * sqrt(d2).
    The smallest m <= max_scale for which every spacing_i / min(spacing) * m lies within rtol (relative) of an integer is taken;
    weights are those integers and unit = min(spacing) / m.  ValueError when no such m exists or a weight exceeds 255.
    Pure host code."""
    sp = [float(v) for v in voxelspacing]
    if len(sp) != 3 or not all(np.isfinite(v) and v > 0 for v in sp):
        raise ValueError(f"spacing_weights: voxelspacing must be three positive numbers (z, y, x), got {voxelspacing!r}")
    lo = min(sp)
    for m in range(1, int(max_scale) + 1):
        q = [v / lo * m for v in sp]
        w = [int(round(v)) for v in q]
        if all(abs(v - r) <= rtol * r for v, r in zip(q, w)):
            if max(w) > 255:
                raise ValueError(f"spacing_weights: voxelspacing {tuple(sp)} needs the weights {tuple(w)}, above the device's 255")
            return tuple(w), lo / m
    raise ValueError(f"spacing_weights: no scale m <= {max_scale} makes voxelspacing {tuple(sp)} / {lo} integer within {rtol}")


def volume_metrics(pred, gt, voxelspacing=None, by_class=False, n_classes=1):
    """medpy's binary.dc / jc / hd / hd95 / asd / assd (what the reference's test() prints per slice, train.py:306-325) per
    CASE, on volumes and in the units of `voxelspacing` (z, y, x; None: voxels) -> dict of float64 [N,K] arrays `dc`, `jc`,
    `hd`, `hd95`, `asd`, `assd`.  pred / gt: HIP tensors [N,(K,)D,H,W], or class maps [N,D,H,W] with by_class, as
    ustrun.functional.surface_metrics_3d takes them.  Counts (dice_counts) and the exact integer records come from the device;
    here: distances = unit * sqrt(d2) (spacing_weights), the percentile with `surface_from_records`' arithmetic, hd = the
    larger of the two directions' maxima, asd = the prediction's mean, assd = the mean of both directions' means.
    Empty prediction: 100 for the four distances (train.py:313-315); empty ground truth: EmptyGroundTruth."""
    from ustrun import functional as F
    weights, unit = ((1, 1, 1), 1.0) if voxelspacing is None else spacing_weights(voxelspacing)
    if by_class:
        cp, cg = pred, gt
    else:                                                  # dice_counts with HW := D H W: planes [N,K,DHW,1]
        K = pred.shape[1] if pred.dim() == 5 else 1
        cp, cg = pred.reshape(pred.shape[0], K, -1, 1), gt.reshape(gt.shape[0], K, -1, 1)
    cnt = np.asarray(_np(F.dice_counts(cp, cg, by_class=by_class, n_classes=n_classes)), dtype=np.int64)
    rec = np.ascontiguousarray(_np(F.surface_metrics_3d(pred, gt, by_class=by_class, n_classes=n_classes, weights=weights)),
                               dtype=np.int32)
    s, g, i = cnt[..., 0], cnt[..., 1], cnt[..., 2]
    if (g == 0).any():
        raise EmptyGroundTruth(*np.argwhere(g == 0)[0], "volume_metrics: ")
    dc = np.where(s + g > 0, 2.0 * i / np.maximum(s + g, 1), 0.0)
    jc = i / (s + g - i).astype(np.float64)
    nbp, nbg = rec[..., 0].astype(np.int64), rec[..., 1].astype(np.int64)
    sums = np.ascontiguousarray(rec[..., 6:10]).view(np.float64)
    pos = 0.95 * (nbp + nbg - 1).astype(np.float64)
    t = pos - np.floor(pos)
    a, b = unit * np.sqrt(rec[..., 2].astype(np.float64)), unit * np.sqrt(rec[..., 3].astype(np.float64))
    hd95 = np.where(t >= 0.5, b - (b - a) * (1 - t), a + (b - a) * t)          # numpy's _lerp, as surface_from_records
    hd = unit * np.sqrt(np.maximum(rec[..., 4], rec[..., 5]).astype(np.float64))
    asd = unit * sums[..., 0] / np.maximum(nbp, 1)
    assd = (asd + unit * sums[..., 1] / np.maximum(nbg, 1)) / 2.0
    empty = s == 0
    out = {"dc": dc, "jc": jc}
    for name, v in (("hd", hd), ("hd95", hd95), ("asd", asd), ("assd", assd)):
        out[name] = np.where(empty, EMPTY_PRED_VALUE, v)
    return out


def distance_transform(bitmap):
    """Euclidean distance from every pixel of bitmap [B,H,W] to the nearest true pixel of its plane (0 on true pixels, inf over
    a plane without one), from the exact integer squared distances of ustrun.functional.signed_dist2.
      numpy in -> float64 out, the square root taken in float64 of the exact integer;  HIP tensor in -> float32 HIP tensor out.
    This is deliberately the exact transform and NOT what the reference's function of this name returns: its square root
    (utils/metrics.py:69) sits inside the column loop, so the whole plane is rooted once per column and every finite value
    ends at 1.0 -- on a 2 x 24 x 40 batch its result is off the true transform by up to 19 pixels."""
    import torch
    from ustrun import functional as F
    if len(bitmap.shape) != 3:
        raise ValueError(f"distance_transform: bitmap must be [B,H,W], got {tuple(bitmap.shape)}")
    if torch.is_tensor(bitmap):
        if not bitmap.is_cuda:
            raise TypeError("distance_transform: a tensor must live on the device (pass a numpy array for host data)")
        s2, _ = F.signed_dist2((bitmap != 0).float())
        d = s2[:, 0].clamp_min(0).double().sqrt().float()        # d2 < 2^21: rounding the f64 root once is the correctly rounded f32 root
        return torch.where(s2[:, 0] == F.DIST_NONE, torch.full_like(d, float("inf")), d)
    s2, _ = F.signed_dist2(torch.from_numpy((np.asarray(bitmap) != 0).astype(np.float32)).cuda())
    s2 = s2.cpu().numpy()[:, 0]
    return np.where(s2 == F.DIST_NONE, np.inf, np.sqrt(np.maximum(s2, 0).astype(np.float64)))


# ---- the label-map losses and metrics of the reference's utils/metrics.py:13-47,72-111,233-266 (ustrun.functional, csrc/labelmap.hip)
def _labels_on_device(x):
    """numpy or tensor label map -> (HIP tensor of int64 or float32 class indices, came from numpy)"""
    import torch
    is_np = not torch.is_tensor(x)
    t = torch.from_numpy(np.ascontiguousarray(x)) if is_np else x
    if t.dtype not in (torch.int64, torch.float32):
        t = t.float() if t.is_floating_point() else t.long()
    return t.cuda(), is_np


def confusion_counts(pred, gt, n_classes, who):
    """[N,K,K] int64 numpy confusion matrices (row = gt, column = pred) of two label batches, counted on the device; this waits
    for the result.  ValueError if a label of either map lies outside [0, n_classes)."""
    from ustrun import functional as F
    p, _ = _labels_on_device(pred)
    g, _ = _labels_on_device(gt)
    counts, skipped = F.confusion(p, g, n_classes)
    skipped = skipped.cpu().numpy()
    if skipped.any():
        n = int(np.flatnonzero(skipped)[0])
        raise ValueError(f"{who}: sample {n} has {int(skipped[n])} pixels whose label is not a class index in [0, {n_classes})")
    return counts.cpu().numpy().astype(np.int64)


def cal_dice(prediction, label, num=2):
    """2 |P_i & L_i| / (|P_i| + |L_i|) for the classes i = 1..num-1 over the whole batch, as a float64 array of num - 1 values
    (nan for a class absent from both, as the reference's 0 / 0), from one confusion matrix counted on the device.  This is the
    formula of utils/metrics.py:13-24 restated: the reference's own lines use np.float, which numpy no longer has."""
    p, g = np.asarray(_np(prediction)), np.asarray(_np(label))
    c = confusion_counts(p.reshape(1, -1), g.reshape(1, -1), num, "cal_dice")[0].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return 2.0 * np.diag(c)[1:] / (c.sum(0)[1:] + c.sum(1)[1:])


def dice(input, target, ignore_index=None):
    """(2 sum i t + 1) / (sum i + sum t + 1) over every element, both operands 0 where target == ignore_index
    (utils/metrics.py:36-47); a device scalar, differentiable in `input`."""
    from ustrun import functional as F
    return F.map_dice(input, target, ignore_index)


def WatershedCrossEntropy(input, target):
    """mean over N*H*W of (1 + t_0) bce(x_0, t_0) + (1 + t_1) bce(x_1, t_1) on logits and {0,1} targets [N,2,H,W]
    (utils/metrics.py:72-91).  The reference's weight, map * (1 - DT / max DT) + 1 with its own distance_transform, equals
    target + 1 wherever it is finite.  A batch with an empty plane makes the reference's weight nan over that whole plane and its
    loss nan; this function returns the finite target + 1 form there too."""
    from ustrun import functional as F
    return F.watershed_ce(input, target)


def cross_entropy2d(input, target, weight=None, size_average=False):
    """The weighted mean of nll over the pixels with target >= 0 (utils/metrics.py:93-111), divided AGAIN by their number when
    size_average: the reference divides nll_loss's mean by the count, and so does this.  weight: K device floats or None."""
    from ustrun import functional as F
    return F.ce_map(input, target, weight=weight, ignore_negative=True, by_weight=True, by_count=bool(size_average))


def dice_loss(pred, target):
    """1 - dice_coeff(pred, target) on the host (utils/metrics.py:233-239).  For a batch dice_coeff returns a list, and the
    reference's `1 - list` raises TypeError; this returns the list of 1 - v instead."""
    d = dice_coeff(pred, target)
    return [1 - v for v in d] if isinstance(d, list) else 1 - d


def DiceLoss(input, target):
    """1 - (2 sum i t + 1) / (sum i + sum t + 1) over every element (utils/metrics.py:242-255); a device scalar."""
    from ustrun import functional as F
    return 1 - F.map_dice(input, target)


def Balanced_DiceLoss(input, target):
    """Half the sum of DiceLoss over the sigmoid of channels 0 and 1 (utils/metrics.py:257-266); a device scalar."""
    from ustrun import functional as F
    return F.balanced_dice_loss(input, target)


def dice_coefficient_numpy(binary_segmentation, binary_gt_label):
    seg = _np(binary_segmentation).astype(bool)
    gt = _np(binary_gt_label).astype(bool)
    return float(dice_from_counts(seg.sum(), gt.sum(), np.logical_and(seg, gt).sum()))


def dice_coeff(pred, target, ret_arr=False):
    pred, target = _np(pred), _np(target)
    if pred.ndim == 2:
        return dice_coefficient_numpy(pred, target)
    vals = [dice_coefficient_numpy(pred[i], target[i]) for i in range(pred.shape[0])]
    if ret_arr:
        return [np.array(vals)]
    return [sum(vals) / len(vals)]


def dice_coeff_2label(pred, target, ret_arr=False):
    pred, target = _np(pred), _np(target)
    if pred.ndim == 3:
        return dice_coefficient_numpy(pred[0], target[0]), dice_coefficient_numpy(pred[1], target[1])
    cup = [dice_coefficient_numpy(pred[i, 0], target[i, 0]) for i in range(pred.shape[0])]
    disc = [dice_coefficient_numpy(pred[i, 1], target[i, 1]) for i in range(pred.shape[0])]
    if ret_arr:
        return [np.array(cup), np.array(disc)]
    return [sum(cup) / len(cup), sum(disc) / len(disc)]


def dice_coeff_3label(pred, target, ret_arr=False, multi_layer=False):
    pred, target = _np(pred), _np(target)
    if pred.ndim == 2:
        return tuple(dice_coefficient_numpy(pred == c, target == c) for c in (1, 2, 3))
    cols = [[dice_coefficient_numpy(pred[i] == c, target[i] == c) for i in range(pred.shape[0])] for c in (1, 2, 3)]
    if ret_arr:
        return [np.array(c) for c in cols]
    return [sum(c) / len(c) for c in cols]
