"""Binary Dice metrics (host side) -- same surface as the reference's utils/metrics.py:114-231.

`dice_coefficient_numpy` is (2I+1)/(1.001+S+G), 0.0 when both masks are empty.  The per-sample
overlap counts can also come from the device (ustrun.functional.dice_counts): `dice_from_counts`
applies the same formula to them, so the training step needs one small D2H copy instead of moving
whole masks to the host.

`surface_from_records` is the host part of the medpy metrics the reference's test() prints beside the Dice
(binary.dc / jc / hd95 / asd, train.py:306-325): the device (ustrun.functional.surface_metrics) delivers, per sample and
part, the border sizes, the two integer order statistics of the squared surface distances and the sum of the
prediction's distances; the square roots, numpy's linear percentile and the reference's empty-mask rules are applied here.

`distance_transform` is the Euclidean distance transform utils/metrics.py:52-70 means to be, computed on the device.
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
