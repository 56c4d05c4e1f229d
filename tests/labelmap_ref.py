"""The label-map losses and metrics of csrc/labelmap.hip restated in numpy / torch on the CPU.  Everything that computes in floating
point takes a `dtype`: torch.float64 gives the expected values, torch.float32 the yardstick of what f32 arithmetic costs at the same
inputs (tests/test_gpu_labelmap.py).  tests/test_labelmap_ref_host.py pins this file to the reference's own results
(tests/golden/g21_labelmap.npz)."""
import numpy as np
import torch

UP = 0.7           # the upstream gradient the tests drive every scalar with


# ---- class-weighted cross-entropy over a label map ---------------------------------------------------------------------------
def ce_map(logits, target, weight=None, ignore_index=None, ignore_negative=False, scale=1.0, by_weight=False, by_count=False,
           dtype=torch.float64, up=UP):
    """logits [N,K,...] f32, target int64 with N*prod(...) elements -> dict of `out` (the five numbers the kernel writes, in dtype),
    `lse` [N,HW] and `grad` = d (up * loss) / d logits.  No valid pixel: the gradient is 0, the loss nan with a divisor and 0
    without."""
    N, K = logits.shape[:2]
    x = logits.detach().to(dtype).reshape(N, K, -1).requires_grad_(True)
    t = target.reshape(N, -1)
    ignored = torch.zeros_like(t, dtype=torch.bool)
    if ignore_index is not None:
        ignored |= t == ignore_index
    if ignore_negative:
        ignored |= t < 0
    in_range = (t >= 0) & (t < K)
    valid = ~ignored & in_range
    tc = t.clamp(0, K - 1)
    w = (torch.ones(K, dtype=dtype) if weight is None else weight.detach().to(dtype))[tc]
    lse = torch.logsumexp(x, dim=1)
    xt = x.gather(1, tc[:, None])[:, 0]
    zero = torch.zeros((), dtype=dtype)
    S = torch.where(valid, w * (lse - xt), zero).sum()
    W = torch.where(valid, w, zero).sum()
    cnt = valid.sum().to(dtype)
    loss = scale * S
    if by_weight:
        loss = loss / W
    if by_count:
        loss = loss / cnt
    if int(cnt) == 0:
        grad = torch.zeros_like(x)
    else:
        grad, = torch.autograd.grad(loss * up, x)
    out = torch.stack([loss.detach(), S.detach(), W, cnt, (~ignored & ~in_range).sum().to(dtype)])
    return {"out": out, "lse": lse.detach(), "grad": grad.reshape(logits.shape), "valid": valid}


# ---- confusion matrices and the three numbers that come from them ------------------------------------------------------------
def confusion(pred, gt, K, ignore_index=None):
    """numpy label maps [N,...] (any integer or float dtype) -> (counts int32 [N,K,K] with row = gt and column = pred, skipped
    int32 [N]); a float label that is no integer is out of range"""
    p, g = np.asarray(pred).reshape(len(pred), -1), np.asarray(gt).reshape(len(gt), -1)
    whole = lambda a: np.where(np.isfinite(a) & (a == np.floor(a)), a, -1).astype(np.int64) if a.dtype.kind == "f" else a.astype(np.int64)
    p, g = whole(p), whole(g)
    skip = (p < 0) | (p >= K) | (g < 0) | (g >= K)
    if ignore_index is not None:
        skip |= g == ignore_index
    counts = np.zeros((len(p), K, K), np.int32)
    for n in range(len(p)):
        keep = ~skip[n]
        counts[n] = np.bincount(g[n][keep] * K + p[n][keep], minlength=K * K).reshape(K, K)
    return counts, skip.sum(1).astype(np.int32)


def iou_from_counts(counts):
    total = 0.0
    for m in np.asarray(counts, np.float64):
        inter = np.diag(m)
        union = m.sum(0) + m.sum(1) - inter
        total += float(np.mean(inter[union > 0] / union[union > 0]))
    return total


def get_dice_from_counts(counts):
    K = counts.shape[1]
    v = np.arange(K, dtype=np.int64)
    total = 0.0
    for m in np.asarray(counts, np.int64):
        total += 2.0 * int(v @ m @ v) / (int((v * v) @ m.sum(0)) + int((v * v) @ m.sum(1)))
    return total


def cal_dice_from_counts(counts):
    m = np.asarray(counts, np.float64).sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return 2.0 * np.diag(m)[1:] / (m.sum(0)[1:] + m.sum(1)[1:])


def iou_direct(pred, gt, K):
    """the intended get_iou, one compare-and-count per class and image"""
    total = 0.0
    for p, g in zip(np.asarray(pred), np.asarray(gt)):
        vals = []
        for j in range(K):
            un = int(((p == j) | (g == j)).sum())
            if un:
                vals.append(int(((p == j) & (g == j)).sum()) / un)
        total += sum(vals) / len(vals)
    return total


def get_dice_direct(pred, gt):
    total = 0.0
    for p, g in zip(np.asarray(pred).astype(np.int64), np.asarray(gt).astype(np.int64)):
        total += 2.0 * int((p * g).sum()) / int((p ** 2).sum() + (g ** 2).sum())
    return total


def cal_dice_direct(pred, gt, num):
    out = np.zeros(num - 1)
    p, g = np.asarray(pred), np.asarray(gt)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(1, num):
            a, b = (p == i).astype(np.float64), (g == i).astype(np.float64)
            out[i - 1] = 2 * np.sum(a * b) / (np.sum(a) + np.sum(b))
    return out


# ---- per-plane sums and the sigmoid-map losses on them ------------------------------------------------------------------------
def plane_sums(x, t, act="none", ignore_value=None, dtype=torch.float64):
    """x, t [N,K,...] -> [K,4] = {sum s t, sum s, sum t, sum (1 + t) bce_with_logits(x, t)} (the last 0 without the sigmoid), both
    operands 0 where t == ignore_value; differentiable in x when x is"""
    N, K = x.shape[:2]
    xx, tt = x.to(dtype).reshape(N, K, -1), t.to(dtype).reshape(N, K, -1)
    keep = torch.ones_like(tt) if ignore_value is None else (tt != ignore_value).to(dtype)
    s = torch.sigmoid(xx) if act == "sigmoid" else xx
    bce = torch.nn.functional.binary_cross_entropy_with_logits(xx, tt, reduction="none") if act == "sigmoid" else torch.zeros_like(xx)
    cols = [s * tt * keep, s * keep, tt * keep, (1 + tt) * bce * keep]
    return torch.stack([c.sum(dim=(0, 2)) for c in cols], dim=1)


def _dice1(i, a, b):
    return (2.0 * i + 1.0) / (a + b + 1.0)


def dice(x, t, ignore_index=None, dtype=torch.float64):
    s = plane_sums(x.reshape(1, 1, -1), t.reshape(1, 1, -1), "none", ignore_index, dtype)[0]
    return _dice1(s[0], s[1], s[2])


def DiceLoss(x, t, dtype=torch.float64):
    return 1 - dice(x, t, None, dtype)


def Balanced_DiceLoss(x, t, dtype=torch.float64):
    s = plane_sums(x[:, :2], t[:, :2], "sigmoid", None, dtype)
    return 0.5 * ((1 - _dice1(s[0, 0], s[0, 1], s[0, 2])) + (1 - _dice1(s[1, 0], s[1, 1], s[1, 2])))


def WatershedCrossEntropy(x, t, dtype=torch.float64):
    """the target + 1 form of the weight: finite for an empty plane, where the reference's is nan"""
    return plane_sums(x[:, :2], t[:, :2], "sigmoid", None, dtype)[:, 3].sum() / (x.shape[0] * x[0, 0].numel())


def value_and_grad(fn, x, *rest, dtype=torch.float64, up=UP, **kw):
    """(value, d (up * value) / dx) of a scalar function of x, both in dtype"""
    xx = x.detach().to(dtype).requires_grad_(True)
    v = fn(xx, *rest, dtype=dtype, **kw)
    g, = torch.autograd.grad(v * up, xx)
    return v.detach(), g


# ---- colour decoding -------------------------------------------------------------------------------------------------------
def pascal_palette():
    """the VOC colour map: bit 3j + c of class i becomes bit 7 - j of channel c"""
    out = np.zeros((21, 3), np.int64)
    for i in range(21):
        for j in range(8):
            for c in range(3):
                out[i, c] |= ((i >> (3 * j + c)) & 1) << (7 - j)
    return out


def colorize(labels, palette):
    """numpy labels [...] -> float64 [..., 3]: palette[l] / 255 inside the palette, l / 255 in every channel outside"""
    l = np.asarray(labels)
    pal = np.asarray(palette, np.float64)
    inside = (l >= 0) & (l < len(pal)) & (l == np.floor(l))
    idx = np.where(inside, l, 0).astype(np.int64)
    return np.where(inside[..., None], pal[idx], l[..., None].astype(np.float64)) / 255.0


def encode_segmap(mask):
    m = np.asarray(mask).astype(int)
    out = np.zeros(m.shape[:2], int)
    for i, c in enumerate(pascal_palette()):
        out[(m == c).all(-1)] = i
    return out
