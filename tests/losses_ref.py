"""Torch restatement of the thirteen loss functions utils/losses.py adds beside DiceLossWithMask, written from the reference's
utils/losses.py (line numbers below are the reference's) in this project's own words.  Every function computes in the dtype of
its first argument: the GPU tests evaluate it in float64 (the expected values) and in float32 on the CPU (the yardstick of
what f32 arithmetic costs); tests/test_losses_ref_host.py pins the float32 evaluation to the reference's own results (g19).

Class axis: dim 1 for everything except `compute_kl_loss` (last dimension).  Logarithms of probabilities come from
log_softmax / logsigmoid; a KL term is 0 where the target probability is 0.
"""
import math

import torch
import torch.nn.functional as F

SMOOTH = 1e-5        # :10, :21, :171
EPS = 1e-6           # :32, :60, :272, :279


def _overlap(inter, below):
    return 1 - (2 * inter + SMOOTH) / (below + SMOOTH)


def dice_loss(score, target):
    """:8-16 -- squared sums below the line"""
    target = target.to(score.dtype)
    return _overlap((score * target).sum(), (score * score).sum() + (target * target).sum())


def dice_loss1(score, target):
    """:19-27 -- plain sums below the line"""
    target = target.to(score.dtype)
    return _overlap((score * target).sum(), score.sum() + target.sum())


def entropy_map(p):
    """:278-281"""
    return -(p * torch.log(p + EPS)).sum(dim=1, keepdim=True)


def entropy_minmization(p):
    """:271-275"""
    return entropy_map(p).squeeze(1).mean()


def entropy_loss(p, C=2):
    """:30-36 -- the reference's .cuda() constant is ln C"""
    return entropy_minmization(p) / math.log(C)


def entropy_loss_map(p, C=2):
    """:59-62"""
    return entropy_map(p) / math.log(C)


def _probs(x, sigmoid):
    """probabilities and their logarithms across dim 1"""
    if sigmoid:
        return torch.sigmoid(x), F.logsigmoid(x)
    return F.softmax(x, dim=1), F.log_softmax(x, dim=1)


def softmax_dice_loss(input_logits, target_logits):
    """:39-56 -- dice_loss1 per class on the two softmaxes, mean over the classes"""
    pa, pb = F.softmax(input_logits, dim=1), F.softmax(target_logits, dim=1)
    K = input_logits.shape[1]
    return sum(dice_loss1(pa[:, k], pb[:, k]) for k in range(K)) / K


def softmax_mse_loss(input_logits, target_logits, sigmoid=False):
    """:65-82 -- the map, no reduction"""
    pa, pb = _probs(input_logits, sigmoid)[0], _probs(target_logits, sigmoid)[0]
    return (pa - pb) ** 2


def _kl_terms(la, pb, lb):
    return torch.where(pb > 0, pb * (lb - la), torch.zeros_like(pb))


def softmax_kl_loss(input_logits, target_logits, sigmoid=False):
    """:85-104 -- F.kl_div(log pa, pb, reduction='mean'): the mean over every element"""
    la = _probs(input_logits, sigmoid)[1]
    pb, lb = _probs(target_logits, sigmoid)
    return _kl_terms(la, pb, lb).mean()


def symmetric_mse_loss(input1, input2):
    """:107-116"""
    return ((input1 - input2) ** 2).mean()


def focal_loss(input, target, gamma=2, alpha=None, size_average=True, detach=True):
    """FocalLoss :119-153.  alpha: None, a number a (the table [a, 1 - a]) or a per-class list.  detach=True is the reference:
    pt inside (1 - pt)^gamma is a constant of the gradient (:141); detach=False differentiates it too (what the tests use to
    show that the two gradients differ)."""
    if input.dim() > 2:
        input = input.reshape(input.shape[0], input.shape[1], -1).transpose(1, 2).reshape(-1, input.shape[1])      # :131-135
    target = target.reshape(-1, 1)
    logpt = F.log_softmax(input, dim=1).gather(1, target).reshape(-1)
    pt = logpt.detach().exp() if detach else logpt.exp()
    if alpha is not None:
        table = [alpha, 1 - alpha] if isinstance(alpha, (float, int)) else list(alpha)
        logpt = logpt * torch.tensor(table, dtype=input.dtype)[target.reshape(-1)]
    loss = -(1 - pt) ** gamma * logpt
    return loss.mean() if size_average else loss.sum()


def class_dice_loss(inputs, target, n_classes, weight=None, softmax=False):
    """DiceLoss.forward :179-192 -- target [N,1,...] class indices, one-hot by equality, dice_loss per class, / n_classes"""
    if softmax:
        inputs = torch.softmax(inputs, dim=1)
    onehot = torch.cat([target == k for k in range(n_classes)], dim=1).to(inputs.dtype)
    assert inputs.size() == onehot.size(), "predict & target shape do not match"
    weight = [1] * n_classes if weight is None else weight
    return sum(dice_loss(inputs[:, k], onehot[:, k]) * weight[k] for k in range(n_classes)) / n_classes


def compute_kl_loss(p, q):
    """:284-295 -- both directions over the last dimension, each a mean over every element, halved"""
    lp, lq = F.log_softmax(p, dim=-1), F.log_softmax(q, dim=-1)
    return (_kl_terms(lp, lq.exp(), lq).mean() + _kl_terms(lq, lp.exp(), lp).mean()) / 2


# ---- the cases the goldens (tools/gen_losses_goldens.py -> g19_losses_rest.npz) and the tests walk ---------------------------------
UP = 0.7
KS = (2, 4)
_ALPHA8, _WEIGHT8 = [0.3, 0.9, 0.5, 1.2, 0.7, 1.1, 0.2, 0.8], [0.4, 1.6, 1.0, 0.25, 0.5, 2.0, 1.5, 0.75]
ALPHA_LIST = {K: _ALPHA8[:K] for K in range(1, 9)}          # per-class tables of the focal / Dice cases
WEIGHT = {K: _WEIGHT8[:K] for K in range(1, 9)}


class Names:
    """the restatement under the reference's names, for `cases`"""
    dice_loss, dice_loss1, softmax_dice_loss = staticmethod(dice_loss), staticmethod(dice_loss1), staticmethod(softmax_dice_loss)
    softmax_mse_loss, softmax_kl_loss = staticmethod(softmax_mse_loss), staticmethod(softmax_kl_loss)
    symmetric_mse_loss, compute_kl_loss = staticmethod(symmetric_mse_loss), staticmethod(compute_kl_loss)
    entropy_minmization, entropy_map = staticmethod(entropy_minmization), staticmethod(entropy_map)

    @staticmethod
    def FocalLoss(gamma=2, alpha=None, size_average=True):
        return lambda x, t: focal_loss(x, t, gamma, alpha, size_average)

    @staticmethod
    def DiceLoss(n):
        return lambda x, t, weight=None, softmax=False: class_dice_loss(x, t, n, weight, softmax)


def cases(K, M):
    """name -> (function of (x, y), first argument, second argument, differentiable in the second, upstream map or None).
    M: a module with the reference's names (the reference itself, or an adapter over tests/losses_ref.py)."""
    c = {
        "dice_loss": (M.dice_loss, "p", "hot", False, None),
        "dice_loss1": (M.dice_loss1, "p", "hot", False, None),
        "softmax_dice_loss": (M.softmax_dice_loss, "a", "b", True, None),
        "softmax_mse_loss": (M.softmax_mse_loss, "a", "b", True, "gm"),
        "softmax_mse_loss_sig": (lambda x, y: M.softmax_mse_loss(x, y, sigmoid=True), "a", "b", True, "gm"),
        "softmax_kl_loss": (M.softmax_kl_loss, "a", "b", True, None),
        "softmax_kl_loss_sig": (lambda x, y: M.softmax_kl_loss(x, y, sigmoid=True), "a", "b", True, None),
        "symmetric_mse_loss": (M.symmetric_mse_loss, "a", "b", True, None),
        "focal": (lambda x, t: M.FocalLoss()(x, t), "a", "idx", False, None),
        "focal_g1p5_list_sum": (lambda x, t: M.FocalLoss(gamma=1.5, alpha=ALPHA_LIST[K], size_average=False)(x, t), "a", "idx", False, None),
        "dice_class": (lambda x, t: M.DiceLoss(K)(x, t), "p", "idx", False, None),
        "dice_class_w_softmax": (lambda x, t: M.DiceLoss(K)(x, t, weight=WEIGHT[K], softmax=True), "a", "idx", False, None),
        "entropy_minmization": (lambda x, _: M.entropy_minmization(x), "p", "idx", False, None),
        "entropy_map": (lambda x, _: M.entropy_map(x), "p", "idx", False, "gm1"),
        "compute_kl_loss": (M.compute_kl_loss, "ra", "rb", True, None),
        "compute_kl_loss_4d": (M.compute_kl_loss, "a", "b", True, None),
    }
    if K == 2:
        c["focal_alpha_float"] = (lambda x, t: M.FocalLoss(gamma=2, alpha=0.25)(x, t), "a", "idx", False, None)
    return c


def evaluate(case, z, dtype=torch.float32, device="cpu"):
    """-> value, gradient of the first argument, gradient of the second (or None), all detached; z: name -> CPU tensor"""
    fn, xa, xb, both, up = case
    x = z[xa].to(device=device, dtype=dtype).clone().requires_grad_(True)
    y = z[xb].to(device)
    if y.is_floating_point():
        y = y.to(dtype).clone().requires_grad_(both)
    v = fn(x, y)
    ((v * z[up].to(device=device, dtype=dtype)).sum() if up else v * UP).backward()
    return v.detach(), x.grad, (y.grad if both else None)
