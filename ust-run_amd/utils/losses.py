"""Loss modules of the hot path -- MI355X build.

DiceLossWithMask keeps the reference's constructor and forward signature
(utils/losses.py:194-268); on HIP tensors it evaluates through ustrun_seg_loss_fwd/_bwd (the two
mode combinations the step uses, fused with their CE / BCE pass) or ustrun_dice_fwd/_bwd (every
other combination: class weights, sigmoid per class, softmax + multi, raw inputs).
The SSL4MIS toolkit of the reference's losses.py (:8-192, :271-295) -- consistency, entropy, focal and Dice terms between
full-resolution logit maps -- keeps the reference's names, signatures and defaults and evaluates through csrc/consistency.hip
(ustrun.functional): fused, one pass over the operands per direction, scalar results left on the device.  Every function is
differentiable as the reference's CODE is (the pairwise ones in BOTH arguments, whatever its docstrings say); `dice_loss`,
`dice_loss1`, `DiceLoss` and `FocalLoss` in their first argument only.  Trailing dimensions beyond two (3-D volumes) count as
pixels.  Classes: at most 8 (`compute_kl_loss`: any).

Where this differs from the reference: `softmax_kl_loss(..., sigmoid=True)` takes log pa from a log-sigmoid of the logits, so
where an f32 sigmoid rounds to 0 the reference's `log(sigmoid(x))` is -inf and the value here is finite.
"""
import math

import torch
import torch.nn as nn

_NO_CPU = "ust-run_amd runs on MI355X (HIP) tensors only; there is no CPU fallback."


def _hip(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(_NO_CPU)


def _no_target_grad(target, who):
    if target.requires_grad:
        raise RuntimeError(f"{who} is differentiable in its first argument only; detach the target")


def dice_loss(score, target):
    from ustrun import functional as F
    _hip(score, target)
    _no_target_grad(target, "dice_loss")
    return F.pair_loss(score, target, "dice_sq")


def dice_loss1(score, target):
    from ustrun import functional as F
    _hip(score, target)
    _no_target_grad(target, "dice_loss1")
    return F.pair_loss(score, target, "dice")


def entropy_loss(p, C=2):
    from ustrun import functional as F
    _hip(p)
    return F.entropy(p, 1.0 / math.log(C), mean=True)


def softmax_dice_loss(input_logits, target_logits):
    from ustrun import functional as F
    _hip(input_logits, target_logits)
    return F.consistency(input_logits, target_logits, "softmax", "soft_dice")


def entropy_loss_map(p, C=2):
    from ustrun import functional as F
    _hip(p)
    return F.entropy(p, 1.0 / math.log(C), mean=False)


def softmax_mse_loss(input_logits, target_logits, sigmoid=False):
    """The elementwise map (pa - pb)^2, not a scalar (losses.py:81-82)."""
    from ustrun import functional as F
    _hip(input_logits, target_logits)
    return F.consistency(input_logits, target_logits, "sigmoid" if sigmoid else "softmax", "mse_map")


def softmax_kl_loss(input_logits, target_logits, sigmoid=False):
    """F.kl_div(..., reduction='mean') (losses.py:102): the sum divided by the element count, classes included."""
    from ustrun import functional as F
    _hip(input_logits, target_logits)
    return F.consistency(input_logits, target_logits, "sigmoid" if sigmoid else "softmax", "kl_mean")


def symmetric_mse_loss(input1, input2):
    from ustrun import functional as F
    _hip(input1, input2)
    assert input1.size() == input2.size()
    return F.pair_loss(input1, input2, "mse")


class FocalLoss(nn.Module):
    def __init__(self, gamma=2, alpha=None, size_average=True):
        super(FocalLoss, self).__init__()
        self.gamma, self.size_average = gamma, size_average
        # a number a stands for the two-class table [a, 1 - a], a list holds one weight per class (losses.py:124-127); kept as a
        # float tensor on the host, as the reference's attribute is
        table = [alpha, 1 - alpha] if isinstance(alpha, (float, int)) else alpha
        self.alpha = torch.tensor(table, dtype=torch.float32) if isinstance(table, list) else table

    def forward(self, input, target):
        """input [N,K,...] or [M,K]; target int64 class indices [N,...] or [N,1,...] ([M] for 2-D input)."""
        from ustrun import functional as F
        _hip(input, target)
        _no_target_grad(target, "FocalLoss")
        alpha = None if self.alpha is None else self.alpha.tolist()       # a host table from the constructor: no device read
        return F.focal(input, target, self.gamma, alpha, self.size_average)


class DiceLoss(nn.Module):
    def __init__(self, n_classes):
        super(DiceLoss, self).__init__()
        self.n_classes = n_classes

    def forward(self, inputs, target, weight=None, softmax=False):
        from ustrun import functional as F
        _hip(inputs, target)
        _no_target_grad(target, "DiceLoss")
        # losses.py:182-185: the one-hot of `target` (n_classes planes, concatenated over dim 1) must have the shape of `inputs`
        if target.dim() != inputs.dim() or target.shape[1] != 1 or target.shape[0] != inputs.shape[0] or \
                tuple(target.shape[2:]) != tuple(inputs.shape[2:]) or inputs.shape[1] != self.n_classes:
            raise AssertionError("predict & target shape do not match")
        if weight is not None and len(weight) < self.n_classes:
            raise IndexError("weight needs one entry per class")
        return F.class_dice(inputs, target, "softmax" if softmax else "none", None if weight is None else list(weight)[:self.n_classes])



class DiceLossWithMask(nn.Module):
    def __init__(self, n_classes):
        super(DiceLossWithMask, self).__init__()
        self.n_classes = n_classes

    def forward(self, inputs, target, mask=None, weight=None, softmax=False, sigmoid=False, multi=False):
        from ustrun import functional as F
        if sigmoid and softmax:
            assert (0)
        if not inputs.is_cuda:
            raise RuntimeError("ust-run_amd runs on MI355X (HIP) tensors only; there is no CPU fallback.")
        unit = weight is None or all(w == 1 for w in weight)
        # the two combinations the reference's step evaluates (train.py:515-521,817,830-836): fused with their CE / BCE pass
        if softmax and not multi and unit:
            _, dice = F.seg_loss(inputs, target.squeeze(1), mask, "softmax", ce_weight=0.0)
            return dice
        if sigmoid and multi:
            _, dice = F.seg_loss(inputs, target.squeeze(1), mask, "sigmoid", ce_weight=0.0)
            return dice
        # every other combination of the reference signature (losses.py:236-268): ustrun_dice_fwd/_bwd
        if sigmoid:
            target = target.squeeze(1)                                   # losses.py:241
        act = "sigmoid" if sigmoid else ("softmax" if softmax else "none")
        if not multi:
            # losses.py:250-253: the one-hot of `target` (concatenated over dim 1) must have the shape of `inputs`
            if target.dim() != inputs.dim() or target.shape[1] != 1 or target.shape[0] != inputs.shape[0] or \
                    tuple(target.shape[2:]) != tuple(inputs.shape[2:]):
                raise AssertionError("predict & target shape do not match")
            if weight is not None and len(weight) != self.n_classes:
                raise IndexError("weight needs one entry per class")
            if inputs.shape[1] != self.n_classes:
                raise AssertionError("predict & target shape do not match")
        return F.dice_general(inputs, target, mask, act=act, multi=multi, weight=None if multi else weight)


def entropy_minmization(p):
    from ustrun import functional as F
    _hip(p)
    return F.entropy(p, 1.0, mean=True)


def entropy_map(p):
    from ustrun import functional as F
    _hip(p)
    return F.entropy(p, 1.0, mean=False)


def compute_kl_loss(p, q):
    """Softmax over the LAST dimension (losses.py:285-288), any number of classes."""
    from ustrun import functional as F
    _hip(p, q)
    return F.row_kl(p, q)
