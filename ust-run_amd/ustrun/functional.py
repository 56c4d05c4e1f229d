"""Python wrappers of the loss / pseudo-label / target-mixing / optimizer entry points."""
from __future__ import annotations

import torch

from . import _lib as L
from .engine import stream_ptr

_MODE = {"softmax": L.LOSS_SOFTMAX, "sigmoid": L.LOSS_SIGMOID}


def _f32c(t, name):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a float32 HIP tensor, got {t.dtype} on {t.device}")
    return t.contiguous()


def _shape(logits):
    N, K = logits.shape[:2]
    HW = logits[0, 0].numel()
    return N, K, HW


def _check_targets(logits, target, mask, mode):
    N, K, HW = _shape(logits)
    if mode == "softmax":
        if target.dtype != torch.int64 or target.numel() != N * HW:
            raise RuntimeError(f"softmax target must be int64 [N,H,W], got {target.dtype} {tuple(target.shape)}")
        if mask is not None and mask.numel() != N * HW:
            raise RuntimeError(f"softmax mask must have N*H*W elements, got {tuple(mask.shape)}")
    else:
        if target.dtype != torch.float32 or target.numel() != N * K * HW:
            raise RuntimeError(f"sigmoid target must be float32 [N,K,H,W], got {target.dtype} {tuple(target.shape)}")
        if mask is not None and mask.numel() != N * K * HW:
            raise RuntimeError(f"sigmoid mask must have N*K*H*W elements, got {tuple(mask.shape)}")


def seg_loss_fwd(logits, target, mask, mode):
    """-> out tensor: [0]=ce mean, [1]=dice, [2:]=reduced sums kept for the backward."""
    lib = L.lib()
    logits = _f32c(logits, "logits")
    target = target.contiguous()
    mask = None if mask is None else _f32c(mask, "mask")
    _check_targets(logits, target, mask, mode)
    N, K, HW = _shape(logits)
    out = torch.empty(4 + 3 * K, dtype=torch.float32, device=logits.device)
    nb = lib.ustrun_loss_partials_bytes(N, K, HW)
    part = torch.empty(nb // 4, dtype=torch.float32, device=logits.device)
    L.check(lib.ustrun_seg_loss_fwd(logits.data_ptr(), target.data_ptr(), L.ptr(mask), N, K, HW, _MODE[mode],
                                    out.data_ptr(), part.data_ptr(), nb, stream_ptr()), "ustrun_seg_loss_fwd")
    return out


def seg_loss_bwd(logits, target, mask, mode, sums, gscale=1.0, ce_weight=1.0, dice_weight=1.0, gdev=None, out=None):
    """out: where the gradient goes (a contiguous f32 tensor of the logits' shape, e.g. this term's slice of the batched
    passes' gradient); a new tensor otherwise."""
    lib = L.lib()
    logits = _f32c(logits, "logits")
    target = target.contiguous()
    mask = None if mask is None else _f32c(mask, "mask")
    N, K, HW = _shape(logits)
    if out is None:
        dl = torch.empty_like(logits)
    else:
        if out.shape != logits.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != logits.device:
            raise RuntimeError("seg_loss_bwd: out must be a contiguous float32 tensor of the logits' shape on their device")
        dl = out
    L.check(lib.ustrun_seg_loss_bwd(logits.data_ptr(), target.data_ptr(), L.ptr(mask), N, K, HW, _MODE[mode],
                                    sums.data_ptr(), L.ptr(gdev), float(gscale), float(ce_weight), float(dice_weight),
                                    dl.data_ptr(), stream_ptr()), "ustrun_seg_loss_bwd")
    return dl


class _SegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, mask, mode, ce_weight, dice_weight):
        out = seg_loss_fwd(logits, target, mask, mode)
        ctx.save_for_backward(logits, target, out) if mask is None else ctx.save_for_backward(logits, target, out, mask)
        ctx.cfg = (mode, ce_weight, dice_weight, mask is not None)
        return out

    @staticmethod
    def backward(ctx, gout):
        mode, cw, dw, has_mask = ctx.cfg
        saved = ctx.saved_tensors
        logits, target, out = saved[:3]
        mask = saved[3] if has_mask else None
        g = gout.contiguous()
        dl = seg_loss_bwd(logits, target, mask, mode, out, 1.0, cw, dw, gdev=g)
        return dl, None, None, None, None, None


def seg_loss(logits, target, mask, mode, ce_weight=1.0, dice_weight=1.0):
    """(ce, dice) of one loss term (train.py:816-817,829-836); differentiable w.r.t. logits."""
    out = _SegLossFn.apply(logits, target, mask, mode, float(ce_weight), float(dice_weight))
    return out[0], out[1]


_ACT = {"none": 0, "softmax": 1, "sigmoid": 2}


class _DiceFn(torch.autograd.Function):
    """DiceLossWithMask.forward in any mode combination (utils/losses.py:236-268) through ustrun_dice_fwd/_bwd."""

    @staticmethod
    def forward(ctx, logits, target, mask, act, multi, weight):
        import ctypes as C
        lib = L.lib()
        logits = _f32c(logits, "inputs")
        N, K, HW = _shape(logits)
        if multi:
            target = _f32c(target.float() if target.dtype != torch.float32 else target, "target")
        else:
            target = target.contiguous() if target.dtype == torch.int64 else _f32c(target.float(), "target")
        mask = None if mask is None else _f32c(mask.float() if mask.dtype != torch.float32 else mask, "mask")
        if target.numel() not in ((N * HW,) if not multi else (N * HW, N * K * HW)):
            raise AssertionError("predict & target shape do not match")          # losses.py:253
        if mask is not None and mask.numel() not in ((N * HW,) if not multi else (N * HW, N * K * HW)):
            raise RuntimeError(f"mask of {tuple(mask.shape)} does not match inputs {tuple(logits.shape)}")
        tper = int(target.numel() != N * K * HW or not multi)              # one value per pixel (class index, or broadcast over classes)
        mper = int(mask is not None and (mask.numel() != N * K * HW or not multi))
        w = None if weight is None else (C.c_float * K)(*[float(v) for v in weight])
        out = torch.empty(1 + 3 * K, dtype=torch.float32, device=logits.device)
        nb = lib.ustrun_loss_partials_bytes(N, K, HW)
        part = torch.empty(nb // 4, dtype=torch.float32, device=logits.device)
        cfg = (int(target.dtype == torch.int64), tper, mper, N, K, HW, _ACT[act], int(multi))
        L.check(lib.ustrun_dice_fwd(logits.data_ptr(), target.data_ptr(), cfg[0], cfg[1], L.ptr(mask), cfg[2], N, K, HW, cfg[6], cfg[7], w,
                                    out.data_ptr(), part.data_ptr(), nb, stream_ptr()), "ustrun_dice_fwd")
        ctx.save_for_backward(logits, target, out) if mask is None else ctx.save_for_backward(logits, target, out, mask)
        ctx.cfg, ctx.w = cfg, w
        return out[0]

    @staticmethod
    def backward(ctx, g):
        lib = L.lib()
        saved = ctx.saved_tensors
        logits, target, out = saved[:3]
        mask = saved[3] if len(saved) > 3 else None
        t64, tper, mper, N, K, HW, act, multi = ctx.cfg
        g = g.contiguous().float().reshape(1)
        dl = torch.empty_like(logits)
        L.check(lib.ustrun_dice_bwd(logits.data_ptr(), target.data_ptr(), t64, tper, L.ptr(mask), mper, N, K, HW, act, multi, ctx.w,
                                    out.data_ptr(), g.data_ptr(), 1.0, dl.data_ptr(), stream_ptr()), "ustrun_dice_bwd")
        return dl, None, None, None, None, None


def dice_general(logits, target, mask=None, act="none", multi=False, weight=None):
    """One DiceLossWithMask value, differentiable w.r.t. logits.  per class (multi False): target = class indices with N*H*W
    elements; multi: target / mask with N*K*H*W elements or N*H*W (broadcast over the classes)."""
    return _DiceFn.apply(logits, target, mask, act, bool(multi), weight)


# ---- the semi-supervised loss toolkit of utils/losses.py (csrc/consistency.hip) ----------------------------------------------------
_CONS = {"mse_map": L.CONS_MSE_MAP, "kl_mean": L.CONS_KL_MEAN, "soft_dice": L.CONS_SOFT_DICE}
_PAIR = {"dice_sq": L.PAIR_DICE_SQ, "dice": L.PAIR_DICE, "mse": L.PAIR_MSE}


def _nkhw(t, name):
    """[N,K,*] -> N, K, HW with every trailing dimension (3-D volumes too) flattened into HW"""
    if t.dim() < 2:
        raise RuntimeError(f"{name}: expected [N,K,...], got {tuple(t.shape)}")
    N, K = t.shape[:2]
    return N, K, t.numel() // max(1, N * K)


def _partials(dev):
    nb = L.lib().ustrun_loss_partials_bytes(1, 1, 1)
    return torch.empty(nb // 4, dtype=torch.float32, device=dev), nb


def _upstream(g):
    return g.contiguous() if g.dtype == torch.float32 else g.float().contiguous()


class _ConsFn(torch.autograd.Function):
    """softmax_mse_loss / softmax_kl_loss / softmax_dice_loss (utils/losses.py:39-104) through ustrun_consistency_fwd/_bwd."""

    @staticmethod
    def forward(ctx, a, b, act, kind):
        lib = L.lib()
        a, b = _f32c(a, "input_logits"), _f32c(b, "target_logits")
        assert a.size() == b.size()                                          # losses.py:47,73,93
        N, K, HW = _nkhw(a, "input_logits")
        if kind == "mse_map":
            out, part, nb = torch.empty_like(a), None, 0
        else:
            out = torch.empty(L.CONS_NOUT, dtype=torch.float32, device=a.device)
            part, nb = _partials(a.device)
        L.check(lib.ustrun_consistency_fwd(a.data_ptr(), b.data_ptr(), N, K, HW, _MODE[act], _CONS[kind], out.data_ptr(), L.ptr(part), nb,
                                           stream_ptr()), "ustrun_consistency_fwd")
        ctx.save_for_backward(a, b) if kind == "mse_map" else ctx.save_for_backward(a, b, out)
        ctx.cfg = (N, K, HW, act, kind)
        return out if kind == "mse_map" else out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        N, K, HW, act, kind = ctx.cfg
        a, b = ctx.saved_tensors[:2]
        sums = ctx.saved_tensors[2] if kind != "mse_map" else None
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        g = _upstream(g)
        L.check(L.lib().ustrun_consistency_bwd(a.data_ptr(), b.data_ptr(), N, K, HW, _MODE[act], _CONS[kind], L.ptr(sums), g.data_ptr(),
                                               L.ptr(da), L.ptr(db), stream_ptr()), "ustrun_consistency_bwd")
        return da, db, None, None


def consistency(a, b, act="softmax", kind="mse_map"):
    """Pair consistency between two logit tensors [N,K,...], differentiable in both: kind "mse_map" -> the map (pa - pb)^2,
    "kl_mean" -> mean pb (log pb - log pa) over every element, "soft_dice" -> the class mean of the unsquared soft Dice."""
    return _ConsFn.apply(a, b, act, kind)


class _EntropyFn(torch.autograd.Function):
    """entropy_loss / entropy_loss_map / entropy_minmization / entropy_map (utils/losses.py:30-36,59-62,271-281)."""

    @staticmethod
    def forward(ctx, p, factor, mean):
        p = _f32c(p, "p")
        N, K, HW = _nkhw(p, "p")
        if mean:
            out = torch.empty(1, dtype=torch.float32, device=p.device)
            part, nb = _partials(p.device)
        else:
            out, part, nb = torch.empty((N, 1) + tuple(p.shape[2:]), dtype=torch.float32, device=p.device), None, 0
        L.check(L.lib().ustrun_entropy_fwd(p.data_ptr(), N, K, HW, factor, int(mean), out.data_ptr(), L.ptr(part), nb, stream_ptr()),
                "ustrun_entropy_fwd")
        ctx.save_for_backward(p)
        ctx.cfg = (N, K, HW, factor, int(mean))
        return out[0] if mean else out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        N, K, HW, factor, mean = ctx.cfg
        p, = ctx.saved_tensors
        dp, g = torch.empty_like(p), _upstream(g)
        L.check(L.lib().ustrun_entropy_bwd(p.data_ptr(), N, K, HW, factor, mean, g.data_ptr(), dp.data_ptr(), stream_ptr()), "ustrun_entropy_bwd")
        return dp, None, None


def entropy(p, factor=1.0, mean=True):
    """-factor sum_k p_k log(p_k + 1e-6) of a probability map [N,K,...]: the mean over the pixels, or the map [N,1,...]."""
    return _EntropyFn.apply(p, float(factor), bool(mean))


class _FocalFn(torch.autograd.Function):
    """FocalLoss.forward (utils/losses.py:130-153); the modulating factor is a constant of the gradient, as there (:141)."""

    @staticmethod
    def forward(ctx, logits, target, gamma, alpha, mean):
        import ctypes as C
        logits = _f32c(logits, "input")
        N, K, HW = _nkhw(logits, "input")
        if target.dtype != torch.int64 or not target.is_cuda or target.numel() != N * HW:
            raise RuntimeError(f"FocalLoss target must be an int64 HIP tensor with N*H*W = {N * HW} elements, got {target.dtype} {tuple(target.shape)} on {target.device}")
        target = target.contiguous()
        if alpha is not None and len(alpha) < K:
            raise IndexError("alpha needs one entry per class")           # (the reference's gather fails on a class beyond the table)
        al = None if alpha is None else (C.c_float * K)(*[float(v) for v in alpha[:K]])
        out = torch.empty(1, dtype=torch.float32, device=logits.device)
        part, nb = _partials(logits.device)
        L.check(L.lib().ustrun_focal_fwd(logits.data_ptr(), target.data_ptr(), N, K, HW, gamma, al, int(mean), out.data_ptr(), part.data_ptr(),
                                         nb, stream_ptr()), "ustrun_focal_fwd")
        ctx.save_for_backward(logits, target)
        ctx.cfg = (N, K, HW, gamma, al, int(mean))
        return out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        N, K, HW, gamma, al, mean = ctx.cfg
        logits, target = ctx.saved_tensors
        dl, g = torch.empty_like(logits), _upstream(g)
        L.check(L.lib().ustrun_focal_bwd(logits.data_ptr(), target.data_ptr(), N, K, HW, gamma, al, mean, g.data_ptr(), dl.data_ptr(),
                                         stream_ptr()), "ustrun_focal_bwd")
        return dl, None, None, None, None


def focal(logits, target, gamma=2.0, alpha=None, mean=True):
    """Focal loss of logits [N,K,...] (or [M,K]) against int64 class indices; alpha: a per-class sequence or None."""
    return _FocalFn.apply(logits, target, float(gamma), None if alpha is None else tuple(alpha), bool(mean))


class _PairFn(torch.autograd.Function):
    """dice_loss / dice_loss1 / symmetric_mse_loss (utils/losses.py:8-27,107-116) through ustrun_pair_sums/_bwd."""

    @staticmethod
    def forward(ctx, a, b, kind):
        a, b = _f32c(a, "input"), _f32c(b if b.dtype == torch.float32 else b.float(), "target")
        if a.shape != b.shape:
            raise RuntimeError(f"the two operands must have one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        out = torch.empty(L.PAIR_NOUT, dtype=torch.float32, device=a.device)
        part, nb = _partials(a.device)
        L.check(L.lib().ustrun_pair_sums(a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(), part.data_ptr(), nb, stream_ptr()), "ustrun_pair_sums")
        ctx.save_for_backward(a, b, out)
        ctx.kind = kind
        return out[6 + _PAIR[kind]]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        a, b, out = ctx.saved_tensors
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        g = _upstream(g).reshape(1)
        L.check(L.lib().ustrun_pair_sums_bwd(a.data_ptr(), b.data_ptr(), a.numel(), _PAIR[ctx.kind], out.data_ptr(), g.data_ptr(), L.ptr(da),
                                             L.ptr(db), stream_ptr()), "ustrun_pair_sums_bwd")
        return da, db, None


def pair_loss(a, b, kind):
    """One scalar over two tensors of one shape: "dice_sq" (squared sums below the line), "dice" (plain sums), "mse"."""
    return _PairFn.apply(a, b, kind)


class _RowKLFn(torch.autograd.Function):
    """compute_kl_loss (utils/losses.py:284-295): softmax over the last dimension."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _f32c(a, "p"), _f32c(b, "q")
        if a.shape != b.shape or a.dim() < 1:
            raise RuntimeError(f"the two operands must have one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        C_ = a.shape[-1]
        rows = a.numel() // C_
        out = torch.empty(1, dtype=torch.float32, device=a.device)
        part, nb = _partials(a.device)
        L.check(L.lib().ustrun_row_kl_fwd(a.data_ptr(), b.data_ptr(), rows, C_, out.data_ptr(), part.data_ptr(), nb, stream_ptr()), "ustrun_row_kl_fwd")
        ctx.save_for_backward(a, b)
        ctx.cfg = (rows, C_)
        return out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        rows, C_ = ctx.cfg
        a, b = ctx.saved_tensors
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        g = _upstream(g).reshape(1)
        L.check(L.lib().ustrun_row_kl_bwd(a.data_ptr(), b.data_ptr(), rows, C_, g.data_ptr(), L.ptr(da), L.ptr(db), stream_ptr()), "ustrun_row_kl_bwd")
        return da, db


def row_kl(a, b):
    return _RowKLFn.apply(a, b)


class _ClassDiceFn(torch.autograd.Function):
    """DiceLoss.forward (utils/losses.py:179-192): the per-class Dice of ustrun_dice_* with the smoothing term as an argument."""

    @staticmethod
    def forward(ctx, logits, target, act, weight, smooth):
        import ctypes as C
        logits = _f32c(logits, "inputs")
        N, K, HW = _nkhw(logits, "inputs")
        target = target.contiguous() if target.dtype == torch.int64 else _f32c(target.float(), "target")
        w = None if weight is None else (C.c_float * K)(*[float(v) for v in weight])
        out = torch.empty(1 + 3 * K, dtype=torch.float32, device=logits.device)
        part, nb = _partials(logits.device)
        cfg = (int(target.dtype == torch.int64), N, K, HW, _ACT[act], w, smooth)
        L.check(L.lib().ustrun_dice_smooth_fwd(logits.data_ptr(), target.data_ptr(), cfg[0], 1, None, 0, N, K, HW, cfg[4], 0, w, smooth,
                                               out.data_ptr(), part.data_ptr(), nb, stream_ptr()), "ustrun_dice_smooth_fwd")
        ctx.save_for_backward(logits, target, out)
        ctx.cfg = cfg
        return out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        logits, target, out = ctx.saved_tensors
        t64, N, K, HW, act, w, smooth = ctx.cfg
        dl, g = torch.empty_like(logits), _upstream(g).reshape(1)
        L.check(L.lib().ustrun_dice_smooth_bwd(logits.data_ptr(), target.data_ptr(), t64, 1, None, 0, N, K, HW, act, 0, w, smooth,
                                               out.data_ptr(), g.data_ptr(), 1.0, dl.data_ptr(), stream_ptr()), "ustrun_dice_smooth_bwd")
        return dl, None, None, None, None


def class_dice(logits, target, act="none", weight=None, smooth=1e-5):
    """mean_k weight[k] (1 - (2 I_k + smooth) / (Z_k + Y_k + smooth)) on the one-hot of a class-index target with N*H*W elements."""
    return _ClassDiceFn.apply(logits, target, act, weight, float(smooth))


# ---- label-map losses and metrics (csrc/labelmap.hip) ---------------------------------------------------------------------------
def _label_map(t, name, numel=None):
    if not t.is_cuda or t.dtype not in (torch.int64, torch.float32):
        raise RuntimeError(f"{name}: expected an int64 or float32 HIP tensor of class indices, got {t.dtype} on {t.device}")
    if numel is not None and t.numel() != numel:
        raise RuntimeError(f"{name}: {tuple(t.shape)} does not hold {numel} labels")
    return t.contiguous()


def _ce_map_args(logits, target, weight, ignore_index, ignore_negative, scale, by_weight, by_count):
    logits = _f32c(logits, "ce_map: logits")
    N, K, HW = _nkhw(logits, "ce_map: logits")
    if target.dtype != torch.int64 or not target.is_cuda or target.numel() != N * HW:
        raise RuntimeError(f"ce_map: target must be an int64 HIP tensor with N*H*W = {N * HW} elements, got {target.dtype} {tuple(target.shape)} on {target.device}")
    if weight is not None:
        weight = _f32c(weight, "ce_map: weight")
        if weight.numel() != K:
            raise RuntimeError(f"ce_map: weight has {weight.numel()} entries for {K} classes")
    cfg = (N, K, HW, int(ignore_index is not None), int(ignore_index or 0), int(bool(ignore_negative)), float(scale), int(bool(by_weight)),
           int(bool(by_count)))
    return logits, target.contiguous(), weight, cfg


def _ce_map_run(*args):
    logits, target, weight, cfg = _ce_map_args(*args)
    N, K, HW = cfg[:3]
    out = torch.empty(L.CE_MAP_NOUT, dtype=torch.float32, device=logits.device)
    lse = torch.empty((N, HW), dtype=torch.float32, device=logits.device)
    part, nb = _partials(logits.device)
    L.check(L.lib().ustrun_ce_map_fwd(logits.data_ptr(), target.data_ptr(), L.ptr(weight), *cfg, out.data_ptr(), lse.data_ptr(), part.data_ptr(), nb,
                                      stream_ptr()), "ustrun_ce_map_fwd")
    return logits, target, weight, cfg, out, lse


def ce_map_stats(logits, target, weight=None, ignore_index=None, ignore_negative=False, scale=1.0, by_weight=False, by_count=False):
    """The forward of `ce_map` with everything it writes, outside autograd: (out, lse) with out = {loss, S = sum w[t] (lse - x_t),
    sum w[t], valid pixels, out-of-range targets} (L.CE_MAP_NOUT device floats) and lse the per-pixel log-sum-exp [N,HW]."""
    return _ce_map_run(logits.detach(), target, weight, ignore_index, ignore_negative, scale, by_weight, by_count)[4:]


class _CeMapFn(torch.autograd.Function):
    """cross_entropy2d of utils/metrics.py:93-111 and dataloaders/utils.py:128-144 through ustrun_ce_map_fwd/_bwd; the per-pixel
    log-sum-exp is saved for the backward (one float per pixel against a second read of all K planes)."""

    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, ignore_negative, scale, by_weight, by_count):
        logits, target, weight, cfg, out, lse = _ce_map_run(logits, target, weight, ignore_index, ignore_negative, scale, by_weight, by_count)
        ctx.save_for_backward(logits, target, lse, out, *(() if weight is None else (weight,)))
        ctx.cfg = cfg
        return out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        logits, target, lse, out = ctx.saved_tensors[:4]
        weight = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
        dl, g = torch.empty_like(logits), _upstream(g)
        L.check(L.lib().ustrun_ce_map_bwd(logits.data_ptr(), target.data_ptr(), L.ptr(weight), lse.data_ptr(), *ctx.cfg, out.data_ptr(), g.data_ptr(),
                                          dl.data_ptr(), stream_ptr()), "ustrun_ce_map_bwd")
        return dl, None, None, None, None, None, None, None


def ce_map(logits, target, weight=None, ignore_index=None, ignore_negative=False, scale=1.0, by_weight=False, by_count=False):
    """Class-weighted cross-entropy of logits [N,K,...] (K up to 256) against an int64 label map, differentiable in the logits:
    scale * sum w[t] (lse - x_t) over the pixels that count, divided by sum w[t] (by_weight) and / or by their number (by_count).
    A pixel does not count if t == ignore_index or, with ignore_negative, t < 0; a target outside [0,K) that is not ignored adds
    nothing (ce_map_stats reports how many there were).  weight: K device floats.  No valid pixel: nan with a divisor, else 0."""
    return _CeMapFn.apply(logits, target, weight, ignore_index, bool(ignore_negative), float(scale), bool(by_weight), bool(by_count))


def confusion(pred, gt, n_classes, ignore_index=None):
    """Confusion matrices of two label maps [N,...] (int64 or float32 class indices): (counts int32 [N,K,K] with row = gt and
    column = pred, skipped int32 [N] = pixels whose gt is ignore_index or where either label is outside [0,K)).  K up to 32."""
    N = pred.shape[0]
    pred = _label_map(pred, "confusion: pred")
    gt = _label_map(gt, "confusion: gt", pred.numel())
    K = int(n_classes)
    counts = torch.empty((N, max(K, 0), max(K, 0)), dtype=torch.int32, device=pred.device)
    skipped = torch.empty(N, dtype=torch.int32, device=pred.device)
    L.check(L.lib().ustrun_confusion(pred.data_ptr(), gt.data_ptr(), int(pred.dtype == torch.int64), int(gt.dtype == torch.int64), N, K,
                                     pred.numel() // max(N, 1), int(ignore_index is not None), int(ignore_index or 0), counts.data_ptr(),
                                     skipped.data_ptr(), stream_ptr()), "ustrun_confusion")
    return counts, skipped


class _PlaneSumsFn(torch.autograd.Function):
    """ustrun_plane_sums_fwd/_bwd: the sums are linear in s and in the weighted BCE, so any loss built on them with torch's scalar
    operators gets its gradient from the three coefficients per plane that autograd hands back."""

    @staticmethod
    def forward(ctx, x, t, act, ignore_value):
        x, t = _f32c(x, "plane_sums: input"), _f32c(t, "plane_sums: target")
        if x.shape != t.shape:
            raise RuntimeError(f"plane_sums: input {tuple(x.shape)} and target {tuple(t.shape)} differ")
        N, K, HW = _nkhw(x, "plane_sums: input")
        out = torch.empty((K, 4), dtype=torch.float32, device=x.device)
        part, nb = _partials(x.device)
        ctx.cfg = (N, K, HW, _MODE["sigmoid"] if act == "sigmoid" else _MODE["softmax"], int(ignore_value is not None), float(ignore_value or 0.0))
        L.check(L.lib().ustrun_plane_sums_fwd(x.data_ptr(), t.data_ptr(), *ctx.cfg, out.data_ptr(), part.data_ptr(), nb, stream_ptr()),
                "ustrun_plane_sums_fwd")
        ctx.save_for_backward(x, t)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, t = ctx.saved_tensors
        g = _upstream(g)
        coef = torch.stack((g[:, 0], g[:, 1], g[:, 3]), dim=1).contiguous()          # d loss / d {sum s t, sum s, sum (1 + t) bce} per plane
        dx = torch.empty_like(x)
        L.check(L.lib().ustrun_plane_sums_bwd(x.data_ptr(), t.data_ptr(), *ctx.cfg, coef.data_ptr(), dx.data_ptr(), stream_ptr()),
                "ustrun_plane_sums_bwd")
        return dx, None, None, None


def plane_sums(x, t, act="none", ignore_value=None):
    """Per class plane of x, t [N,K,...] (K up to 8), over N and the pixels: [K,4] = {sum s t, sum s, sum t, sum (1 + t) bce(x, t)}
    with s = x (act "none") or sigmoid(x) ("sigmoid"; the last column is 0 without it); where t == ignore_value both operands
    count as 0.  Differentiable in x."""
    if act not in ("none", "sigmoid"):
        raise ValueError(f"plane_sums: act {act!r} (none / sigmoid)")
    return _PlaneSumsFn.apply(x, t, act, ignore_value)


def _smooth_dice(rows, smooth=1.0):
    """[R,4] plane sums -> [R] values of (2 sum s t + smooth) / (sum s + sum t + smooth); whole rows at once: every scalar
    operator here is a launch of its own, forward and backward"""
    return (2.0 * rows[:, 0] + smooth) / (rows[:, 1] + rows[:, 2] + smooth)


def map_dice(x, t, ignore_value=None):
    """(2 sum x t + 1) / (sum x + sum t + 1) over every element (dice of utils/metrics.py:36-47; 1 - this is DiceLoss, :242-255)."""
    return _smooth_dice(plane_sums(x.reshape(1, 1, -1), t.reshape(1, 1, -1), "none", ignore_value))[0]


def balanced_dice_loss(x, t):
    """Balanced_DiceLoss (utils/metrics.py:257-266): half the sum of 1 - dice over the sigmoid of channels 0 and 1."""
    if x.shape[1] > 2:
        x, t = x[:, :2], t[:, :2]
    return 1.0 - 0.5 * _smooth_dice(plane_sums(x, t, "sigmoid")).sum()


def watershed_ce(x, t):
    """mean over N*H*W of sum_{k<2} (1 + t_k) bce_with_logits(x_k, t_k) (WatershedCrossEntropy, utils/metrics.py:72-91, with the
    weight in the form target + 1 it takes wherever the reference's is finite)."""
    if x.shape[1] > 2:
        x, t = x[:, :2], t[:, :2]
    N, K, HW = _nkhw(x, "watershed_ce: input")
    return plane_sums(x, t, "sigmoid")[:, 3].sum() / float(N * HW)


def colorize(labels, palette):
    """Label maps [N,...] (int64 or float32 HIP tensor) -> float32 [N,3,...] = palette[l] / 255 with palette a [K,3] uint8 tensor or
    array (K up to 256); a label outside [0,K) gives l / 255 in all three channels."""
    labels = _label_map(labels, "colorize: labels")
    pal = torch.as_tensor(palette)
    if pal.dim() != 2 or pal.shape[1] != 3 or pal.dtype != torch.uint8:
        raise RuntimeError(f"colorize: palette must be [K,3] uint8, got {tuple(pal.shape)} {pal.dtype}")
    pal = pal.to(labels.device).contiguous()
    N = labels.shape[0]
    out = torch.empty((N, 3) + tuple(labels.shape[1:]), dtype=torch.float32, device=labels.device)
    L.check(L.lib().ustrun_colorize(labels.data_ptr(), int(labels.dtype == torch.int64), N, labels.numel() // max(N, 1), pal.data_ptr(), pal.shape[0],
                                    out.data_ptr(), stream_ptr()), "ustrun_colorize")
    return out


def pseudo_label(logits, threshold, mode):
    """train.py:648-667.  softmax -> (label int64 [N,H,W], mask f32 [N,1,H,W]); sigmoid -> f32 [N,K,H,W] x2."""
    lib = L.lib()
    logits = _f32c(logits, "logits")
    N, K, HW = _shape(logits)
    sp = logits.shape[2:]
    if mode == "softmax":
        label = torch.empty((N,) + tuple(sp), dtype=torch.int64, device=logits.device)
        mask = torch.empty((N, 1) + tuple(sp), dtype=torch.float32, device=logits.device)
    else:
        label = torch.empty_like(logits)
        mask = torch.empty_like(logits)
    L.check(lib.ustrun_pseudo_label(logits.data_ptr(), N, K, HW, float(threshold), _MODE[mode], label.data_ptr(),
                                    mask.data_ptr(), stream_ptr()), "ustrun_pseudo_label")
    return label, mask


def mix_targets(mode, box, pl, mask, pl_w_ul, mask_w_ul, pl_w_lu, mask_w_lu, cut_label, cut_mask):
    """train.py:677-697 -> (pl_w, mask_w, pl_ul, mask_ul, pl_lu, mask_lu)."""
    lib = L.lib()
    ts = [t.contiguous() for t in (pl, mask, pl_w_ul, mask_w_ul, pl_w_lu, mask_w_lu, cut_label, cut_mask)]
    box = _f32c(box, "box")
    N = box.shape[0]
    HW = box[0].numel()
    K = mask.shape[1] if mode == "sigmoid" else 1
    want = torch.float32 if mode == "sigmoid" else torch.int64
    for t in (ts[0], ts[2], ts[4], ts[6]):
        if t.dtype != want or t.numel() != ts[0].numel():
            raise RuntimeError("mix_targets: label tensors must share dtype/shape")
    for t in (ts[1], ts[3], ts[5], ts[7]):
        if t.dtype != torch.float32 or t.numel() != ts[1].numel():
            raise RuntimeError("mix_targets: mask tensors must be float32 of one shape")
    outs = [torch.empty_like(ts[0]), torch.empty_like(ts[1]), torch.empty_like(ts[0]), torch.empty_like(ts[1]),
            torch.empty_like(ts[0]), torch.empty_like(ts[1])]
    L.check(lib.ustrun_mix_targets(_MODE[mode], N, K, HW, box.data_ptr(), *[t.data_ptr() for t in ts],
                                   *[t.data_ptr() for t in outs], stream_ptr()), "ustrun_mix_targets")
    return tuple(outs)


def box_mix(a, b, box):
    """a*(1-box) + b*box with box [N,H,W] broadcast over channels (train.py:644-646,688,691)."""
    lib = L.lib()
    a, b, box = _f32c(a, "a"), _f32c(b, "b"), _f32c(box, "box")
    N, C = a.shape[:2]
    out = torch.empty_like(a)
    L.check(lib.ustrun_box_mix(a.data_ptr(), b.data_ptr(), box.data_ptr(), N, C, a[0, 0].numel(), out.data_ptr(),
                               stream_ptr()), "ustrun_box_mix")
    return out


def row_ptrs(t):
    """Device address of every row t[i] of a contiguous tensor (for `assemble`)."""
    if not t.is_cuda or not t.is_contiguous():
        raise RuntimeError("row_ptrs: expected a contiguous HIP tensor")
    base, step = t.data_ptr(), (t[0].numel() * t.element_size() if len(t) else 0)
    return [base + i * step for i in range(len(t))]


def assemble(rows, like, HW=0, out=None):
    """One launch that builds a batch from rows scattered over the device (ustrun_assemble): `rows` = a list of
    (a, b, box) device ADDRESSES -- b = box = 0: row = the bytes at a; else the f32 CutMix composite a*(1-box) + b*box with
    box [HW] broadcast over the row's channels.  `like`: a tensor whose [0] gives the row's shape and dtype (e.g. one of the
    sources).  Replaces x[index], torch.cat and clone chains around the forwards (train.py:627,643-647,689-702,734)
    without an index tensor or an intermediate concatenation.  The caller keeps the source tensors alive until this returns
    (the launch is then ordered on the stream)."""
    lib = L.lib()
    n = len(rows)
    row_shape, row_bytes = tuple(like.shape[1:]), like[0].numel() * like.element_size()
    if out is None:
        out = torch.empty((n,) + row_shape, dtype=like.dtype, device=like.device)
    elif tuple(out.shape) != (n,) + row_shape or out.dtype != like.dtype or not out.is_contiguous():
        raise RuntimeError("assemble: out does not match the rows")
    for o in range(0, n, L.ASM_MAX):
        part = rows[o:o + L.ASM_MAX]
        tab = (L.AsmRow * len(part))()
        for i, (a, b, bx) in enumerate(part):
            tab[i].a, tab[i].b, tab[i].box = a, b or None, bx or None
        L.check(lib.ustrun_assemble(tab, len(part), row_bytes, int(HW), out.data_ptr() + o * row_bytes, stream_ptr()),
                "ustrun_assemble")
    return out


_LABEL_KIND = {"fundus": 0, "prostate": 1, "BUSI": 2, "MNMS": 3}


def decode_labels(dataset, y):
    """train.py:590-608, train_mnms.py:549-556 in one pass (ustrun_decode_labels): the loader's float label tensor ->
    fundus: float [N,2,H,W] {cup = y == 0, disc = y <= 128}; prostate / BUSI: int64 [N,H,W] foreground map; MNMS: int64
    class map from the three 255-coded channels."""
    lib = L.lib()
    y = _f32c(y, "labels")
    kind = _LABEL_KIND[dataset]
    if kind == 3:
        if y.dim() != 4 or y.shape[-1] != 3:
            raise RuntimeError(f"MNMS labels must be [N,H,W,3], got {tuple(y.shape)}")
        sp = tuple(y.shape[1:3])
    else:
        if y.dim() != 3:
            raise RuntimeError(f"{dataset} labels must be [N,H,W], got {tuple(y.shape)}")
        sp = tuple(y.shape[1:])
    N, HW = y.shape[0], sp[0] * sp[1]
    if kind == 0:
        out = torch.empty((N, 2) + sp, dtype=torch.float32, device=y.device)
    else:
        out = torch.empty((N,) + sp, dtype=torch.int64, device=y.device)
    L.check(lib.ustrun_decode_labels(y.data_ptr(), kind, N, HW, out.data_ptr(), stream_ptr()), "ustrun_decode_labels")
    return out


def region_bbox_partials(planes, H, W, out):
    """Per-block bounding rectangles of the union of the planes' non-zero pixels -> `out` (int32 [BBOX_BLOCKS,4] on the
    device: {min y, max y, min x, max x}, {H,-1,W,-1} where a block saw none); fold them with `fold_bbox` on the host."""
    import ctypes as C
    lib = L.lib()
    bits = 0
    arr = (C.c_void_p * len(planes))()
    for k, t in enumerate(planes):
        if not t.is_cuda or not t.is_contiguous() or t.numel() != H * W or t.dtype not in (torch.float32, torch.int64):
            raise RuntimeError("region_bbox: planes must be contiguous float32 / int64 HIP tensors of H*W elements")
        bits |= int(t.dtype == torch.int64) << k
        arr[k] = t.data_ptr()
    L.check(lib.ustrun_region_bbox(arr, len(planes), bits, H, W, out.data_ptr(), stream_ptr()), "ustrun_region_bbox")
    return out


def fold_bbox(partial):
    """numpy int32 [blocks,4] -> the rectangle {y0, y1, x0, x1} of train.py:242-251 (exclusive ends), or None when no pixel is set."""
    y0, y1 = int(partial[:, 0].min()), int(partial[:, 1].max())
    x0, x1 = int(partial[:, 2].min()), int(partial[:, 3].max())
    if y1 < 0:
        return None
    return (y0, y1 + 1, x0, x1 + 1)


def rect_masks(rects, H, W, device):
    """{0,1} maps [N,H,W] on the device from N host rectangles {y0,y1,x0,x1} (train.py:222-251's maps, built where
    they are used; the corners ride in the launch's arguments, so nothing waits on a copy)."""
    import numpy as np
    lib = L.lib()
    r = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 4)
    if len(r) == 0:
        raise RuntimeError("rect_masks: no rectangles")
    out = torch.empty((len(r), H, W), dtype=torch.float32, device=device)
    for o in range(0, len(r), MAX_RECTS):                 # the launch's argument block holds 64 rectangles
        part = np.ascontiguousarray(r[o:o + MAX_RECTS])
        L.check(lib.ustrun_rect_masks(part.ctypes.data, len(part), H, W, out[o:o + len(part)].data_ptr(), stream_ptr()),
                "ustrun_rect_masks")
    return out


UPLOAD_MAX = 2048
MAX_RECTS = 64


def upload_small(arr, device, dtype):
    """A few host values -> a device tensor, stream-ordered, without a copy-engine transfer or a host wait."""
    import numpy as np
    lib = L.lib()
    t = torch.from_numpy(np.ascontiguousarray(arr)).to(dtype).contiguous()
    out = torch.empty(t.shape, dtype=dtype, device=device)
    nb = t.numel() * t.element_size()
    if nb == 0:
        return out
    if nb % 4 or nb > 64 * UPLOAD_MAX:
        raise RuntimeError(f"upload_small: {nb} bytes (needs a multiple of 4, at most {64 * UPLOAD_MAX}: it is meant for a few values)")
    for o in range(0, nb, UPLOAD_MAX):                    # 2 KB per launch's argument block
        n = min(UPLOAD_MAX, nb - o)
        L.check(lib.ustrun_upload_small(out.data_ptr() + o, t.data_ptr() + o, n, stream_ptr()), "ustrun_upload_small")
    return out


def dice_counts(pred, gt, by_class=False, n_classes=1):
    """Per-sample {|pred|, |gt|, |pred&gt|} as int32 [N,K,3] (inputs of utils/metrics.py:114-146)."""
    lib = L.lib()
    pred, gt = pred.contiguous(), gt.contiguous()
    N = pred.shape[0]
    if by_class:
        K, HW = n_classes, pred[0].numel()
    else:
        K = pred.shape[1] if pred.dim() == 4 else 1
        HW = pred[0].numel() // K
    counts = torch.empty((N, K, 3), dtype=torch.int32, device=pred.device)
    L.check(lib.ustrun_dice_counts(pred.data_ptr(), gt.data_ptr(), int(pred.dtype == torch.int64),
                                   int(gt.dtype == torch.int64), N, K, HW, int(by_class), counts.data_ptr(),
                                   stream_ptr()), "ustrun_dice_counts")
    return counts


SURFACE_RECORD_I32 = 6          # USTRUN_SURFACE_RECORD_BYTES / 4


def surface_metrics(pred, gt, by_class=False, n_classes=1):
    """Per (sample, part) surface-distance records as int32 [N,K,6] on the device (binary.hd95 / binary.asd of
    train.py:306-325 up to the host's part, utils.metrics.surface_from_records): {|border(pred)|, |border(gt)|, d2[k], d2[k+1]}
    and, in the last two words, the f64 sum of sqrt(d2) over the prediction's border.  pred / gt as `dice_counts` takes them,
    with the two image axes last."""
    lib = L.lib()
    pred, gt = pred.contiguous(), gt.contiguous()
    N, (H, W) = pred.shape[0], pred.shape[-2:]
    if pred.dim() < 3 or pred.shape != gt.shape:
        raise RuntimeError(f"surface_metrics: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must be equal [N,(K,)H,W]")
    for t, name in ((pred, "pred"), (gt, "gt")):
        if t.dtype not in (torch.float32, torch.int64) or not t.is_cuda:
            raise RuntimeError(f"surface_metrics: {name} must be a float32 or int64 HIP tensor, got {t.dtype} on {t.device}")
    K = n_classes if by_class else (pred.shape[1] if pred.dim() == 4 else 1)
    nb = lib.ustrun_surface_metrics_work_bytes(N, K, H, W)
    if nb < 0:
        L.check(1, "ustrun_surface_metrics_work_bytes")
    work = torch.empty(nb, dtype=torch.uint8, device=pred.device)
    out = torch.empty((N, K, SURFACE_RECORD_I32), dtype=torch.int32, device=pred.device)
    L.check(lib.ustrun_surface_metrics(pred.data_ptr(), gt.data_ptr(), int(pred.dtype == torch.int64),
                                       int(gt.dtype == torch.int64), N, K, int(by_class), H, W, work.data_ptr(), nb,
                                       out.data_ptr(), stream_ptr()), "ustrun_surface_metrics")
    return out


def post_process(pred, by_class=False, n_classes=1, fill_holes=True, min_share=(1, 5)):
    """The reference's dataloaders/utils.py:193-204 `post_processing` on every (sample, part) plane of `pred` (taken as
    `surface_metrics` takes it) -> float32 {0,1} planes [N,K,H,W] on the device (ustrun_post_process): holes filled (4-connected
    background that does not reach the image border), then every 8-connected component c with den * |c| < num * |filled plane|
    removed, min_share = (num, den); None switches the removal off.  With fill_holes=False and min_share=None the call only
    decodes `pred` to planes.  Filled parts may overlap, so the result is never a class map."""
    lib = L.lib()
    pred = pred.contiguous()
    if pred.dim() < 3 or (by_class and pred.dim() != 3):
        raise RuntimeError(f"post_process: pred {tuple(pred.shape)} must be [N,(K,)H,W], a class map [N,H,W] with by_class")
    if pred.dtype not in (torch.float32, torch.int64) or not pred.is_cuda:
        raise RuntimeError(f"post_process: pred must be a float32 or int64 HIP tensor, got {pred.dtype} on {pred.device}")
    N, (H, W) = pred.shape[0], pred.shape[-2:]
    K = n_classes if by_class else (pred.shape[1] if pred.dim() == 4 else 1)
    num, den = (0, 1) if min_share is None else (int(min_share[0]), int(min_share[1]))
    nb = lib.ustrun_post_process_work_bytes(N, K, H, W)
    if nb < 0:
        L.check(1, "ustrun_post_process_work_bytes")
    work = torch.empty(nb, dtype=torch.uint8, device=pred.device)
    out = torch.empty((N, K, H, W), dtype=torch.float32, device=pred.device)
    L.check(lib.ustrun_post_process(pred.data_ptr(), int(pred.dtype == torch.int64), N, K, int(by_class), H, W, int(bool(fill_holes)),
                                    num, den, work.data_ptr(), nb, out.data_ptr(), stream_ptr()), "ustrun_post_process")
    return out


DIST_NONE = 0x7fffffff          # USTRUN_DIST_NONE: |s2| of a pixel whose plane has no pixel of the opposite kind
PLANE_EMPTY, PLANE_MIXED, PLANE_FULL = 0, 1, 2


def _dist_planes(mask, by_class, num_classes, who):
    if not torch.is_tensor(mask) or not mask.is_cuda or mask.dtype not in (torch.float32, torch.int64):
        raise RuntimeError(f"{who}: mask must be a float32 or int64 HIP tensor, got "
                           f"{getattr(mask, 'dtype', type(mask))} on {getattr(mask, 'device', 'the host')}")
    if by_class:
        if mask.dim() != 3 or num_classes is None or int(num_classes) < 1:
            raise RuntimeError(f"{who}: by_class takes a class map [N,H,W] and num_classes >= 1, got {tuple(mask.shape)}, {num_classes}")
        K = int(num_classes)
    else:
        if mask.dim() not in (3, 4) or mask.dtype != torch.float32:
            raise RuntimeError(f"{who}: mask must be float32 planes [N,(K,)H,W] (or a class map with by_class), got "
                               f"{mask.dtype} {tuple(mask.shape)}")
        K = mask.shape[1] if mask.dim() == 4 else 1
        if num_classes is not None and int(num_classes) != K:
            raise RuntimeError(f"{who}: num_classes {num_classes} against {K} planes")
    return mask.contiguous(), mask.shape[0], K, mask.shape[-2], mask.shape[-1]


@torch.no_grad()
def signed_dist2(mask, by_class=False, num_classes=None):
    """Exact signed squared Euclidean distances of every plane of `mask` (ustrun_signed_dist2; taken as `surface_metrics` takes
    pred: float32 planes [N,(K,)H,W] binarised as != 0, or with by_class an int64 / float32 class map [N,H,W] whose plane c is
    == c + 1) -> (s2 int32 [N,K,H,W], flags int32 [N,K]) on the device: + d2 to the nearest foreground pixel at a background
    pixel, - d2 to the nearest background pixel at a foreground pixel, inside the image only (scipy's convention);
    flags 0 / 1 / 2 = empty / mixed / full plane, whose pixels hold +- DIST_NONE where no opposite kind exists.  Integer
    labels, no gradient; nothing waits for the device."""
    lib = L.lib()
    mask, N, K, H, W = _dist_planes(mask, by_class, num_classes, "signed_dist2")
    nb = lib.ustrun_signed_dist2_work_bytes(N, K, H, W)
    if nb < 0:
        L.check(1, "ustrun_signed_dist2_work_bytes")
    work = torch.empty(nb, dtype=torch.uint8, device=mask.device)
    s2 = torch.empty((N, K, H, W), dtype=torch.int32, device=mask.device)
    flags = torch.empty((N, K), dtype=torch.int32, device=mask.device)
    L.check(lib.ustrun_signed_dist2(mask.data_ptr(), int(mask.dtype == torch.int64), N, K, int(bool(by_class)), H, W,
                                    work.data_ptr(), nb, s2.data_ptr(), flags.data_ptr(), stream_ptr()), "ustrun_signed_dist2")
    return s2, flags


@torch.no_grad()
def signed_distance_map(mask, by_class=False, num_classes=None):
    """The normalised signed distance map of the reference's compute_sdf (utils/util.py:208-239) for every plane of `mask`
    (as `signed_dist2` takes it) -> (sdf float32 [N,K,H,W], flags int32 [N,K]) on the device: in [-1, 0) inside, exactly 0 on
    the inner boundary, in (0, 1] outside, -1 and +1 at the deepest pixels.  Empty planes (flag 0) are zeros as in the
    reference; full planes (flag 2), where the reference divides 0 / 0, are zeros too -- read the flags.  A ground-truth
    target: not differentiable; nothing waits for the device."""
    lib = L.lib()
    s2, flags = signed_dist2(mask, by_class, num_classes)
    N, K, H, W = s2.shape
    nb = lib.ustrun_sdf_from_dist2_work_bytes(N, K, H, W)
    if nb < 0:
        L.check(1, "ustrun_sdf_from_dist2_work_bytes")
    work = torch.empty(nb, dtype=torch.uint8, device=s2.device)
    sdf = torch.empty((N, K, H, W), dtype=torch.float32, device=s2.device)
    L.check(lib.ustrun_sdf_from_dist2(s2.data_ptr(), flags.data_ptr(), N, K, H, W, work.data_ptr(), nb, sdf.data_ptr(),
                                      stream_ptr()), "ustrun_sdf_from_dist2")
    return sdf, flags


SURFACE3D_RECORD_I32 = 10       # USTRUN_SURFACE3D_RECORD_BYTES / 4


def _axis_weights(weights, who):
    w = tuple(int(v) for v in weights)
    if len(w) != 3 or any(int(v) != v for v in weights):
        raise RuntimeError(f"{who}: weights must be three integers (wz, wy, wx), got {weights!r}")
    return w


def _dist_volumes(mask, by_class, num_classes, who):
    """`_dist_planes` with one more axis -> (mask, N, K, D, H, W)"""
    if not torch.is_tensor(mask) or not mask.is_cuda or mask.dtype not in (torch.float32, torch.int64):
        raise RuntimeError(f"{who}: mask must be a float32 or int64 HIP tensor, got "
                           f"{getattr(mask, 'dtype', type(mask))} on {getattr(mask, 'device', 'the host')}")
    if by_class:
        if mask.dim() != 4 or num_classes is None or int(num_classes) < 1:
            raise RuntimeError(f"{who}: by_class takes a class map [N,D,H,W] and num_classes >= 1, got {tuple(mask.shape)}, {num_classes}")
        K = int(num_classes)
    else:
        if mask.dim() not in (4, 5) or mask.dtype != torch.float32:
            raise RuntimeError(f"{who}: mask must be float32 volumes [N,(K,)D,H,W] (or a class map with by_class), got "
                               f"{mask.dtype} {tuple(mask.shape)}")
        K = mask.shape[1] if mask.dim() == 5 else 1
        if num_classes is not None and int(num_classes) != K:
            raise RuntimeError(f"{who}: num_classes {num_classes} against {K} volumes")
    return (mask.contiguous(), mask.shape[0], K) + tuple(mask.shape[-3:])


@torch.no_grad()
def signed_dist2_3d(mask, by_class=False, num_classes=None, weights=(1, 1, 1)):
    """Exact signed squared distances of every volume of `mask` (ustrun_signed_dist2_3d), the 3-D form of `signed_dist2` for
    the volumes compute_sdf is documented for (utils/util.py:208-217, shape = (batch_size, x, y, z)): float32 volumes
    [N,(K,)D,H,W] binarised as != 0, or with by_class an int64 / float32 class map [N,D,H,W] whose volume c is == c + 1
    -> (s2 int32 [N,K,D,H,W], flags int32 [N,K]) on the device.  d2 = wz^2 dz^2 + wy^2 dy^2 + wx^2 dx^2 with the integer
    `weights` (wz, wy, wx), each in 1..255 (unit weights: scipy.ndimage.distance_transform_edt's default, util.py:226-227;
    others: its `sampling`): + d2 to the nearest foreground voxel at a background voxel, - d2 to the nearest background voxel
    at a foreground voxel, inside the volume only; flags 0 / 1 / 2 = empty / mixed / full volume, whose voxels hold
    +- DIST_NONE where no opposite kind exists.  No gradient; nothing waits for the device."""
    lib = L.lib()
    mask, N, K, D, H, W = _dist_volumes(mask, by_class, num_classes, "signed_dist2_3d")
    wz, wy, wx = _axis_weights(weights, "signed_dist2_3d")
    nb = lib.ustrun_signed_dist2_3d_work_bytes(N, K, D, H, W)
    if nb < 0:
        L.check(1, "ustrun_signed_dist2_3d_work_bytes")
    work = torch.empty(nb, dtype=torch.uint8, device=mask.device)
    s2 = torch.empty((N, K, D, H, W), dtype=torch.int32, device=mask.device)
    flags = torch.empty((N, K), dtype=torch.int32, device=mask.device)
    L.check(lib.ustrun_signed_dist2_3d(mask.data_ptr(), int(mask.dtype == torch.int64), N, K, int(bool(by_class)), D, H, W, wz, wy,
                                       wx, work.data_ptr(), nb, s2.data_ptr(), flags.data_ptr(), stream_ptr()),
            "ustrun_signed_dist2_3d")
    return s2, flags


@torch.no_grad()
def signed_distance_map_3d(mask, by_class=False, num_classes=None):
    """The normalised signed distance map of the reference's compute_sdf (utils/util.py:208-239) for every VOLUME of `mask`
    (as `signed_dist2_3d` takes it, unit weights) -> (sdf float32 [N,K,D,H,W], flags int32 [N,K]) on the device: the
    normalisation of util.py:231-234 with the maxima over the whole volume; in [-1, 0) inside, exactly 0 on the inner boundary
    (a foreground voxel with a background 6-neighbour, util.py:228), in (0, 1] outside.  Empty and full volumes are zeros --
    read the flags.  Not differentiable; nothing waits for the device."""
    lib = L.lib()
    s2, flags = signed_dist2_3d(mask, by_class, num_classes)
    N, K, D, H, W = s2.shape
    nb = lib.ustrun_sdf_from_dist2_3d_work_bytes(N, K, D, H, W)
    if nb < 0:
        L.check(1, "ustrun_sdf_from_dist2_3d_work_bytes")
    work = torch.empty(nb, dtype=torch.uint8, device=s2.device)
    sdf = torch.empty((N, K, D, H, W), dtype=torch.float32, device=s2.device)
    L.check(lib.ustrun_sdf_from_dist2_3d(s2.data_ptr(), flags.data_ptr(), N, K, D, H, W, work.data_ptr(), nb, sdf.data_ptr(),
                                         stream_ptr()), "ustrun_sdf_from_dist2_3d")
    return sdf, flags


def surface_metrics_3d(pred, gt, by_class=False, n_classes=1, weights=(1, 1, 1)):
    """Per (case, part) surface-distance records of VOLUMES as int32 [N,K,10] on the device (ustrun_surface_metrics_3d): what
    medpy's binary.hd / hd95 / asd / assd (train.py:306-325, called there on slices) take from n-dimensional masks, up to the
    host's part (utils.metrics.volume_metrics).  pred / gt: float32 volumes [N,(K,)D,H,W] or, with by_class, class maps
    [N,D,H,W]; borders with the 6-neighbour cross, d2 with the integer axis `weights` (wz, wy, wx) in 1..255 (medpy's
    `voxelspacing` through utils.metrics.spacing_weights).  Record: {|border(pred)|, |border(gt)|, d2[k], d2[k+1], max d2 over
    border(pred), max d2 over border(gt)}, then the f64 sums of sqrt(d2) over border(pred) and over border(gt) in two words
    each."""
    lib = L.lib()
    pred, gt = pred.contiguous(), gt.contiguous()
    if pred.dim() < 4 or pred.shape != gt.shape or (by_class and pred.dim() != 4) or pred.dim() > 5:
        raise RuntimeError(f"surface_metrics_3d: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must be equal [N,(K,)D,H,W] "
                           "(a class map [N,D,H,W] with by_class)")
    for t, name in ((pred, "pred"), (gt, "gt")):
        if t.dtype not in (torch.float32, torch.int64) or not t.is_cuda:
            raise RuntimeError(f"surface_metrics_3d: {name} must be a float32 or int64 HIP tensor, got {t.dtype} on {t.device}")
    N, (D, H, W) = pred.shape[0], pred.shape[-3:]
    K = n_classes if by_class else (pred.shape[1] if pred.dim() == 5 else 1)
    wz, wy, wx = _axis_weights(weights, "surface_metrics_3d")
    nb = lib.ustrun_surface_metrics_3d_work_bytes(N, K, D, H, W)
    if nb < 0:
        L.check(1, "ustrun_surface_metrics_3d_work_bytes")
    work = torch.empty(nb, dtype=torch.uint8, device=pred.device)
    out = torch.empty((N, K, SURFACE3D_RECORD_I32), dtype=torch.int32, device=pred.device)
    L.check(lib.ustrun_surface_metrics_3d(pred.data_ptr(), gt.data_ptr(), int(pred.dtype == torch.int64),
                                          int(gt.dtype == torch.int64), N, K, int(bool(by_class)), D, H, W, wz, wy, wx,
                                          work.data_ptr(), nb, out.data_ptr(), stream_ptr()), "ustrun_surface_metrics_3d")
    return out


def post_process_3d(pred, by_class=False, n_classes=1, fill_holes=True, min_share=(1, 5), largest=False):
    """The reference's dataloaders/utils.py:193-204 `post_processing` on every (case, part) VOLUME of `pred` (taken as
    `surface_metrics_3d` takes it: float32 [N,(K,)D,H,W], or with by_class a class map [N,D,H,W]) -> float32 {0,1} volumes
    [N,K,D,H,W] on the device (ustrun_post_process_3d): holes filled (background that no path of face steps leads from to a face
    of the volume), then every 26-connected component c with den * |c| < num * |filled volume| removed, min_share = (num, den);
    None switches the removal off.  largest=True keeps only the largest component after that (ties: the one with the smallest
    voxel index).  With fill_holes=False, min_share=None and largest=False the call only decodes `pred`.  Filled parts may
    overlap, so the result is never a class map."""
    lib = L.lib()
    pred = pred.contiguous()
    if pred.dim() < 4 or (by_class and pred.dim() != 4) or pred.dim() > 5:
        raise RuntimeError(f"post_process_3d: pred {tuple(pred.shape)} must be [N,(K,)D,H,W] (a class map [N,D,H,W] with by_class)")
    if pred.dtype not in (torch.float32, torch.int64) or not pred.is_cuda:
        raise RuntimeError(f"post_process_3d: pred must be a float32 or int64 HIP tensor, got {pred.dtype} on {pred.device}")
    N, (D, H, W) = pred.shape[0], pred.shape[-3:]
    K = n_classes if by_class else (pred.shape[1] if pred.dim() == 5 else 1)
    num, den = (0, 1) if min_share is None else (int(min_share[0]), int(min_share[1]))
    nb = lib.ustrun_post_process_3d_work_bytes(N, K, D, H, W)
    if nb < 0:
        L.check(1, "ustrun_post_process_3d_work_bytes")
    work = torch.empty(nb, dtype=torch.uint8, device=pred.device)
    out = torch.empty((N, K, D, H, W), dtype=torch.float32, device=pred.device)
    L.check(lib.ustrun_post_process_3d(pred.data_ptr(), int(pred.dtype == torch.int64), N, K, int(bool(by_class)), D, H, W,
                                       int(bool(fill_holes)), num, den, int(bool(largest)), work.data_ptr(), nb, out.data_ptr(),
                                       stream_ptr()), "ustrun_post_process_3d")
    return out


METRIC_TAXICAB, METRIC_CHESSBOARD = 0, 1
MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE, MORPH_BAND = 0, 1, 2, 3, 4
MORPH_WIDTH_MAX = 4095          # no distance in a box the kernels accept exceeds 3069: every larger count gives the same answer


def _morph_box(mask, by_class, num_classes, who):
    """planes [N,K,H,W] / volumes [N,K,D,H,W], or with by_class class maps [N,H,W] / [N,D,H,W] -> (mask, N, K, rank, D, H, W)"""
    if not torch.is_tensor(mask) or not mask.is_cuda or mask.dtype not in (torch.float32, torch.int64):
        raise RuntimeError(f"{who}: mask must be a float32 or int64 HIP tensor, got "
                           f"{getattr(mask, 'dtype', type(mask))} on {getattr(mask, 'device', 'the host')}")
    if by_class:
        if mask.dim() not in (3, 4) or num_classes is None or int(num_classes) < 1:
            raise RuntimeError(f"{who}: by_class takes a class map [N,H,W] or [N,D,H,W] and num_classes >= 1, got "
                               f"{tuple(mask.shape)}, {num_classes}")
        K, rank = int(num_classes), mask.dim() - 1
    else:
        if mask.dim() not in (4, 5) or mask.dtype != torch.float32:
            raise RuntimeError(f"{who}: mask must be float32 planes [N,K,H,W] or volumes [N,K,D,H,W] (or a class map with by_class), "
                               f"got {mask.dtype} {tuple(mask.shape)}")
        K, rank = mask.shape[1], mask.dim() - 2
        if num_classes is not None and int(num_classes) != K:
            raise RuntimeError(f"{who}: num_classes {num_classes} against {K} parts")
    D = mask.shape[-3] if rank == 3 else 1
    return mask.contiguous(), mask.shape[0], K, rank, D, mask.shape[-2], mask.shape[-1]


def _metric_code(metric, who):
    codes = {"taxicab": METRIC_TAXICAB, "cityblock": METRIC_TAXICAB, "manhattan": METRIC_TAXICAB, "chessboard": METRIC_CHESSBOARD}
    if metric not in codes:
        raise RuntimeError(f"{who}: metric must be 'taxicab' (alias 'cityblock', 'manhattan') or 'chessboard', got {metric!r}")
    return codes[metric]


def _structure_code(structure, rank, who):
    """None, 1 or "cross": scipy's default generate_binary_structure(rank, 1) -> the city-block metric; the rank or "full":
    generate_binary_structure(rank, rank) -> the chessboard metric.  Nothing else is a threshold of a separable distance."""
    if structure is None or (isinstance(structure, str) and structure == "cross"):
        return METRIC_TAXICAB
    if isinstance(structure, str) and structure == "full":
        return METRIC_CHESSBOARD
    if isinstance(structure, int) and not isinstance(structure, bool):
        if structure == 1:
            return METRIC_TAXICAB
        if structure == rank:
            return METRIC_CHESSBOARD
        if rank == 3 and structure == 2:
            raise RuntimeError(f"{who}: connectivity 2 in 3-D (18 neighbours) is not built: its distance is not separable per axis; "
                               "use 1 / 'cross' (6 neighbours) or 3 / 'full' (26 neighbours)")
    raise RuntimeError(f"{who}: structure must be None, 1 or 'cross' (the cross), or {rank} or 'full' (the full structure) for rank "
                       f"{rank}; arbitrary structuring elements are not built, got {structure!r}")


@torch.no_grad()
def chamfer_distance(mask, metric="taxicab", outside=0, by_class=False, num_classes=None):
    """Exact signed chamfer distances of every plane or volume of `mask` (ustrun_chamfer_dist): float32 [N,K,H,W] / [N,K,D,H,W]
    binarised as != 0, or with by_class an int64 / float32 class map [N,H,W] / [N,D,H,W] whose part c is == c + 1
    -> (sd int32 like [N,K,...], flags int32 [N,K]) on the device.  metric 'taxicab' (city-block, L1) or 'chessboard' (L-inf):
    + d to the nearest foreground pixel at a background pixel, - d to the nearest background pixel at a foreground pixel.
    outside 0: nothing outside the box is of either kind (scipy.ndimage.distance_transform_cdt's convention); 1: the outside is
    background; 2: the outside is foreground.  flags 0 / 1 / 2 = empty / mixed / full; where no pixel of the opposite kind exists
    and `outside` supplies none, sd holds +- DIST_NONE.  No gradient; nothing waits for the device."""
    lib = L.lib()
    mask, N, K, rank, D, H, W = _morph_box(mask, by_class, num_classes, "chamfer_distance")
    code = _metric_code(metric, "chamfer_distance")
    if outside not in (0, 1, 2):
        raise RuntimeError(f"chamfer_distance: outside must be 0 (neither kind), 1 (background) or 2 (foreground), got {outside!r}")
    nb = lib.ustrun_chamfer_dist_work_bytes(N, K, rank, D, H, W)
    if nb < 0:
        L.check(1, "ustrun_chamfer_dist_work_bytes")
    work = torch.empty(nb, dtype=torch.uint8, device=mask.device)
    box = (D, H, W) if rank == 3 else (H, W)
    sd = torch.empty((N, K) + box, dtype=torch.int32, device=mask.device)
    flags = torch.empty((N, K), dtype=torch.int32, device=mask.device)
    L.check(lib.ustrun_chamfer_dist(mask.data_ptr(), int(mask.dtype == torch.int64), N, K, int(bool(by_class)), rank, D, H, W, code,
                                    int(outside), work.data_ptr(), nb, sd.data_ptr(), flags.data_ptr(), stream_ptr()),
            "ustrun_chamfer_dist")
    return sd, flags


@torch.no_grad()
def distance_transform_cdt(mask, metric="chessboard", by_class=False, num_classes=None):
    """scipy.ndimage.distance_transform_cdt(part, metric) of every plane or volume of `mask` (as `chamfer_distance` takes it), as
    int32 on the device: the distance to the nearest background pixel on the foreground, 0 on the background, and -1 everywhere
    on a part without background, which is what scipy returns for it.  Nothing waits for the device."""
    sd, flags = chamfer_distance(mask, metric, 0, by_class, num_classes)
    full = (flags == PLANE_FULL).view(flags.shape + (1,) * (sd.dim() - 2))
    return torch.where(full, torch.full_like(sd, -1), (-sd).clamp_(min=0))


def _morph(mask, op, metric, width, border_value, reduce_parts, by_class, num_classes, who):
    lib = L.lib()
    mask, N, K, rank, D, H, W = _morph_box(mask, by_class, num_classes, who)
    code = metric(rank) if callable(metric) else metric
    if int(width) != width or width < 1:
        raise RuntimeError(f"{who}: iterations / width must be an integer >= 1, got {width!r} (scipy's iterations < 1, repeating "
                           "until nothing changes, is not built)")
    if border_value not in (0, 1, False, True):
        raise RuntimeError(f"{who}: border_value must be 0 or 1, got {border_value!r}")
    width = min(int(width), MORPH_WIDTH_MAX)
    nb = lib.ustrun_morph_work_bytes(N, K, rank, D, H, W, op)
    if nb < 0:
        L.check(1, "ustrun_morph_work_bytes")
    work = torch.empty(nb, dtype=torch.uint8, device=mask.device)
    box = (D, H, W) if rank == 3 else (H, W)
    out = torch.empty(((N,) if reduce_parts else (N, K)) + box, dtype=torch.uint8, device=mask.device)
    L.check(lib.ustrun_morph(mask.data_ptr(), int(mask.dtype == torch.int64), N, K, int(bool(by_class)), rank, D, H, W, code, op,
                             width, int(border_value), int(bool(reduce_parts)), work.data_ptr(), nb, out.data_ptr(), stream_ptr()),
            "ustrun_morph")
    return out


def _binary_op(op, who):
    @torch.no_grad()
    def fn(mask, structure=None, iterations=1, border_value=0, by_class=False, num_classes=None):
        return _morph(mask, op, lambda rank: _structure_code(structure, rank, who), iterations, border_value, False, by_class,
                      num_classes, who).view(torch.bool)
    fn.__name__ = fn.__qualname__ = who
    fn.__doc__ = (f"scipy.ndimage.{who}(part, structure, iterations, border_value=border_value) of every plane or volume of `mask` "
                  "(ustrun_morph; float32 [N,K,H,W] / [N,K,D,H,W] binarised as != 0, or with by_class a class map [N,H,W] / "
                  "[N,D,H,W] whose part c is == c + 1) -> bool like [N,K,...] on the device.  structure: None, 1 or 'cross' = "
                  "generate_binary_structure(rank, 1), scipy's default; the rank or 'full' = generate_binary_structure(rank, rank); "
                  "anything else raises.  iterations >= 1 (counts past 4095 are clamped: they give the same answer).  border_value "
                  "has scipy's meaning and, as in scipy, goes to both halves of an opening or closing.  Nothing waits for the device.")
    return fn


binary_dilation = _binary_op(MORPH_DILATE, "binary_dilation")
binary_erosion = _binary_op(MORPH_ERODE, "binary_erosion")
binary_opening = _binary_op(MORPH_OPEN, "binary_opening")
binary_closing = _binary_op(MORPH_CLOSE, "binary_closing")


@torch.no_grad()
def boundary_band(mask, width=5, structure=None, reduce_parts=True, by_class=False, num_classes=None):
    """The reference's GetBoundary map (dataloaders/custom_transforms.py:630-647) of every image of `mask` (as `binary_dilation`
    takes it): per part, the pixels where the dilation and the erosion by `width` steps differ (border_value 0, as the reference
    calls scipy); reduce_parts ORs the K parts of an image (custom_transforms.py:646) -> uint8 {0,1} [N,...] on the device,
    otherwise [N,K,...].  Nothing waits for the device."""
    return _morph(mask, MORPH_BAND, lambda rank: _structure_code(structure, rank, "boundary_band"), width, 0, reduce_parts, by_class,
                  num_classes, "boundary_band")


def sgd_ema(p, g, v, t, lr, momentum, weight_decay, first, alpha, grad_scale=1.0):
    """Fused SGD(momentum, wd) step on flat f32 buffers + EMA teacher update (train.py:512,848,87-93)."""
    lib = L.lib()
    L.check(lib.ustrun_sgd_ema(p.data_ptr(), g.data_ptr(), v.data_ptr(), L.ptr(t), p.numel(), float(lr), float(momentum),
                               float(weight_decay), int(first), float(alpha), float(grad_scale), stream_ptr()),
            "ustrun_sgd_ema")


class LossScale:
    """torch.cuda.amp.GradScaler semantics (train.py:552,842-845) on the device: no step waits for the host.  `state` is the four
    floats {scale, scale, growth_tracker, found_inf} of include/ustrun.h; pass `state` as `gdev` to `seg_loss_bwd` to scale the
    backward, then call `step(...)` where the reference calls scaler.step(optimizer); scaler.update()."""

    def __init__(self, device, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.state = torch.tensor([init_scale, init_scale, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=device)
        self.growth_factor, self.backoff_factor, self.growth_interval = growth_factor, backoff_factor, growth_interval

    def step(self, p, g, v, t, lr, momentum, weight_decay, first, alpha, grad_scale=1.0):
        lib = L.lib()
        st = stream_ptr()
        L.check(lib.ustrun_amp_check(g.data_ptr(), g.numel(), self.state.data_ptr(), st), "ustrun_amp_check")
        L.check(lib.ustrun_sgd_ema_scaled(p.data_ptr(), g.data_ptr(), v.data_ptr(), L.ptr(t), p.numel(), float(lr), float(momentum),
                                          float(weight_decay), int(first), float(alpha), float(grad_scale), self.state.data_ptr(),
                                          st), "ustrun_sgd_ema_scaled")
        L.check(lib.ustrun_amp_update(self.state.data_ptr(), float(self.growth_factor), float(self.backoff_factor),
                                      int(self.growth_interval), st), "ustrun_amp_update")

    def skipped_steps(self):
        """(host read) -> (steps skipped, steps seen)"""
        s = self.state.cpu()
        return int(s[4]), int(s[5])

    def get_scale(self):
        """(host read: logging / checkpoints only)"""
        return float(self.state[0])

    def state_dict(self):
        s = self.state.cpu()
        return {"scale": float(s[0]), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": int(s[2])}

    def load_state_dict(self, sd):
        self.growth_factor, self.backoff_factor = float(sd["growth_factor"]), float(sd["backoff_factor"])
        self.growth_interval = int(sd["growth_interval"])
        self.state.copy_(torch.tensor([sd["scale"], sd["scale"], float(sd.get("_growth_tracker", 0)), 0.0, 0.0, 0.0, 0.0, 0.0]))
