"""Checkpoint I/O and meters used by the training scripts -- surface of the reference's
utils/util.py:167-183,259-297 --, the two overlay pictures of utils/util.py:346-390 that test.py --save_img
writes, and compute_sdf of utils/util.py:208-239, the signed distance map shape-aware losses regress on, computed on
the device (the rest of that file is dead code there).  state_dict keys are identical to the reference's, so
checkpoints interchange in both directions."""
import os

import numpy as np
import torch


class AverageMeter(object):
    """Computes and stores the average and current value"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def save_osmancheckpoint(epoch, ema_model, model, optimizer, best_dice, best_iter, stu_best_dice, stu_best_iter, path):
    torch.save({"epoch": epoch, "ema_state_dict": ema_model.state_dict(), "state_dict": model.state_dict(),
                "optimizer_state_dict": optimizer.state_dict(), "best_dice": best_dice, "best_iter": best_iter,
                "stu_best_dice": stu_best_dice, "stu_best_iter": stu_best_iter}, path)


def load_osmancheckpoint(path, ema_model, model, optimizer, from_ddp=False):
    ck = torch.load(path, map_location="cpu")
    ema_model.load_state_dict(ck["ema_state_dict"])
    model.load_state_dict(ck["state_dict"])
    optimizer.load_state_dict(ck["optimizer_state_dict"])
    return (ck["epoch"], ema_model, model, optimizer, ck["best_dice"], ck["best_iter"],
            ck["stu_best_dice"], ck["stu_best_iter"])


def _one_image(img, *maps):
    """The reference's argument forms for ONE image -> the batch forms of ustrun.render: img [H,W] or [C,H,W] -> f32
    [1,C,H,W]; a map [H,W] or [P,H,W] of any dtype -> f32 planes [1,P,H,W] (== 1 and > 0 read the same after .float())."""
    img = img.unsqueeze(0) if img.dim() == 2 else img
    out = [img.unsqueeze(0).float().cuda()]
    for m in maps:
        m = m.unsqueeze(0) if m.dim() == 2 else m
        out.append(m.unsqueeze(0).float().cuda())
    return out


def _write(rgb, save_path):
    from ustrun import render
    d = os.path.dirname(save_path)
    if d:
        os.makedirs(d, exist_ok=True)
    render.save_png(rgb[0].cpu().numpy(), save_path)


def draw_contour_and_save(img, pred, mask, save_path='./img/1/example.png'):
    """utils/util.py:346-365 for one image, rendered on the device: the contours of the prediction's parts and of the
    ground truth's (red) over the min-max scaled image."""
    from ustrun import render
    img, pred, mask = _one_image(img, pred, mask)
    _write(render.render_contour(img, pred, mask), save_path)


def draw_mask_and_save(img, pred, save_path='./img/1/example.png'):
    """utils/util.py:367-390 for one image, rendered on the device: the predicted parts tinted over the image."""
    from ustrun import render
    img, pred = _one_image(img, pred)
    _write(render.render_mask(img, pred), save_path)


def _sdf_planes(in_shape, out_shape):
    """compute_sdf's shapes, checked before anything touches the device -> (B, H, W)"""
    in_shape, out_shape = tuple(int(d) for d in in_shape), tuple(int(d) for d in out_shape)
    if len(in_shape) > 3 or len(out_shape) > 4 or (len(out_shape) == 4 and out_shape[1] != 1):
        raise NotImplementedError(f"compute_sdf: only 2-D planes are built -- img_gt [B,H,W] with out_shape [B,H,W] or "
                                  f"[B,1,H,W]; 3-D volumes such as img_gt {in_shape} / out_shape {out_shape} are not")
    if len(in_shape) != 3 or out_shape not in (in_shape, (in_shape[0], 1) + in_shape[1:]):
        raise ValueError(f"compute_sdf: img_gt {in_shape} must be [B,H,W] and out_shape {out_shape} the same or [B,1,H,W]")
    return in_shape


def compute_sdf(img_gt, out_shape):
    """utils/util.py:208-239 on the device (ustrun.functional.signed_distance_map): the signed distance map of every binary
    mask img_gt[b] (binarised as != 0), normalised to [-1, 1] -- negative inside, 0 on the inner boundary, positive outside;
    all zeros for an empty mask, as the reference leaves it.
      numpy [B,H,W] (any integer or bool dtype) -> float64 ndarray of out_shape: the exact integer squared distances come from
        the device, square roots and quotients are taken in float64 as the reference takes them.  A mask with no background,
        where the reference divides 0 / 0, raises ValueError naming the sample (the call waits for the device anyway).
      HIP tensor [B,H,W] -> float32 HIP tensor of out_shape, no host trip and no wait; a full mask gives zeros there --
        ustrun.functional.signed_distance_map returns the per-plane flags that tell.
    out_shape is [B,H,W] or [B,1,H,W]; the reference's 3-D volumes are not built (NotImplementedError)."""
    B, H, W = _sdf_planes(img_gt.shape, out_shape)
    from ustrun import functional as F
    if torch.is_tensor(img_gt):
        if not img_gt.is_cuda:
            raise TypeError("compute_sdf: a tensor must live on the device (pass a numpy array for host data)")
        sdf, _ = F.signed_distance_map((img_gt != 0).float())
        return sdf.reshape(tuple(out_shape))
    mask = np.asarray(img_gt) != 0
    s2, flags = F.signed_dist2(torch.from_numpy(mask.astype(np.float32)).cuda())
    s2, flags = s2.cpu().numpy()[:, 0].astype(np.int64), flags.cpu().numpy()[:, 0]
    if (flags == F.PLANE_FULL).any():
        b = int(np.argmax(flags == F.PLANE_FULL))
        raise ValueError(f"compute_sdf: sample {b} has no background pixel: its signed distance map is undefined "
                         "(the reference divides 0 / 0 here)")
    out = np.zeros((B, H, W), np.float64)
    for b in np.flatnonzero(flags == F.PLANE_MIXED):
        pos, neg = np.sqrt(np.maximum(-s2[b], 0).astype(np.float64)), np.sqrt(np.maximum(s2[b], 0).astype(np.float64))
        out[b] = neg / neg.max() - pos / pos.max()
        out[b][s2[b] == -1] = 0.0
    return out.reshape(tuple(out_shape))


def _sdf_volumes(in_shape, out_shape):
    """compute_sdf_volume's shapes, checked before anything touches the device -> (B, D, H, W)"""
    in_shape, out_shape = tuple(int(d) for d in in_shape), tuple(int(d) for d in out_shape)
    if len(in_shape) != 4 or out_shape not in (in_shape, (in_shape[0], 1) + in_shape[1:]):
        raise ValueError(f"compute_sdf_volume: img_gt {in_shape} must be [B,D,H,W] and out_shape {out_shape} the same or "
                         "[B,1,D,H,W]")
    return in_shape


def compute_sdf_volume(img_gt, out_shape):
    """utils/util.py:208-239 for the volumes its docstring names (shape = (batch_size, x, y, z), :208-217), on the device
    (ustrun.functional.signed_distance_map_3d): the signed distance map of every binary volume img_gt[b] (binarised as != 0),
    normalised over the whole volume to [-1, 1] -- negative inside, 0 on the inner boundary (a foreground voxel with a
    background 6-neighbour), positive outside; all zeros for an empty volume, as the reference leaves it.  `compute_sdf` keeps
    its planes; volumes come in under this name.
      numpy [B,D,H,W] (any integer or bool dtype) -> float64 ndarray of out_shape from the device's exact integer squared
        distances, square roots and quotients in float64 as the reference takes them.  A volume with no background, where the
        reference divides 0 / 0, raises ValueError naming the sample.
      HIP tensor [B,D,H,W] -> float32 HIP tensor of out_shape, no host trip and no wait; a full volume gives zeros there.
    out_shape is [B,D,H,W] or [B,1,D,H,W]."""
    B, D, H, W = _sdf_volumes(img_gt.shape, out_shape)
    from ustrun import functional as F
    if torch.is_tensor(img_gt):
        if not img_gt.is_cuda:
            raise TypeError("compute_sdf_volume: a tensor must live on the device (pass a numpy array for host data)")
        sdf, _ = F.signed_distance_map_3d((img_gt != 0).float())
        return sdf.reshape(tuple(out_shape))
    mask = np.asarray(img_gt) != 0
    s2, flags = F.signed_dist2_3d(torch.from_numpy(mask.astype(np.float32)).cuda())
    s2, flags = s2.cpu().numpy()[:, 0].astype(np.int64), flags.cpu().numpy()[:, 0]
    if (flags == F.PLANE_FULL).any():
        b = int(np.argmax(flags == F.PLANE_FULL))
        raise ValueError(f"compute_sdf_volume: sample {b} has no background voxel: its signed distance map is undefined "
                         "(the reference divides 0 / 0 here)")
    out = np.zeros((B, D, H, W), np.float64)
    for b in np.flatnonzero(flags == F.PLANE_MIXED):
        pos, neg = np.sqrt(np.maximum(-s2[b], 0).astype(np.float64)), np.sqrt(np.maximum(s2[b], 0).astype(np.float64))
        out[b] = neg / neg.max() - pos / pos.max()
        out[b][s2[b] == -1] = 0.0
    return out.reshape(tuple(out_shape))
