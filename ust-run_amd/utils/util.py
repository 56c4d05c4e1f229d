"""Checkpoint I/O and meters used by the training scripts -- surface of the reference's
utils/util.py:167-183,259-297 -- and the two overlay pictures of utils/util.py:346-390 that test.py --save_img
writes (the rest of that file is dead code there).  state_dict keys are identical to the reference's, so
checkpoints interchange in both directions."""
import os

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
