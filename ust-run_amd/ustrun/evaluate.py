"""Validation on the device: the reference's `test()` (train.py:253-395, train_mnms.py twin, test.py:64-206).

Eval-mode forward through the HIP U-Net (BatchNorm from the running statistics, applied on load by the consuming
kernel: no separate normalisation pass), prediction and the per-sample overlap counts on the device
(ustrun_pseudo_label, ustrun_dice_counts), so one [N, parts, 3] int32 copy per batch reaches the host instead of the
logits and masks the reference moves with .cpu(); consecutive loader batches share one forward (eval mode: samples do
not interact).  Dice and its averaging (per batch, per domain loader, over the
domains) are the reference's.  The medpy metrics it prints beside the Dice (dc / jc / hd95 / asd, train.py:306-325) are
optional (`validate(..., surface_metrics=True)`): borders, the exact squared distance transform and the percentile's order
statistics run on the device (ustrun_surface_metrics) over the same coalesced batch, one more [N, parts, 6] int32 copy reaches the
host, and utils.metrics.surface_from_records finishes them in float64; they are averaged as the Dice is.  The per-batch
loss the reference computes is never accumulated there and is not computed here.

`validate(..., save_dir=...)` is the reference's `--save_img` (test.py:110-113): the coalesced batch is rendered once on the
device (ustrun/render.py), its uint8 [N,H,W,3] block is copied to the host and written as one PNG per image under the
reference's file names, on a few host threads beside the next batches' forwards (render.PngWriter).  Nothing else changes: the metrics and the logged lines are those of a run without it.

`validate(..., post_process=True)` applies the reference's `post_processing` (dataloaders/utils.py:193-204: holes filled, components
below a fifth of the foreground removed) to every part of the prediction before anything is measured or drawn, on the device
(ustrun_post_process).  Filled parts may overlap, so from there on prediction and ground truth are float planes [N,parts,H,W].

`validate_volumes` is the per-CASE form for datasets that are volumes cut into slices: the slices of a resident test pool are
grouped into cases by a pattern over their names, each case's predictions are stacked to a volume on the device and measured with
utils.metrics.volume_metrics (medpy's dc / jc / hd95 / asd / assd with `voxelspacing`).  `validate` does not call it.
"""
import logging
import os
import re

import numpy as np
import torch

from utils import metrics

from . import functional as F
from . import render
from .trainer import DATASETS, decode_labels

PARTS = {"fundus": ["cup", "disc"], "prostate": ["base"], "BUSI": ["base"], "MNMS": ["lv", "myo", "rv"]}


def predict(dataset, logits):
    """Device prediction: fundus -> f32 {0,1} [N,2,H,W] (sigmoid >= .5 per channel); others -> int64 arg-max [N,H,W]
    (first index on ties), train.py:292-299."""
    mode = DATASETS[dataset][3]
    return F.pseudo_label(logits, 0.5, mode)[0]


def _part_kw(dataset):
    """How the dataset's prediction and ground truth name their parts: MNMS class maps by value, the others as planes."""
    return dict(by_class=True, n_classes=3) if dataset == "MNMS" else {}


def post_processed(dataset, pred, mask):
    """-> (prediction after the reference's post_processing, ground truth), both as float planes [N, parts, H, W]: the mask
    goes through the same call with both steps off, which only decodes it."""
    kw = _part_kw(dataset)
    return F.post_process(pred, **kw), F.post_process(mask, fill_holes=False, min_share=None, **kw)


def post_processed_volume(dataset, pred, mask, post_process=True, largest=False):
    """`post_processed` for stacked cases [N,(parts,)D,H,W]: the prediction through the reference's post_processing on the whole
    volume (post_process) and / or reduced to each part's largest component (largest), the ground truth through the plain decode
    -> both float volumes [N, parts, D, H, W]."""
    kw = _part_kw(dataset)
    return (F.post_process_3d(pred, fill_holes=post_process, min_share=(1, 5) if post_process else None, largest=largest, **kw),
            F.post_process_3d(mask, fill_holes=False, min_share=None, **kw))


def sample_dice(dataset, pred, mask, planes=False):
    """Per-sample, per-part Dice [N, parts] from device overlap counts (utils/metrics.py:114-146 on every sample).
    planes: pred and mask are float planes [N, parts, H, W] whatever the dataset (`post_processed`)."""
    if dataset == "MNMS" and not planes:
        cnt = F.dice_counts(pred, mask, by_class=True, n_classes=3)
    else:
        cnt = F.dice_counts(pred, mask)
    c = cnt.cpu().numpy().astype(np.float64)              # [N, parts, 3]
    return metrics.dice_from_counts(c[..., 0], c[..., 1], c[..., 2])


def sample_metrics(dataset, pred, mask, planes=False):
    """Per-sample, per-part (dice, dc, jc, hd95, asd), [N, parts] each: the Dice of `sample_dice` and the four medpy metrics
    of train.py:306-320 (hd95 = asd = 100 for an empty prediction; an empty ground truth raises, as medpy does)."""
    kw = {} if planes else _part_kw(dataset)
    cnt, rec = F.dice_counts(pred, mask, **kw), F.surface_metrics(pred, mask, **kw)
    c, r = cnt.cpu().numpy(), rec.cpu().numpy()
    cf = c.astype(np.float64)
    return (metrics.dice_from_counts(cf[..., 0], cf[..., 1], cf[..., 2]),) + metrics.surface_from_records(r, c)


def batch_dice(dataset, pred, mask):
    """Per-part Dice of one batch, averaged over its samples (utils/metrics.py:149-231 without ret_arr)."""
    d = sample_dice(dataset, pred, mask)
    return [float(sum(d[:, p]) / len(d)) for p in range(d.shape[1])]


@torch.no_grad()
def validate(dataset, model, loaders, epoch=0, log=logging.info, coalesce=64, surface_metrics=False, save_dir=None,
             save_mode="mask", post_process=False):
    """loaders: one iterable of (image, raw label) batches per domain (any device; moved to the model's).
    Returns (val_dice[parts], per_domain[domain][parts]); leaves the model in train mode, as the reference does.
    surface_metrics=True: returns (val_dice, per_domain, extra) with extra[m] = {"val": [parts], "per_domain": [domain][parts]}
    for m in dc, jc, hd, asd, and logs the reference's val_%s_dc / _jc / _hd / _asd lines (train.py:349-365,378-395).

    In eval mode the samples of a batch do not interact (BatchNorm uses the running statistics), so up to `coalesce`
    images of consecutive loader batches go through ONE forward -- the reference's `test_bs` 1 would otherwise leave the
    deep layers with 8-64 workgroups -- and the Dice is still averaged per loader batch, then per domain, then over the
    domains, exactly as train.py:318-372 does.

    save_dir: also write one picture per image there, `{domain}_{num}_{avg}.png` as test.py:113 names them (domain from 1, num
    the running image count from 1 over all domains, avg = round(mean over the parts of the Dice of the image's LOADER batch, 4));
    save_mode "mask" is the reference's draw_mask_and_save, "contour" its draw_contour_and_save (prediction against ground truth).

    post_process=True: every part of the prediction goes through the reference's post_processing first (`post_processed`); Dice,
    the surface metrics and the pictures are those of the processed prediction (one emptied by it takes hd = asd = 100 like any
    empty prediction), the logged lines, the averaging and the file names keep their form."""
    if save_mode not in ("mask", "contour"):
        raise ValueError("save_mode is 'mask' or 'contour', got %r" % (save_mode,))
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
    writer = render.PngWriter() if save_dir is not None else None
    part = PARTS[dataset]
    dev = next(model.parameters()).device
    model.eval()
    val = [0.0] * len(part)
    per_domain = []
    names = ("dc", "jc", "hd", "asd") if surface_metrics else ()
    xval = {m: [0.0] * len(part) for m in names}
    xper = {m: [] for m in names}
    xdom = {}
    seen = [0, 0]                                           # domain, loader batches flushed in it (for error messages)
    num = [0]                                               # pictures written so far (test.py:70,112)

    def flush(pending, dom):
        if not pending:
            return 0
        image = torch.cat([b[0] for b in pending], 0) if len(pending) > 1 else pending[0][0]
        label = torch.cat([b[1] for b in pending], 0) if len(pending) > 1 else pending[0][1]
        pred, mask = predict(dataset, model(image)), decode_labels(dataset, label)
        if post_process:
            pred, mask = post_processed(dataset, pred, mask)
        if surface_metrics:
            try:
                d, *x = sample_metrics(dataset, pred, mask, planes=post_process)
            except metrics.EmptyGroundTruth as e:           # e.sample counts over the coalesced loader batches
                b, n = 0, e.sample
                while n >= len(pending[b][0]):
                    n -= len(pending[b][0])
                    b += 1
                raise metrics.EmptyGroundTruth(n, e.part, "domain %d, loader batch %d, " % (seen[0] + 1, seen[1] + b)) from None
        else:
            d = sample_dice(dataset, pred, mask, planes=post_process)
        if save_dir is not None:                            # one render and one uint8 [N,H,W,3] copy per coalesced batch
            if save_mode == "mask":
                rgb = render.render_mask(image, pred, parts=len(part))
            else:
                rgb = render.render_contour(image, pred, mask, parts=len(part))
            rgb = rgb.cpu().numpy()
        o = 0
        for b in pending:                                   # the batch's Dice = mean over ITS samples
            n = len(b[0])
            if save_dir is not None:                        # test.py:108-113
                dice = [float(sum(d[o:o + n, p]) / n) for p in range(len(part))]
                avg = round(sum(dice) / len(dice), 4)
                for j in range(o, o + n):
                    num[0] += 1
                    writer.save(rgb[j], os.path.join(save_dir, "%d_%d_%s.png" % (seen[0] + 1, num[0], avg)))
            for p in range(len(part)):
                dom[p] += float(sum(d[o:o + n, p]) / n)
                for m, v in zip(names, x if surface_metrics else ()):
                    xdom[m][p] += float(sum(v[o:o + n, p]) / n)
            o += n
        seen[1] += len(pending)
        return len(pending)

    try:
        for i, loader in enumerate(loaders):
            dom, nb, pending, held = [0.0] * len(part), 0, [], 0
            seen[0], seen[1] = i, 0
            for m in names:
                xdom[m] = [0.0] * len(part)
            for image, label in loader:
                image, label = image.to(dev), label.to(dev)
                if pending and (held + len(image) > coalesce or image.shape[1:] != pending[0][0].shape[1:]):
                    nb += flush(pending, dom)
                    pending, held = [], 0
                pending.append((image, label))
                held += len(image)
            nb += flush(pending, dom)
            dom = [d / max(nb, 1) for d in dom]
            per_domain.append(dom)
            for p in range(len(part)):
                val[p] += dom[p]
            for m in names:
                xdom[m] = [d / max(nb, 1) for d in xdom[m]]
                xper[m].append(xdom[m])
                for p in range(len(part)):
                    xval[m][p] += xdom[m][p]
            if log:
                log("domain%d epoch %d :\n\t%s" % (i + 1, epoch, "".join("val_%s_dice: %f, " % (n, dom[k]) for k, n in enumerate(part)))
                    + _surface_lines(part, xdom))
    finally:
        if writer is not None:                              # the files are complete when validate returns
            writer.close()
    model.train()
    val = [v / max(len(loaders), 1) for v in val]
    for m in names:
        xval[m] = [v / max(len(loaders), 1) for v in xval[m]]
    if log:
        log("epoch %d :\n\t%s" % (epoch, "".join("val_%s_dice: %f, " % (n, val[k]) for k, n in enumerate(part)))
            + _surface_lines(part, xval))
    if surface_metrics:
        return val, per_domain, {m: {"val": xval[m], "per_domain": xper[m]} for m in names}
    return val, per_domain


def _surface_lines(part, x):
    """The reference's lines behind the Dice line (train.py:353-364): dc and jc on one, hd and asd on the next."""
    if not x:
        return ""
    line = lambda m: "".join("val_%s_%s: %f, " % (n, m, x[m][k]) for k, n in enumerate(part))
    return "\n\t" + line("dc") + "\t" + line("jc") + "\n\t" + line("hd") + "\t" + line("asd")


def case_groups(names, case_pattern):
    """The slices of a listing grouped into cases: name i belongs to case re.match(case_pattern, name).group(1); cases and the
    slices inside a case keep the listing's order -> [(case, [i, ...]), ...].  ValueError for a name the pattern does not match."""
    rx = re.compile(case_pattern)
    groups = {}
    for i, name in enumerate(names):
        m = rx.match(name)
        if m is None or not m.groups():
            raise ValueError("case_pattern %r with one group does not match the name %r" % (case_pattern, name))
        groups.setdefault(m.group(1), []).append(i)
    return list(groups.items())


VOLUME_METRICS = ("dc", "jc", "hd95", "asd", "assd")


@torch.no_grad()
def validate_volumes(dataset, model, ds_list, case_pattern, voxelspacing=None, log=logging.info, coalesce=64, post_process=False,
                     largest=False):
    """Per-case volume metrics of a test pool (test.py --volume_metrics): ds_list holds one ustrun.datasets.ResidentDataset per
    domain; its `names` are grouped by `case_groups`, each case's slices go through the model (up to `coalesce` per forward) and
    `predict`, prediction and ground truth are stacked to one volume [1,(parts,)D,H,W] on the device in listing order and measured
    with utils.metrics.volume_metrics(voxelspacing) -- medpy's binary.dc / jc / hd95 / asd / assd (train.py:306-325) on the
    volume instead of the slice.  -> per_domain[domain][metric] = [parts] means over the domain's cases; one
    vol_<part>_dc / jc / hd95 / asd / assd line per domain is logged.  Leaves the model in train mode, as `validate` does.

    post_process=True: every part of the stacked prediction goes through the reference's post_processing AS A VOLUME first
    (`post_processed_volume`: cavities filled, components below a fifth of the case's foreground removed); largest=True keeps only
    the largest component of each part, after the share rule when both are set.  Default off: the path is the one above."""
    from .datasets import stage_finish
    part = PARTS[dataset]
    kw = _part_kw(dataset)
    dev = next(model.parameters()).device
    model.eval()
    per_domain = []
    for i, ds in enumerate(ds_list):
        cases = case_groups(ds.names, case_pattern)
        acc = {m: np.zeros(len(part)) for m in VOLUME_METRICS}
        for case, idx in cases:
            preds, masks = [], []
            for o in range(0, len(idx), coalesce):
                sel = torch.as_tensor(idx[o:o + coalesce], device=ds.images.device)
                x, _, y = stage_finish(ds.images[sel], None, ds.labels[sel])
                preds.append(predict(dataset, model(x.to(dev))))
                masks.append(decode_labels(dataset, y.to(dev)))
            pred, mask = torch.cat(preds), torch.cat(masks)               # [D,H,W] class maps, or planes [D,parts,H,W]
            if pred.dim() == 4:
                pred, mask = pred.transpose(0, 1), mask.transpose(0, 1)
            pred, mask, vkw = pred[None].contiguous(), mask[None].contiguous(), kw
            if post_process or largest:
                pred, mask = post_processed_volume(dataset, pred, mask, post_process=post_process, largest=largest)
                vkw = {}
            try:
                got = metrics.volume_metrics(pred, mask, voxelspacing=voxelspacing, **vkw)
            except metrics.EmptyGroundTruth as e:
                raise metrics.EmptyGroundTruth(0, e.part, "domain %d, case %s, " % (i + 1, case)) from None
            for m in VOLUME_METRICS:
                acc[m] += got[m][0]
        dom = {m: (acc[m] / max(len(cases), 1)).tolist() for m in VOLUME_METRICS}
        per_domain.append(dom)
        if log:
            log("domain%d, %d cases :\n\t%s" % (i + 1, len(cases), "\n\t".join(
                "".join("vol_%s_%s: %f, " % (n, m, dom[m][k]) for k, n in enumerate(part)) for m in VOLUME_METRICS)))
    model.train()
    return per_domain

