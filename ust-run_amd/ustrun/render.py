"""Segmentation overlays on the device (csrc/render.hip): the pictures the reference's `test.py --save_img`
writes with numpy and cv2 (utils/util.py:299-390), rendered per batch by HIP kernels so that one uint8 [N,H,W,3] block is all
that reaches the host.

`pred` / `gt` come in the two forms evaluate.predict and trainer.decode_labels return: f32 planes [N,P,H,W] (fundus), or an
int64 label map [N,H,W] whose part i is label i + 1 (prostate / BUSI: one part; M&Ms: three).
"""
from __future__ import annotations

import collections
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib as L
from .engine import stream_ptr

MASK_PARTS, CONTOUR_PARTS = 5, 4        # colours the reference lists: util.py:368, util.py:348


def _image(image):
    if image.dtype != torch.float32 or not image.is_cuda or image.dim() != 4:
        raise RuntimeError(f"image: expected a float32 HIP tensor [N,C,H,W], got {image.dtype} {tuple(image.shape)} on {image.device}")
    return image.contiguous()


def _parts(name, t, image, parts, most):
    """-> (contiguous tensor, kind, P).  An int64 map carries no part count: `parts`, or every colour there is (a part
    without pixels draws nothing, so the picture is the same)."""
    N, _, H, W = image.shape
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a HIP tensor, got one on {t.device}")
    if t.dtype == torch.int64 and tuple(t.shape) == (N, H, W):
        return t.contiguous(), 1, most if parts is None else int(parts)
    if t.dtype == torch.float32 and t.dim() == 4 and t.shape[0] == N and tuple(t.shape[2:]) == (H, W):
        if parts is not None and int(parts) != t.shape[1]:
            raise RuntimeError(f"{name}: {t.shape[1]} planes, parts = {parts}")
        return t.contiguous(), 0, t.shape[1]
    raise RuntimeError(f"{name}: expected float32 [N,P,H,W] or int64 [N,H,W] for an image batch {tuple(image.shape)}, "
                       f"got {t.dtype} {tuple(t.shape)}")


def image_range(image):
    """Per-image (min, max) over all channels, f32 [N,2] (img.min() / img.max() of util.py:357,378-380)."""
    image = _image(image)
    N, C, H, W = image.shape
    out = torch.empty((N, 2), dtype=torch.float32, device=image.device)
    L.check(L.lib().ustrun_render_range(image.data_ptr(), N, C, H, W, out.data_ptr(), stream_ptr()), "ustrun_render_range")
    return out


def render_mask(image, pred, parts=None):
    """draw_mask_and_save (util.py:367-390) of every image of the batch -> uint8 [N,H,W,3] RGB on the device."""
    image = _image(image)
    pred, kind, P = _parts("pred", pred, image, parts, MASK_PARTS)
    N, C, H, W = image.shape
    rng = image_range(image)
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=image.device)
    L.check(L.lib().ustrun_render_mask(image.data_ptr(), rng.data_ptr(), pred.data_ptr(), kind, N, C, P, H, W, out.data_ptr(),
                                       stream_ptr()), "ustrun_render_mask")
    return out


def render_contour(image, pred, gt, parts=None):
    """draw_contour_and_save (util.py:299-365) of every image of the batch -> uint8 [N,H,W,3] RGB on the device.  A constant
    image renders as 0 outside the contours (the reference divides 0 by 0 there)."""
    image = _image(image)
    pred, kind, P = _parts("pred", pred, image, parts, CONTOUR_PARTS)
    gt, gkind, G = _parts("gt", gt, image, parts, CONTOUR_PARTS)
    if (kind, P) != (gkind, G):
        raise RuntimeError(f"pred and gt differ in form: {pred.dtype} with {P} parts, {gt.dtype} with {G}")
    N, C, H, W = image.shape
    rng = image_range(image)
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=image.device)
    L.check(L.lib().ustrun_render_contour(image.data_ptr(), rng.data_ptr(), pred.data_ptr(), gt.data_ptr(), kind, N, C, P, H, W,
                                          out.data_ptr(), stream_ptr()), "ustrun_render_contour")
    return out


def _pil():
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("writing the --save_img pictures needs Pillow, which is not installed") from e
    return Image


PNG_COMPRESS_LEVEL = 1      # zlib level of the files (PIL's default: 6).  Lossless either way: the decoded pixels are the same


def save_png(array, path):
    """One uint8 [H,W,3] RGB array -> a PNG file (what cv2.imwrite leaves after the reference's RGB -> BGR swap)."""
    a = np.ascontiguousarray(array)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise RuntimeError(f"save_png: expected uint8 [H,W,3], got {a.dtype} {a.shape}")
    _pil().fromarray(a).save(path, format="PNG", compress_level=PNG_COMPRESS_LEVEL)


class PngWriter:
    """save_png on a few host threads (zlib runs without the interpreter lock), so that encoding overlaps the next batches'
    forwards: encoding is nearly all of what --save_img costs (profiles/render.md).  At most `limit` pictures wait at a time;
    close() waits for the rest and raises the first failure."""

    def __init__(self, threads=None, limit=256):
        self.threads = threads or max(1, min(8, len(os.sched_getaffinity(0))))
        self.pool = ThreadPoolExecutor(max_workers=self.threads)
        self.jobs, self.limit = collections.deque(), limit

    def save(self, array, path):
        while len(self.jobs) >= self.limit:
            self.jobs.popleft().result()
        self.jobs.append(self.pool.submit(save_png, array, path))

    def close(self):
        self.pool.shutdown(wait=True)
        while self.jobs:
            self.jobs.popleft().result()
