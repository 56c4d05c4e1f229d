"""`GetBoundary` of the reference's dataloaders/custom_transforms.py (:630-647, built inside Normalize_tf at :659) on the device, and
NOTHING ELSE of that module: its PIL / numpy image transforms live in ustrun.datasets and csrc/augment.hip, where they run on the
device per step.

The reference takes `ndimage.binary_dilation(part, iterations=width)` and `ndimage.binary_erosion(part, iterations=width)` of the
cup and the disc channel, keeps the pixels where the two differ, and ORs the two channels.  Both are thresholds of the exact
city-block distance to the part, so one call of ustrun_morph (op = band, reduce_parts) writes the map for a whole batch.
There is no CPU fallback: without the library or a HIP device the call raises."""
import numpy as np
import torch

from ustrun import functional as F


class GetBoundary(object):
    """The boundary band of a multi-label mask, `width` steps to either side of every part's edge.

    `__call__(mask)`:
      * a numpy array H x W x 2 (cup, disc; non-zero = inside), as the reference's data pipeline hands it over -> the reference's
        H x W uint8 numpy array of {0, 1};
      * a device tensor [N, K, H, W] (float32 planes, non-zero = inside; any K >= 1) -> uint8 [N, H, W] on the device, nothing
        waits for it: the form for labels that are augmented on the device."""

    def __init__(self, width=5):
        self.width = width

    def __call__(self, mask):
        if torch.is_tensor(mask):
            if mask.dim() != 4:
                raise ValueError("GetBoundary takes a device tensor [N, K, H, W], got shape %r" % (tuple(mask.shape),))
            return F.boundary_band(mask if mask.dtype == torch.float32 else (mask != 0).float(), width=self.width)
        a = np.asarray(mask)
        if a.ndim != 3 or a.shape[2] != 2:
            raise ValueError("GetBoundary takes an H x W x 2 mask, got shape %r" % (a.shape,))
        planes = torch.from_numpy(np.ascontiguousarray((a != 0).transpose(2, 0, 1), dtype=np.float32))[None]
        return F.boundary_band(planes.cuda(), width=self.width)[0].cpu().numpy()
