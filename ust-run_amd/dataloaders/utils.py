"""`post_processing` of the reference's dataloaders/utils.py:193-204, computed on the device (ustrun_post_process).  There is no
CPU fallback: without the library or a HIP device the call raises."""
import numpy as np
import torch

from ustrun import functional as F


def post_processing(prediction):
    """One 2-D binary plane (numpy array or tensor on any device; non-zero = foreground) -> the plane with its holes filled and
    every 8-connected component below a fifth of the filled foreground removed.  A numpy input gives a bool numpy array, as the
    reference returns; a tensor gives a tensor of its device and dtype."""
    is_np = not torch.is_tensor(prediction)
    t = torch.from_numpy(np.ascontiguousarray(prediction)) if is_np else prediction
    if t.dim() != 2:
        raise ValueError("post_processing takes one 2-D plane, got shape %r" % (tuple(t.shape),))
    out = F.post_process((t != 0).to(device="cuda", dtype=torch.float32)[None, None])[0, 0]
    if is_np:
        return out.cpu().numpy().astype(bool)
    return out.to(device=t.device, dtype=t.dtype)
