"""float64 numpy restatement of the BatchNorm + ReLU (+ MaxPool2d(2)) backward through FROZEN statistics (include/ustrun.h,
`ustrun_bn_bwd_frozen`): what autograd computes for nn.BatchNorm2d in eval mode followed by ReLU (and, pooled, by MaxPool2d(2)).

Everything is NHWC.  With scale = gamma * rstd, rstd = 1 / sqrt(running_var + eps), shift = beta - running_mean * scale:

    a  = y * scale + shift
    g  = (da [+ dp routed to the first maximum of relu(a) in each 2x2 window]) * [a > 0]
    dy = scale * g,   dbeta = sum g,   dgamma = rstd * sum g * (y - running_mean)

The window scan is torch's: (0,0) (0,1) (1,0) (1,1), a later pixel wins only when strictly greater; the odd last row / column that
MaxPool2d drops belongs to no window and receives da alone.  tests/test_frozen_bn_ref_host.py pins this to torch's float64 autograd.
"""
import numpy as np


def routed(dp, a):
    """dp [N, H//2, W//2, C] scattered to the first arg-max of relu(a) in each complete 2x2 window of a [N, H, W, C]"""
    n, h, w, c = a.shape
    hp, wp = h // 2, w // 2
    r = np.maximum(a, 0.0)
    out = np.zeros_like(a)
    if hp == 0 or wp == 0:
        return out
    win = np.stack([r[:, 0:2 * hp:2, 0:2 * wp:2], r[:, 0:2 * hp:2, 1:2 * wp:2], r[:, 1:2 * hp:2, 0:2 * wp:2],
                    r[:, 1:2 * hp:2, 1:2 * wp:2]], 0)
    best = np.argmax(win, 0)                # numpy returns the FIRST maximum: the strict-> scan
    for q in range(4):
        out[:, (q >> 1):2 * hp:2, (q & 1):2 * wp:2] = np.where(best == q, dp, 0.0)
    return out


def frozen_bn_bwd(da, dp, y, scale, shift, mean, rstd):
    """-> dy [N,H,W,C], dgamma [C], dbeta [C], all float64.  da or dp may be None (not both)."""
    y = np.asarray(y, np.float64)
    scale, shift, mean, rstd = (np.asarray(v, np.float64) for v in (scale, shift, mean, rstd))
    a = y * scale + shift
    g = np.zeros_like(y) if da is None else np.asarray(da, np.float64).copy()
    if dp is not None:
        g = g + routed(np.asarray(dp, np.float64), a)
    g = g * (a > 0)
    dy = scale * g
    dbeta = g.sum((0, 1, 2))
    dgamma = rstd * (g * (y - mean)).sum((0, 1, 2))
    return dy, dgamma, dbeta
