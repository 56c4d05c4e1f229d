"""Float64 restatement, in plain numpy, of the operators between the convolutions (csrc/bn.hip, csrc/upsample.hip) for the tests:
train-mode BatchNorm statistics -> constants (include/ustrun.h, `ustrun_bn_finalize`), the eval-mode constants, the BatchNorm + ReLU
activation with per-pass constants, MaxPool2d(2) and its gradient routing, and nn.Upsample(scale_factor=2, mode='bilinear',
align_corners=True) with its adjoint.  No GPU, nothing from oracle/.  tests/test_bn_ops_ref_host.py pins every function against torch's
own float64 operators on the CPU.

Activations are NHWC arrays [N, H, W, C]; every function converts what it is given to float64 and never modifies it.
"""
import math
from collections import namedtuple

import numpy as np

Finalized = namedtuple("Finalized", "scale shift mean rstd running_mean running_var")


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def stat_sums(stat):
    """stat[rows, 2, C] -> (sum[C], sum of squares[C]), each column summed exactly (math.fsum: one rounding, to float64)."""
    stat = _f64(stat)
    s1 = np.array([math.fsum(stat[:, 0, c]) for c in range(stat.shape[2])])
    s2 = np.array([math.fsum(stat[:, 1, c]) for c in range(stat.shape[2])])
    return s1, s2


def raw_variance(stat, count):
    """sum2 / count - mean^2 BEFORE the clamp at zero (negative where the table's roundings make it so)."""
    s1, s2 = stat_sums(stat)
    m = s1 / count
    return s2 / count - m * m


def finalize(stat, count, gamma, beta, rm, rv, momentum, eps):
    """The contract of ustrun_bn_finalize: mean = sum / count, var = max(sum2 / count - mean^2, 0) (biased), rstd = 1 / sqrt(var + eps),
    scale = gamma rstd, shift = beta - mean scale; the running buffers blend in the batch mean and the UNBIASED variance
    (var count / (count - 1)) with `momentum`, as torch does: new = (1 - momentum) old + momentum batch.  momentum and eps are taken at the
    float32 value the C ABI receives."""
    gamma, beta, rm, rv = _f64(gamma), _f64(beta), _f64(rm), _f64(rv)
    mom, eps = float(np.float32(momentum)), float(np.float32(eps))
    s1, s2 = stat_sums(stat)
    count = float(count)
    mean = s1 / count
    var = np.maximum(s2 / count - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * rstd
    shift = beta - mean * scale
    unbiased = var * count / (count - 1.0) if count > 1 else var
    return Finalized(scale, shift, mean, rstd, (1.0 - mom) * rm + mom * mean, (1.0 - mom) * rv + mom * unbiased)


def eval_affine(gamma, beta, rm, rv, eps):
    """eval-mode constants: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean scale."""
    scale = _f64(gamma) / np.sqrt(_f64(rv) + float(np.float32(eps)))
    return scale, _f64(beta) - _f64(rm) * scale


def _constants(table, N, C, gN, gstride):
    """[N, C] rows of a constant table: image n reads table[(n // gN) * gstride : ... + C] (gN = 0: one pass, every image row 0)."""
    table = _f64(table).ravel()
    return np.stack([table[(n // gN if gN > 0 else 0) * gstride:][:C] for n in range(N)])


def act(y, scale=None, shift=None, relu=False, gN=0, gstride=0):
    """a = y scale[c] + shift[c], then max(0, .) when relu; scale None: a = y and NO ReLU (the operators' "plain copy" form)."""
    y = _f64(y)
    if scale is None:
        return y.copy()
    N, C = y.shape[0], y.shape[3]
    s, b = _constants(scale, N, C, gN, gstride), _constants(shift, N, C, gN, gstride)
    a = y * s[:, None, None, :] + b[:, None, None, :]
    return np.maximum(a, 0.0) if relu else a


def act_magnitude(y, scale=None, shift=None, gN=0, gstride=0):
    """|y scale| + |shift|: what a float32 evaluation's rounding errors are proportional to (0 for the plain copy: it is exact)."""
    y = _f64(y)
    if scale is None:
        return np.zeros_like(y)
    N, C = y.shape[0], y.shape[3]
    s, b = _constants(scale, N, C, gN, gstride), _constants(shift, N, C, gN, gstride)
    return np.abs(y * s[:, None, None, :]) + np.abs(b[:, None, None, :])


def _windows(a):
    """[N, H, W, C] -> [N, H//2, W//2, 4, C]: the 2x2 windows in row-major order (0,0) (0,1) (1,0) (1,1); an odd last row / column is dropped."""
    N, H, W, C = a.shape
    Hp, Wp = H // 2, W // 2
    w = a[:, :2 * Hp, :2 * Wp].reshape(N, Hp, 2, Wp, 2, C)
    return w.transpose(0, 1, 3, 2, 4, 5).reshape(N, Hp, Wp, 4, C)


def pool2(a):
    """MaxPool2d(2): floor extents."""
    return _windows(_f64(a)).max(axis=3)


def maxpool_route(dp, x):
    """Gradient of pool2 at x: dp goes to the FIRST maximum of each window (row-major scan, strict >), zero elsewhere, the odd last row /
    column included.  Returns (dx, winner[N, H//2, W//2, C] in 0..3)."""
    dp, x = _f64(dp), _f64(x)
    N, H, W, C = x.shape
    Hp, Wp = H // 2, W // 2
    w = _windows(x)
    best = np.zeros((N, Hp, Wp, C), dtype=np.int64)
    bv = w[:, :, :, 0].copy()
    for q in (1, 2, 3):
        m = w[:, :, :, q] > bv
        bv = np.where(m, w[:, :, :, q], bv)
        best = np.where(m, q, best)
    dx = np.zeros_like(x)
    for q in range(4):
        dx[:, (q >> 1):2 * Hp:2, (q & 1):2 * Wp:2] = np.where(best == q, dp, 0.0)
    return dx, best


def src_coord(n_in):
    """align_corners=True source coordinate of each of the 2 n_in outputs: o (n_in - 1) / (2 n_in - 1); all 0 for n_in = 1."""
    o = np.arange(2 * n_in, dtype=np.float64)
    return o * (n_in - 1) / (2 * n_in - 1)


def lerp_matrix(n_in):
    """U[2 n_in, n_in]: output o = (1 - l) in[i0] + l in[min(i0 + 1, n_in - 1)], i0 = floor(src), l = src - i0."""
    src = src_coord(n_in)
    U = np.zeros((2 * n_in, n_in))
    for o, s in enumerate(src):
        i0 = min(int(math.floor(s)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        l = s - i0
        U[o, i0] += 1.0 - l
        U[o, i1] += l
    return U


def touch_matrix(n_in):
    """T[2 n_in, n_in] = 1 where |src(o) - i| <= 1: the closed support of the interpolation weights -- every (o, i) whose weight can be
    nonzero when src is evaluated with a small error."""
    return (np.abs(src_coord(n_in)[:, None] - np.arange(n_in)[None, :]) <= 1.0).astype(np.float64)


def upsample2x(x):
    """[N, H, W, C] -> [N, 2H, 2W, C]"""
    x = _f64(x)
    return np.einsum("oh,nhwc,pw->nopc", lerp_matrix(x.shape[1]), x, lerp_matrix(x.shape[2]))


def upsample2x_adjoint(dy, Uy=None, Ux=None):
    """[N, 2H, 2W, C] -> [N, H, W, C]: the transpose of upsample2x (Uy / Ux: other matrices of the same shape, e.g. touch_matrix)."""
    dy = _f64(dy)
    H, W = dy.shape[1] // 2, dy.shape[2] // 2
    return np.einsum("oh,nopc,pw->nhwc", lerp_matrix(H) if Uy is None else Uy, dy, lerp_matrix(W) if Ux is None else Ux)
