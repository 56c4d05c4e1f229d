"""Float64 restatement, in plain numpy, of DeepLabV2's operators between the convolutions (csrc/resnet_ops.hip) for the tests: the stem's
MaxPool2d(3, 2, 1) over the activated tensor and its gradient routing, the bottleneck's residual join and its gradient, the bilinear resize
(align_corners=True, any ratio) of the summed classifier maps with its adjoint, the classifier's shifted add over a 1x1 GEMM's columns
(`ustrun_aspp_gather`, include/ustrun.h) with its adjoint, the column sum, space-to-batch and the stem's row-window patches.  No GPU, no
torch, nothing from oracle/.  tests/test_resnet_ops_ref_host.py pins every function against torch's own float64 operators on the CPU.

Tensors are NCHW arrays [N, C, H, W] in and out (the kernels' NHWC layout is the caller's business); every function converts what it is
given to float64 and never modifies it.
"""
import math

import numpy as np

from bn_ops_ref import _f64


def _chan(v):
    """a per-channel constant [C] against [N, C, H, W]"""
    return _f64(v)[None, :, None, None]


def act(y, scale, shift):
    """relu(y scale[c] + shift[c]): the ACTIVATED tensor the stem's pool reads"""
    return np.maximum(_f64(y) * _chan(scale) + _chan(shift), 0.0)


def act_magnitude(y, scale, shift):
    """|y scale| + |shift|: what a float32 evaluation's rounding errors are proportional to"""
    return np.abs(_f64(y) * _chan(scale)) + np.abs(_chan(shift))


def _padded(a, fill):
    """a with the pool's border of `fill`: [N, C, 2 Ho + 1, 2 Wo + 1], Ho = (H + 1) // 2, the image at (1, 1)"""
    a = _f64(a)
    N, C, H, W = a.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    p = np.full((N, C, 2 * Ho + 1, 2 * Wo + 1), float(fill))
    p[:, :, 1:H + 1, 1:W + 1] = a
    return p, Ho, Wo


def _tap(p, q, Ho, Wo):
    """window position q = 3 dy + dx of every window: a view [N, C, Ho, Wo] of the padded array"""
    return p[:, :, q // 3:q // 3 + 2 * Ho:2, q % 3:q % 3 + 2 * Wo:2]


def windows3(a, fill):
    """[N, C, H, W] -> [N, C, 9, Ho, Wo], Ho = (H + 1) // 2: the 3x3 / stride-2 / padding-1 windows in row-major order, `fill` where a
    window position lies outside the image"""
    p, Ho, Wo = _padded(a, fill)
    return np.stack([_tap(p, q, Ho, Wo) for q in range(9)], axis=2)


def window_max(a, fill):
    """the largest element of every window, positions outside the image counting as `fill`"""
    p, Ho, Wo = _padded(a, fill)
    m = _tap(p, 0, Ho, Wo).copy()
    for q in range(1, 9):
        np.maximum(m, _tap(p, q, Ho, Wo), out=m)
    return m


def window_ties(a):
    """how many in-image positions of every window hold its maximum (> 1: the window is tied)"""
    p, Ho, Wo = _padded(a, -np.inf)
    m = window_max(a, -np.inf)
    return sum((_tap(p, q, Ho, Wo) == m).astype(np.int64) for q in range(9))


def maxpool3x3s2(a):
    """MaxPool2d(3, stride 2, padding 1) of the activated tensor a: the padding never wins (-inf)"""
    return window_max(a, -np.inf)


def maxpool3x3s2_route(dp, a):
    """The adjoint of maxpool3x3s2 at a: each window's dp goes to its FIRST maximum in row-major window order (strict >), counted over
    in-image positions only; an input pixel sums what its up to four windows send.  Returns (da, winner[N, C, Ho, Wo] in 0..8)."""
    dp = _f64(dp)
    H, W = np.shape(a)[2:]
    p, Ho, Wo = _padded(a, -np.inf)
    best = np.zeros(dp.shape, dtype=np.int64)
    bv = _tap(p, 0, Ho, Wo).copy()
    for q in range(1, 9):
        t = _tap(p, q, Ho, Wo)
        m = t > bv
        bv = np.where(m, t, bv)
        best = np.where(m, q, best)
    pa = np.zeros(p.shape)
    for q in range(9):
        _tap(pa, q, Ho, Wo)[...] += np.where(best == q, dp, 0.0)
    return pa[:, :, 1:H + 1, 1:W + 1].copy(), best


def join(y, s, b, idn, is_=None, ib=None):
    """The bottleneck's join relu(y s + b + identity), identity = idn is_ + ib (the projection's BatchNorm) or idn itself (is_ None)"""
    r = _f64(idn) if is_ is None else _f64(idn) * _chan(is_) + _chan(ib)
    return np.maximum(_f64(y) * _chan(s) + _chan(b) + r, 0.0)


def join_magnitude(y, s, b, idn, is_=None, ib=None):
    """M = |y s| + |b| + |idn is_| + |ib| (|idn| without the projection's constants): no partial sum of the join exceeds it"""
    r = np.abs(_f64(idn)) if is_ is None else np.abs(_f64(idn) * _chan(is_)) + np.abs(_chan(ib))
    return act_magnitude(y, s, b) + r


def relu_bwd_add(a, b=None, ref=None):
    """g = (a + b) where ref > 0, +0 elsewhere (-0.0, negative and NaN-free `ref` values mask); b None: one contribution; ref None: no mask"""
    v = _f64(a) if b is None else _f64(a) + _f64(b)
    return v.copy() if ref is None else np.where(_f64(ref) > 0, v, 0.0)


def resize_coord(n_in, n_out):
    """align_corners=True source coordinate of each of the n_out outputs: o (n_in - 1) / (n_out - 1); 0 when n_out == 1"""
    o = np.arange(n_out, dtype=np.float64)
    return o * (n_in - 1) / (n_out - 1) if n_out > 1 else np.zeros(n_out)


def resize_matrix(n_in, n_out):
    """M[n_out, n_in]: output o = (1 - l) in[i0] + l in[min(i0 + 1, n_in - 1)], i0 = floor(src), l = src - i0 -- the same matrix serves
    every ratio: up, down and identity"""
    M = np.zeros((n_out, n_in))
    for o, s in enumerate(resize_coord(n_in, n_out)):
        i0 = min(int(math.floor(s)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        l = s - i0
        M[o, i0] += 1.0 - l
        M[o, i1] += l
    return M


def resize_touch(n_in, n_out):
    """T[n_out, n_in] = 1 where |src(o) - i| <= 1: the closed support of the weights, every (o, i) whose weight can be nonzero when src is
    evaluated with a small error"""
    return (np.abs(resize_coord(n_in, n_out)[:, None] - np.arange(n_in)[None, :]) <= 1.0).astype(np.float64)


def sum_resize(maps, H, W):
    """sum of the maps [N, K, h, w], resized to [N, K, H, W]: My @ x @ Mx^T"""
    x = _f64(maps[0]).copy()
    for m in maps[1:]:
        x = x + _f64(m)
    return resize_matrix(x.shape[2], H) @ x @ resize_matrix(x.shape[3], W).T


def sum_resize_adjoint(dout, h, w, My=None, Mx=None):
    """[N, K, H, W] -> [N, K, h, w]: My^T @ dout @ Mx (My / Mx: other matrices of the same shapes, e.g. resize_touch)"""
    dout = _f64(dout)
    My = resize_matrix(h, dout.shape[2]) if My is None else My
    Mx = resize_matrix(w, dout.shape[3]) if Mx is None else Mx
    return My.T @ dout @ Mx


def _shifted(src, dy, dx):
    """out[..., y, x] = src[..., y + dy, x + dx], zero where that lies outside the image"""
    h, w = src.shape[-2:]
    out = np.zeros_like(src)
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[..., y0:y1, x0:x1] = src[..., y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def aspp_gather(z, K, rates, bias_sum):
    """out[n, k, p] = bias_sum[k] + sum_{r, tap} z[n, (r 9 + tap) K + k, p + rates[r] (tap / 3 - 1, tap % 3 - 1)], zero outside the image
    (include/ustrun.h); z: [N, >= len(rates) 9 K, h, w]"""
    z = _f64(z)
    out = np.zeros((z.shape[0], K) + z.shape[2:]) + _chan(bias_sum)
    for r, rate in enumerate(rates):
        for tap in range(9):
            c0 = (r * 9 + tap) * K
            out += _shifted(z[:, c0:c0 + K], rate * (tap // 3 - 1), rate * (tap % 3 - 1))
    return out


def aspp_taps(h, w, rates):
    """[h, w]: how many of the len(rates) x 9 taps of a pixel land inside the image"""
    one = np.ones((1, 1, h, w))
    return sum(_shifted(one, rate * (tap // 3 - 1), rate * (tap % 3 - 1)) for rate in rates for tap in range(9))[0, 0]


def aspp_scatter(dlow, K, rates, zc_padded):
    """The adjoint of aspp_gather: dz[n, (r 9 + tap) K + k, p] = dlow[n, k, p - rates[r] (tap / 3 - 1, tap % 3 - 1)], zero outside the image
    and in the columns >= len(rates) 9 K"""
    dlow = _f64(dlow)
    dz = np.zeros((dlow.shape[0], zc_padded) + dlow.shape[2:])
    for r, rate in enumerate(rates):
        for tap in range(9):
            c0 = (r * 9 + tap) * K
            dz[:, c0:c0 + K] = _shifted(dlow, -rate * (tap // 3 - 1), -rate * (tap % 3 - 1))
    return dz


def colsum(x):
    """x[rows, C] -> [C], each column summed exactly (math.fsum: one rounding, to float64)"""
    x = _f64(x)
    return np.array([math.fsum(x[:, c]) for c in range(x.shape[1])])


def space_to_batch(x, r, scale=None, shift=None, relu=False):
    """out[(n r + a) r + b, c, i, j] = act(x[n, c, i r + a, j r + b]), every residue class (a, b) an image of ceil(H / r) x ceil(W / r),
    ZERO (not act(0)) past a shorter sub-grid's edge; act = x scale + shift (then max(0, .) when relu), a copy without constants"""
    x = _f64(x)
    N, C, H, W = x.shape
    v = x if scale is None else x * _chan(scale) + _chan(shift)
    if scale is not None and relu:
        v = np.maximum(v, 0.0)
    Hs, Ws = (H + r - 1) // r, (W + r - 1) // r
    out = np.zeros((N * r * r, C, Hs, Ws))
    for n in range(N):
        for a in range(r):
            for b in range(r):
                sub = v[n, :, a::r, b::r]
                out[(n * r + a) * r + b, :, :sub.shape[1], :sub.shape[2]] = sub
    return out


def rowwin_patches(xp, Cin, Ho, Wo, nrows, win, stride, k_padded):
    """xp: the zero-padded source [N, Cin, Hp, Wp].  out[n, s win + j, y, x] = element j of the `win` contiguous NHWC elements that start
    at pixel (stride y + s, stride x) -- channel j % Cin of pixel stride x + j // Cin -- for the s < nrows kernel rows; columns
    >= nrows win are zero"""
    xp = _f64(xp)
    N, Hp, Wp = xp.shape[0], xp.shape[2], xp.shape[3]
    assert xp.shape[1] == Cin and stride * (Ho - 1) + nrows <= Hp and stride * (Wo - 1) * Cin + win <= Wp * Cin and k_padded >= nrows * win
    flat = xp.transpose(0, 2, 3, 1).reshape(N, Hp, Wp * Cin)
    out = np.zeros((N, k_padded, Ho, Wo))
    for s in range(nrows):
        for x in range(Wo):
            c0 = stride * x * Cin
            out[:, s * win:(s + 1) * win, :, x] = flat[:, s:s + stride * (Ho - 1) + 1:stride, c0:c0 + win].transpose(0, 2, 1)
    return out
