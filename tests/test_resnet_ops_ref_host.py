"""CPU pin of tests/resnet_ops_ref.py (the float64 references of tests/test_gpu_resnet_ops.py) against torch's own float64 operators:
F.max_pool2d(3, 2, 1) with autograd and return_indices under planted ties, F.interpolate(mode="bilinear", align_corners=True) with
autograd for up-, down- and same-size, the sum of dilated F.conv2d for the classifier's shifted add and its autograd for the adjoint,
and plain slicing for space-to-batch and the row-window patches."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_ops_ref as R

TIGHT = dict(rtol=1e-12, atol=1e-13)       # float64 against float64: only the order of a few operations differs
POOL_SHAPES = [(2, 8, 13, 10), (3, 20, 7, 9), (1, 4, 1, 1), (1, 4, 1, 7), (2, 12, 6, 1), (1, 8, 2, 2)]
RESIZE_SHAPES = [((9, 13), (41, 50)), ((9, 7), (67, 50)), ((5, 5), (5, 5)), ((1, 6), (7, 1)), ((17, 12), (9, 5)), ((2, 3), (129, 200)),
                 ((65, 65), (513, 513))]
RATES = [(1,), (2, 3), (6, 12, 18), (6, 12, 18, 24)]


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


@pytest.mark.parametrize("n,c,h,w", POOL_SHAPES)
def test_maxpool_and_route_equal_max_pool2d_autograd_with_ties(n, c, h, w):
    rng = np.random.default_rng(h * 10 + w)
    a = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 2.0]), size=(n, c, h, w), p=[0.4, 0.15, 0.15, 0.15, 0.15])      # activations: >= 0, ties
    dp = rng.integers(-16, 17, size=(n, c, (h + 1) // 2, (w + 1) // 2)) / 4.0          # multiples of 1/4: a pixel's sum of four is exact
    at = t64(a).requires_grad_(True)
    p, idx = F.max_pool2d(at, 3, 2, 1, return_indices=True)
    p.backward(t64(dp))
    np.testing.assert_array_equal(R.maxpool3x3s2(a), p.detach().numpy())
    da, best = R.maxpool3x3s2_route(dp, a)
    np.testing.assert_array_equal(da, at.grad.numpy())
    # the winner as a flat index into the plane == return_indices
    oy, ox = np.meshgrid(np.arange(p.shape[2]), np.arange(p.shape[3]), indexing="ij")
    flat = (2 * oy - 1 + best // 3) * w + (2 * ox - 1 + best % 3)
    np.testing.assert_array_equal(flat, idx.numpy())
    win = R.windows3(a, -np.inf)
    tied = (win == win.max(axis=2, keepdims=True)).sum(axis=2) > 1
    if best.size >= 200:                                        # (the small shapes hold a handful of windows: no share to speak of)
        assert tied.mean() >= 0.3 and set(np.unique(best)) == set(range(9))


def test_route_takes_the_first_in_image_maximum():
    a = np.zeros((1, 1, 3, 3))                                   # two windows per axis; everything tied
    dp = np.arange(1.0, 5.0).reshape(1, 1, 2, 2)
    da, best = R.maxpool3x3s2_route(dp, a)
    np.testing.assert_array_equal(best[0, 0], [[4, 3], [1, 0]])  # window (0,0): positions 0..3 lie outside the image; (1,1): all inside
    np.testing.assert_array_equal(da[0, 0], [[1.0, 2.0, 0.0], [3.0, 4.0, 0.0], [0.0, 0.0, 0.0]])


def test_join_and_relu_bwd_add_equal_autograd():
    rng = np.random.default_rng(3)
    n, c, h, w = 2, 12, 5, 3
    y, idn = rng.normal(size=(n, c, h, w)), rng.normal(size=(n, c, h, w))
    s, b, is_, ib = (rng.normal(size=c) for _ in range(4))
    ch = lambda v: t64(v)[None, :, None, None]
    for proj in (False, True):
        yt, it = t64(y).requires_grad_(True), t64(idn).requires_grad_(True)
        pre = yt * ch(s) + ch(b) + (it * ch(is_) + ch(ib) if proj else it)
        out = torch.relu(pre)
        got = R.join(y, s, b, idn, is_ if proj else None, ib if proj else None)
        np.testing.assert_allclose(got, out.detach().numpy(), **TIGHT)
        M = R.join_magnitude(y, s, b, idn, is_ if proj else None, ib if proj else None)
        assert (np.abs(got) <= M * (1 + 1e-15)).all()
        # the join's gradient with respect to its pre-ReLU sum, from two contributions
        ga, gb = rng.normal(size=y.shape), rng.normal(size=y.shape)
        (gp,) = torch.autograd.grad(out, pre, t64(ga + gb))
        np.testing.assert_array_equal(R.relu_bwd_add(ga, gb, out.detach().numpy()), gp.numpy())
    a = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    np.testing.assert_array_equal(R.relu_bwd_add(a, None, np.array([0.0, -0.0, -1e-45, 1e-45, 2.0])), [0.0, 0.0, 0.0, 4.0, 5.0])
    np.testing.assert_array_equal(R.relu_bwd_add(a, a, None), 2 * a)
    np.testing.assert_array_equal(R.relu_bwd_add(a), a)


@pytest.mark.parametrize("lo,hi", RESIZE_SHAPES)
def test_sum_resize_and_adjoint_equal_interpolate_autograd(lo, hi):
    (h, w), (H, W) = lo, hi
    rng = np.random.default_rng(h * 31 + W)
    n, k, nmaps = 2, 3, 1 + (h + w) % 4
    maps = [rng.normal(size=(n, k, h, w)) for _ in range(nmaps)]
    dout = rng.normal(size=(n, k, H, W))
    xs = [t64(m).requires_grad_(True) for m in maps]
    yt = F.interpolate(sum(xs), size=(H, W), mode="bilinear", align_corners=True)
    yt.backward(t64(dout))
    y, dx = R.sum_resize(maps, H, W), R.sum_resize_adjoint(dout, h, w)
    np.testing.assert_allclose(y, yt.detach().numpy(), **TIGHT)
    for x in xs:                                                                # every map receives the same gradient
        np.testing.assert_allclose(dx, x.grad.numpy(), rtol=1e-12, atol=1e-12)
    lhs, rhs = (y * dout).sum(), (sum(maps) * dx).sum()
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(y * dout).sum() + 1.0)
    for n_in, n_out in ((h, H), (w, W)):       # rows sum to one; the support lies inside the touch set; identity is the identity
        M, T = R.resize_matrix(n_in, n_out), R.resize_touch(n_in, n_out)
        np.testing.assert_allclose(M.sum(1), 1.0, rtol=1e-15)
        assert not (M[T == 0] != 0).any()
        if n_in == n_out:
            np.testing.assert_array_equal(M, np.eye(n_in))
    if H == 1 or W == 1:
        np.testing.assert_array_equal(y[:, :, 0, 0], sum(maps)[:, :, 0, 0])   # one output: source coordinate 0


@pytest.mark.parametrize("h,w", [(29, 26), (21, 17), (5, 4), (1, 1), (1, 9), (7, 1)])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("rates", RATES)
def test_aspp_gather_and_scatter_equal_dilated_convolutions(rates, K, h, w):
    rng = np.random.default_rng(100 * len(rates) + 10 * K + h)
    n, ci, nr = 2, 5, len(rates)
    zc = nr * 9 * K
    feat = rng.normal(size=(n, ci, h, w))
    ws = [rng.normal(size=(K, ci, 3, 3)) for _ in rates]
    bs = [rng.normal(size=K) for _ in rates]
    ft = t64(feat).requires_grad_(True)
    want = sum(F.conv2d(ft, t64(ws[r]), t64(bs[r]), 1, rates[r], rates[r]) for r in range(nr))
    wall = np.stack([wq.reshape(K, ci, 9).transpose(2, 0, 1) for wq in ws], 0).reshape(zc, ci)        # row (r 9 + tap) K + k
    z = np.einsum("nchw,oc->nohw", feat, wall)
    got = R.aspp_gather(z, K, rates, sum(bs))
    np.testing.assert_allclose(got, want.detach().numpy(), rtol=1e-11, atol=1e-11)
    # the adjoint: d feat = wall^T dz, dz = scatter(d)
    d = rng.normal(size=got.shape)
    want.backward(t64(d))
    for zcp in (zc, (zc + 127) // 128 * 128):
        dz = R.aspp_scatter(d, K, rates, zcp)
        assert dz.shape[1] == zcp and not dz[:, zc:].any()
        np.testing.assert_allclose(np.einsum("nohw,oc->nchw", dz[:, :zc], wall), ft.grad.numpy(), rtol=1e-11, atol=1e-11)
    # <gather(z), d> == <z, scatter(d)> (bias zero), on a z that is NOT a product: every column independent
    z2 = rng.normal(size=z.shape)
    lhs, rhs = (R.aspp_gather(z2, K, rates, np.zeros(K)) * d).sum(), (z2 * R.aspp_scatter(d, K, rates, zc)).sum()
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(z2).sum() + 1.0)
    # a map no larger than the smallest rate: only the centre taps land
    taps = R.aspp_taps(h, w, rates)
    if min(rates) >= max(h, w):
        np.testing.assert_array_equal(taps, nr)
    assert taps.max() <= 9 * nr and taps.min() >= nr


def test_colsum():
    rng = np.random.default_rng(8)
    x = rng.normal(size=(257, 5)) * 1e3
    np.testing.assert_allclose(R.colsum(x), t64(x).sum(0).numpy(), rtol=1e-12)
    assert R.colsum(np.array([[1e16], [1.0], [-1e16]]))[0] == 1.0             # exact: one rounding


@pytest.mark.parametrize("r", [2, 3, 4, 8])
@pytest.mark.parametrize("h,w", [(9, 7), (3, 10), (8, 8)])
def test_space_to_batch_is_slicing(r, h, w):
    rng = np.random.default_rng(r + h)
    n, c = 2, 3
    x = rng.normal(size=(n, c, h, w))
    s, b = rng.normal(size=c), rng.normal(size=c)
    hs, ws = -(-h // r), -(-w // r)
    for consts, relu in ((False, False), (True, False), (True, True)):
        out = R.space_to_batch(x, r, s if consts else None, b if consts else None, relu)
        assert out.shape == (n * r * r, c, hs, ws)
        v = t64(x)
        if consts:
            v = v * t64(s)[None, :, None, None] + t64(b)[None, :, None, None]
            v = torch.relu(v) if relu else v
        back = np.zeros((n, c, hs * r, ws * r))                                # the inverse permutation of the zero-padded image
        back[:, :, :h, :w] = v.numpy()
        want = back.reshape(n, c, hs, r, ws, r).transpose(0, 3, 5, 1, 2, 4).reshape(n * r * r, c, hs, ws)
        np.testing.assert_array_equal(out, want)
        if h < r:
            assert not out.reshape(n, r, r, c, hs, ws)[:, h:].any()            # whole sub-grids are zero, constants or not


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("nrows", [1, 3, 7])
@pytest.mark.parametrize("cin,win", [(1, 8), (1, 24), (3, 8), (3, 24)])
def test_rowwin_patches_is_slicing(cin, win, nrows, stride):
    rng = np.random.default_rng(cin + win + nrows)
    n, ho, wo = 2, 4, 5
    hp = stride * (ho - 1) + nrows
    wp = -(-(stride * (wo - 1) * cin + win) // cin)
    xp = rng.normal(size=(n, cin, hp, wp))
    nhwc = xp.transpose(0, 2, 3, 1)
    for kp in (nrows * win, nrows * win + 16):
        out = R.rowwin_patches(xp, cin, ho, wo, nrows, win, stride, kp)
        assert out.shape == (n, kp, ho, wo) and not out[:, nrows * win:].any()
        for s in range(nrows):
            for j in range(win):
                want = nhwc[:, s:s + stride * (ho - 1) + 1:stride, j // cin:j // cin + stride * (wo - 1) + 1:stride, j % cin]
                np.testing.assert_array_equal(out[:, s * win + j], want)
    if cin == 3 and win == 24 and nrows == 7 and stride == 2:
        # the stem: a 1x1 GEMM over the patches is the 7x7 / stride-2 convolution of the unpadded image
        wt = rng.normal(size=(6, 3, 7, 7))
        xz = np.zeros_like(xp)                                                 # the image with its border of three zeros
        xz[:, :, 3:hp - 3, 3:wp - 3] = xp[:, :, 3:hp - 3, 3:wp - 3]
        ref = F.conv2d(t64(xz), t64(wt), None, 2, 0)[:, :, :ho, :wo]
        wk = np.zeros((6, 7, 24))
        wk[:, :, :21] = wt.transpose(0, 2, 3, 1).reshape(6, 7, 21)
        got = np.einsum("nkyx,ok->noyx", R.rowwin_patches(xz, 3, ho, wo, 7, 24, 2, 168), wk.reshape(6, 168))
        np.testing.assert_allclose(got, ref.numpy(), rtol=1e-11, atol=1e-11)
