"""CPU pin of tests/bn_ops_ref.py (the float64 references of tests/test_gpu_bn_forward_ops.py) against torch's own float64 operators:
F.batch_norm in training mode with the running buffers it updates, F.max_pool2d and its autograd, F.interpolate(scale_factor=2,
mode="bilinear", align_corners=True) and its autograd -- odd and one-pixel extents and planted ties included."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_ops_ref as R

TIGHT = dict(rtol=1e-12, atol=1e-13)       # float64 against float64: only the order of a few operations differs


def nchw(a):           # numpy NHWC -> torch NCHW float64
    return torch.from_numpy(np.ascontiguousarray(a)).double().permute(0, 3, 1, 2).contiguous()


def nhwc(t):           # torch NCHW -> numpy NHWC
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


@pytest.mark.parametrize("n,h,w,c,rows", [(2, 5, 7, 6, 1), (3, 4, 4, 24, 7), (1, 1, 2, 3, 2), (4, 9, 11, 8, 97)])
@pytest.mark.parametrize("momentum", [0.1, 1.0])
def test_finalize_equals_batch_norm_training(n, h, w, c, rows, momentum):
    rng = np.random.default_rng(n * 100 + c)
    y = rng.normal(size=(n, h, w, c)) * rng.uniform(0.5, 2, c) + rng.normal(size=c)
    y[..., 0] += 1e3                                          # |mean| / std = 1e3
    gamma, beta = rng.normal(size=c), rng.normal(size=c)
    gamma[1 % c] = 0.0
    rm, rv = rng.normal(size=c), rng.uniform(0.5, 2, c)
    flat = y.reshape(-1, c)
    chunks = np.array_split(flat, rows)                       # the rows of a statistics table: per-chunk sums, here kept in float64
    stat = np.stack([np.stack([ch.sum(0), (ch * ch).sum(0)]) for ch in chunks])
    mom, eps = float(np.float32(momentum)), float(np.float32(1e-5))
    got = R.finalize(stat, flat.shape[0], gamma, beta, rm, rv, momentum, 1e-5)

    trm, trv = torch.from_numpy(rm.copy()), torch.from_numpy(rv.copy())
    out = F.batch_norm(nchw(y), trm, trv, torch.from_numpy(gamma), torch.from_numpy(beta), True, mom, eps)
    np.testing.assert_allclose(got.mean, flat.mean(0), **TIGHT)
    # the one-pass variance loses mean^2 / var digits: 1e6 x 2^-53 on channel 0
    var = flat.var(0)
    np.testing.assert_allclose(got.rstd, 1.0 / np.sqrt(var + eps), rtol=1e-9)
    np.testing.assert_allclose(got.running_mean, trm.numpy(), **TIGHT)
    np.testing.assert_allclose(got.running_var, trv.numpy(), rtol=1e-9)
    np.testing.assert_allclose(R.act(y, got.scale, got.shift), nhwc(out), rtol=1e-9, atol=1e-9)
    assert got.scale[1 % c] == 0.0 and got.shift[1 % c] == beta[1 % c]


def test_finalize_clamps_a_negative_variance_and_counts_one_sample():
    stat = np.array([[[3.0], [2.9999]]])                       # sum2 / 3 - 1 < 0
    assert R.raw_variance(stat, 3)[0] < 0
    f = R.finalize(stat, 3, [2.0], [0.5], [0.0], [1.0], 0.1, 1e-5)
    eps = float(np.float32(1e-5))
    assert f.rstd[0] == 1.0 / np.sqrt(eps) and f.running_var[0] == (1.0 - float(np.float32(0.1))) * 1.0
    one = R.finalize(np.array([[[4.0], [16.0]]]), 1, [1.0], [0.0], [0.0], [1.0], 1.0, 1e-5)      # count 1: no n / (n - 1)
    assert one.mean[0] == 4.0 and one.running_var[0] == 0.0


def test_eval_affine_equals_batch_norm_eval():
    rng = np.random.default_rng(5)
    c = 24
    y = rng.normal(size=(2, 3, 5, c))
    gamma, beta, rm, rv = rng.normal(size=c), rng.normal(size=c), rng.normal(size=c), rng.uniform(0.1, 2, c)
    rv[3] = 0.0
    eps = float(np.float32(1e-5))
    s, b = R.eval_affine(gamma, beta, rm, rv, 1e-5)
    out = F.batch_norm(nchw(y), torch.from_numpy(rm), torch.from_numpy(rv), torch.from_numpy(gamma), torch.from_numpy(beta), False, 0.0, eps)
    np.testing.assert_allclose(R.act(y, s, b), nhwc(out), rtol=1e-11, atol=1e-11)
    assert s[3] == gamma[3] / np.sqrt(eps)


def test_act_picks_the_constants_of_each_pass():
    rng = np.random.default_rng(6)
    n, c, gstride = 4, 8, 8 + 32
    y = rng.normal(size=(n, 3, 2, c))
    table_s, table_b = rng.normal(size=gstride + c), rng.normal(size=gstride + c)
    a = R.act(y, table_s, table_b, relu=True, gN=2, gstride=gstride)
    for i in range(n):
        o = (i // 2) * gstride
        want = torch.relu(torch.from_numpy(y[i]) * torch.from_numpy(table_s[o:o + c]) + torch.from_numpy(table_b[o:o + c])).numpy()
        np.testing.assert_array_equal(a[i], want)
    assert not np.array_equal(a[2], R.act(y, table_s, table_b, relu=True)[2])             # (pass 1's constants are not pass 0's)
    np.testing.assert_array_equal(R.act(y, table_s, table_b, relu=False)[3], y[3] * table_s[:c] + table_b[:c])     # gN = 0: row 0
    np.testing.assert_array_equal(R.act(y), y)                                                                      # no constants: no ReLU
    np.testing.assert_array_equal(R.act_magnitude(y, table_s, table_b, gN=2, gstride=gstride)[2],
                                  np.abs(y[2] * table_s[gstride:gstride + c]) + np.abs(table_b[gstride:gstride + c]))


@pytest.mark.parametrize("n,h,w,c", [(2, 4, 6, 3), (1, 5, 7, 2), (3, 2, 3, 1), (1, 2, 2, 4), (2, 9, 8, 5)])
def test_pool_and_route_equal_max_pool2d_autograd_with_ties(n, h, w, c):
    rng = np.random.default_rng(h * 10 + w)
    x = rng.choice(np.array([-1.0, 0.0, 0.5, 2.0]), size=(n, h, w, c))         # four values: ties in most windows
    dp = rng.normal(size=(n, h // 2, w // 2, c))
    xt = nchw(x).requires_grad_(True)
    p = F.max_pool2d(xt, 2)
    p.backward(nchw(dp))
    np.testing.assert_array_equal(R.pool2(x), nhwc(p))
    dx, best = R.maxpool_route(dp, x)
    np.testing.assert_array_equal(dx, nhwc(xt.grad))
    win = R._windows(x)
    tied = (win == win.max(axis=3, keepdims=True)).sum(axis=3) > 1
    assert tied.mean() >= 0.25
    if best.size >= 32:
        assert set(np.unique(best)) == {0, 1, 2, 3}
    if h % 2:
        assert not dx[:, -1].any()
    if w % 2:
        assert not dx[:, :, -1].any()


def test_route_takes_the_first_of_four_equal_values():
    x = np.zeros((1, 2, 2, 1))
    dx, best = R.maxpool_route(np.full((1, 1, 1, 1), 3.0), x)
    assert best.item() == 0 and dx[0, 0, 0, 0] == 3.0 and dx.sum() == 3.0
    x[0, 1, 0, 0] = x[0, 1, 1, 0] = 1.0                                       # the maximum twice in the second row: (1,0) wins
    dx, best = R.maxpool_route(np.full((1, 1, 1, 1), 3.0), x)
    assert best.item() == 2 and dx[0, 1, 0, 0] == 3.0 and dx.sum() == 3.0


@pytest.mark.parametrize("n,c,h,w", [(1, 4, 1, 1), (1, 4, 1, 3), (2, 8, 3, 1), (2, 12, 5, 7), (3, 4, 16, 16), (1, 1, 2, 2)])
def test_upsample_and_adjoint_equal_interpolate_autograd(n, c, h, w):
    rng = np.random.default_rng(h * 31 + w)
    x, dy = rng.normal(size=(n, h, w, c)), rng.normal(size=(n, 2 * h, 2 * w, c))
    xt = nchw(x).requires_grad_(True)
    yt = F.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=True)
    yt.backward(nchw(dy))
    y, dx = R.upsample2x(x), R.upsample2x_adjoint(dy)
    np.testing.assert_allclose(y, nhwc(yt), **TIGHT)
    np.testing.assert_allclose(dx, nhwc(xt.grad), **TIGHT)
    assert abs((y * dy).sum() - (x * dx).sum()) <= 1e-12 * (np.abs(y * dy).sum() + 1.0)
    for k in (h, w):                       # rows of the interpolation matrix sum to one; its support lies inside the touch set
        U, T = R.lerp_matrix(k), R.touch_matrix(k)
        np.testing.assert_allclose(U.sum(1), 1.0, rtol=1e-15)
        assert not (U[T == 0] != 0).any()
    if h == 1:
        np.testing.assert_array_equal(y[:, 0], y[:, 1])
