"""CPU: tests/frozen_bn_ref.py (the float64 restatement the GPU tests of ustrun_bn_bwd_frozen compare against) is torch's own
float64 autograd through F.batch_norm(training=False) -> relu (-> max_pool2d(2) for the pooled form)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from frozen_bn_ref import frozen_bn_bwd

EPS = 1e-5


def _case(n, h, w, c, seed, pooled, with_da=True):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    gamma = (1 + 0.5 * torch.randn(c, generator=g, dtype=torch.float64))        # some negative scales among them
    gamma[0] = -gamma[0].abs()
    beta = 0.2 * torch.randn(c, generator=g, dtype=torch.float64)
    rm = 0.3 * torch.randn(c, generator=g, dtype=torch.float64)
    rv = 0.5 + 1.5 * torch.rand(c, generator=g, dtype=torch.float64)
    da = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) if with_da else None
    dp = torch.randn(n, c, h // 2, w // 2, generator=g, dtype=torch.float64) if pooled else None
    return y, gamma, beta, rm, rv, da, dp


def _autograd(y, gamma, beta, rm, rv, da, dp):
    y = y.clone().requires_grad_(True)
    gamma, beta = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm0, rv0 = rm.clone(), rv.clone()
    a = F.relu(F.batch_norm(y, rm0, rv0, gamma, beta, training=False, eps=EPS))
    outs, grads = [], []
    if da is not None:
        outs.append(a); grads.append(da)
    if dp is not None:
        outs.append(F.max_pool2d(a, 2)); grads.append(dp)
    torch.autograd.backward(outs, grads)
    assert torch.equal(rm0, rm) and torch.equal(rv0, rv)            # frozen: the buffers do not move
    return y.grad, gamma.grad, beta.grad


def _nhwc(t):
    return None if t is None else t.permute(0, 2, 3, 1).contiguous().numpy()


@pytest.mark.parametrize("n,h,w,c,pooled,with_da", [(1, 1, 1, 4, False, True), (2, 16, 16, 8, False, True), (3, 5, 7, 24, False, True),
                                                     (2, 5, 7, 8, True, True), (1, 6, 4, 4, True, True), (2, 8, 8, 4, True, False),
                                                     (2, 3, 2, 4, True, True)])
def test_restatement_is_torch_float64_autograd(n, h, w, c, pooled, with_da):
    y, gamma, beta, rm, rv, da, dp = _case(n, h, w, c, 100 * h + w + c, pooled, with_da)
    want_dy, want_dg, want_db = _autograd(y, gamma, beta, rm, rv, da, dp)
    rstd = 1.0 / torch.sqrt(rv + EPS)
    scale = gamma * rstd
    shift = beta - rm * scale
    dy, dg, db = frozen_bn_bwd(_nhwc(da), _nhwc(dp), _nhwc(y), scale.numpy(), shift.numpy(), rm.numpy(), rstd.numpy())
    # float64 on both sides, the same formulas in a different association: a few ulps of the values
    np.testing.assert_allclose(dy, _nhwc(want_dy), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(dg, want_dg.numpy(), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(db, want_db.numpy(), rtol=1e-11, atol=1e-12)


def test_ties_go_to_the_first_pixel_of_the_window():
    """all four activations of a window equal and positive, and all four clipped to zero: torch routes the pooled gradient to
    pixel (0, 0); clipped pixels then lose it to the ReLU mask"""
    c = 4
    y = torch.ones(1, c, 2, 4, dtype=torch.float64)
    y[:, :, :, 2:] = -1.0                                           # second window: every activation clipped
    gamma, beta = torch.ones(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)
    rm, rv = torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64) - EPS
    dp = torch.full((1, c, 1, 2), 3.0, dtype=torch.float64)
    want_dy, want_dg, want_db = _autograd(y, gamma, beta, rm, rv, None, dp)
    dy, dg, db = frozen_bn_bwd(None, _nhwc(dp), _nhwc(y), np.ones(c), np.zeros(c), np.zeros(c), np.ones(c))
    assert np.array_equal(dy, _nhwc(want_dy))
    assert dy[0, 0, 0, 0] == 3.0 and dy.sum() == 3.0 * c
    np.testing.assert_allclose(dg, want_dg.numpy(), rtol=1e-12)
    np.testing.assert_allclose(db, want_db.numpy(), rtol=1e-12)
