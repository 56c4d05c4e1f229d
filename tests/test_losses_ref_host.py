"""tests/losses_ref.py, the restatement the GPU tests of utils/losses.py compare against, is itself pinned to the reference's own
float32 results (g19_losses_rest.npz, tools/gen_losses_goldens.py); the public surface of utils/losses.py is pinned to the
names and signatures recorded from the reference in the same file; nothing in it runs on a CPU tensor."""
import inspect
import math

import numpy as np
import pytest
import torch

import losses_ref as R

CASES = [(name, K) for K in R.KS for name in R.cases(K, R.Names)]


@pytest.fixture(scope="module")
def g19(request):
    from conftest import load_golden
    return load_golden("g19_losses_rest")


def golden_inputs(g, K):
    tail = "_K%d" % K
    return {k[3:-len(tail)]: torch.from_numpy(g[k]) for k in g.files if k.startswith("in_") and k.endswith(tail)}


@pytest.mark.parametrize("name,K", CASES)
def test_restatement_in_float32_equals_the_reference(g19, name, K):
    """Values to rtol 2e-5, gradients to 2e-6 max|g|: the reference's own f32-against-f64 error stays below 1e-6 max|g| at
    these inputs (the generator prints it)."""
    v, ga, gb = R.evaluate(R.cases(K, R.Names)[name], golden_inputs(g19, K))
    key = "%s_K%d" % (name, K)
    np.testing.assert_allclose(v.numpy(), g19[key + "_v"], rtol=2e-5, atol=0)
    for got, want in ((ga, g19[key + "_ga"]),) + (((gb, g19[key + "_gb"]),) if gb is not None else ()):
        assert np.abs(got.numpy() - want).max() <= 2e-6 * np.abs(want).max()
    assert (gb is None) == (key + "_gb" not in g19.files)


def test_entropy_loss_is_the_entropy_over_ln_c():
    p = torch.softmax(torch.randn(2, 4, 5, 3, dtype=torch.float64), dim=1)
    assert torch.equal(R.entropy_loss(p, C=4), R.entropy_minmization(p) / math.log(4))
    assert torch.equal(R.entropy_loss_map(p, C=4), R.entropy_map(p) / math.log(4))
    assert torch.equal(R.entropy_loss(p), R.entropy_minmization(p) / math.log(2)) and R.entropy_map(p).shape == (2, 1, 5, 3)
    u = torch.full((1, 4, 2, 2), 0.25, dtype=torch.float64)
    assert abs(float(R.entropy_loss(u, C=4)) - 1.0) < 1e-5                 # the uniform map has entropy ln C


def test_kl_term_is_zero_where_the_target_probability_is_zero():
    a = torch.tensor([[60.0, -60.0]]).reshape(1, 2, 1, 1)
    assert float(R.softmax_kl_loss(-a, a)) == pytest.approx(60.0, rel=1e-6)      # (1 * (0 - -120) + 0) / 2
    assert float(R.compute_kl_loss(a.reshape(1, 2), a.reshape(1, 2))) == 0.0


def _signature(obj):
    s = str(inspect.signature(obj))
    return s + " forward" + str(inspect.signature(obj.forward)) if inspect.isclass(obj) else s


def test_public_names_and_signatures_match_the_reference(g19):
    from utils import losses
    names = [str(n) for n in g19["names"]]
    assert len(names) == 14 and "DiceLossWithMask" in names
    for name, sig in zip(names, g19["signatures"]):
        assert hasattr(losses, name), name
        assert _signature(getattr(losses, name)) == str(sig), name


def test_every_function_refuses_a_cpu_tensor():
    from utils import losses
    x, y = torch.randn(2, 2, 4, 4), torch.randn(2, 2, 4, 4)
    p, idx = torch.softmax(x, dim=1), torch.zeros(2, 1, 4, 4, dtype=torch.int64)
    calls = {"dice_loss": lambda: losses.dice_loss(p, y), "dice_loss1": lambda: losses.dice_loss1(p, y),
             "entropy_loss": lambda: losses.entropy_loss(p), "entropy_loss_map": lambda: losses.entropy_loss_map(p),
             "entropy_minmization": lambda: losses.entropy_minmization(p), "entropy_map": lambda: losses.entropy_map(p),
             "softmax_dice_loss": lambda: losses.softmax_dice_loss(x, y), "softmax_mse_loss": lambda: losses.softmax_mse_loss(x, y),
             "softmax_kl_loss": lambda: losses.softmax_kl_loss(x, y), "symmetric_mse_loss": lambda: losses.symmetric_mse_loss(x, y),
             "FocalLoss": lambda: losses.FocalLoss()(x, idx), "DiceLoss": lambda: losses.DiceLoss(2)(p, idx),
             "compute_kl_loss": lambda: losses.compute_kl_loss(x, y)}
    assert len(calls) == 13
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
