"""tests/nonfinite_ref.py pinned to torch's CPU semantics: the facts the non-finite GPU tests take as their reference."""
import torch
import torch.nn.functional as TF

import nonfinite_ref as NF

INF, NAN = float("inf"), float("nan")


def test_half_cast_overflows_at_65520():
    x = torch.tensor([65504.0, 65519.0, 65520.0, 2e6, -65519.0, -65520.0], dtype=torch.float64)
    assert NF.stored(x, "f16").tolist() == [65504.0, 65504.0, INF, INF, -65504.0, -INF]
    cls, val = NF.expect(x, "f16")
    assert cls.tolist() == [NF.FINITE, NF.FINITE, NF.PINF, NF.PINF, NF.FINITE, NF.NINF]
    assert val[:2].tolist() == [65504.0, 65504.0]
    # bf16 keeps f32's range: the same values stay finite and round to 8 significant bits
    cls, val = NF.expect(x, "bf16")
    assert cls.tolist() == [NF.FINITE] * 6 and val[0].item() == 65536.0


def test_classify():
    x = torch.tensor([0.0, -0.0, 1.5, INF, -INF, NAN, -NAN])
    assert NF.classify(x).tolist() == [0, 0, 0, NF.PINF, NF.NINF, NF.NAN, NF.NAN]


def test_conv_inf_times_zero_weight_is_nan():
    x = torch.ones(1, 2, 5, 5, dtype=torch.float64)
    x[0, 1, 2, 2] = INF
    w = torch.ones(3, 2, 3, 3, dtype=torch.float64)
    w[1, 1] = 0                                   # output channel 1 meets the inf with a zero weight
    w[2, 1] = -1
    y = TF.conv2d(x, w, padding=1)
    cls = NF.classify(y)
    cone = torch.zeros(5, 5, dtype=torch.bool)
    cone[1:4, 1:4] = True
    assert (cls[0, 0][cone] == NF.PINF).all() and (cls[0, 1][cone] == NF.NAN).all() and (cls[0, 2][cone] == NF.NINF).all()
    assert (cls[0][:, ~cone] == NF.FINITE).all()


def test_batchnorm_train_poisons_exactly_the_channel_with_an_inf():
    torch.manual_seed(0)
    x = torch.randn(2, 3, 4, 4, dtype=torch.float64)
    bn = torch.nn.BatchNorm2d(3).double().train()
    clean = bn(x).detach()
    rv_clean = bn.running_var.clone()
    bn2 = torch.nn.BatchNorm2d(3).double().train()
    xp = x.clone()
    xp[1, 1, 2, 3] = INF
    y = bn2(xp).detach()
    assert torch.isnan(y[:, 1]).all() and torch.isnan(bn2.running_var[1])
    for c in (0, 2):
        assert torch.equal(y[:, c], clean[:, c]) and bn2.running_var[c] == rv_clean[c]


def test_relu_and_max_pool_propagate_nan_in_torch():
    x = torch.tensor([[[[1.0, NAN], [-2.0, 3.0]]]], dtype=torch.float64)
    assert torch.isnan(torch.relu(x)[0, 0, 0, 1])
    assert torch.isnan(TF.max_pool2d(x, 2)).all()
    a = torch.tensor([NAN, -1.0, 2.0], dtype=torch.float64, requires_grad=True)
    torch.relu(a).backward(torch.tensor([5.0, 6.0, 7.0], dtype=torch.float64))
    assert a.grad.tolist() == [5.0, 0.0, 7.0]                  # relu'(nan) passes the gradient


def test_relu_conventions():
    a = torch.tensor([NAN, -NAN, -1.0, 0.0, 2.0, INF, -INF], dtype=torch.float64)
    g = torch.arange(1.0, 8.0, dtype=torch.float64)
    t, s = NF.relu(a, "torch"), NF.relu(a, "select")
    assert NF.classify(t).tolist() == [NF.NAN, NF.NAN, 0, 0, 0, NF.PINF, 0]
    assert s.tolist() == [0.0, 0.0, 0.0, 0.0, 2.0, INF, 0.0]
    assert NF.relu_bwd(a, g, "torch").tolist() == [1.0, 2.0, 0.0, 0.0, 5.0, 6.0, 0.0]
    assert NF.relu_bwd(a, g, "select").tolist() == [0.0, 0.0, 0.0, 0.0, 5.0, 6.0, 0.0]
    # the helper's torch convention IS autograd's
    ar = a.clone().requires_grad_()
    torch.relu(ar).backward(g)
    assert ar.grad.tolist() == NF.relu_bwd(a, g, "torch").tolist()


def test_mismatches_sees_class_and_bit_differences():
    ref = torch.tensor([1.0, 65520.0, NAN, 2049.0], dtype=torch.float64)       # 2049 rounds to 2048 in half
    good = torch.tensor([1.0, INF, NAN, 2048.0]).half()
    assert NF.mismatches(good, ref, "f16")[:2] == (0, 0)
    NF.assert_matches(good, ref, "f16")
    sat = torch.tensor([1.0, 65504.0, NAN, 2048.0]).half()                    # saturated instead of inf
    assert NF.mismatches(sat, ref, "f16")[:2] == (1, 0)
    zeroed = torch.tensor([1.0, INF, 0.0, 2050.0]).half()                     # NaN dropped, one wrong bit
    assert NF.mismatches(zeroed, ref, "f16")[:2] == (1, 1)
    assert NF.which_convention(good, {"torch": ref, "select": ref.nan_to_num(0.0)}, "f16") == ["torch"]
