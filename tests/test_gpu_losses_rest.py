"""utils/losses.py beside DiceLossWithMask on the device (csrc/consistency.hip through ustrun.functional) against
tests/losses_ref.py in float64 and against the reference's own results (g19_losses_rest.npz).

Bars.  Scalar values: rtol 2e-5, the bar of test_gpu_losses.py.  Maps and gradients: the restatement is also evaluated with torch
float32 on the CPU; its max-abs error against float64 is the yardstick of what f32 arithmetic costs at these inputs, and the
device's max-abs error must be <= max(4 x yardstick, 8 * 2^-24 * max|expected|) -- 4 for a different expf / logf and a different
summation tree, the floor eight f32 roundings of the largest value.  Both errors are printed (pytest -s)."""
import math

import numpy as np
import pytest
import torch

import losses_ref as R

pytestmark = pytest.mark.gpu

# (N,K,H,W): the 16-byte path; HW = 1221, one pixel per lane, unaligned planes; KMAX; K = 1 with HW < 4; a grid-stride loop that wraps
# with many partial rows; then HW % 4 == 0 tensors entered through a view one float into its buffer (first / second operand)
SHAPES = {"vec": (3, 2, 40, 40), "odd": (2, 4, 33, 37), "kmax": (1, 8, 5, 7), "k1": (2, 1, 3, 1), "big": (2, 3, 512, 512),
          "view_a": (2, 2, 8, 12), "view_b": (2, 2, 8, 12), "extreme": (1, 2, 4, 8)}
_cache = {}


def make_inputs(tag):
    """CPU float32 inputs of one shape, made once"""
    if tag in _cache:
        return _cache[tag]
    N, K, H, W = SHAPES[tag]
    g = torch.Generator().manual_seed(sum(map(ord, tag)))
    rn = lambda *s: torch.randn(*s, generator=g)
    z = {"a": 3 * rn(N, K, H, W), "b": 3 * rn(N, K, H, W), "gm": rn(N, K, H, W), "gm1": rn(N, 1, H, W),
         "ra": 3 * rn(7, 5), "rb": 3 * rn(7, 5)}
    if tag == "extreme":            # logits of +-60: probabilities that round to 0 and 1 in f32
        z["a"] = 60.0 * torch.sign(z["a"])
        z["b"] = 60.0 * torch.sign(z["b"])
        z["ra"], z["rb"] = 60.0 * torch.sign(z["ra"]), 60.0 * torch.sign(z["rb"])
    z["p"] = torch.softmax(3 * rn(N, K, H, W), dim=1)
    z["idx"] = torch.randint(0, K, (N, 1, H, W), generator=g)
    z["hot"] = torch.cat([z["idx"] == k for k in range(K)], dim=1).float()
    _cache[tag] = z
    return z


def one_float_in(t):
    """the same values in a contiguous tensor whose storage starts 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def on_device(case, z, shift_first=False, shift_second=False):
    from utils import losses  # noqa: F401
    fn, xa, xb, both, up = case
    x = z[xa].cuda()
    x = (one_float_in(x) if shift_first else x.clone()).requires_grad_(True)
    y = z[xb].cuda()
    if y.is_floating_point():
        y = (one_float_in(y) if shift_second else y.clone()).requires_grad_(both)
    v = fn(x, y)
    ((v * z[up].cuda()).sum() if up else v * R.UP).backward()
    return v.detach().cpu(), x.grad.cpu(), (y.grad.cpu() if both else None)


def compare(label, got, want64, yard32, scalar_value):
    """got: device results (value, ga, gb); want64 / yard32: the restatement in float64 / float32 on the CPU"""
    for part, g, w, y in zip(("value", "ga", "gb"), got, want64, yard32):
        if w is None:
            assert g is None
            continue
        assert g.shape == w.shape and g.dtype == torch.float32, (label, part)
        assert torch.isfinite(g).all(), (label, part)
        err = float((g.double() - w).abs().max())
        yard = float((y.double() - w).abs().max())
        top = float(w.abs().max())
        if part == "value" and scalar_value:
            print("%-44s %-5s err %.2e  yardstick %.2e  |expected| %.3e  (rtol 2e-5)" % (label, part, err, yard, top))
            assert err <= 2e-5 * top, (label, part, err, top)
        else:
            bar = max(4 * yard, 8 * 2.0 ** -24 * top)
            print("%-44s %-5s err %.2e  yardstick %.2e  bar %.2e" % (label, part, err, yard, bar))
            assert err <= bar, (label, part, err, yard, bar)


# every function at every shape; the sigmoid KL is left out at the +-60 logits (utils/losses.py: it differs from the reference there)
PAIRS = [(tag, name) for tag in SHAPES for name in R.cases(SHAPES[tag][1], R.Names)
         if not (tag == "extreme" and name == "softmax_kl_loss_sig")]


@pytest.mark.parametrize("tag,name", PAIRS)
def test_value_and_gradients_against_float64(tag, name):
    from utils import losses
    K = SHAPES[tag][1]
    z = make_inputs(tag)
    ref = R.cases(K, R.Names)[name]
    want = R.evaluate(ref, z, torch.float64)
    yard = R.evaluate(ref, z, torch.float32)
    got = on_device(R.cases(K, losses)[name], z, shift_first=tag == "view_a", shift_second=tag == "view_b")
    compare("%s %s %s" % (name, tag, SHAPES[tag]), got, want, yard, scalar_value=want[0].dim() == 0)


@pytest.mark.parametrize("name", ["entropy_loss", "entropy_loss_map"])
@pytest.mark.parametrize("tag", ["vec", "odd", "kmax"])
def test_entropy_over_ln_c(tag, name):
    from utils import losses
    K = SHAPES[tag][1]
    z = make_inputs(tag)
    up = "gm1" if name == "entropy_loss_map" else None
    C = max(K, 2)
    mk = lambda M: ((lambda x, _: getattr(M, name)(x, C=C)), "p", "idx", False, up)
    want, yard = R.evaluate(mk(R), z, torch.float64), R.evaluate(mk(R), z, torch.float32)
    compare("%s %s" % (name, SHAPES[tag]), on_device(mk(losses), z), want, yard, scalar_value=up is None)
    if K == 2:          # the default C
        d = lambda M: ((lambda x, _: getattr(M, name)(x)), "p", "idx", False, up)
        compare("%s default C" % name, on_device(d(losses), z), R.evaluate(d(R), z, torch.float64), R.evaluate(d(R), z), up is None)


@pytest.mark.parametrize("name,K", [(n, K) for K in R.KS for n in R.cases(K, R.Names)])
def test_against_the_reference_goldens(golden, name, K):
    from utils import losses
    g = golden("g19_losses_rest")
    tail = "_K%d" % K
    z = {k[3:-len(tail)]: torch.from_numpy(g[k]) for k in g.files if k.startswith("in_") and k.endswith(tail)}
    key = "%s_K%d" % (name, K)
    want = tuple(torch.from_numpy(g[key + s]).double() if key + s in g.files else None for s in ("_v", "_ga", "_gb"))
    ref = R.cases(K, R.Names)[name]
    w64, y32 = R.evaluate(ref, z, torch.float64), R.evaluate(ref, z, torch.float32)
    yard = tuple(None if w is None else w + (y.double() - e) for w, y, e in zip(want, y32, w64))      # the same yardstick, around the golden
    compare("golden " + key, on_device(R.cases(K, losses)[name], z), want, yard, scalar_value=want[0].dim() == 0)


def test_focal_gradient_keeps_the_detached_factor():
    """The reference's gradient has no derivative of (1 - pt)^gamma (losses.py:141).  A restatement that differentiates the factor
    is more than ten bars away from what the device returns."""
    from utils import losses
    z = make_inputs("vec")
    case = lambda f: (f, "a", "idx", False, None)
    kept = R.evaluate(case(lambda x, t: R.focal_loss(x, t)), z, torch.float64)
    yard = R.evaluate(case(lambda x, t: R.focal_loss(x, t)), z, torch.float32)
    full = R.evaluate(case(lambda x, t: R.focal_loss(x, t, detach=False)), z, torch.float64)
    got = on_device(case(lambda x, t: losses.FocalLoss()(x, t)), z)
    bar = max(4 * float((yard[1].double() - kept[1]).abs().max()), 8 * 2.0 ** -24 * float(kept[1].abs().max()))
    assert float((got[1].double() - kept[1]).abs().max()) <= bar
    assert float((got[1].double() - full[1]).abs().max()) > 10 * bar
    assert float(got[0]) == pytest.approx(float(full[0]), rel=2e-5)            # the value is the same either way


def test_focal_targets_and_two_dimensional_input():
    from utils import losses
    z = make_inputs("odd")
    a, idx = z["a"].cuda(), z["idx"].cuda()
    f = losses.FocalLoss(gamma=2, alpha=R.ALPHA_LIST[4])
    v4, v3 = f(a, idx), f(a, idx.squeeze(1))                                    # [N,1,H,W] and [N,H,W]
    flat = a.reshape(2, 4, -1).transpose(1, 2).reshape(-1, 4)                   # losses.py:133-135
    v2 = f(flat, idx.reshape(-1))
    want = float(R.focal_loss(z["a"].double(), z["idx"], 2, R.ALPHA_LIST[4]))
    assert torch.equal(v4, v3)
    assert float(v4) == pytest.approx(want, rel=2e-5) and float(v2) == pytest.approx(want, rel=2e-5)
    z2 = {"a": flat.cpu(), "idx": z["idx"].reshape(-1)}
    mk = lambda M: ((lambda x, t: M.FocalLoss(gamma=2, alpha=R.ALPHA_LIST[4])(x, t)), "a", "idx", False, None)
    compare("focal [M,K]", on_device(mk(losses), z2), R.evaluate(mk(R.Names), z2, torch.float64), R.evaluate(mk(R.Names), z2), True)


def test_compute_kl_loss_takes_its_softmax_over_the_last_dimension():
    from utils import losses
    g = torch.Generator().manual_seed(5)
    for shape in ((7, 5), (2, 3, 4, 6)):
        z = {"a": 3 * torch.randn(*shape, generator=g), "b": 3 * torch.randn(*shape, generator=g)}
        mk = lambda M: (M.compute_kl_loss, "a", "b", True, None)
        compare("compute_kl_loss %s" % (shape,), on_device(mk(losses), z), R.evaluate(mk(R), z, torch.float64), R.evaluate(mk(R), z), True)
        other = F_softmax_dim1_kl(z)
        assert len(shape) == 2 or abs(float(on_device(mk(losses), z)[0]) - other) > 1e-3 * abs(other)        # not the dim-1 softmax


def F_softmax_dim1_kl(z):
    a, b = z["a"].double(), z["b"].double()
    if a.dim() == 2:
        return float(R.compute_kl_loss(a, b))
    return float(R.compute_kl_loss(a.movedim(1, -1), b.movedim(1, -1)))


def test_dice_loss_shape_assertion_and_target_gradient():
    from utils import losses
    z = make_inputs("kmax")
    p, idx = z["p"].cuda(), z["idx"].cuda()
    with pytest.raises(AssertionError, match="predict & target shape do not match"):
        losses.DiceLoss(4)(p, idx)                                              # 8 planes against a 4-class one-hot
    with pytest.raises(AssertionError, match="predict & target shape do not match"):
        losses.DiceLoss(8)(p, idx.squeeze(1))
    assert float(losses.DiceLoss(8)(p, idx.float())) == float(losses.DiceLoss(8)(p, idx))        # float or int class indices
    t = z["hot"].cuda().requires_grad_(True)
    for call in (lambda: losses.dice_loss(p, t), lambda: losses.dice_loss1(p, t)):
        with pytest.raises(RuntimeError, match="first argument only"):
            call()
    with pytest.raises(RuntimeError, match="classes"):
        losses.softmax_mse_loss(torch.zeros(1, 9, 2, 2, device="cuda"), torch.zeros(1, 9, 2, 2, device="cuda"))


def test_detached_second_argument_gets_no_gradient_buffer():
    from utils import losses
    a = torch.randn(4, 4, 256, 256, device="cuda", requires_grad=True)          # 4 MiB
    b = torch.randn(4, 4, 256, 256, device="cuda")
    room = {}
    for both in (False, True):
        a.grad = None
        t = b.clone().requires_grad_(both)
        loss = losses.softmax_kl_loss(a, t if both else t.detach())
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss.backward()
        torch.cuda.synchronize()
        room[both] = torch.cuda.max_memory_allocated() - before
        assert a.grad is not None and (t.grad is not None) == both
    nbytes = a.numel() * 4
    assert room[False] < 1.5 * nbytes <= 2 * nbytes <= room[True] < 2.5 * nbytes


def test_same_tensor_twice_noncontiguous_no_grad_and_half():
    from utils import losses
    z = make_inputs("vec")
    # the same tensor as both arguments: autograd adds the two sides
    x = z["a"].cuda().requires_grad_(True)
    (losses.softmax_mse_loss(x, x, sigmoid=True) * z["gm"].cuda()).sum().backward()
    assert float(x.grad.abs().max()) == 0.0                                     # (pa - pa)^2: both sides vanish
    twice = lambda M: ((lambda u, _: M.symmetric_mse_loss(u, u) + M.softmax_dice_loss(u, u) + M.softmax_kl_loss(u, 2 * u)), "a", "idx", False, None)
    compare("one tensor twice", on_device(twice(losses), z), R.evaluate(twice(R), z, torch.float64), R.evaluate(twice(R), z), True)
    # a non-contiguous input is made contiguous
    assert not z["a"].cuda().transpose(2, 3).is_contiguous()
    turned = lambda M: ((lambda u, v: M.softmax_kl_loss(u.transpose(2, 3), v.transpose(2, 3))), "a", "b", True, None)
    compare("transposed views", on_device(turned(losses), z), R.evaluate(turned(R), z, torch.float64), R.evaluate(turned(R), z), True)
    # no_grad: a plain value
    with torch.no_grad():
        m = losses.softmax_mse_loss(x, z["b"].cuda())
        e = losses.entropy_minmization(z["p"].cuda())
    assert not m.requires_grad and not e.requires_grad and m.shape == x.shape and e.dim() == 0
    # 16-bit inputs are out of scope: they raise
    with pytest.raises(RuntimeError, match="expected a float32 HIP tensor"):
        losses.softmax_mse_loss(x.half(), x.half())
    with pytest.raises(RuntimeError, match="expected a float32 HIP tensor"):
        losses.entropy_map(z["p"].cuda().half())


def test_three_dimensional_volumes_count_as_pixels():
    from utils import losses
    z = make_inputs("vec")
    vol = lambda t: t.reshape(3, -1, 4, 10, 40)
    a, b = z["a"].cuda(), z["b"].cuda()
    assert torch.equal(losses.softmax_mse_loss(vol(a), vol(b)), vol(losses.softmax_mse_loss(a, b)))
    assert torch.equal(losses.softmax_kl_loss(vol(a), vol(b)), losses.softmax_kl_loss(a, b))
    assert losses.entropy_map(vol(z["p"].cuda())).shape == (3, 1, 4, 10, 40)


def test_repeated_calls_are_bit_identical():
    from utils import losses
    z = make_inputs("big")
    for name, case in R.cases(3, losses).items():
        first, second = on_device(case, z), on_device(case, z)
        for u, v in zip(first, second):
            assert (u is None and v is None) or torch.equal(u, v), name


def test_consistency_term_trains_a_student():
    from networks.unet_model import UNet
    from utils import losses
    torch.manual_seed(0)
    student, teacher = UNet(1, 2, base_channels=8).cuda().train(), UNet(1, 2, base_channels=8).cuda().train()
    x = torch.randn(2, 1, 32, 32, device="cuda")
    losses.softmax_mse_loss(student(x), teacher(x).detach()).mean().backward()
    grads = [p.grad for p in student.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    assert sum(float(g.abs().sum()) for g in grads) > 0 and float(grads[0].abs().max()) > 0
    assert all(p.grad is None for p in teacher.parameters())
