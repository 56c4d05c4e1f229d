"""GPU: the gradient of the DeepLabV2-ResNet's input image -- ustrun_conv_stem_dgrad (csrc/conv_stem_dgrad.hip: the input gradient of
Conv2d(3, 64, 7, stride=2, padding=3, bias=False), reference networks/backbone/resnet.py:124,160) alone, and `x.grad` through
DeepLabV2.forward (ustrun.resnet_engine.DeepLabFn) against torch autograd over the CPU oracle, with frozen parameters, for a grey image
and in eval mode."""
import copy
import functools

import pytest
import torch

from test_gpu_deeplab_bwd import _field_stats, rel

pytestmark = pytest.mark.gpu

TILE = 32            # stem_dgrad_plan.h: SD_T x SD_T input pixels per block (tests/test_stem_dgrad_plan_host.py compares the two)
_ST = {"f32": (torch.float32, 0), "bf16": (torch.bfloat16, 1), "f16": (torch.float16, 2), "f32x3": (torch.float32, 3)}


def out_extent(h):
    return (h - 1) // 2 + 1


def dgrad(dy, w, h, wd, dtype, dx=None):
    """dy [N,Ho,Wo,Cout] in the storage type (device), w [Cout,3,7,7] f32 (device) -> dx [N,3,H,W] f32"""
    from ustrun import _lib as L
    n, ho, wo, cout = dy.shape
    assert (ho, wo) == (out_extent(h), out_extent(wd))
    if dx is None:
        dx = torch.full((n, w.shape[1], h, wd), float("nan"), device=dy.device)           # overwritten, not accumulated
    L.check(L.lib().ustrun_conv_stem_dgrad(dy.data_ptr(), w.data_ptr(), n, h, wd, cout, w.shape[1], dx.data_ptr(), _ST[dtype][1],
                                           torch.cuda.current_stream().cuda_stream), "ustrun_conv_stem_dgrad")
    return dx


def dgrad_ref(dy, w, h, wd):
    """float64 on the CPU, on the values as stored"""
    return torch.nn.grad.conv2d_input((dy.shape[0], w.shape[1], h, wd), w.double().cpu(), dy.double().cpu().permute(0, 3, 1, 2).contiguous(),
                                      stride=2, padding=3)


# ---- 1-3. the operator -----------------------------------------------------------------------------------------------------
# (1, 1, 1): one input pixel under one output pixel, everything else of the patch is halo; (1, 75, 51): both extents odd (the last input
# row and column lie beyond the last output's centre); (2, 2 TILE + 3, TILE + 5): three tiles down with 3 rows in the last, two across
# with 5 columns
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (1, 7, 7), (2, 32, 32), (1, 75, 51), (3, 17, 6), (2, 2 * TILE + 3, TILE + 5)])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "f32x3"])
def test_operator_exact_on_small_integers(dtype, n, h, w):
    """dy and w are integers in -2..2: every product and every partial sum (|.| <= 4 * 16 * 64) is exact in every storage type, so the
    result equals the float64 one bit for bit whatever the summation order.  Cout 8 and 24: one partial 32-channel chunk (two of its
    4-channel groups: two waves idle; six: two waves with two groups, two with one); 64: two whole chunks."""
    g = torch.Generator().manual_seed(2000 + 31 * h + w)
    for cout in (8, 24, 64):
        dy = torch.randint(-2, 3, (n, out_extent(h), out_extent(w), cout), generator=g).to(_ST[dtype][0]).cuda()
        wt = torch.randint(-2, 3, (cout, 3, 7, 7), generator=g).float().cuda()
        got = dgrad(dy, wt, h, w, dtype).cpu()
        want = dgrad_ref(dy, wt, h, w)
        assert torch.equal(got.double(), want), (cout, float((got.double() - want).abs().max()))


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "f32x3"])
def test_operator_random_values_and_repeats(dtype):
    """real values: against float64 on the same rounded operands, rel-L2 < 1e-5 (f32 accumulation of <= 16 * 64 terms); two launches
    give the same bits; dx is overwritten (it starts as NaN)"""
    g = torch.Generator().manual_seed(78)
    h, w = 133, 90                                      # dy [2, 67, 45, 64]: an odd and an even input extent, 5 x 3 tiles
    dy = torch.randn(2, 67, 45, 64, generator=g).to(_ST[dtype][0]).cuda()
    wt = (0.1 * torch.randn(64, 3, 7, 7, generator=g)).cuda()
    a, b = dgrad(dy, wt, h, w, dtype), dgrad(dy, wt, h, w, dtype)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
    err = rel(a.cpu(), dgrad_ref(dy, wt, h, w))
    print(f"conv_stem_dgrad {dtype}: rel-L2 against float64 {err:.2e}")
    assert err < 1e-5, err


def test_operator_refuses_other_channel_counts():
    from ustrun import _lib as L
    dy = torch.zeros(1, 4, 4, 72).cuda()
    wt = torch.zeros(72, 4, 7, 7).cuda()
    dx = torch.zeros(1, 4, 8, 8).cuda()
    rc = L.lib().ustrun_conv_stem_dgrad(dy.data_ptr(), wt.data_ptr(), 1, 8, 8, 8, 4, dx.data_ptr(), 0, None)
    assert rc != 0 and b"conv_stem_dgrad" in L.lib().ustrun_last_error() and b"Cin=4" in L.lib().ustrun_last_error()
    rc = L.lib().ustrun_conv_stem_dgrad(dy.data_ptr(), wt.data_ptr(), 1, 8, 8, 72, 3, dx.data_ptr(), 0, None)
    assert rc != 0 and b"Cout=72" in L.lib().ustrun_last_error()


# ---- 4-6. the network against the oracle ---------------------------------------------------------------------------------------
def _state_dict(K, bn3_scale):
    from oracle import deeplab_ref as D
    sd = D.make_state_dict("resnet50", K, 23)
    if bn3_scale != 1:
        for k in sd:
            if k.endswith("bn3.weight"):
                sd[k] = sd[k] * bn3_scale
    return sd


def _oracle_run(x, sd, R, dt):
    """test_gpu_deeplab_bwd._oracle_grads' construction with x a leaf too: {parameter key or 'x': gradient}"""
    from oracle import deeplab_ref as D
    sdo = {}
    for k, v in sd.items():
        v = v.clone().to(dt) if v.is_floating_point() else v.clone()
        sdo[k] = v.requires_grad_(True) if v.is_floating_point() and "running" not in k else v
    xx = x.detach().clone().to(dt).requires_grad_(True)         # (a leaf of its own: the cached x stays as it is)
    out = D.deeplabv2_forward(xx, sdo, "resnet50", True)
    (out * R.to(dt)).sum().backward()
    gr = {k: v.grad for k, v in sdo.items() if v.requires_grad}
    gr["x"] = xx.grad
    return gr


@functools.lru_cache(maxsize=None)
def oracle_case(h, w, K, bn3_scale=1.0):
    """(state dict, x, R, float64 oracle gradients) of test_deeplab_backward_vs_oracle_f32's / _bf16's case: computed once per shape
    and shared, never modified"""
    sd = _state_dict(K, bn3_scale)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, h, w, generator=g)
    R = torch.randn(2, K, h, w, generator=g)
    return sd, x, R, _oracle_run(x, sd, R, torch.float64)


@functools.lru_cache(maxsize=None)
def x_yardstick(h, w, K):
    """(rel-L2, cosine) of the float32 oracle's x.grad against the float64 oracle's"""
    sd, x, R, g64 = oracle_case(h, w, K)
    g32 = _oracle_run(x, sd, R, torch.float32)
    e, _, cos, _ = _field_stats({"x": g32["x"]}, {"x": g64["x"]})
    return e, cos


def hip_run(sd, dtype, x, R, x_grad=True, allow_nonfinite=False):
    """({parameter key: gradient}, x.grad) of one forward + backward of the HIP network, loss <logits, R>"""
    from networks.deeplabv2 import DeepLabV2
    m = DeepLabV2("resnet50", R.shape[1], pretrained=False, dtype=dtype)
    m.load_state_dict(sd)
    m = m.cuda().train()
    xg = x.detach().cuda().requires_grad_(x_grad)
    out = m(xg)
    assert out.requires_grad
    (out * R.cuda()).sum().backward()
    got = {k: p.grad for k, p in m.named_parameters()}
    assert all(v is not None for v in got.values())
    if x_grad:
        assert xg.grad is not None and xg.grad.shape == x.shape
        assert allow_nonfinite or torch.isfinite(xg.grad).all()
    return got, (xg.grad.cpu() if x_grad else xg.grad)


def _check_f32_level(dtype, h, w, K):
    sd, x, R, g64 = oracle_case(h, w, K)
    yerr, ycos = x_yardstick(h, w, K)
    assert 0.0 < yerr < 0.5, yerr                       # (the bar means something)
    pg, xg = hip_run(sd, dtype, x, R)
    err, _, cos, ratio = _field_stats({"x": xg}, {"x": g64["x"]})
    print(f"deeplab x.grad {dtype} {h}x{w} K={K}: rel-L2 {err:.3e}, cosine {cos:.6f}, norm ratio {ratio:.4f} against the f64 oracle; "
          f"f32 oracle: rel-L2 {yerr:.3e}, cosine {ycos:.6f}")
    assert err <= 2 * yerr and cos >= ycos - 5e-4, (err, yerr, cos, ycos)
    return sd, x, R, pg


@pytest.mark.parametrize("h,w,K", [(96, 80, 2), (100, 76, 2)])
def test_input_gradient_vs_oracle_f32(h, w, K):
    """resnet50, train mode, loss <logits, R>: x.grad against torch autograd over the CPU oracle in float64 with x a leaf, held to the
    bars of test_deeplab_backward_vs_oracle_f32 -- rel-L2 <= 2x the float32 oracle's own against float64, cosine >= the float32
    oracle's - 5e-4.  (On the CPU the float32 oracle's x.grad sits 2.3e-2 / 1.7e-2 rel-L2 from the float64 one at 96 x 80 / 100 x 76,
    cosine 0.99973 / 0.99985: neither zero nor near 1, so the bar means something.)  100 x 76 makes the stem's output 50 x 38 and the
    pooled map 25 x 19.  Asking for x.grad moves no bit of a parameter gradient, and without it x.grad stays None."""
    sd, x, R, pg = _check_f32_level("f32", h, w, K)
    plain, none = hip_run(sd, "f32", x, R, x_grad=False)
    assert none is None
    for kk in pg:
        assert torch.equal(pg[kk], plain[kk]), kk


def test_input_gradient_vs_oracle_f32x3():
    _check_f32_level("f32x3", 96, 80, 2)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_input_gradient_vs_oracle_16bit(dtype):
    """The conditioning of test_deeplab_backward_vs_oracle_bf16 (every bn3.weight x 0.25).  Yardstick: the f32 HIP path on parameters
    and input rounded to the 16-bit type, against the float64 oracle; the 16-bit path, which also rounds every stored activation and
    gradient, must keep x.grad within 2.5x of the yardstick's rel-L2 and 4x of its 1 - cosine -- the factors the parameter gradients
    of this same run are held to.  f16 carries the loss scale with the back-off of test_deeplab_backward_vs_oracle_f16.  Measured:
    bf16 rel-L2 0.511 against the yardstick's 0.352 (ratio 1.45), 1 - cosine 0.132 against 0.063 (2.10); f16 0.181 against 0.120
    (1.51), 0.0164 against 0.0072 (2.28), at loss scale 64."""
    td = torch.bfloat16 if dtype == "bf16" else torch.float16
    sd, x, R, g64 = oracle_case(96, 80, 2, 0.25)
    scale = 64.0 if dtype == "f16" else 1.0
    for _ in range(10):
        pg, xg = hip_run(sd, dtype, x, R * scale, allow_nonfinite=True)
        if bool(torch.isfinite(xg).all()) and all(bool(torch.isfinite(v).all()) for v in pg.values()):
            break
        scale *= 0.25
    assert torch.isfinite(xg).all()
    xg = xg / scale
    sdr = {k: (v.to(td).float() if v.is_floating_point() and v.dim() == 4 else v) for k, v in sd.items()}
    _, yard = hip_run(sdr, "f32", x.to(td).float(), R)
    err, _, cos, ratio = _field_stats({"x": xg}, {"x": g64["x"]})
    yerr, _, ycos, _ = _field_stats({"x": yard}, {"x": g64["x"]})
    print(f"deeplab x.grad {dtype} (loss scale {scale}): rel-L2 {err:.3e}, cosine {cos:.5f}, norm ratio {ratio:.3f} against the f64 oracle; "
          f"f32 path on rounded parameters + input: rel-L2 {yerr:.3e}, cosine {ycos:.5f}; ratios {err / yerr:.2f}, "
          f"{(1 - cos) / (1 - ycos):.2f}")
    assert err < 2.5 * yerr and (1 - cos) < 4 * (1 - ycos), (err, yerr, cos, ycos)


# ---- 7-9. frozen parameters, a grey image, eval mode -----------------------------------------------------------------------------
def _small_model(dtype="f32", seed=5):
    from networks.deeplabv2 import DeepLabV2
    torch.manual_seed(seed)
    return DeepLabV2("resnet50", 2, pretrained=False, dtype=dtype).cuda().train()


def test_frozen_parameters_record_the_node_for_x_alone():
    m = _small_model()
    twin = copy.deepcopy(m)
    for p in m.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 64, 64, generator=g).cuda()
    R = torch.randn(2, 2, 64, 64, generator=g).cuda()
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    out = m(xa)
    assert out.grad_fn is not None
    (out * R).sum().backward()
    (twin(xb) * R).sum().backward()
    assert xa.grad is not None and torch.isfinite(xa.grad).all() and float(xa.grad.abs().max()) > 0
    assert torch.equal(xa.grad, xb.grad)
    assert all(p.grad is None for p in m.parameters())
    assert all(p.grad is not None for p in twin.parameters())


def test_grey_input_gradient_is_the_channel_sum():
    m = _small_model()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 1, 64, 64, generator=g).cuda()
    R = torch.randn(2, 2, 64, 64, generator=g).cuda()
    x1 = x.clone().requires_grad_()
    (m(x1) * R).sum().backward()
    assert x1.grad is not None and x1.grad.shape == x.shape
    x3 = x.expand(-1, 3, -1, -1).contiguous().requires_grad_()
    (m(x3) * R).sum().backward()
    e = rel(x1.grad.cpu(), x3.grad.sum(1, keepdim=True).cpu())
    print(f"grey x.grad against the channel sum: rel-L2 {e:.2e}")
    assert e < 1e-6, e


def test_eval_mode_input_gradient_is_refused():
    m = _small_model().eval()
    for p in m.parameters():
        p.requires_grad_(False)
    x = torch.zeros(1, 3, 64, 64).cuda().requires_grad_()
    with pytest.raises(NotImplementedError, match="eval mode"):
        m(x)
    with torch.no_grad():                               # no graph asked for: the plain forward
        assert m(x).shape == (1, 2, 64, 64)
