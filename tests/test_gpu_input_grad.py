"""GPU: the gradient of the network input (ustrun_conv_first_dgrad behind ustrun_unet_backward_io) and of the feature output
(`forward(x, feature=True)` returns two ordinary autograd tensors, reference networks/unet_model.py:25-39)."""
import copy
import functools

import pytest
import torch

from oracle import unet_ref as U
from test_gpu_unet import YARD_X, build_model, rel_l2

pytestmark = pytest.mark.gpu

TILE = 16            # conv_first_dgrad.hip: DT x DT output pixels per block, 32 channels of dy per chunk
_ST = {"f32": (torch.float32, 0), "bf16": (torch.bfloat16, 1), "f16": (torch.float16, 2), "f32x3": (torch.float32, 3)}


def dgrad(dy, w, dtype):
    """dy [N,H,W,Cout] in the storage type (device), w [Cout,Cin,3,3] f32 (device) -> dx [N,Cin,H,W] f32"""
    from ustrun import _lib as L
    n, h, wd, cout = dy.shape
    cin = w.shape[1]
    dx = torch.full((n, cin, h, wd), float("nan"), device=dy.device)           # overwritten, not accumulated
    L.check(L.lib().ustrun_conv_first_dgrad(dy.data_ptr(), w.data_ptr(), n, h, wd, cout, cin, dx.data_ptr(), _ST[dtype][1],
                                            torch.cuda.current_stream().cuda_stream), "ustrun_conv_first_dgrad")
    return dx


def dgrad_ref(dy, w):
    """float64 on the CPU, on the values as stored"""
    n, h, wd, _ = dy.shape
    return torch.nn.grad.conv2d_input((n, w.shape[1], h, wd), w.double().cpu(), dy.double().cpu().permute(0, 3, 1, 2).contiguous(),
                                      padding=1)


# ---- 1. the operator -------------------------------------------------------------------------------------------------
# (2, 35, 21): both extents exceed the 16 x 16 tile by a non-multiple (three tiles down with 3 rows in the last, two across with 5
# columns); (1, 50, 38) and (3, 17, 5) do too, (1, 1, 1) is all halo
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (2, 16, 16), (1, 50, 38), (3, 17, 5), (2, 2 * TILE + 3, TILE + 5)])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "f32x3"])
def test_operator_exact_on_small_integers(dtype, n, h, w):
    """dy and w are integers in -2..2: every product and every partial sum (|.| <= 4 * 576) is exact in every storage type, so the
    result equals the float64 one bit for bit whatever the summation order."""
    g = torch.Generator().manual_seed(1000 + 31 * h + w)
    for cin in (1, 3, 4):
        for cout in (8, 24, 64):
            dy = torch.randint(-2, 3, (n, h, w, cout), generator=g).to(_ST[dtype][0]).cuda()
            wt = torch.randint(-2, 3, (cout, cin, 3, 3), generator=g).float().cuda()
            got = dgrad(dy, wt, dtype).cpu()
            want = dgrad_ref(dy, wt)
            assert torch.equal(got.double(), want), (cin, cout, float((got.double() - want).abs().max()))


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "f32x3"])
def test_operator_random_values_and_repeats(dtype):
    """real values: against float64 on the same rounded operands, rel-L2 < 1e-5 (f32 accumulation of <= 576 terms); two launches
    give the same bits"""
    g = torch.Generator().manual_seed(77)
    dy = torch.randn(2, 33, 29, 64, generator=g).to(_ST[dtype][0]).cuda()
    wt = (0.1 * torch.randn(64, 3, 3, 3, generator=g)).cuda()
    a, b = dgrad(dy, wt, dtype), dgrad(dy, wt, dtype)
    assert torch.equal(a, b)
    err = rel_l2(a.cpu(), dgrad_ref(dy, wt))
    print(f"conv_first_dgrad {dtype}: rel-L2 against float64 {err:.2e}")
    assert err < 1e-5, err


def test_operator_refuses_five_input_channels():
    from ustrun import _lib as L
    dy = torch.zeros(1, 4, 4, 8).cuda()
    wt = torch.zeros(8, 5, 3, 3).cuda()
    dx = torch.zeros(1, 5, 4, 4).cuda()
    rc = L.lib().ustrun_conv_first_dgrad(dy.data_ptr(), wt.data_ptr(), 1, 4, 4, 8, 5, dx.data_ptr(), 0, None)
    assert rc != 0 and b"Cin=5" in L.lib().ustrun_last_error()


# ---- 2 / 3. the network against the oracle -----------------------------------------------------------------------------
LOSSES = {"logits": lambda lg, ft: lg.square().mean(), "feat": lambda lg, ft: ft.square().mean(),
          "both": lambda lg, ft: lg.square().mean() + ft.square().mean()}


def _inputs(c, k, n, h, w, base, seed, bilinear=False):
    """the construction of test_gpu_unet.run_pair: seeded state dict with a non-trivial BatchNorm affine, seeded input"""
    torch.manual_seed(seed)
    sd = U.make_state_dict(c, k, bilinear=bilinear, base=base)
    g = torch.Generator().manual_seed(seed + 1)
    for key in sd:
        if key.endswith(("1.weight", "4.weight")) and sd[key].dim() == 1:
            sd[key] = 1 + 0.5 * torch.randn(sd[key].shape, generator=g)
        if key.endswith(("1.bias", "4.bias")) and sd[key].dim() == 1 and "double_conv" in key:
            sd[key] = 0.2 * torch.randn(sd[key].shape, generator=g)
    return sd, torch.randn(n, c, h, w, generator=g)


@functools.lru_cache(maxsize=None)
def oracle_grads(c, k, n, h, w, base, seed, bilinear=False):
    """{loss: {parameter key or 'x': (f32 CPU gradient, f64 gradient)}}: ONE f32 and ONE f64 forward of the oracle, a backward per
    loss; computed once per shape and shared by the tests below"""
    sd, x = _inputs(c, k, n, h, w, base, seed, bilinear)
    out = {}
    per = []
    for dt in (torch.float32, torch.float64):
        s = {kk: (v.to(dt) if v.is_floating_point() else v.clone()) for kk, v in sd.items()}
        keys = U.param_keys(s)
        for kk in keys:
            s[kk].requires_grad_(True)
        xx = x.to(dt).requires_grad_(True)
        lg, ft = U.unet_forward(xx, s, train=True, bilinear=bilinear, feature=True)
        leaves = [s[kk] for kk in keys] + [xx]
        gr = {}
        for name, fn in LOSSES.items():
            gs = torch.autograd.grad(fn(lg, ft), leaves, retain_graph=True, allow_unused=True)
            gr[name] = {kk: (torch.zeros_like(l) if g_ is None else g_).detach() for kk, l, g_ in zip(keys + ["x"], leaves, gs)}
        per.append(gr)
    for name in LOSSES:
        out[name] = {kk: (per[0][name][kk], per[1][name][kk]) for kk in per[0][name]}
    return out


def hip_grads(model, x, loss, x_grad=True):
    for p in model.parameters():
        p.grad = None
    xg = x.cuda().requires_grad_(x_grad)
    lg, ft = model(xg, feature=True)
    LOSSES[loss](lg, ft).backward()
    return {kk: p.grad for kk, p in model.named_parameters()}, xg.grad


def check_against_oracle(c, k, n, h, w, base, seed, loss, bilinear=False):
    """test_forward_backward_vs_oracle's rule, x.grad included: the HIP error against the f64 oracle is at most five times the CPU
    f32 oracle's own, floor 2e-4 (base < 64) / 1e-2 (base 64: ReLU-kink flips through the tiny bottleneck BatchNorms)"""
    sd, x = _inputs(c, k, n, h, w, base, seed, bilinear)
    if bilinear:
        from networks.unet_model import UNet
        model = UNet(c, k, bilinear=True, base_channels=base)
        model.load_state_dict({kk: v.detach().clone() for kk, v in sd.items()})
        model = model.cuda()
    else:
        model = build_model(sd, c, k, base)
    model.train()
    want = oracle_grads(c, k, n, h, w, base, seed, bilinear)[loss]
    pg, xg = hip_grads(model, x, loss)
    assert xg is not None and xg.shape == x.shape
    got = dict(pg, x=xg)
    floor = 2e-4 if base < 64 else 1e-2
    for key, (g32, g64) in want.items():
        if float(g64.norm()) == 0.0:                     # (the head under the features-only loss)
            assert got[key] is not None and float(got[key].abs().max()) == 0.0, key
            continue
        err_hip, err_cpu = rel_l2(got[key].cpu(), g64), rel_l2(g32, g64)
        if key == "x":
            print(f"x.grad [{loss}] {(c, k, n, h, w, base)}: HIP {err_hip:.2e}, CPU f32 {err_cpu:.2e} against the f64 oracle")
        assert err_hip < max(5 * err_cpu, floor), (key, err_hip, err_cpu)
    return model, x, pg


@pytest.mark.parametrize("c,k,n,h,w,base,seed", [(3, 2, 2, 32, 32, 8, 5), (1, 4, 3, 48, 32, 8, 5), (3, 2, 1, 50, 38, 8, 5),
                                                 (3, 2, 2, 64, 48, 64, 12)])
def test_input_gradient_vs_oracle(c, k, n, h, w, base, seed):
    model, x, pg = check_against_oracle(c, k, n, h, w, base, seed, "logits")
    pg = {kk: v.clone() for kk, v in pg.items()}
    plain, none = hip_grads(model, x, "logits", x_grad=False)         # asking for x.grad moves no parameter gradient bit
    assert none is None
    for kk in pg:
        assert torch.equal(pg[kk], plain[kk]), kk


@pytest.mark.parametrize("loss", ["feat", "both"])
@pytest.mark.parametrize("c,k,n,h,w,base,seed", [(3, 2, 2, 32, 32, 8, 5), (3, 2, 2, 64, 48, 64, 12)])
def test_feature_gradient_vs_oracle(c, k, n, h, w, base, seed, loss):
    model, x, pg = check_against_oracle(c, k, n, h, w, base, seed, loss)
    if loss == "feat":
        assert float(pg["outc.conv.weight"].abs().max()) == 0.0 and float(pg["outc.conv.bias"].abs().max()) == 0.0


# ---- 4. 16-bit storage and f32x3 against the f32 network --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def f32_reference(c, k, n, h, w, base):
    """(state dict, x, the f32 network's x.grad, its x.grad at the input rounded to bf16) -- test_bf16_compute_tracks_f32's weights,
    input and perturbation yardstick"""
    from networks.unet_model import UNet
    torch.manual_seed(21)
    sd = U.make_state_dict(c, k, base=base)
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(22))
    res = []
    for xin in (x, x.to(torch.bfloat16).float()):
        m = UNet(c, k, base_channels=base, dtype="f32")
        m.load_state_dict({kk: v.clone() for kk, v in sd.items()})
        xg = xin.cuda().requires_grad_()
        m.cuda().train()(xg).square().mean().backward()
        res.append(xg.grad.cpu())
    return sd, x, res[0], res[1]


@pytest.mark.parametrize("c,k,n,h,w,base", [(3, 2, 2, 64, 64, 64), (1, 4, 2, 48, 32, 16), (3, 2, 2, 64, 64, 24)])
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32x3"])
def test_low_precision_input_gradient_tracks_f32(dtype, c, k, n, h, w, base):
    """x.grad of the bf16 / f16 / f32x3 network against the f32 HIP network on the same weights, held to the f32 network's own
    response to ONE bf16 rounding of the input: max(YARD_X * yardstick, 3e-3)."""
    from networks.unet_model import UNet
    sd, x, g32, g32r = f32_reference(c, k, n, h, w, base)
    m = UNet(c, k, base_channels=base, dtype=dtype)
    m.load_state_dict({kk: v.clone() for kk, v in sd.items()})
    xg = x.cuda().requires_grad_()
    m.cuda().train()(xg).square().mean().backward()
    err, yard = rel_l2(xg.grad.cpu(), g32), rel_l2(g32r, g32)
    print(f"x.grad {dtype} vs f32 {(c, k, n, h, w, base)}: error {err:.3e}, yardstick {yard:.3e}, ratio {err / max(yard, 1e-30):.2f}")
    assert err < max(YARD_X * yard, 3e-3), (err, yard)


# ---- 5. passes, parts, variants -----------------------------------------------------------------------------------------
def test_passes_with_lead_and_tail():
    """groups = 3, lead = 1, tail = 1: dx's rows of the two gradient passes equal those of separate calls (BatchNorm is per pass, so
    the same numbers up to the f32 summation order of the batched reductions: 1e-5), the leading and the tail rows are zero"""
    from networks.unet_model import UNet
    torch.manual_seed(29)
    m1 = UNet(3, 2, base_channels=16, dtype="f32").cuda().train()
    m2 = copy.deepcopy(m1)
    g = torch.Generator().manual_seed(12)
    n = 2
    x = torch.randn(3 * n + 1, 3, 40, 40, generator=g).cuda()
    dl = torch.randn(3 * n, 2, 40, 40, generator=g).cuda()
    xg = x.clone().requires_grad_()
    lg = m1.forward_batched(xg, 3, tail=1, lead=1)
    assert lg.shape[0] == 3 * n
    lg.backward(dl)
    assert xg.grad.shape == x.shape
    assert float(xg.grad[:n].abs().max()) == 0.0 and float(xg.grad[3 * n:].abs().max()) == 0.0
    for q in (1, 2):
        xs = x[q * n:(q + 1) * n].clone().requires_grad_()
        m2(xs).backward(dl[q * n:(q + 1) * n])
        e = rel_l2(xg.grad[q * n:(q + 1) * n].cpu(), xs.grad.cpu())
        assert e < 1e-5, (q, e)


def test_backward_in_parts_gives_the_same_dx():
    """parts 1 | 3 | 4 (dfeat consumed by part 1, dx written by part 4) == the single call, bit for bit"""
    from networks.unet_model import UNet
    torch.manual_seed(7)
    m1 = UNet(3, 2, base_channels=16, dtype="bf16").cuda().train()
    m2 = copy.deepcopy(m1)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 32, 32, generator=g).cuda()
    dl = torch.randn(2, 2, 32, 32, generator=g).cuda()
    df = torch.randn(2, 16, 32, 32, generator=g).cuda()
    fired = []
    m2._ustrun_backward_split_hook = lambda: fired.append(1)
    m2._ustrun_backward_mid_hook = lambda: fired.append(3)
    grads = []
    for m in (m1, m2):
        xg = x.clone().requires_grad_()
        lg, ft = m(xg, feature=True)
        torch.autograd.backward([lg, ft], [dl, df])
        grads.append(xg.grad)
    assert fired == [1, 3]
    assert torch.equal(grads[0], grads[1])
    for (kk, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(p1.grad, p2.grad), kk


def test_bilinear_input_and_feature_gradient_vs_oracle():
    check_against_oracle(3, 2, 2, 32, 32, 8, 11, "both", bilinear=True)


def test_domain_specific_batchnorm_and_frozen_parameters():
    """UNet(num_domains = 2): x.grad and the feature gradient's parameter gradients are those of the plain network carrying the
    call's domain's members, bit for bit; with every parameter frozen the node is still recorded for x alone"""
    from networks.unet_model import UNet
    torch.manual_seed(41)
    plain = UNet(3, 2, base_channels=16).cuda().train()
    torch.manual_seed(41)
    ds = UNet(3, 2, base_channels=16, num_domains=2).cuda().train()
    g = torch.Generator().manual_seed(8)
    for m in ds.modules():
        if hasattr(m, "bns"):
            for bn in m.bns:
                with torch.no_grad():
                    bn.weight.copy_(torch.rand(bn.num_features, generator=g) + 0.5)
                    bn.bias.copy_(torch.randn(bn.num_features, generator=g) * 0.1)
    sd = {}
    for kk, v in ds.state_dict().items():
        if ".bns." in kk:
            head, rest = kk.split(".bns.")
            d_, name = rest.split(".", 1)
            if int(d_) == 1:
                sd[f"{head}.{name}"] = v.clone()
        else:
            sd[kk] = v.clone()
    plain.load_state_dict(sd)
    x = torch.randn(2, 3, 32, 32, generator=g).cuda()
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    la, fa = plain(xa, feature=True)
    (la.square().mean() + fa.square().mean()).backward()
    lb, fb = ds(xb, feature=True, domain_label=torch.tensor([1, 0]))
    (lb.square().mean() + fb.square().mean()).backward()
    assert torch.equal(xa.grad, xb.grad)
    assert torch.equal(plain.inc.double_conv[0].weight.grad, ds.inc.double_conv[0].weight.grad)
    assert torch.equal(plain.up4.conv.double_conv[4].weight.grad, ds.up4.conv.double_conv[4].bns[1].weight.grad)
    for p in plain.parameters():
        p.requires_grad_(False)
        p.grad = None
    xc = x.clone().requires_grad_()
    lc, fc = plain(xc, feature=True)
    assert lc.requires_grad and fc.requires_grad
    (lc.square().mean() + fc.square().mean()).backward()
    assert torch.equal(xc.grad, xa.grad)
    assert all(p.grad is None for p in plain.parameters())


# ---- 6. what is not built ---------------------------------------------------------------------------------------------------
def test_eval_mode_input_gradient_is_refused():
    from networks.unet_model import UNet
    m = UNet(1, 2, base_channels=8).cuda().eval()
    with pytest.raises(NotImplementedError, match="eval-mode backward"):
        m(torch.zeros(1, 1, 32, 32).cuda().requires_grad_())
    with torch.no_grad():                               # no graph asked for: the plain forward
        assert m(torch.zeros(1, 1, 32, 32).cuda().requires_grad_()).shape == (1, 2, 32, 32)
