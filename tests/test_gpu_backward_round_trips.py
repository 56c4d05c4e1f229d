"""GPU: the two full-resolution gradient round trips the backward no longer makes.

Layer 17 (under the head): `head_bwd_kernel` stores no da17; the layer's BatchNorm-backward apply pass forms it again from dlogits
(`ustrun_bn_bwd_apply_head`).  Layer 0: no apply pass; the first convolution's streaming weight gradient forms dy0 from da0 and y0 in its
loader (`ustrun_conv_first_wgrad_bn`).  ustrun_debug_flags2 bit 4 keeps both round trips: every gradient must be bit-identical either
way, the route taken is read back (`ustrun_debug_last_backward_route`), and each operator is checked alone against a float64 statement
of its formulas on data that float32 evaluates exactly (so the expectation is exact whatever the compiler contracts)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

KEEP = 16              # ustrun_debug_flags2 bit 4: both round trips stay
ELT = {"bf16": (torch.bfloat16, 1), "f16": (torch.float16, 2)}
GUARD = 4096


def L():
    from ustrun import _lib
    return _lib


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def guarded(t, poison):
    """a copy of `t` on the device inside a larger buffer whose surroundings hold `poison`; returns (view, whole buffer)"""
    flat = torch.full((t.numel() + 2 * GUARD,), poison, dtype=t.dtype, device="cuda")
    flat[GUARD:GUARD + t.numel()] = t.reshape(-1).to(flat.device)
    return flat[GUARD:GUARD + t.numel()].view(t.shape), flat


def guards_intact(flat, n, poison):
    lo, hi = flat[:GUARD], flat[GUARD + n:]
    if poison != poison:
        return bool(torch.isnan(lo.float()).all()) and bool(torch.isnan(hi.float()).all())
    return bool((lo == poison).all()) and bool((hi == poison).all())


# ---- whole network -----------------------------------------------------------------------------------------------------------

_MODELS = {}


def _model(elt, c, k):
    """one network per (storage type, channels, classes), shared by the cases; BatchNorm weights away from their (1, 0) start"""
    from networks.unet_model import UNet
    key = (elt, c, k)
    if key not in _MODELS:
        torch.manual_seed(11 + 3 * c + k)
        m = UNet(c, k, base_channels=64, dtype=elt)
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, torch.nn.BatchNorm2d):
                    mod.weight.copy_(1 + 0.3 * torch.randn(mod.num_features, generator=g))
                    mod.bias.copy_(0.1 * torch.randn(mod.num_features, generator=g))
        _MODELS[key] = m.cuda().train()
    return _MODELS[key]


class Net:
    """a forward through ustrun_unet_forward and what its backward calls need"""

    def __init__(self, elt, c, k, n, h, w, groups=1, tail=0, lead=0, feature=False):
        from ustrun import engine
        self.model = _model(elt, c, k)
        g = torch.Generator().manual_seed(n + h + w)
        self.x = torch.randn(n, c, h, w, generator=g).cuda()
        logits, feat, self.ws, self.d = engine._run_forward(self.model, self.x, feature, groups, tail, lead)
        # (f16 gradients arrive multiplied by the loss scale)
        self.dl = (torch.randn(n - tail, k, h, w, generator=g) * (256.0 if elt == "f16" else 1.0)).cuda()
        self.dfeat = (torch.randn(n - tail, 64, h, w, generator=g) * (256.0 if elt == "f16" else 1.0)).cuda() if feature else None
        self.params = engine.model_params(self.model)
        assert len(self.params) == 64

    def backward(self, keep, parts=(0,), dfeat=False, dx=False):
        """-> (the 64 gradients, dx or None, the route codes of the calls); scratch and outputs start as NaN"""
        l = L()
        lib = l.lib()
        d = self.d
        scratch = torch.full((lib.ustrun_unet_bwd_scratch_bytes(C.byref(d)),), 0xFF, dtype=torch.uint8, device="cuda")
        flat = torch.full((sum(p.numel() for p in self.params),), float("nan"), device="cuda")
        grads, o = [], 0
        for p in self.params:
            grads.append(flat[o:o + p.numel()].view_as(p))
            o += p.numel()
        arr = (C.c_void_p * len(grads))(*[t.data_ptr() for t in grads])
        dxt = torch.full_like(self.x, float("nan")) if dx else None
        routes = []
        old = lib.ustrun_debug_flags2(0)
        lib.ustrun_debug_flags2((old & ~(KEEP | 32 | 64)) | (KEEP if keep is True else int(keep)))
        try:
            for part in parts:
                if dfeat or dx:
                    rc = lib.ustrun_unet_backward_io(C.byref(d), self.x.data_ptr(), self.dl.data_ptr(), l.ptr(self.dfeat if dfeat else None),
                                                     self.ws.data_ptr(), scratch.data_ptr(), arr, 0, part, l.ptr(dxt), None)
                elif part == 0:
                    rc = lib.ustrun_unet_backward(C.byref(d), self.x.data_ptr(), self.dl.data_ptr(), self.ws.data_ptr(), scratch.data_ptr(),
                                                  arr, 0, None)
                else:
                    rc = lib.ustrun_unet_backward_part(C.byref(d), self.x.data_ptr(), self.dl.data_ptr(), self.ws.data_ptr(),
                                                       scratch.data_ptr(), arr, 0, part, None)
                l.check(rc, "ustrun_unet_backward")
                routes.append(lib.ustrun_debug_last_backward_route())
        finally:
            lib.ustrun_debug_flags2(old)
        torch.cuda.synchronize()
        return grads, dxt, routes


def assert_same(got, want):
    assert len(got) == len(want) == 64
    for i, (a, b) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(b).all()), i
        assert torch.equal(a, b), (i, float((a - b).abs().max()))


# (a) one pass; (b) three passes of two images, the first without gradient, and a one-image tail behind them; (c) ragged strips of the
# first-convolution kernel (40 % 16 != 0), one input channel, the run-time class count
NET_CASES = {"a": dict(c=3, k=2, n=2, h=32, w=32), "b": dict(c=3, k=2, n=7, h=32, w=64, groups=3, lead=1, tail=1),
             "c": dict(c=1, k=4, n=2, h=48, w=40)}


@pytest.mark.parametrize("elt", ["bf16", "f16"])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_whole_network_both_routes_bit_identical(case, elt):
    """ustrun_unet_forward once, ustrun_unet_backward with the round trips kept (ustrun_debug_flags2 bit 4) and without: all 64
    gradient tensors torch.equal, the new route taken at both layers (route code 3) and at neither under the switch.  The scratch
    starts as NaN, so a reader of the da17 nobody stored would show."""
    net = Net(elt, **NET_CASES[case])
    old, _, r_old = net.backward(keep=True)
    new, _, r_new = net.backward(keep=False)
    assert r_old == [0] and r_new == [3], (r_old, r_new)
    assert_same(new, old)
    if case == "a":             # bits 5 / 6 keep one round trip each (how each half is timed alone)
        for bit, route in ((32, 2), (64, 1)):
            half, _, r_half = net.backward(keep=bit)
            assert r_half == [route], (bit, r_half)
            assert_same(half, old)


@pytest.mark.parametrize("elt", ["bf16", "f16"])
def test_split_backward_takes_the_routes_inside_its_parts(elt):
    """Layer 17 lies inside part 1, layer 0 inside parts 2 and 4: the split calls take the same routes and give the single call's
    gradients (two parts and three)."""
    net = Net(elt, **NET_CASES["a"])
    one, _, r = net.backward(keep=False)
    assert r == [3]
    two, _, r2 = net.backward(keep=False, parts=(1, 2))
    assert r2 == [1, 2], r2
    assert_same(two, one)
    three, _, r3 = net.backward(keep=False, parts=(1, 3, 4))
    assert r3 == [1, 0, 2], r3
    assert_same(three, one)
    kept, _, rk = net.backward(keep=True, parts=(1, 2))
    assert rk == [0, 0]
    assert_same(kept, one)


@pytest.mark.parametrize("elt", ["bf16", "f16"])
def test_fallbacks_with_input_gradient_and_feature_gradient(elt):
    """dx requested: conv_first_dgrad needs the stored dy0, layer 0 keeps its apply pass (route 1).  dfeat given: the head's sums would
    miss it and da17 is summed in memory, layer 17 keeps its round trip (route 2).  Gradients equal the switch-set run's."""
    net = Net(elt, feature=True, **NET_CASES["a"])
    old, dx_old, r = net.backward(keep=True, dx=True)
    new, dx_new, r_new = net.backward(keep=False, dx=True)
    assert r == [0] and r_new == [1], (r, r_new)
    assert_same(new, old)
    assert bool(torch.isfinite(dx_old).all()) and torch.equal(dx_new, dx_old)
    old, _, r = net.backward(keep=True, dfeat=True)
    new, _, r_new = net.backward(keep=False, dfeat=True)
    assert r == [0] and r_new == [2], (r, r_new)
    assert_same(new, old)
    old, dx_old, r = net.backward(keep=True, dfeat=True, dx=True)
    new, dx_new, r_new = net.backward(keep=False, dfeat=True, dx=True)
    assert r == [0] and r_new == [0], (r, r_new)
    assert_same(new, old)
    assert torch.equal(dx_new, dx_old)


# ---- operators against float64 -----------------------------------------------------------------------------------------------

def _apply_ref(y, da, scale, shift, coef):
    """float64: dy = k0 (y scale + shift > 0 ? da : 0) + k1 y + k2, per pass constants; y, da [P, N, H, W, C]; tables [P, C] / [P, 3, C]"""
    y, da = np.asarray(y, np.float64), np.asarray(da, np.float64)
    sc, sh = np.asarray(scale, np.float64)[:, None, None, None, :], np.asarray(shift, np.float64)[:, None, None, None, :]
    k = np.asarray(coef, np.float64)[:, :, None, None, None, :]
    z = np.where(y * sc + sh > 0, da, 0.0)
    return k[:, 0] * z + k[:, 1] * y + k[:, 2]


def _round16(a, t16):
    return torch.from_numpy(np.asarray(a, np.float64)).to(torch.float32).to(t16).float()


@pytest.mark.parametrize("elt", ["bf16", "f16"])
@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("n,h,w", [(2, 24, 40), (3, 9, 7)])
def test_apply_from_dlogits_against_float64(n, h, w, k, passes, elt):
    """`ustrun_bn_bwd_apply_head` alone, C = 64: g = sum_k dl[k] w[k] rounded to the storage type, then the apply formula, against
    float64 on dyadic data (dl, w multiples of 1/32: g has up to 12 significant bits, so the rounding to 8 / 11 bits is exercised;
    every float32 intermediate is exact, so float64 gives the same value before each rounding) -- the bound of
    test_bf16_storage_bn_head_backward (1e-5 against the rounded expectation), which exact data meets with equality.  Also
    bit-identical to ustrun_head_bwd (da stored) + ustrun_bn_bwd_apply.  16-bit y between NaN zones, dl between NaN zones, dy between
    sentinel zones.  9 x 7: 63-pixel images, a block's 32 pixels straddle image ends."""
    l = L()
    lib = l.lib()
    t16, code = ELT[elt]
    c = 64
    g = torch.Generator().manual_seed(100 * k + 10 * passes + h)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    y = ri(-8, 8, passes, n, h, w, c) / 4
    dl = ri(-31, 31, passes, n, k, h, w) / 32
    wt = ri(-31, 31, k, c) / 32
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (passes, c), generator=g)] * (2 * ri(0, 1, passes, c) - 1)
    shift = ri(-4, 4, passes, c) / 4
    coef = torch.stack([ri(-15, 15, passes, c) / 8, ri(-15, 15, passes, c) / 16, ri(-15, 15, passes, c) / 8], 1)     # [P, 3, C]
    # expectation
    g64 = np.einsum("pnkhw,kc->pnhwc", dl.double().numpy(), wt.double().numpy())
    g16 = _round16(g64, t16)
    want = _round16(_apply_ref(y.numpy(), g16.numpy(), scale.numpy(), shift.numpy(), coef.numpy()), t16)
    # device
    aff = torch.zeros(passes, 4, c)
    aff[:, 0], aff[:, 1] = scale, shift
    affg, coefg, wg = aff.cuda(), coef.contiguous().cuda(), wt.contiguous().cuda()
    yg, yflat = guarded(y.to(t16), float("nan"))
    dlg, dlflat = guarded(dl, float("nan"))
    dy, dyflat = guarded(torch.zeros(passes, n, h, w, c, dtype=t16), 7.0)
    l.check(lib.ustrun_bn_bwd_apply_head(dlg.data_ptr(), wg.data_ptr(), yg.data_ptr(), affg.data_ptr(), affg.data_ptr() + 4 * c,
                                         coefg.data_ptr(), n, h, w, c, k, dy.data_ptr(), code, passes, 4 * c, None))
    torch.cuda.synchronize()
    got = dy.float().cpu()
    assert bool(torch.isfinite(got).all())
    assert rel(got, want) < 1e-5, rel(got, want)
    assert torch.equal(got, want)
    assert guards_intact(dyflat, dy.numel(), 7.0) and guards_intact(yflat, yg.numel(), float("nan")) and guards_intact(dlflat, dlg.numel(), float("nan"))
    # the two-kernel route, pass by pass: the head stores da, the apply pass reads it
    row = k * c + k + 2 * c
    part = torch.empty(1024 * row, device="cuda")
    for p in range(passes):
        da = torch.empty(n, h, w, c, dtype=t16, device="cuda")
        dw, db = torch.empty(k, c, device="cuda"), torch.empty(k, device="cuda")
        sc_p, sh_p = affg.data_ptr() + 16 * c * p, affg.data_ptr() + 16 * c * p + 4 * c
        l.check(lib.ustrun_head_bwd(dlg[p].data_ptr(), yg[p].data_ptr(), sc_p, sh_p, n * h * w, h * w, c, k, wg.data_ptr(), da.data_ptr(),
                                    dw.data_ptr(), db.data_ptr(), 0, part.data_ptr(), part.numel() * 4, code, None))
        assert torch.equal(da.float().cpu(), g16[p])
        dy2 = torch.empty_like(da)
        l.check(lib.ustrun_bn_bwd_apply(da.data_ptr(), None, yg[p].data_ptr(), sc_p, sh_p, coefg[p].data_ptr(), n, h, w, c, dy2.data_ptr(),
                                        code, None))
        assert torch.equal(dy2, dy[p])


@pytest.mark.parametrize("elt", ["bf16", "f16"])
@pytest.mark.parametrize("h,w", [(32, 32), (40, 48)])
@pytest.mark.parametrize("cin", [1, 3])
def test_first_convolution_weight_gradient_with_apply_on_load(cin, h, w, elt):
    """`ustrun_conv_first_wgrad_bn` alone, N = 2 as two passes of one image (each image its own constants): dw of the first convolution
    with dY = apply(da, y) formed in the loader, against float64 (autograd of conv2d on the float64 apply formula) by the small-integer
    method and bound of test_conv_first_weight_gradient_exact (1e-6; x in -3..3, dY multiples of 1/4 below 8: every product and sum is
    exact), accumulate included; bit-identical to ustrun_bn_bwd_apply + ustrun_conv3x3_wgrad.  da and y between NaN zones, dw between
    sentinels, the partials' published bound respected."""
    l = L()
    lib = l.lib()
    t16, code = ELT[elt]
    n, c = 2, 64
    g = torch.Generator().manual_seed(7 * cin + w)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    x = ri(-3, 3, n, cin, h, w)
    da = ri(-2, 2, n, 1, h, w, c)
    y = ri(-4, 4, n, 1, h, w, c) / 2
    scale = (1 + ri(0, 1, n, c)) * (2 * ri(0, 1, n, c) - 1)
    shift = ri(-2, 2, n, c) / 2
    coef = torch.stack([torch.tensor([-2.0, -1.0, 0.5, 1.0, 2.0])[torch.randint(0, 5, (n, c), generator=g)], ri(-2, 2, n, c) / 2,
                        ri(-2, 2, n, c) / 2], 1)
    dy64 = _apply_ref(y.numpy(), da.numpy(), scale.numpy(), shift.numpy(), coef.numpy())[:, 0]          # [N, H, W, C]
    assert np.array_equal(dy64, _round16(dy64, t16).double().numpy())                                    # the storage type holds it
    wr = torch.zeros(64, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wr, None, 1, 1).backward(torch.from_numpy(dy64).permute(0, 3, 1, 2).contiguous())
    aff = torch.zeros(n, 4, c)
    aff[:, 0], aff[:, 1] = scale, shift
    affg, coefg, xg = aff.cuda(), coef.contiguous().cuda(), x.contiguous().cuda()
    dag, daflat = guarded(da.to(t16), float("nan"))
    yg, yflat = guarded(y.to(t16), float("nan"))
    src = l.nchw_src(xg.data_ptr(), cin, h, w)
    nb = lib.ustrun_wgrad_partials_bytes(9, cin, 64, n * h * w)
    part = torch.full((nb // 4 + 1024,), 5.0, device="cuda")
    Z = 512
    buf = torch.full((Z + 64 * cin * 9 + Z,), 9.0, device="cuda")
    dw = buf[Z:Z + 64 * cin * 9].view(64, cin, 3, 3)
    args = (C.byref(src), dag.data_ptr(), yg.data_ptr(), affg.data_ptr(), affg.data_ptr() + 4 * c, coefg.data_ptr(), 1, 4 * c, n, h, w, 64,
            dw.data_ptr())
    l.check(lib.ustrun_conv_first_wgrad_bn(*args, 0, part.data_ptr(), nb, code, None))
    got = dw.cpu().clone()
    assert bool(torch.isfinite(got).all())
    assert rel(got, wr.grad) < 1e-6, rel(got, wr.grad)
    l.check(lib.ustrun_conv_first_wgrad_bn(*args, 1, part.data_ptr(), nb, code, None))
    assert rel(dw.cpu(), 2 * wr.grad) < 1e-6
    assert bool((buf[:Z] == 9.0).all()) and bool((buf[-Z:] == 9.0).all())
    assert bool((part[nb // 4:] == 5.0).all()), "slabs beyond the published partials bound"
    assert guards_intact(daflat, dag.numel(), float("nan")) and guards_intact(yflat, yg.numel(), float("nan"))
    # the two-kernel route: apply pass per image, then the weight gradient over the stored dy
    dys = torch.empty(n, h, w, c, dtype=t16, device="cuda")
    for p in range(n):
        l.check(lib.ustrun_bn_bwd_apply(dag[p].data_ptr(), None, yg[p].data_ptr(), affg.data_ptr() + 16 * c * p,
                                        affg.data_ptr() + 16 * c * p + 4 * c, coefg[p].data_ptr(), 1, h, w, c, dys[p].data_ptr(), code, None))
    assert torch.equal(dys.float().cpu().double(), torch.from_numpy(dy64))
    dw2 = torch.empty(64, cin, 3, 3, device="cuda")
    l.check(lib.ustrun_conv3x3_wgrad(C.byref(src), 1, dys.data_ptr(), n, h, w, 64, dw2.data_ptr(), 0, part.data_ptr(), nb, code, None))
    assert torch.equal(dw2.cpu(), got)
