"""GPU parity of DeepLabV2-ResNet in dtype "f32x3" (f32 tensors, every convolution product as six bf16 MFMAs over three-term
operand splits): the one-tap-per-block weight-gradient kernel (csrc/wgrad_tap_x3.hip) on exact small integers and on operands
that carry 24 significant bits, the fallbacks it leaves to the f32 kernel, the forward / input-gradient implicit GEMM on the
packed planes (ustrun_pack_conv with USTRUN_F32X3), and the whole network -- forward, backward, SGD steps -- at the bars of the
f32 path."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu

X3 = 3                  # USTRUN_F32X3
TAP_X3 = 0x58           # ustrun_debug_last_wgrad_variant >> 24 of wgrad_tap_x3.hip


def L():
    from ustrun import _lib
    return _lib


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def from_nhwc(t):
    return t.float().permute(0, 3, 1, 2).contiguous().cpu()


def _wgrad(l, src, dyg, n, ho, wo, ci, co, k, s, d, dt, accumulate=0, dw=None):
    lib = l.lib()
    pb = lib.ustrun_wgrad_partials_bytes(k * k, ci, co, n * ho * wo)
    part = torch.empty(pb, dtype=torch.uint8, device="cuda")
    if dw is None:
        dw = torch.full((co, ci, k, k), 3.0, device="cuda")
    l.check(lib.ustrun_conv2d_wgrad(C.byref(src), 1, dyg.data_ptr(), n, ho, wo, co, k, s, d, dw.data_ptr(), accumulate, part.data_ptr(), pb, dt,
                                    None))
    return dw, lib.ustrun_debug_last_wgrad_variant()


def _int_case(n, ci, co, h, w, k, s, d):
    """test_conv2d_wgrad_general's construction: small integers, BatchNorm + ReLU evaluated by the loader"""
    g = torch.Generator().manual_seed(ci + 3 * co + k + s + d)
    y = torch.randint(-3, 4, (n, ci, h, w), generator=g).float()
    sc = torch.randint(1, 3, (ci,), generator=g).float()
    sh = torch.randint(-2, 3, (ci,), generator=g).float()
    x = torch.relu(y * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    ho, wo = F.conv2d(x, torch.zeros(co, ci, k, k), None, s, d * (k // 2), d).shape[-2:]
    dy = torch.randint(-2, 3, (n, co, ho, wo), generator=g).float()
    want = torch.nn.grad.conv2d_weight(x, (co, ci, k, k), dy, s, d * (k // 2), d)
    return y, sc, sh, dy, ho, wo, want


@pytest.mark.parametrize("n,ci,co,h,w,k,s,d", [(2, 64, 128, 12, 15, 1, 1, 1), (2, 128, 64, 13, 16, 1, 2, 1), (2, 64, 64, 14, 12, 3, 2, 1),
                                               (2, 64, 64, 15, 13, 3, 1, 2), (1, 128, 64, 12, 12, 3, 1, 4), (1, 128, 128, 7, 70, 3, 1, 2),
                                               (2, 128, 64, 5, 67, 1, 2, 1), (3, 128, 128, 9, 7, 1, 1, 1)])
def test_wgrad_tap_x3_exact(n, ci, co, h, w, k, s, d):
    """1x1 / 3x3, stride 2, dilation 2 / 4 through the three-term one-tap kernel: odd extents into stride 2 (a dangling last row /
    column), rows wider and narrower than the 32-pixel stage, pixel counts that are no multiple of it, split-K tails.  Integers this
    small are exact in the first bf16 term and the sums stay below 2^24: equality with torch.nn.grad.conv2d_weight, and twice the
    value with accumulate = 1.  The variant code says the new kernel, not the f32 fallback, produced it."""
    l = L()
    y, sc, sh, dy, ho, wo, want = _int_case(n, ci, co, h, w, k, s, d)
    yg, dyg, scg, shg = nhwc(y), nhwc(dy), sc.cuda(), sh.cuda()
    src = l.nhwc_src(yg.data_ptr(), ci, h, w, scg.data_ptr(), shg.data_ptr(), relu=1)
    dw, v = _wgrad(l, src, dyg, n, ho, wo, ci, co, k, s, d, X3)
    assert (v >> 24) == TAP_X3, hex(v)
    assert (v >> 20) & 15 == (2 if ci % 128 == 0 else 1) and (v >> 16) & 15 == (2 if co % 128 == 0 else 1) and (v >> 12) & 15 == (k == 1)
    assert torch.equal(dw.cpu(), want)
    dw, v = _wgrad(l, src, dyg, n, ho, wo, ci, co, k, s, d, X3, accumulate=1, dw=dw)
    assert (v >> 24) == TAP_X3, hex(v)
    assert torch.equal(dw.cpu(), 2 * want)


@pytest.mark.parametrize("n,ci,co,h,w,k,s,d", [(2, 128, 64, 13, 16, 1, 2, 1), (1, 128, 64, 12, 12, 3, 1, 4)])
def test_wgrad_tap_x3_uses_all_three_terms(n, ci, co, h, w, k, s, d):
    """Operands with 24 significant bits, x = a + b 2^-9 + c 2^-18 (small integers a, b, c): the three-term products against
    conv2d_weight in float64.  Yardstick: the f32 matrix-core kernel (dtype 0) on the same inputs -- the three dropped products are
    below 2^-24 of a product, one f32 rounding, so the error may be at most 2x that kernel's; and it must be at least 100x smaller
    than what the same operands rounded to bf16 ONCE give, which a kernel multiplying only the leading terms would show."""
    l = L()
    g = torch.Generator().manual_seed(7 * ci + co + k + d)

    def fine(shape):
        a, b, c = (torch.randint(-3, 4, shape, generator=g).double() for _ in range(3))
        return (a + b * 2.0 ** -9 + c * 2.0 ** -18).float()
    x = fine((n, ci, h, w))
    ho, wo = F.conv2d(x, torch.zeros(co, ci, k, k), None, s, d * (k // 2), d).shape[-2:]
    dy = fine((n, co, ho, wo))
    assert torch.equal(x.double().float(), x)
    pad = d * (k // 2)
    want = torch.nn.grad.conv2d_weight(x.double(), (co, ci, k, k), dy.double(), s, pad, d)
    once = torch.nn.grad.conv2d_weight(x.bfloat16().double(), (co, ci, k, k), dy.bfloat16().double(), s, pad, d)
    xg, dyg = nhwc(x), nhwc(dy)
    src = l.nhwc_src(xg.data_ptr(), ci, h, w)
    dw3, v = _wgrad(l, src, dyg, n, ho, wo, ci, co, k, s, d, X3)
    assert (v >> 24) == TAP_X3, hex(v)
    dw0, v0 = _wgrad(l, src, dyg, n, ho, wo, ci, co, k, s, d, 0)
    assert (v0 >> 24) != TAP_X3
    e3, e0, e16 = rel(dw3.cpu(), want), rel(dw0.cpu(), want), rel(once, want)
    print(f"wgrad_tap_x3 ({n},{ci},{co},{h},{w},{k},{s},{d}): rel-L2 vs float64 -- f32x3 {e3:.3e}, f32 kernel {e0:.3e}, bf16 once {e16:.3e}")
    assert e3 <= 2 * e0
    assert 100 * e3 <= e16


def test_wgrad_x3_fallback_stays_exact():
    """Cin = 96 is no multiple of 64: dtype 3 keeps the generic f32 kernel, exact on integers, and the variant code is not the
    new kernel's."""
    l = L()
    n, ci, co, h, w, k, s, d = 1, 96, 128, 9, 10, 1, 1, 1
    y, sc, sh, dy, ho, wo, want = _int_case(n, ci, co, h, w, k, s, d)
    yg, dyg, scg, shg = nhwc(y), nhwc(dy), sc.cuda(), sh.cuda()
    src = l.nhwc_src(yg.data_ptr(), ci, h, w, scg.data_ptr(), shg.data_ptr(), relu=1)
    dw, v = _wgrad(l, src, dyg, n, ho, wo, ci, co, k, s, d, X3)
    assert (v >> 24) != TAP_X3, hex(v)
    assert torch.equal(dw.cpu(), want)


def test_rowwin_stem_x3():
    """The 7x7 / stride-2 stem through its row-window view with dtype 3 (24-element windows: no x3 kernel takes them, the f32
    kernels run): the forward of test_rowwin_stem_and_aspp_gather_direct from a pack of the dtype's own size, and the weight
    gradient of test_rowwin_stem_wgrad, both exact."""
    l = L()
    lib = l.lib()
    g = torch.Generator().manual_seed(41)
    n, h, w = 2, 29, 34
    x = torch.randint(-3, 4, (n, 3, h, w), generator=g).float()
    wt = torch.randint(-2, 3, (64, 3, 7, 7), generator=g).float()
    ref = F.conv2d(x, wt, None, 2, 3)
    ho, wo = ref.shape[-2:]
    dy = torch.randint(-2, 3, (n, 64, ho, wo), generator=g).float()
    want = torch.nn.grad.conv2d_weight(x, (64, 3, 7, 7), dy, 2, 3)
    xp = F.pad(x.permute(0, 2, 3, 1), (0, 0, 3, 4, 3, 3)).contiguous().cuda()
    hp, wp = h + 6, w + 7
    src = l.Src(xp.data_ptr(), None, None, 24, hp, wp - 7, hp * wp * 3, wp * 3, 3, 1, 0, 0, 0, 0, 0, 0, 0)
    wr = F.pad(wt.permute(0, 2, 3, 1).reshape(64, 7, 21), (0, 3)).permute(0, 2, 1).contiguous().cuda()   # [co][24][ky]
    ne = lib.ustrun_pack_conv_elems_dtype(64, 24, 7, X3)
    assert ne >= 2.5 * 64 * 24 * 7 and lib.ustrun_pack_conv_elems_dtype(64, 24, 7, 0) == lib.ustrun_pack_conv_elems(64, 24, 7)
    wf = torch.zeros(ne, device="cuda")
    l.check(lib.ustrun_pack_conv(wr.data_ptr(), 64, 24, 7, wf.data_ptr(), X3, None))
    yo = torch.empty(n, ho, wo, 64, device="cuda")
    l.check(lib.ustrun_conv_rowwin_fwd(C.byref(src), wf.data_ptr(), n, ho, wo, 64, 7, 2, yo.data_ptr(), None, None, X3, None))
    assert rel(from_nhwc(yo), ref) < 1e-6
    pb = lib.ustrun_wgrad_partials_bytes(7, 24, 64, n * ho * wo)
    part = torch.empty(pb, dtype=torch.uint8, device="cuda")
    dwr = torch.empty(64, 24, 7, device="cuda")
    l.check(lib.ustrun_conv_rowwin_wgrad(C.byref(src), nhwc(dy).data_ptr(), n, ho, wo, 64, 7, 2, dwr.data_ptr(), 0, part.data_ptr(), pb, X3, None))
    got = dwr[:, :21].reshape(64, 7, 3, 7).permute(0, 2, 3, 1).cpu()       # [co][kx][ci][ky] -> [co][ci][ky][kx]
    assert torch.equal(got, want)


@pytest.mark.parametrize("n,ci,co,h,w,k,s,d", [(2, 64, 64, 17, 23, 1, 1, 1), (2, 256, 128, 16, 12, 1, 2, 1), (2, 128, 128, 14, 18, 3, 1, 2)])
def test_conv2d_fwd_x3_packed_planes(n, ci, co, h, w, k, s, d):
    """ustrun_conv2d_fwd with dtype 3 reads the three bf16 planes ustrun_pack_conv writes behind the f32 pack (a buffer of
    ustrun_pack_conv_elems_dtype elements): a 1x1, a strided 1x1 and a dilated 3x3 of test_conv2d_general's list, small integers,
    rel < 1e-6 as that test asserts for f32, plus the BatchNorm-statistics rows."""
    l = L()
    lib = l.lib()
    g = torch.Generator().manual_seed(ci + co + k + d)
    x = torch.randint(-3, 4, (n, ci, h, w), generator=g).float()
    wt = torch.randint(-2, 3, (co, ci, k, k), generator=g).float()
    ref = F.conv2d(x, wt, None, s, d * (k // 2), d)
    ho, wo = ref.shape[-2:]
    ne = lib.ustrun_pack_conv_elems_dtype(co, ci, k * k, X3)
    assert 2 * ne >= 5 * co * ci * k * k
    wf = torch.zeros(ne, device="cuda")
    wg = wt.cuda()
    l.check(lib.ustrun_pack_conv(wg.data_ptr(), co, ci, k * k, wf.data_ptr(), X3, None))
    # the planes are there: plane 0 of tap 0 holds the weights' leading bf16 terms as [Cin/8][Cout][8]
    planes = wf[k * k * ci * co:].view(torch.bfloat16)[:ci * co].float().reshape(ci // 8, co, 8).cpu()
    assert torch.equal(planes, wt[:, :, 0, 0].t().reshape(ci // 8, 8, co).permute(0, 2, 1))
    xg = nhwc(x)
    src = l.nhwc_src(xg.data_ptr(), ci, h, w)
    y = torch.empty(n, ho, wo, co, device="cuda")
    rows = lib.ustrun_conv_mtiles(n, ho, wo, co)
    stat = torch.zeros(rows, 2, co, device="cuda")
    used = C.c_int(0)
    l.check(lib.ustrun_conv2d_fwd(C.byref(src), 1, wf.data_ptr(), None, n, ho, wo, co, k, s, d, y.data_ptr(), 0, stat.data_ptr(), C.byref(used),
                                  X3, None))
    assert rel(from_nhwc(y), ref) < 1e-6
    assert 0 < used.value <= rows
    np.testing.assert_allclose(stat[:, 0].sum(0).cpu().numpy(), ref.sum((0, 2, 3)).numpy(), rtol=1e-5, atol=1e-2)


def _model(arch, k, seed, dtype):
    from networks.deeplabv2 import DeepLabV2
    torch.manual_seed(seed)
    return DeepLabV2(arch, k, pretrained=False, dtype=dtype).cuda()


def test_deeplab_x3_vs_oracle():
    """test_deeplab_vs_oracle's construction with dtype "f32x3": resnet50 on an odd-extent input, train then eval mode, at the f32
    bar (5e-4 rel-L2 of the CPU oracle)."""
    from oracle import deeplab_ref as D
    sd = D.make_state_dict("resnet50", 4, 21)
    m = _model("resnet50", 4, 21, "f32x3").train()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 72, 104, generator=g)
    with torch.no_grad():
        sdo = {k: v.clone() for k, v in sd.items()}
        ref = D.deeplabv2_forward(x, sdo, "resnet50", True)
        got = m(x.cuda()).cpu()
        assert got.shape == ref.shape
        e_train = rel(got, ref)
        m.eval()
        ref_e = D.deeplabv2_forward(x, sdo, "resnet50", False)
        e_eval = rel(m(x.cuda()).cpu(), ref_e)
    print(f"deeplab f32x3: train rel-L2 {e_train:.2e}, eval {e_eval:.2e}")
    assert e_train < 5e-4 and e_eval < 5e-4


def test_deeplab_x3_reference_golden():
    """dtype "f32x3" against the logits captured from the reference's own modules (g10_deeplabv2_r50_n2_96x80): the sampled
    train-mode and eval-mode values within 5e-4, the f32 path's bar."""
    g = load_golden("g10_deeplabv2_r50_n2_96x80")
    n, _, h, w, k = [int(v) for v in g["shape"]]
    m = _model("resnet50", k, int(g["model_seed"]), "f32x3").train()
    gen = torch.Generator().manual_seed(int(g["input_seed"]))
    x = (torch.randint(0, 256, (n, 3, h, w), generator=gen).float() / 127.5 - 1).cuda()
    idx = torch.from_numpy(g["sample_idx"])
    with torch.no_grad():
        tr = m(x).flatten().cpu()
        m.eval()
        ev = m(x).flatten().cpu()
    e_tr, e_ev = rel(tr[idx], torch.from_numpy(g["sample_val"])), rel(ev[idx], torch.from_numpy(g["eval_val"]))
    print(f"deeplab f32x3 vs reference golden: train samples {e_tr:.2e}, eval samples {e_ev:.2e}")
    assert e_tr < 5e-4 and e_ev < 5e-4


def _oracle_grads(x, sd, arch, R, dt=torch.float32):
    from oracle import deeplab_ref as D
    sdo = {}
    for k, v in sd.items():
        v = v.clone().to(dt) if v.is_floating_point() else v.clone()
        sdo[k] = v.requires_grad_(True) if v.is_floating_point() and "running" not in k else v
    out = D.deeplabv2_forward(x.to(dt), sdo, arch, True)
    (out * R.to(dt)).sum().backward()
    return out.detach(), {k: v.grad for k, v in sdo.items() if v.requires_grad}


def _field_stats(got, ref):
    """(worst per-tensor rel-L2, its name, cosine of the concatenated gradient, norm ratio)"""
    worst, dots, n1, n2 = (0.0, ""), 0.0, 0.0, 0.0
    for k in ref:
        e = rel(got[k], ref[k])
        if e > worst[0]:
            worst = (e, k)
        dots += float((got[k].double() * ref[k].double()).sum())
        n1 += float(got[k].double().norm() ** 2); n2 += float(ref[k].double().norm() ** 2)
    return worst[0], worst[1], dots / (n1 ** 0.5 * n2 ** 0.5), (n1 / n2) ** 0.5


@pytest.mark.parametrize("h,w,K", [(96, 80, 2), (100, 76, 4)])
def test_deeplab_x3_backward_vs_oracle(h, w, K):
    """test_deeplab_backward_vs_oracle_f32's construction and criteria with dtype "f32x3": every parameter's gradient of
    loss = <logits, R> against autograd over the CPU oracle in FLOAT64; the oracle's own float32 evaluation (CPU, never the code
    under test) is the yardstick -- worst per-tensor error < 2x its worst, cosine > its cosine - 5e-4, norm ratio within 5e-3.  The
    weight gradients run on the side stream as for the other dtypes; 100 x 76 enters the stride-2 convolutions with odd extents."""
    from networks.deeplabv2 import DeepLabV2
    from oracle import deeplab_ref as D
    sd = D.make_state_dict("resnet50", K, 23)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, h, w, generator=g)
    R = torch.randn(2, K, h, w, generator=g)
    ref_out, ref = _oracle_grads(x, sd, "resnet50", R, torch.float64)
    _, o32 = _oracle_grads(x, sd, "resnet50", R, torch.float32)
    m = DeepLabV2("resnet50", K, pretrained=False, dtype="f32x3")
    m.load_state_dict(sd)
    m = m.cuda().train()
    out = m(x.cuda())
    assert out.requires_grad
    (out * R.cuda()).sum().backward()
    got = {}
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, k
        got[k] = p.grad.cpu()
        assert torch.isfinite(got[k]).all(), k
    assert set(got) == set(ref)
    wst, wk, cos, ratio = _field_stats(got, ref)
    yw, ywk, ycos, _ = _field_stats(o32, ref)
    print(f"deeplab backward f32x3: logits rel {rel(out.detach().cpu(), ref_out):.2e}; vs f64 oracle: worst grad rel-L2 {wst:.2e} ({wk}), "
          f"cosine {cos:.5f}, norm ratio {ratio:.3f}; f32 oracle: worst {yw:.2e} ({ywk}), cosine {ycos:.5f}")
    assert wst < 2 * yw and cos > ycos - 5e-4 and abs(ratio - 1) < 5e-3


def test_deeplab_x3_public_surface():
    """DeepLabV2(..., dtype="f32x3") constructs and trains: three SGD steps on the 64 x 64 disc target of
    test_deeplab_sgd_steps_reduce_loss (lr per step 0.1 L / |g|^2) leave the loss of the fixed batch at least 10 % lower -- so the
    packed planes followed the in-place updates.  Directly: after an in-place update of convolution weights the next forward equals
    that of a fresh model built from the updated state (the f32 pack AND its planes were refreshed)."""
    from networks.deeplabv2 import DeepLabV2
    m = _model("resnet50", 2, 5, "f32x3").train()
    assert m.compute_dtype == "f32x3" and m.backbone.compute_dtype == "f32x3"
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(4, 3, 64, 64, generator=g).cuda()
    yy, xx = torch.meshgrid(torch.arange(64), torch.arange(64), indexing="ij")
    tgt = ((yy - 32) ** 2 + (xx - 32) ** 2 < 300).long().expand(4, 64, 64).contiguous().cuda()
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = F.cross_entropy(m(x), tgt)
        loss.backward()
        losses.append(float(loss.detach()))
        g2 = sum(float(p.grad.double().pow(2).sum()) for p in m.parameters())
        opt.param_groups[0]["lr"] = 0.1 * losses[-1] / g2
        opt.step()
    with torch.no_grad():
        losses.append(float(F.cross_entropy(m(x), tgt)))
        print("deeplab f32x3 sgd losses", [round(v, 4) for v in losses])
        assert losses[-1] < 0.9 * losses[0]
        m.eval()
        before = m(x)
        m.backbone.layer1[0].conv1.weight.mul_(1.5)
        m.backbone.layer4[0].conv2.weight.add_(0.01)
        m.classifier[1].weight.mul_(-2.0)
        after = m(x)
        fresh = DeepLabV2("resnet50", 2, pretrained=False, dtype="f32x3")
        fresh.load_state_dict(m.state_dict())
        want = fresh.cuda().eval()(x)
    assert rel(after.cpu(), before.cpu()) > 1e-2
    assert torch.equal(after, want)
