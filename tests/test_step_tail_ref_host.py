"""tests/step_tail_ref.py pinned on the CPU: against torch float64 (F.cross_entropy, F.binary_cross_entropy_with_logits, autograd,
torch.optim.SGD), oracle/losses_ref, oracle/host_ref, oracle/step_ref and utils.metrics, all in double.  It also shows that the caps of
tests/test_gpu_step_tail_ops.py are met by the reference alone: the 0.1 % zone of the pseudo-label cases, and the derived bounds of
box_mix and sgd_ema by a float32 evaluation of the kernels' expressions on the CPU."""
import itertools
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import step_tail_ref as R
from oracle import host_ref as H
from oracle import losses_ref as LR
from oracle import step_ref as S

SM, SG = R.SOFTMAX, R.SIGMOID
T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()


def close(a, b, rtol=1e-10, atol=1e-12):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def seg_case(mode, N, K, HW, mask, seed=0):
    rng = np.random.default_rng(seed + K + HW)
    x = (3 * rng.normal(size=(N, K, HW))).astype(np.float32)
    if mode == SM:
        t, ms = rng.integers(0, K, size=(N, HW)), (N, HW)
    else:
        t, ms = (rng.random((N, K, HW)) > 0.5).astype(np.float32), (N, K, HW)
    m = {None: None, "01": (rng.random(ms) > 0.4).astype(np.float32), "zero": np.zeros(ms, np.float32),
         "half": rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=ms)}[mask]
    return x, t, m


@pytest.mark.parametrize("mode,shape,mask", [(SM, (2, 3, 35), None), (SM, (2, 3, 35), "half"), (SM, (1, 8, 77), "01"), (SM, (1, 1, 5), "zero"),
                                             (SG, (2, 3, 35), None), (SG, (2, 3, 35), "01"), (SG, (1, 2, 9), "zero")])
def test_seg_loss_against_torch_and_the_oracle(mode, shape, mask, monkeypatch):
    monkeypatch.setattr(LR, "SMOOTH", R.SMOOTH)                                 # the kernels' constant is the float 1e-10f
    N, K, HW = shape
    x, t, m = seg_case(mode, N, K, HW, mask)
    out = R.seg_loss_fwd(x, t, m, mode)
    lg = T64(x).view(N, K, HW, 1).requires_grad_(True)
    if mode == SM:
        tt = torch.from_numpy(t).view(N, HW, 1)
        mm = None if m is None else T64(m).view(N, 1, HW, 1)
        ce = F.cross_entropy(lg, tt, reduction="none")
        ce = ce.mean() if mm is None else (ce * mm[:, 0]).mean()
    else:
        tt = T64(t).view(N, K, HW, 1)
        mm = None if m is None else T64(m).view(N, K, HW, 1)
        ce = F.binary_cross_entropy_with_logits(lg, tt, reduction="none")
        ce = ce.mean() if mm is None else (ce * mm).mean()
    oce, odc = LR.seg_loss(lg, tt, mm, "softmax" if mode == SM else "sigmoid", K)
    close(out[0], ce.item())
    close(out[0], oce.item())
    close(out[1], odc.item())
    close(out[2], out[0] * (N * HW if mode == SM else N * K * HW))
    kk = K if mode == SM else 1
    assert np.isnan(out[3 + 3 * kk:]).all() and np.isfinite(out[:3 + 3 * kk]).all()
    for gdev, gscale, (cw, dw) in [(None, 1.0, (1.0, 1.0)), ((2.0, -0.5), 1024.0, (0.5, 0.0)), ((2.0, -0.5), 1.0, (0.0, 0.7))]:
        g0, g1 = (1.0, 1.0) if gdev is None else gdev
        (grad,) = torch.autograd.grad(gscale * (cw * g0 * ce + dw * g1 * odc), lg, retain_graph=True)
        got = R.seg_loss_bwd(x, t, m, mode, np.where(np.isnan(out), 0.0, out), gdev, gscale, cw, dw)
        close(got, grad.view(N, K, HW).numpy(), rtol=1e-9, atol=1e-12 * gscale)


DICE_FORMS = [(0, ti, 1, mk) for ti in (1, 0) for mk in (None, "pix")] + [(1, 0, tp, mk) for tp in (0, 1) for mk in (None, "full", "pix")]


@pytest.mark.parametrize("act,form", list(itertools.product((0, 1, 2), DICE_FORMS)))
@pytest.mark.parametrize("smooth", [1e-10, 1e-5])
def test_dice_against_the_oracle_in_double(act, form, smooth, monkeypatch):
    monkeypatch.setattr(LR, "SMOOTH", R.f32(smooth))
    multi, ti, tper, mk = form
    N, K, HW = 2, 3, 35
    rng = np.random.default_rng(act + 10 * multi + tper)
    x = (2 * rng.normal(size=(N, K, HW))).astype(np.float32)
    if not multi:
        t = rng.choice(np.array([0, 2]), size=(N, HW))                          # class 1 is absent
        t = t.astype(np.int64) if ti else t.astype(np.float32)
        m = None if mk is None else rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=(N, HW))
    else:
        t = (rng.random((N, HW) if tper else (N, K, HW)) > 0.5).astype(np.float32)
        m = None if mk is None else (rng.random((N, HW) if mk == "pix" else (N, K, HW)) > 0.4).astype(np.float32)
    mper = int(mk != "full")
    pix = lambda a: torch.from_numpy(a).view(N, 1, HW, 1)
    lg = T64(x).view(N, K, HW, 1).requires_grad_(True)
    tt = pix(t) if (not multi or tper) else torch.from_numpy(t).view(N, K, HW, 1)
    mm = None if m is None else (pix(m) if mper else torch.from_numpy(m).view(N, K, HW, 1))
    if act == 2:
        tt = tt.unsqueeze(1)                                                    # (the reference squeezes dim 1 of a sigmoid target)
    for w in ([None] if multi else [None, [0.25, 0.75, 1.25]]):
        val = LR.dice_loss_with_mask(lg, tt, K, mask=mm, weight=w, softmax=act == 1, sigmoid=act == 2, multi=bool(multi))
        out = R.dice_fwd(x, t, m, act, multi, tper, mper, w, smooth)
        close(out[0], val.item())
        if not multi:
            assert out[2] == 0 and out[1 + 2 * K + 1] == 0
        (grad,) = torch.autograd.grad(-1.5 * 1024.0 * val, lg)
        got = R.dice_bwd(x, t, m, act, multi, tper, mper, out, w, smooth, (-1.5, 9.0), 1024.0)
        close(got, grad.view(N, K, HW).numpy(), rtol=1e-9, atol=1e-9)


def test_y_is_counted_once_for_a_per_pixel_target():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(2, 3, 7)).astype(np.float32)
    t = np.ones((2, 7), np.float32)
    assert R.dice_fwd(x, t, None, 0, 1, 1, 1)[1 + 2 * 3] == 14                  # not 3 x 14
    assert R.dice_fwd(x, t, np.ones((2, 3, 7), np.float32), 0, 1, 1, 0)[1 + 2 * 3] == 42


PSEUDO = [(mode, shp, th) for mode in (SM, SG) for shp in R.PSEUDO_SHAPES for th in R.PSEUDO_THRESHOLDS]


@pytest.mark.parametrize("mode,shape,th", PSEUDO + [(SM, (1, 2, 1048583), 0.95), (SG, (1, 2, 524803), 0.95)])
def test_pseudo_label_against_the_oracle_and_the_zone_cap(mode, shape, th):
    N, K, HW = shape
    x, planted = R.pseudo_label_case(N, K, HW)
    lab, msk, p = R.pseudo_label(x, th, mode)
    ol, om = LR.pseudo_label(T64(x).view(N, K, HW, 1), R.f32(th), "softmax" if mode == SM else "sigmoid")
    if mode == SM:
        assert np.array_equal(lab, ol.view(N, HW).numpy()) and np.array_equal(msk, om.view(N, HW).numpy())
    else:
        assert np.array_equal(lab, ol.view(N, K, HW).numpy())
        lo = float(np.float32(1) - np.float32(th))                              # the kernel's 1.f - th; the oracle takes 1 - th in double
        same = np.abs(p - lo) > 1e-7
        assert np.array_equal(msk[same], om.view(N, K, HW).numpy()[same])
    lab_ok, mask_ok, lz, mz = R.pseudo_label_accept(x, th, mode, lab, msk)
    assert lab_ok.all() and mask_ok.all()
    pl = planted if mode == SM else np.broadcast_to(planted[:, None, :], shape)
    zone = (lz | mz) & ~pl
    assert zone.sum() <= R.PSEUDO_ZONE_CAP * zone.size, (int(zone.sum()), zone.size)
    if mode == SG and th == 0.5 and HW >= 12:
        assert (msk[0, :, :4] == 2).all()
    # a float32 evaluation on the CPU is accepted too, and a wrong answer outside the zone is not
    x32 = torch.from_numpy(x)
    if mode == SM:
        p32 = torch.softmax(x32, 1)
        c32, l32 = p32.max(1)
        l_ok, m_ok, _, _ = R.pseudo_label_accept(x, th, mode, l32.numpy(), (c32 > np.float32(th)).double().numpy())
    else:
        p32 = torch.sigmoid(x32)
        m32 = (p32 >= np.float32(th)).double() + (p32 <= np.float32(1) - np.float32(th)).double()
        l_ok, m_ok, _, _ = R.pseudo_label_accept(x, th, mode, (p32 >= 0.5).double().numpy(), m32.numpy())
    assert l_ok.all() and m_ok.all()
    if K > 1 or mode == SG:
        wrong = (lab + 1) % K if mode == SM else 1 - lab
        l_bad, _, _, _ = R.pseudo_label_accept(x, th, mode, wrong, msk)
        assert (~l_bad & ~lz).sum() == (~lz).sum()


@pytest.mark.parametrize("mode", [SM, SG])
def test_mix_targets_box_mix_against_the_oracle(mode):
    N, K, HW = 3, 2, 24
    rng = np.random.default_rng(mode)
    box = (rng.random((N, HW)) > 0.5).astype(np.float32)
    box[0], box[1] = 0, 1
    ls = (N, HW) if mode == SM else (N, K, HW)
    lab = (lambda: rng.integers(0, 4, size=ls)) if mode == SM else (lambda: (rng.random(ls) > 0.5).astype(np.float32))
    msk = lambda: (rng.random(ls) > 0.3).astype(np.float32)
    ins = [lab(), msk(), lab(), msk(), lab(), msk(), lab(), msk()]
    ref = R.mix_targets(mode, box, *ins)
    tl = lambda a: torch.from_numpy(a).view(*((N, HW, 1) if mode == SM else (N, K, HW, 1)))
    tm = lambda a: torch.from_numpy(a).double().view(*((N, 1, HW, 1) if mode == SM else (N, K, HW, 1)))
    lt = (lambda a: tl(a)) if mode == SM else (lambda a: tl(a).double())
    o = LR.mix_targets("softmax" if mode == SM else "sigmoid", lt(ins[0]), tm(ins[1]), lt(ins[2]), tm(ins[3]), lt(ins[4]), tm(ins[5]),
                       torch.from_numpy(box).double().view(N, HW, 1), lt(ins[6]), tm(ins[7]))
    for r, q in zip(ref, o):
        assert np.array_equal(np.asarray(r, np.float64).reshape(-1), q.double().numpy().reshape(-1))
    a, b = rng.normal(size=(N, 3, HW)).astype(np.float32), rng.normal(size=(N, 3, HW)).astype(np.float32)
    eighths = (rng.integers(0, 9, size=(N, HW)) / 8.0).astype(np.float32)
    v, mag = R.box_mix(a, b, eighths)
    bx = eighths[:, None]
    close(v, a.astype(np.float64) * (1 - bx) + b.astype(np.float64) * bx)
    f32v = a * (np.float32(1) - bx) + b * bx                                   # the kernel's expression in float32 meets its bound
    assert (np.abs(f32v - v) <= 3 * R.U * mag * (1 + 2.0 ** -20)).all()
    v01, _ = R.box_mix(a, b, box)
    assert np.array_equal(v01.astype(np.float32), a * (np.float32(1) - box[:, None]) + b * box[:, None])


def test_decode_labels_against_the_oracle():
    rng = np.random.default_rng(1)
    vals = np.array([0.0, -0.0, 1.0, 127.5, 128.0, 129.0, 255.0], np.float32)
    y = rng.choice(vals, size=(2, 5, 7))
    for kind, name in enumerate(["fundus", "prostate", "BUSI"]):
        ref = S.decode_labels(name, torch.from_numpy(y))
        assert np.array_equal(R.decode_labels(y.reshape(2, 35), kind), ref.numpy().reshape(2, *([2, 35] if kind == 0 else [35])))
    y3 = rng.choice(vals, size=(2, 5, 7, 3), p=[.1, .1, .1, .1, .1, .1, .4])
    assert np.array_equal(R.decode_labels(y3.reshape(2, 35, 3), 3), S.decode_labels("MNMS", torch.from_numpy(y3)).numpy().reshape(2, 35))


def test_region_bbox_and_rect_masks_against_the_cover_box():
    rng = np.random.default_rng(2)
    for S_ in (40, 300):
        for trial in range(4):
            planes = [np.zeros(S_ * S_, np.float32), np.zeros(S_ * S_, np.int64)]
            for p in planes:
                p[rng.integers(0, S_ * S_, size=1 + trial)] = 3
            region = ((planes[0] != 0) | (planes[1] != 0)).reshape(S_, S_).astype(np.float32)
            tab = R.region_bbox(planes, S_, S_)
            assert tab.shape == (64, 4) and tab.dtype == np.int32
            rect = R.fold_bbox(tab)
            assert np.array_equal(R.rect_masks([rect], S_, S_)[0], H.all_cover_box(region))
    tab = R.region_bbox([np.zeros(37 * 53)], 37, 53)
    assert (tab == np.array([37, -1, 53, -1])).all() and R.fold_bbox(tab) is None
    one = np.zeros(37 * 53)
    one[37 * 53 - 1] = 1
    tab = R.region_bbox([one], 37, 53)                                           # element 1960: block (1960 // 256) % 64 = 7
    assert (tab[7] == [36, 36, 52, 52]).all() and (np.delete(tab, 7, 0) == [37, -1, 53, -1]).all()
    random.seed(3); np.random.seed(3)
    ref = H.cutmix_box(64, p=1.0)
    loc = np.argwhere(ref != 0)
    r = (loc[:, 0].min(), loc[:, 0].max() + 1, loc[:, 1].min(), loc[:, 1].max() + 1)
    assert np.array_equal(R.rect_masks([r], 64, 64)[0], ref)
    assert R.rect_masks([(5, 5, 0, 9), (-4, 0, 0, 9), (0, 9, 9, 12), (-3, 20, -3, 20)], 9, 9).sum(axis=(1, 2)).tolist() == [0, 0, 0, 81]


def test_dice_counts_against_utils_metrics_and_the_oracle():
    from utils import metrics
    rng = np.random.default_rng(3)
    p, g = rng.integers(0, 2, size=(3, 2, 100)), rng.integers(0, 2, size=(3, 2, 100))
    c = R.dice_counts(p.astype(np.float32), g, 2, 0).astype(np.float64)
    assert c.shape == (3, 2, 3)
    d = metrics.dice_from_counts(c[..., 0], c[..., 1], c[..., 2])
    for n in range(3):
        for k in range(2):
            close(d[n, k], H.dice_binary(p[n, k], g[n, k]))
    pc, gc = rng.integers(0, 5, size=(2, 400)), rng.integers(0, 5, size=(2, 400))
    c = R.dice_counts(pc + 0.5, gc.astype(np.float32), 3, 1)                    # floats truncate towards zero
    for k in range(3):
        assert np.array_equal(c[:, k, 0], (pc == k + 1).sum(1)) and np.array_equal(c[:, k, 2], ((pc == k + 1) & (gc == k + 1)).sum(1))
    assert [R.dice_split(*s) for s in [(1, 1, 4096), (2, 3, 70001), (3, 2, 100), (16, 2, 65536)]] == [2, 32, 1, 16]


@pytest.mark.parametrize("t_on,gsc,scale", [(True, 1.0, None), (False, 0.5, None), (True, 0.5, 1024.0)])
def test_sgd_ema_against_torch_sgd_in_double(t_on, gsc, scale):
    n, lr, mu, wd, alpha = 1023, 0.03, 0.9, 1e-4, 0.99
    rng = np.random.default_rng(4)
    p0 = rng.normal(size=n).astype(np.float32)
    f = R.f32
    pr = T64(p0).clone().requires_grad_(True)
    opt = torch.optim.SGD([pr], lr=f(lr), momentum=f(mu), weight_decay=f(wd))
    p, v, t = p0.astype(np.float64), np.zeros(n), (0.5 * p0.astype(np.float64) if t_on else None)
    tr = None if t is None else t.copy()
    for step in range(3):
        g = rng.normal(size=n).astype(np.float32)
        pr.grad = T64(g) * f(gsc)
        opt.step()
        (p, v, t), (ep, ev, et) = R.sgd_ema(p, g * (scale or 1.0), v, t, lr, mu, wd, step == 0, alpha, gsc, scale=scale)
        close(p, pr.detach().numpy(), rtol=1e-12)
        close(v, opt.state[pr]["momentum_buffer"].numpy(), rtol=1e-12)
        if t_on:
            tr = f(alpha) * tr + float(np.float32(1) - np.float32(alpha)) * pr.detach().numpy()
            close(t, tr, rtol=1e-12)
    # the kernel's expression in float32 on the CPU stays inside the derived bounds; a skipped step leaves p and v alone
    F32 = np.float32
    g, v0, t0 = (rng.normal(size=n).astype(F32) for _ in range(3))
    for first in (0, 1):
        (rp, rv, rt), (ep, ev, et) = R.sgd_ema(p0, g, v0, t0, lr, mu, wd, first, alpha, gsc, scale=scale)
        c = F32(gsc) / F32(scale) if scale else F32(gsc)
        gv = g * c + F32(wd) * p0
        vv = gv if first else F32(mu) * v0 + gv
        pv = p0 - F32(lr) * vv
        tv = F32(alpha) * t0 + (F32(1) - F32(alpha)) * pv
        assert (np.abs(vv - rv) <= ev).all() and (np.abs(pv - rp) <= ep).all() and (np.abs(tv - rt) <= et).all()
        assert ev.max() < 1e-6 and ep.max() < 1e-6 and et.max() < 1e-6           # ... and the bounds are a few ulp, not a tolerance
    (rp, rv, rt), (ep, ev, _) = R.sgd_ema(p0, g, v0, t0, lr, mu, wd, 0, alpha, gsc, scale=1024.0, skip=True)
    assert np.array_equal(rp, p0) and np.array_equal(rv, v0) and not ep.any() and not ev.any() and not np.array_equal(rt, t0)


def test_amp_update_follows_gradscaler():
    s = np.array([1024.0, 1024.0, 0, 0, 0, 0, -3.5, 42.0], np.float32)
    scale, tracker, skipped = 1024.0, 0, 0
    for step, found in enumerate([0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0]):
        s[3] = found
        s = R.amp_update(s, 2.0, 0.5, 3)
        if found:                                                               # GradScaler.update(): back off, reset the tracker
            scale, tracker, skipped = scale * 0.5, 0, skipped + 1
        else:
            tracker += 1
            if tracker == 3:
                scale, tracker = scale * 2.0, 0
        assert s.tolist() == [scale, scale, tracker, 0, skipped, step + 1, -3.5, 42.0]
    assert R.amp_update(s, 2.0, 0.5, 1)[0] == 2 * scale
    assert R.amp_check(np.array([1.0, np.finfo(np.float32).max, 1e-45], np.float32)) == 0
    assert R.amp_check(np.array([1.0, np.inf])) == 1 and R.amp_check(np.array([np.nan, 1.0])) == 1


@pytest.mark.parametrize("C_,H_,W_,b", [(1, 8, 8, 0), (3, 16, 12, 1), (1, 5, 7, 1), (1, 33, 47, 2), (2, 64, 40, 3), (1, 100, 100, 4), (1, 50, 131, 5)])
def test_freq_mix_against_the_oracle_and_its_two_stage_form(C_, H_, W_, b):
    rng = np.random.default_rng(b)
    img = lambda: rng.integers(0, 256, size=(3, C_, H_, W_)).astype(np.float32) / np.float32(127.5) - np.float32(1)
    src, trg, ratios = img(), img(), [0.0, 0.37, 1.0]
    ref = R.freq_mix(src, trg, ratios, b)
    close(ref[0], src.astype(np.float64)[0], rtol=0, atol=1e-12)                 # ratio 0: the source
    if H_ == W_ and b > 0:                                                      # the oracle's window is floor(min(h, w) L)
        Lb = (b + 0.5) / H_
        for i, r in enumerate(ratios):
            S64, T64_ = (src[i].astype(np.float64) + 1) * 127.5, (trg[i].astype(np.float64) + 1) * 127.5
            o = H.freq_mix(S64, H.amp_spectrum(T64_), L=Lb, ratio=R.f32(r))
            close(ref[i], np.clip(o, 0, 255) / 127.5 - 1, rtol=0, atol=1e-11)
    for s_, r_ in ((src, ratios), (np.full_like(src, -1.0), ratios), ((rng.integers(0, 2, size=src.shape) * 2 - 1).astype(np.float32), [1.0] * 3)):
        full = R.freq_mix(s_, trg, r_, b)
        close(R.freq_mix_two_stage(s_, trg, r_, b, np.float64), full, rtol=0, atol=1e-9)
        y = R.freq_mix_two_stage(s_, trg, r_, b)
        assert y.dtype == np.float32 and np.abs(y - full).max() < 2e-5          # float32 itself meets the atol cap
