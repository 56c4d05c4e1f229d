"""The kernels of the step's tail (csrc/loss.hip, csrc/fftmix.hip), one C-ABI call at a time against the float64 restatement of
tests/step_tail_ref.py (pinned on the CPU by tests/test_step_tail_ref_host.py).  Every output -- out, partials, dlogits, counts, the
bbox table, the FFT work buffer, amp_state -- lies between two 4096-element guard zones and starts as the sentinel; no element is
excluded from any comparison.  Items are written (N, K, HW).  u = 2^-24.

Bars, derived, not tuned:
  integer and copy outputs   bit for bit.
  box_mix                    fl(fl(a fl(1 - x)) + fl(b x)): three roundings on the first product, two on the second:
                             3u (|a (1 - x)| + |b x|) (1 + 2^-20).  With x in {0, 1} every operation is exact: bit for bit.
  sgd_ema / sgd_ema_scaled   the kernel's expression, one rounding of u |result| per operation, errors of the operands carried along
                             (step_tail_ref.sgd_ema):  gv = g c + wd p: u (|g c| + |wd p| + |gv|), plus u |g c| for c = gsc / scale;
                             v' = mu v + gv: u |mu v| + e(gv) + u |v'|;  p' = p - lr v': lr e(v') + u |lr v'| + u |p'|;
                             t' = alpha t + (1 - alpha) p': u |alpha t| + (1 - alpha) e(p') + u |(1 - alpha) p'| + u |t'|, with
                             1 - alpha the float the kernel computes.  An FMA contraction only removes roundings.
  reduced sums               out[2..] of seg_loss, out[1..] of dice: (T + 9) u sum|term| + 4 sum|term32 - term64|: T = the trips of one
                             thread (T - 1 roundings), 6 shuffle levels, 3 adds of the four waves, the partial rows are summed in
                             double and rounded once; term32 = the same terms evaluated in float32 on the CPU.  The scalars out[0]
                             (/ count) and the Dice values carry that bound through the quotient (interval evaluation at I -+ dI,
                             D +- dD) plus one rounding.
  maps through expf / logf / sincosf   the two dlogits and the freq_mix output: device max-abs error <= max(4 x the error of the float32
                             CPU restatement against float64, 8 u max|expected|) (the rule of test_gpu_losses_rest.py); for freq_mix the
                             restatement is the kernel's two-stage form in complex64 and atol = 2e-5 stays as an upper cap.
  pseudo labels              every label and mask element equals the float64 result OR its float64 probability lies within the error
                             of p (step_tail_ref.pseudo_label_p_err) of the decision boundary; outside the planted pixels at most
                             0.1 % of a case's elements may lie there (asserted here and, by the reference alone, on the CPU).
Each worst error / bound is printed (pytest -s).
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import step_tail_ref as R
from test_gpu_bn_forward_ops import SENT, L, Out, hold

pytestmark = pytest.mark.gpu

U = R.U
SM, SG = R.SOFTMAX, R.SIGMOID
CAP_ITEMS = 1024 * 1024          # stream_blocks' 1024 blocks of 256 threads, four items each


def dev(a, tdt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if tdt is None else t.to(tdt)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def sentinel(o):
    return o.guards_ok() and bool((o.t == SENT).all())


def bits(o, ref, tdt):
    """the output's elements equal ref (cast to the output's type) bit for bit; the guards are whole"""
    assert o.guards_ok(), "a guard zone was written"
    want = torch.from_numpy(np.ascontiguousarray(ref)).to(tdt).reshape(o.t.shape)
    got = o.t.cpu()
    if tdt.is_floating_point:
        got, want = got.view(torch.int32), want.view(torch.int32)
    bad = got != want
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} differ; first at {bad.flatten().nonzero()[0].item()}"


def yardstick(what, got, want, yard, cap=None):
    err = float(np.abs(got - want).max())
    y = float(np.abs(yard.astype(np.float64) - want).max())
    bar = max(4 * y, 8 * U * float(np.abs(want).max()))
    if cap is not None:
        bar = min(bar, cap)
    print(f"{what}: err {err:.3g} yardstick {y:.3g} bar {bar:.3g} err/bar {err / bar if bar else 0:.3g}")
    assert np.isfinite(got).all() and err <= bar, (what, err, y, bar)


def sum_bound(t64, t32, T):
    """(T + 9) u sum|term| + 4 sum|term32 - term64| over the last axis"""
    return (T + 9) * U * np.abs(t64).sum(-1) + 4 * np.abs(t32.astype(np.float64) - t64).sum(-1)


def dice_bound(I, Z, Y, dI, dZ, dY, smooth):
    """|dice(I', Z', Y') - dice(I, Z, Y)| for |I' - I| <= dI ...: the quotient at the corners of the box, one rounding on top"""
    D, dD = Z + Y + smooth, dZ + dY
    r = (2 * I + smooth) / D
    assert D - dD > 0
    hi, lo = (2 * (I + dI) + smooth) / (D - dD), (2 * (I - dI) + smooth) / (D + dD)
    return max(hi - r, r - lo) * (1 + 2.0 ** -20)


# ---- seg_loss -----------------------------------------------------------------------------------------------------------------------
SEG_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 8, 77), (3, 2, 1089), (2, 4, 1600)]
SEG_ROWS = {SM: [(34, (1, 2, 33793)), (98, (2, 2, 49665)), (130, (1, 3, 132097)), (1024, (2, 2, 524801))],
            SG: [(34, (1, 1, 33793)), (98, (1, 2, 49665)), (130, (1, 1, 132097)), (1024, (1, 2, 524801))]}
SEG_CASES = [(mode, shp, mask, False) for mode in (SM, SG) for shp in SEG_SHAPES
             for mask in ((None, "01", "zero", "half") if mode == SM else (None, "01", "zero"))]
SEG_CASES += [(mode, (2, 4, 1600), "01", True) for mode in (SM, SG)]
SEG_CASES += [(mode, shp, "half" if mode == SM else "01", False) for mode in (SM, SG) for _, shp in SEG_ROWS[mode]]
GRADS = list(itertools.product((None, (2.0, -0.5)), (1.0, 1024.0), ((1.0, 1.0), (0.5, 0.0), (0.0, 0.7))))


def seg_inputs(mode, shape, mask, extreme):
    N, K, HW = shape
    rng = np.random.default_rng(N * 1000003 + K * 1009 + HW + 7 * mode)
    x = (3 * rng.normal(size=shape)).astype(np.float32)
    if extreme:
        x = rng.choice(np.array([-60.0, 0.0, 60.0], np.float32), size=shape)
    if mode == SM:
        t = rng.integers(0, K, size=(N, HW))
        ms = (N, HW)
    else:
        t = (rng.random(shape) > 0.5).astype(np.float32)
        ms = shape
    m = {None: None, "01": (rng.random(ms) > 0.4).astype(np.float32), "zero": np.zeros(ms, np.float32),
         "half": rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=ms)}[mask]
    return x, t, m


@pytest.mark.parametrize("mode,shape,mask,extreme", SEG_CASES)
def test_seg_loss_fwd_bwd(mode, shape, mask, extreme):
    l = L()
    lib = l.lib()
    N, K, HW = shape
    x, t, m = seg_inputs(mode, shape, mask, extreme)
    items = N * HW if mode == SM else N * K * HW
    rows, kk = R.stream_blocks(items), (K if mode == SM else 1)
    for want_rows, shp in SEG_ROWS[mode]:
        assert shp != shape or rows == want_rows
    xg, tg, mg = dev(x), dev(t), (None if m is None else dev(m))
    nb = lib.ustrun_loss_partials_bytes(N, K, HW)
    tag = f"seg_loss mode={mode} {shape} mask={mask}"

    def forward():
        out, part = Out((R.nsums(K),)), Out((nb // 4,))
        l.check(lib.ustrun_seg_loss_fwd(xg.data_ptr(), tg.data_ptr(), ptr(mg), N, K, HW, mode, out.ptr, part.ptr, nb, None))
        return out, part

    out, part = forward()
    got = out.get()
    assert part.guards_ok()
    pg = part.t.cpu().numpy()
    assert (pg[rows * 25:] == SENT).all()                                     # rows of NS = 25 floats, nothing behind the grid's
    ref = R.seg_loss_fwd(x, t, m, mode)
    t64, t32 = R.seg_loss_terms(x, t, m, mode), R.seg_loss_terms(x, t, m, mode, np.float32)
    T = R.trips(items)
    bce = sum_bound(t64[0], t32[0], T)
    bI, bZ, bY = (sum_bound(a, b, T) for a, b in zip(t64[1:], t32[1:]))
    bound = np.zeros(3 + 3 * kk)
    bound[0] = bce / items + U * abs(ref[0])
    bound[2] = bce
    bound[3:3 + kk], bound[3 + kk:3 + 2 * kk], bound[3 + 2 * kk:] = bI, bZ, bY
    I, Z, Y = ref[3:3 + kk], ref[3 + kk:3 + 2 * kk], ref[3 + 2 * kk:3 + 3 * kk]
    bound[1] = sum(dice_bound(I[k], Z[k], Y[k], bI[k], bZ[k], bY[k], R.SMOOTH) for k in range(kk)) / kk + U * abs(ref[1])
    hold(tag + " out", got[:3 + 3 * kk], ref[:3 + 3 * kk], bound)
    assert (got[3 + 3 * kk:] == SENT).all()
    if mask == "zero" and mode == SG:
        assert got[1] == 0.0 and got[0] == 0.0                                # the denominator is SMOOTH alone: dice = 1 - s / s
    out2, part2 = forward()                                                   # fixed order: a repeated call gives the same bits
    assert torch.equal(out.t.view(torch.int32), out2.t.view(torch.int32))
    assert torch.equal(part.t[:rows * 25].view(torch.int32), part2.t[:rows * 25].view(torch.int32))

    sums = np.where(np.isnan(ref), 0.0, ref).astype(np.float32)               # the STORED sums the backward reads
    sg = dev(sums)
    gd = dev(np.array([2.0, -0.5], np.float32))
    combos = GRADS if items <= 8192 else [GRADS[0], GRADS[-1]]
    for gdev, gscale, (cw, dw) in combos:
        d = Out(shape)
        l.check(lib.ustrun_seg_loss_bwd(xg.data_ptr(), tg.data_ptr(), ptr(mg), N, K, HW, mode, sg.data_ptr(), None if gdev is None else
                                        gd.data_ptr(), gscale, cw, dw, d.ptr, None))
        want = R.seg_loss_bwd(x, t, m, mode, sums, gdev, gscale, cw, dw)
        yard = R.seg_loss_bwd(x, t, m, mode, sums, gdev, gscale, cw, dw, np.float32)
        yardstick(f"{tag} dlogits g={gdev} gscale={gscale} w=({cw},{dw})", d.get(), want, yard)


# ---- dice -----------------------------------------------------------------------------------------------------------------------------
# (multi, t_i64, tper, mask: None / "pix" (N, HW) / "full" (N, K, HW)): every combination dice_cfg accepts
DICE_FORMS = [(0, ti, 1, mk) for ti in (1, 0) for mk in (None, "pix")] + [(1, 0, tp, mk) for tp in (0, 1) for mk in (None, "full", "pix")]
DICE_CASES = [(act, form, shp) for act in (0, 1, 2) for form in DICE_FORMS for shp in ((2, 3, 35), (1, 8, 1030))]
DICE_CASES.append((2, (0, 0, 1, None), (2, 1, 524801)))                        # past the cap: 1 049 602 pixels, five trips of 1024 blocks


def dice_inputs(act, form, shape):
    multi, ti, tper, mk = form
    N, K, HW = shape
    rng = np.random.default_rng(act * 101 + multi * 53 + ti * 29 + tper * 13 + HW)
    x = (2 * rng.normal(size=shape)).astype(np.float32)
    if not multi:
        classes = np.array([k for k in range(K) if k != K // 2 or K == 1])      # class K // 2 is absent from the target
        t = rng.choice(classes, size=(N, HW))
        t = t.astype(np.int64) if ti else t.astype(np.float32)
        m = None if mk is None else rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=(N, HW))
    else:
        t = (rng.random((N, HW) if tper else shape) > 0.5).astype(np.float32)
        m = None if mk is None else (rng.random((N, HW) if mk == "pix" else shape) > 0.4).astype(np.float32)
    return x, t, m


@pytest.mark.parametrize("act,form,shape", DICE_CASES)
def test_dice_fwd_bwd(act, form, shape):
    l = L()
    lib = l.lib()
    multi, ti, tper, mk = form
    mper = int(mk != "full")
    N, K, HW = shape
    x, t, m = dice_inputs(act, form, shape)
    xg, tg, mg = dev(x), dev(t), (None if m is None else dev(m))
    nb = lib.ustrun_loss_partials_bytes(N, K, HW)
    T = R.trips(N * HW)
    t64, t32 = R.dice_terms(x, t, m, act, multi, tper, mper), R.dice_terms(x, t, m, act, multi, tper, mper, np.float32)
    bI, bZ, bY = (sum_bound(a, b, T) for a, b in zip(t64, t32))
    wts = [None] if multi or K == 1 else [None, [0.25 + 0.5 * k for k in range(K)]]
    gd = dev(np.array([-1.5, 9.0], np.float32))
    for smooth, w in itertools.product((1e-10, 1e-5), wts):
        sm = R.f32(smooth)
        wp = None if w is None else (C.c_float * K)(*w)
        out, part = Out((1 + 3 * K,)), Out((nb // 4,))
        args = (xg.data_ptr(), tg.data_ptr(), ti, tper, ptr(mg), mper, N, K, HW, act, multi, wp)
        l.check(lib.ustrun_dice_smooth_fwd(*args, smooth, out.ptr, part.ptr, nb, None))
        ref = R.dice_fwd(x, t, m, act, multi, tper, mper, w, smooth)
        I, Z, Y = ref[1:1 + K], ref[1 + K:1 + 2 * K], ref[1 + 2 * K:]
        bound = np.zeros(1 + 3 * K)
        if multi:
            bound[1], bound[1 + K], bound[1 + 2 * K] = bI.sum(), bZ.sum(), bY.sum()
            bound[0] = dice_bound(I[0], Z[0], Y[0], bI.sum(), bZ.sum(), bY.sum(), sm) + U * abs(ref[0])
        else:
            bound[1:1 + K], bound[1 + K:1 + 2 * K], bound[1 + 2 * K:] = bI, bZ, bY
            ww = np.ones(K) if w is None else np.asarray(w)
            bound[0] = sum(ww[k] * dice_bound(I[k], Z[k], Y[k], bI[k], bZ[k], bY[k], sm) for k in range(K)) / K + U * abs(ref[0])
        tag = f"dice act={act} form={form} {shape} smooth={smooth} w={w is not None}"
        got = out.get()
        hold(tag + " out", got, ref, bound)
        assert part.guards_ok()
        if not multi and K > 1:
            assert got[1 + K // 2] == 0.0 and got[1 + 2 * K + K // 2] == 0.0    # the absent class: I = Y = 0 exactly
        sums = ref.astype(np.float32)
        sg = dev(sums)
        for gdev, gscale in ((None, 1.0), ((-1.5, 9.0), 1024.0)):
            d = Out(shape)
            l.check(lib.ustrun_dice_smooth_bwd(*args, smooth, sg.data_ptr(), None if gdev is None else gd.data_ptr(), gscale, d.ptr, None))
            want = R.dice_bwd(x, t, m, act, multi, tper, mper, sums, w, smooth, gdev, gscale)
            yard = R.dice_bwd(x, t, m, act, multi, tper, mper, sums, w, smooth, gdev, gscale, np.float32)
            yardstick(f"{tag} dlogits g={gdev}", d.get(), want, yard)
        if smooth == 1e-10:                                                     # the dice_* pair IS the smooth pair at SMOOTH
            o2, p2, d2 = Out((1 + 3 * K,)), Out((nb // 4,)), Out(shape)
            l.check(lib.ustrun_dice_fwd(*args, o2.ptr, p2.ptr, nb, None))
            assert o2.guards_ok() and p2.guards_ok() and torch.equal(o2.t.view(torch.int32), out.t.view(torch.int32))
            l.check(lib.ustrun_dice_bwd(*args, sg.data_ptr(), gd.data_ptr(), 1024.0, d2.ptr, None))
            assert d2.guards_ok() and torch.equal(d2.t.view(torch.int32), d.t.view(torch.int32))


# ---- pseudo_label ---------------------------------------------------------------------------------------------------------------------
PSEUDO_CASES = [(mode, shp, th) for mode in (SM, SG) for shp in R.PSEUDO_SHAPES for th in R.PSEUDO_THRESHOLDS]
PSEUDO_CASES += [(SM, (1, 2, 1048583), 0.95), (SG, (1, 2, 524803), 0.95)]     # past the cap


@pytest.mark.parametrize("mode,shape,th", PSEUDO_CASES)
def test_pseudo_label(mode, shape, th):
    l = L()
    N, K, HW = shape
    x, planted = R.pseudo_label_case(N, K, HW)
    lab = Out((N, HW), torch.int64) if mode == SM else Out(shape)
    msk = Out((N, HW)) if mode == SM else Out(shape)
    xg = dev(x)
    l.check(l.lib().ustrun_pseudo_label(xg.data_ptr(), N, K, HW, th, mode, lab.ptr, msk.ptr, None))
    assert lab.guards_ok() and msk.guards_ok()
    gl, gm = lab.t.cpu().numpy(), msk.t.cpu().numpy().astype(np.float64)
    lab_ok, mask_ok, lz, mz = R.pseudo_label_accept(x, th, mode, gl if mode == SM else gl.astype(np.float64), gm)
    rl, rm, p = R.pseudo_label(x, th, mode)
    pl = planted if mode == SM else np.broadcast_to(planted[:, None, :], shape)
    zone = (lz | mz) & ~pl
    print(f"pseudo_label mode={mode} {shape} th={th}: {int((gl != rl).sum())} labels and {int((gm != rm).sum())} mask elements differ "
          f"from float64, {int(zone.sum())} of {zone.size} in the zone")
    assert zone.sum() <= R.PSEUDO_ZONE_CAP * zone.size
    assert lab_ok.all(), f"{int((~lab_ok).sum())} labels neither equal nor within the error of the boundary"
    assert mask_ok.all(), f"{int((~mask_ok).sum())} mask elements neither equal nor within the error of the boundary"
    if HW >= 12:                                                                # the planted pixels are exact in float32 too
        if mode == SM:
            assert (gl[0, :8] == 0).all()                                       # ties: the first index
            assert (gl[0, 8:12] == 0).all() and (gm[0, 8:12] == (1.0 if (1.0 / ((K + 1) // 2)) > R.f32(th) else 0.0)).all()
        else:
            assert (gl[0, :, :4] == 1).all()                                    # p = 0.5 exactly: >= 0.5
            if th == 0.5:
                assert (gm[0, :, :4] == 2).all()                                # p >= th and p <= 1 - th
            want = (np.arange(K) % 2 == 0).astype(np.float64)[:, None]
            assert (gl[0, :, 8:12] == want).all()


# ---- mix_targets ----------------------------------------------------------------------------------------------------------------------
MIX_CASES = [(mode, shp) for mode in (SM, SG) for shp in ((1, 1, 1), (3, 2, 577), (2, 8, 1030))] + [(SM, (1, 1, 1048583)), (SG, (1, 2, 524801))]      # past the cap


@pytest.mark.parametrize("mode,shape", MIX_CASES)
def test_mix_targets(mode, shape):
    l = L()
    N, K, HW = shape
    rng = np.random.default_rng(N * 31 + K * 7 + HW + mode)
    box = (rng.random((N, HW)) > 0.5).astype(np.float32)
    box[0] = 0.0 if HW > 1 else 1.0                                             # an all-0 sample ...
    if N > 1:
        box[1] = 1.0                                                            # ... and an all-1 sample
    ls = (N, HW) if mode == SM else shape
    lab = (lambda: rng.integers(0, 4, size=ls)) if mode == SM else (lambda: (rng.random(ls) > 0.5).astype(np.float32))
    msk = lambda: (rng.random(ls) > 0.3).astype(np.float32) * rng.choice(np.array([1.0, 0.25], np.float32), size=ls)
    ins = [lab(), msk(), lab(), msk(), lab(), msk(), lab(), msk() + 2]          # pl, mask, plwul, mwul, plwlu, mwlu, cutl, cutm (never = mask)
    ltd = torch.int64 if mode == SM else torch.float32
    outs = [Out(ls, ltd), Out(ls), Out(ls, ltd), Out(ls), Out(ls, ltd), Out(ls)]
    ing, bg = [dev(a) for a in ins], dev(box)
    l.check(l.lib().ustrun_mix_targets(mode, N, K, HW, bg.data_ptr(), *[a.data_ptr() for a in ing], *[o.ptr for o in outs], None))
    ref = R.mix_targets(mode, box, *ins)
    for o, r, td in zip(outs, ref, (ltd, torch.float32) * 3):
        bits(o, r, td)


@pytest.mark.parametrize("C_,frac", [(1, False), (3, False), (1, True), (3, True)])
def test_box_mix(C_, frac):
    l = L()
    N, HW = 2, 1029
    rng = np.random.default_rng(C_ + 10 * frac)
    a, b = rng.normal(size=(N, C_, HW)).astype(np.float32), rng.normal(size=(N, C_, HW)).astype(np.float32)
    box = (rng.integers(0, 9, size=(N, HW)) / 8.0 if frac else rng.integers(0, 2, size=(N, HW))).astype(np.float32)
    o = Out((N, C_, HW))
    ag, bg, xg = dev(a), dev(b), dev(box)
    l.check(l.lib().ustrun_box_mix(ag.data_ptr(), bg.data_ptr(), xg.data_ptr(), N, C_, HW, o.ptr, None))
    ref, mag = R.box_mix(a, b, box)
    if frac:
        hold(f"box_mix C={C_} eighths", o.get(), ref, 3 * U * mag * (1 + 2.0 ** -20))
    else:
        bits(o, ref, torch.float32)


# ---- assemble -------------------------------------------------------------------------------------------------------------------------
def asm_table(l, rows):
    tab = (l.AsmRow * len(rows))()
    for i, (a, b, bx) in enumerate(rows):
        tab[i].a, tab[i].b, tab[i].box = a, b or None, bx or None
    return tab


@pytest.mark.parametrize("nrows,C_,HW", [(1, 1, 4), (128, 1, 4), (128, 3, 5564)])
def test_assemble(nrows, C_, HW):
    """rows of 16 bytes, and 128 rows of 16 x (4096 + 77) bytes: 16 blocks per row under the 2048 / nrows cap, more than one trip"""
    l = L()
    lib = l.lib()
    rb = C_ * HW * 4
    assert rb % 16 == 0 and (rb == 16 or (rb == 16 * (4096 + 77) and rb // 16 > 256 * (2048 // nrows)))
    rng = np.random.default_rng(nrows + HW)
    a, b = dev(rng.normal(size=(nrows, C_, HW)).astype(np.float32)), dev(rng.normal(size=(nrows, C_, HW)).astype(np.float32))
    box = dev((rng.random((nrows, HW)) > 0.5).astype(np.float32))
    pick = rng.integers(0, nrows, size=nrows)
    rows = [(a[i].data_ptr(), b[j].data_ptr(), box[i].data_ptr()) for i, j in enumerate(pick)]
    o = Out((nrows, C_, HW))
    l.check(lib.ustrun_assemble(asm_table(l, rows), nrows, rb, HW, o.ptr, None))
    m = Out((nrows, C_, HW))                                                  # the composite IS box_mix on the same operands
    bp = b[torch.from_numpy(pick).cuda()].contiguous()
    l.check(lib.ustrun_box_mix(a.data_ptr(), bp.data_ptr(), box.data_ptr(), nrows, C_, HW, m.ptr, None))
    assert o.guards_ok() and m.guards_ok() and torch.equal(o.t.view(torch.int32), m.t.view(torch.int32))
    ref, _ = R.box_mix(a.cpu().numpy(), b.cpu().numpy()[pick], box.cpu().numpy())
    bits(o, ref, torch.float32)
    lab = dev(rng.integers(-5, 2 ** 40, size=(nrows, rb // 8)))                 # int64 copies, one row aliased many times
    sel = [0] * (nrows // 2) + list(rng.integers(0, nrows, size=nrows - nrows // 2))
    oc = Out((nrows, rb // 8), torch.int64)
    l.check(lib.ustrun_assemble(asm_table(l, [(lab[i].data_ptr(), 0, 0) for i in sel]), nrows, rb, 0, oc.ptr, None))
    assert oc.guards_ok() and torch.equal(oc.t, lab[torch.tensor(sel).cuda()])


# ---- decode_labels, region_bbox, rect_masks, dice_counts ------------------------------------------------------------------------------
LABEL_VALUES = np.array([0.0, -0.0, 1.0, 127.5, 128.0, 129.0, 255.0], np.float32)


@pytest.mark.parametrize("kind,N,HW", [(0, 2, 1031), (1, 2, 1031), (2, 2, 1031), (3, 2, 1031), (3, 1, 1048583)])
def test_decode_labels(kind, N, HW):
    l = L()
    rng = np.random.default_rng(kind + HW)
    y = rng.choice(LABEL_VALUES, size=(N, HW, 3) if kind == 3 else (N, HW), p=[.15, .1, .1, .1, .15, .1, .3])
    y.reshape(-1)[:7] = LABEL_VALUES
    o = Out((N, 2, HW)) if kind == 0 else Out((N, HW), torch.int64)
    yg = dev(y)
    l.check(l.lib().ustrun_decode_labels(yg.data_ptr(), kind, N, HW, o.ptr, None))
    bits(o, R.decode_labels(y, kind), torch.float32 if kind == 0 else torch.int64)


def bbox_call(l, planes, H, W):
    arr = (C.c_void_p * len(planes))(*[p.data_ptr() for p in planes])
    b = sum(int(p.dtype == torch.int64) << k for k, p in enumerate(planes))
    o = Out((R.BBOX_BLOCKS, 4), torch.int32)
    l.check(l.lib().ustrun_region_bbox(arr, len(planes), b, H, W, o.ptr, None))
    return o


@pytest.mark.parametrize("H,W", [(37, 53), (1, 300), (300, 1), (1024, 1024)])
def test_region_bbox(H, W):
    l = L()
    rng = np.random.default_rng(H + W)
    HW = H * W
    zero = np.zeros(HW, np.float32)
    for e in sorted({0, W - 1, HW - W, HW - 1}):                                 # a single pixel: each corner, the last element
        z = zero.copy()
        z[e] = -2.5
        o = bbox_call(l, [dev(z)], H, W)
        ref = R.region_bbox([z], H, W)
        bits(o, ref, torch.int32)
        assert R.fold_bbox(ref) == (e // W, e // W + 1, e % W, e % W + 1)
    o = bbox_call(l, [dev(zero), dev(zero.astype(np.int64))], H, W)              # empty: every block reports {H, -1, W, -1}
    bits(o, np.tile(np.array([H, -1, W, -1]), (64, 1)), torch.int32)
    assert R.fold_bbox(o.t.cpu().numpy()) is None
    mixes = [m for n in range(1, 5) for m in itertools.product((0, 1), repeat=n)] if HW < 4096 else [(0, 1)]
    for mix in mixes:                                                           # 1 to 4 planes, every int64 / f32 mix
        planes = []
        for i64 in mix:
            z = np.zeros(HW, np.int64 if i64 else np.float32)
            idx = rng.integers(0, HW, size=3)
            z[idx] = rng.integers(1, 4, size=3)
            planes.append(z)
        o = bbox_call(l, [dev(z) for z in planes], H, W)
        bits(o, R.region_bbox(planes, H, W), torch.int32)


def test_rect_masks():
    l = L()
    N, H, W = 64, 37, 53
    rng = np.random.default_rng(5)
    r = np.stack([rng.integers(-10, H + 10, N), rng.integers(-10, H + 10, N), rng.integers(-10, W + 10, N), rng.integers(-10, W + 10, N)], 1)
    r[0], r[1], r[2], r[3] = (5, 5, 0, W), (9, 3, 0, W), (-7, -1, 0, W), (0, H, W, W + 9)     # empty; inverted; above; right of the image
    r[4], r[5] = (0, H, 0, W), (-3, H + 3, -3, W + 3)                            # the whole image, exactly and generously
    r = np.ascontiguousarray(r, dtype=np.int32)
    o = Out((N, H, W))
    l.check(l.lib().ustrun_rect_masks(r.ctypes.data, N, H, W, o.ptr, None))
    ref = R.rect_masks(r, H, W)
    assert ref[:4].sum() == 0 and ref[4].all() and ref[5].all()
    bits(o, ref, torch.float32)


@pytest.mark.parametrize("N,K,HW,split", [(1, 1, 4096, 2), (2, 3, 70001, 32), (3, 2, 100, 1)])
def test_dice_counts(N, K, HW, split):
    l = L()
    assert R.dice_split(N, K, HW) == split
    rng = np.random.default_rng(HW)
    for by_class, pi, gi in itertools.product((0, 1), (0, 1), (0, 1)):
        if by_class:
            p, g = rng.integers(0, K + 2, size=(N, HW)), rng.integers(0, K + 2, size=(N, HW))
        else:
            p, g = rng.integers(0, 3, size=(N, K, HW)) * (rng.random((N, K, HW)) > 0.4), rng.integers(-1, 2, size=(N, K, HW))
        p, g = p.astype(np.int64 if pi else np.float32), g.astype(np.int64 if gi else np.float32)
        pg, gg = dev(p), dev(g)
        ref = R.dice_counts(p, g, K, by_class)
        first = None
        for garbage in (123456789, -77):                                        # counts prefilled with garbage; a repeated call
            o = Out((N, K, 3), torch.int32, init=np.full((N, K, 3), garbage))
            l.check(l.lib().ustrun_dice_counts(pg.data_ptr(), gg.data_ptr(), pi, gi, N, K, HW, by_class, o.ptr, None))
            bits(o, ref, torch.int32)
            first = o if first is None else first
            assert torch.equal(first.t, o.t)


# ---- sgd_ema, the loss scale ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 40961, 4198403])
def test_sgd_ema(n):
    """4 198 403 floats: n / 4 + 1 work items are past stream_blocks' cap (1 048 576) and three floats are left to the scalar tail"""
    l = L()
    lib = l.lib()
    rng = np.random.default_rng(n)
    p0, g0, v0, t0 = (rng.normal(size=n).astype(np.float32) for _ in range(4))
    lr, mu, wd, alpha = 0.03, 0.9, 1e-4, 0.99
    gg = dev(g0)
    state = dev(np.array([1024.0, 1024.0, 1.0, 0.0, 0.0, 3.0, 0.0, 0.0], np.float32))
    skipst = dev(np.array([1024.0, 1024.0, 1.0, 1.0, 0.0, 3.0, 0.0, 0.0], np.float32))
    combos = list(itertools.product((True, False), (0, 1), (1.0, 0.5), ("plain", "scaled", "skip")))
    if n > 100000:
        combos = [(True, 0, 0.5, "plain"), (False, 1, 1.0, "scaled"), (True, 0, 1.0, "skip")]
    for has_t, first, gsc, kind in combos:
        p, v, t = Out((n,), init=p0), Out((n,), init=v0), (Out((n,), init=t0) if has_t else None)
        tp = t.ptr if has_t else None
        if kind == "plain":
            l.check(lib.ustrun_sgd_ema(p.ptr, gg.data_ptr(), v.ptr, tp, n, lr, mu, wd, first, alpha, gsc, None))
        else:
            l.check(lib.ustrun_sgd_ema_scaled(p.ptr, gg.data_ptr(), v.ptr, tp, n, lr, mu, wd, first, alpha, gsc,
                                              (skipst if kind == "skip" else state).data_ptr(), None))
        (rp, rv, rt), (ep, ev, et) = R.sgd_ema(p0, g0, v0, t0 if has_t else None, lr, mu, wd, first, alpha, gsc,
                                               scale=None if kind == "plain" else 1024.0, skip=kind == "skip")
        tag = f"sgd_ema n={n} t={has_t} first={first} gsc={gsc} {kind}"
        if kind == "skip":                                                      # found_inf: p and v keep their bits, t moves
            bits(p, p0, torch.float32)
            bits(v, v0, torch.float32)
        else:
            hold(tag + " p", p.get(), rp, ep)
            hold(tag + " v", v.get(), rv, ev)
        if has_t:
            hold(tag + " t", t.get(), rt, et)
            assert not np.array_equal(t.get(), t0.astype(np.float64))


def test_amp_check():
    l = L()
    lib = l.lib()
    n = 4 * 262144 + 1031                                                       # n & 3 == 3; more float4s than one grid's threads
    rng = np.random.default_rng(11)
    clean = rng.normal(size=n).astype(np.float32)
    clean[1], clean[2], clean[n - 2] = np.finfo(np.float32).max, 1e-45, -np.finfo(np.float32).max      # FLT_MAX and a subnormal: finite
    st0 = np.array([512.0, 512.0, 2.0, 0.0, 1.0, 7.0, -3.5, 42.0], np.float32)
    for where, val in [(None, 0.0), (0, np.inf), (n - 1, np.nan), (n - 1, -np.inf), (n - 3, np.inf), (4 * 262144 + 5, np.nan), (4 * 262144 - 1, -np.inf)]:
        g = clean.copy()
        if where is not None:
            g[where] = val
        for preset in (0.0, 1.0):                                               # a set flag stays set
            s = st0.copy()
            s[3] = preset
            o = Out((8,), init=s)
            gg = dev(g)
            l.check(lib.ustrun_amp_check(gg.data_ptr(), n, o.ptr, None))
            s[3] = max(preset, R.amp_check(g))
            assert s[3] == (1.0 if where is not None or preset else 0.0)
            bits(o, s, torch.float32)                                           # the other seven floats keep their bits


@pytest.mark.parametrize("interval", [1, 3])
def test_amp_update(interval):
    l = L()
    s = np.array([1024.0, 1024.0, 0.0, 0.0, 0.0, 0.0, -3.5, 42.0], np.float32)
    o = Out((8,), init=s)
    for step, found in enumerate([0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0]):
        o.t[3] = float(found)
        s[3] = found
        l.check(l.lib().ustrun_amp_update(o.ptr, 2.0, 0.5, interval, None))
        s = R.amp_update(s, 2.0, 0.5, interval)
        bits(o, s, torch.float32)
    assert s[5] == 11 and s[4] == 3 and s[3] == 0                                # steps seen, steps skipped
    o = Out((8,), init=s)                                                       # factors that are no powers of two: float arithmetic
    l.check(l.lib().ustrun_amp_update(o.ptr, 1.7, 0.3, 1, None))
    bits(o, R.amp_update(s, 1.7, 0.3, 1), torch.float32)


# ---- freq_mix -------------------------------------------------------------------------------------------------------------------------
FREQ_CASES = [(1, 8, 8, 0), (3, 16, 12, 1), (1, 5, 7, 1), (1, 33, 47, 2), (2, 64, 40, 3), (1, 100, 100, 4), (1, 50, 131, 5)]
RATIOS = [0.0, 0.37, 1.0]


def freq_call(l, src, trg, ratios, b):
    n, C_, H, W = src.shape
    wb = l.lib().ustrun_freq_mix_work_bytes(n, C_, b)
    assert wb == n * C_ * 2 * 8 * (2 * b + 1) ** 2 * 8
    o, work = Out(src.shape), Out((wb // 4,))
    sg, tg, rg = dev(src), dev(trg), dev(np.asarray(ratios, np.float32))
    l.check(l.lib().ustrun_freq_mix(sg.data_ptr(), tg.data_ptr(), rg.data_ptr(), n, C_, H, W, b, o.ptr, work.ptr, wb, None))
    assert work.guards_ok()
    return o.get()


@pytest.mark.parametrize("C_,H,W,b", FREQ_CASES)
@pytest.mark.parametrize("kind", ["random", "constant", "binary"])
def test_freq_mix(C_, H, W, b, kind):
    l = L()
    rng = np.random.default_rng(C_ + H + W + b)
    img = lambda: (rng.integers(0, 256, size=(3, C_, H, W)).astype(np.float32) / np.float32(127.5) - np.float32(1))
    src, trg, ratios = img(), img(), RATIOS
    if kind == "constant":                                                      # S = 0: every amplitude of src is zero, phase (1, 0)
        src = np.full_like(src, -1.0)
    if kind == "binary":                                                        # pure 0 / 255 with ratio 1: the clip acts
        src, ratios = (rng.integers(0, 2, size=src.shape) * 2 - 1).astype(np.float32), [1.0, 1.0, 1.0]
    got = freq_call(l, src, trg, ratios, b)
    want = R.freq_mix(src, trg, ratios, b)
    yard = R.freq_mix_two_stage(src, trg, ratios, b)
    if kind == "binary":
        assert ((want == -1.0) | (want == 1.0)).any()
    if kind == "constant":
        assert np.abs(want[2] + 1.0).max() > 1e-3                               # the mix is not a no-op there
    yardstick(f"freq_mix {(C_, H, W, b)} {kind}", got, want, yard, cap=2e-5)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_before_any_launch():
    """Every USTRUN_CHECK of these entries: nonzero, ustrun_last_error() names the entry, outputs and guards keep the sentinel."""
    l = L()
    lib = l.lib()
    f = torch.zeros(4096, device="cuda")
    i8 = torch.zeros(4096, dtype=torch.int64, device="cuda")
    fp, ip = f.data_ptr(), i8.data_ptr()
    outs = [Out((4096,)) for _ in range(6)]
    o = [x.ptr for x in outs]
    nb = lib.ustrun_loss_partials_bytes(1, 2, 16)
    part = Out((nb // 4,))
    st = Out((8,))

    def refused(rc, entry):
        msg = lib.ustrun_last_error()
        assert rc != 0, entry
        assert msg.startswith(entry.encode() + b":"), (entry, msg)

    big = (1 << 16, 1 << 16)                                                    # N x HW = 2^32, by arguments only
    for K, N, HW in [(0, 1, 16), (9, 1, 16), (2, 0, 16), (2, 1, 0), (2,) + big]:
        refused(lib.ustrun_seg_loss_fwd(fp, ip, None, N, K, HW, SM, o[0], part.ptr, nb, None), "seg_loss_fwd")
        refused(lib.ustrun_seg_loss_bwd(fp, ip, None, N, K, HW, SM, fp, None, 1.0, 1.0, 1.0, o[0], None), "seg_loss_bwd")
        refused(lib.ustrun_pseudo_label(fp, N, K, HW, 0.95, SM, o[0], o[1], None), "pseudo_label")
        refused(lib.ustrun_dice_smooth_fwd(fp, ip, 1, 1, None, 1, N, K, HW, 1, 0, None, 1e-5, o[0], part.ptr, nb, None), "dice_fwd")
        refused(lib.ustrun_dice_smooth_bwd(fp, ip, 1, 1, None, 1, N, K, HW, 1, 0, None, 1e-5, fp, None, 1.0, o[0], None), "dice_bwd")
        refused(lib.ustrun_dice_fwd(fp, ip, 1, 1, None, 1, N, K, HW, 1, 0, None, o[0], part.ptr, nb, None), "dice_fwd")
        refused(lib.ustrun_dice_bwd(fp, ip, 1, 1, None, 1, N, K, HW, 1, 0, None, fp, None, 1.0, o[0], None), "dice_bwd")
        if N * HW < 2 ** 32:
            refused(lib.ustrun_mix_targets(SG, N, K, HW, fp, *([fp] * 8), *o, None), "mix_targets")
    for mode in (-1, 2):
        refused(lib.ustrun_seg_loss_fwd(fp, ip, None, 1, 2, 16, mode, o[0], part.ptr, nb, None), "seg_loss_fwd")
        refused(lib.ustrun_seg_loss_bwd(fp, ip, None, 1, 2, 16, mode, fp, None, 1.0, 1.0, 1.0, o[0], None), "seg_loss_bwd")
        refused(lib.ustrun_pseudo_label(fp, 1, 2, 16, 0.95, mode, o[0], o[1], None), "pseudo_label")
        refused(lib.ustrun_mix_targets(mode, 1, 2, 16, fp, *([fp] * 8), *o, None), "mix_targets")
    # null pointers; partials one byte short
    refused(lib.ustrun_seg_loss_fwd(None, ip, None, 1, 2, 16, SM, o[0], part.ptr, nb, None), "seg_loss_fwd")
    refused(lib.ustrun_seg_loss_fwd(fp, ip, None, 1, 2, 16, SM, o[0], part.ptr, nb - 1, None), "seg_loss_fwd")
    refused(lib.ustrun_seg_loss_bwd(fp, ip, None, 1, 2, 16, SM, None, None, 1.0, 1.0, 1.0, o[0], None), "seg_loss_bwd")
    refused(lib.ustrun_dice_smooth_fwd(fp, ip, 1, 1, None, 1, 1, 2, 16, 1, 0, None, 1e-5, o[0], part.ptr, nb - 1, None), "dice_fwd")
    refused(lib.ustrun_dice_smooth_bwd(fp, ip, 1, 1, None, 1, 1, 2, 16, 1, 0, None, 1e-5, None, None, 1.0, o[0], None), "dice_bwd")
    refused(lib.ustrun_pseudo_label(None, 1, 2, 16, 0.95, SM, o[0], o[1], None), "pseudo_label")
    refused(lib.ustrun_mix_targets(SG, 1, 2, 16, None, *([fp] * 8), *o, None), "mix_targets")
    # the dice_cfg rules: smooth < 0, activation 3 / -1, a per-class form without a class-index target, multi with an int64 target
    for kw in [dict(smooth=-1.0), dict(act=3), dict(act=-1), dict(multi=0, tper=0), dict(multi=1, ti=1)]:
        a = dict(ti=0, tper=1, act=1, multi=0, smooth=1e-5)
        a.update(kw)
        refused(lib.ustrun_dice_smooth_fwd(fp, ip, a["ti"], a["tper"], None, 1, 1, 2, 16, a["act"], a["multi"], None, a["smooth"], o[0], part.ptr,
                                           nb, None), "dice_fwd")
        refused(lib.ustrun_dice_smooth_bwd(fp, ip, a["ti"], a["tper"], None, 1, 1, 2, 16, a["act"], a["multi"], None, a["smooth"], fp, None, 1.0,
                                           o[0], None), "dice_bwd")
    # box_mix, decode_labels, region_bbox, rect_masks, dice_counts
    refused(lib.ustrun_box_mix(fp, fp, fp, 0, 1, 16, o[0], None), "box_mix")
    refused(lib.ustrun_box_mix(fp, fp, None, 1, 1, 16, o[0], None), "box_mix")
    refused(lib.ustrun_decode_labels(fp, 4, 1, 16, o[0], None), "decode_labels")
    refused(lib.ustrun_decode_labels(fp, -1, 1, 16, o[0], None), "decode_labels")
    refused(lib.ustrun_decode_labels(fp, 0, 0, 16, o[0], None), "decode_labels")
    pl = (C.c_void_p * 4)(fp, fp, fp, fp)
    refused(lib.ustrun_region_bbox(pl, 0, 0, 8, 8, o[0], None), "region_bbox")
    refused(lib.ustrun_region_bbox(pl, 5, 0, 8, 8, o[0], None), "region_bbox")
    refused(lib.ustrun_region_bbox(pl, 1, 0, 1 << 15, 1 << 15, o[0], None), "region_bbox")
    refused(lib.ustrun_region_bbox((C.c_void_p * 2)(fp, None), 2, 0, 8, 8, o[0], None), "region_bbox")
    rc = np.zeros((65, 4), np.int32)
    refused(lib.ustrun_rect_masks(rc.ctypes.data, 0, 8, 8, o[0], None), "rect_masks")
    refused(lib.ustrun_rect_masks(rc.ctypes.data, 65, 8, 8, o[0], None), "rect_masks")
    refused(lib.ustrun_rect_masks(rc.ctypes.data, 1, 0, 8, o[0], None), "rect_masks")
    refused(lib.ustrun_dice_counts(fp, fp, 0, 0, 1, 0, 16, 0, o[0], None), "dice_counts")
    refused(lib.ustrun_dice_counts(fp, None, 0, 0, 1, 1, 16, 0, o[0], None), "dice_counts")
    # assemble: 0 / 129 rows, row_bytes % 16, an unaligned row, a composite whose HW does not divide the row
    tab = asm_table(l, [(fp, 0, 0)] * 129)
    refused(lib.ustrun_assemble(tab, 0, 64, 0, o[0], None), "assemble")
    refused(lib.ustrun_assemble(tab, 129, 64, 0, o[0], None), "assemble")
    refused(lib.ustrun_assemble(tab, 1, 40, 0, o[0], None), "assemble")
    refused(lib.ustrun_assemble(tab, 1, 0, 0, o[0], None), "assemble")
    refused(lib.ustrun_assemble(tab, 1, 64, 0, o[0] + 4, None), "assemble")
    refused(lib.ustrun_assemble(asm_table(l, [(fp + 4, 0, 0)]), 1, 64, 0, o[0], None), "assemble")
    refused(lib.ustrun_assemble(asm_table(l, [(fp, fp, fp)]), 1, 64, 6, o[0], None), "assemble")
    refused(lib.ustrun_assemble(asm_table(l, [(fp, fp, 0)]), 1, 64, 4, o[0], None), "assemble")
    # sgd_ema: a view one float in, for each pointer; n = 0
    for k in range(4):
        a = [o[0], fp, o[1], o[2]]
        a[k] += 4
        refused(lib.ustrun_sgd_ema(*a, 64, 0.1, 0.9, 0.0, 0, 0.99, 1.0, None), "sgd_ema")
        refused(lib.ustrun_sgd_ema_scaled(*a, 64, 0.1, 0.9, 0.0, 0, 0.99, 1.0, fp, None), "sgd_ema_scaled")
    refused(lib.ustrun_sgd_ema(o[0], fp, o[1], o[2], 0, 0.1, 0.9, 0.0, 0, 0.99, 1.0, None), "sgd_ema")
    refused(lib.ustrun_sgd_ema_scaled(o[0], fp, o[1], o[2], 64, 0.1, 0.9, 0.0, 0, 0.99, 1.0, None, None), "sgd_ema_scaled")
    refused(lib.ustrun_amp_check(fp + 4, 64, st.ptr, None), "amp_check")
    refused(lib.ustrun_amp_check(fp, 0, st.ptr, None), "amp_check")
    for gr, bk, iv in [(0.5, 0.5, 1), (2.0, 0.0, 1), (2.0, 1.5, 1), (2.0, 0.5, 0)]:
        refused(lib.ustrun_amp_update(st.ptr, gr, bk, iv, None), "amp_update")
    refused(lib.ustrun_amp_update(None, 2.0, 0.5, 1, None), "amp_update")
    # freq_mix: b = 6 and -1, a work buffer one byte short, an extent whose twiddle tables exceed the LDS
    wb = lib.ustrun_freq_mix_work_bytes(1, 1, 1)
    refused(lib.ustrun_freq_mix(fp, fp, fp, 1, 1, 8, 8, 6, o[0], part.ptr, nb, None), "freq_mix")
    refused(lib.ustrun_freq_mix(fp, fp, fp, 1, 1, 8, 8, -1, o[0], part.ptr, nb, None), "freq_mix")
    refused(lib.ustrun_freq_mix(fp, fp, fp, 1, 1, 8, 8, 1, o[0], part.ptr, wb - 1, None), "freq_mix")
    refused(lib.ustrun_freq_mix(fp, fp, fp, 0, 1, 8, 8, 1, o[0], part.ptr, wb, None), "freq_mix")
    refused(lib.ustrun_freq_mix(fp, fp, fp, 1, 1, 4096, 4096, 5, o[0], part.ptr, nb, None), "freq_mix")
    torch.cuda.synchronize()
    assert all(sentinel(x) for x in outs) and sentinel(part) and sentinel(st)
    assert not bool(f.any()) and not bool(i8.any())
