"""The BatchNorm + ReLU (+ MaxPool routing) backward in train mode (csrc/bn.hip, kernels in csrc/bn_bwd.h) and the 1x1 head (csrc/head.hip),
one C-ABI call at a time against the float64 references of tests/bn_head_bwd_ref.py (pinned to torch's float64 autograd on the CPU by
tests/test_bn_head_bwd_ref_host.py): ustrun_bn_bwd_reduce, ustrun_bn_bwd_apply, ustrun_bn_bwd_finalize_stat on synthetic row tables,
ustrun_bn_bwd_apply_head, ustrun_head_fwd and ustrun_head_bwd, in f32, f32x3, bf16 and f16.  Every output lies between two 4096-element
sentinel zones that must come back untouched and starts out as the sentinel; y, da, dp and dlogits lie between NaN zones, so a load past
either end poisons a sum or an output.  The harness (Out, stored, half_ulp, hold, DT, table) is tests/test_gpu_bn_forward_ops.py's.

INPUT CONDITIONS (asserted on the CPU before every launch, bn_head_bwd_ref.bn_case).  The ReLU mask [a > 0] and the window arg-max are not
Lipschitz: an f32 pre-activation a = y s + b carries an error of at most 2^-22 (|y s| + |b|) (one product and one sum rounded, 2^-24 each
of at most |y s| + |b|, twice over as in the forward file), so a float64 a within that of zero, or two window values closer than their two
errors, may go the other way on the device.  The generators move such y by a few units of the storage type's spacing until, in units of
|y s| + |b|, the smallest nonzero |a| and the smallest gap between a window's maximum and a DIFFERENT value of it are both >= 4 x 2^-22.
Then mask and arg-max are the reference's on the device: NO element is excluded from any comparison.  Planted ties are exact (the same
stored y in the same channel gives the same f32 activation, whatever the compiler contracts) and must go to the first maximum.

BOUNDS on |got - ref| (ref: float64 on the SAME stored inputs), derived, not tuned; u = 2^-24, and U = 2^-22 = 4u carries the forward
file's factor-4 slack where a chain of roundings is bounded by its length.
  reduce sums    A lane adds T = (windows per lane) x (pixels per window) elements in f32, block_fold adds the block's PL = 256 / G pixel
                 lanes in f32, the block rows are then summed in float64.  T + PL roundings, each at most u x (the running sum <= sum|dz|)
                 (the first addition of a chain is exact; the two spared cover dz = da + routed dp, one f32 rounding):
                     d1 = (T + PL) U sum|dz|,   d2 = (T + PL + 1) U sum|dz y|   (+ 1: the product dz y)
                 dbeta: d1 + u |dbeta|;  dgamma = rstd (s2 - mean s1): |rstd| (d2 + |mean| d1) + u |dgamma|   (the f32 result)
                 accumulate: + u |old + new|, one more f32 rounding.
  coef           c0 = gamma rstd: 2u |c0|.  c1 = -c0 (dgamma / count) rstd: |c0 rstd| d(dgamma) / count + 2u |c1|, d(dgamma) the
                 propagated part above.  c2 = -c0 dbeta / count - c1 mean cancels, so its bound is absolute:
                 |c0| d1 / count + |mean| d(c1) + 2u (|c0 dbeta / count| + |c1 mean|).
  apply          dy = c0 dz + c1 y + c2 on a table of the test's own: U (|c0 dz| + |c1 y| + |c2|) (three roundings of at most that, and
                 dz's own) + HALF_ULP of the storage type at the reference (exact half spacing, see the forward file).
  finalize_stat  the table's f32 entries ARE the inputs and the device sums them in float64, as the reference does: no sum term.  dgamma /
                 dbeta: each pass's term is rounded to f32 and added in f32, one after the other: (passes [+ 1 with accumulate]) u
                 sum_pass |term| + u |result|.  c0, c1: 2u relative; c2: 2u (|c0 dbeta / count| + |c1 mean|).
  head logits    (C + 2) u sum_c |a w| (C products and sums in whatever order, the shuffles included, + bias) + sum_c |w| U (|y s| + |b|)
                 (the activation's own f32 error, 1-Lipschitz through max(., 0)) + u |logit|.
  head da        (K + 1) u sum_k |dl w| + HALF_ULP.
  head dw        a lane adds T pixels, the block PPB = 256 / LPP lanes, the rows go to float64: (T + PPB + 1) u sum_p |dl a| +
                 sum_p |dl| U (|y s| + |b|) + u |dw|;  db: the same without the activation term.  accumulate: + u |old + new|.
                 No pre-activation margin is needed for the head: relu enters dw and the logits only through max(., 0).
Out of scope here (covered through the network): the batched launchers with passes > 1, the head's bn_rows, the frozen pass, timing.
"""
import numpy as np
import pytest
import torch

import bn_head_bwd_ref as R
from test_gpu_bn_forward_ops import DT, FINALIZE_CASES, GUARD, SENT, L, Out, half_ulp, hold, stored

pytestmark = pytest.mark.gpu

u = 2.0 ** -24
U = 2.0 ** -22
WIDE = ("bf16", "f16")


def guarded_in(a, tdt=torch.float32):
    """An INPUT between two NaN zones: `a` must already hold values of the storage type.  -> (the device view, the whole buffer)"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(tdt)
    assert np.array_equal(t.double().numpy(), a), "the generator's values are not of the storage type"
    buf = torch.full((GUARD + t.numel() + GUARD,), float("nan"), dtype=tdt, device="cuda")
    buf[GUARD:GUARD + t.numel()] = t.reshape(-1).cuda()
    return buf[GUARD:GUARD + t.numel()].view(t.shape), buf


def guarded(a, tdt=torch.float32):
    return guarded_in(a, tdt)[0]


def consts(*arrays):
    return [stored(a)[0] for a in arrays]


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- ustrun_bn_bwd_reduce, ustrun_bn_bwd_apply ----------------------------------------------------------------------------------------
def bn_check(name, n, c, h, w, pooled, mask_all=False, flags=0):
    l = L()
    lib = l.lib()
    dt, tdt = DT[name]
    k = R.bn_case(name, n, c, h, w, pooled, mask_all)
    y, scale, shift, mean, rstd, gamma = (k[v] for v in ("y", "scale", "shift", "mean", "rstd", "gamma"))
    zero, gap = R.margins(y, scale, shift, pooled)
    assert zero >= R.MARGIN and gap >= R.MARGIN, (zero, gap)                # the input conditions, nothing excluded
    if pooled and not mask_all:
        assert all((k["pattern"] == p).any() for p in range(7))
    yg, dag = guarded(y, tdt), guarded(k["da"], tdt)
    dpg = guarded(k["dp"], tdt) if pooled else None
    sg, bg, mg, rg, gg = consts(scale, shift, mean, rstd, gamma)
    count = n * h * w
    nb = lib.ustrun_bn_bwd_partials_bytes(count, c)
    rng = np.random.default_rng(c + h)
    old_dg, old_db = R.f32(rng.normal(size=c)), R.f32(rng.normal(size=c))
    table_ = R.f32(rng.normal(size=(3, c)) * np.array([1.0, 0.3, 0.3])[:, None])           # check 3: coefficients of the test's own
    tg = stored(table_)[0]
    tag0 = f"{name} {(n, c, h, w)} {'pooled' if pooled else 'plain'}{' mask=1' if mask_all else ''}{' flag4096' if flags else ''}"
    old = lib.ustrun_debug_flags(flags)
    try:
        for mode, has_da in ((("da+dp", True), ("dp", False)) if pooled else (("da", True),)):
            plan = R.bn_bwd_plan(name, n, c, h, w, pooled, has_da, four=bool(flags & 4096))
            z, _, _ = R.dz(k["da"] if has_da else None, k["dp"], y, scale, shift)
            s1, s2 = R.bn_bwd_sums(z, y)
            m1, m2 = R.bn_bwd_sums_magnitude(z, y)
            dgamma, dbeta, coef = R.bn_bwd_finalize(s1, s2, count, gamma, mean, rstd)
            d1 = (plan["T"] + plan["PL"]) * U * m1
            d2 = (plan["T"] + plan["PL"] + 1) * U * m2
            ddg = np.abs(rstd) * (d2 + np.abs(mean) * d1)
            dc1 = np.abs(coef[0] * rstd) * ddg / count
            cb = np.stack([2 * u * np.abs(coef[0]), dc1 + 2 * u * np.abs(coef[1]),
                           np.abs(coef[0]) * d1 / count + np.abs(mean) * dc1 + 2 * u * (np.abs(coef[0] * dbeta / count) + np.abs(coef[1] * mean))])
            dap = dag.data_ptr() if has_da else None
            dpp = dpg.data_ptr() if pooled else None
            for acc in ((0, 1) if has_da else (0,)):
                tag = f"{tag0} {mode} accumulate={acc}"
                odg, odb = Out((c,), init=old_dg if acc else None), Out((c,), init=old_db if acc else None)
                ocf, part = Out((3, c)), Out((nb // 4,))
                l.check(lib.ustrun_bn_bwd_reduce(dap, dpp, yg.data_ptr(), sg.data_ptr(), bg.data_ptr(), mg.data_ptr(), rg.data_ptr(),
                                                 gg.data_ptr(), n, h, w, c, odg.ptr, odb.ptr, acc, ocf.ptr, part.ptr, nb, dt, None))
                assert lib.ustrun_debug_last_bn_variant() == plan["code"], (tag, hex(lib.ustrun_debug_last_bn_variant()))
                rdb, rdg = (old_db + dbeta, old_dg + dgamma) if acc else (dbeta, dgamma)
                hold(f"bn_dbeta {tag}", odb.get(), rdb, d1 + u * np.abs(dbeta) + (u * np.abs(rdb) if acc else 0.0))
                hold(f"bn_dgamma {tag}", odg.get(), rdg, ddg + u * np.abs(dgamma) + (u * np.abs(rdg) if acc else 0.0))
                hold(f"bn_coef {tag}", ocf.get(), coef, cb)
                assert part.guards_ok()
            # the apply pass alone, on the test's table
            tag = f"{tag0} {mode}"
            dy = Out((n, h, w, c), tdt)
            l.check(lib.ustrun_bn_bwd_apply(dap, dpp, yg.data_ptr(), sg.data_ptr(), bg.data_ptr(), tg.data_ptr(), n, h, w, c, dy.ptr, dt, None))
            assert lib.ustrun_debug_last_bn_variant() == plan["code"] | 1 << 8, (tag, hex(lib.ustrun_debug_last_bn_variant()))
            ref = R.bn_bwd_apply(z, y, table_)
            hold(f"bn_apply {tag}", dy.get(), ref, U * R.bn_bwd_apply_magnitude(z, y, table_) + half_ulp(ref, name))
            if has_da:          # in place (dy == da): a lane owns its window, loaded before it is stored -- the same bytes
                inp, whole = guarded_in(k["da"], tdt)
                l.check(lib.ustrun_bn_bwd_apply(inp.data_ptr(), dpp, yg.data_ptr(), sg.data_ptr(), bg.data_ptr(), tg.data_ptr(), n, h, w, c,
                                                inp.data_ptr(), dt, None))
                assert lib.ustrun_debug_last_bn_variant() == plan["code"] | 1 << 8
                assert torch.equal(bits(inp), bits(dy.t)), f"bn_apply in place {tag}"
                assert bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[-GUARD:]).all())
    finally:
        lib.ustrun_debug_flags(old)


@pytest.mark.parametrize("name", R.TYPES)
@pytest.mark.parametrize("n,c,h,w,pooled", R.BN_SHAPES)
def test_bn_bwd_reduce_and_apply(n, c, h, w, pooled, name):
    bn_check(name, n, c, h, w, pooled)


@pytest.mark.parametrize("name", WIDE)
def test_bn_bwd_four_channel_kernels_on_16_bit_data(name):
    """ustrun_debug_flags bit 12: (3, 64, 9, 7) on the 4-channel kernels instead of the 8-channel ones"""
    bn_check(name, 3, 64, 9, 7, False, flags=4096)


@pytest.mark.parametrize("name", R.TYPES)
@pytest.mark.parametrize("n,c,h,w,pooled", R.MASK_ALL_SHAPES)
def test_bn_bwd_without_relu(n, c, h, w, pooled, name):
    """scale = 0, shift = 1: how a BatchNorm that no ReLU follows is passed (include/ustrun.h).  The mask is all ones and every window
    an all-way tie: dp goes to position 0."""
    bn_check(name, n, c, h, w, pooled, mask_all=True)


# ---- ustrun_bn_bwd_finalize_stat ------------------------------------------------------------------------------------------------------
# bn_bwd_finalize_stat (csrc/bn.hip), the rule of the forward statistics: staged (bn_stat_stage1_kernel reduces the table in place, then
# bn_bwd_finalize_kernel<true>) when rows >= 96 and C % 32 == 0, with R = ceil(rows / 32) raised until rows % R != 1; else
# bn_bwd_finalize_kernel<false> sums the rows directly.  Four passes per round of the kernel's loop: five take a second round.
@pytest.mark.parametrize("passes", [1, 3, 5])
@pytest.mark.parametrize("rows,c", FINALIZE_CASES)
def test_bn_bwd_finalize_stat(rows, c, passes):
    l = L()
    lib = l.lib()
    for aff_stride in (c, c + 8):
        stat, count, gamma, mean, rstd, old_dg, old_db = R.finalize_stat_case(rows, c, passes, aff_stride)
        assert aff_stride == c or (np.isnan(mean).sum() == 8 * (passes - 1) and np.isnan(rstd).sum() == 8 * (passes - 1))
        assert abs(mean[R.HI] * rstd[R.HI]) > 999 and gamma[R.G0 % c] == 0 and gamma[R.GNEG % c] < 0
        per = [R.finalize_rows(stat[p], count, gamma, mean[p * aff_stride:][:c], rstd[p * aff_stride:][:c]) for p in range(passes)]
        coef = np.stack([p[2] for p in per])
        cb = np.stack([np.stack([2 * u * np.abs(k[0]), 2 * u * np.abs(k[1]),
                                 2 * u * (np.abs(k[0] * db / count) + np.abs(k[1] * mean[p * aff_stride:][:c]))])
                       for p, (_, db, k) in enumerate(per)])
        gg, mg, rg = consts(gamma, mean, rstd)
        for acc in (0, 1):
            tag = f"({rows},{c}) passes={passes} aff_stride={aff_stride} accumulate={acc}"
            st = Out(stat.shape, init=stat)             # reduced in place: a copy between guard zones
            odg, odb, ocf = Out((c,), init=old_dg if acc else None), Out((c,), init=old_db if acc else None), Out((passes, 3, c))
            l.check(lib.ustrun_bn_bwd_finalize_stat(st.ptr, rows, passes, c, count, gg.data_ptr(), mg.data_ptr(), rg.data_ptr(), aff_stride,
                                                    odg.ptr, odb.ptr, acc, ocf.ptr, None))
            for what, o, first, col in (("dgamma", odg, old_dg, 0), ("dbeta", odb, old_db, 1)):
                terms = ([first] if acc else []) + [p[col] for p in per]
                ref, mag = np.sum(terms, axis=0), np.sum(np.abs(terms), axis=0)
                hold(f"finalize_stat_{what} f32 {tag}", o.get(), ref, (passes + acc) * u * mag + u * np.abs(ref))
            hold(f"finalize_stat_coef f32 {tag}", ocf.get(), coef, cb)
            assert (ocf.get()[:, :, R.G0 % c] == 0).all()
            assert st.guards_ok()


# ---- ustrun_bn_bwd_apply_head ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WIDE)
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("c", [8, 128, 2048])
@pytest.mark.parametrize("n,h,w", [(3, 9, 7), (1, 1, 1)])
def test_apply_head_runtime_k_against_float64(n, h, w, c, k, name):
    """The run-time-K build of bn_bwd_apply_head_x8_kernel (K not in {2, 4}) at G8 = 1, 16 and 256, by the dyadic-data method of
    test_gpu_backward_round_trips.py's test_apply_from_dlogits_against_float64: dl and w are multiples of 1/32 below 1, so g = sum_k dl w
    (up to 13 significant bits at K = 8) is exact in float32 and its rounding to 8 / 11 bits is exercised; y multiples of 1/4, the
    constants dyadic: every float32 intermediate is exact and float64 gives the same value before each rounding -- the expectation is
    met bit for bit.  Also bit-identical to ustrun_head_bwd (da stored; head_bwd_kernel<2, 0>) + ustrun_bn_bwd_apply."""
    l = L()
    lib = l.lib()
    dt, tdt = DT[name]
    rng = np.random.default_rng(100 * k + c + h)
    ri = lambda lo, hi, *shape: rng.integers(lo, hi + 1, size=shape).astype(np.float64)
    y = ri(-8, 8, n, h, w, c) / 4
    dl = ri(-31, 31, n, k, h, w) / 32
    wt = ri(-31, 31, k, c) / 32
    scale = rng.choice([0.5, 1.0, 2.0], size=c) * (2 * ri(0, 1, c) - 1)
    shift = ri(-4, 4, c) / 4
    coef = np.stack([ri(-15, 15, c) / 8, ri(-15, 15, c) / 16, ri(-15, 15, c) / 8])
    g64, _, _ = R.head_bwd(dl, y, None, None, wt)
    g16 = R.rounded(g64, name)
    if n * h * w > 1 and (name == "bf16" or k == 8):      # (f16 holds 11 bits: three products of 5-bit numbers rarely need more)
        assert (g16 != g64).any()                         # the rounding to the storage type is exercised
    z = np.where(y * scale + shift > 0, g16, 0.0)
    want = R.rounded(R.bn_bwd_apply(z, y, coef), name)
    yg, dlg = guarded(y, tdt), guarded(dl)
    sg, bg, cg, wg = consts(scale, shift, coef, wt)
    dy = Out((n, h, w, c), tdt)
    l.check(lib.ustrun_bn_bwd_apply_head(dlg.data_ptr(), wg.data_ptr(), yg.data_ptr(), sg.data_ptr(), bg.data_ptr(), cg.data_ptr(), n, h, w, c,
                                         k, dy.ptr, dt, 1, c, None))
    assert np.array_equal(dy.get(), want), f"apply_head {name} C={c} K={k} {(n, h, w)}"
    # the two-kernel route
    row = k * c + k
    part = torch.empty(1024 * row, device="cuda")
    da, dw, db = Out((n, h, w, c), tdt), Out((k, c)), Out((k,))
    l.check(lib.ustrun_head_bwd(dlg.data_ptr(), yg.data_ptr(), sg.data_ptr(), bg.data_ptr(), n * h * w, h * w, c, k, wg.data_ptr(), da.ptr, dw.ptr,
                                db.ptr, 0, part.data_ptr(), part.numel() * 4, dt, None))
    assert np.array_equal(da.get(), g16)
    dy2 = Out((n, h, w, c), tdt)
    l.check(lib.ustrun_bn_bwd_apply(da.ptr, None, yg.data_ptr(), sg.data_ptr(), bg.data_ptr(), cg.data_ptr(), n, h, w, c, dy2.ptr, dt, None))
    assert torch.equal(bits(dy2.t), bits(dy.t)) and dy2.guards_ok()


# ---- ustrun_head_fwd, ustrun_head_bwd -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.TYPES)
@pytest.mark.parametrize("c,k", R.HEAD_CK)
def test_head_forward_and_backward(c, k, name):
    """Every dispatch edge of ustrun_head_fwd (K > G = C / 8 and G = 3: the generic kernel; G = 64: one wave per pixel; C = 1024: four
    channel rounds; C = 64 with H W = 256: the 64-channel kernel, bit-identical to the generic 16-bit one) and of ustrun_head_bwd
    (K = 2 / 4 at compile time, every other K at run time; C = 264: a second channel round with 62 idle lanes behind the barriers),
    with the BatchNorm constants + ReLU and without (scale = shift = NULL), accumulate 0 and 1."""
    l = L()
    lib = l.lib()
    dt, tdt = DT[name]
    for n, h, w in R.HEAD_EXTENTS + ([(2, 16, 16)] if c == 64 else []):
        q = R.head_case(name, c, k, n, h, w)
        y, wt, bias, dl = q["y"], q["w"], q["bias"], q["dl"]
        npix = n * h * w
        yg, dlg = guarded(y, tdt), guarded(dl)
        sg, bg, wg, biasg = consts(q["scale"], q["shift"], wt, bias)
        lpp, ppb, blocks, T = R.head_plan(npix, c)
        part = Out((1024 * (k * c + k),))
        for affine in (True, False):
            s, b = (q["scale"], q["shift"]) if affine else (None, None)
            sp, bp = (sg.data_ptr(), bg.data_ptr()) if affine else (None, None)
            tag = f"{name} C={c} K={k} {(n, h, w)} affine={affine}"
            ref = R.head_fwd(y, s, b, wt, bias)
            maw, mw = R.head_fwd_magnitude(y, s, b, wt)
            lg = Out((n, k, h, w))
            l.check(lib.ustrun_head_fwd(yg.data_ptr(), sp, bp, npix, h * w, c, k, wg.data_ptr(), biasg.data_ptr(), lg.ptr, dt, None))
            hold(f"head_logits {tag}", lg.get(), ref, (c + 2) * u * maw + U * mw + u * np.abs(ref))
            if c == 64 and h * w == 256 and name in WIDE and k <= 4:
                old = lib.ustrun_debug_flags(1 << 27)
                try:
                    lg2 = Out((n, k, h, w))
                    l.check(lib.ustrun_head_fwd(yg.data_ptr(), sp, bp, npix, h * w, c, k, wg.data_ptr(), biasg.data_ptr(), lg2.ptr, dt, None))
                finally:
                    lib.ustrun_debug_flags(old)
                assert torch.equal(bits(lg2.t), bits(lg.t)) and lg2.guards_ok(), f"head_fwd 64-channel kernel {tag}"
            rda, rdw, rdb = R.head_bwd(dl, y, s, b, wt)
            mda, mdw, mdwa, mdb = R.head_bwd_magnitude(dl, y, s, b, wt)
            for acc in (0, 1):
                da, dw, db = Out((n, h, w, c), tdt), Out((k, c), init=q["dw0"] if acc else None), Out((k,), init=q["db0"] if acc else None)
                l.check(lib.ustrun_head_bwd(dlg.data_ptr(), yg.data_ptr(), sp, bp, npix, h * w, c, k, wg.data_ptr(), da.ptr, dw.ptr, db.ptr, acc,
                                            part.ptr, part.t.numel() * 4, dt, None))
                hold(f"head_da {tag} accumulate={acc}", da.get(), rda, (k + 1) * u * mda + half_ulp(rda, name))
                fw, fb = (q["dw0"] + rdw, q["db0"] + rdb) if acc else (rdw, rdb)
                hold(f"head_dw {tag} accumulate={acc}", dw.get(), fw,
                     (T + ppb + 1) * u * mdw + U * mdwa + u * np.abs(rdw) + (u * np.abs(fw) if acc else 0.0))
                hold(f"head_db {tag} accumulate={acc}", db.get(), fb, (T + ppb + 1) * u * mdb + u * np.abs(rdb) + (u * np.abs(fb) if acc else 0.0))
                assert part.guards_ok()


# ---- documented refusals --------------------------------------------------------------------------------------------------------------
def test_documented_refusals():
    """Each returns nonzero with its message and leaves the outputs' sentinels untouched: refused before any launch."""
    l = L()
    lib = l.lib()
    n, h, w, c, k = 1, 4, 6, 8, 2
    x32 = torch.zeros(4096, device="cuda")
    one = torch.ones(64, device="cuda")
    p, xp = one.data_ptr(), x32.data_ptr()
    nb = lib.ustrun_bn_bwd_partials_bytes(n * h * w, c)
    outs = {v: Out((4096,)) for v in ("dgamma", "dbeta", "coef", "dy", "part", "logits", "da", "dw", "db")}
    o = {v: t.ptr for v, t in outs.items()}

    def refused(rc, text):
        assert rc != 0, text
        assert text.encode() in lib.ustrun_last_error(), (text, lib.ustrun_last_error())

    def reduce(da=xp, dp=None, hh=h, ww=w, cc=c, bytes_=nb, dt=0):
        return lib.ustrun_bn_bwd_reduce(da, dp, xp, p, p, p, p, p, n, hh, ww, cc, o["dgamma"], o["dbeta"], 0, o["coef"], o["part"], bytes_, dt, None)

    def apply(da=xp, dp=None, hh=h, ww=w, cc=c, dt=0):
        return lib.ustrun_bn_bwd_apply(da, dp, xp, p, p, p, n, hh, ww, cc, o["dy"], dt, None)

    refused(reduce(cc=6, bytes_=1 << 20), "bn_bwd_reduce: N=1 H=4 W=6 C=6 (must be a multiple of 4)")
    refused(apply(cc=6), "bn_bwd_apply: N=1 H=4 W=6 C=6 (must be a multiple of 4)")
    refused(reduce(dt=7), "bn_bwd_reduce: dtype 7 not built")
    refused(apply(dt=7), "bn_bwd_apply: dtype 7 not built")
    refused(reduce(da=None), "bn_bwd_reduce: null pointer")
    refused(apply(da=None), "bn_bwd_apply: null pointer")
    refused(reduce(bytes_=nb - 4), "bn_bwd_reduce: partials too small")
    for dt in (0, 1, 2, 3):          # a pooled map without elements: dp would be read outside the tensor
        for hh, ww in ((1, 6), (4, 1), (1, 1)):
            for da in (xp, None):
                refused(reduce(da=da, dp=xp, hh=hh, ww=ww, dt=dt), f"bn_bwd_reduce: pooled windows need H, W >= 2 ({hh}x{ww})")
                refused(apply(da=da, dp=xp, hh=hh, ww=ww, dt=dt), f"bn_bwd_apply: pooled windows need H, W >= 2 ({hh}x{ww})")

    npix, hw = n * h * w, h * w

    def fwd(kk=k, cc=c, np_=npix, hw_=hw):
        return lib.ustrun_head_fwd(xp, p, p, np_, hw_, cc, kk, p, p, o["logits"], 0, None)

    def bwd(kk=k, cc=c, da="da", dw="dw", db="db"):
        return lib.ustrun_head_bwd(xp, xp, p, p, npix, hw, cc, kk, p, o.get(da), o.get(dw), o.get(db), 0, o["part"], 4 * 4096, 0, None)

    refused(fwd(kk=0), "head_fwd: C=8 K=0 unsupported")
    refused(fwd(kk=9), "head_fwd: C=8 K=9 unsupported")
    refused(fwd(cc=6), "head_fwd: C=6 K=2 unsupported")
    refused(fwd(np_=npix + 1), "head_fwd: bad extent")
    refused(bwd(kk=0), "head_bwd: C=8 K=0 unsupported")
    refused(bwd(kk=9), "head_bwd: C=8 K=9 unsupported")
    refused(bwd(cc=6), "head_bwd: C=6 K=2 unsupported")
    for missing in ("da", "dw", "db"):
        refused(bwd(**{missing: None}), "head_bwd: null pointer")
    torch.cuda.synchronize()
    for v, t in outs.items():
        assert t.guards_ok() and bool((t.t == SENT).all()), v
