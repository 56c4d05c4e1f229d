"""inf and NaN through the BatchNorm kernels of the f16 step and the kernels fused with them, one C-ABI call at a time
(the gates of tests/test_gpu_nonfinite_ops.py; float64 classes from tests/nonfinite_ref.py):

  ustrun_bn_finalize                       a statistics row as an inf / -inf / NaN element leaves it (sum AND sum of squares)
  ustrun_bn_bwd_reduce                     inf in da, inf in y, a NaN BatchNorm scale (the backward mask's operand turns NaN, y stays finite)
  ustrun_bn_bwd_finalize_stat              a poisoned row of one pass
  ustrun_bn_bwd_apply, _apply_head         the same plants, elementwise, plus gate 1 on their 16-bit store
  ustrun_conv3x3_dgrad_bnsum               (linear tiles, and the streaming 64 -> 64 kernel) and
  ustrun_convT2x2_dgrad_bnsum              inf in the incoming gradient, a NaN scale: da per element, the statistics rows per pass and channel
  ustrun_conv_first_wgrad_bn               the step's first-layer weight gradient (apply + mask in its loader): poisoned da, y, scale, image
  ustrun_seg_loss_bwd                      an infinite loss scale in the device state it reads (gdev)

Containment of the BatchNorm kernels is per channel and per pass: every channel (and pass) the plant does not touch keeps, bit for bit,
what a clean run of the same call gives; in the poisoned channel everything that is a function of a non-finite sum must be non-finite
(dbeta = s1 with the float64 class; dgamma = rstd (s2 - mean s1), c1 = -c0 dgamma rstd / count, c2 = -c0 dbeta / count - c1 mean: no IEEE
operation there makes a finite value of inf or NaN), c0 = gamma rstd keeps its bits.  Elementwise kernels are judged per element against
float64 on dyadic data (every float32 intermediate exact).  Backward masks: "torch" passes the gradient where a is NaN, "select" is
a > 0 ? g : 0; a NaN *scale* makes a NaN while y stays finite, so the two conventions give different finite values.

Special values go into floating operands only (gradients, raw outputs, BatchNorm constants, statistics rows, the loss scale); label maps
and masks of ustrun_seg_loss_bwd stay clean.  bn_bwd.h casts indices only; no case was dropped."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nonfinite_ref as NF
from test_gpu_nonfinite_ops import INF, NAN, OVERFLOW_STORED, TDT, ZO, from_nhwc, guarded, nhwc16, weight_gradient_mismatches, wgrad_in_range, whole
from test_gpu_production_tiles import L, variant

pytestmark = pytest.mark.gpu

ELT = "f16"
T16, CODE = TDT[ELT]


def gen(seed):
    g = torch.Generator().manual_seed(seed)
    return g, (lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float())


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def apply_ref(y, da, sc, sh, coef, conv):
    """float64: dy = k0 relu'(y scale + shift; da) + k1 y + k2; y, da [P, N, H, W, C], tables [P, C] / [P, 3, C]"""
    e = lambda t: t.double()[:, None, None, None, :]
    z = NF.relu_bwd(y * e(sc) + e(sh), da, conv)
    return e(coef[:, 0]) * z + e(coef[:, 1]) * y + e(coef[:, 2]), z


def apply_case(seed, P, n, h, w, c):
    g, ri = gen(seed)
    y, da = ri(-4, 4, P, n, h, w, c) / 2, ri(-2, 2, P, n, h, w, c)
    sc = (1 + ri(0, 1, P, c)) * (2 * ri(0, 1, P, c) - 1)
    sh = ri(-2, 2, P, c) / 2
    coef = torch.stack([torch.tensor([-2.0, -1.0, 0.5, 1.0, 2.0])[torch.randint(0, 5, (P, c), generator=g)], ri(-2, 2, P, c) / 2, ri(-2, 2, P, c) / 2], 1)
    return y, da, sc, sh, coef


def overflow_tables(y, da, sc, sh, coef, pix):
    """channels 0..3 of pass 0 store 32 * 2047, + 15, + 16 and 1024 * 2047 at pixel `pix`, channels 4..7 their negatives"""
    i, yy, xx = pix
    sc[0, :8], sh[0, :8] = 1.0, 0.5                                        # a = y + 0.5 > 0 at y = 1
    coef[0, 0, :4], coef[0, 1, :8] = torch.tensor([32.0, 32.0, 32.0, 1024.0]), 0.0
    coef[0, 2, :4] = torch.tensor([0.0, 15.0, 16.0, 0.0])
    coef[0, 0, 4:8], coef[0, 2, 4:8] = -coef[0, 0, :4], -coef[0, 2, :4]
    y[0, i, yy, xx, :8], da[0, i, yy, xx, :8] = 1.0, 2047.0


APPLY_PLANTS = ["da inf corner", "da -inf last pixel, channel tail", "y inf", "+nan y", "nan scale", "overflow"]


@pytest.mark.parametrize("n,c,h,w", [(2, 64, 12, 16), (3, 8, 9, 7), (2, 96, 8, 8)])
def test_bn_bwd_apply_nonfinite(n, c, h, w):
    """ustrun_bn_bwd_apply (8 channels per lane, one octet on an odd extent, the 4-channel kernels at 12 octets), per element"""
    l, lib = L(), L().lib()
    for label in APPLY_PLANTS:
        y, da, sc, sh, coef = apply_case(c + h, 1, n, h, w, c)
        if label == "da inf corner":
            da[0, 0, 0, 0, 0] = INF
        elif label.startswith("da -inf"):
            da[0, n - 1, h - 1, w - 1, c - 1] = -INF
        elif label == "y inf":
            y[0, 0, 3, 2, 1] = INF * float(torch.sign(sc[0, 1]))           # a = +inf: the mask passes, k1 y is +-inf (NaN where k1 = 0)
        elif label == "+nan y":
            y[0, n - 1, 1, 1, 2] = NAN
        elif label == "nan scale":
            sc[0, 3] = NAN
        else:
            overflow_tables(y, da, sc, sh, coef, (n - 1, 2, 3))
        refs = {cv: apply_ref(NF.stored(y, ELT), NF.stored(da, ELT), sc, sh, coef, cv)[0][0] for cv in NF.CONVENTIONS}
        yg, dag = y[0].to(T16).cuda(), da[0].to(T16).cuda()
        scg, shg, cg = sc[0].cuda(), sh[0].cuda(), coef[0].contiguous().cuda()
        ob, dy = guarded((n, h, w, c), T16, 9.0)
        l.check(lib.ustrun_bn_bwd_apply(dag.data_ptr(), None, yg.data_ptr(), scg.data_ptr(), shg.data_ptr(), cg.data_ptr(), n, h, w, c, dy.data_ptr(), CODE, None))
        assert whole(ob, 9.0), "bn_bwd_apply wrote outside dy"
        got = dy.float().cpu()
        if label == "overflow":
            assert got[n - 1, 2, 3, :4].tolist() == OVERFLOW_STORED and got[n - 1, 2, 3, 4:8].tolist() == [-t for t in OVERFLOW_STORED], got[n - 1, 2, 3, :8].tolist()
        names = [cv for cv in refs if NF.mismatches(got, refs[cv], ELT)[:2] == (0, 0)]
        assert names, f"bn_bwd_apply C={c} {label}: {NF.mismatches(got, refs['torch'], ELT)}"
        if label == "nan scale":
            assert len(names) == 1
            print(f"NaN convention: bn_bwd_apply C={c} backward mask: {names[0]}")


@pytest.mark.parametrize("n,h,w,k,passes", [(3, 9, 7, 2, 2), (2, 12, 16, 4, 1)])
def test_bn_bwd_apply_head_nonfinite(n, h, w, k, passes):
    """ustrun_bn_bwd_apply_head, C = 64: g = sum_k dlogits[k] w[k] rounded to half (65520 becomes inf THERE), then the apply formula;
    per element, per pass"""
    l, lib = L(), L().lib()
    c = 64
    for label in ["dl inf corner", "dl -inf last pixel, last pass", "nan scale", "overflow", "overflow of g"]:
        y, _, sc, sh, coef = apply_case(k + h, passes, n, h, w, c)
        g_, ri = gen(17 * k + h)
        dl, wt = ri(-4, 4, passes, n, k, h, w) / 4, ri(-4, 4, k, c) / 4
        if label == "dl inf corner":
            dl[0, 0, 0, 0, 0] = INF
        elif label.startswith("dl -inf"):
            dl[passes - 1, n - 1, k - 1, h - 1, w - 1] = -INF
        elif label == "nan scale":
            sc[passes - 1, 5] = NAN
        elif label == "overflow":                  # g = 2047 through a one-hot weight, then the four sums
            da0 = torch.zeros(passes, n, h, w, c)
            overflow_tables(y, da0, sc, sh, coef, (n - 1, 2, 3))
            wt[:, :8], wt[0, :8] = 0.0, 1.0
            dl[0, n - 1, :, 2, 3], dl[0, n - 1, 0, 2, 3] = 0.0, 2047.0
        else:                                      # g itself: 65504, 65519 -> 65504, 65520, 2096128 -> inf; dy = 1 g (+ 0 y + 0)
            sc[0, :8], sh[0, :8] = 1.0, 0.5
            coef[0, 0, :8], coef[0, 1, :8], coef[0, 2, :8] = 1.0, 0.0, 0.0
            wt[:, :8] = 0.0
            wt[0, :4], wt[0, 4:8] = 1.0, -1.0
            y[0, 0, 1:5, 1, :8] = 1.0
            dl[0, 0, :, 1:5, 1] = 0.0
            dl[0, 0, 0, 1:5, 1] = torch.tensor([65504.0, 65519.0, 65520.0, 2096128.0])
        g64 = torch.einsum("pnkhw,kc->pnhwc", dl.double(), wt.double())
        refs = {cv: apply_ref(NF.stored(y, ELT), NF.stored(g64, ELT), sc, sh, coef, cv)[0] for cv in NF.CONVENTIONS}
        aff = torch.zeros(passes, 4, c)
        aff[:, 0], aff[:, 1] = sc, sh
        affg, cg, wg, yg, dlg = aff.cuda(), coef.contiguous().cuda(), wt.contiguous().cuda(), y.to(T16).cuda(), dl.contiguous().cuda()
        ob, dy = guarded((passes, n, h, w, c), T16, 9.0)
        l.check(lib.ustrun_bn_bwd_apply_head(dlg.data_ptr(), wg.data_ptr(), yg.data_ptr(), affg.data_ptr(), affg.data_ptr() + 4 * c, cg.data_ptr(),
                                             n, h, w, c, k, dy.data_ptr(), CODE, passes, 4 * c, None))
        assert whole(ob, 9.0), "bn_bwd_apply_head wrote outside dy"
        got = dy.float().cpu()
        if label == "overflow":
            assert got[0, n - 1, 2, 3, :4].tolist() == OVERFLOW_STORED and got[0, n - 1, 2, 3, 4:8].tolist() == [-t for t in OVERFLOW_STORED], got[0, n - 1, 2, 3, :8].tolist()
        if label == "overflow of g":
            assert got[0, 0, 1:5, 1, 0].tolist() == OVERFLOW_STORED and got[0, 0, 1:5, 1, 4].tolist() == [-t for t in OVERFLOW_STORED], got[0, 0, 1:5, 1, 0].tolist()
        names = [cv for cv in refs if NF.mismatches(got, refs[cv], ELT)[:2] == (0, 0)]
        assert names, f"bn_bwd_apply_head K={k} {label}: {NF.mismatches(got, refs['torch'], ELT)}"
        if label == "nan scale":
            assert len(names) == 1
            print(f"NaN convention: bn_bwd_apply_head K={k} backward mask: {names[0]}")


def reduce_call(l, lib, y, da, sc, sh, mean, rstd, gamma, n, h, w, c):
    nb = lib.ustrun_bn_bwd_partials_bytes(n * h * w, c)
    part = torch.full((nb // 4,), NAN, device="cuda")                        # written before it is read, not assumed clean
    yg, dag = y.to(T16).cuda(), da.to(T16).cuda()
    t = [v.contiguous().cuda() for v in (sc, sh, mean, rstd, gamma)]
    ob, out = guarded((5, c), torch.float32, NAN)                            # dgamma, dbeta, coef[3]
    l.check(lib.ustrun_bn_bwd_reduce(dag.data_ptr(), None, yg.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                     t[4].data_ptr(), n, h, w, c, out[0].data_ptr(), out[1].data_ptr(), 0, out[2].data_ptr(), part.data_ptr(), nb, CODE, None))
    assert whole(ob, NAN), "bn_bwd_reduce wrote outside its outputs"
    return out.cpu().clone()


def judge_channels(got, clean, bad, what):
    """rows: dgamma, dbeta, c0, c1, c2.  Clean channels keep the clean run's bits in every row; a poisoned channel keeps c0 and has
    non-finite dgamma, dbeta, c1, c2 (functions of the non-finite sums)"""
    for ch in range(got.shape[-1]):
        if ch in bad:
            assert bits_equal(got[2, ch:ch + 1], clean[2, ch:ch + 1]), f"{what}: c0 of channel {ch} moved"
            assert not bool(torch.isfinite(got[[0, 1, 3, 4], ch]).any()), f"{what}: channel {ch} is poisoned, got finite {got[:, ch].tolist()}"
        else:
            assert bits_equal(got[:, ch].clone(), clean[:, ch].clone()), f"{what}: untouched channel {ch} differs from the clean run: {got[:, ch].tolist()} / {clean[:, ch].tolist()}"


@pytest.mark.parametrize("n,c,h,w", [(2, 64, 12, 16), (3, 8, 9, 7), (2, 96, 8, 8)])
def test_bn_bwd_reduce_nonfinite(n, c, h, w):
    l, lib = L(), L().lib()
    g_, ri = gen(c + w)
    mean, rstd, gamma = ri(-2, 2, c) / 2, torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c,), generator=g_)], ri(1, 3, c) / 2
    base = apply_case(c + h, 1, n, h, w, c)
    clean = reduce_call(l, lib, base[0][0], base[1][0], base[2][0], base[3][0], mean, rstd, gamma, n, h, w, c)
    assert bool(torch.isfinite(clean).all())
    for label, ch in (("da inf corner", 0), ("da -inf last pixel", c - 1), ("y inf", 1), ("-nan da", 2), ("nan scale", 3)):
        y, da, sc, sh, _ = (t.clone() for t in base)
        up = 2.0 * float(torch.sign(sc[0, ch]))          # y that makes a = y scale + shift >= 1: the mask passes the planted gradient
        if label == "da inf corner":
            da[0, 0, 0, 0, ch], y[0, 0, 0, 0, ch] = INF, up
        elif label.startswith("da -inf"):
            da[0, n - 1, h - 1, w - 1, ch], y[0, n - 1, h - 1, w - 1, ch] = -INF, up
        elif label == "y inf":
            y[0, 0, 3, 2, ch] = INF * float(torch.sign(sc[0, ch]))
            da[0, 0, 3, 2, ch] = 1.0
        elif label == "-nan da":
            da[0, n - 1, 1, 1, ch], y[0, n - 1, 1, 1, ch] = -NAN, up
        else:
            sc[0, ch] = NAN
        got = reduce_call(l, lib, y[0], da[0], sc[0], sh[0], mean, rstd, gamma, n, h, w, c)
        tag = f"bn_bwd_reduce C={c} {label}"
        if label == "nan scale":
            # the mask's operand is NaN in the whole channel, y and da are finite: dbeta = sum of the passed gradients, an exact integer
            s1 = {cv: float(apply_ref(NF.stored(y, ELT), NF.stored(da, ELT), sc, sh, torch.zeros(1, 3, c), cv)[1][..., ch].sum()) for cv in NF.CONVENTIONS}
            assert s1["torch"] != s1["select"]
            names = [cv for cv in NF.CONVENTIONS if float(got[1, ch]) == s1[cv]]
            assert len(names) == 1, (tag, float(got[1, ch]), s1)
            print(f"NaN convention: bn_bwd_reduce C={c} backward mask: {names[0]}")
            judge_channels(torch.cat([got[:, :ch], got[:, ch + 1:]], 1), torch.cat([clean[:, :ch], clean[:, ch + 1:]], 1), (), tag)
            continue
        z = apply_ref(NF.stored(y, ELT), NF.stored(da, ELT), sc, sh, torch.zeros(1, 3, c), "torch")[1]
        s1, s2 = z[..., ch].sum(), (z * NF.stored(y, ELT))[..., ch].sum()
        if int(NF.classify(s1)) == NF.FINITE:     # an inf y under a finite gradient: s2 alone goes; dbeta = s1 is an exact dyadic sum
            assert int(NF.classify(s2)) != NF.FINITE and float(got[1, ch]) == float(s1), (tag, float(got[1, ch]), float(s1), float(s2))
            assert bits_equal(got[2, ch:ch + 1], clean[2, ch:ch + 1]) and not bool(torch.isfinite(got[[0, 3, 4], ch]).any()), (tag, got[:, ch].tolist())
            keep = [i for i in range(c) if i != ch]
            judge_channels(got[:, keep], clean[:, keep], (), tag)
            continue
        assert int(NF.classify(got[1, ch])) == int(NF.classify(s1)), (tag, "dbeta", float(got[1, ch]), float(s1))
        judge_channels(got, clean, (ch,), tag)


@pytest.mark.parametrize("rows,c,passes", [(7, 24, 1), (97, 64, 3)])
def test_bn_bwd_finalize_stat_nonfinite(rows, c, passes):
    """direct and staged reduction of the rows; the plant sits in one row of ONE pass: that pass's coefficients of the channel go, the other
    passes' stay to the bit; dgamma and dbeta add the passes up and go with it"""
    l, lib = L(), L().lib()
    g_, ri = gen(rows + c)
    stat = ri(-64, 64, passes, rows, 2, c) / 4
    mean, rstd, gamma = ri(-2, 2, passes, c) / 2, torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (passes, c), generator=g_)], ri(1, 3, c) / 2
    count = 4 * rows

    def call(st):
        sb, sg = guarded((passes, rows, 2, c), torch.float32, 7.0)
        sg.copy_(st)
        ob, out = guarded((2 + 3 * passes, c), torch.float32, NAN)
        mg, rg, gg = mean.contiguous().cuda(), rstd.contiguous().cuda(), gamma.cuda()
        l.check(lib.ustrun_bn_bwd_finalize_stat(sg.data_ptr(), rows, passes, c, count, gg.data_ptr(), mg.data_ptr(), rg.data_ptr(), c, out[0].data_ptr(),
                                                out[1].data_ptr(), 0, out[2].data_ptr(), None))
        assert whole(sb, 7.0) and whole(ob, NAN), "bn_bwd_finalize_stat wrote outside its table or outputs"
        return out.cpu().clone()

    clean = call(stat)
    assert bool(torch.isfinite(clean).all())
    for label, val, p, r, col, ch in (("inf sum, first row", INF, 0, 0, 0, 0), ("-inf sum, last row, last pass", -INF, passes - 1, rows - 1, 0, c - 1),
                                      ("nan product sum", NAN, passes // 2, rows // 2, 1, 5)):
        st = stat.clone()
        st[p, r, col, ch] = val
        got = call(st)
        tag = f"bn_bwd_finalize_stat ({rows},{c}) x{passes} {label}"
        for q in range(passes):
            rows_q = torch.cat([got[:2], got[2 + 3 * q:5 + 3 * q]])
            clean_q = torch.cat([clean[:2], clean[2 + 3 * q:5 + 3 * q]])
            if q == p:
                if col == 1:                     # s2 alone: dbeta (= sum of s1) stays, dgamma, c1, c2 go
                    assert bits_equal(got[1], clean[1]) and not bool(torch.isfinite(rows_q[[0, 3, 4], ch]).any()), (tag, rows_q[:, ch].tolist())
                    judge_channels(torch.cat([rows_q[:, :ch], rows_q[:, ch + 1:]], 1), torch.cat([clean_q[:, :ch], clean_q[:, ch + 1:]], 1), (), tag)
                else:
                    assert int(NF.classify(got[1, ch])) == (NF.PINF if val > 0 else NF.NINF), (tag, float(got[1, ch]))
                    judge_channels(rows_q, clean_q, (ch,), tag)
            else:                                # another pass: its coefficients keep their bits in every channel
                assert bits_equal(got[2 + 3 * q:5 + 3 * q], clean[2 + 3 * q:5 + 3 * q]), f"{tag}: the coefficients of pass {q} moved"


@pytest.mark.parametrize("mtiles,c", [(7, 24), (97, 64)])
def test_bn_finalize_nonfinite(mtiles, c):
    """direct and staged; one row of one channel as a convolution leaves it when ONE stored output is +inf / -inf / NaN (sum and sum of
    squares both).  torch's BatchNorm2d (tests/test_nonfinite_ref_host.py): mean of the element's class, everything after it NaN, the running
    variance NaN -- the class of every output of the channel is computed in float64 by the kernel's own formula; every other channel
    keeps the clean run's bits, running buffers included"""
    l, lib = L(), L().lib()
    g_, ri = gen(mtiles + c)
    s1 = ri(-64, 64, mtiles, c) / 4
    stat = torch.stack([s1, s1.abs() * 8 + 64], 1)                            # a variance well above zero
    gamma, beta, rm, rv = ri(1, 3, c) / 2, ri(-2, 2, c) / 2, ri(-2, 2, c) / 2, ri(1, 3, c) / 2
    count, momentum, eps = 16 * mtiles, 0.1, 1e-5

    def call(st):
        sb, sg = guarded((mtiles, 2, c), torch.float32, 7.0)
        sg.copy_(st)
        ob, out = guarded((6, c), torch.float32, NAN)                          # scale, shift, mean, rstd, running_mean, running_var
        out[4].copy_(rm), out[5].copy_(rv)
        nbt = torch.tensor([5], dtype=torch.int64, device="cuda")
        gg, bg = gamma.cuda(), beta.cuda()
        l.check(lib.ustrun_bn_finalize(sg.data_ptr(), mtiles, c, count, gg.data_ptr(), bg.data_ptr(), out[4].data_ptr(), out[5].data_ptr(), nbt.data_ptr(),
                                       momentum, eps, 1, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), None))
        assert whole(sb, 7.0) and whole(ob, NAN) and int(nbt.item()) == 6
        return out.cpu().clone()

    clean = call(stat)
    assert bool(torch.isfinite(clean).all())
    for label, v1, r, ch in (("+inf element, first row", INF, 0, 0), ("-inf element, last row, channel tail", -INF, mtiles - 1, c - 1), ("nan element", NAN, mtiles // 2, 3)):
        st = stat.clone()
        st[r, 0, ch], st[r, 1, ch] = v1, (NAN if v1 != v1 else INF)
        got = call(st)
        tag = f"bn_finalize ({mtiles},{c}) {label}"
        t1, t2 = st[:, 0, ch].double().sum(), st[:, 1, ch].double().sum()
        m = t1 / count
        var = t2 / count - m * m
        rs = 1.0 / torch.sqrt(var + eps)
        scale = gamma[ch].double() * rs
        want = [scale, beta[ch].double() - m * scale, m, rs, 0.9 * rm[ch].double() + 0.1 * m, 0.9 * rv[ch].double() + 0.1 * var * count / (count - 1)]
        assert [int(NF.classify(v)) for v in want[3:]] == [NF.NAN, int(NF.classify(v1 * torch.ones(()))), NF.NAN]
        assert [int(NF.classify(v)) for v in got[:, ch]] == [int(NF.classify(v)) for v in want], (tag, got[:, ch].tolist(), [float(v) for v in want])
        keep = [i for i in range(c) if i != ch]
        assert bits_equal(got[:, keep], clean[:, keep]), f"{tag}: another channel moved"


# ---- input gradients that form the BatchNorm-backward sums in their epilogue ---------------------------------------------------------
def bnsum_rows_judged(stat, clean, da_ref64, z64, G, what, nan_channel=None, s1_by_conv=None):
    """stat [G, rows, 2, C]: (pass, channel) pairs whose dz holds a non-finite value have non-finite sums; every other pair keeps the
    clean run's rows to the bit; a channel whose scale is NaN shows the mask's convention in its exact sum of dz"""
    n, c = da_ref64.shape[:2]
    bad = (NF.classify(z64) != NF.FINITE).view(G, n // G, c, -1).any(3).any(1)          # (the rows sum dz = mask ? da : 0, not da)
    names = None
    for g in range(G):
        for ch in range(c):
            if ch == nan_channel:
                s = float(stat[g, :, 0, ch].double().sum())
                hit = [cv for cv in NF.CONVENTIONS if s == float(s1_by_conv[cv][g])]
                assert len(hit) == 1 and (names is None or names == hit), (what, g, s, {k: float(v[g]) for k, v in s1_by_conv.items()})
                names = hit
            elif bool(bad[g, ch]):
                assert not bool(torch.isfinite(stat[g, :, :, ch].double().sum(0)).any()), f"{what}: pass {g} channel {ch}: non-finite da, finite sums"
            else:
                assert bits_equal(stat[g, :, :, ch].clone(), clean[g, :, :, ch].clone()), f"{what}: rows of pass {g} channel {ch} differ from the clean run's"
    return names


BNSUM_CASES = [
    ("conv3x3 linear", "conv", 30, 2, 512, 32, 18, 18, variant("lin", 18, 128, 4, 1, False, False)),
    ("conv3x3 streaming", "conv", 8, 2, 64, 64, 60, 70, 0x57530600),
    ("convT 128-column", "convT", 8, 2, 128, 64, 64, 64, 0x43541000 | (128 // 32) << 8 | 2 << 4 | 1),
]


@pytest.mark.parametrize("case", BNSUM_CASES, ids=[c[0] for c in BNSUM_CASES])
def test_dgrad_bnsum_nonfinite(case):
    """ustrun_conv3x3_dgrad_bnsum / ustrun_convT2x2_dgrad_bnsum: +inf in the incoming gradient of the LAST pass (da per element against
    float64, rows per pass and channel), then a NaN scale in one channel (da untouched, the channel's rows show the mask's convention)"""
    name, kind, n, G, cin, cout, h, w, code = case
    l, lib = L(), L().lib()
    gn = n // G
    g_, ri = gen(len(name) * 23 + n)
    if kind == "conv":
        wt, dy = ri(-1, 1, cout, cin, 3, 3), ri(-1, 1, n, cout, h, w)
        ref = lambda d: F.conv_transpose2d(d, NF.stored(wt, ELT), None, 1, 1)
    else:
        wt, dy = ri(-1, 1, cin, cout, 2, 2), ri(-1, 1, n, cout, 2 * h, 2 * w)
        ref = lambda d: F.conv2d(d, NF.stored(wt, ELT), None, 2)
    y = ri(-3, 3, n, cin, h, w) * 0.5
    sc = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (G, cin), generator=g_)]
    sh = ri(-1, 1, G, cin) * 0.25
    sh[sh == 0] = 0.25
    if kind == "conv":
        nel = 9 * cin * cout
        wf, wd = torch.zeros(nel, dtype=T16, device="cuda"), torch.zeros(nel, dtype=T16, device="cuda")
        wg = wt.contiguous().cuda()
        l.check(lib.ustrun_pack_conv3x3(wg.data_ptr(), cout, cin, wf.data_ptr(), wd.data_ptr(), CODE, None))
    else:
        nel = 4 * cin * cout
        wf, wd = torch.zeros(nel, dtype=T16, device="cuda"), torch.zeros(nel, dtype=T16, device="cuda")
        wg = wt.contiguous().cuda()
        l.check(lib.ustrun_pack_convT2x2(wg.data_ptr(), cin, cout, wf.data_ptr(), wd.data_ptr(), CODE, None))
    yg = nhwc16(y, ELT)

    def call(dy_, sc_):
        aff = torch.zeros(G, 4, cin)
        aff[:, 0], aff[:, 1] = sc_, sh
        affg, dyg = aff.cuda(), nhwc16(dy_, ELT)
        db, da = guarded((n, h, w, cin), T16, 9.0)
        rows_max = lib.ustrun_conv_mtiles(n, h, w, cin)
        stat = torch.full((rows_max + 64, 2, cin), 5.0, device="cuda")
        rows = C.c_int(-1)
        fn = lib.ustrun_conv3x3_dgrad_bnsum if kind == "conv" else lib.ustrun_convT2x2_dgrad_bnsum
        l.check(fn(dyg.data_ptr(), wd.data_ptr(), n, h, w, cout, cin, da.data_ptr(), yg.data_ptr(), affg.data_ptr(), affg.data_ptr() + 4 * cin, gn, 4 * cin,
                   stat.data_ptr(), C.byref(rows), CODE, None), name)
        assert rows.value > 0 and rows.value % G == 0 and rows.value <= rows_max, rows.value
        assert lib.ustrun_debug_last_conv_variant() == code, hex(lib.ustrun_debug_last_conv_variant())
        assert whole(db, 9.0) and bool((stat[rows.value:] == 5.0).all()), f"{name}: wrote outside da or past the rows it reported"
        return from_nhwc(da.float()), stat[:rows.value].view(G, rows.value // G, 2, cin).cpu()

    da_clean, st_clean = call(dy, sc)
    NF.assert_matches(da_clean, ref(NF.stored(dy, ELT)), ELT, f"{name} clean")
    # +inf at the last pixel of the last image, -inf at a tile edge of the same pass
    dyp = dy.clone()
    dyp[n - 1, cout - 1, -1, -1], dyp[n - 1, 0, 7, 31 if dyp.shape[3] > 32 else 15] = INF, -INF
    da_ref = ref(NF.stored(dyp, ELT))
    da, st = call(dyp, sc)
    NF.assert_matches(da, da_ref, ELT, f"{name} inf gradient")
    assert bool((NF.classify(da_ref[:n - gn]) == NF.FINITE).all()) and bool((NF.classify(da_ref[n - gn:]) != NF.FINITE).any())
    e = lambda t: t.double().repeat_interleave(gn, 0)[:, :, None, None]
    z_ref = NF.relu_bwd(NF.stored(y, ELT) * e(sc) + e(sh), NF.stored(da_ref, ELT), "select")
    assert bool((NF.classify(z_ref[n - gn:]) != NF.FINITE).any()), "the mask removes every planted value: the case checks nothing"
    bnsum_rows_judged(st, st_clean, da_ref, z_ref, G, f"{name} inf gradient")
    # a NaN scale in channel 3 of every pass
    scn = sc.clone()
    scn[:, 3] = NAN
    da, st = call(dy, scn)
    assert torch.equal(da, da_clean), f"{name}: a BatchNorm constant changed da"
    da64 = ref(NF.stored(dy, ELT))
    s1 = {cv: NF.relu_bwd(NF.stored(y, ELT) * e(scn) + e(sh), NF.stored(da64, ELT), cv)[:, 3].reshape(G, -1).sum(1) for cv in NF.CONVENTIONS}
    assert all(float(a) != float(b) for a, b in zip(s1["torch"], s1["select"]))
    names = bnsum_rows_judged(st, st_clean, da64, da64, G, f"{name} nan scale", nan_channel=3, s1_by_conv=s1)
    print(f"NaN convention: {name} dgrad_bnsum backward mask: {names[0]}")


@pytest.mark.parametrize("cin,h,w", [(1, 19, 37), (3, 16, 32)])
def test_conv_first_wgrad_bn_nonfinite(cin, h, w):
    """ustrun_conv_first_wgrad_bn, the first layer's weight gradient as the step runs it (dY = apply(da, y) with the ReLU mask formed in
    the loader), N = 2 as two passes of one image.  Plants: inf in da, inf in y, an inf pixel of the image, a NaN scale.  dw is judged per
    channel line over in-range pixel pairs (tests/test_gpu_nonfinite_ops.py): a bad dY channel k0 may touch dw[k0] only, a bad image
    channel dw[:, c0] only."""
    l, lib = L(), L().lib()
    n, c = 2, 64
    for label, axis in (("clean", 0), ("da inf corner", 0), ("da -inf last pixel, second pass", 0), ("y inf", 0), ("image inf", 1), ("nan scale", 0)):
        g_, ri = gen(7 * cin + w)
        x = ri(-3, 3, n, cin, h, w)
        y, da, sc, sh, coef = apply_case(cin + h, n, 1, h, w, c)
        if label == "da inf corner":             # (y such that a >= 1: the mask passes the planted gradient)
            da[0, 0, 0, 0, 5], y[0, 0, 0, 0, 5] = INF, 2.0 * float(torch.sign(sc[0, 5]))
        elif label.startswith("da -inf"):
            da[1, 0, h - 1, w - 1, c - 1], y[1, 0, h - 1, w - 1, c - 1] = -INF, 2.0 * float(torch.sign(sc[1, c - 1]))
        elif label == "y inf":
            y[0, 0, 7, 15, 9] = INF * float(torch.sign(sc[0, 9]))
        elif label == "image inf":
            x[1, cin - 1, 8, 16] = INF
        elif label == "nan scale":
            sc[1, 11] = NAN
        xs = NF.stored(x, ELT)
        refs = {cv: wgrad_in_range(xs, apply_ref(NF.stored(y, ELT), NF.stored(da, ELT), sc, sh, coef, cv)[0][:, 0].permute(0, 3, 1, 2).contiguous())
                for cv in NF.CONVENTIONS}
        aff = torch.zeros(n, 4, c)
        aff[:, 0], aff[:, 1] = sc, sh
        affg, cg, xg = aff.cuda(), coef.contiguous().cuda(), x.contiguous().cuda()
        dag, yg = da.to(T16).cuda(), y.to(T16).cuda()
        src = l.nchw_src(xg.data_ptr(), cin, h, w)
        nb = lib.ustrun_wgrad_partials_bytes(9, cin, 64, n * h * w)
        part = torch.full((nb // 4 + 1024,), NAN, device="cuda")
        wb, dw = guarded((64, cin, 3, 3), torch.float32, NAN)
        l.check(lib.ustrun_conv_first_wgrad_bn(C.byref(src), dag.data_ptr(), yg.data_ptr(), affg.data_ptr(), affg.data_ptr() + 4 * c, cg.data_ptr(), 1, 4 * c,
                                               n, h, w, 64, dw.data_ptr(), 0, part.data_ptr(), nb, CODE, None))
        assert whole(wb, NAN) and bool(torch.isnan(part[nb // 4:]).all()), f"conv_first_wgrad_bn {label}: wrote outside dw or its slabs"
        res = {cv: weight_gradient_mismatches(dw, refs[cv], axis) for cv in NF.CONVENTIONS}
        names = [cv for cv in NF.CONVENTIONS if res[cv][:2] == (0, 0)]
        assert names, f"conv_first_wgrad_bn C={cin} {label}: {res['torch']}"
        if label == "clean":
            assert bool(torch.isfinite(dw).all())
        elif label == "nan scale":
            assert len(names) == 1
            print(f"NaN convention: conv_first_wgrad_bn C={cin} backward mask: {names[0]}")
        else:
            assert not bool(torch.isfinite(dw).all()), f"conv_first_wgrad_bn C={cin} {label}: the poison did not reach dw"


def test_seg_loss_bwd_infinite_device_scale():
    """ustrun_seg_loss_bwd reads the upstream gradients of its two outputs from a device state (gdev) and multiplies them into the
    class weights of its expression.  With (inf, 0) and (0, inf) in that state the class of every element is that of the same expression
    evaluated in float64 (step_tail_ref.seg_loss_bwd): +-inf by the cross-entropy term's sign for the first; for the second the softmax
    Jacobian l (G - sum G l) of an infinite G is inf - inf = NaN.  No element stays finite.  Logits, labels and masks stay clean."""
    import step_tail_ref as R
    l, lib = L(), L().lib()
    N, K, HW = 2, 2, 63
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.normal(size=(N, K, HW)).astype(np.float32)).cuda()
    t = torch.from_numpy(rng.integers(0, K, size=(N, HW))).cuda()           # int64 class indices: never poisoned
    nb = lib.ustrun_loss_partials_bytes(N, K, HW)
    out, part = torch.zeros(R.nsums(K), device="cuda"), torch.zeros(nb // 4, device="cuda")
    l.check(lib.ustrun_seg_loss_fwd(x.data_ptr(), t.data_ptr(), None, N, K, HW, R.SOFTMAX, out.data_ptr(), part.data_ptr(), nb, None))

    def bwd(g0, g1):
        gd = torch.tensor([g0, g1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], device="cuda")
        db, d = guarded((N, K, HW), torch.float32, 9.0)
        l.check(lib.ustrun_seg_loss_bwd(x.data_ptr(), t.data_ptr(), None, N, K, HW, R.SOFTMAX, out.data_ptr(), gd.data_ptr(), 1.0, 1.0, 1.0, d.data_ptr(), None))
        assert whole(db, 9.0)
        return d.cpu().clone()

    sums = out.cpu().numpy()
    for gd in ((INF, 0.0), (0.0, INF)):
        got = bwd(*gd)
        with np.errstate(all="ignore"):
            want = torch.from_numpy(R.seg_loss_bwd(x.cpu().numpy(), t.cpu().numpy(), None, R.SOFTMAX, sums, gd, 1.0, 1.0, 1.0))
        assert not bool(torch.isfinite(want).any()) and (gd[0] == 0.0 or not bool(torch.isnan(want).any()))
        assert torch.equal(NF.classify(got), NF.classify(want)), f"seg_loss_bwd, device scale {gd}: {int((NF.classify(got) != NF.classify(want)).sum())} classes differ"
