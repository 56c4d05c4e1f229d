"""The operators BETWEEN the convolutions, one C-ABI call at a time against the float64 references of tests/bn_ops_ref.py (pinned to torch
on the CPU by tests/test_bn_ops_ref_host.py): ustrun_bn_finalize on synthetic statistics tables (direct and staged reduction, every row
split), ustrun_bn_eval_affine, ustrun_bn_relu_apply, ustrun_act16, ustrun_pool_act / _pool_act2, ustrun_maxpool_bwd and the four
ustrun_upsample2x_* passes.  Every output tensor lies between two 4096-element guard zones which must come back untouched.

Bounds on |got - ref| (ref: float64 on the SAME stored inputs), derived, not tuned:
  constants      2^-22 |v| (f64 reduction: one f32 rounding plus slack); shift: 2^-22 (|beta| + |mean scale|)
  f32 element    2^-22 (|y s| + |b|): one product and one sum rounded (2^-24 each of at most |y s| + |b|), twice over
  pooled         max is 1-Lipschitz in the sup norm: the largest of the window's four elementwise bounds
  16-bit output  the f32 bound plus HALF AN ULP of the storage type at the reference value.  For a value in [2^e, 2^(e+1)) that is
                 2^(e-8) (bf16, 8 significand bits) or 2^(e-11) (f16, 11 bits; 2^-25 in its subnormal range): between 2^-9 |ref| and
                 2^-8 |ref| (2^-12 .. 2^-11 for f16).  It equals 2^-9 |ref| only at the top of a binade; round-to-nearest itself
                 reaches 2^(e-8) just above 2^e, so the half ulp is taken exactly (HALF_ULP below), not as 2^-9 |ref|.
  upsample       forward 4 x 2^-24 x (largest |a| of the four taps): two inner and two outer roundings of a convex combination; adjoint
                 16 x 2^-24 x A, A = the f64 adjoint of |dy| (at most 6 + 6 products and sums per output, two per step).
                 Plus the COORDINATE term: the kernels evaluate src = o (in - 1) / (2 in - 1) in float32, scale first, as ATen does
                 for float tensors (csrc/upsample.hip): the quotient and the product are rounded once each, |d src| <= 2^-23 src, and a
                 weight moves by as much.  A forward output moves by at most (dsrc_y + dsrc_x) x (the largest difference of two
                 neighbours <= 2 max |a| of the image's channel plane; the plane, not the taps: at an integer src the f32 value may fall
                 just below it and read the neighbour before with a weight of ~1e-7).  An adjoint output moves by at most the sum of
                 (dsrc_y(o) + dsrc_x(p)) |dy(o, p)| over the closed support |src - i| <= 1 of its weights.
A ReLU whose float64 pre-activation lies within the f32 bound of zero cannot exceed these bounds (max(., 0) is 1-Lipschitz): no
element is excluded anywhere.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import bn_ops_ref as R

pytestmark = pytest.mark.gpu

DT = {"f32": (0, torch.float32), "f32x3": (3, torch.float32), "bf16": (1, torch.bfloat16), "f16": (2, torch.float16)}
GUARD, SENT = 4096, 7.0
E32 = 2.0 ** -22


def L():
    from ustrun import _lib
    return _lib


class Out:
    """An output tensor between two guard zones; the tensor itself starts out as the sentinel too, so an element the kernel skips shows."""

    def __init__(self, shape, tdt=torch.float32, init=None):
        n = int(np.prod(shape))
        self.buf = torch.full((GUARD + n + GUARD,), SENT if tdt.is_floating_point else int(SENT), device="cuda", dtype=tdt)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        if init is not None:
            self.t.copy_(torch.as_tensor(init).to(tdt).reshape(*shape))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_ok(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[-GUARD:] == SENT).all())

    def get(self):
        assert self.guards_ok(), "a guard zone was written"
        return self.t.double().cpu().numpy()


def stored(a, tdt=torch.float32):
    """a (numpy) rounded once to the storage type: (device tensor, the stored values in float64)"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(tdt)
    return t.cuda(), t.double().numpy()


def half_ulp(ref, name):
    """HALF_ULP of the header: half the spacing of the storage type at |ref| (0 for the f32 types: their rounding is in the f32 bound)."""
    if name in ("f32", "f32x3"):
        return np.zeros_like(ref)
    _, e = np.frexp(np.abs(ref))                  # |ref| = m 2^e, m in [0.5, 1): |ref| in [2^(e-1), 2^e)
    if name == "bf16":
        return np.where(ref == 0, 0.0, np.ldexp(1.0, e - 1 - 8))
    return np.maximum(np.where(ref == 0, 0.0, np.ldexp(1.0, e - 1 - 11)), 2.0 ** -25)


def hold(what, got, ref, bound):
    """|got - ref| <= bound everywhere; prints the worst error / bound ratio first (pytest -s), names the worst element when it fails."""
    got, ref, bound = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)                         # (a NaN fails)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    i = np.unravel_index(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)), ratio.shape) if ratio.size else ()
    print(f"{what}: worst err/bound {ratio[i] if ratio.size else 0:.3g} at {i}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} past the bound; worst at {i}: got {got[i]!r} ref {ref[i]!r} bound {bound[i]!r}"


def table(rng, C, groups, gstride):
    """scale / shift tables of `groups` passes gstride floats apart, different in every pass, NaN between the passes' rows"""
    n = (groups - 1) * gstride + C
    s, b = np.full(n, np.nan), np.full(n, np.nan)
    for g in range(groups):
        s[g * gstride:g * gstride + C] = (0.05 + np.abs(rng.normal(size=C))) * rng.choice([-1.0, 1.0], size=C, p=[0.3, 0.7])
        b[g * gstride:g * gstride + C] = rng.normal(size=C) * 0.5
    return s, b


# ---- ustrun_bn_finalize ---------------------------------------------------------------------------------------------------------------
# bn_finalize_passes (csrc/bn.hip): staged (in-place stage 1, then bn_finalize_kernel<true>) when mtiles >= 96 and C % 32 == 0, with
# R = ceil(mtiles / 32) raised until mtiles % R != 1; else bn_finalize_kernel<false> sums the rows directly.  The C ABI passes no ticket
# table, so the staged form is always the two-launch one.
FINALIZE_CASES = [
    (1, 8),        # direct: one row, a quarter of one 32-channel block
    (7, 24),       # direct (C % 32 != 0): fewer rows than the eight row lanes, ragged channel block
    (95, 64),      # direct: the last size below the staged threshold, two channel blocks
    (96, 32),      # staged: R = 3 (96 % 3 = 0), 32 splits
    (97, 64),      # staged: R = ceil(97 / 32) = 4, 97 % 4 = 1 -> R = 5 (97 % 5 = 2), 20 splits, the last of two rows
    (129, 96),     # staged: R = 5 (129 % 5 = 4), 26 splits, three channel blocks
    (1025, 64),    # staged: R = 33 (1025 % 33 = 2), 32 splits, the last of two rows
    (2049, 32),    # staged: R = 65 (2049 % 65 = 34), 32 splits; stage 1's four-rows-per-trip loop and its remainder
]
HI, G0, GNEG = 0, 2, 3            # channels: |mean| / std = 1e3; gamma = 0; gamma < 0; the constant channel is the last one


def finalize_case(mtiles, C):
    """A synthetic statistics table: y[count, C] in f64, its rows split into mtiles ragged chunks, each chunk's sum and sum of squares
    rounded once to float32."""
    rng = np.random.default_rng(1000 * mtiles + C)
    sizes = rng.integers(2, 6, size=mtiles) + (0 if mtiles >= 32 else 30)       # (few rows: longer chunks, so that the 1e3 channel keeps a variance)
    count = int(sizes.sum())
    y = rng.normal(size=(count, C)) * rng.uniform(0.5, 2.0, C) + rng.normal(size=C)
    y[:, HI] = 1e3 + rng.normal(size=count)
    edges = np.concatenate([[0], np.cumsum(sizes)])

    def tab(y):
        return np.stack([np.stack([y[a:b].sum(0), (y[a:b] ** 2).sum(0)]) for a, b in zip(edges[:-1], edges[1:])]).astype(np.float32)

    # the constant channel: the first value of a fixed list whose float32 table gives sum2 / count - mean^2 clearly below zero
    for v in 1.1 + 0.1 * np.arange(60):
        y[:, C - 1] = v
        stat = tab(y)
        if R.raw_variance(stat, count)[C - 1] < -1e-10 * v * v:
            break
    gamma, beta = rng.normal(size=C), rng.normal(size=C)
    gamma[G0], gamma[GNEG] = 0.0, -1.5
    rm, rv = rng.normal(size=C), rng.uniform(0.5, 2.0, C)
    f32 = lambda a: a.astype(np.float32)
    return stat, count, f32(gamma), f32(beta), f32(rm), f32(rv)


@pytest.mark.parametrize("mtiles,C", FINALIZE_CASES)
def test_bn_finalize_direct_and_staged(mtiles, C):
    l = L()
    lib = l.lib()
    stat, count, gamma, beta, rm, rv = finalize_case(mtiles, C)
    raw = R.raw_variance(stat, count)
    assert raw[C - 1] < 0 and raw[HI] > 0.1, (raw[C - 1], raw[HI])         # the clamp is exercised; the 1e3 channel is well conditioned
    eps = 1e-5
    gg, bg = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
    for update, momentum in ((0, 0.1), (1, 0.1), (1, 1.0)):
        ref = R.finalize(stat, count, gamma, beta, rm, rv, momentum, eps)
        assert ref.rstd[C - 1] == 1.0 / np.sqrt(float(np.float32(eps)))
        st = Out(stat.shape, init=stat)               # a fresh table (the call may overwrite it), guarded: stage 1 parks its sums IN it
        o = {k: Out((C,)) for k in ("scale", "shift", "mean", "rstd")}
        orm, orv, nbt = Out((C,), init=rm), Out((C,), init=rv), Out((1,), torch.int64, init=[5])
        l.check(lib.ustrun_bn_finalize(st.ptr, mtiles, C, count, gg.data_ptr(), bg.data_ptr(), orm.ptr, orv.ptr, nbt.ptr, momentum,
                                       eps, update, o["scale"].ptr, o["shift"].ptr, o["mean"].ptr, o["rstd"].ptr, None))
        tag = f"finalize({mtiles},{C}) update={update} momentum={momentum}"
        for k in ("scale", "mean", "rstd"):
            hold(f"{tag} {k}", o[k].get(), getattr(ref, k), E32 * np.abs(getattr(ref, k)))
        hold(f"{tag} shift", o["shift"].get(), ref.shift, E32 * (np.abs(beta.astype(np.float64)) + np.abs(ref.mean * ref.scale)))
        assert o["scale"].get()[G0] == 0.0 and o["shift"].get()[G0] == float(beta[G0]) and o["scale"].get()[GNEG] < 0
        assert st.guards_ok() and orm.guards_ok() and orv.guards_ok() and nbt.guards_ok()
        if update:
            hold(f"{tag} running_mean", orm.get(), ref.running_mean, E32 * np.abs(ref.running_mean))
            hold(f"{tag} running_var", orv.get(), ref.running_var, E32 * np.abs(ref.running_var))
            assert int(nbt.t.item()) == 6
        else:
            assert torch.equal(orm.t.cpu(), torch.from_numpy(rm)) and torch.equal(orv.t.cpu(), torch.from_numpy(rv))
            assert int(nbt.t.item()) == 5


@pytest.mark.parametrize("C", [1, 24, 2048])
def test_bn_eval_affine(C):
    l = L()
    rng = np.random.default_rng(C)
    f32 = lambda a: a.astype(np.float32)
    gamma, beta, rm, rv = f32(rng.normal(size=C)), f32(rng.normal(size=C)), f32(rng.normal(size=C)), f32(rng.uniform(0.05, 2.0, C))
    rv[C // 2] = 0.0
    dev = [torch.from_numpy(a).cuda() for a in (gamma, beta, rm, rv)]
    sc, sh = Out((C,)), Out((C,))
    l.check(l.lib().ustrun_bn_eval_affine(C, *[t.data_ptr() for t in dev], 1e-5, sc.ptr, sh.ptr, None))
    rs, rb = R.eval_affine(gamma, beta, rm, rv, 1e-5)
    hold(f"eval_affine({C}) scale", sc.get(), rs, E32 * np.abs(rs))
    hold(f"eval_affine({C}) shift", sh.get(), rb, E32 * (np.abs(beta.astype(np.float64)) + np.abs(rm.astype(np.float64) * rs)))


# ---- ustrun_bn_relu_apply -------------------------------------------------------------------------------------------------------------
def relu_apply_check(name, n, c, h, w, nchw, seed):
    l = L()
    dt, tdt = DT[name]
    g = torch.Generator().manual_seed(seed)
    yg = torch.randn(n, h, w, c, generator=g).to(tdt).cuda()
    y = yg.double().cpu().numpy()
    rng = np.random.default_rng(seed)
    s, b = table(rng, c, 1, c)
    (sg, s), (bg, b) = stored(s), stored(b)
    shape = (n, c, h, w) if nchw else (n, h, w, c)
    lay = (lambda a: a.transpose(0, 3, 1, 2)) if nchw else (lambda a: a)
    for aff in (True, False):
        out = Out(shape)
        l.check(l.lib().ustrun_bn_relu_apply(yg.data_ptr(), sg.data_ptr() if aff else None, bg.data_ptr() if aff else None, n * h * w, c, h * w,
                                             out.ptr, int(nchw), dt, None))
        tag = f"bn_relu_apply {name} {(n, c, h, w)} nchw={nchw} affine={aff}"
        if aff:
            hold(tag, out.get(), lay(R.act(y, s, b, relu=True)), lay(E32 * R.act_magnitude(y, s, b)))
        else:                                          # scale = NULL: a copy, no ReLU, exact
            got = out.get()
            assert np.array_equal(got, lay(y)) and (y.size < 100 or (got < 0).any()), tag


@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("name", ["f32", "bf16", "f16", "f32x3"])
@pytest.mark.parametrize("n,c,h,w", [(1, 3, 1, 1), (2, 24, 5, 7), (3, 64, 9, 4), (2, 64, 136, 136)])
def test_bn_relu_apply(n, c, h, w, name, nchw):
    """(2, 64, 136, 136): 2.4 M elements, 2312 blocks of 256 threads -- the grid-stride loop goes round four times."""
    relu_apply_check(name, n, c, h, w, nchw, seed=c + h)


def test_bn_relu_apply_past_the_block_cap():
    """8.65 M elements ask for 8450 blocks: the launcher caps the grid at 8192, and the grid-stride loop covers the rest in a fifth trip."""
    relu_apply_check("bf16", 2, 64, 260, 260, True, seed=9)


# ---- ustrun_act16 ---------------------------------------------------------------------------------------------------------------------
# 256 / (C / 8) pixels per block, eight per thread and trip: extents giving more than one block and a ragged last one
ACT16_EXTENT = {8: (23, 29), 24: (13, 17), 96: (7, 9), 512: (5, 7), 2048: (5, 7)}


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("c", [8, 24, 96, 512, 2048])
@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_act16(name, c, relu):
    l = L()
    dt, tdt = DT[name]
    rng = np.random.default_rng(c + relu)
    for n, (h, w), gN in ((1, (1, 1), 0), (4, ACT16_EXTENT[c], 2)):
        groups, gstride = (2, c + 32) if gN else (1, c)
        s, b = table(rng, c, groups, gstride)
        (sg, s), (bg, b) = stored(s), stored(b)
        yg, y = stored(rng.normal(size=(n, h, w, c)), tdt)
        src = l.nhwc_src(yg.data_ptr(), c, h, w, sg.data_ptr(), bg.data_ptr(), relu=relu, gN=gN, gstride=gstride if gN else 0)
        out = Out((n, h, w, c), tdt)
        l.check(l.lib().ustrun_act16(C.byref(src), n, out.ptr, dt, None))
        ref = R.act(y, s, b, relu=bool(relu), gN=gN, gstride=gstride)
        if gN:      # the passes' constants differ: group 0's constants on a group-1 image are far outside the bound
            assert np.abs(ref[2:] - R.act(y, s, b, relu=bool(relu))[2:]).max() > 0.1
        hold(f"act16 {name} C={c} relu={relu} n={n}", out.get(), ref,
             E32 * R.act_magnitude(y, s, b, gN=gN, gstride=gstride) + half_ulp(ref, name))


# ---- ustrun_pool_act / ustrun_pool_act2 -----------------------------------------------------------------------------------------------
def pool_bound(y, s, b, gN, gstride, ref, name):
    return E32 * R.pool2(R.act_magnitude(y, s, b, gN=gN, gstride=gstride)) + half_ulp(ref, name)


# 16-bit storage moves eight channels per lane, the f32 types four: C = 4 exists for those only
@pytest.mark.parametrize("name,c", [(t, c) for t in ("f32", "f32x3", "bf16", "f16") for c in (4, 8, 24, 96, 1024) if c % 8 == 0 or t[:3] == "f32"])
def test_pool_act(name, c):
    l = L()
    lib = l.lib()
    dt, tdt = DT[name]
    wide = tdt != torch.float32
    rng = np.random.default_rng(c + dt)
    n, gN, gstride = 4, 2, c + 32
    zero_windows = order_matters = 0
    for h, w in [(4, 6), (5, 7), (2, 3), (2, 2)] + ([(34, 38)] if c <= 24 else []):       # (34, 38): more than one block at few channels
        s, b = table(rng, c, 2, gstride)
        (sg, s), (bg, b) = stored(s), stored(b)
        y = rng.normal(size=(n, h, w, c))
        sel = np.arange(c) % 3 != 1                    # window (0, 0) of every image, two channels in three: a = -1 at all four pixels
        for i in range(n):
            o = (i // gN) * gstride
            y[i, :2, :2][:, :, sel] = ((-1.0 - b[o:o + c]) / s[o:o + c])[sel]
        yg, y = stored(y, tdt)
        for aff, relu in ((False, 0), (True, 0), (True, 1)):
            src = l.nhwc_src(yg.data_ptr(), c, h, w, sg.data_ptr() if aff else None, bg.data_ptr() if aff else None, relu=relu, gN=gN,
                             gstride=gstride)
            out = Out((n, h // 2, w // 2, c), tdt)
            l.check(lib.ustrun_pool_act(C.byref(src), n, out.ptr, dt, None))
            a = R.act(y, s if aff else None, b if aff else None, relu=bool(relu), gN=gN, gstride=gstride)
            ref = R.pool2(a)
            tag = f"pool_act {name} C={c} {h}x{w} affine={aff} relu={relu}"
            got = out.get()
            if not aff:
                assert np.array_equal(got, ref), tag                              # a plain maximum of stored values: exact
            else:
                hold(tag, got, ref, pool_bound(y, s, b, gN, gstride, ref, name))
            if aff and not relu:     # negative scales: the maximum of the activations is not the activation of the maximum
                order_matters += int((np.abs(ref - R.act(R.pool2(y), s, b, gN=gN, gstride=gstride)) > 0.1).any())
            if relu:
                z = (ref[:, 0, 0, sel] == 0).all()
                assert z, tag
                zero_windows += int(z)
                assert (got[:, 0, 0, sel] == 0).all(), tag
            if wide and h % 2 == 0 and w % 2 == 0:
                out2, act = Out((n, h // 2, w // 2, c), tdt), Out((n, h, w, c), tdt)
                l.check(lib.ustrun_pool_act2(C.byref(src), n, out2.ptr, act.ptr, dt, None))
                ga, gp = act.get(), out2.get()
                if aff:
                    hold(tag + " act", ga, a, E32 * R.act_magnitude(y, s, b, gN=gN, gstride=gstride) + half_ulp(a, name))
                else:
                    assert np.array_equal(ga, a), tag
                assert np.array_equal(gp, got), tag                               # the same pooled tensor with and without `act`
                assert np.array_equal(gp, R.pool2(ga)), tag                       # rounding is monotone: round-then-max == max-then-round
    assert zero_windows > 0 and order_matters > 0


def test_pool_act2_refuses_odd_extents_and_f32():
    l = L()
    lib = l.lib()
    y = torch.zeros(1, 5, 6, 8, device="cuda", dtype=torch.bfloat16)
    out, act = Out((1, 2, 3, 8), torch.bfloat16), Out((1, 5, 6, 8), torch.bfloat16)
    src = l.nhwc_src(y.data_ptr(), 8, 5, 6)
    assert lib.ustrun_pool_act2(C.byref(src), 1, out.ptr, act.ptr, 1, None) != 0
    assert b"16-bit storage and even extents" in lib.ustrun_last_error()
    yf = torch.zeros(1, 4, 6, 8, device="cuda")
    outf, actf = Out((1, 2, 3, 8)), Out((1, 4, 6, 8))
    src = l.nhwc_src(yf.data_ptr(), 8, 4, 6)
    for dt in (0, 3):
        assert lib.ustrun_pool_act2(C.byref(src), 1, outf.ptr, actf.ptr, dt, None) != 0
        assert b"16-bit storage and even extents" in lib.ustrun_last_error()
    torch.cuda.synchronize()
    for o in (out, act, outf, actf):
        assert o.guards_ok() and bool((o.t == SENT).all())                       # refused before any launch


# ---- ustrun_maxpool_bwd ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 8, 24])
@pytest.mark.parametrize("name", ["f32", "f32x3", "bf16", "f16"])
def test_maxpool_bwd_routes_to_the_first_maximum(name, c):
    l = L()
    dt, tdt = DT[name]
    rng = np.random.default_rng(c + dt)
    n = 3
    windows = tied = 0
    winners = set()
    for h, w in ((6, 8), (5, 7), (2, 3), (2, 2)):
        xg, x = stored(rng.choice(np.array([-1.0, 0.0, 0.5, 2.0]), size=(n, h, w, c)), tdt)      # a four-value alphabet: ties everywhere
        dpg, dp = stored(rng.normal(size=(n, h // 2, w // 2, c)), tdt)
        dx = Out((n, h, w, c), tdt)
        l.check(l.lib().ustrun_maxpool_bwd(dpg.data_ptr(), xg.data_ptr(), n, h, w, c, dx.ptr, dt, None))
        ref, best = R.maxpool_route(dp, x)
        win = R._windows(x)
        tied += int(((win == win.max(axis=3, keepdims=True)).sum(axis=3) > 1).sum())
        windows += best.size
        winners |= set(np.unique(best).tolist())
        assert dx.guards_ok()
        # every output is a copy of a dp element or +0: bit for bit
        want = torch.from_numpy(ref).to(tdt)
        bits = torch.int32 if tdt == torch.float32 else torch.int16
        assert torch.equal(dx.t.cpu().view(bits), want.view(bits)), f"maxpool_bwd {name} C={c} {h}x{w}"
    assert tied >= 0.25 * windows and winners == {0, 1, 2, 3}, (tied, windows, winners)


# ---- ustrun_upsample2x_fwd / _bwd / _act / _bwd_t -------------------------------------------------------------------------------------
def coord_err(k):
    """|d src| of each of the 2k outputs: the f32 quotient and the f32 product, 2^-24 of src each (header)"""
    return 2.0 ** -23 * R.src_coord(k)


def tap_max(a):
    """largest |a| of the four taps of every output"""
    a = np.abs(a)
    H, W = a.shape[1], a.shape[2]
    iy0 = np.minimum(np.floor(R.src_coord(H)).astype(int), H - 1)
    ix0 = np.minimum(np.floor(R.src_coord(W)).astype(int), W - 1)
    iy1, ix1 = np.minimum(iy0 + 1, H - 1), np.minimum(ix0 + 1, W - 1)
    m = None
    for iy in (iy0, iy1):
        for ix in (ix0, ix1):
            t = a[:, iy][:, :, ix]
            m = t if m is None else np.maximum(m, t)
    return m


def fwd_bound(a, mag, ref, name, coord_term=True):
    """a: the (activated) f64 source; mag: act_magnitude of the source (its f32 evaluation error / 2^-22, interpolated with the same
    convex weights)"""
    H, W = a.shape[1], a.shape[2]
    plane = np.abs(a).max(axis=(1, 2), keepdims=True)
    coord = (coord_err(H)[None, :, None, None] + coord_err(W)[None, None, :, None]) * 2.0 * plane
    return 4 * 2.0 ** -24 * tap_max(a) + (coord if coord_term else 0.0) + E32 * R.upsample2x(mag) + half_ulp(ref, name)


def bwd_bound(dy, ref, name, coord_term=True):
    H, W = dy.shape[1] // 2, dy.shape[2] // 2
    ady = np.abs(dy)
    Ty, Tx = R.touch_matrix(H), R.touch_matrix(W)
    coord = (R.upsample2x_adjoint(ady, Ty * coord_err(H)[:, None], Tx) + R.upsample2x_adjoint(ady, Ty, Tx * coord_err(W)[:, None]))
    return 16 * 2.0 ** -24 * R.upsample2x_adjoint(ady) + (coord if coord_term else 0.0) + half_ulp(ref, name)


UPSAMPLE_SHAPES = [(1, 4, 1, 1), (1, 4, 1, 3), (2, 8, 3, 1), (2, 12, 5, 7), (3, 64, 16, 16)]


@pytest.mark.parametrize("name", ["f32", "f32x3", "bf16", "f16"])
@pytest.mark.parametrize("n,c,h,w", UPSAMPLE_SHAPES)
def test_upsample2x(n, c, h, w, name):
    l = L()
    lib = l.lib()
    dt, tdt = DT[name]
    rng = np.random.default_rng(31 * h + w + dt)
    xg, x = stored(rng.normal(size=(n, h, w, c)), tdt)
    dyg, dy = stored(rng.normal(size=(n, 2 * h, 2 * w, c)), tdt)
    zero = np.zeros_like(x)
    tag = f"upsample2x {name} {(n, c, h, w)}"

    # forward, no constants
    ref = R.upsample2x(x)
    yb = fwd_bound(x, zero, ref, name)
    out = Out((n, 2 * h, 2 * w, c), tdt)
    src = l.nhwc_src(xg.data_ptr(), c, h, w)
    l.check(lib.ustrun_upsample2x_act(C.byref(src), n, out.ptr, dt, None))
    y_dev = out.get()
    hold(tag + " act plain", y_dev, ref, yb)
    with np.errstate(divide="ignore", invalid="ignore"):      # (a figure, not a check: how far the coordinate term is needed)
        print(f"{tag} act plain without the coordinate term: {np.nanmax(np.abs(y_dev - ref) / fwd_bound(x, zero, ref, name, False)):.3g}")
    if h == 1:
        assert np.array_equal(y_dev[:, 0], y_dev[:, 1])                           # one input row: both output rows are it

    # forward through BatchNorm constants + ReLU, per-pass constants (n = 1: one pass; n = 2: two passes of one; n = 3: passes of 2 and 1)
    gN = 1 if n < 3 else 2
    groups, gstride = (n - 1) // gN + 1, c + 32
    s, b = table(rng, c, groups, gstride)
    (sg, s), (bg, b) = stored(s), stored(b)
    src = l.nhwc_src(xg.data_ptr(), c, h, w, sg.data_ptr(), bg.data_ptr(), relu=1, gN=gN, gstride=gstride)
    out = Out((n, 2 * h, 2 * w, c), tdt)
    l.check(lib.ustrun_upsample2x_act(C.byref(src), n, out.ptr, dt, None))
    a = R.act(x, s, b, relu=True, gN=gN, gstride=gstride)
    ref_a = R.upsample2x(a)
    hold(tag + " act bn+relu", out.get(), ref_a, fwd_bound(a, R.act_magnitude(x, s, b, gN=gN, gstride=gstride), ref_a, name))

    # adjoint: twice into the same buffer, bit-identical (fixed order, nothing accumulated into what is there)
    dref = R.upsample2x_adjoint(dy)
    db = bwd_bound(dy, dref, name)
    dx = Out((n, h, w, c), tdt)
    l.check(lib.ustrun_upsample2x_bwd_t(dyg.data_ptr(), n, h, w, c, dx.ptr, dt, None))
    first = dx.t.clone()
    l.check(lib.ustrun_upsample2x_bwd_t(dyg.data_ptr(), n, h, w, c, dx.ptr, dt, None))
    bits = torch.int32 if tdt == torch.float32 else torch.int16
    assert torch.equal(first.view(bits), dx.t.view(bits)), tag
    dx_dev = dx.get()
    hold(tag + " bwd_t", dx_dev, dref, db)
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"{tag} bwd_t without the coordinate term: {np.nanmax(np.abs(dx_dev - dref) / bwd_bound(dy, dref, name, False)):.3g}")

    # <U x, dy> == <x, U^T dy> on the device outputs, to the bounds the two sides were held to
    lhs, rhs = float((y_dev * dy).sum()), float((x * dx_dev).sum())
    assert abs(lhs - rhs) <= float((yb * np.abs(dy)).sum() + (np.abs(x) * db).sum()), (tag, lhs, rhs)

    if name == "f32":        # the stand-alone f32 pair (the bilinear Up block)
        out = Out((n, 2 * h, 2 * w, c))
        l.check(lib.ustrun_upsample2x_fwd(xg.data_ptr(), n, h, w, c, out.ptr, None))
        yf = out.get()
        hold(tag + " fwd", yf, ref, yb)
        dx = Out((n, h, w, c))
        l.check(lib.ustrun_upsample2x_bwd(dyg.data_ptr(), n, h, w, c, dx.ptr, None))
        first = dx.t.clone()
        l.check(lib.ustrun_upsample2x_bwd(dyg.data_ptr(), n, h, w, c, dx.ptr, None))
        assert torch.equal(first.view(bits), dx.t.view(bits)), tag
        dxf = dx.get()
        hold(tag + " bwd", dxf, dref, db)
        lhs, rhs = float((yf * dy).sum()), float((x * dxf).sum())
        assert abs(lhs - rhs) <= float((yb * np.abs(dy)).sum() + (np.abs(x) * db).sum()), (tag, lhs, rhs)


# ---- documented refusals --------------------------------------------------------------------------------------------------------------
def test_documented_refusals():
    """Every USTRUN_CHECK these operators document returns nonzero with its message, before anything is launched."""
    l = L()
    lib = l.lib()
    n, h, w = 1, 4, 6
    x16 = torch.zeros(n * h * w * 16, device="cuda", dtype=torch.bfloat16)
    x32 = torch.zeros(n * h * w * 16, device="cuda")
    const = torch.ones(64, device="cuda")
    o16, o32 = Out((4 * n * h * w * 16,), torch.bfloat16), Out((4 * n * h * w * 16,))
    cp = const.data_ptr()

    def refused(rc, text):
        assert rc != 0, text
        assert text.encode() in lib.ustrun_last_error(), (text, lib.ustrun_last_error())

    def src16(c=8, hh=h, ww=w, scale=cp, shift=cp, **kw):
        return l.nhwc_src(x16.data_ptr(), c, hh, ww, scale, shift, **kw)

    def strided(s):
        s.sW += 8
        return s

    # act16: C % 8, f32 storage, missing constants, strided / pooled / offset / f32 sources
    refused(lib.ustrun_act16(C.byref(src16(c=12)), n, o16.ptr, 1, None), "act16: C=12 unsupported")
    refused(lib.ustrun_act16(C.byref(src16()), n, o16.ptr, 0, None), "act16: 16-bit storage only")
    refused(lib.ustrun_act16(C.byref(src16(scale=None, shift=None)), n, o16.ptr, 1, None), "act16: bad args")
    refused(lib.ustrun_act16(C.byref(src16(shift=None)), n, o16.ptr, 1, None), "act16: bad args")
    for bad in (strided(src16()), src16(pool=1), src16(off=(1, 0)), src16(off=(0, 1)), src16(f32=1)):
        refused(lib.ustrun_act16(C.byref(bad), n, o16.ptr, 1, None), "act16: source must be a plain contiguous NHWC activation")
        refused(lib.ustrun_pool_act(C.byref(bad), n, o16.ptr, 1, None), "pool_act: source must be a plain contiguous NHWC activation")
        refused(lib.ustrun_upsample2x_act(C.byref(bad), n, o16.ptr, 1, None), "upsample2x_act: source must be a plain contiguous NHWC tensor")
    # pool_act: H < 2, W < 2, channel vector, a lone scale or shift
    refused(lib.ustrun_pool_act(C.byref(src16(hh=1)), n, o16.ptr, 1, None), "pool_act: C=8 extent 1x6 unsupported")
    refused(lib.ustrun_pool_act(C.byref(src16(ww=1)), n, o16.ptr, 1, None), "pool_act: C=8 extent 4x1 unsupported")
    refused(lib.ustrun_pool_act(C.byref(src16(c=12)), n, o16.ptr, 1, None), "pool_act: C=12")
    refused(lib.ustrun_pool_act(C.byref(l.nhwc_src(x32.data_ptr(), 6, h, w)), n, o32.ptr, 0, None), "pool_act: C=6")
    refused(lib.ustrun_pool_act(C.byref(src16(shift=None)), n, o16.ptr, 1, None), "pool_act: scale/shift must come together")
    refused(lib.ustrun_pool_act(C.byref(src16(scale=None)), n, o16.ptr, 1, None), "pool_act: scale/shift must come together")
    # maxpool_bwd: H < 2, W < 2
    refused(lib.ustrun_maxpool_bwd(x32.data_ptr(), x32.data_ptr(), n, 1, w, 4, o32.ptr, 0, None), "maxpool_bwd: bad args")
    refused(lib.ustrun_maxpool_bwd(x16.data_ptr(), x16.data_ptr(), n, h, 1, 8, o16.ptr, 1, None), "maxpool_bwd: bad args")
    # upsample: C % 4 in all four passes, a lone scale
    refused(lib.ustrun_upsample2x_fwd(x32.data_ptr(), n, h, w, 6, o32.ptr, None), "upsample2x_fwd: bad shape (C=6 must be a multiple of 4)")
    refused(lib.ustrun_upsample2x_bwd(x32.data_ptr(), n, h, w, 6, o32.ptr, None), "upsample2x_bwd: bad shape (C=6 must be a multiple of 4)")
    refused(lib.ustrun_upsample2x_bwd_t(x16.data_ptr(), n, h, w, 6, o16.ptr, 1, None), "upsample2x_bwd_t: bad args (C=6 must be a multiple of 4)")
    refused(lib.ustrun_upsample2x_act(C.byref(src16(c=6, scale=None, shift=None)), n, o16.ptr, 1, None), "upsample2x_act: C=6 / constants")
    refused(lib.ustrun_upsample2x_act(C.byref(src16(shift=None)), n, o16.ptr, 1, None), "upsample2x_act: C=8 / constants")
    torch.cuda.synchronize()
    for o in (o16, o32):
        assert o.guards_ok() and bool((o.t == SENT).all())
