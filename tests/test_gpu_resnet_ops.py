"""DeepLabV2's operators BETWEEN the convolutions (csrc/resnet_ops.hip), one C-ABI call at a time against the float64 references of
tests/resnet_ops_ref.py (pinned to torch on the CPU by tests/test_resnet_ops_ref_host.py): ustrun_maxpool3x3s2, _bn_add_relu,
_sum_resize_bilinear, _aspp_gather, _rowwin_patches, _space_to_batch forward; _relu_bwd_add, _maxpool3x3s2_bwd, _sum_resize_bilinear_bwd,
_aspp_scatter, _colsum backward.  Conventions of test_gpu_bn_forward_ops.py: every output tensor lies between two
4096-element guard zones and starts out as the sentinel itself; references are float64 on the SAME stored inputs; bounds are
element-wise, no element is ever excluded; every storage type the entry takes.

Every kernel here is a grid-stride loop whose launcher caps the grid at 4096 blocks of 256 threads; the *_past_the_grid_cap cases have
more than 1 048 576 work items and no multiple of it, so that some threads go round twice and others once.

BIT FOR BIT (no tolerance): relu_bwd_add (an f32 sum of two stored values, rounded once to the storage type: exact in f32 whenever the
exponents of two 16-bit operands differ by less than 13, and where they differ by more the small operand is below a quarter ulp of the
result in either order of rounding), aspp_scatter, rowwin_patches, space_to_batch without constants (copies and zeros),
maxpool3x3s2_bwd (activations from an alphabet exact in every type, gradients multiples of 1/4 in [-4, 4]: any sum of four is exact).

BOUNDS on |got - ref|, derived from the kernels' expressions on their uncontracted form, one rounding of 2^-24 per f32 operation (a
fused multiply-add only drops a rounding); u = 2^-24:
  bn_add_relu      v = y s + b (2 roundings), r = i is + ib (2), v + r (1): 5 u M with the projection's constants, 3 u M without, each
                   partial result being at most M = |y s| + |b| + |i is| + |ib| in magnitude.  max(., 0) is 1-Lipschitz: an element
                   whose float64 sum lies within the bound of zero cannot exceed it, nothing is excluded.
  maxpool3x3s2     max is 1-Lipschitz in the sup norm: the largest of the window's element-wise bounds 2^-22 (|y s| + |b|)
  space_to_batch   with constants: 2^-23 (|x s| + |b|) (a product and a sum); the zero padding is exact
  16-bit output    the f32 bound plus HALF AN ULP of the storage type at the reference value (half_ulp)
  aspp_gather      acc = bias, then t in-image taps added one by one: t roundings of partial sums of at most |bias| + sum |z|
  colsum           thread-strided and tree sums in f64, one rounding to f32: u |ref| + rows 2^-53 sum |x|; accumulate = 1 adds the f32
                   sum out + s: u (|out_before| + |s|) more
  sum_resize       at(.) sums nmaps values (nmaps - 1 roundings), then 1 - lx, two products and a sum per row, 1 - ly, two products and
                   a sum: along any path to the output the value passes 6 roundings of at most A each, A = the largest over the four
                   taps of sum_i |a_i|: (6 + nmaps - 1) u A.  Plus the COORDINATE term of DESIGN 19: the kernel forms ry = (h - 1) /
                   (H - 1) and fy = ry y in float32, |d src| <= 2 u src, a weight moves by as much and the output by at most
                   2 u (src_y + src_x) x (the largest difference of two neighbours of the summed plane -- the plane, not the taps: at
                   an integer src the f32 value may fall just below it and read the neighbour before with a weight of ~1e-7).
  sum_resize_bwd   wy, wx as above (one rounding each beyond fr), row += wx d over at most nx outputs, acc += wy row over at most ny:
                   (nx + ny + 4) u (My^T |dout| Mx), nx / ny = the largest column populations of the two matrices; plus the adjoint
                   coordinate term: the sum of 2 u (src_y(o) + src_x(p)) |dout(o, p)| over the closed support |src - i| <= 1.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import resnet_ops_ref as R
from test_gpu_bn_forward_ops import DT, SENT, L, Out, half_ulp, hold, stored, table

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
E32 = 2.0 ** -22
NAMES = ["f32", "f32x3", "bf16", "f16"]
CAP = 4096 * 256
POOL_SHAPES = [(2, 8, 13, 10), (3, 20, 7, 9), (1, 4, 1, 1), (1, 4, 1, 7), (2, 12, 6, 1), (1, 8, 2, 2)]
RATES = [(1,), (2, 3), (6, 12, 18), (6, 12, 18, 24)]


def nchw(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def past_the_cap(items):
    """the work-item count of an over-cap case: more than one grid of 4096 x 256, and some threads one trip short of the others"""
    assert items > CAP and items % CAP != 0, items
    return items


def same_bits(tag, out, ref, tdt):
    """the output equals the float64 reference, rounded once to the storage type, bit for bit; the guard zones are untouched"""
    assert out.guards_ok(), f"{tag}: a guard zone was written"
    want = torch.from_numpy(np.ascontiguousarray(ref)).to(tdt)
    got = out.t.cpu()
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bits = torch.int32 if tdt == torch.float32 else torch.int16
    ne = got.view(bits) != want.view(bits)
    if bool(ne.any()):
        i = tuple(int(v) for v in ne.nonzero()[0])
        raise AssertionError(f"{tag}: {int(ne.sum())} of {ne.numel()} differ; first at {i}: got {float(got[i])!r} want {float(want[i])!r}")
    print(f"{tag}: bit for bit ({ne.numel()} elements)")


def signed_constants(rng, c):
    """per-channel scale / shift: 30 % negative scales, none near zero"""
    s, b = table(rng, c, 1, c)
    return stored(s), stored(b)


# ---- ustrun_relu_bwd_add --------------------------------------------------------------------------------------------------------------
def relu_bwd_add_check(name, n, seed):
    l = L()
    dt, tdt = DT[name]
    rng = np.random.default_rng(seed)
    (ag, a), (bg, b) = stored(rng.normal(size=n), tdt), stored(rng.normal(size=n) * rng.choice([1.0, 1e-3, 1e3], size=n), tdt)
    r = rng.normal(size=n)
    tiny = {torch.float32: 1e-45, torch.bfloat16: 1e-40, torch.float16: 6e-8}[tdt]           # a subnormal of the storage type
    r[:4] = [0.0, -0.0, -tiny, tiny]
    rg, r = stored(r, tdt)
    assert r[2] < 0 and r[3] > 0 and abs(r[2]) < torch.finfo(tdt).smallest_normal and np.signbit(r[1]) and r[1] == 0
    for has_b in (True, False):
        for has_ref in (True, False):
            g = Out((n,), tdt)
            l.check(l.lib().ustrun_relu_bwd_add(ag.data_ptr(), bg.data_ptr() if has_b else None, rg.data_ptr() if has_ref else None, n,
                                                g.ptr, dt, None))
            ref = R.relu_bwd_add(a, b if has_b else None, r if has_ref else None)
            if has_ref:
                assert (ref[:3] == 0).all() and ref[3] != 0                     # +0, -0 and the negative subnormal mask; the positive one passes
            same_bits(f"relu_bwd_add {name} n={n} b={has_b} ref={has_ref}", g, ref, tdt)


@pytest.mark.parametrize("n", [4, 1020])
@pytest.mark.parametrize("name", NAMES)
def test_relu_bwd_add_bit_for_bit(name, n):
    relu_bwd_add_check(name, n, seed=n)


def test_relu_bwd_add_past_the_grid_cap():
    relu_bwd_add_check("bf16", 4 * past_the_cap(1081537), seed=5)


# ---- ustrun_aspp_scatter / ustrun_aspp_gather -----------------------------------------------------------------------------------------
# (29, 26): every tap of every rate lands somewhere (rate 24 too); (9, 11): the rates from 12 on are larger than the map; (5, 4) and below:
# smaller than every rate from 6 on, only the centre taps land
ASPP_EXTENTS = [(29, 26), (9, 11), (5, 4), (1, 1), (1, 7), (6, 1)]


def aspp_scatter_check(name, rates, K, n, h, w, zcp, seed):
    l = L()
    dt, tdt = DT[name]
    rng = np.random.default_rng(seed)
    dlg, dl = stored(rng.normal(size=(n, h, w, K)))
    dz = Out((n, h, w, zcp), tdt)
    rr = (C.c_int * len(rates))(*rates)
    l.check(l.lib().ustrun_aspp_scatter(dlg.data_ptr(), n, h, w, K, len(rates), rr, zcp, dz.ptr, dt, None))
    ref = nhwc(R.aspp_scatter(nchw(dl), K, rates, zcp))
    same_bits(f"aspp_scatter {name} rates={rates} K={K} {(n, h, w)} zcp={zcp}", dz, ref, tdt)


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name", NAMES)
def test_aspp_scatter_bit_for_bit(name, rates):
    for K in (1, 2, 3, 4):
        zc = len(rates) * 9 * K
        for h, w in ASPP_EXTENTS:
            for zcp in (zc, (zc + 127) // 128 * 128):
                aspp_scatter_check(name, rates, K, 2, h, w, zcp, seed=zc + h)
    if min(rates) >= 6:
        assert (R.aspp_taps(5, 4, rates) == len(rates)).all()                   # nothing but the centre taps
    assert max(rates) < min(ASPP_EXTENTS[0])                                    # there every tap of every rate lands somewhere


def test_aspp_scatter_past_the_grid_cap():
    past_the_cap(2 * 65 * 65 * 128)
    aspp_scatter_check("bf16", (6, 12, 18, 24), 3, 2, 65, 65, 128, seed=6)


def aspp_gather_check(rates, K, n, h, w, seed):
    l = L()
    rng = np.random.default_rng(seed)
    zc = len(rates) * 9 * K
    zg, z = stored(rng.normal(size=(n, h, w, zc)))
    bg, bias = stored(rng.normal(size=K) * 3.0)
    out = Out((n, h, w, K))
    rr = (C.c_int * len(rates))(*rates)
    l.check(l.lib().ustrun_aspp_gather(zg.data_ptr(), n, h, w, K, len(rates), rr, bg.data_ptr(), out.ptr, None))
    zn = nchw(z)
    ref = R.aspp_gather(zn, K, rates, bias)
    bound = R.aspp_taps(h, w, rates)[None, None] * U24 * R.aspp_gather(np.abs(zn), K, rates, np.abs(bias))
    hold(f"aspp_gather rates={rates} K={K} {(n, h, w)}", out.get(), nhwc(ref), nhwc(bound))


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("rates", RATES)
def test_aspp_gather(rates, K):
    for h, w in ASPP_EXTENTS:
        aspp_gather_check(rates, K, 2, h, w, seed=10 * K + h)


def test_aspp_gather_past_the_grid_cap():
    past_the_cap(2 * 365 * 363 * 4)
    aspp_gather_check((3,), 4, 2, 365, 363, seed=7)


# ---- ustrun_rowwin_patches ------------------------------------------------------------------------------------------------------------
def rowwin_src(l, ptr, cin, win, hp, wp, stride, wo):
    """the padded NHWC source [N, hp, wp, cin] described window-wise (include/ustrun.h): "channels" = the window, pixel stride = cin"""
    return l.Src(ptr, None, None, win, hp, stride * (wo - 1) + 1, hp * wp * cin, wp * cin, cin, 1, 0, 0, 0, 0, 0, 0, 0)


def rowwin_check(name, n, ho, wo, cin, win, nrows, stride, kp, seed):
    l = L()
    dt, tdt = DT[name]
    rng = np.random.default_rng(seed)
    hp = stride * (ho - 1) + nrows
    wp = -(-(stride * (wo - 1) * cin + win) // cin)               # the last window ends inside the last row
    xg, x = stored(rng.normal(size=(n, hp, wp, cin)), tdt)
    out = Out((n, ho, wo, kp), tdt)
    src = rowwin_src(l, xg.data_ptr(), cin, win, hp, wp, stride, wo)
    l.check(l.lib().ustrun_rowwin_patches(C.byref(src), n, ho, wo, nrows, stride, kp, out.ptr, dt, None))
    ref = nhwc(R.rowwin_patches(nchw(x), cin, ho, wo, nrows, win, stride, kp))
    same_bits(f"rowwin_patches {name} Cin={cin} win={win} nrows={nrows} stride={stride} kp={kp}", out, ref, tdt)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_rowwin_patches_bit_for_bit(name, stride):
    for nrows in (1, 3, 7):
        for cin, win in ((1, 8), (1, 24), (3, 8), (3, 24)):
            for kp in (nrows * win, nrows * win + 24):
                rowwin_check(name, 2, 5, 6, cin, win, nrows, stride, kp, seed=nrows + win)


def test_rowwin_patches_past_the_grid_cap():
    past_the_cap(2 * 150 * 150 * (192 // 8))
    rowwin_check("bf16", 2, 150, 150, 3, 24, 7, 2, 192, seed=8)


# ---- ustrun_space_to_batch ------------------------------------------------------------------------------------------------------------
def s2b_check(name, n, c, h, w, r, seed, constants=True):
    l = L()
    dt, tdt = DT[name]
    rng = np.random.default_rng(seed)
    xg, x = stored(rng.normal(size=(n, h, w, c)), tdt)
    (sg, s), (bg, b) = signed_constants(rng, c)
    hs, ws = -(-h // r), -(-w // r)
    xn = nchw(x)
    tag = f"space_to_batch {name} r={r} C={c} {(n, h, w)}"
    out = Out((n * r * r, hs, ws, c), tdt)
    l.check(l.lib().ustrun_space_to_batch(C.byref(l.nhwc_src(xg.data_ptr(), c, h, w)), n, r, out.ptr, dt, None))
    plain = R.space_to_batch(xn, r)
    same_bits(tag + " copy", out, nhwc(plain), tdt)
    if h < r:
        assert not plain.reshape(n, r, r, c, hs, ws)[:, h:].any()               # whole sub-grids of zeros
    if not constants:
        return
    mag = R.space_to_batch(np.abs(xn * s[None, :, None, None]) + np.abs(b[None, :, None, None]), r)     # (zero in the padding: exact there)
    for relu in (1, 0):
        out = Out((n * r * r, hs, ws, c), tdt)
        src = l.nhwc_src(xg.data_ptr(), c, h, w, sg.data_ptr(), bg.data_ptr(), relu=relu)
        l.check(l.lib().ustrun_space_to_batch(C.byref(src), n, r, out.ptr, dt, None))
        ref = R.space_to_batch(xn, r, s, b, bool(relu))
        assert relu or (ref < -0.1).any()
        hold(f"{tag} relu={relu}", out.get(), nhwc(ref), nhwc(2 * U24 * mag + half_ulp(ref, name)))


@pytest.mark.parametrize("r", [2, 3, 4, 8])
@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_space_to_batch(name, r):
    for c in (8, 24):
        for h, w in ((13, 10), (1, 5), (3, 3), (2 * r, 3 * r), (r + 1, 2 * r - 1)):
            s2b_check(name, 2, c, h, w, r, seed=r + c + h)


def test_space_to_batch_past_the_grid_cap():
    past_the_cap(2 * 2 * 2 * 65 * 66 * (256 // 8))
    s2b_check("bf16", 2, 256, 130, 131, 2, seed=9, constants=False)


# ---- ustrun_maxpool3x3s2_bwd ----------------------------------------------------------------------------------------------------------
SCALES, SHIFTS = [1.0, 2.0, -1.0, 0.5, 0.0, -2.0], [0.0, -0.5, 0.25, 1.0]


def maxpool_bwd_check(name, n, c, h, w, seed):
    """every activation y s + b with y in {-1, -1/4, 1/2, 1} and these constants is exact in f32 and in both 16-bit types; dp is a multiple
    of 1/4 in [-4, 4].  Returns (share of tied windows, the set of winning positions)."""
    l = L()
    dt, tdt = DT[name]
    rng = np.random.default_rng(seed)
    ho, wo = (h + 1) // 2, (w + 1) // 2
    yg, y = stored(rng.choice(np.array([-1.0, -0.25, 0.5, 1.0]), size=(n, h, w, c)), tdt)
    dpg, dp = stored(rng.integers(-16, 17, size=(n, ho, wo, c)) / 4.0, tdt)
    (sg, s), (bg, b) = stored(np.array([SCALES[i % 6] for i in range(c)])), stored(np.array([SHIFTS[i % 4] for i in range(c)]))
    da = Out((n, h, w, c), tdt)
    l.check(l.lib().ustrun_maxpool3x3s2_bwd(dpg.data_ptr(), yg.data_ptr(), sg.data_ptr(), bg.data_ptr(), n, h, w, c, da.ptr, dt, None))
    a = R.act(nchw(y), s, b)
    ref, best = R.maxpool3x3s2_route(nchw(dp), a)
    same_bits(f"maxpool3x3s2_bwd {name} {(n, c, h, w)}", da, nhwc(ref), tdt)
    tied = float((R.window_ties(a) > 1).mean())
    if c > 4:       # channel 4: scale 0, shift 0 -- every window all-tied: the FIRST in-image position takes the gradient
        first = np.where(np.arange(ho) == 0, 3, 0)[:, None] + np.where(np.arange(wo) == 0, 1, 0)[None, :]
        assert (a[:, 4] == 0).all() and (best[:, 4] == first[None]).all()
    return tied, set(np.unique(best).tolist())


@pytest.mark.parametrize("n,c,h,w", POOL_SHAPES)
@pytest.mark.parametrize("name", NAMES)
def test_maxpool3x3s2_bwd_routes_to_the_first_maximum(name, n, c, h, w):
    tied, winners = maxpool_bwd_check(name, n, c, h, w, seed=200 + h * 10 + w)      # (a draw at which the few-window shapes are tied enough too)
    print(f"tied share {tied:.2f}, winners {sorted(winners)}")
    if h * w > 1:
        assert tied >= 0.3, tied
    if (n, c, h, w) in POOL_SHAPES[:2]:
        assert winners == set(range(9)), winners


def test_maxpool3x3s2_bwd_past_the_grid_cap():
    past_the_cap(131 * 131 * (256 // 4))
    maxpool_bwd_check("bf16", 1, 256, 131, 131, seed=11)


# ---- ustrun_maxpool3x3s2 --------------------------------------------------------------------------------------------------------------
def maxpool_check(name, n, c, h, w, seed):
    l = L()
    dt, tdt = DT[name]
    rng = np.random.default_rng(seed)
    (sg, s), (bg, b) = signed_constants(rng, c)
    y = rng.normal(size=(n, h, w, c))
    sel = np.arange(c) % 3 != 1                      # window (0, 0) of every image, two channels in three: y s + b = -1 at all its pixels
    y[:, :2, :2][:, :, :, sel] = ((-1.0 - b) / s)[sel]
    yg, y = stored(y, tdt)
    out = Out((n, (h + 1) // 2, (w + 1) // 2, c), tdt)
    l.check(l.lib().ustrun_maxpool3x3s2(yg.data_ptr(), sg.data_ptr(), bg.data_ptr(), n, h, w, c, out.ptr, dt, None))
    yn = nchw(y)
    ref = R.maxpool3x3s2(R.act(yn, s, b))
    bound = E32 * R.window_max(R.act_magnitude(yn, s, b), 0.0) + half_ulp(ref, name)
    got = out.get()
    hold(f"maxpool3x3s2 {name} {(n, c, h, w)}", got, nhwc(ref), nhwc(bound))
    assert (ref[:, sel, 0, 0] == 0).all() and (got[:, 0, 0, sel] == 0).all()     # windows whose every activation is zero


@pytest.mark.parametrize("n,c,h,w", POOL_SHAPES + [(2, 64, 37, 45)])
@pytest.mark.parametrize("name", NAMES)
def test_maxpool3x3s2(name, n, c, h, w):
    maxpool_check(name, n, c, h, w, seed=h * 10 + w)


def test_maxpool3x3s2_past_the_grid_cap():
    past_the_cap(129 * 129 * (256 // 4))
    maxpool_check("f16", 1, 256, 257, 257, seed=12)


# ---- ustrun_bn_add_relu ---------------------------------------------------------------------------------------------------------------
def join_check(name, c, npix, seed):
    l = L()
    dt, tdt = DT[name]
    rng = np.random.default_rng(seed)
    (sg, s), (bg, b) = signed_constants(rng, c)
    (isg, is_), (ibg, ib) = signed_constants(rng, c)
    yg, y = stored(rng.normal(size=(1, 1, npix, c)), tdt)
    yn = nchw(y)
    pre = yn * s[None, :, None, None] + b[None, :, None, None]
    for proj in (True, False):
        idn = rng.normal(size=yn.shape)
        cancel = rng.random(size=yn.shape) < 0.4      # an identity that cancels y s + b up to its own rounding to the storage type
        idn = np.where(cancel, (-pre - ib[None, :, None, None]) / is_[None, :, None, None] if proj else -pre, idn)
        ig, idn = stored(nhwc(idn), tdt)
        out = Out((1, 1, npix, c), tdt)
        l.check(l.lib().ustrun_bn_add_relu(yg.data_ptr(), sg.data_ptr(), bg.data_ptr(), ig.data_ptr(), isg.data_ptr() if proj else None,
                                           ibg.data_ptr() if proj else None, npix, c, out.ptr, dt, None))
        args = (yn, s, b, nchw(idn), is_ if proj else None, ib if proj else None)
        ref, M = R.join(*args), R.join_magnitude(*args)
        assert cancel.sum() == 0 or (np.abs(ref[cancel]) <= 2.0 ** -7 * M[cancel]).all()
        hold(f"bn_add_relu {name} C={c} npix={npix} proj={proj}", out.get(), nhwc(ref), nhwc((5 if proj else 3) * U24 * M + half_ulp(ref, name)))


@pytest.mark.parametrize("c,npix", [(4, 1), (4, 37), (12, 35), (64, 1), (64, 129), (2048, 1), (2048, 5)])
@pytest.mark.parametrize("name", NAMES)
def test_bn_add_relu(name, c, npix):
    join_check(name, c, npix, seed=c + npix)


def test_bn_add_relu_past_the_grid_cap():
    past_the_cap(129 * 131 * (256 // 4))
    join_check("bf16", 256, 129 * 131, seed=13)


# ---- ustrun_colsum --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3, 21])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 8450])
def test_colsum(rows, c):
    l = L()
    lib = l.lib()
    rng = np.random.default_rng(rows + c)
    x = rng.normal(size=(rows, c)) * rng.uniform(0.5, 20.0, c)
    cc = c // 2
    if rows > 1:      # one column whose terms cancel to about 1e-6 of sum |x|
        x[-1, cc] = -R.colsum(x[:-1])[cc] + 1e-6 * np.abs(x[:, cc]).sum()
    xg, x = stored(x)
    ref, sabs = R.colsum(x), np.abs(x).sum(0)
    if rows > 1:
        assert 1e-7 * sabs[cc] < abs(ref[cc]) < 1e-5 * sabs[cc], (ref[cc], sabs[cc])
    base = U24 * np.abs(ref) + rows * 2.0 ** -53 * sabs
    out = Out((c,))
    l.check(lib.ustrun_colsum(xg.data_ptr(), rows, c, out.ptr, 0, None))
    first = out.t.clone()
    hold(f"colsum rows={rows} C={c}", out.get(), ref, base)
    l.check(lib.ustrun_colsum(xg.data_ptr(), rows, c, out.ptr, 0, None))
    assert torch.equal(first.view(torch.int32), out.t.view(torch.int32)) and out.guards_ok()       # fixed order: a repeated call is bit-identical
    before = rng.normal(size=c) * 10.0
    acc = Out((c,), init=before)
    before = acc.t.double().cpu().numpy()
    l.check(lib.ustrun_colsum(xg.data_ptr(), rows, c, acc.ptr, 1, None))
    hold(f"colsum rows={rows} C={c} accumulate", acc.get(), before + ref, base + U24 * (np.abs(before) + np.abs(ref)))


# ---- ustrun_sum_resize_bilinear / _bwd ------------------------------------------------------------------------------------------------
def coord_err(n_in, n_out):
    """|d src| of each output: the f32 quotient and the f32 product, 2^-24 of src each (header)"""
    return 2 * U24 * R.resize_coord(n_in, n_out)


def tap_max(a, H, W):
    """largest a of the four taps of every output: [N, K, h, w] -> [N, K, H, W]"""
    h, w = a.shape[2:]
    y0 = np.minimum(np.floor(R.resize_coord(h, H)).astype(int), h - 1)
    x0 = np.minimum(np.floor(R.resize_coord(w, W)).astype(int), w - 1)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    m = None
    for iy in (y0, y1):
        for ix in (x0, x1):
            t = a[:, :, iy][:, :, :, ix]
            m = t if m is None else np.maximum(m, t)
    return m


def neighbour_diff(s):
    """the largest |difference| of two vertical or horizontal neighbours of every plane: [N, K, h, w] -> [N, K, 1, 1]"""
    d = np.zeros(s.shape[:2])
    if s.shape[2] > 1:
        d = np.maximum(d, np.abs(np.diff(s, axis=2)).max(axis=(2, 3)))
    if s.shape[3] > 1:
        d = np.maximum(d, np.abs(np.diff(s, axis=3)).max(axis=(2, 3)))
    return d[:, :, None, None]


def resize_fwd_check(n, k, h, w, H, W, nmaps, seed):
    l = L()
    rng = np.random.default_rng(seed)
    dev, maps = zip(*[stored(rng.normal(size=(n, h, w, k))) for _ in range(nmaps)])
    arr = (C.c_void_p * 4)(*[t.data_ptr() for t in dev], *([None] * (4 - nmaps)))
    out = Out((n, k, H, W))
    l.check(l.lib().ustrun_sum_resize_bilinear(arr, nmaps, n, h, w, k, H, W, out.ptr, None))
    mn = [nchw(m) for m in maps]
    ref = R.sum_resize(mn, H, W)
    arith = (6 + nmaps - 1) * U24 * tap_max(sum(np.abs(m) for m in mn), H, W)
    coord = (coord_err(h, H)[:, None] + coord_err(w, W)[None, :])[None, None] * neighbour_diff(sum(mn))
    got = out.get()
    tag = f"sum_resize_bilinear {(h, w)}->{(H, W)} N={n} K={k} maps={nmaps}"
    hold(tag, got, ref, arith + coord)
    with np.errstate(divide="ignore", invalid="ignore"):      # (a figure, not a check: how far the coordinate term is needed)
        print(f"{tag} without the coordinate term: {np.nanmax(np.abs(got - ref) / arith):.3g}")
    if (h, w) == (H, W) and nmaps == 1:
        assert np.array_equal(got, mn[0])


def resize_bwd_check(n, k, h, w, H, W, seed):
    l = L()
    lib = l.lib()
    rng = np.random.default_rng(seed)
    dg, d = stored(rng.normal(size=(n, k, H, W)))
    dlow = Out((n, h, w, k))
    l.check(lib.ustrun_sum_resize_bilinear_bwd(dg.data_ptr(), n, h, w, k, H, W, dlow.ptr, None))
    first = dlow.t.clone()
    l.check(lib.ustrun_sum_resize_bilinear_bwd(dg.data_ptr(), n, h, w, k, H, W, dlow.ptr, None))
    assert torch.equal(first.view(torch.int32), dlow.t.view(torch.int32))           # fixed order, nothing accumulated into what is there
    ref = R.sum_resize_adjoint(d, h, w)
    ad = np.abs(d)
    My, Mx = R.resize_matrix(h, H), R.resize_matrix(w, W)
    ny, nx = int((My != 0).sum(0).max()), int((Mx != 0).sum(0).max())
    Ty, Tx = R.resize_touch(h, H), R.resize_touch(w, W)
    coord = (R.sum_resize_adjoint(ad, h, w, Ty * coord_err(h, H)[:, None], Tx) + R.sum_resize_adjoint(ad, h, w, Ty, Tx * coord_err(w, W)[:, None]))
    arith = (nx + ny + 4) * U24 * R.sum_resize_adjoint(ad, h, w)
    got = dlow.get()
    tag = f"sum_resize_bilinear_bwd {(h, w)}<-{(H, W)} N={n} K={k}"
    hold(tag, got, nhwc(ref), nhwc(arith + coord))
    return got, ref


RESIZE_CASES = [      # (h, w), (H, W), maps, N, K
    ((9, 13), (41, 50), 4, 2, 3),
    ((9, 7), (67, 50), 1, 1, 4),
    ((5, 5), (5, 5), 2, 2, 1),                   # the identity
    ((1, 6), (7, 1), 3, 1, 3),
    ((17, 12), (9, 5), 2, 2, 4),                 # a downsample
    ((2, 3), (129, 200), 1, 1, 3),
    ((65, 65), (513, 513), 1, 1, 3),             # the production head
]


@pytest.mark.parametrize("lo,hi,nmaps,n,k", RESIZE_CASES)
def test_sum_resize_bilinear(lo, hi, nmaps, n, k):
    resize_fwd_check(n, k, *lo, *hi, nmaps, seed=lo[0] * 31 + hi[1])
    if nmaps != 1:
        resize_fwd_check(n, k, *lo, *hi, 1, seed=lo[0] * 31 + hi[1] + 1)        # the engine's own call: one map


@pytest.mark.parametrize("lo,hi,nmaps,n,k", RESIZE_CASES)
def test_sum_resize_bilinear_bwd(lo, hi, nmaps, n, k):
    resize_bwd_check(n, k, *lo, *hi, seed=lo[0] * 31 + hi[1])


def test_sum_resize_bilinear_past_the_grid_cap():
    past_the_cap(2 * 3 * 419 * 421)
    resize_fwd_check(2, 3, 53, 53, 419, 421, 2, seed=14)


def test_sum_resize_bilinear_bwd_past_the_grid_cap():
    past_the_cap(2 * 363 * 365 * 4)
    resize_bwd_check(2, 4, 363, 365, 400, 402, seed=15)


# ---- documented refusals --------------------------------------------------------------------------------------------------------------
def test_documented_refusals():
    """Every refusal these entries document returns nonzero with a message that names the entry, before anything is launched: the
    outputs and their guard zones keep the sentinel."""
    l = L()
    lib = l.lib()
    x16 = torch.zeros(8192, device="cuda", dtype=torch.bfloat16)
    x32 = torch.zeros(8192, device="cuda")
    const = torch.ones(64, device="cuda")
    o16, o32 = Out((8192,), torch.bfloat16), Out((8192,))
    p16, p32, cp = x16.data_ptr(), x32.data_ptr(), const.data_ptr()

    def refused(rc, entry):
        msg = lib.ustrun_last_error()
        assert rc != 0, entry
        assert msg.startswith(entry.encode() + b":"), (entry, msg)

    # C % 4 != 0: the pools and the join; a lone iscale / ishift
    refused(lib.ustrun_maxpool3x3s2(p32, cp, cp, 1, 4, 6, 6, o32.ptr, 0, None), "maxpool3x3s2")
    refused(lib.ustrun_maxpool3x3s2(p16, cp, cp, 1, 4, 6, 10, o16.ptr, 1, None), "maxpool3x3s2")
    refused(lib.ustrun_maxpool3x3s2_bwd(p32, p32, cp, cp, 1, 4, 6, 6, o32.ptr, 0, None), "maxpool3x3s2_bwd")
    refused(lib.ustrun_maxpool3x3s2_bwd(p16, p16, cp, cp, 1, 4, 6, 10, o16.ptr, 1, None), "maxpool3x3s2_bwd")
    refused(lib.ustrun_bn_add_relu(p32, cp, cp, p32, None, None, 24, 6, o32.ptr, 0, None), "bn_add_relu")
    refused(lib.ustrun_bn_add_relu(p16, cp, cp, p16, cp, None, 24, 8, o16.ptr, 1, None), "bn_add_relu")
    refused(lib.ustrun_bn_add_relu(p16, cp, cp, p16, None, cp, 24, 8, o16.ptr, 1, None), "bn_add_relu")
    # relu_bwd_add: n % 4 != 0
    refused(lib.ustrun_relu_bwd_add(p32, p32, p32, 1022, o32.ptr, 0, None), "relu_bwd_add")
    refused(lib.ustrun_relu_bwd_add(p16, None, None, 1021, o16.ptr, 1, None), "relu_bwd_add")
    # nrates of 0 and of 5; zc_padded below nrates * 9 * K
    rr = (C.c_int * 5)(1, 2, 3, 4, 5)
    for nr in (0, 5):
        refused(lib.ustrun_aspp_gather(p32, 1, 3, 3, 2, nr, rr, cp, o32.ptr, None), "aspp_gather")
        refused(lib.ustrun_aspp_scatter(p32, 1, 3, 3, 2, nr, rr, 128, o16.ptr, 1, None), "aspp_scatter")
    refused(lib.ustrun_aspp_scatter(p32, 1, 3, 3, 2, 2, rr, 35, o32.ptr, 0, None), "aspp_scatter")
    refused(lib.ustrun_aspp_scatter(p32, 1, 3, 3, 3, 4, rr, 104, o16.ptr, 1, None), "aspp_scatter")
    # nmaps of 0 and of 5
    arr = (C.c_void_p * 5)(*([p32] * 5))
    for nm in (0, 5):
        refused(lib.ustrun_sum_resize_bilinear(arr, nm, 1, 3, 3, 2, 6, 6, o32.ptr, None), "sum_resize_bilinear")
    # colsum: one block per column, 65535 at the most
    refused(lib.ustrun_colsum(p32, 1, 65536, o32.ptr, 0, None), "colsum")
    # space_to_batch: f32 storage, r outside 2..8, C % 8, a strided source, ReLU without constants
    def s2b(c=8, **kw):
        return l.nhwc_src(p16, c, 4, 6, **kw)

    def strided(s):
        s.sW += 8
        return s

    for dt in (0, 3):
        refused(lib.ustrun_space_to_batch(C.byref(l.nhwc_src(p32, 8, 4, 6)), 1, 2, o32.ptr, dt, None), "space_to_batch")
    for r in (1, 9):
        refused(lib.ustrun_space_to_batch(C.byref(s2b()), 1, r, o16.ptr, 1, None), "space_to_batch")
    refused(lib.ustrun_space_to_batch(C.byref(s2b(c=12)), 1, 2, o16.ptr, 1, None), "space_to_batch")
    refused(lib.ustrun_space_to_batch(C.byref(strided(s2b())), 1, 2, o16.ptr, 1, None), "space_to_batch")
    refused(lib.ustrun_space_to_batch(C.byref(s2b(relu=1)), 1, 2, o16.ptr, 1, None), "space_to_batch")
    refused(lib.ustrun_space_to_batch(C.byref(s2b(scale=cp)), 1, 2, o16.ptr, 1, None), "space_to_batch")
    # rowwin_patches: window % 8, k_padded % 8, k_padded < nrows * window, a source that does not cover the windows (rows; window starts)
    def rw(win=24, hp=13, wp=16, wo=5):
        return rowwin_src(l, p16, 3, win, hp, wp, 2, wo)

    refused(lib.ustrun_rowwin_patches(C.byref(rw(win=20)), 1, 4, 5, 7, 2, 192, o16.ptr, 1, None), "rowwin_patches")
    refused(lib.ustrun_rowwin_patches(C.byref(rw()), 1, 4, 5, 7, 2, 172, o16.ptr, 1, None), "rowwin_patches")
    refused(lib.ustrun_rowwin_patches(C.byref(rw()), 1, 4, 5, 7, 2, 160, o16.ptr, 1, None), "rowwin_patches")
    refused(lib.ustrun_rowwin_patches(C.byref(rw(hp=12)), 1, 4, 5, 7, 2, 192, o16.ptr, 1, None), "rowwin_patches")
    refused(lib.ustrun_rowwin_patches(C.byref(rw(wo=4)), 1, 4, 5, 7, 2, 192, o16.ptr, 1, None), "rowwin_patches")
    torch.cuda.synchronize()
    for o in (o16, o32):
        assert o.guards_ok() and bool((o.t == SENT).all())
