"""Exact-integer parity of the bf16 kernels AT THE SHAPES THAT SELECT THE PRODUCTION TILES.

`conv3x3_halo_launch_bf16` picks its tile from the extent and the grid size: the 256-pixel x 128-channel tiles
(<8,32,128,MI4> wide, <16,16,128,MI4> narrow) only from 512 blocks up, the 64-channel tiles <8,32,64,MI2,NT2> /
<16,16,64,MI2,NT2> for Cout % 128 != 0, <8,16,128,MI2,NT2> and <8,16,64,MI1,NT2> for mid-sized / small grids.  The
step of BASELINE.json configs[1] spends its time in the first four; the small operator tests (test_gpu_ops.py) only ever
reach the last two.  Every case here asserts the tile it was written for (`ustrun_debug_last_conv_variant`) and checks
forward (+ BatchNorm statistics), the input gradient (whole and split over two destinations with an offset window) and
the weight gradient against torch-CPU on small-integer data: integers up to 2^8 are exact in bf16 and their sums exact
in f32, so a fragment-layout, tap, halo, pass-constant or edge-mask slip shows as an O(1) error (rel 1e-6 bound).
Sources carry BatchNorm affine + ReLU with power-of-two scales and integer shifts (the transforming loader, `XF`),
gradients come from plain sources (the LDS-DMA loader); batched passes (`gN`, `gstride`) use different constants per
pass and are compared with per-pass torch results.  Reference ops: networks/unet_parts.py:8-68 and their autograd.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


class E:
    """the 16-bit element type the current test runs on: every test of this file runs for both builds of the kernel sources
    (bf16, and IEEE half = the reference's torch.cuda.amp autocast type, train.py:551-552); the integer data is exact in both"""
    t, code = torch.bfloat16, 1


@pytest.fixture(autouse=True, params=["bf16", "f16"])
def elt(request):
    E.t, E.code = (torch.bfloat16, 1) if request.param == "bf16" else (torch.float16, 2)
    yield request.param
    E.t, E.code = torch.bfloat16, 1


def L():
    from ustrun import _lib
    return _lib


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def nhwc16(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda().to(E.t)


def from_nhwc(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def r16(t):
    return t.to(E.t).float()


def pack16(w):
    l = L()
    co, ci = w.shape[:2]
    n = 9 * ((ci + 7) // 8 * 8) * ((co + 7) // 8 * 8)
    wf = torch.zeros(n, dtype=E.t, device="cuda")
    wd = torch.zeros(n, dtype=E.t, device="cuda")
    wg = w.contiguous().cuda()
    l.check(l.lib().ustrun_pack_conv3x3(wg.data_ptr(), co, ci, wf.data_ptr(), wd.data_ptr(), E.code, None))
    return wf, wd


def variant(th, tw, bn, mi, nt, *rest):
    """rest = [build tag,] pool, xf; build tag "m16" = the 16x16x32 build (bit 7 of the code).
    ("lin", W, 128, 4, 1): the linear tiles of round 5 (256 consecutive positions of the flat padded space, row length W)"""
    if th == "lin":
        return 1 << 30 | tw << 16 | bn << 8 | (0 if rest[-1] else 0x80) | mi << 4 | nt << 2 | (1 if rest[-1] else 0)
    m16 = 0x80 if (rest and rest[0] == "m16") else 0
    pool, xf = rest[-2], rest[-1]
    return th << 24 | tw << 16 | bn << 8 | m16 | mi << 4 | nt << 2 | (2 if pool else 0) | (1 if xf else 0)


def vstr(v):
    if v >> 30 & 1:
        return "linear W%d BN%d MI%d%s xf%d" % ((v >> 16) & 255, (v >> 8) & 255, (v >> 4) & 7, " m16" if v & 0x80 else "", v & 1)
    return "TH%d TW%d BN%d MI%d%s NT%d pool%d xf%d" % (v >> 24, (v >> 16) & 255, (v >> 8) & 255, (v >> 4) & 7, " m16" if v & 0x80 else "",
                                                    (v >> 2) & 3, (v >> 1) & 1, v & 1)


# (id, N, source channels, Cout, H, W, groups, forward tile, input-gradient tile)
#   tiles as (TH, TW, BN, MI, NT); the input gradient runs the same kernel with Cin/Cout swapped on a plain source
CASES = [
    # 256 px x 128 ch, wide rows: every wide layer (>= 32 px) of the step; dgrad the same tile
    ("tall_wide_128", 8, (128,), 128, 128, 128, 2, (8, 32, 128, 4, 1), (8, 32, 128, 4, 1)),
    # the concat conv of up4 (skip 64 ++ ConvTranspose 64 -> 64) at full resolution: 64-channel wide tile forward, the
    # 128-channel tall tile with the two-destination epilogue for its input gradient
    ("cat_128_to_64", 8, (64, 64), 64, 128, 128, 2, (8, 32, 64, 2, 2), (8, 32, 128, 4, 1)),
    # 256 px x 128 ch with 16-pixel rows (extent < 32 px), ragged right / bottom edges
    # (24-pixel rows run on the linear tiles since round 5: ustrun_debug_flags2 bit 0 keeps this case on the tile it was written for)
    ("tall_narrow_512", 16, (512,), 512, 56, 24, 1, (16, 16, 128, 4, 1), (16, 16, 128, 4, 1), (0, 1)),
    # the bottleneck of the student's four batched passes as the step runs it: N = 64, 16 x 16, 1024 -> 1024
    ("bottleneck_n64", 64, (1024,), 1024, 16, 16, 4, (16, 16, 128, 4, 1), (16, 16, 128, 4, 1)),
    # 64 -> 64 full-resolution layers (inc.conv2, up4.conv2): wide and narrow 64-channel tiles
    ("c64_wide", 2, (64,), 64, 64, 64, 1, (8, 32, 64, 2, 2), (8, 32, 64, 2, 2)),
    ("c64_narrow", 2, (64,), 64, 40, 24, 1, (16, 16, 64, 2, 2), (16, 16, 64, 2, 2)),
    # mid-sized grid (>= 256 blocks of 8 x 16 px, < 512 tall blocks): two taps per barrier at 128 channels; its input
    # gradient (512 -> 128 channels) is a small grid: 64-channel blocks with one sub-tile per wave
    ("mid_grid_512", 8, (128,), 512, 32, 32, 1, (8, 16, 128, 2, 2), (8, 16, 64, 1, 2)),
    # 64 -> 64 at full resolution with enough strips to fill the chip: the weight-stationary row-streaming kernel
    # (conv_ws64_bf16.hip) -- 8 segments of 2 steps; then ragged: 9 row-steps in segments of 2 (the last one short), 2.5
    # strips of 32 px, four passes
    ("ws64_n8_128", 8, (64,), 64, 128, 128, 2, "ws", "ws"),
    ("ws64_ragged", 16, (64,), 64, 72, 80, 4, "ws", "ws"),
    # the same two with the other builds of that kernel forced (ustrun_debug_flags bit 1: four waves, bit 2: eight waves; the
    # default is the consumer / producer build)
    ("ws64w4_n8_128", 8, (64,), 64, 128, 128, 2, "ws4", "ws4"),
    ("ws64w4_ragged", 16, (64,), 64, 72, 80, 4, "ws4", "ws4"),
    ("ws64w8_n8_128", 8, (64,), 64, 128, 128, 2, "ws8", "ws8"),
    ("ws64w8_ragged", 16, (64,), 64, 72, 80, 4, "ws8", "ws8"),
    # single pass, odd strip count, a last segment of one step, N not a multiple of anything
    ("ws64_odd", 9, (64,), 64, 88, 104, 1, "ws", "ws"),
    # the FLAT plan of that kernel (round 6: block b takes steps [b L, (b + 1) L) of the strips' step sequence; variant | 0x800): 260
    # strips of 8 steps -> 9 steps per block, pieces cut mid-strip and across images and passes; then ragged: 270 strips (2.5 per
    # image row) of 9 steps (the last one 6 rows) in three passes, 10 steps per block
    ("ws64f_130_64", 130, (64,), 64, 64, 64, 2, "wsf", "wsf"),
    ("ws64f_ragged", 90, (64,), 64, 70, 80, 3, "wsf", "wsf"),
    # ---- what the padding-aware tile rule (halo_plan.h::halo_tile128, round 3) selects on the maps of BASELINE.json
    # configs[2] / configs[3] (prostate 384 x 384: 48 / 24-pixel levels; M&Ms 288 x 288: 144 / 18-pixel levels;
    # reference train.py:416-418, train_mnms.py:397-399) -- VERDICT r3 next 3.  48 x 48 is >= 32 wide but pads 48 -> 64 on
    # the 8 x 32 tile: the rule takes 16 x 16 tiles; 18 x 18 and 24 x 24 pad to 32 on 16 x 16 tiles: 8 x 16 MI 2;
    # 144 x 144 (= 4.5 x 32): 16 x 16 as well
    ("pad_48_512", 16, (512,), 512, 48, 48, 2, (16, 16, 128, 4, 1), (16, 16, 128, 4, 1)),
    # (since round 5 these two maps run on the linear tiles -- the LIN cases below; ustrun_debug_flags2 bit 0 keeps the rule's tile: a
    # case's flags are one int for ustrun_debug_flags or a pair for (ustrun_debug_flags, ustrun_debug_flags2))
    ("pad_18_1024", 64, (1024,), 1024, 18, 18, 4, (8, 16, 128, 2, 2), (8, 16, 128, 2, 2), (0, 1)),
    ("pad_24_1024", 64, (1024,), 1024, 24, 24, 4, (8, 16, 128, 2, 2), (8, 16, 128, 2, 2), (0, 1)),
    ("pad_144_128", 8, (128,), 128, 144, 144, 2, (16, 16, 128, 4, 1), (16, 16, 128, 4, 1)),
    # ---- the 512-pixel x 64-channel tile (16 x 32 px, wave tile 128 px x 64 ch, one block per CU; ustrun_debug_flags bit 13):
    # the concat conv of up4 forward, and the input gradient of a 64 -> 128 layer (a 128 -> 64 product on a plain source)
    ("t512_cat_128_to_64", 8, (64, 64), 64, 128, 128, 2, (16, 32, 64, 4, 1), (8, 32, 128, 4, 1), 8192),
    ("t512_dgrad_128_to_64", 8, (64,), 128, 72, 96, 1, (8, 16, 128, 2, 2), (16, 32, 64, 4, 1), 8192),
    # ---- the v_mfma_f32_16x16x32 build of the 256-pixel x 128-channel tiles (plain sources = the input gradients; also with
    # ustrun_debug_flags bit 15): wide rows, 16-pixel rows with ragged edges, the bottleneck, a 48 x 48 map
    ("m16_tall_wide_128", 8, (128,), 128, 128, 128, 2, (8, 32, 128, 4, 1), (8, 32, 128, 4, 1, "m16"), 32768),
    ("m16_tall_narrow_512", 16, (512,), 512, 56, 24, 1, (16, 16, 128, 4, 1), (16, 16, 128, 4, 1, "m16"), 32768),
    ("m16_bottleneck_n64", 64, (1024,), 1024, 16, 16, 4, (16, 16, 128, 4, 1), (16, 16, 128, 4, 1, "m16"), 32768),
    ("m16_cat_128_to_64", 8, (64, 64), 64, 128, 128, 2, (8, 32, 64, 2, 2), (8, 32, 128, 4, 1, "m16"), 32768),
    ("m16_pad_48_512", 16, (512,), 512, 48, 48, 2, (16, 16, 128, 4, 1), (16, 16, 128, 4, 1, "m16"), 32768),
]
# the default already runs the input gradients of the 256-pixel tiles on the 16x16x32 build: say so in the expectations above
CASES = [c[:8] + ((c[8] + ("m16",)) if (isinstance(c[8], tuple) and c[8][3] == 4 and c[8][4] == 1 and len(c[8]) == 5) else c[8],) + c[9:]
         for c in CASES]
# bit 15: EVERY plain-source tile on the 16x16x32 build -- the input gradients of the 64-column / two-taps-per-stage / small-grid
# tiles too (the forward reads through BatchNorm + ReLU: it stays on 32x32x16, the transforming variants are not built on 16x16x32)
for _c in list(CASES):
    if _c[0] in ("tall_wide_128", "cat_128_to_64", "tall_narrow_512", "c64_wide", "c64_narrow", "mid_grid_512", "pad_18_1024", "pad_144_128"):
        tag = lambda v: v if not isinstance(v, tuple) or (len(v) > 5 and v[5] == "m16") else v[:5] + ("m16",)
        _f = _c[9] if len(_c) > 9 else 0
        CASES.append(("m16all_" + _c[0],) + _c[1:7] + (_c[7], tag(_c[8]), (32768 | _f[0], _f[1]) if isinstance(_f, tuple) else 32768 | _f))
# ---- linear tiles (round 5, conv_halo_bf16.hip LINW: VERDICT r4 next 4): the maps of configs[2] / configs[3] whose sides no
# rectangular tile divides -- 18 / 36 / 72 pixels (M&Ms 288 x 288, train_mnms.py:397-399), 24 (prostate 384 x 384, train.py:416-418).
# A tile is 256 consecutive positions of a pass's flat padded space: tiles cross rows and images (never passes), the last tile of a
# pass is partial, pad positions are computed and dropped.  Forward through BatchNorm + ReLU on load (32x32x16 build) with
# statistics, input gradient on the 16x16x32 build; a two-source concat with an offset window and the two-destination input
# gradient; a map with H != W in one pass
LIN = lambda w: ("lin", w, 128, 4, 1)
CASES += [
    ("lin_18_1024", 64, (1024,), 1024, 18, 18, 4, LIN(18), LIN(18)),
    ("lin_24_1024", 64, (1024,), 1024, 24, 24, 4, LIN(24), LIN(24)),
    ("lin_36_512", 20, (512,), 512, 36, 36, 4, LIN(36), LIN(36)),
    ("lin_72_256", 8, (256,), 256, 72, 72, 2, LIN(72), LIN(72)),
    ("lin_cat_36", 24, (128, 128), 256, 36, 36, 2, LIN(36), LIN(36)),
    ("lin_18x20_512", 48, (512,), 512, 20, 18, 1, LIN(18), LIN(18)),
    # a plain first source that still carries the pass structure (the pooled operand of a Down block in a batched call): the
    # statistics rows must split by pass although no constants are read
    ("plain_lin_24_512", 30, (512,), 1024, 24, 24, 3, LIN(24), LIN(24)),
    ("plain_lin_cat_36", 24, (128, 128), 256, 36, 36, 2, LIN(36), LIN(36)),
]

WS_CODE = {"ws4": 0x57530000, "ws8": 0x57530100, "ws": 0x57530200,      # four waves / eight waves / consumer + producer waves (default)
           "wsf": 0x57530A00}                                             # ... on the flat plan


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_production_tile_exact(case):
    name, n, cs, co, h, w, G, vf, vd = case[:9]
    l = L()
    lib = l.lib()
    fl = case[9] if len(case) > 9 else {"ws4": 2, "ws8": 4}.get(vf, 0)
    f1, f2 = fl if isinstance(fl, tuple) else (fl, 0)
    old_flags, old_flags2 = lib.ustrun_debug_flags(f1), lib.ustrun_debug_flags2(f2)
    try:
        _production_tile_exact(l, lib, name, n, cs, co, h, w, G, vf, vd)
    finally:
        lib.ustrun_debug_flags(old_flags)
        lib.ustrun_debug_flags2(old_flags2)


def _production_tile_exact(l, lib, name, n, cs, co, h, w, G, vf, vd):
    g = torch.Generator().manual_seed(len(name) * 131 + n)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    ci = sum(cs)
    gn = n // G
    # source 0: raw conv output with per-pass BatchNorm affine + ReLU on load; source 1 (concat): a plain tensor of smaller
    # extent placed at an offset (F.pad of unet_parts.py:62-63)
    y0 = ri(-3, 3, n, cs[0], h, w)
    sc = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (G, cs[0]), generator=g)]
    sh = ri(-1, 1, G, cs[0])
    scn = sc.repeat_interleave(gn, 0)[:, :, None, None]
    shn = sh.repeat_interleave(gn, 0)[:, :, None, None]
    a0 = torch.relu(y0 * scn + shn)
    acts, srcs, keep = [a0], [], []
    aff = torch.zeros(G, 4, cs[0])
    aff[:, 0], aff[:, 1] = sc, sh
    affg = aff.cuda()
    y0g = nhwc16(y0)
    keep += [affg, y0g]
    plain = name.startswith("plain_")      # source 0 as a finished activation (a pooled / materialised operand): no constants, but passes
    if plain:
        a0g = nhwc16(a0)
        keep.append(a0g)
        srcs.append(l.nhwc_src(a0g.data_ptr(), cs[0], h, w, gN=gn if G > 1 else 0, gstride=4 * cs[0]))
    else:
        srcs.append(l.nhwc_src(y0g.data_ptr(), cs[0], h, w, affg.data_ptr(), affg.data_ptr() + 4 * cs[0], relu=1,
                               gN=gn if G > 1 else 0, gstride=4 * cs[0]))
    if len(cs) == 2:
        uh, uw, oy, ox = h - 2, w - 4, 1, 2
        u = ri(-3, 3, n, cs[1], uh, uw)
        acts.append(F.pad(u, [ox, w - uw - ox, oy, h - uh - oy]))
        ug = nhwc16(u)
        keep.append(ug)
        srcs.append(l.nhwc_src(ug.data_ptr(), cs[1], uh, uw, off=(oy, ox)))
    a = torch.cat(acts, 1).requires_grad_(True)
    wt = ri(-2, 2, co, ci, 3, 3)
    wr = wt.clone().requires_grad_(True)
    dy = ri(-2, 2, n, co, h, w)
    ref = F.conv2d(a, wr, None, 1, 1)
    ref.backward(dy)
    assert float(ref.detach().abs().max()) < 2 ** 24 and float(wr.grad.abs().max()) < 2 ** 24      # f32 sums stay exact

    wf, wd = pack16(wt)
    sarr = (l.Src * len(srcs))(*srcs)
    # output and statistics rows between sentinel zones (nothing outside the tensor / the rows the call reports is written)
    ZO = 8192
    obuf = torch.full((ZO + n * h * w * co + ZO,), 9.0, device="cuda", dtype=E.t)
    out = obuf[ZO:ZO + n * h * w * co].view(n, h, w, co)
    rows_max = lib.ustrun_conv_mtiles(n, h, w, co)
    stat = torch.full((rows_max + 64, 2, co), 5.0, device="cuda")
    rows = C.c_int(0)
    l.check(lib.ustrun_conv3x3_fwd_rows(sarr, len(srcs), wf.data_ptr(), n, h, w, co, out.data_ptr(), stat.data_ptr(),
                                        C.byref(rows), E.code, None), "fwd")
    got = lib.ustrun_debug_last_conv_variant()
    assert got == (WS_CODE[vf] | 1 if vf in WS_CODE else variant(*vf, False, not plain)), f"forward ran {vstr(got)}"
    yc = from_nhwc(out.float())
    assert rel(yc, r16(ref.detach())) < 1e-6
    # statistics rows: per pass, sums of the STORED (bf16-rounded) outputs
    assert rows.value % G == 0 and rows.value <= rows_max
    assert bool((stat[rows.value:] == 5.0).all()), "statistics rows written beyond the count the call reported"
    assert bool((obuf[:ZO] == 9.0).all()) and bool((obuf[-ZO:] == 9.0).all()), "forward wrote outside its output"
    st = stat[:rows.value].view(G, rows.value // G, 2, co).double().sum(1).cpu()
    ys = yc.double().view(G, gn, co, h, w)
    # (integer outputs: the 128-pixel f32 partial sums of y are exact; those of y^2 round, all terms positive)
    assert float((st[:, 0] - ys.sum((1, 3, 4))).abs().max()) <= 1e-6 * float(ys.abs().sum((1, 3, 4)).max())
    np.testing.assert_allclose(st[:, 1].numpy(), ys.square().sum((1, 3, 4)).numpy(), rtol=1e-5)

    # input gradient: whole, then split into [source 0 | source 1 window]
    dyg = nhwc16(dy)
    dbuf = torch.full((ZO + n * h * w * ci + ZO,), 9.0, device="cuda", dtype=E.t)
    da = dbuf[ZO:ZO + n * h * w * ci].view(n, h, w, ci)
    l.check(lib.ustrun_conv3x3_dgrad(dyg.data_ptr(), wd.data_ptr(), n, h, w, co, ci, da.data_ptr(), ci, None, 0, 0, 0, 0, E.code, None), "dgrad")
    got = lib.ustrun_debug_last_conv_variant()
    assert got == (WS_CODE[vd] if vd in WS_CODE else variant(*vd, False, False)), f"input gradient ran {vstr(got)}"
    assert rel(from_nhwc(da.float()), r16(a.grad)) < 1e-6
    assert bool((dbuf[:ZO] == 9.0).all()) and bool((dbuf[-ZO:] == 9.0).all()), "input gradient wrote outside its output"
    if len(cs) == 2:
        d0 = torch.empty(n, h, w, cs[0], device="cuda", dtype=E.t)
        d1 = torch.full((n, uh, uw, cs[1]), 7.0, device="cuda", dtype=E.t)
        l.check(lib.ustrun_conv3x3_dgrad(dyg.data_ptr(), wd.data_ptr(), n, h, w, co, ci, d0.data_ptr(), cs[0], d1.data_ptr(),
                                         uh, uw, oy, ox, E.code, None), "dgrad split")
        assert lib.ustrun_debug_last_conv_variant() == variant(*vd, False, False)
        assert rel(from_nhwc(d0.float()), r16(a.grad[:, :cs[0]])) < 1e-6
        assert rel(from_nhwc(d1.float()), r16(a.grad[:, cs[0]:, oy:oy + uh, ox:ox + uw])) < 1e-6

    # weight gradient (all nine taps per block, split-K slabs + fixed-order reduce), then accumulated a second time
    nb = lib.ustrun_wgrad_partials_bytes(9, ci, co, n * h * w)
    part = torch.empty(nb // 4, device="cuda")
    dw = torch.empty(co, ci, 3, 3, device="cuda")
    l.check(lib.ustrun_conv3x3_wgrad(sarr, len(srcs), dyg.data_ptr(), n, h, w, co, dw.data_ptr(), 0, part.data_ptr(), nb, E.code, None), "wgrad")
    assert rel(dw.cpu(), wr.grad) < 1e-6
    l.check(lib.ustrun_conv3x3_wgrad(sarr, len(srcs), dyg.data_ptr(), n, h, w, co, dw.data_ptr(), 1, part.data_ptr(), nb, E.code, None), "wgrad acc")
    assert rel(dw.cpu(), 2 * wr.grad) < 1e-6


def test_linear_tiles_shorter_last_pass_exact():
    """Linear tiles with a last pass shorter than the others (the student's batched call: G passes of B images + the one-image
    low-quality pass, ustrun_unet_desc_t::tail): 4 x 5 + 2 images of 36 x 36, 512 -> 512; the last pass has its own tile count, its
    BatchNorm constants, and its statistics rows at the end (the count ustrun_unet_forward splits them by is checked through the
    per-pass sums)."""
    l = L()
    lib = l.lib()
    n, gn, c, h, w = 22, 5, 512, 36, 36
    G = (n + gn - 1) // gn
    g = torch.Generator().manual_seed(77)
    ri = lambda lo, hi, *s_: torch.randint(lo, hi + 1, s_, generator=g).float()
    y0 = ri(-3, 3, n, c, h, w)
    sc = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (G, c), generator=g)]
    sh = ri(-1, 1, G, c)
    scn = sc.repeat_interleave(gn, 0)[:n, :, None, None]
    shn = sh.repeat_interleave(gn, 0)[:n, :, None, None]
    a0 = torch.relu(y0 * scn + shn)
    wt = ri(-2, 2, c, c, 3, 3)
    ref = F.conv2d(a0, wt, None, 1, 1)
    assert float(ref.abs().max()) < 2 ** 24
    aff = torch.zeros(G, 4, c)
    aff[:, 0], aff[:, 1] = sc, sh
    affg, y0g = aff.cuda(), nhwc16(y0)
    src = l.nhwc_src(y0g.data_ptr(), c, h, w, affg.data_ptr(), affg.data_ptr() + 4 * c, relu=1, gN=gn, gstride=4 * c)
    sarr = (l.Src * 1)(src)
    wf, _ = pack16(wt)
    ZO = 8192
    obuf = torch.full((ZO + n * h * w * c + ZO,), 9.0, device="cuda", dtype=E.t)
    out = obuf[ZO:ZO + n * h * w * c].view(n, h, w, c)
    rows_max = lib.ustrun_conv_mtiles(n, h, w, c)
    stat = torch.full((rows_max + 64, 2, c), 5.0, device="cuda")
    rows = C.c_int(0)
    # a shorter last pass is an error through the operator API unless the caller declares it
    assert lib.ustrun_conv3x3_fwd_rows(sarr, 1, wf.data_ptr(), n, h, w, c, out.data_ptr(), stat.data_ptr(), C.byref(rows), E.code, None) != 0
    assert b"inconsistent pass groups" in lib.ustrun_last_error()
    assert lib.ustrun_short_last_pass(1) == 0
    try:
        l.check(lib.ustrun_conv3x3_fwd_rows(sarr, 1, wf.data_ptr(), n, h, w, c, out.data_ptr(), stat.data_ptr(), C.byref(rows), E.code, None), "fwd")
    finally:
        assert lib.ustrun_short_last_pass(0) == 1
    assert lib.ustrun_debug_last_conv_variant() == variant("lin", 36, 128, 4, 1, False, True), vstr(lib.ustrun_debug_last_conv_variant())
    yc = from_nhwc(out.float())
    assert rel(yc, r16(ref)) < 1e-6
    assert bool((obuf[:ZO] == 9.0).all()) and bool((obuf[-ZO:] == 9.0).all()) and bool((stat[rows.value:] == 5.0).all())
    per = lambda imgs: -(-imgs * (h + 1) * (w + 1) // 256)
    assert rows.value == (G - 1) * per(gn) + per(n - (G - 1) * gn)
    r0 = 0
    for p_ in range(G):
        imgs = min(gn, n - p_ * gn)
        st = stat[r0:r0 + per(imgs)].double().sum(0).cpu()
        r0 += per(imgs)
        ys = yc[p_ * gn:p_ * gn + imgs].double()
        assert float((st[0] - ys.sum((0, 2, 3))).abs().max()) <= 1e-6 * float(ys.abs().sum((0, 2, 3)).max())
        np.testing.assert_allclose(st[1].numpy(), ys.square().sum((0, 2, 3)).numpy(), rtol=1e-5)


# ustrun_debug_flags 512: the builds with weight tiles in LDS (convT_bf16_kernel<256, 32, 0> forward, <128, 64, 1> gradient at these sizes)
CONVT_BATCHED_CASES = [
    # (N, passes, Cin, Cout, H, W, flags)
    (8, 4, 128, 64, 24, 40, 0),              # the full-resolution level's channel plan, four batched passes, 60 tiles
    (6, 2, 256, 128, 20, 24, 0),             # 4 K chunks forward / 8 in the gradient, two N tiles forward, a ragged last tile
    (3, 1, 512, 256, 9, 11, 0),              # odd extents, M % 128 != 0, 8 K chunks forward / 16 in the gradient
    (8, 2, 128, 64, 128, 128, 0),            # the full-resolution level of the U-Net at its natural extent: 1024 tiles
    (6, 2, 256, 128, 20, 24, 512),
    (3, 1, 512, 256, 9, 11, 512),
]


def convT_batched_variants(flags):
    """(forward, input gradient) codes: 'CT' | register-fed weights | BN/32 | BK/32 | MODE -- 256 columns forward, 128 in the gradient
    (none of these launches has the 512 blocks of 256 columns the wide gradient tile asks for)"""
    breg = 0 if flags & 512 else 0x1000
    return 0x43540000 | breg | 8 << 8 | (1 if flags & 512 else 2) << 4, 0x43540000 | breg | 4 << 8 | 2 << 4 | 1


@pytest.mark.parametrize("n,G,ci,co,h,w,flags", CONVT_BATCHED_CASES,
                         ids=["-".join(str(v) for v in (c[:6] if c[6] == 0 else c)) for c in CONVT_BATCHED_CASES])
def test_convT_bf16_batched_passes_exact(n, G, ci, co, h, w, flags):
    """ConvTranspose forward with per-pass BatchNorm constants on its source (the producer's raw output), its input gradient and
    its weight gradient over the batched passes; outputs between sentinel zones; the build each launch ran is asserted."""
    l = L()
    lib = l.lib()
    g = torch.Generator().manual_seed(77 + ci + h)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    gn = n // G
    y = ri(-3, 3, n, ci, h, w)
    sc = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (G, ci), generator=g)]
    sh = ri(-1, 1, G, ci)
    a = torch.relu(y * sc.repeat_interleave(gn, 0)[:, :, None, None] + sh.repeat_interleave(gn, 0)[:, :, None, None])
    wt, b = ri(-2, 2, ci, co, 2, 2), ri(-2, 2, co)
    du = ri(-2, 2, n, co, 2 * h, 2 * w)
    ar, wr, br = a.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.conv_transpose2d(ar, wr, br, stride=2)
    ref.backward(du)
    nel = 4 * ci * co
    wf = torch.zeros(nel, dtype=E.t, device="cuda")
    wd = torch.zeros(nel, dtype=E.t, device="cuda")
    wg = wt.cuda()
    l.check(lib.ustrun_pack_convT2x2(wg.data_ptr(), ci, co, wf.data_ptr(), wd.data_ptr(), E.code, None))
    aff = torch.zeros(G, 4, ci)
    aff[:, 0], aff[:, 1] = sc, sh
    affg, yg, bg, dug = aff.cuda(), nhwc16(y), b.cuda(), nhwc16(du)
    src = l.nhwc_src(yg.data_ptr(), ci, h, w, affg.data_ptr(), affg.data_ptr() + 4 * ci, relu=1, gN=gn if G > 1 else 0, gstride=4 * ci)
    Z = 4096
    ubuf = torch.full((Z + n * 4 * h * w * co + Z,), 9.0, device="cuda", dtype=E.t)
    u = ubuf[Z:Z + n * 4 * h * w * co].view(n, 2 * h, 2 * w, co)
    old_flags = lib.ustrun_debug_flags(flags)
    try:
        l.check(lib.ustrun_convT2x2_fwd(C.byref(src), wf.data_ptr(), bg.data_ptr(), n, h, w, co, u.data_ptr(), E.code, None))
        vf = lib.ustrun_debug_last_conv_variant()
        dbuf = torch.full((Z + n * h * w * ci + Z,), 9.0, device="cuda", dtype=E.t)
        da = dbuf[Z:Z + n * h * w * ci].view(n, h, w, ci)
        l.check(lib.ustrun_convT2x2_dgrad(dug.data_ptr(), wd.data_ptr(), n, h, w, co, ci, da.data_ptr(), E.code, None))
        vd = lib.ustrun_debug_last_conv_variant()
    finally:
        lib.ustrun_debug_flags(old_flags)
    assert (vf, vd) == convT_batched_variants(flags), (hex(vf), hex(vd))
    assert rel(from_nhwc(u.float()), r16(ref.detach())) < 1e-6
    assert rel(from_nhwc(da.float()), r16(ar.grad)) < 1e-6
    for b_ in (ubuf, dbuf):
        assert bool((b_[:Z] == 9.0).all()) and bool((b_[-Z:] == 9.0).all()), "wrote outside its output"
    nb = max(lib.ustrun_wgrad_partials_bytes(4, ci, co, n * h * w), 512 * co * 4)
    part = torch.empty(nb // 4, device="cuda")
    dw, db = torch.empty(ci, co, 2, 2, device="cuda"), torch.empty(co, device="cuda")
    l.check(lib.ustrun_convT2x2_wgrad(C.byref(src), dug.data_ptr(), n, h, w, co, dw.data_ptr(), db.data_ptr(), 0, part.data_ptr(), nb, E.code, None))
    assert rel(dw.cpu(), wr.grad) < 1e-6 and rel(db.cpu(), br.grad) < 1e-6


# ConvTranspose weight + bias gradient, the round-5 kernel (wgradT_bf16.hip: 256- / 128-ci x 256-column tiles, both operands by
# buffer-addressed LDS-DMA three stages deep).  Exact (integer data): rows of 16 pixels (a 32-pixel stage spans two image rows), 18 /
# 24 / 36 / 48 pixels (one or two wraps at changing positions: the M&Ms and prostate levels), pixel counts that are not a multiple of
# the stage, several ci tiles (only the first forms the bias sums), plain and transforming sources, batched passes, accumulation;
# the kernel that ran is asserted, the slabs' consumer (dw, db) sits between sentinel zones.
CONVT_WGRAD_CASES = [
    # (id, N, Cin, Cout, H, W, passes, transform, flags, expected variant)
    ("t256_w16", 4, 256, 128, 16, 16, 2, True, 0, 0x54320100),
    ("t256_w18_tail", 3, 512, 256, 18, 18, 1, True, 0, 0x54320100),
    ("t256_w24_plain", 2, 256, 64, 24, 24, 1, False, 0, 0x54320100),
    ("t256_w48", 2, 1024, 512, 12, 48, 1, True, 0, 0x54320100),
    ("t128_w36", 4, 128, 64, 36, 36, 2, True, 0, 0x54320080),
    ("t128_w144_tail", 1, 128, 64, 9, 144, 1, True, 0, 0x54320080),
    ("t128_w256", 2, 128, 64, 64, 256, 2, True, 0, 0x54320080),
    ("old_forced", 4, 256, 128, 16, 16, 2, True, 1 << 27, 0x54310000),
    ("old_w7", 2, 128, 64, 5, 7, 1, True, 0, 0x54310000),              # the round-1 kernel on its production routes: rows under 16 pixels,
    ("old_co96", 2, 128, 96, 16, 16, 2, True, 0, 0x54310000),          # ... and column tiles of 32 co
]


@pytest.mark.parametrize("name,n,ci,co,h,w,G,xf,flags,variant", CONVT_WGRAD_CASES, ids=[c[0] for c in CONVT_WGRAD_CASES])
def test_convT_weight_gradient_round5_kernel_exact(name, n, ci, co, h, w, G, xf, flags, variant):
    l = L()
    lib = l.lib()
    g = torch.Generator().manual_seed(31 + ci + w)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    gn = n // G
    y = ri(-3, 3, n, ci, h, w)
    du = ri(-2, 2, n, co, 2 * h, 2 * w)
    if xf:
        sc = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (G, ci), generator=g)]
        sh = ri(-1, 1, G, ci)
        a = torch.relu(y * sc.repeat_interleave(gn, 0)[:, :, None, None] + sh.repeat_interleave(gn, 0)[:, :, None, None])
    else:
        a = y
    wt = ri(-2, 2, ci, co, 2, 2)
    ar, wr, br = a.clone().requires_grad_(True), wt.clone().requires_grad_(True), torch.zeros(co, requires_grad=True)
    F.conv_transpose2d(ar, wr, br, stride=2).backward(du)
    yg, dug = nhwc16(y), nhwc16(du)
    if xf:
        aff = torch.zeros(G, 4, ci)
        aff[:, 0], aff[:, 1] = sc, sh
        affg = aff.cuda()
        src = l.nhwc_src(yg.data_ptr(), ci, h, w, affg.data_ptr(), affg.data_ptr() + 4 * ci, relu=1, gN=gn if G > 1 else 0, gstride=4 * ci)
    else:
        src = l.nhwc_src(yg.data_ptr(), ci, h, w, gN=gn if G > 1 else 0, gstride=4 * ci)
    nb = max(lib.ustrun_wgrad_partials_bytes(4, ci, co, n * h * w), 512 * co * 4)
    part = torch.full((nb // 4 + 1024,), 5.0, device="cuda")
    Z = 1024
    wbuf = torch.full((Z + 4 * ci * co + Z,), 9.0, device="cuda")
    bbuf = torch.full((Z + co + Z,), 9.0, device="cuda")
    dw, db = wbuf[Z:Z + 4 * ci * co].view(ci, co, 2, 2), bbuf[Z:Z + co]
    old = lib.ustrun_debug_flags(flags)
    try:
        l.check(lib.ustrun_convT2x2_wgrad(C.byref(src), dug.data_ptr(), n, h, w, co, dw.data_ptr(), db.data_ptr(), 0, part.data_ptr(), nb, E.code, None))
        v = lib.ustrun_debug_last_wgrad_variant()
        assert v == variant, (hex(v), hex(variant))
        assert rel(dw.cpu(), wr.grad) < 1e-6 and rel(db.cpu(), br.grad) < 1e-6, (rel(dw.cpu(), wr.grad), rel(db.cpu(), br.grad))
        l.check(lib.ustrun_convT2x2_wgrad(C.byref(src), dug.data_ptr(), n, h, w, co, dw.data_ptr(), db.data_ptr(), 1, part.data_ptr(), nb, E.code, None))
        assert rel(dw.cpu(), 2 * wr.grad) < 1e-6 and rel(db.cpu(), 2 * br.grad) < 1e-6
    finally:
        lib.ustrun_debug_flags(old)
    for b_ in (wbuf, bbuf):
        assert bool((b_[:Z] == 9.0).all()) and bool((b_[-Z:] == 9.0).all()), "wrote outside its output"
    assert bool((part[nb // 4:] == 5.0).all()), "slabs beyond the published partials bound"


# 3x3 weight gradient, the three builds of the all-taps kernel (wgrad_halo_bf16.hip): 0x482 = two wave groups in opposite phases
# (>= 256 channels: 16 (ci, co) pairs), 0x481 = buffer-addressed transfers, 256-thread blocks, 0x480 = the round-2 kernel (kept for
# operands beyond 2 GB per image; forced here with ustrun_debug_flags 64).  Exact (integer data), ragged extents, a source placed at
# an offset (zero padding through the buffer range check), batched passes with per-pass BatchNorm constants, odd tile counts (the
# two groups get unequal shares), every output between sentinel zones.
WGRAD_CASES = [
    # (id, N, source channels, Cout, H, W, groups, flags, expected variant family)
    ("pp_512", 6, (512,), 512, 24, 40, 2, 0, 0x482),
    ("pp_cat_256_256", 4, (256, 256), 256, 16, 24, 1, 0, 0x482),
    ("pp_odd_tiles", 3, (256,), 256, 24, 16, 1, 0, 0x482),
    ("pp_off_512", 6, (512,), 512, 24, 40, 2, 256, 0x481),
    ("buf_128", 4, (128,), 128, 40, 56, 2, 0, 0x481),
    ("buf_cat_64_64", 4, (64, 64), 64, 24, 40, 1, 0, 0x481),
    ("buf_rows4", 5, (128,), 64, 4, 24, 1, 0, 0x481),
    ("old_512", 6, (512,), 512, 24, 40, 2, 64, 0x480),
    # four-row tiles of the pointer-addressed build: three buffers, transfers two tiles ahead; 10 tiles in 2 slices of 5, so the
    # two-ahead pipeline fills and drains
    ("old_rows4", 5, (128,), 64, 4, 24, 1, 64, 0x480),
    # its concat: the second source at an offset with a smaller extent (the zero page)
    ("old_cat_64_64", 4, (64, 64), 64, 24, 40, 1, 64, 0x480),
    # the pooled kernel: the source is [4, 64, 23, 42] read through its 2x2 max window (pool on load), two passes
    ("pool_64_128", 4, (64,), 128, 11, 21, 2, 0, 0x480),
]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_wgrad_all_taps_builds_exact(case):
    name, n, cs, co, h, w, G, flags, fam = case
    l = L()
    lib = l.lib()
    g = torch.Generator().manual_seed(len(name) * 17 + n)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    ci, gn = sum(cs), n // G
    pool = name.startswith("pool_")          # the first source is pooled on load: stored at [2 h + 1, 2 w] (an odd row is dropped)
    sh_, sw_ = (2 * h + 1, 2 * w) if pool else (h, w)
    y0 = ri(-3, 3, n, cs[0], sh_, sw_)
    sc = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (G, cs[0]), generator=g)]
    sh = ri(-1, 1, G, cs[0])
    a0 = torch.relu(y0 * sc.repeat_interleave(gn, 0)[:, :, None, None] + sh.repeat_interleave(gn, 0)[:, :, None, None])
    if pool:
        a0 = F.max_pool2d(a0, 2)
    aff = torch.zeros(G, 4, cs[0])
    aff[:, 0], aff[:, 1] = sc, sh
    affg, y0g = aff.cuda(), nhwc16(y0)
    srcs = [l.nhwc_src(y0g.data_ptr(), cs[0], sh_, sw_, affg.data_ptr(), affg.data_ptr() + 4 * cs[0], relu=1, gN=gn if G > 1 else 0,
                       gstride=4 * cs[0], pool=int(pool))]
    acts, keep = [a0], [affg, y0g]
    if len(cs) == 2:
        uh, uw, oy, ox = h - 3, w - 5, 2, 3
        u = ri(-3, 3, n, cs[1], uh, uw)
        acts.append(F.pad(u, [ox, w - uw - ox, oy, h - uh - oy]))
        ug = nhwc16(u)
        keep.append(ug)
        srcs.append(l.nhwc_src(ug.data_ptr(), cs[1], uh, uw, off=(oy, ox)))
    a = torch.cat(acts, 1)
    dy = ri(-2, 2, n, co, h, w)
    wr = torch.zeros(co, ci, 3, 3, requires_grad=True)
    F.conv2d(a, wr, None, 1, 1).backward(dy)
    assert float(wr.grad.abs().max()) < 2 ** 24
    sarr = (l.Src * len(srcs))(*srcs)
    dyg = nhwc16(dy)
    nb = lib.ustrun_wgrad_partials_bytes(9, ci, co, n * h * w)
    part = torch.empty(nb // 4, device="cuda")
    Z = 4096
    buf = torch.full((Z + co * ci * 9 + Z,), 7.0, device="cuda")
    dw = buf[Z:Z + co * ci * 9]
    old = lib.ustrun_debug_flags(flags)
    try:
        l.check(lib.ustrun_conv3x3_wgrad(sarr, len(srcs), dyg.data_ptr(), n, h, w, co, dw.data_ptr(), 0, part.data_ptr(), nb, E.code, None), "wgrad")
        v = lib.ustrun_debug_last_wgrad_variant()
        l.check(lib.ustrun_conv3x3_wgrad(sarr, len(srcs), dyg.data_ptr(), n, h, w, co, dw.data_ptr(), 1, part.data_ptr(), nb, E.code, None), "wgrad acc")
    finally:
        lib.ustrun_debug_flags(old)
    assert (v >> 20) == fam, f"weight gradient ran variant {v:#x}"
    assert torch.equal(dw.view(co, ci, 3, 3).cpu(), 2 * wr.grad)
    assert bool((buf[:Z] == 7.0).all()) and bool((buf[-Z:] == 7.0).all())


@pytest.mark.parametrize("name,n,G,cin,cout,h,w,tile", [
    ("wide_128", 16, 2, 128, 128, 128, 128, (8, 32, 128, 4, 1, "m16")),       # 8 x 32 tiles, two passes
    ("narrow_512_ragged", 16, 1, 512, 512, 56, 40, (16, 16, 128, 4, 1, "m16")),   # 16 x 16 tiles, ragged right / bottom edges
    ("bottleneck", 64, 4, 1024, 512, 16, 16, (16, 16, 128, 4, 1, "m16")),     # N = 64, four passes, 512 -> 1024 channels back
    ("too_small", 2, 1, 128, 128, 32, 32, None),
    # linear tiles (round 5): 18 x 18 at the bottleneck's width, four passes; 36 x 36 with a partial last tile per pass
    ("lin_18", 64, 4, 1024, 512, 18, 18, ("lin", 18, 128, 4, 1)),
    ("lin_36", 20, 4, 512, 512, 36, 36, ("lin", 36, 128, 4, 1)),                                # a grid the fused epilogue does not cover: rows = 0, no launch
    # the 64 -> 64 streaming kernel (consumer / producer build; the sums ride on the producers' stores): two passes; then four
    # passes on a ragged map (9 row-steps in segments, 2.5 strips of 32 px)
    ("ws64_n8_128", 8, 2, 64, 64, 128, 128, "ws"),
    ("ws64_ragged", 16, 4, 64, 64, 72, 80, "ws"),
    # the same build on the flat plan (260 strips of 8 steps -> 9 per block): sums of pieces cut mid-strip, the zero rows of uncut strips
    ("ws64f_130_64", 130, 2, 64, 64, 64, 64, "wsf"),
])
def test_input_gradient_with_batchnorm_backward_sums_exact(name, n, G, cin, cout, h, w, tile):
    """ustrun_conv3x3_dgrad_bnsum (round 4): the input gradient of a DoubleConv's second convolution IS da of the BatchNorm + ReLU
    between the two convolutions (unet_parts.py:17-21); the 16x16x32 epilogue loads y beside each stored da piece and writes
    sum(da mask), sum(da mask y) as statistics rows instead of leaving them to a reduce pass.  Small-integer data: da must equal the
    plain input gradient BITWISE, the rows' per-pass column sums must equal torch's exactly, nothing may be written outside the rows
    the call reports; then ustrun_bn_bwd_finalize_stat against ustrun_bn_bwd_reduce on the same tensors (dgamma, dbeta, coef)."""
    l = L()
    lib = l.lib()
    g = torch.Generator().manual_seed(len(name) * 17 + n)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    gn = n // G
    wt = ri(-1, 1, cout, cin, 3, 3)          # conv: cin -> cout; its input gradient maps dy [cout] back to da [cin]
    dy = ri(-1, 1, n, cout, h, w)
    y = ri(-3, 3, n, cin, h, w) * 0.5        # the previous layer's pre-BatchNorm output (halves: exact in 16 bits)
    sc = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (G, cin), generator=g)]
    sh = ri(-1, 1, G, cin) * 0.25            # (never makes y sc + sh exactly 0 for y a multiple of 0.5 ... unless both vanish: excluded below)
    sh[sh == 0] = 0.25
    aff = torch.zeros(G, 4, cin)
    aff[:, 0], aff[:, 1] = sc, sh
    aff[:, 2], aff[:, 3] = ri(-1, 1, G, cin) * 0.5, torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (G, cin), generator=g)]      # mean, rstd
    gamma = ri(1, 3, cin) * 0.5
    da_ref = F.conv_transpose2d(dy, wt, None, 1, 1)          # = conv input gradient
    assert float(da_ref.abs().max()) < 256
    wf, wd = pack16(wt)
    dyg, yg, affg = nhwc16(dy), nhwc16(y), aff.cuda()
    ZO = 8192
    dbuf = torch.full((ZO + n * h * w * cin + ZO,), 9.0, device="cuda", dtype=E.t)
    da = dbuf[ZO:ZO + n * h * w * cin].view(n, h, w, cin)
    rows_max = lib.ustrun_conv_mtiles(n, h, w, cin)
    stat = torch.full((rows_max + 64, 2, cin), 5.0, device="cuda")
    rows = C.c_int(-1)
    l.check(lib.ustrun_conv3x3_dgrad_bnsum(dyg.data_ptr(), wd.data_ptr(), n, h, w, cout, cin, da.data_ptr(), yg.data_ptr(),
                                           affg.data_ptr(), affg.data_ptr() + 4 * cin, gn if G > 1 else 0, 4 * cin, stat.data_ptr(),
                                           C.byref(rows), E.code, None), "dgrad_bnsum")
    if tile is None:
        assert rows.value == 0 and bool((dbuf == 9.0).all()) and bool((stat == 5.0).all()), "an unsupported shape must not launch"
        return
    assert rows.value > 0 and rows.value % G == 0 and rows.value <= rows_max
    if tile in ("ws", "wsf"):         # 'WS' | consumer/producer | sums, | 0x800 on the flat plan
        assert lib.ustrun_debug_last_conv_variant() == {"ws": 0x57530600, "wsf": 0x57530E00}[tile], hex(lib.ustrun_debug_last_conv_variant())
    else:
        assert lib.ustrun_debug_last_conv_variant() == variant(*tile, False, False), vstr(lib.ustrun_debug_last_conv_variant())
    plain = torch.empty(n, h, w, cin, device="cuda", dtype=E.t)
    l.check(lib.ustrun_conv3x3_dgrad(dyg.data_ptr(), wd.data_ptr(), n, h, w, cout, cin, plain.data_ptr(), cin, None, 0, 0, 0, 0, E.code, None), "dgrad")
    assert torch.equal(da, plain) and rel(from_nhwc(da.float()), da_ref) < 1e-6
    assert bool((dbuf[:ZO] == 9.0).all()) and bool((dbuf[-ZO:] == 9.0).all()) and bool((stat[rows.value:] == 5.0).all())
    scn, shn = sc.repeat_interleave(gn, 0)[:, :, None, None], sh.repeat_interleave(gn, 0)[:, :, None, None]
    dz = torch.where(y * scn + shn > 0, da_ref, torch.zeros(()))
    st = stat[:rows.value].view(G, rows.value // G, 2, cin).double().sum(1).cpu()
    assert torch.equal(st[:, 0], dz.double().view(G, gn, cin, h, w).sum((1, 3, 4)))
    assert torch.equal(st[:, 1], (dz * y).double().view(G, gn, cin, h, w).sum((1, 3, 4)))
    # the finalize over these rows against the reduce pass + its finalize on the same tensors
    gam, mean, rstd = gamma.cuda(), affg[:, 2].contiguous(), affg[:, 3].contiguous()
    out = {}
    for kind in ("rows", "pass"):
        dg, db, coef = torch.zeros(cin, device="cuda"), torch.zeros(cin, device="cuda"), torch.zeros(G, 3, cin, device="cuda")
        if kind == "rows":
            l.check(lib.ustrun_bn_bwd_finalize_stat(stat.data_ptr(), rows.value // G, G, cin, gn * h * w, gam.data_ptr(), affg.data_ptr() + 8 * cin,
                                                    affg.data_ptr() + 12 * cin, 4 * cin, dg.data_ptr(), db.data_ptr(), 0, coef.data_ptr(), None), "finalize_stat")
        else:
            pb = lib.ustrun_bn_bwd_partials_bytes(gn * h * w, cin)
            part = torch.empty(pb // 4, device="cuda")
            for p_ in range(G):          # the public reduce entry point takes one pass per call
                sl = slice(p_ * gn, (p_ + 1) * gn)
                l.check(lib.ustrun_bn_bwd_reduce(da[sl].data_ptr(), None, yg[sl].data_ptr(), affg[p_, 0].data_ptr(), affg[p_, 1].data_ptr(),
                                                 affg[p_, 2].data_ptr(), affg[p_, 3].data_ptr(), gam.data_ptr(), gn, h, w, cin, dg.data_ptr(),
                                                 db.data_ptr(), 1 if p_ else 0, coef[p_].data_ptr(), part.data_ptr(), pb, E.code, None), "bn_bwd_reduce")
        out[kind] = (dg.cpu(), db.cpu(), coef.cpu())
    for a_, b_ in zip(out["rows"], out["pass"]):
        np.testing.assert_allclose(a_.numpy(), b_.numpy(), rtol=2e-6, atol=1e-6)


@pytest.mark.parametrize("name,n,G,cin,cout,h,w,code", [
    ("up4_like", 8, 2, 128, 64, 64, 64, 0x43541000 | (128 // 32) << 8 | 2 << 4 | 1),      # da [.,64,64,128]: the 128-column build
    ("up1_like", 64, 4, 1024, 512, 16, 16, 0x43541000 | (256 // 32) << 8 | 2 << 4 | 1),   # N = 64: 512 blocks of 256 columns
    ("ragged_m", 3, 1, 256, 128, 20, 24, 0x43541000 | (128 // 32) << 8 | 2 << 4 | 1),     # M = 1440: a last tile of 32 pixels
    ("pass_straddles_tile", 6, 2, 128, 64, 10, 12, None),                                 # 3 x 120 pixels per pass: not covered, no launch
])
def test_convT_input_gradient_with_batchnorm_backward_sums_exact(name, n, G, cin, cout, h, w, code):
    """ustrun_convT2x2_dgrad_bnsum: the ConvTranspose's input gradient IS da of the conv2 one level down (unet_parts.py:56-68 into
    17-21); its epilogue forms that layer's BatchNorm-backward sums from the stored pieces and y, one row per 128-pixel tile.
    Integer data: da bitwise equal to the plain input gradient, per-pass column sums equal to torch's, no write outside the rows."""
    l = L()
    lib = l.lib()
    g = torch.Generator().manual_seed(len(name) * 23 + n)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    gn = n // G
    wt = ri(-1, 1, cin, cout, 2, 2)          # ConvTranspose2d(cin, cout, 2, 2): u = convT(a); da = conv2d(du, wt, stride 2)
    du = ri(-1, 1, n, cout, 2 * h, 2 * w)
    y = ri(-3, 3, n, cin, h, w) * 0.5
    sc = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (G, cin), generator=g)]
    sh = ri(-1, 1, G, cin) * 0.25
    sh[sh == 0] = 0.25
    aff = torch.zeros(G, 4, cin)
    aff[:, 0], aff[:, 1] = sc, sh
    da_ref = F.conv2d(du, wt, None, 2)
    assert float(da_ref.abs().max()) < 256
    nel = 4 * cin * cout
    wf, wd = torch.zeros(nel, dtype=E.t, device="cuda"), torch.zeros(nel, dtype=E.t, device="cuda")
    wg = wt.cuda()
    l.check(lib.ustrun_pack_convT2x2(wg.data_ptr(), cin, cout, wf.data_ptr(), wd.data_ptr(), E.code, None))
    dug, yg, affg = nhwc16(du), nhwc16(y), aff.cuda()
    ZO = 8192
    dbuf = torch.full((ZO + n * h * w * cin + ZO,), 9.0, device="cuda", dtype=E.t)
    da = dbuf[ZO:ZO + n * h * w * cin].view(n, h, w, cin)
    rows_max = lib.ustrun_conv_mtiles(n, h, w, cin)
    stat = torch.full((rows_max + 64, 2, cin), 5.0, device="cuda")
    rows = C.c_int(-1)
    l.check(lib.ustrun_convT2x2_dgrad_bnsum(dug.data_ptr(), wd.data_ptr(), n, h, w, cout, cin, da.data_ptr(), yg.data_ptr(), affg.data_ptr(),
                                            affg.data_ptr() + 4 * cin, gn if G > 1 else 0, 4 * cin, stat.data_ptr(), C.byref(rows), E.code, None),
            "convT_dgrad_bnsum")
    if code is None:
        assert rows.value == 0 and bool((dbuf == 9.0).all()) and bool((stat == 5.0).all())
        return
    assert rows.value == (n * h * w + 127) // 128 and rows.value <= rows_max
    assert lib.ustrun_debug_last_conv_variant() == code, hex(lib.ustrun_debug_last_conv_variant())
    plain = torch.empty(n, h, w, cin, device="cuda", dtype=E.t)
    l.check(lib.ustrun_convT2x2_dgrad(dug.data_ptr(), wd.data_ptr(), n, h, w, cout, cin, plain.data_ptr(), E.code, None), "convT_dgrad")
    assert torch.equal(da, plain) and rel(from_nhwc(da.float()), da_ref) < 1e-6
    assert bool((dbuf[:ZO] == 9.0).all()) and bool((dbuf[-ZO:] == 9.0).all()) and bool((stat[rows.value:] == 5.0).all())
    scn, shn = sc.repeat_interleave(gn, 0)[:, :, None, None], sh.repeat_interleave(gn, 0)[:, :, None, None]
    dz = torch.where(y * scn + shn > 0, da_ref, torch.zeros(()))
    assert rows.value % G == 0
    st = stat[:rows.value].view(G, rows.value // G, 2, cin).double().sum(1).cpu()
    assert torch.equal(st[:, 0], dz.double().view(G, gn, cin, h, w).sum((1, 3, 4)))
    assert torch.equal(st[:, 1], (dz * y).double().view(G, gn, cin, h, w).sum((1, 3, 4)))
