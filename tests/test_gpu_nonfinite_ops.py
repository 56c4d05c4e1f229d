"""inf and NaN through the 3x3 convolution family, one C-ABI call at a time, against float64 (tests/nonfinite_ref.py).

What a dynamic loss scale needs of every kernel between the loss and the flat gradient buffer:
  gate 1  storage overflow: an exact f32 sum of 65504 / 65519 is stored as 65504, 65520 / 2096128 as +inf (the mirrored channel: -inf),
          as Tensor.half() stores them -- not saturated, not zeroed; the statistics rows of those channels are non-finite, the rows of
          every other channel equal, bit for bit, those of a run in which those channels' weights are zero;
  gate 2  propagation: where the float64 result is +inf / -inf / NaN (0 * inf at the zero weights of the integer weight tensor
          included), the device result has the same class;
  gate 3  containment: every element whose float64 class is finite equals the storage-rounded float64 value to the bit (small
          integers: exact), sentinel zones stay whole, the statistics rows of an untouched pass equal the clean run's bit for bit, the
          split-K slabs start out as NaN;
  gate 4  NaN of either sign in an operand that goes through the ReLU of the transforming loader: the outputs equal the float64
          result under the "torch" convention (NaN propagates) or under "select" (x > 0 ? x : 0); which one is printed (pytest -s)
          and recorded in DESIGN.md.  Anything else fails.
No tolerance anywhere: class equality, then bit equality.

Entries of the first half: ustrun_conv3x3_fwd_rows (transforming loader: BatchNorm affine + ReLU on load, two-source concat with an offset window,
two batched passes, statistics rows), ustrun_conv3x3_dgrad (plain loader, whole and split over two destinations),
ustrun_conv3x3_wgrad.  Families, each asserted by its variant code: the halo kernel's 16 x 16 x 64, 8 x 16 x 64 and 8 x 32 x 64 tiles,
its linear tiles (forward on 32x32x16 MFMAs, input gradient on the 16x16x32 build; 30 images of 18 x 18 with 32 <-> 512 channels is
the smallest launch that keeps 160 tile-columns), the 64 -> 64 streaming kernel (8 x 64 x 60 x 70: 192 items, its threshold), the
generic implicit GEMM (1 x 24 -> 40 x 9 x 7: channel tails), the all-taps weight gradient (and the generic one where a source has
fewer than 64 channels).

Special values go only into floating operands of arithmetic (raw convolution outputs, activations, gradients).  The kernels called
here convert none of them to an index: sources are read through ld / buffer loads at integer coordinates, BatchNorm constants are
multiplied and added (csrc/loader.h, conv_halo_bf16.hip, conv_ws64_bf16.hip, igemm_bf16.hip, wgrad_halo_bf16.hip, wgrad_tap_bf16.hip).

The second half of the file holds the ConvTranspose trio, the head, ustrun_pool_act and the first convolution's forward and input
gradient to the same gates (gate 1 included for every 16-bit store: ConvTranspose forward and input gradient, the pooled activation,
the split input gradient).  test_conv_first_nonfinite calls ustrun_conv3x3_wgrad on the NCHW image, the stand-alone first-layer weight
gradient; the one the training step runs, ustrun_conv_first_wgrad_bn, is in tests/test_gpu_nonfinite_bn_ops.py with the BatchNorm
kernels, the dgrad_bnsum epilogues and the loss gradient's device-side scale.  No case was dropped for a float-to-index conversion."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import nonfinite_ref as NF
from test_gpu_production_tiles import L, variant, vstr

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
TDT = {"bf16": (torch.bfloat16, 1), "f16": (torch.float16, 2)}
NAN_BITS = {"f16": {"+nan": 0x7E00, "-nan": 0xFE00 - 0x10000}, "bf16": {"+nan": 0x7FC0, "-nan": 0xFFC0 - 0x10000}}
ZO = 8192
WS = 0x57530200          # the streaming kernel, consumer / producer build (| 1: transforming loader)


def nhwc16(t, elt):
    return t.permute(0, 2, 3, 1).contiguous().cuda().to(TDT[elt][0])


def from_nhwc(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def pack16(w, elt):
    l = L()
    co, ci = w.shape[:2]
    n = 9 * ((ci + 7) // 8 * 8) * ((co + 7) // 8 * 8)
    wf = torch.zeros(n, dtype=TDT[elt][0], device="cuda")
    wd = torch.zeros(n, dtype=TDT[elt][0], device="cuda")
    wg = w.contiguous().cuda()
    l.check(l.lib().ustrun_pack_conv3x3(wg.data_ptr(), co, ci, wf.data_ptr(), wd.data_ptr(), TDT[elt][1], None))
    return wf, wd


def plant(dev_nhwc, cpu_nchw, where, value, elt):
    """one special value into the stored operand (device, NHWC) and its CPU image (NCHW); NaNs by their bit pattern, sign included"""
    n, c, y, x = where
    if isinstance(value, str):
        dev_nhwc.view(torch.int16)[n, y, x, c] = NAN_BITS[elt][value]
        cpu_nchw[n, c, y, x] = NAN
    else:
        dev_nhwc[n, y, x, c] = value
        cpu_nchw[n, c, y, x] = value


def wgrad_in_range(a, dy):
    """dw[co, ci, ky, kx] = sum over the pixel pairs that both lie inside the image, tap by tap (float64 einsum).  torch's own
    convolution backward materialises the zero padding and multiplies it: next to an inf gradient at the border it reports 0 * inf =
    NaN for the taps whose activation lies in the padding, a product the operation's definition does not contain.  The kernels differ
    among themselves there (see weight_gradient_mismatches)."""
    n, ci, h, w = a.shape
    dw = torch.zeros(dy.shape[1], ci, 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            oy, ox = ky - 1, kx - 1
            y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
            dw[:, :, ky, kx] = torch.einsum("nchw,nkhw->kc", a[:, :, y0 + oy:y1 + oy, x0 + ox:x1 + ox], dy[:, :, y0:y1, x0:x1])
    return dw


def weight_gradient_mismatches(dev, ref64, axis):
    """The weight gradient is judged per channel line, as a BatchNorm statistic is: a bad activation in input channel c0 may touch
    only dw[:, c0] (axis 1), a bad gradient in output channel k0 only dw[k0] (axis 0).  Where the reference is non-finite the class
    must be the reference's; every line the reference leaves finite must hold its values to the bit.  Inside a poisoned line a finite
    reference entry is not compared: the all-taps kernel multiplies the poisoned operand with the masked-off (zero) partner of a
    border tap and stores NaN there, its 32-pixel-row builds and torch do not -- the line is lost to the step either way."""
    cls, val = NF.expect(ref64, "f32")
    g = dev.detach().cpu().double()
    gcls = NF.classify(g)
    other = tuple(d for d in range(4) if d != axis)
    line = (cls != NF.FINITE).sum(other, keepdim=True) > 0
    bad_c = (gcls != cls) & ((cls != NF.FINITE) | ~line)
    bad_v = (cls == NF.FINITE) & (gcls == NF.FINITE) & (g != val) & ~line
    text = "; ".join("%s: got %r, expected %r" % (tuple(i), float(g[tuple(i)]), float(val[tuple(i)])) for i in (bad_c | bad_v).nonzero()[:6].tolist())
    return int(bad_c.sum()), int(bad_v.sum()), text


class Conv:
    """one layer's operands on both sides: sources (source 0 a raw convolution output under per-pass BatchNorm affine + ReLU on load,
    source 1 a plain tensor of smaller extent at an offset), weights, the output's gradient; small integers, power-of-two scales"""

    def __init__(self, name, n, cs, co, h, w, G, elt, unit_affine=()):
        self.name, self.n, self.cs, self.co, self.h, self.w, self.G, self.elt = name, n, cs, co, h, w, G, elt
        g = torch.Generator().manual_seed(len(name) * 131 + n)
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        self.ci, self.gn = sum(cs), n // G
        self.y0 = ri(-3, 3, n, cs[0], h, w)
        self.sc = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (G, cs[0]), generator=g)]
        self.sh = ri(-1, 1, G, cs[0])
        for c in unit_affine:
            self.sc[:, c], self.sh[:, c] = 1.0, 0.0
        aff = torch.zeros(G, 4, cs[0])
        aff[:, 0], aff[:, 1] = self.sc, self.sh
        self.affg = aff.cuda()
        self.y0g = nhwc16(self.y0, elt)
        self.u = self.ug = None
        if len(cs) == 2:
            self.uh, self.uw, self.oy, self.ox = h - 2, w - 4, 1, 2
            self.u = ri(-3, 3, n, cs[1], self.uh, self.uw)
            self.ug = nhwc16(self.u, elt)
        self.wt = ri(-2, 2, co, self.ci, 3, 3)
        self.dy = ri(-2, 2, n, co, h, w)
        self.dyg = nhwc16(self.dy, elt)

    def srcs(self):
        l, cs = L(), self.cs
        s = [l.nhwc_src(self.y0g.data_ptr(), cs[0], self.h, self.w, self.affg.data_ptr(), self.affg.data_ptr() + 4 * cs[0], relu=1,
                        gN=self.gn if self.G > 1 else 0, gstride=4 * cs[0])]
        if self.u is not None:
            s.append(l.nhwc_src(self.ug.data_ptr(), cs[1], self.uh, self.uw, off=(self.oy, self.ox)))
        return (l.Src * len(s))(*s), len(s)

    def reference(self, convention="torch"):
        """float64: (forward, input gradient, weight gradient) from the operands as stored"""
        e = self.elt
        scn = self.sc.double().repeat_interleave(self.gn, 0)[:, :, None, None]
        shn = self.sh.double().repeat_interleave(self.gn, 0)[:, :, None, None]
        acts = [NF.stored(NF.relu(NF.stored(self.y0, e) * scn + shn, convention), e)]       # (the loader rounds the activation to the storage type)
        if self.u is not None:
            acts.append(F.pad(NF.stored(self.u, e), [self.ox, self.w - self.uw - self.ox, self.oy, self.h - self.uh - self.oy]))
        a = torch.cat(acts, 1).requires_grad_(True)
        dy = NF.stored(self.dy, e)
        out = F.conv2d(a, NF.stored(self.wt, e), None, 1, 1)
        out.backward(dy)
        return out.detach(), a.grad, wgrad_in_range(a.detach(), dy)

    # ---- the three calls; every output between sentinel zones / pre-filled with NaN where a kernel is said to overwrite
    def forward(self, wt=None):
        l, lib = L(), L().lib()
        n, h, w, co = self.n, self.h, self.w, self.co
        wf, _ = pack16(self.wt if wt is None else wt, self.elt)
        sarr, ns = self.srcs()
        obuf = torch.full((ZO + n * h * w * co + ZO,), 9.0, device="cuda", dtype=TDT[self.elt][0])
        out = obuf[ZO:ZO + n * h * w * co].view(n, h, w, co)
        rows_max = lib.ustrun_conv_mtiles(n, h, w, co)
        stat = torch.full((rows_max + 64, 2, co), 5.0, device="cuda")
        rows = C.c_int(0)
        l.check(lib.ustrun_conv3x3_fwd_rows(sarr, ns, wf.data_ptr(), n, h, w, co, out.data_ptr(), stat.data_ptr(), C.byref(rows),
                                            TDT[self.elt][1], None), "fwd")
        v = lib.ustrun_debug_last_conv_variant()
        assert rows.value % self.G == 0 and 0 < rows.value <= rows_max
        assert bool((stat[rows.value:] == 5.0).all()), "statistics rows written beyond the count the call reported"
        assert bool((obuf[:ZO] == 9.0).all()) and bool((obuf[-ZO:] == 9.0).all()), "forward wrote outside its output"
        return from_nhwc(out.float()), stat[:rows.value].view(self.G, rows.value // self.G, 2, co).cpu(), v

    def dgrad(self, split=False, wt=None):
        l, lib = L(), L().lib()
        n, h, w, co, ci, cs = self.n, self.h, self.w, self.co, self.ci, self.cs
        _, wd = pack16(self.wt if wt is None else wt, self.elt)
        t, code = TDT[self.elt]
        if not split:
            dbuf = torch.full((ZO + n * h * w * ci + ZO,), 9.0, device="cuda", dtype=t)
            da = dbuf[ZO:ZO + n * h * w * ci].view(n, h, w, ci)
            l.check(lib.ustrun_conv3x3_dgrad(self.dyg.data_ptr(), wd.data_ptr(), n, h, w, co, ci, da.data_ptr(), ci, None, 0, 0, 0, 0, code, None), "dgrad")
            v = lib.ustrun_debug_last_conv_variant()
            assert bool((dbuf[:ZO] == 9.0).all()) and bool((dbuf[-ZO:] == 9.0).all()), "input gradient wrote outside its output"
            return from_nhwc(da.float()), v
        b0 = torch.full((ZO + n * h * w * cs[0] + ZO,), 9.0, device="cuda", dtype=t)
        b1 = torch.full((ZO + n * self.uh * self.uw * cs[1] + ZO,), 7.0, device="cuda", dtype=t)
        d0 = b0[ZO:-ZO].view(n, h, w, cs[0])
        d1 = b1[ZO:-ZO].view(n, self.uh, self.uw, cs[1])
        l.check(lib.ustrun_conv3x3_dgrad(self.dyg.data_ptr(), wd.data_ptr(), n, h, w, co, ci, d0.data_ptr(), cs[0], d1.data_ptr(),
                                         self.uh, self.uw, self.oy, self.ox, code, None), "dgrad split")
        v = lib.ustrun_debug_last_conv_variant()
        for b, s in ((b0, 9.0), (b1, 7.0)):
            assert bool((b[:ZO] == s).all()) and bool((b[-ZO:] == s).all()), "split input gradient wrote outside a destination"
        return (from_nhwc(d0.float()), from_nhwc(d1.float())), v

    def wgrad(self):
        l, lib = L(), L().lib()
        n, h, w, co, ci = self.n, self.h, self.w, self.co, self.ci
        sarr, ns = self.srcs()
        nb = lib.ustrun_wgrad_partials_bytes(9, ci, co, n * h * w)
        part = torch.full((nb // 4 + 1024,), NAN, device="cuda")          # the slabs are written before they are read, not assumed clean
        wbuf = torch.full((1024 + co * ci * 9 + 1024,), NAN, device="cuda")
        dw = wbuf[1024:-1024].view(co, ci, 3, 3)
        l.check(lib.ustrun_conv3x3_wgrad(sarr, ns, self.dyg.data_ptr(), n, h, w, co, dw.data_ptr(), 0, part.data_ptr(), nb, TDT[self.elt][1], None), "wgrad")
        v = lib.ustrun_debug_last_wgrad_variant()
        assert bool(torch.isnan(wbuf[:1024]).all()) and bool(torch.isnan(wbuf[-1024:]).all()), "weight gradient wrote outside dw"
        assert bool(torch.isnan(part[nb // 4:]).all()), "weight gradient wrote past the slab bytes it asked for"
        return dw.cpu().clone(), v


def check_stats(stat, clean, ref_out, G, what):
    """per pass and channel: an output column that is finite throughout keeps the clean run's rows to the bit; one that holds a
    non-finite value has a non-finite sum"""
    n, co = ref_out.shape[:2]
    bad = (NF.classify(ref_out) != NF.FINITE).view(G, n // G, co, -1).any(3).any(1)            # [G, co]
    for g in range(G):
        for c in range(co):
            rows, crow = stat[g, :, :, c], clean[g, :, :, c]
            if bool(bad[g, c]):
                assert not bool(torch.isfinite(rows.double().sum(0)).all()), f"{what}: pass {g} channel {c} holds a non-finite output, its statistics rows are finite"
            else:
                assert torch.equal(rows.view(torch.int32), crow.view(torch.int32)), f"{what}: statistics rows of pass {g} channel {c} differ from the clean run's"


# (name, N, source channels, Cout, H, W, passes, forward variant, input-gradient variant, weight-gradient family, what runs)
HALO16 = (16, 16, 64, 2, 2)
CASES = [
    ("halo_2x64_16", 2, (64,), 64, 16, 16, 2, variant(*HALO16, False, True), variant(*HALO16, False, False), 0x48, "fdw"),
    ("halo_cat_12x20", 2, (64, 64), 64, 12, 20, 2, variant(*HALO16, False, True), variant(8, 16, 64, 1, 2, False, False), 0x48, "fdsw"),
    ("halo_wide_11x37", 3, (64,), 64, 11, 37, 1, variant(8, 32, 64, 2, 2, False, True), variant(8, 32, 64, 2, 2, False, False), 0x48, "fdw"),
    ("generic_24_40", 1, (24,), 40, 9, 7, 1, None, None, None, "fdw"),
    ("lin_fwd_18", 30, (32,), 512, 18, 18, 2, variant("lin", 18, 128, 4, 1, False, True), None, None, "fw"),
    ("lin_dgrad_18", 30, (512,), 32, 18, 18, 1, None, variant("lin", 18, 128, 4, 1, False, False), None, "d"),
    ("ws64_60x70", 8, (64,), 64, 60, 70, 2, WS | 1, WS, 0x48, "fdw"),
]
SMALL = [c for c in CASES if c[1] * c[4] * c[5] < 2000]


def placements(case):
    """[(label, operand, [(n, c, y, x), ...])]: operand "y0" (raw output under affine + ReLU), "u" (the concat's second source, inside
    its window), "dy" (the gradient).  Two positions per call where their cones cannot meet (different images / passes).  The edge
    position is the last pixel of one tile whose right / lower neighbour opens the next: 16- or 32-pixel tile columns and 8-row
    tiles, or position 255 of a linear tile's flat padded space (row length W + 1 = 19: row 13, column 8).  The larger shapes keep
    two calls: edge + end of the last pass, and the gradient's."""
    name, n, cs, co, h, w, G = case[:7]
    last = n - 1                                     # an image of the last pass
    edge = (13, 8) if name.startswith("lin_") else (min(7, h - 1), 31 if w > 32 else min(15, w - 1))
    end = (last, 1, h - 1, w - 1)                    # the last, partial tile
    dy2 = ("dy corner + last pass", "dy", [(0, co - 1, 0, w - 1)] + ([(last, 0, h - 1, 0)] if n > 1 else []))
    if case not in SMALL:
        return [("tile edge + end of the last pass", "y0", [(0, cs[0] - 1) + edge, end]), dy2]
    out = [("corner", "y0", [(0, 0, 0, 0)]),
           ("tile edge + last pass", "y0", [(0, cs[0] - 1) + edge] + ([(last, 1, min(8, h - 1), min(16, w - 1))] if n > 1 else [])),
           ("last partial tile", "y0", [end]),
           dy2,
           ("dy tile edge", "dy", [(0, co // 2, min(8, h - 1), min(16, w - 1))])]
    if len(cs) == 2:
        out.append(("second source, window corner + last pass", "u", [(0, 0, 0, 0), (last, cs[1] - 1, h - 3, w - 5)]))
    return out


def run_checks(L_, case, elt, refs, tag, conventions=("torch",), line_axis=1):
    """run what the case lists ("f" forward, "d" input gradient, "s" split input gradient, "w" weight gradient) and hold each to the
    float64 reference of one of `conventions`; returns {kernel: matching conventions}"""
    vf, vd, vw, parts = case[7:11]
    got = {}

    def hold(what, dev, pick, dtype):
        names = [k for k in conventions if NF.mismatches(dev, pick(refs[k]), dtype)[:2] == (0, 0)]
        if not names:
            NF.assert_matches(dev, pick(refs[conventions[0]]), dtype, f"{tag} {what} (convention {conventions[0]})")
        got[what] = names

    if "f" in parts:
        out, stat, v = L_.forward()
        assert vf is None or v == vf, f"forward ran {vstr(v)}"
        hold("forward", out, lambda r: r[0], elt)
        got["stat"] = stat
    if "d" in parts:
        da, v = L_.dgrad()
        assert vd is None or v == vd, f"input gradient ran {vstr(v)}"
        hold("input gradient", da, lambda r: r[1], elt)
    if "s" in parts:
        (d0, d1), v = L_.dgrad(split=True)
        c0 = L_.cs[0]
        hold("split input gradient [0]", d0, lambda r: r[1][:, :c0], elt)
        hold("split input gradient [1]", d1, lambda r: r[1][:, c0:, L_.oy:L_.oy + L_.uh, L_.ox:L_.ox + L_.uw], elt)
    if "w" in parts:
        dw, v = L_.wgrad()
        assert vw is None or v >> 24 == vw, f"weight gradient ran {hex(v)}"
        res = {k: weight_gradient_mismatches(dw, refs[k][2], line_axis) for k in conventions}
        got["weight gradient"] = [k for k in conventions if res[k][:2] == (0, 0)]
        k0 = conventions[0]
        assert got["weight gradient"], f"{tag} weight gradient (convention {k0}): {res[k0][0]} class / {res[k0][1]} value mismatches: {res[k0][2]}"
    return got


def plant_inf(L_, operand, where, k):
    """+inf / -inf alternating over positions and calls.  Under the loader's affine + ReLU the FIRST position is given the sign that
    makes the activation +inf (a -inf activation is relu'd to 0 and reaches nothing); the second gets the other sign: it must vanish."""
    for j, pos in enumerate(where):
        s = 1.0 if (j + k) % 2 == 0 else -1.0
        if operand == "y0":
            s = (1.0 if j == 0 else -1.0) * float(torch.sign(L_.sc[pos[0] // L_.gn, pos[1]]))
        dev, cpu = {"y0": (L_.y0g, L_.y0), "u": (L_.ug, L_.u), "dy": (L_.dyg, L_.dy)}[operand]
        plant(dev, cpu, pos, s * INF, L_.elt)


_CLEAN = {}


def clean_stats(case, elt):
    key = (case[0], elt)
    if key not in _CLEAN:
        L_ = Conv(*case[:7], elt)
        got = run_checks(L_, case, elt, {"torch": L_.reference()}, f"{case[0]} {elt} clean")
        _CLEAN[key] = got.get("stat")
    return _CLEAN[key]


INF_CASES = [(c, e) for e in ("f16", "bf16") for c in CASES]


@pytest.mark.parametrize("case,elt", INF_CASES, ids=[f"{c[0]}-{e}" for c, e in INF_CASES])
def test_inf_propagates_and_stays_contained(case, elt):
    """gates 2 and 3: +inf and -inf, one placement per call"""
    clean_stats(case, elt)                           # (the clean call itself against float64, once per case and type)
    for k, (label, operand, where) in enumerate(placements(case)):
        if operand == "dy" and not set("dsw") & set(case[10]) or operand != "dy" and not set("fw") & set(case[10]):
            continue
        L_ = Conv(*case[:7], elt)
        plant_inf(L_, operand, where, k)
        ref = L_.reference()
        nonfinite = sum(int((NF.classify(r) != NF.FINITE).sum()) for r in ref)
        assert nonfinite > 0, "the planted value reaches no output: the case checks nothing"
        got = run_checks(L_, case, elt, {"torch": ref}, f"{case[0]} {elt} {label}", line_axis=0 if operand == "dy" else 1)
        if "stat" in got:
            # the clean run of the same call: a raw value that the ReLU takes to 0, as it takes the planted -inf, in its place
            Lc = Conv(*case[:7], elt)
            if operand == "y0":
                for pos in where[1:]:
                    plant(Lc.y0g, Lc.y0, pos, -4.0 * float(torch.sign(Lc.sc[pos[0] // Lc.gn, pos[1]])), elt)
            check_stats(got["stat"], Lc.forward()[1], ref[0], L_.G, f"{case[0]} {elt} {label}")


@pytest.mark.parametrize("case", [c for c in CASES if "f" in c[10] or "w" in c[10]], ids=[c[0] for c in CASES if "f" in c[10] or "w" in c[10]])
def test_nan_through_the_loaders_relu(case):
    """gate 4 (f16): a NaN of each sign in the raw output that the loader passes through BatchNorm affine + ReLU, in a channel with a
    positive and in one with a negative scale; every kernel that recomputes the activation must follow one of the two conventions"""
    elt = "f16"
    for sign in ("+nan", "-nan"):
        L_ = Conv(*case[:7], elt)
        cpos = int((L_.sc[0] > 0).nonzero()[0])
        cneg = int((L_.sc[0] < 0).nonzero()[0])
        plant(L_.y0g, L_.y0, (0, cpos, 2, 3), sign, elt)
        plant(L_.y0g, L_.y0, (0, cneg, L_.h - 2, L_.w - 3), sign, elt)
        refs = {k: L_.reference(k) for k in NF.CONVENTIONS}
        part_case = case[:10] + (case[10].replace("d", "").replace("s", ""),)      # (the input gradient reads no activation)
        got = run_checks(L_, part_case, elt, refs, f"{case[0]} {sign}", conventions=NF.CONVENTIONS)
        for what, names in got.items():
            if what != "stat":
                print(f"NaN convention: {case[0]} {what} {sign}: {' / '.join(names)}")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_f16_storage_overflow_becomes_inf(case):
    """gate 1: exact f32 sums of 65504, 65519, 65520 and 2096128 at four outputs of channel 0, their negatives in channel 1.  Three
    operand channels carry 2047, 15 / 16 and 2047 at those pixels; the two output channels read them through the centre tap with weights
    +-(32, 1, 1024) and nothing else, every other channel through its small integer weights (|sum| < 2^13: finite)."""
    elt = "f16"
    name, n, cs, co, h, w, G = case[:7]
    pix = [(0, 1, 2), (0, h - 2, w - 3), (n - 1, 3, w - 2), (n - 1, h - 1, 0)]
    vals = [(2047, 0, 0), (2047, 15, 0), (2047, 16, 0), (0, 0, 2047)]
    want = [65504.0, 65504.0, INF, INF]
    if "f" in case[10]:
        L_ = Conv(*case[:7], elt, unit_affine=(0, 1, 2))
        L_.wt[:2] = 0
        L_.wt[0, :3, 1, 1] = torch.tensor([32.0, 1.0, 1024.0])
        L_.wt[1, :3, 1, 1] = -L_.wt[0, :3, 1, 1]
        for (i, y, x), v3 in zip(pix, vals):
            for c, v in enumerate(v3):
                plant(L_.y0g, L_.y0, (i, c, y, x), float(v), elt)
        ref = L_.reference()
        out, stat, v = L_.forward()
        assert case[7] is None or v == case[7], f"forward ran {vstr(v)}"
        for (i, y, x), t in zip(pix, want):
            assert float(out[i, 0, y, x]) == t and float(out[i, 1, y, x]) == -t, (name, (i, y, x), float(out[i, 0, y, x]), float(out[i, 1, y, x]), t)
        NF.assert_matches(out, ref[0], elt, f"{name} forward overflow")
        wz = L_.wt.clone()
        wz[:2] = 0
        _, clean, _ = L_.forward(wt=wz)
        # every other channel against the run without the two; the two themselves: non-finite in the pass that holds the infinities
        check_stats(stat[:, :, :, 2:], clean[:, :, :, 2:], ref[0][:, 2:], G, f"{name} forward overflow")
        assert not bool(torch.isfinite(stat[G - 1, :, :, :2].double().sum(0)).any()), "65520 / 2096128 were stored as inf, their statistics rows are finite"
    if "d" in case[10]:
        L_ = Conv(*case[:7], elt)
        L_.wt[:, :2] = 0
        L_.wt[:3, 0, 1, 1] = torch.tensor([32.0, 1.0, 1024.0])
        L_.wt[:3, 1, 1, 1] = -L_.wt[:3, 0, 1, 1]
        for (i, y, x), v3 in zip(pix, vals):
            for c, v in enumerate(v3):
                plant(L_.dyg, L_.dy, (i, c, y, x), float(v), elt)
        ref = L_.reference()
        da, v = L_.dgrad()
        assert case[8] is None or v == case[8], f"input gradient ran {vstr(v)}"
        for (i, y, x), t in zip(pix, want):
            assert float(da[i, 0, y, x]) == t and float(da[i, 1, y, x]) == -t, (name, (i, y, x), float(da[i, 0, y, x]), float(da[i, 1, y, x]), t)
        NF.assert_matches(da, ref[1], elt, f"{name} input gradient overflow")
        if "s" in case[10]:                       # the two-destination epilogue stores the same four sums (channels 0, 1 lie in destination 0)
            (d0, d1), _ = L_.dgrad(split=True)
            for (i, y, x), t in zip(pix, want):
                assert float(d0[i, 0, y, x]) == t and float(d0[i, 1, y, x]) == -t, (name, "split", (i, y, x), float(d0[i, 0, y, x]), float(d0[i, 1, y, x]), t)
            NF.assert_matches(d0, ref[1][:, :cs[0]], elt, f"{name} split input gradient [0] overflow")
            NF.assert_matches(d1, ref[1][:, cs[0]:, L_.oy:L_.oy + L_.uh, L_.ox:L_.ox + L_.uw], elt, f"{name} split input gradient [1] overflow")


# ---- the kernels around the 3x3 convolutions, f16 (bf16 again for the ConvTranspose containment) ---------------------------------------
# Each reads its poisoned operand through the same affine + ReLU or plainly, multiplies and adds; none converts it to an index
# (csrc/convT_bf16.hip, wgradT_bf16.hip, head.hip, bn.hip: the only casts are vector bit casts and the 16-bit integer max of act8).
def ri_gen(seed):
    g = torch.Generator().manual_seed(seed)
    return g, (lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float())


def guarded(shape, tdt, fill):
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((ZO + n + ZO,), fill, device="cuda", dtype=tdt)
    return buf, buf[ZO:ZO + n].view(*shape)


def whole(buf, fill):
    ok = lambda t: bool(torch.isnan(t).all()) if fill != fill else bool((t == fill).all())
    return ok(buf[:ZO]) and ok(buf[-ZO:])


CONVT_CASES = [(2, 64, 32, 5, 7), (2, 16, 8, 8, 8)]
CONVT_PLANTS = [("x corner", "x", [(0, 0, 0, 0)]), ("x last pixel, channel tail + other image", "x", [(1, -1, -1, -1), (0, 1, 2, 3)]),
                ("du corner + other image", "du", [(0, -1, 0, 0), (1, 0, -1, -1)]), ("+nan", "x", [(0, 2, 1, 1)]), ("-nan", "x", [(1, 3, 2, 2)]),
                ("overflow forward", "x", [(0, 1, 2), (0, -2, -3), (1, 3, -2), (1, -1, 0)]), ("overflow input gradient", "du", [(0, 1, 2), (0, -2, -3), (1, 3, -2), (1, -1, 0)])]
OVERFLOW_VALUES = [(2047, 0, 0), (2047, 15, 0), (2047, 16, 0), (0, 0, 2047)]          # through weights (32, 1, 1024): 65504, 65519, 65520, 2096128
OVERFLOW_STORED = [65504.0, 65504.0, INF, INF]


@pytest.mark.parametrize("elt", ["f16", "bf16"])
@pytest.mark.parametrize("n,ci,co,h,w", CONVT_CASES)
def test_convT_trio_nonfinite(n, ci, co, h, w, elt):
    """ustrun_convT2x2_fwd / _dgrad / _wgrad (the dedicated GEMM at 64 -> 32, the generic kernel at 16 -> 8): gates 2-4.  No padding
    exists here (every output pixel has one input pixel), so torch autograd is the weight gradient's reference as it stands; dw is
    judged per input-channel line (axis 0 of [Cin, Cout, 2, 2]) for a bad activation, per output-channel line for a bad gradient,
    db with the gradient's channel."""
    l, lib = L(), L().lib()
    tdt, code = TDT[elt]
    for label, operand, where in CONVT_PLANTS:
        g, ri = ri_gen(ci + co)
        x, wt, b, du = ri(-3, 3, n, ci, h, w), ri(-2, 2, ci, co, 2, 2), ri(-2, 2, co), ri(-3, 3, n, co, 2 * h, 2 * w)
        sc = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (ci,), generator=g)]
        sh = ri(-1, 1, ci)
        over = label.startswith("overflow")
        if over and elt != "f16":
            continue
        if label == "overflow forward":           # u[2y + i, 2x + j, 0] = 32 a0 + a1 + 1024 a2 at every tap, channel 1 its negative
            sc[:3], sh[:3] = 1.0, 0.0
            wt[:, :2], b[:2] = 0, 0
            wt[:3, 0] = torch.tensor([32.0, 1.0, 1024.0])[:, None, None]
            wt[:3, 1] = -wt[:3, 0]
        elif over:                                # da[y, x, 0] = 32 du0 + du1 + 1024 du2 at (2y, 2x), input channel 1 its negative
            wt[:2] = 0
            wt[0, :3, 0, 0] = torch.tensor([32.0, 1.0, 1024.0])
            wt[1, :3, 0, 0] = -wt[0, :3, 0, 0]
        xg, dug = nhwc16(x, elt), nhwc16(du, elt)
        opix = []
        for j, pos in enumerate(where if over else []):
            i, yy, xx = pos[0], pos[1] % h, pos[2] % w
            opix.append((i, yy, xx))
            for ch, v in enumerate(OVERFLOW_VALUES[j]):
                if operand == "x":
                    plant(xg, x, (i, ch, yy, xx), float(v), elt)
                else:
                    plant(dug, du, (i, ch, 2 * yy, 2 * xx), float(v), elt)
        for j, pos in enumerate([] if over else where):
            dev, cpu = (xg, x) if operand == "x" else (dug, du)
            pos = tuple(p % s for p, s in zip(pos, cpu.shape))
            if label.endswith("nan"):
                val = label
            else:
                val = (1.0 if j == 0 else -1.0) * INF * (float(torch.sign(sc[pos[1]])) if operand == "x" else 1.0)
            plant(dev, cpu, pos, val, elt)
        refs = {}
        for conv in (NF.CONVENTIONS if label.endswith("nan") else ("torch",)):
            a = NF.stored(NF.relu(NF.stored(x, elt) * sc.double()[None, :, None, None] + sh.double()[None, :, None, None], conv), elt).requires_grad_(True)
            wr, br = NF.stored(wt, elt).requires_grad_(True), b.double().requires_grad_(True)
            u = F.conv_transpose2d(a, wr, br, stride=2)
            u.backward(NF.stored(du, elt))
            refs[conv] = (u.detach(), a.grad, wr.grad, br.grad)
        nel = 4 * ((ci + 7) // 8 * 8) * ((co + 7) // 8 * 8)
        wf, wd = torch.zeros(nel, dtype=tdt, device="cuda"), torch.zeros(nel, dtype=tdt, device="cuda")
        wg, bg, scg, shg = wt.cuda(), b.cuda(), sc.cuda(), sh.cuda()
        l.check(lib.ustrun_pack_convT2x2(wg.data_ptr(), ci, co, wf.data_ptr(), wd.data_ptr(), code, None))
        src = l.nhwc_src(xg.data_ptr(), ci, h, w, scale=scg.data_ptr(), shift=shg.data_ptr(), relu=1)
        ub, u = guarded((n, 2 * h, 2 * w, co), tdt, 9.0)
        l.check(lib.ustrun_convT2x2_fwd(C.byref(src), wf.data_ptr(), bg.data_ptr(), n, h, w, co, u.data_ptr(), code, None))
        db_, da = guarded((n, h, w, ci), tdt, 9.0)
        l.check(lib.ustrun_convT2x2_dgrad(dug.data_ptr(), wd.data_ptr(), n, h, w, co, ci, da.data_ptr(), code, None))
        nb = max(lib.ustrun_wgrad_partials_bytes(4, ci, co, n * h * w), 512 * co * 4)
        part = torch.full((nb // 4,), NAN, device="cuda")
        wb, dw = guarded((ci, co, 2, 2), torch.float32, NAN)
        bb, db = guarded((co,), torch.float32, NAN)
        l.check(lib.ustrun_convT2x2_wgrad(C.byref(src), dug.data_ptr(), n, h, w, co, dw.data_ptr(), db.data_ptr(), 0, part.data_ptr(), nb, code, None))
        assert whole(ub, 9.0) and whole(db_, 9.0) and whole(wb, NAN) and whole(bb, NAN), f"convT {label}: a guard zone was written"
        tag = f"convT {ci}->{co} {elt} {label}"
        uc, dac = from_nhwc(u.float()), from_nhwc(da.float())
        for (i, yy, xx), t in zip(opix, OVERFLOW_STORED):
            got2 = (uc[i, :2, 2 * yy + 1, 2 * xx + 1] if operand == "x" else dac[i, :2, yy, xx]).tolist()
            assert got2 == [t, -t], (tag, (i, yy, xx), got2, t)
        axis = 1 if operand == "du" else 0
        res = {}
        for conv, (ru, ra, rw, rb) in refs.items():
            res[conv] = {"forward": NF.mismatches(from_nhwc(u.float()), ru, elt), "input gradient": NF.mismatches(from_nhwc(da.float()), ra, elt),
                         "weight gradient": weight_gradient_mismatches(dw, rw, axis), "bias gradient": NF.mismatches(db, rb, "f32")}
        for what in ("forward", "input gradient", "weight gradient", "bias gradient"):
            names = [c for c in refs if res[c][what][:2] == (0, 0)]
            assert names, f"{tag} {what}: {res['torch'][what]}"
            if label.endswith("nan") and elt == "f16" and what in ("forward", "weight gradient"):
                print(f"NaN convention: convT {ci}->{co} {what} {label}: {' / '.join(names)}")


@pytest.mark.parametrize("n,c,k,h,w", [(1, 8, 4, 9, 7), (2, 64, 2, 16, 16)])
def test_head_nonfinite(n, c, k, h, w):
    """ustrun_head_fwd / ustrun_head_bwd, f16 storage (the generic kernel at 8 channels, the 64-channel one): an inf activation and
    an inf logit gradient (gates 2, 3), NaN of both signs under the affine + ReLU (gate 4), and gate 1 on the head's 16-bit
    gradient store: da[p][c] = sum_k dlogits[k][p] w[k][c] with dlogits of 65504, 65519, 65520, 2096128 through a unit weight."""
    l, lib = L(), L().lib()
    elt, (tdt, code) = "f16", TDT["f16"]
    hw = h * w
    plants = [("y corner", "y", [(0, 0, 0, 0)], None), ("y last pixel", "y", [(n - 1, c - 1, h - 1, w - 1)], None),
              ("dl corner + last pixel", "dl", [(0, 0, 0, 0), (n - 1, k - 1, h - 1, w - 1)], None),
              ("+nan", "y", [(0, 1, 2, 3)], None), ("-nan", "y", [(0, 2, 3, 1)], None),
              ("overflow", "dl", [(0, 0, 1, 2), (0, 0, 4, 5), (n - 1, 0, 6, 3), (n - 1, 0, h - 1, 0)], [65504.0, 65519.0, 65520.0, 2096128.0])]
    for label, operand, where, values in plants:
        g, ri = ri_gen(c + k)
        y, wt, b, dl = ri(-3, 3, n, c, h, w), ri(-2, 2, k, c), ri(-2, 2, k), ri(-2, 2, n, k, h, w)
        sc = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (c,), generator=g)]
        sh = ri(-1, 1, c)
        if values:
            wt[0, 0], wt[0, 1] = 1.0, -1.0
            wt[1:, :2] = 0                        # (channels 0 and 1 of da see class 0 of dlogits alone)
            dl[:, 1:] = 0                         # ... and every other channel sees nothing else: |2 * 2096128| overflows there too, by the reference
        yg, dlg = nhwc16(y, elt), dl.cuda()
        for j, pos in enumerate(where):
            if operand == "y":
                val = label if label.endswith("nan") else INF * float(torch.sign(sc[pos[1]]))
                plant(yg, y, pos, val, elt)
            else:
                v = values[j] if values else (INF if j == 0 else -INF)
                dlg[pos], dl[pos] = v, v
        refs = {}
        for conv in (NF.CONVENTIONS if label.endswith("nan") else ("torch",)):
            a = NF.stored(NF.relu(NF.stored(y, elt) * sc.double()[None, :, None, None] + sh.double()[None, :, None, None], conv), elt).requires_grad_(True)
            wr, br = wt.double().requires_grad_(True), b.double().requires_grad_(True)
            lg = F.conv2d(a, wr[:, :, None, None], br)
            lg.backward(dl.double())
            refs[conv] = (lg.detach(), a.grad, wr.grad, br.grad)
        scg, shg, wg, bg = sc.cuda(), sh.cuda(), wt.cuda(), b.cuda()
        lb, lgd = guarded((n, k, h, w), torch.float32, 9.0)
        l.check(lib.ustrun_head_fwd(yg.data_ptr(), scg.data_ptr(), shg.data_ptr(), n * hw, hw, c, k, wg.data_ptr(), bg.data_ptr(), lgd.data_ptr(), code, None))
        ab, da = guarded((n, h, w, c), tdt, 9.0)
        wb, dw = guarded((k, c), torch.float32, NAN)
        bb, db = guarded((k,), torch.float32, NAN)
        nb = 1024 * (k * c + k) * 4
        part = torch.full((nb // 4,), NAN, device="cuda")
        l.check(lib.ustrun_head_bwd(dlg.data_ptr(), yg.data_ptr(), scg.data_ptr(), shg.data_ptr(), n * hw, hw, c, k, wg.data_ptr(), da.data_ptr(),
                                    dw.data_ptr(), db.data_ptr(), 0, part.data_ptr(), nb, code, None))
        assert whole(lb, 9.0) and whole(ab, 9.0) and whole(wb, NAN) and whole(bb, NAN), f"head {label}: a guard zone was written"
        dac = from_nhwc(da.float())
        if values:
            for pos, t in zip(where, [65504.0, 65504.0, INF, INF]):
                i, _, yy, xx = pos
                assert float(dac[i, 0, yy, xx]) == t and float(dac[i, 1, yy, xx]) == -t, (label, pos, float(dac[i, 0, yy, xx]), float(dac[i, 1, yy, xx]))
        tag = f"head C={c} K={k} {label}"
        for what, dev, idx, dt in (("logits", lgd.cpu(), 0, "f32"), ("input gradient", dac, 1, elt), ("bias gradient", db.cpu(), 3, "f32")):
            names = [cv for cv in refs if NF.mismatches(dev, refs[cv][idx], dt)[:2] == (0, 0)]
            assert names, f"{tag} {what}: {NF.mismatches(dev, refs['torch'][idx], dt)}"
            if label.endswith("nan") and what == "logits":
                print(f"NaN convention: head C={c} forward {label}: {' / '.join(names)}")
        # dw [K][C]: a bad activation poisons column c0, a bad logit gradient row k0
        axis = 0 if operand == "dl" else 1
        res = {}
        for cv in refs:
            cls, val = NF.expect(refs[cv][2], "f32")
            gg = dw.cpu().double()
            gcls = NF.classify(gg)
            line = (cls != NF.FINITE).sum(1 - axis, keepdim=True) > 0
            res[cv] = (int(((gcls != cls) & ((cls != NF.FINITE) | ~line)).sum()), int(((cls == NF.FINITE) & (gcls == NF.FINITE) & (gg != val) & ~line).sum()))
        names = [cv for cv in refs if res[cv] == (0, 0)]
        assert names, f"{tag} weight gradient: {res}"
        if label.endswith("nan"):
            print(f"NaN convention: head C={c} weight gradient {label}: {' / '.join(names)}")


@pytest.mark.parametrize("n,c,h,w", [(2, 64, 16, 16), (1, 24, 9, 7)])
def test_pool_act_nonfinite(n, c, h, w):
    """ustrun_pool_act, f16: MaxPool2d(2)(relu(y * scale + shift)).  +inf in a window gives +inf, -inf is relu'd away (gates 2, 3: every
    other window bit for bit); a NaN of either sign gives torch's NaN or select's maximum of the other three (gate 4)."""
    l, lib = L(), L().lib()
    elt, (tdt, code) = "f16", TDT["f16"]
    for label, where in (("corner", [(0, 0, 0, 0)]), ("last window + channel tail", [(n - 1, c - 1, 2 * (h // 2) - 1, 2 * (w // 2) - 1)]),
                         ("vanishing -inf", [(0, c // 2, 3, 2)]), ("+nan", [(0, 1, 2, 3)]), ("-nan", [(n - 1, 2, 4, 5)]),
                         # gate 1: relu(2047 scale + shift) = 65504, 65519, 65520, 2096128 in channels 0..3, the maximum of window (1, 1)
                         ("overflow", [])):
        g, ri = ri_gen(c + h)
        y = ri(-3, 3, n, c, h, w)
        sc = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (c,), generator=g)]
        sh = ri(-1, 1, c)
        if label == "overflow":
            sc[:4], sh[:4] = torch.tensor([32.0, 32.0, 32.0, 1024.0]), torch.tensor([0.0, 15.0, 16.0, 0.0])
            y[0, :4, 3, 2] = 2047.0
        yg = nhwc16(y, elt)
        for pos in where:
            s = float(torch.sign(sc[pos[1]])) * (-1.0 if label.startswith("vanishing") else 1.0)
            plant(yg, y, pos, label if label.endswith("nan") else s * INF, elt)
        refs = {cv: F.max_pool2d(NF.relu(NF.stored(y, elt) * sc.double()[None, :, None, None] + sh.double()[None, :, None, None], cv), 2)
                for cv in (NF.CONVENTIONS if label.endswith("nan") else ("torch",))}
        if label.endswith("nan"):                 # select: the NaN is 0 before the maximum; torch's max_pool2d would propagate it anyway
            assert int(torch.isnan(refs["torch"]).sum()) == 1 and int(torch.isnan(refs["select"]).sum()) == 0
        scg, shg = sc.cuda(), sh.cuda()
        src = l.nhwc_src(yg.data_ptr(), c, h, w, scg.data_ptr(), shg.data_ptr(), relu=1)
        ob, out = guarded((n, h // 2, w // 2, c), tdt, 9.0)
        l.check(lib.ustrun_pool_act(C.byref(src), n, out.data_ptr(), code, None))
        assert whole(ob, 9.0), "pool_act wrote outside its output"
        if label == "overflow":
            assert from_nhwc(out.float())[0, :4, 1, 1].tolist() == OVERFLOW_STORED, from_nhwc(out.float())[0, :4, 1, 1].tolist()
        names = [cv for cv in refs if NF.mismatches(from_nhwc(out.float()), refs[cv], elt)[:2] == (0, 0)]
        assert names, f"pool_act C={c} {label}: {NF.mismatches(from_nhwc(out.float()), refs['torch'], elt)}"
        if label.endswith("nan"):
            print(f"NaN convention: pool_act C={c} {label}: {' / '.join(names)}")


@pytest.mark.parametrize("n,c,h,w", [(1, 1, 19, 37), (2, 3, 16, 32)])
def test_conv_first_nonfinite(n, c, h, w):
    """The first convolution, f16 (NCHW f32 image, C <= 4 -> 64): forward with statistics rows (ustrun_conv3x3_fwd_rows on an NCHW
    source), weight gradient (ustrun_conv3x3_wgrad on the same source) and input gradient (ustrun_conv_first_dgrad, f32 output).
    +-inf in the image and in the output's gradient: corner, last pixel, the 16- / 32-pixel strip edge (gates 2, 3; the weight
    gradient per channel line over in-range pixel pairs, as above; statistics rows per image against a clean run); storage overflow
    through three image channels at C = 3 (gate 1).  No ReLU on this path: no gate 4."""
    l, lib = L(), L().lib()
    elt, (tdt, code) = "f16", TDT["f16"]
    co = 64
    # (two values per call only in different channels: every pixel of a channel meets in that channel's line of dw)
    plants = [("x corner", "x", [(0, 0, 0, 0)])] + \
             ([("x strip edge + last pixel", "x", [(0, c - 1, 7, 31), (n - 1, 0, h - 1, w - 1)])] if c > 1 else
              [("x strip edge", "x", [(0, 0, 7, 31)]), ("x last pixel", "x", [(0, 0, h - 1, w - 1)])]) + [
              ("dy corner + last pixel", "dy", [(0, co - 1, 0, 0), (n - 1, 0, h - 1, w - 1)]), ("dy strip edge", "dy", [(0, 5, 8, 16)])]
    if c == 3:
        plants.append(("overflow", "x", [(0, 1, 2), (0, h - 2, w - 3), (n - 1, 3, w - 2), (n - 1, h - 1, 0)]))

    def forward(xg, wt):
        nel = 9 * 8 * 64
        wf, wd = torch.zeros(nel, dtype=tdt, device="cuda"), torch.zeros(nel, dtype=tdt, device="cuda")
        wg = wt.cuda()
        l.check(lib.ustrun_pack_conv3x3(wg.data_ptr(), co, c, wf.data_ptr(), wd.data_ptr(), code, None))
        src = l.nchw_src(xg.data_ptr(), c, h, w)
        yb, y = guarded((n, h, w, co), tdt, 9.0)
        rows_max = lib.ustrun_conv_mtiles(n, h, w, co)
        stat = torch.full((rows_max + 16, 2, co), 7.0, device="cuda")
        rows = C.c_int(0)
        l.check(lib.ustrun_conv3x3_fwd_rows(C.byref(src), 1, wf.data_ptr(), n, h, w, co, y.data_ptr(), stat.data_ptr(), C.byref(rows), code, None))
        assert whole(yb, 9.0) and 0 < rows.value <= rows_max and rows.value % n == 0 and bool((stat[rows.value:] == 7.0).all())
        return from_nhwc(y.float()), stat[:rows.value].view(n, rows.value // n, 2, co).cpu()

    for label, operand, where in plants:
        g, ri = ri_gen(11 * c + h)
        x, wt, dy = ri(-3, 3, n, c, h, w), ri(-2, 2, co, c, 3, 3), ri(-2, 2, n, co, h, w)
        xg, dyg = x.contiguous().cuda(), nhwc16(dy, elt)
        if label == "overflow":
            wt[:2] = 0
            wt[0, :, 1, 1] = torch.tensor([32.0, 1.0, 1024.0])
            wt[1, :, 1, 1] = -wt[0, :, 1, 1]
            for (i, yy, xx), v3 in zip(where, [(2047, 0, 0), (2047, 15, 0), (2047, 16, 0), (0, 0, 2047)]):
                for ch, v in enumerate(v3):
                    xg[i, ch, yy, xx], x[i, ch, yy, xx] = float(v), float(v)
        else:
            for j, pos in enumerate(where):
                v = INF if j == 0 else -INF
                if operand == "x":
                    xg[pos], x[pos] = v, v
                else:
                    plant(dyg, dy, pos, v, elt)
        a = NF.stored(x, elt).requires_grad_(True)
        ref_y = F.conv2d(a, NF.stored(wt, elt), None, 1, 1)
        ref_y.backward(NF.stored(dy, elt))
        ref_y, ref_dx, ref_dw = ref_y.detach(), a.grad, wgrad_in_range(a.detach(), NF.stored(dy, elt))
        tag = f"conv_first C={c} {label}"
        y, stat = forward(xg, wt)
        NF.assert_matches(y, ref_y, elt, tag + " forward")
        if label == "overflow":
            for (i, yy, xx), t in zip(where, [65504.0, 65504.0, INF, INF]):
                assert float(y[i, 0, yy, xx]) == t and float(y[i, 1, yy, xx]) == -t, (tag, (i, yy, xx), float(y[i, 0, yy, xx]), float(y[i, 1, yy, xx]))
            wz = wt.clone()
            wz[:2] = 0
            check_stats(stat[:, :, :, 2:], forward(xg, wz)[1][:, :, :, 2:], ref_y[:, 2:], n, tag)
            assert not bool(torch.isfinite(stat[n - 1, :, :, :2].double().sum(0)).any()), "65520 / 2096128 were stored as inf, their statistics rows are finite"
            continue
        # statistics rows per image: a poisoned image's are non-finite, the others' equal the clean image's (finite stand-in at the planted pixels)
        xc = torch.where(torch.isfinite(x), x, torch.zeros(())).contiguous().cuda()
        check_stats(stat, forward(xc, wt)[1], ref_y, n, tag)
        src = l.nchw_src(xg.data_ptr(), c, h, w)
        nb = lib.ustrun_wgrad_partials_bytes(9, c, co, n * h * w)
        part = torch.full((nb // 4 + 1024,), NAN, device="cuda")
        wb, dw = guarded((co, c, 3, 3), torch.float32, NAN)
        l.check(lib.ustrun_conv3x3_wgrad(C.byref(src), 1, dyg.data_ptr(), n, h, w, co, dw.data_ptr(), 0, part.data_ptr(), nb, code, None))
        assert whole(wb, NAN) and bool(torch.isnan(part[nb // 4:]).all()), tag + ": the weight gradient wrote outside dw or its slabs"
        nc, nv, text = weight_gradient_mismatches(dw, ref_dw, 0 if operand == "dy" else 1)
        assert (nc, nv) == (0, 0), f"{tag} weight gradient: {nc} class / {nv} value mismatches: {text}"
        wg = wt.cuda()
        xb, dx = guarded((n, c, h, w), torch.float32, NAN)
        l.check(lib.ustrun_conv_first_dgrad(dyg.data_ptr(), wg.data_ptr(), n, h, w, co, c, dx.data_ptr(), code, None))
        assert whole(xb, NAN), tag + ": the input gradient wrote outside dx"
        NF.assert_matches(dx, ref_dx, "f32", tag + " input gradient")
