#!/usr/bin/env python3
"""A/B of the pixel-linear GEMM family (convT_bf16.hip: ConvTranspose forward / input gradient with and without BatchNorm-backward sums, the
1x1 convolution plain / with the residual join / with join + sums; wgradT_bf16.hip: the ConvTranspose weight + bias gradient, both kernels,
accumulate 0 and 1) between builds of the library loaded side by side in one process, in the form of tools/ab_igemm.py: bit equality of
every output, statistics table, dw, db and the whole partials buffer on random data, for bf16 and f16, under ustrun_debug_flags 0, 512 (weight
tiles in LDS) and 1 << 27 (round-1 weight gradient), at the small shapes of the tests; then interleaved timing rounds at the four U-Net
ConvTranspose layers and the DeepLabV2 1x1 shapes of tools/bench_conv1x1.py (outputs compared there too: the wide tiles).  The first library
is the baseline, a second copy of it gives the noise band.  Paths are relative to ust-run_amd/ustrun/.

    python tools/ab_convT.py [libustrun_parent.so libustrun_parent2.so libustrun.so] [--n 64] [--n1x1 16] [--rounds 7] [--reps 20] [--no-time]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ab_igemm import DEV, TDT, act, ck, l, load, packed  # noqa: E402
from bench_conv1x1 import SHAPES as SHAPES_1X1  # noqa: E402

LDS_W, ROUND1 = 512, 1 << 27


def convT_case(h, g, dt, n, ci, co, hh, ww, G=1):
    """forward of a BatchNorm + ReLU source (G passes), input gradient plain and with sums, weight + bias gradient (accumulate 0, then 1)"""
    t = TDT[dt]
    gn = n // G
    wf, wd, keep = packed(h, torch.randn(ci, co, 2, 2, generator=g) / ci ** 0.5, 4, dt)
    b = torch.randn(co, generator=g).to(DEV)
    xg, dug = act(torch.randn(n, ci, hh, ww, generator=g), dt), act(torch.randn(n, co, 2 * hh, 2 * ww, generator=g), dt)
    aff = torch.zeros(G, 4, ci)
    aff[:, 0], aff[:, 1] = torch.rand(G, ci, generator=g) + 0.5, 0.3 * torch.randn(G, ci, generator=g)
    aff = aff.to(DEV)
    src = l.nhwc_src(xg.data_ptr(), ci, hh, ww, aff.data_ptr(), aff.data_ptr() + 4 * ci, relu=1, gN=gn if G > 1 else 0, gstride=4 * ci)
    nb = max(h.ustrun_wgrad_partials_bytes(4, ci, co, n * hh * ww), 512 * co * 4)
    o = {"u": torch.zeros(n, 2 * hh, 2 * ww, co, device=DEV, dtype=t), "da": torch.zeros(n, hh, ww, ci, device=DEV, dtype=t),
         "da_s": torch.zeros(n, hh, ww, ci, device=DEV, dtype=t), "stat": torch.zeros(h.ustrun_conv_mtiles(n, hh, ww, ci), 2, ci, device=DEV),
         "dw": torch.zeros(ci, co, 2, 2, device=DEV), "db": torch.zeros(co, device=DEV), "dw2": torch.zeros(ci, co, 2, 2, device=DEV),
         "db2": torch.zeros(co, device=DEV), "part": torch.zeros(nb // 4, device=DEV)}
    rows = C.c_int(0)

    def fwd(h):
        ck(h, h.ustrun_convT2x2_fwd(C.byref(src), wf.data_ptr(), b.data_ptr(), n, hh, ww, co, o["u"].data_ptr(), dt, None))

    def dgrad(h):
        ck(h, h.ustrun_convT2x2_dgrad(dug.data_ptr(), wd.data_ptr(), n, hh, ww, co, ci, o["da"].data_ptr(), dt, None))

    def dgrad_sums(h):       # (y = the source's raw tensor; no launch where the sums are not covered: the outputs keep their fill)
        ck(h, h.ustrun_convT2x2_dgrad_bnsum(dug.data_ptr(), wd.data_ptr(), n, hh, ww, co, ci, o["da_s"].data_ptr(), xg.data_ptr(), aff.data_ptr(),
                                            aff.data_ptr() + 4 * ci, gn if G > 1 else 0, 4 * ci, o["stat"].data_ptr(), C.byref(rows), dt, None))

    def wgrad(h):
        ck(h, h.ustrun_convT2x2_wgrad(C.byref(src), dug.data_ptr(), n, hh, ww, co, o["dw"].data_ptr(), o["db"].data_ptr(), 0, o["part"].data_ptr(), nb, dt, None))

    def run(h):
        fwd(h), dgrad(h), dgrad_sums(h), wgrad(h)
        o["dw2"].copy_(o["dw"]), o["db2"].copy_(o["db"])
        ck(h, h.ustrun_convT2x2_wgrad(C.byref(src), dug.data_ptr(), n, hh, ww, co, o["dw2"].data_ptr(), o["db2"].data_ptr(), 1, o["part"].data_ptr(), nb, dt, None))
    run.parts = {"fwd": fwd, "dgrad": dgrad, "dgrad+sums": dgrad_sums, "wgrad": wgrad}
    run.keep = (keep, xg, b, aff)
    return run, o


def conv1x1_case(h, g, dt, n, ci, co, hh, ww):
    """ci -> co forward of a BatchNorm + ReLU source with statistics; its input gradient (co -> ci) with the join, and with join + sums"""
    t = TDT[dt]
    w = torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5
    wf, wd = torch.zeros(4 * h.ustrun_pack_conv_elems(co, ci, 1), device=DEV), torch.zeros(4 * h.ustrun_pack_conv_elems(ci, co, 1), device=DEV)
    wg, wtg = w.to(DEV), w.permute(1, 0, 2, 3).contiguous().to(DEV)
    ck(h, h.ustrun_pack_conv(wg.data_ptr(), co, ci, 1, wf.data_ptr(), dt, None))
    ck(h, h.ustrun_pack_conv(wtg.data_ptr(), ci, co, 1, wd.data_ptr(), dt, None))
    xg, dyg = act(torch.randn(n, ci, hh, ww, generator=g), dt), act(torch.randn(n, co, hh, ww, generator=g), dt)
    add, ref, y3 = (act(torch.randn(n, ci, hh, ww, generator=g), dt) for _ in range(3))
    sc, sh = (torch.rand(ci, generator=g) + 0.5).to(DEV), (0.3 * torch.randn(ci, generator=g)).to(DEV)
    src = l.nhwc_src(xg.data_ptr(), ci, hh, ww, sc.data_ptr(), sh.data_ptr(), relu=1)
    o = {"y": torch.zeros(n, hh, ww, co, device=DEV, dtype=t), "stat": torch.zeros(h.ustrun_conv_mtiles(n, hh, ww, co), 2, co, device=DEV),
         "dx_j": torch.zeros(n, hh, ww, ci, device=DEV, dtype=t), "dx_js": torch.zeros(n, hh, ww, ci, device=DEV, dtype=t),
         "stat_js": torch.zeros(h.ustrun_conv_mtiles(n, hh, ww, ci), 2, ci, device=DEV)}
    used, u2, fused = C.c_int(0), C.c_int(0), C.c_int(0)

    def fwd(h):
        ck(h, h.ustrun_conv2d_fwd(C.byref(src), 1, wf.data_ptr(), None, n, hh, ww, co, 1, 1, 1, o["y"].data_ptr(), 0, o["stat"].data_ptr(), C.byref(used), dt, None))

    def join(h):             # (no launch where the join is not covered, e.g. 64 columns or flag 512: the output keeps its fill)
        ck(h, h.ustrun_conv1x1_dgrad_join(dyg.data_ptr(), wd.data_ptr(), n, hh, ww, co, ci, add.data_ptr(), ref.data_ptr(), o["dx_j"].data_ptr(), None, None,
                                          None, None, None, C.byref(fused), dt, None))

    def join_sums(h):
        ck(h, h.ustrun_conv1x1_dgrad_join(dyg.data_ptr(), wd.data_ptr(), n, hh, ww, co, ci, add.data_ptr(), ref.data_ptr(), o["dx_js"].data_ptr(),
                                          y3.data_ptr(), None, None, o["stat_js"].data_ptr(), C.byref(u2), C.byref(fused), dt, None))

    def run(h):
        fwd(h), join(h), join_sums(h)
    run.parts = {"1x1 fwd": fwd, "1x1 join": join, "1x1 join+sums": join_sums}
    run.keep = (wg, wtg, xg, sc, sh)
    return run, o


def same_bits(hs, run, outs, flags, title, names):
    got, bad = [], 0
    for h in hs:
        for v in outs.values():
            v.fill_(7.0)
        old = h.ustrun_debug_flags(flags)
        try:
            run(h)
        finally:
            h.ustrun_debug_flags(old)
        torch.cuda.synchronize()
        got.append({k: v.clone() for k, v in outs.items()})
    for other in (1, 2):
        diff = [k for k in outs if not torch.equal(got[0][k], got[other][k]) or bool(torch.isnan(got[0][k].float()).any())]
        bad += len(diff)
        print(f"bits {title:52s} {len(outs)} tensors parent vs {names[other]:8s}: {'bit-equal' if not diff else 'DIFFERENT ' + ','.join(diff)}", flush=True)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", default=["libustrun_parent.so", "libustrun_parent2.so", "libustrun.so"])
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--n1x1", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-time", action="store_true")
    a = ap.parse_args()
    assert len(a.libs) == 3, "baseline, its control copy, the new build"
    names = ("parent", "control", "new")
    hs = [load(p) for p in a.libs]
    g = torch.Generator().manual_seed(13)

    bad = 0
    for dt, tn in ((1, "bf16"), (2, "f16")):          # (packing runs on the baseline: the packed layouts are not what changed)
        for s in ((6, 256, 128, 20, 24, 2), (3, 512, 256, 9, 11, 1), (2, 128, 64, 5, 7, 1), (2, 128, 96, 16, 16, 2), (4, 256, 128, 16, 16, 2),
                  (4, 128, 64, 36, 36, 2)):
            run, outs = convT_case(hs[0], g, dt, *s)
            for fl in (0, LDS_W, ROUND1):
                bad += same_bits(hs, run, outs, fl, f"{tn} convT {s} flags {fl}", names)
        for s in ((2, 256, 128, 20, 24), (3, 64, 64, 9, 11), (2, 128, 256, 5, 7)):
            run, outs = conv1x1_case(hs[0], g, dt, *s)
            for fl in (0, LDS_W):
                bad += same_bits(hs, run, outs, fl, f"{tn} 1x1 {s} flags {fl}", names)
    print("BITS (small shapes):", "all bit-equal" if not bad else f"{bad} DIFFERENT", flush=True)
    if a.no_time:
        return 1 if bad else 0

    # ---- speed (bf16): the four U-Net ConvTranspose layers at N = --n, the DeepLabV2 1x1 shapes at N = --n1x1; the flag-only builds too
    band, verdicts = [], []
    todo = [(f"{name} N={a.n}", lambda ci=ci, co=co, hw=hw: convT_case(hs[0], g, 1, a.n, ci, co, hw, hw), (0, LDS_W, ROUND1))
            for name, ci, co, hw in (("up1.up 1024->512 @16", 1024, 512, 16), ("up2.up 512->256 @32", 512, 256, 32), ("up3.up 256->128 @64", 256, 128, 64),
                                     ("up4.up 128->64 @128", 128, 64, 128))]
    todo += [(f"{name} @{hw} N={a.n1x1}", lambda ci=ci, co=co, hw=hw: conv1x1_case(hs[0], g, 1, a.n1x1, ci, co, hw, hw), (0, LDS_W)) for name, ci, co, hw, _ in SHAPES_1X1]
    for title, make, flagset in todo:
        run, outs = make()
        for fl in flagset:
            bad += same_bits(hs, run, outs, fl, f"bf16 {title} flags {fl}", names)
            for part, fn in run.parts.items():
                if (fl == ROUND1) != (part == "wgrad") and fl:      # (bit 27 is read by the weight gradient alone, bit 9 by the others)
                    continue
                ms = [[], [], []]
                for r in range(a.rounds):
                    for i, h in enumerate(hs):
                        old = h.ustrun_debug_flags(fl)
                        fn(h)
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.reps):
                            fn(h)
                        e1.record()
                        torch.cuda.synchronize()
                        h.ustrun_debug_flags(old)
                        ms[i].append(e0.elapsed_time(e1) / a.reps * 1e3)
                p, c, n = (np.array(v) for v in ms)
                if np.median(p) < 4.0:      # (sums / join not covered for this shape or flag: the entry point returned without a launch)
                    continue
                band += list(c / p)
                verdicts.append((f"{title} {part} flags {fl}", float(np.median(n / p))))
                print(f"time {title:34s} {part:14s} flags {fl:9d}: parent {np.median(p):8.1f} us  control {np.median(c):8.1f} us  new {np.median(n):8.1f} us   "
                      f"control/parent {(c / p).min():.3f}..{(c / p).max():.3f}   new/parent median {np.median(n / p):.3f} ({(n / p).min():.3f}..{(n / p).max():.3f})",
                      flush=True)
        del run, outs
        torch.cuda.empty_cache()
    print("BITS (all shapes):", "all bit-equal" if not bad else f"{bad} DIFFERENT")
    lo, hi = min(band), max(band)
    print(f"CONTROL BAND (control / parent, every round of every launch): {lo:.3f}..{hi:.3f}")
    for title, m in verdicts:
        print(f"  {title:64s}: new/parent median {m:.3f} -> {'inside' if lo <= m <= hi else ('FASTER than the band' if m < lo else 'SLOWER than the band')}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
