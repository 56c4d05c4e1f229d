"""A/B of the generic implicit-GEMM kernels (igemm.hip, igemm_bf16.hip, igemm_x3_kernel of x3.hip) between builds of the library
loaded side by side in one process: bit equality of every output and statistics table on random data at the smallest shapes that
reach each arm of the shared loader and epilogue (csrc/igemm_tile.h), then interleaved timing rounds.  The first library is the
baseline, a second copy of it gives the noise band.  Paths are relative to ust-run_amd/ustrun/.

    python tools/ab_igemm.py [libustrun_parent.so libustrun_parent2.so libustrun.so] [--rounds 9] [--reps 20] [--no-time]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

PKG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ust-run_amd")
sys.path.insert(0, PKG)
from ustrun import _lib as l  # noqa: E402

TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16, 3: torch.float32}
DEV = "cuda"


def load(name):
    h = C.CDLL(os.path.join(PKG, "ustrun", name))
    for fn, (res, args) in l.SIGNATURES.items():
        f = getattr(h, fn)
        f.restype, f.argtypes = res, args
    return h


def ck(h, rc):
    if rc:
        raise RuntimeError(h.ustrun_last_error().decode())


def act(t, dt):         # [N,C,H,W] f32 on the host -> NHWC in the storage type of dt on the device
    return t.permute(0, 2, 3, 1).contiguous().to(DEV).to(TDT[dt])


def packed(h, wt, taps, dt):
    """wt: conv weight [co][ci][3][3] (taps 9) or ConvTranspose weight [ci][co][2][2] (taps 4); room for every dtype's layout"""
    a, b = wt.shape[:2]
    nel = 4 * taps * ((a + 7) // 8 * 8) * ((b + 7) // 8 * 8)
    wf, wd = torch.zeros(nel, device=DEV), torch.zeros(nel, device=DEV)
    wg = wt.contiguous().to(DEV)
    fn = h.ustrun_pack_conv3x3 if taps == 9 else h.ustrun_pack_convT2x2
    ck(h, fn(wg.data_ptr(), a, b, wf.data_ptr(), wd.data_ptr(), dt, None))
    return wf, wd, wg


# ---- the cases: each returns (closure running every launch on library h, dict of output tensors the closure fills) ----------------
def conv_case(h, g, dt, n, ci, co, hh, ww, nsrc=1):
    """3x3 forward with statistics (nsrc = 2: two sources of ci / 2 channels, the first with BatchNorm + ReLU), input gradient whole
    and (ci % 8 == 0) split over two destinations"""
    t = TDT[dt]
    x = torch.randn(n, ci, hh, ww, generator=g)
    wt = torch.randn(co, ci, 3, 3, generator=g) / (3 * ci ** 0.5)
    dy = torch.randn(n, co, hh, ww, generator=g)
    sc, sh = (torch.rand(ci, generator=g) + 0.5).to(DEV), (0.3 * torch.randn(ci, generator=g)).to(DEV)
    wf, wd, keep = packed(h, wt, 9, dt)
    c0 = ci // 2
    if nsrc == 2:
        xs = [act(x[:, :c0], dt), act(x[:, c0:], dt)]
        srcs = (l.Src * 2)(l.nhwc_src(xs[0].data_ptr(), c0, hh, ww, sc.data_ptr(), sh.data_ptr(), relu=1), l.nhwc_src(xs[1].data_ptr(), ci - c0, hh, ww))
    else:
        xs = [act(x, dt)]
        srcs = (l.Src * 1)(l.nhwc_src(xs[0].data_ptr(), ci, hh, ww))
    dyg = act(dy, dt)
    o = {"y": torch.zeros(n, hh, ww, co, device=DEV, dtype=t), "stat": torch.zeros(h.ustrun_conv_mtiles(n, hh, ww, co), 2, co, device=DEV),
         "da": torch.zeros(n, hh, ww, ci, device=DEV, dtype=t)}
    split = ci % 8 == 0
    if split:
        o["da0"], o["da1"] = torch.zeros(n, hh, ww, c0, device=DEV, dtype=t), torch.zeros(n, hh, ww, ci - c0, device=DEV, dtype=t)

    def fwd(h):
        ck(h, h.ustrun_conv3x3_fwd(srcs, nsrc, wf.data_ptr(), n, hh, ww, co, o["y"].data_ptr(), o["stat"].data_ptr(), dt, None))

    def dgrad(h):
        ck(h, h.ustrun_conv3x3_dgrad(dyg.data_ptr(), wd.data_ptr(), n, hh, ww, co, ci, o["da"].data_ptr(), ci, None, 0, 0, 0, 0, dt, None))

    def run(h):
        fwd(h)
        dgrad(h)
        if split:
            ck(h, h.ustrun_conv3x3_dgrad(dyg.data_ptr(), wd.data_ptr(), n, hh, ww, co, ci, o["da0"].data_ptr(), c0, o["da1"].data_ptr(), hh, ww, 0, 0,
                                         dt, None))
    run.fwd, run.dgrad, run.keep = fwd, dgrad, (xs, keep, sc, sh)
    return run, o


def pool_concat_case(h, g, dt):
    """the pooled source (statistics on) and the concat with a pad offset of test_conv3x3_loader_affine_relu_pool_concat_pad, and the
    input gradient split into c0 channels and the offset window of c1 channels"""
    t = TDT[dt]
    n, c0, c1, co, hh, ww = 2, 16, 8, 24, 11, 13
    ys = torch.randn(n, c0, 2 * hh + 1, 2 * ww, generator=g)
    sc, sh = torch.randn(c0, generator=g).to(DEV), (0.3 * torch.randn(c0, generator=g)).to(DEV)
    wf, _, k1 = packed(h, torch.randn(co, c0, 3, 3, generator=g) / 12, 9, dt)
    wf2, wd2, k2 = packed(h, torch.randn(co, c0 + c1, 3, 3, generator=g) / 14, 9, dt)
    yg, sg, ug = act(ys, dt), act(torch.randn(n, c0, hh, ww, generator=g), dt), act(torch.randn(n, c1, hh - 3, ww - 2, generator=g), dt)
    dyg = act(torch.randn(n, co, hh, ww, generator=g), dt)
    src = l.nhwc_src(yg.data_ptr(), c0, 2 * hh + 1, 2 * ww, sc.data_ptr(), sh.data_ptr(), relu=1, pool=1)
    srcs = (l.Src * 2)(l.nhwc_src(sg.data_ptr(), c0, hh, ww, sc.data_ptr(), sh.data_ptr(), relu=1), l.nhwc_src(ug.data_ptr(), c1, hh - 3, ww - 2, off=(1, 1)))
    o = {"pool": torch.zeros(n, hh, ww, co, device=DEV, dtype=t), "pstat": torch.zeros(h.ustrun_conv_mtiles(n, hh, ww, co), 2, co, device=DEV),
         "cat": torch.zeros(n, hh, ww, co, device=DEV, dtype=t), "da0": torch.zeros(n, hh, ww, c0, device=DEV, dtype=t),
         "da1": torch.zeros(n, hh - 3, ww - 2, c1, device=DEV, dtype=t)}

    def run(h):
        ck(h, h.ustrun_conv3x3_fwd(C.byref(src), 1, wf.data_ptr(), n, hh, ww, co, o["pool"].data_ptr(), o["pstat"].data_ptr(), dt, None))
        ck(h, h.ustrun_conv3x3_fwd(srcs, 2, wf2.data_ptr(), n, hh, ww, co, o["cat"].data_ptr(), None, dt, None))
        ck(h, h.ustrun_conv3x3_dgrad(dyg.data_ptr(), wd2.data_ptr(), n, hh, ww, co, c0 + c1, o["da0"].data_ptr(), c0, o["da1"].data_ptr(), hh - 3, ww - 2,
                                     1, 1, dt, None))
    run.keep = (k1, k2, yg, sg, ug, sc, sh)
    return run, o


def convT_case(h, g, dt, n, ci, co, hh, ww):
    t = TDT[dt]
    x = torch.randn(n, ci, hh, ww, generator=g)
    wf, wd, keep = packed(h, torch.randn(ci, co, 2, 2, generator=g) / ci ** 0.5, 4, dt)
    b = torch.randn(co, generator=g).to(DEV)
    xg, dug = act(x, dt), act(torch.randn(n, co, 2 * hh, 2 * ww, generator=g), dt)
    src = l.nhwc_src(xg.data_ptr(), ci, hh, ww)
    o = {"u": torch.zeros(n, 2 * hh, 2 * ww, co, device=DEV, dtype=t), "da": torch.zeros(n, hh, ww, ci, device=DEV, dtype=t)}

    def run(h):
        ck(h, h.ustrun_convT2x2_fwd(C.byref(src), wf.data_ptr(), b.data_ptr(), n, hh, ww, co, o["u"].data_ptr(), dt, None))
        ck(h, h.ustrun_convT2x2_dgrad(dug.data_ptr(), wd.data_ptr(), n, hh, ww, co, ci, o["da"].data_ptr(), dt, None))
    run.keep = (keep, xg)
    return run, o


def cases(h, g):
    for s in ((1, 24, 40, 9, 7), (2, 3, 64, 16, 16), (3, 128, 256, 6, 10)):
        yield f"f32 conv {s}", 0, 0, conv_case(h, g, 0, *s)
    yield "f32 pool+concat", 0, 0, pool_concat_case(h, g, 0)
    for s in ((2, 16, 8, 8, 8), (2, 64, 32, 5, 7)):
        yield f"f32 convT {s}", 0, 0, convT_case(h, g, 0, *s)
    for dt, name in ((1, "bf16"), (2, "f16")):
        for s in ((1, 24, 40, 9, 7), (2, 3, 64, 16, 16)):
            yield f"{name} conv {s}", dt, 0, conv_case(h, g, dt, *s)
        yield f"{name} pool+concat", dt, 0, pool_concat_case(h, g, dt)
        yield f"{name} convT (2, 40, 24, 6, 5)", dt, 0, convT_case(h, g, dt, 2, 40, 24, 6, 5)
    yield "f32x3/bit30 conv (3, 64+64, 128, 9, 21)", 3, 1 << 30, conv_case(h, g, 3, 3, 128, 128, 9, 21, nsrc=2)
    yield "f32x3/bit30 convT (2, 128, 64, 5, 7)", 3, 1 << 30, convT_case(h, g, 3, 2, 128, 64, 5, 7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", default=["libustrun_parent.so", "libustrun_parent2.so", "libustrun.so"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-time", action="store_true")
    a = ap.parse_args()
    assert len(a.libs) == 3, "baseline, its control copy, the new build"
    names = ("parent", "control", "new")
    hs = [load(p) for p in a.libs]
    g = torch.Generator().manual_seed(11)

    bad = 0
    for title, dt, flags, (run, outs) in cases(hs[0], g):       # (packing runs on the baseline: the packed layouts are not what changed)
        got = []
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
        for k in outs:
            for other in (1, 2):
                same = torch.equal(got[0][k], got[other][k]) and not bool(torch.isnan(got[0][k].float()).any())
                bad += not same
                print(f"bits {title:42s} {k:6s} parent vs {names[other]:8s}: {'bit-equal' if same else 'DIFFERENT'}")
    print("BITS:", "all bit-equal" if not bad else f"{bad} DIFFERENT")
    if a.no_time:
        return 1 if bad else 0

    # ---- speed: the f32 3x3 forward / input gradient of a mid-size layer of the f32 U-Net (fundus 256 x 256, base 64, 16 images: the
    # 128 -> 128 convolution at 128 x 128, tools/bench_layers.py), the generic 16-bit kernel on (1, 24, 40, 9, 7) with every extent
    # x 32 (16 images of 288 x 224), the f32x3 ConvTranspose pair of that U-Net's third up-step (256 -> 128 at 64 x 64 -> 128 x 128)
    timed = []
    run, _ = conv_case(hs[0], g, 0, 16, 128, 128, 128, 128)
    timed += [("f32 fwd   16x128->128 128x128", 0, run.fwd, run), ("f32 dgrad 16x128->128 128x128", 0, run.dgrad, run)]
    run, _ = conv_case(hs[0], g, 1, 16, 24, 40, 288, 224)
    timed += [("bf16 fwd   16x24->40 288x224", 0, run.fwd, run), ("bf16 dgrad 16x24->40 288x224", 0, run.dgrad, run)]
    run, _ = convT_case(hs[0], g, 3, 16, 256, 128, 64, 64)
    timed += [("f32x3 convT fwd+dgrad 16x256->128 64x64", 0, run, run)]
    band = []
    verdicts = []
    for title, flags, fn, _keep in timed:
        ms = [[], [], []]
        for r in range(a.rounds):
            for i, h in enumerate(hs):
                old = h.ustrun_debug_flags(flags)
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
        band += list(c / p)
        verdicts.append((title, float(np.median(n / p))))
        print(f"time {title:40s}: parent {np.median(p):8.1f} us  control {np.median(c):8.1f} us  new {np.median(n):8.1f} us   control/parent per round "
              f"{(c / p).min():.3f}..{(c / p).max():.3f} (median {np.median(c / p):.3f})   new/parent median {np.median(n / p):.3f} "
              f"({(n / p).min():.3f}..{(n / p).max():.3f})")
    lo, hi = min(band), max(band)
    print(f"CONTROL BAND (control / parent, every round of every shape): {lo:.3f}..{hi:.3f}")
    for title, m in verdicts:
        print(f"  {title:40s}: new/parent median {m:.3f} -> {'inside' if lo <= m <= hi else ('FASTER than the band' if m < lo else 'SLOWER than the band')}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
