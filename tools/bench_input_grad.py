#!/usr/bin/env python3
"""The input gradient of the first convolution (ustrun_conv_first_dgrad) alone, beside the weight gradient of the same layer on the
same tensors (ustrun_conv3x3_wgrad: it reads the same dy), and the whole-network backward with and without dx; then the input
gradient of the DeepLabV2-ResNet stem (ustrun_conv_stem_dgrad: 7x7, stride 2) alone.  Development tool.

    python3 tools/bench_input_grad.py [--reps 20] [--dtype bf16,f32] [--net 1] [--stem 1]

Per case: kernel ms, the algorithmic bytes N*H*W*(Cout*esz + 4*Cin) over that time, and their share of the 8 TB/s HBM peak.
--net 1: UNet(3, 2) at BASELINE.json configs[1]'s shape (32 x 3 x 256^2), the backward alone (events around .backward()).
--stem 1: per case kernel ms, the algorithmic FMAs N*Ho*Wo*Cout*147 (every dy element meets 49 taps x 3 channels; the border's
missing taps are not subtracted) over that time, and their share of the f32 VALU peak (157.3 TFLOP/s = 78.65 TFMA/s).
"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ust-run_amd"))
from ustrun import _lib as l  # noqa: E402

HBM_PEAK = 8.0e12
VALU_FMA_PEAK = 157.3e12 / 2
STEM_CASES = [(16, 512), (16, 256)]       # (N, H = W): BASELINE.json configs[4]'s batch at BUSI's 512^2, and at 256^2
# (N, Cin, H = W): Fundus (configs[1]), Prostate (configs[2]), M&Ms (configs[3]) per-device batches
CASES = [(16, 3, 256), (8, 1, 384), (8, 1, 288)]


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(dtype, reps):
    lib = l.lib()
    dt = {"bf16": l.BF16, "f16": l.F16, "f32": l.F32, "f32x3": l.F32X3}[dtype]
    st = {"bf16": torch.bfloat16, "f16": torch.float16}.get(dtype, torch.float32)
    esz, cout = (2 if st != torch.float32 else 4), 64
    print(f"{'case':22s} {'MB':>7s} {'dgrad ms':>9s} {'TB/s':>6s} {'% HBM':>6s} {'wgrad ms':>9s} {'dgrad/wgrad':>11s}")
    for n, cin, hw in CASES:
        dy = torch.randn(n, hw, hw, cout, device="cuda").to(st)
        x = torch.randn(n, cin, hw, hw, device="cuda")
        w = torch.randn(cout, cin, 3, 3, device="cuda") * 0.1
        dx = torch.empty(n, cin, hw, hw, device="cuda")
        dw = torch.empty_like(w)
        src = l.nchw_src(x.data_ptr(), cin, hw, hw)
        pb = lib.ustrun_wgrad_partials_bytes(9, cin, cout, n * hw * hw)
        part = torch.empty(pb // 4, device="cuda")
        dg = lambda: l.check(lib.ustrun_conv_first_dgrad(dy.data_ptr(), w.data_ptr(), n, hw, hw, cout, cin, dx.data_ptr(), dt, None), "dgrad")
        wg = lambda: l.check(lib.ustrun_conv3x3_wgrad(C.byref(src), 1, dy.data_ptr(), n, hw, hw, cout, dw.data_ptr(), 0, part.data_ptr(), pb,
                                                      dt, None), "wgrad")
        ms_d, ms_w = timed(dg, reps), timed(wg, reps)
        by = n * hw * hw * (cout * esz + 4 * cin)
        print(f"{dtype:5s} N={n:<2d} C={cin} {hw}^2   {by / 1e6:7.1f} {ms_d:9.4f} {by / ms_d / 1e9:6.2f} {100 * by / (ms_d * 1e-3) / HBM_PEAK:6.1f} "
              f"{ms_w:9.4f} {ms_d / ms_w:11.2f}", flush=True)


def stem_kernels(dtype, reps):
    lib = l.lib()
    dt = {"bf16": l.BF16, "f16": l.F16, "f32": l.F32, "f32x3": l.F32X3}[dtype]
    st = {"bf16": torch.bfloat16, "f16": torch.float16}.get(dtype, torch.float32)
    esz, cout = (2 if st != torch.float32 else 4), 64
    print(f"{'stem case':22s} {'GFMA':>7s} {'MB':>7s} {'dgrad ms':>9s} {'TFMA/s':>7s} {'% VALU':>7s} {'TB/s':>6s}")
    for n, hw in STEM_CASES:
        ho = (hw - 1) // 2 + 1
        dy = torch.randn(n, ho, ho, cout, device="cuda").to(st)
        w = torch.randn(cout, 3, 7, 7, device="cuda") * 0.1
        dx = torch.empty(n, 3, hw, hw, device="cuda")
        dg = lambda: l.check(lib.ustrun_conv_stem_dgrad(dy.data_ptr(), w.data_ptr(), n, hw, hw, cout, 3, dx.data_ptr(), dt, None), "stem dgrad")
        ms = timed(dg, reps)
        fma = n * ho * ho * cout * 147
        by = n * ho * ho * cout * esz + n * hw * hw * 12
        print(f"{dtype:5s} N={n:<2d} C=3 {hw}^2   {fma / 1e9:7.2f} {by / 1e6:7.1f} {ms:9.4f} {fma / ms / 1e9:7.2f} "
              f"{100 * fma / (ms * 1e-3) / VALU_FMA_PEAK:7.1f} {by / ms / 1e9:6.2f}", flush=True)


def network(dtype, reps):
    from networks.unet_model import UNet
    torch.manual_seed(0)
    m = UNet(3, 2, dtype=dtype).cuda().train()
    x = torch.randn(32, 3, 256, 256, device="cuda")
    out = {}
    for want_dx in (False, True, False, True):                  # alternating: the two arms see the same clocks
        tot = 0.0
        for i in range(reps + 2):
            xg = x.clone().requires_grad_(want_dx)
            loss = m(xg).square().mean()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss.backward()
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                tot += e0.elapsed_time(e1)
        out.setdefault(want_dx, []).append(tot / reps)
    for k in (False, True):
        print(f"UNet(3,2) {dtype} 32x3x256^2 backward {'with   ' if k else 'without'} dx: " + ", ".join(f"{v:.3f} ms" for v in out[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dtype", default="bf16,f32")
    ap.add_argument("--net", type=int, default=1)
    ap.add_argument("--stem", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_grad: no GPU (there is nothing to time without one)")
    for dtype in a.dtype.split(","):
        kernels(dtype, a.reps)
    if a.net:
        network("bf16", max(3, a.reps // 4))
    if a.stem:
        for dtype in a.dtype.split(","):
            stem_kernels(dtype, a.reps)


if __name__ == "__main__":
    main()
