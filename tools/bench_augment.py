#!/usr/bin/env python3
"""Times ResidentLoader.__next__ (ust-run_amd/ustrun/datasets.py) at 16 + 16 images for the three U-Net datasets, split per
kernel entry, next to the training step's time (README: 26.1-27.4 ms at Fundus 256^2 16 + 16; `--step_ms` to give another).

    python tools/bench_augment.py [--iters 20] [--step_ms 26.7]

Pools are noise (the kernels' cost does not depend on the pixel values); per-entry times are HIP-event times of that entry
run alone on the batch the previous entries produced, every gate on (the worst case: each gate is on for half the samples in
training); the loader line is wall time per __next__ with the sampler's own gates, device synchronised."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ust-run_amd"))
from ustrun import datasets as D  # noqa: E402


class Pool:
    def __init__(self, dataset, n, dev):
        s = D.SPECS[dataset]
        self.dataset, self.patch = dataset, s["patch"]
        g = torch.Generator().manual_seed(1)
        self.images = torch.randint(0, 256, (n, self.patch, self.patch, s["C"]), generator=g, dtype=torch.uint8).to(dev)
        self.labels = torch.randint(0, 2, (n, self.patch, self.patch, s["Cl"]), generator=g, dtype=torch.uint8).to(dev) * 255

    def __len__(self):
        return self.images.shape[0]


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--step_ms", type=float, default=26.7)
    args = ap.parse_args()
    dev = torch.device("cuda")
    print(f"date {time.strftime('%Y-%m-%d')}, {torch.cuda.get_device_name(0)}, {args.bs} + {args.bs} images, step {args.step_ms} ms (Fundus 256^2)")
    for ds in ("fundus", "prostate", "BUSI"):
        pool = Pool(ds, 64, dev)
        P, B = pool.patch, args.bs
        rows = D.AugmentSampler(ds, P, 3).batch(0, B)
        rows[:, D.SC], rows[:, D.ROT], rows[:, D.EL] = 1, 1, 1
        rows[:, D.SC + 1:D.SC + 6] = [int(1.3 * P), int(1.2 * P), 0, 11, 7]
        rows[:, D.ROT + 4:D.ROT + 22] = D.rotate_words(13, P, P)
        p = torch.from_numpy(rows).to(dev)
        idx = torch.arange(B, dtype=torch.int32, device=dev)
        t = {}
        t["gather"], (img, lab) = timed(lambda: D.stage_gather(pool.images, pool.labels, idx), args.iters)
        t["scale_crop"], (img, lab) = timed(lambda: D.stage_scale_crop(img, lab, p, P), args.iters)
        t["rotate"], (img, lab) = timed(lambda: D.stage_rotate(img, lab, p), args.iters)
        t["elastic_field"], field = timed(lambda: D.stage_elastic_field(p, B, P, P, 5), args.iters)
        t["elastic_warp"], (img, lab) = timed(lambda: D.stage_elastic_warp(img, lab, field, p), args.iters)
        t["strong"], s = timed(lambda: D.stage_strong(img, p, D.blur_radius(P)), args.iters)
        t["finish"], _ = timed(lambda: D.stage_finish(img, s, lab), args.iters)
        ld = D.ResidentLoader(pool, pool, B, B, seed=7)
        next(ld)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            next(ld)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / args.iters * 1e3
        weak = sum(t[k] for k in ("gather", "scale_crop", "rotate", "elastic_field", "elastic_warp"))
        both = 2 * weak + t["strong"] + 2 * t["finish"]
        print(f"{ds} {P}^2: " + ", ".join(f"{k} {v:.3f}" for k, v in t.items()) + f" ms per {B} images, every gate on")
        print(f"    kernels for {B} + {B}: {both:.3f} ms; ResidentLoader.__next__ wall {wall:.3f} ms = {100 * wall / args.step_ms:.1f} % of the step")


if __name__ == "__main__":
    main()
