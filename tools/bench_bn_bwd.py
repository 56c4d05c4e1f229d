#!/usr/bin/env python3
"""GPU box: the BatchNorm(+ReLU, +MaxPool routing) backward passes through the C ABI at the U-Net's shapes (bf16): time and
algorithmic GB/s of ustrun_bn_bwd_reduce (reads y, da [, dp]), ustrun_bn_bwd_apply (the same reads + one write) and
ustrun_bn_bwd_frozen (one pass: the same reads + one write, with and without the sums).

    python tools/bench_bn_bwd.py [--n 64] [--reps 10]

A/B of builds of the library loaded side by side in one process (the first is the baseline, a second copy of it gives the noise
band; paths relative to ust-run_amd/ustrun/): bit equality of every output of every entry point of csrc/bn.hip's backward half on
random data at the smallest shapes that reach each arm, the U-Net's backward and one training step (the multi-pass reduce and
apply) in a process per library, then interleaved timing rounds.

    python tools/bench_bn_bwd.py --ab [libustrun_parent.so libustrun_parent2.so libustrun.so] [--n 16] [--rounds 9] [--reps 20] [--no-time]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PKG = os.path.join(ROOT, "ust-run_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)
from ustrun import _lib as l  # noqa: E402

DEV = "cuda"
TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
DTN = {0: "f32", 1: "bf16", 2: "f16"}
SHAPES = [(64, 256, False), (64, 256, True), (128, 128, False), (128, 128, True), (256, 64, False), (256, 64, True), (512, 32, False),
          (512, 32, True), (1024, 16, False)]


def load(name):
    h = C.CDLL(os.path.join(PKG, "ustrun", name))
    for fn, (res, args) in l.SIGNATURES.items():
        f = getattr(h, fn)
        f.restype, f.argtypes = res, args
    return h


def ck(h, rc):
    if rc:
        raise RuntimeError(h.ustrun_last_error().decode())


class Layer:
    """one BatchNorm + ReLU (+ MaxPool) layer's tensors, `passes` forward passes stacked along N; the outputs are refilled by the
    caller before a run"""

    def __init__(self, g, dt, n, c, h, w, pool, passes=1, with_da=True):
        t = TDT[dt]
        r = lambda *s: torch.randn(*s, generator=g)
        self.dt, self.n, self.c, self.h, self.w, self.passes = dt, n, c, h, w, passes
        self.y = r(passes * n, h, w, c).to(DEV).to(t)
        self.da = r(passes * n, h, w, c).to(DEV).to(t) if with_da else None
        self.dp = r(passes * n, h // 2, w // 2, c).to(DEV).to(t) if pool else None
        k = torch.stack([torch.rand(passes, c, generator=g) + 0.5, 0.1 * r(passes, c), 0.1 * r(passes, c), torch.rand(passes, c, generator=g) + 0.5], 1)
        self.k = k.contiguous().to(DEV)                      # [pass][scale, shift, mean, rstd][C]
        self.gamma = (torch.rand(c, generator=g) + 0.5).to(DEV)
        self.pb = 1024 * 2 * c * 4
        self.out = {"dy": torch.zeros(passes * n, h, w, c, device=DEV, dtype=t), "dgamma": torch.zeros(c, device=DEV),
                    "dbeta": torch.zeros(c, device=DEV), "coef": torch.zeros(passes, 3, c, device=DEV), "part": torch.zeros(self.pb // 4, device=DEV)}

    def k_(self, i):
        return self.k.data_ptr() + 4 * i * self.c

    def reduce(self, h, acc=0):
        o = self.out
        ck(h, h.ustrun_bn_bwd_reduce(l.ptr(self.da), l.ptr(self.dp), self.y.data_ptr(), self.k_(0), self.k_(1), self.k_(2), self.k_(3), self.gamma.data_ptr(),
                                     self.n, self.h, self.w, self.c, o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), acc, o["coef"].data_ptr(),
                                     o["part"].data_ptr(), self.pb, self.dt, None))

    def apply(self, h):
        o = self.out
        ck(h, h.ustrun_bn_bwd_apply(l.ptr(self.da), l.ptr(self.dp), self.y.data_ptr(), self.k_(0), self.k_(1), o["coef"].data_ptr(), self.n, self.h, self.w,
                                    self.c, o["dy"].data_ptr(), self.dt, None))

    def frozen(self, h, sums=True, acc=0):
        o = self.out
        dg, db = (o["dgamma"].data_ptr(), o["dbeta"].data_ptr()) if sums else (None, None)
        if self.passes == 1:
            ck(h, h.ustrun_bn_bwd_frozen(l.ptr(self.da), l.ptr(self.dp), self.y.data_ptr(), self.k_(0), self.k_(1), self.k_(2), self.k_(3), self.n, self.h,
                                         self.w, self.c, o["dy"].data_ptr(), dg, db, acc, o["part"].data_ptr(), self.pb, self.dt, None))
        else:
            ck(h, h.ustrun_bn_bwd_frozen_passes(l.ptr(self.da), l.ptr(self.dp), self.y.data_ptr(), self.k_(0), self.k_(1), self.k_(2), self.k_(3), self.n,
                                                self.h, self.w, self.c, o["dy"].data_ptr(), dg, db, acc, o["part"].data_ptr(), self.pb, self.dt, self.passes,
                                                4 * self.c, None))


def snapshots(run, outs, hs, flags=0):
    """run(h, record) on every library from the same starting state of `outs`; record(tag) clones every output under that tag"""
    got = []
    for h in hs:
        for i, v in enumerate(outs.values()):
            v.fill_(3.0 + i)
        snap = {}
        old = h.ustrun_debug_flags(flags)
        try:
            run(h, lambda tag: (torch.cuda.synchronize(), snap.update({f"{tag}.{k}": v.clone() for k, v in outs.items()})))
        finally:
            h.ustrun_debug_flags(old)
        got.append(snap)
    return got


def layer_runs(L):
    def run(h, rec):
        L.reduce(h); L.apply(h); rec("reduce+apply")
        L.reduce(h, acc=1); rec("reduce accumulate")
        L.frozen(h, True); rec("frozen sums")
        L.frozen(h, True, acc=1); rec("frozen sums accumulate")
        L.frozen(h, False); rec("frozen no sums")
    return run


def head_case(g, dt, K, passes, n=2, hh=9, ww=7):
    c = 64
    L = Layer(g, dt, n, c, hh, ww, False, passes)
    dl = torch.randn(passes * n, K, hh, ww, generator=g).to(DEV)
    wh = torch.randn(K, c, generator=g).to(DEV)
    coef = torch.randn(passes, 3, c, generator=g).to(DEV)
    outs = {"dy": L.out["dy"]}

    def run(h, rec):
        ck(h, h.ustrun_bn_bwd_apply_head(dl.data_ptr(), wh.data_ptr(), L.y.data_ptr(), L.k_(0), L.k_(1), coef.data_ptr(), n, hh, ww, c, K,
                                         outs["dy"].data_ptr(), dt, passes, 4 * c, None))
        rec("apply_head")
    run.keep = (L, dl, wh, coef)
    return run, outs


def stat_case(g, rows, c, passes):
    stat0 = torch.randn(passes, rows, 2, c, generator=g).to(DEV)
    k = (torch.rand(passes, 4, c, generator=g) + 0.5).to(DEV)
    gamma = (torch.rand(c, generator=g) + 0.5).to(DEV)
    outs = {"stat": torch.zeros_like(stat0), "dgamma": torch.zeros(c, device=DEV), "dbeta": torch.zeros(c, device=DEV),
            "coef": torch.zeros(passes, 3, c, device=DEV)}

    def run(h, rec):
        for acc in (0, 1):
            outs["stat"].copy_(stat0)             # (the staged path rewrites the table in place)
            ck(h, h.ustrun_bn_bwd_finalize_stat(outs["stat"].data_ptr(), rows, passes, c, 4321, gamma.data_ptr(), k.data_ptr() + 8 * c, k.data_ptr() + 12 * c,
                                                4 * c, outs["dgamma"].data_ptr(), outs["dbeta"].data_ptr(), acc, outs["coef"].data_ptr(), None))
            rec(f"finalize_stat acc={acc}")
    run.keep = (stat0, k, gamma)
    return run, outs


def bit_cases(g):
    """(title, debug flags, run, outputs): (N, C, H, W) the smallest that reach each arm"""
    def layer(title, dt, s, pool, flags=0, passes=1, with_da=True):
        n, c, hh, ww = s
        L = Layer(g, dt, n, c, hh, ww, pool, passes, with_da)
        run = layer_runs(L)
        run.keep = L
        return f"{DTN[dt]} {title} {s}", flags, run, L.out
    for dt in (1, 2):
        for s in ((2, 64, 12, 16), (3, 8, 9, 7), (2, 2048, 3, 5)):
            yield layer("plain x8", dt, s, False)
    yield layer("plain x4", 0, (3, 24, 5, 7), False)
    yield layer("plain x4", 1, (2, 96, 8, 8), False)
    yield layer("plain x4 flag 4096", 1, (2, 64, 12, 16), False, flags=4096)
    for dt in (0, 1):
        yield layer("plain two rounds", dt, (1, 1032, 3, 5), False)
        yield layer("pooled two rounds", dt, (1, 1032, 4, 6), True)
    for dt in (0, 1, 2):
        for s in ((2, 64, 12, 16), (1, 8, 6, 4)):
            yield layer("pooled even", dt, s, True)
        for s in ((2, 64, 11, 15), (1, 24, 9, 7)):
            yield layer("pooled odd", dt, s, True)
        yield layer("pooled da=NULL", dt, (2, 16, 8, 12), True, with_da=False)
    for dt in (0, 1):
        yield layer("3 passes plain", dt, (2, 16, 8, 12), False, passes=3)
        yield layer("3 passes pooled", dt, (2, 16, 8, 12), True, passes=3)
    # a 16-bit output hides an f32 statement that two builds contract differently in all but about one element in 2^16 (bf16) or
    # 2^13 (f16): 8M elements show it where the small shapes cannot
    for dt in (1, 2):
        yield layer("large plain x8", dt, (8, 64, 128, 128), False)
        yield layer("large plain x4 flag 4096", dt, (8, 64, 128, 128), False, flags=4096)
        yield layer("large pooled even", dt, (8, 64, 128, 128), True)
        yield layer("large pooled odd", dt, (8, 64, 127, 129), True)
    for dt in (1, 2):
        for K in (2, 4, 3):
            run, outs = head_case(g, dt, K, 2)
            yield f"{DTN[dt]} apply_head C=64 (2, ., 9, 7) K={K} 2 passes", 0, run, outs
        run, outs = head_case(g, dt, 2, 1, 8, 128, 128)
        yield f"{DTN[dt]} large apply_head C=64 (8, ., 128, 128) K=2", 0, run, outs
    for rows, c, what in ((96, 64, "staged"), (40, 24, "direct")):
        run, outs = stat_case(g, rows, c, 2)
        yield f"finalize_stat {rows} rows x C={c} ({what}) 2 passes", 0, run, outs


def unet_child(out_path):
    """the U-Net's backward (every parameter gradient and the input gradient, f32 and bf16) and one semi-supervised step (whose backward
    runs the multi-pass reduce and apply) at the smallest configuration of tests/test_gpu_step.py, with the library USTRUN_LIB names"""
    import random
    from networks.unet_model import UNet
    from oracle import unet_ref as U
    from ustrun.trainer import SSLTrainer
    res = {}
    for dtype in ("f32", "bf16"):
        torch.manual_seed(1)
        sd = U.make_state_dict(1, 2, base=8)
        m = UNet(1, 2, base_channels=8, dtype=dtype)
        m.load_state_dict({k: v.clone() for k, v in sd.items()})
        m = m.cuda().train()
        x = torch.randn(2, 1, 32, 32, generator=torch.Generator().manual_seed(5)).cuda().requires_grad_(True)
        m(x).square().mean().backward()
        res[f"{dtype} grad x"] = x.grad.cpu()
        for n_, p in m.named_parameters():
            res[f"{dtype} grad {n_}"] = p.grad.cpu()
        torch.manual_seed(1)
        stu, tea = UNet(1, 2, base_channels=8, dtype=dtype), UNet(1, 2, base_channels=8, dtype=dtype)
        stu.load_state_dict({k: v.clone() for k, v in sd.items()})
        tea.load_state_dict({k: v.clone() for k, v in U.make_state_dict(1, 2, base=8).items()})
        trn = SSLTrainer("prostate", stu.cuda(), tea.cuda(), max_iterations=300, threshold=0.52, patch_size=32, num_eval_iter=2)
        g = torch.Generator().manual_seed(100)
        img = lambda: torch.randint(0, 256, (2, 1, 32, 32), generator=g).float() / 127.5 - 1
        lab = lambda: torch.tensor([0.0, 255.0])[torch.randint(0, 2, (2, 32, 32), generator=g)]
        random.seed(7); np.random.seed(7)
        trn.step(*[t.cuda() for t in (img(), lab(), img(), img(), lab())], epoch_start=True)
        for k, v in stu.state_dict().items():
            res[f"{dtype} step student {k}"] = v.cpu()
    torch.save(res, out_path)


def ab(a):
    assert len(a.libs) == 3, "baseline, its control copy, the new build"
    names = ("parent", "control", "new")
    hs = [load(p) for p in a.libs]
    g = torch.Generator().manual_seed(11)
    bad = n_cmp = 0
    for title, flags, run, outs in bit_cases(g):
        got = snapshots(run, outs, hs, flags)
        for other in (1, 2):
            diff = [k for k in got[0] if not torch.equal(got[0][k], got[other][k]) or bool(torch.isnan(got[0][k].float()).any())]
            n_cmp += len(got[0])
            bad += len(diff)
            print(f"bits {title:58s} parent vs {names[other]:8s}: {len(got[0])} tensors {'bit-equal' if not diff else 'DIFFERENT: ' + ', '.join(diff)}", flush=True)
    with tempfile.TemporaryDirectory() as d:
        res = []
        for i, p in enumerate(a.libs):
            out = os.path.join(d, f"unet{i}.pt")
            env = dict(os.environ, USTRUN_LIB=os.path.join(PKG, "ustrun", p))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--unet-grads", out], env=env, check=True, timeout=240)
            res.append(torch.load(out))
        for other in (1, 2):
            diff = [k for k in res[0] if not torch.equal(res[0][k], res[other][k])]
            n_cmp += len(res[0])
            bad += len(diff)
            print(f"bits U-Net (2, 1, 32, 32) base 8, f32 and bf16: backward + one SSL step parent vs {names[other]:8s}: {len(res[0])} tensors "
                  f"{'bit-equal' if not diff else 'DIFFERENT: ' + ', '.join(diff)}", flush=True)
    print("BITS:", f"all {n_cmp} comparisons bit-equal" if not bad else f"{bad} of {n_cmp} DIFFERENT", flush=True)
    if a.no_time:
        return 1 if bad else 0

    band, verdicts = [], []
    for c, hw, pool in SHAPES:
        L = Layer(g, 1, a.n, c, hw, hw, pool)
        ops = [("reduce", L.reduce), ("apply", L.apply), ("frozen", lambda h: L.frozen(h, False))]
        if c == 64:
            ops.append(("frozen+sums", lambda h: L.frozen(h, True)))
        for op, fn in ops:
            title = f"C={c:4d} {hw:3d}x{hw:<3d} N={a.n} {'pool ' if pool else 'plain'} {op}"
            ms = [[], [], []]
            for r in range(a.rounds):
                for i, h in enumerate(hs):
                    fn(h)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        fn(h)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[i].append(e0.elapsed_time(e1) / a.reps * 1e3)
            p, q, n = (np.array(v) for v in ms)
            band += list(q / p)
            verdicts.append((title, float(np.median(n / p))))
            print(f"time {title:44s}: parent {np.median(p):7.1f} us  control {np.median(q):7.1f} us  new {np.median(n):7.1f} us   control/parent "
                  f"{(q / p).min():.3f}..{(q / p).max():.3f}   new/parent median {np.median(n / p):.3f} ({(n / p).min():.3f}..{(n / p).max():.3f})", flush=True)
        del L
    lo, hi = min(band), max(band)
    print(f"CONTROL BAND (control / parent, every round of every shape): {lo:.3f}..{hi:.3f}")
    for title, m in verdicts:
        print(f"  {title:44s}: new/parent median {m:.3f} -> {'inside' if lo <= m <= hi else ('FASTER than the band' if m < lo else 'SLOWER than the band')}")
    return 1 if bad else 0


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", default=["libustrun_parent.so", "libustrun_parent2.so", "libustrun.so"])
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--unet-grads", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.unet_grads:
        return unet_child(a.unet_grads)
    if a.ab:
        a.n, a.reps = a.n or 16, a.reps or 20
        return ab(a)
    n, reps = a.n or 64, a.reps or 10
    h = l.lib()
    g = torch.Generator().manual_seed(3)
    tot = [0.0] * 4
    for c, hw, pool in SHAPES:
        L = Layer(g, 1, n, c, hw, hw, pool)
        ts = [timed(f, reps) for f in (lambda: L.reduce(h), lambda: L.apply(h), lambda: L.frozen(h, False), lambda: L.frozen(h, True))]
        t = n * hw * hw * c * 2.0
        br = t * (2.25 if pool else 2.0)
        ba = br + t
        tot = [x + y for x, y in zip(tot, ts)]
        print(f"C={c:4d} {hw:3d}x{hw:<3d} N={n} {'pool ' if pool else 'plain'}: reduce (+ finalize) {ts[0] * 1e3:7.1f} us {br / ts[0] / 1e6:6.0f} GB/s | "
              f"apply {ts[1] * 1e3:7.1f} us {ba / ts[1] / 1e6:6.0f} GB/s | frozen {ts[2] * 1e3:7.1f} us {ba / ts[2] / 1e6:6.0f} GB/s | "
              f"frozen + sums (+ finalize) {ts[3] * 1e3:7.1f} us {ba / ts[3] / 1e6:6.0f} GB/s", flush=True)
        del L
    print(f"total: reduce {tot[0]:.3f} ms, apply {tot[1]:.3f} ms, frozen {tot[2]:.3f} ms, frozen + sums {tot[3]:.3f} ms")
    return 0


if __name__ == "__main__":
    sys.exit(main())
