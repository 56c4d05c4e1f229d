"""Cost of the per-case post-processing (ustrun_post_process_3d: cavities filled, small 26-connected components removed, largest
component kept) alone and in validate_volumes.

  * `F.post_process_3d` on one case: 16 x 288 x 288 x 3 parts (M&Ms-like), 32 x 384 x 384 x 1 (prostate-like) and a 64^3 cube, each
    on SPECKLE (the stacked predictions of a random-init model; thresholded noise for the cube: the worst case, thousands of
    components and cavities) and on a BLOB (nested ellipsoids with a cavity and a few stray specks: what a trained model gives).
    Device events over back-to-back calls, every launch and the work-buffer allocation from torch's cache included, the shader
    clock read meanwhile; with both steps, with largest-only added, as the plain decode, and with every z-pair united
    (ustrun_debug_flags2 bit 7: the z-merge without its redundancy rules);
  * the route a user has without it: D2H copy, scipy binary_fill_holes + label (3 x 3 x 3) + the reference's loop, H2D copy, as
    volumes/s over --procs worker processes (each part of a case is one job);
  * `validate_volumes` on a synthetic resident pool with and without `post_process=True`, as cases/s (host clock around runs that
    end in a device synchronise, alternating, median over --repeats);
  * `--loop CASE`: nothing but 200 calls on that case's speckle, for a kernel trace taken in a run of its own
    (rocprofv3 --kernel-trace --stats -- python tools/bench_postprocess3d.py --loop mnms): the share of each launch.

    python tools/bench_postprocess3d.py [--dtype bf16] [--repeats 5] [--procs 16]
"""
import argparse
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ust-run_amd"))
sys.path.insert(0, HERE)

CASES = {"mnms": ("MNMS", 16, 288), "prostate": ("prostate", 32, 384), "cube": (None, 64, 64)}


def scipy_volume(p):
    """the reference's post_processing on a volume, skimage's label restated with scipy's (full 3 x 3 x 3 structure)"""
    import scipy.ndimage as nd
    f = nd.binary_fill_holes(p)
    lab, n = nd.label(f, structure=np.ones((3, 3, 3)))
    total = f.sum()
    sizes = np.bincount(lab.ravel(), minlength=n + 1)          # (the reference sums a mask per component: far slower on speckle)
    f[(sizes / max(total, 1) < 0.2)[lab]] = 0
    return int(f.sum())


def blob(D, H, parts, seed):
    """class map [D,H,H]: nested ellipsoids, a cavity in the innermost, a few stray specks of class 1"""
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.mgrid[:D, :H, :H]
    m = np.zeros((D, H, H), np.int64)
    for c in range(parts):
        s = 1 - c / (parts + 0.5)
        m[((zz - D / 2) / (0.45 * D * s)) ** 2 + ((yy - H / 2) / (0.3 * H * s)) ** 2 + ((xx - H / 2) / (0.25 * H * s)) ** 2 <= 1] = c + 1
    m[D // 2 - 1:D // 2 + 1, H // 2 - 3:H // 2 + 3, H // 2 - 3:H // 2 + 3] = 0
    for _ in range(6):
        z, y, x = rng.integers(0, D), rng.integers(0, H - 4), rng.integers(0, H - 4)
        m[z, y:y + 3, x:x + 3] = 1
    return m


def volumes(name, dtype):
    """-> {kind: (tensor, kwargs of F.post_process_3d)}"""
    import torch
    dataset, D, H = CASES[name]
    if dataset is None:
        rng = np.random.default_rng(64)
        return {"speckle": (torch.from_numpy((rng.random((1, 1, D, H, H)) < 0.5).astype(np.float32)).cuda(), {}),
                "blob": (torch.from_numpy((blob(D, H, 1, 1) != 0).astype(np.float32)[None, None]).cuda(), {})}
    from bench_postprocess import centred_model, predictions
    from ustrun.evaluate import _part_kw
    from ustrun.trainer import DATASETS
    C, _, K = DATASETS[dataset][:3]
    parts = DATASETS[dataset][4]
    pred = predictions(dataset, centred_model(dataset, C, H, K, dtype), C, H, n=D)          # [D,H,H] class map
    kw = _part_kw(dataset)
    b = torch.from_numpy(blob(D, H, parts, 2)).cuda()
    return {"speckle": (pred[None].contiguous(), kw), "blob": (b[None].contiguous(), kw)}


class Pool:
    """what validate_volumes reads of a resident dataset: uint8 images / labels [n,H,W,C] on the device, names"""

    def __init__(self, dataset, cases, D, H, C):
        import torch
        rng = np.random.default_rng(5)
        parts = 3 if dataset == "MNMS" else 1
        truth = np.concatenate([blob(D, H, parts, 10 + k) for k in range(cases)])
        img = np.clip(truth * (200 // parts) + 20 + rng.normal(0, 25, truth.shape), 0, 255).astype(np.uint8)
        self.images = torch.from_numpy(np.repeat(img[..., None], C, -1)).cuda()
        if dataset == "prostate":
            lab = np.where(truth == 1, 0, 255).astype(np.uint8)[..., None]
        else:
            lab = np.stack([np.where(truth == c + 1, 255, 0) for c in range(3)], -1).astype(np.uint8)
        self.labels = torch.from_numpy(lab).cuda()
        self.names = ["case%03d_s%03d.png" % (k, z) for k in range(cases) for z in range(D)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--cases", type=int, default=4, help="cases per validate_volumes run")
    ap.add_argument("--loop", default="", choices=[""] + list(CASES))
    a = ap.parse_args()
    import torch
    from clock_probe import clock_mhz, probe
    from ustrun import _lib as L
    from ustrun import functional as F
    lib = L.lib()
    try:
        import scipy
        have_scipy = scipy.__version__
    except ImportError:
        have_scipy = None
    print(f"device {torch.cuda.get_device_name(0)}, dtype {a.dtype}, scipy {have_scipy}", flush=True)
    for name in ([a.loop] if a.loop else CASES):
        dataset, D, H = CASES[name]
        vols = volumes(name, a.dtype)
        if a.loop:
            x, kw = vols["speckle"]
            for _ in range(200):
                F.post_process_3d(x, **kw)
            torch.cuda.synchronize()
            print(f"{name}: 200 calls done", flush=True)
            return
        for kind, (x, kw) in vols.items():
            out = F.post_process_3d(x, **kw)
            plain = F.post_process_3d(x, fill_holes=False, min_share=None, **kw)
            filled = F.post_process_3d(x, min_share=None, **kw)
            parts = out.shape[1]
            print(f"{name} {kind} {D}x{H}x{H} x {parts} part(s): foreground {plain.sum().item():.0f} raw, {filled.sum().item():.0f} filled, "
                  f"{out.sum().item():.0f} kept; work buffer {lib.ustrun_post_process_3d_work_bytes(1, parts, D, H, H) / 2 ** 20:.1f} MiB", flush=True)
            for label, opts, flags in (("fill + removal", {}, 0), ("fill + removal + largest", dict(largest=True), 0),
                                       ("fill + removal, every z-pair united", {}, 128), ("fill only", dict(min_share=None), 0),
                                       ("decode only", dict(fill_holes=False, min_share=None), 0)):
                call = lambda: F.post_process_3d(x, **kw, **opts)
                old = lib.ustrun_debug_flags2(flags)
                try:
                    for _ in range(10):
                        call()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    reps = 100
                    pa = probe(lib)
                    e0.record()
                    for _ in range(reps):
                        call()
                    e1.record()
                    pb = probe(lib)
                    torch.cuda.synchronize()
                finally:
                    lib.ustrun_debug_flags2(old)
                ms = e0.elapsed_time(e1) / reps
                mhz, lo, hi, nx = clock_mhz(pa, pb)
                print(f"{name} {kind}: F.post_process_3d, {label:36s}: {ms:.3f} ms per case ({1e3 / ms:.0f} cases/s, "
                      f"{D * H * H * parts / ms / 1e6:.2f} Gvoxel/s); shader clock {mhz:.0f} MHz ({lo:.0f}-{hi:.0f} over {nx} XCDs)", flush=True)
            if have_scipy:
                t0 = time.perf_counter()
                p = plain.cpu().numpy().astype(bool)
                d2h = time.perf_counter() - t0
                jobs = [p[0, k] for k in range(parts)] * a.procs
                with mp.get_context("spawn").Pool(a.procs) as pool:
                    pool.map(scipy_volume, jobs[:a.procs])             # the workers import scipy before the clock starts
                    t0 = time.perf_counter()
                    pool.map(scipy_volume, jobs, chunksize=1)
                    dt = time.perf_counter() - t0
                t0 = time.perf_counter()
                torch.from_numpy(p.astype(np.float32)).cuda()
                torch.cuda.synchronize()
                h2d = time.perf_counter() - t0
                print(f"{name} {kind}: host route, {a.procs} processes: {len(jobs) / parts / dt:.1f} cases/s "
                      f"({dt / len(jobs) * a.procs * 1e3:.1f} ms per part per process; copies {d2h * 1e3:.1f} + {h2d * 1e3:.1f} ms per case)", flush=True)
        if dataset is None:
            continue
        from bench_postprocess import centred_model
        from ustrun.evaluate import validate_volumes
        from ustrun.trainer import DATASETS
        C, _, K = DATASETS[dataset][:3]
        model, pool = centred_model(dataset, C, H, K, a.dtype), Pool(dataset, a.cases, D, H, C)

        def timed(post):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            validate_volumes(dataset, model, [pool], r"(case\d+)_", log=None, post_process=post)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        for post in (False, True):
            timed(post)
        t = {False: [], True: []}
        for _ in range(a.repeats):
            for post in (False, True):
                t[post].append(timed(post))
        med = {k: statistics.median(v) for k, v in t.items()}
        print(f"{name} validate_volumes, {a.cases} cases of {D} slices ({a.repeats} runs): post_process off {a.cases / med[False]:.2f} cases/s, "
              f"on {a.cases / med[True]:.2f} cases/s; added {(med[True] - med[False]) / a.cases * 1e3:.2f} ms per case "
              f"({(med[True] / med[False] - 1) * 100:+.1f} %)", flush=True)


if __name__ == "__main__":
    main()
