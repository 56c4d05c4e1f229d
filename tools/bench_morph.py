"""Time of the chamfer / morphology entries (csrc/morph.hip) against the route they replace for labels that live on the device:
D2H copy, scipy.ndimage on one host core per part, H2D copy of the result.

Four operations, each at [32,2,256,256] (cup / disc planes: nested discs) and on one [1,1,64,384,384] volume (a few balls):
`boundary_band` at width 5 (the reference's GetBoundary, dataloaders/custom_transforms.py:630-647), `binary_closing` at 3
iterations, and `chamfer_distance` in both metrics (host: two distance_transform_cdt calls per part, one per sign).

Timing as tools/bench_sdf.py: windows of at least --seconds each, the routes alternating over --repeats windows, median
(min-max) per call; the device route with device events and the shader clock the chip held over the window read beside it
(tools/clock_probe.py), the host route, which waits for the device by its nature, with the wall clock.  Every device result is
compared with the host route's before it is timed.  Without scipy the device times are recorded alone, and the output says so.

    python tools/bench_morph.py [--repeats 5] [--seconds 0.25]
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ust-run_amd"))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402


def balls(rng, shape, n, rmin, rmax):
    grid = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    p = np.zeros(shape, bool)
    for _ in range(n):
        c = [rng.integers(s // 4, 3 * s // 4) for s in shape]
        r = rng.integers(int(rmin * min(shape)), int(rmax * min(shape)) + 1)
        p |= sum((g - ci) ** 2 for g, ci in zip(grid, c)) <= r * r
    return p


def cases():
    rng = np.random.default_rng(31)
    planes = np.zeros((32, 2, 256, 256), bool)
    for n in range(32):
        planes[n, 1] = balls(rng, (256, 256), 1, 0.15, 0.3)
        planes[n, 0] = balls(rng, (256, 256), 1, 0.05, 0.1) & planes[n, 1]
    vol = balls(rng, (64, 384, 384), 4, 0.2, 0.4)[None, None]
    return [("[32,2,256,256] planes", planes, 2), ("[1,1,64,384,384] volume", vol, 3)]


def host_ops(ndi):
    def band(p):
        out = np.zeros((p.shape[0],) + p.shape[2:], np.uint8)
        for n in range(p.shape[0]):
            for k in range(p.shape[1]):
                out[n] |= ndi.binary_dilation(p[n, k], iterations=5) ^ ndi.binary_erosion(p[n, k], iterations=5)
        return out

    def closing(p):
        return np.stack([np.stack([ndi.binary_closing(p[n, k], iterations=3) for k in range(p.shape[1])]) for n in range(p.shape[0])])

    def cdt(metric):
        def fn(p):
            out = np.zeros(p.shape, np.int32)
            for n in range(p.shape[0]):
                for k in range(p.shape[1]):
                    a = p[n, k]
                    if a.any() and not a.all():
                        out[n, k] = np.where(a, -ndi.distance_transform_cdt(a, metric=metric), ndi.distance_transform_cdt(~a, metric=metric))
                    else:                                  # no opposite kind: the entry's sentinel, + on an empty part, - on a full one
                        out[n, k] = -0x7fffffff if a.any() else 0x7fffffff
            return out
        return fn
    return {"boundary_band(5)": band, "binary_closing(3)": closing, "chamfer taxicab": cdt("taxicab"), "chamfer chessboard": cdt("chessboard")}


def dev_window(fn, reps, lib):
    import torch
    from clock_probe import clock_mhz, probe
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    pa = probe(lib)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    pb = probe(lib)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, clock_mhz(pa, pb)[0]


def wall_window(fn, reps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.25, help="least length of a timed window")
    a = ap.parse_args()
    import torch
    from ustrun import _lib as L
    from ustrun import functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_morph: no HIP device; nothing is measured on a CPU")
    lib = L.lib()
    try:
        import scipy
        from scipy import ndimage as ndi
        host = host_ops(ndi)
        note = f"host route: D2H + scipy {scipy.__version__} per part on one core + H2D, wall clock"
    except ImportError:
        host, note = None, "scipy is absent: device times alone"
    print(f"device {torch.cuda.get_device_name(0)}, {a.repeats} windows of >= {a.seconds} s each, median (min-max) ms per call; {note}", flush=True)
    for name, parts, rank in cases():
        x = torch.from_numpy(parts.astype(np.float32)).cuda()
        dev = {"boundary_band(5)": lambda: F.boundary_band(x, 5), "binary_closing(3)": lambda: F.binary_closing(x, iterations=3),
               "chamfer taxicab": lambda: F.chamfer_distance(x, "taxicab")[0], "chamfer chessboard": lambda: F.chamfer_distance(x, "chessboard")[0]}
        print(f"{name}: foreground {100 * parts.mean():.1f} % of the voxels", flush=True)
        for op, fn in dev.items():
            line = f"  {op:20s}"
            if host:
                route = lambda: torch.from_numpy(host[op]((x.cpu().numpy() != 0))).cuda()
                same = bool((fn().to(torch.int32) == route().to(torch.int32)).all().item())
                line += f" equal to the host route: {same} |"
            fn()
            reps = max(1, int(a.seconds * 1e3 / max(dev_window(fn, 1, lib)[0], 1e-3)))
            hreps = max(1, int(a.seconds * 1e3 / max(wall_window(route, 1), 1e-3))) if host else 0
            td, th, mhz = [], [], []
            for _ in range(a.repeats):
                ms, clk = dev_window(fn, reps, lib)
                td.append(ms)
                mhz.append(clk)
                if host:
                    th.append(wall_window(route, hreps))
            line += f" device {statistics.median(td):.4f} ({min(td):.4f}-{max(td):.4f}) ms at {statistics.median(mhz):.0f} MHz"
            if host:
                line += f" | host {statistics.median(th):.2f} ({min(th):.2f}-{max(th):.2f}) ms | host / device x{statistics.median(th) / statistics.median(td):.0f}"
            print(line, flush=True)


if __name__ == "__main__":
    main()
