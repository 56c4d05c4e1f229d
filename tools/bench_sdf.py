"""Time of ustrun.functional.signed_distance_map (csrc/distmap.hip) against the reference's host route for the same labels in the
same process: D2H copy of the resident label batch, compute_sdf's two scipy.ndimage.distance_transform_edt calls and its
normalisation per image (utils/util.py:219-239), H2D copy of the float32 map.

Inputs are blob masks (a few discs, 5-30 % foreground), not noise: the row pass searches as far as the distance it finds, so
its time depends on the size of the objects.  One more case is the search's worst plane, 1024 x 1024 with a single background
pixel.  Timing as tools/bench_losses.py: windows of at least --seconds each, the two routes alternating over --repeats windows,
median (min-max) per call; the device route is timed with device events, the host route, which waits for the device by its
nature, with the wall clock around it.  Without scipy the device times are recorded alone, and the output says so.

    python tools/bench_sdf.py [--repeats 7] [--seconds 0.25]
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ust-run_amd"))

import numpy as np  # noqa: E402


def discs(rng, H, W, n, rmin, rmax):
    yy, xx = np.mgrid[:H, :W]
    p = np.zeros((H, W), bool)
    for _ in range(n):
        cy, cx = rng.integers(H // 5, 4 * H // 5), rng.integers(W // 5, 4 * W // 5)
        r = rng.integers(int(rmin * min(H, W)), int(rmax * min(H, W)) + 1)
        p |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return p


def cases():
    rng = np.random.default_rng(25)
    out = []
    for N, S in ((32, 256), (32, 512)):
        m = np.stack([discs(rng, S, S, 2, 0.08, 0.2) for _ in range(N)])[:, None].astype(np.float32)
        out.append((f"[{N},1,{S},{S}] planes", m, False, None))
    lab = np.zeros((16, 288, 288), np.int64)
    for n in range(16):                                   # nested structures, as cardiac labels are: 1 outside 2 outside 3
        big = discs(rng, 288, 288, 1, 0.2, 0.3)
        cy, cx = np.argwhere(big).mean(axis=0)
        yy, xx = np.mgrid[:288, :288]
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        r2 = big.sum() / np.pi
        lab[n][big] = 1
        lab[n][d2 <= 0.5 * r2] = 2
        lab[n][d2 <= 0.2 * r2] = 3
    out.append(("[16,288,288] class map, 3 classes", lab, True, 3))
    worst = np.ones((1, 1, 1024, 1024), np.float32)
    worst[0, 0, 0, 0] = 0
    out.append(("[1,1,1024,1024] one background pixel (worst search)", worst, False, None))
    return out


def host_route(edt, dev_mask, by_class, K):
    """the reference's way for labels that live on the device -> float32 map on the device"""
    import torch
    m = dev_mask.cpu().numpy()
    planes = np.stack([m == c + 1 for c in range(K)], axis=1) if by_class else m != 0
    out = np.zeros(planes.shape, np.float64)
    for n in range(planes.shape[0]):
        for k in range(planes.shape[1]):
            pos = planes[n, k]
            if pos.any() and not pos.all():
                inside, outside = edt(pos), edt(~pos)
                sdf = outside / outside.max() - inside / inside.max()
                sdf[inside == 1] = 0
                out[n, k] = sdf
    return torch.from_numpy(out.astype(np.float32)).cuda()


def dev_window(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


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
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.25, help="least length of a timed window")
    a = ap.parse_args()
    import torch
    from ustrun import functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_sdf: no HIP device; nothing is measured on a CPU")
    try:
        from scipy.ndimage import distance_transform_edt as edt
    except ImportError:
        edt = None
    print(f"device {torch.cuda.get_device_name(0)}, {a.repeats} windows of >= {a.seconds} s each, median (min-max) ms per call; "
          + ("host route: D2H + scipy per image + H2D, wall clock" if edt else "scipy is absent: device times alone"), flush=True)
    for name, m, by_class, K in cases():
        x = torch.from_numpy(m).cuda()
        planes = np.stack([m == c + 1 for c in range(K)], axis=1) if by_class else m != 0
        frac = planes.reshape(-1, planes.shape[-2] * planes.shape[-1]).mean(axis=1)
        routes = [("device", lambda: F.signed_distance_map(x, by_class, K), dev_window),
                  ("s2 only", lambda: F.signed_dist2(x, by_class, K), dev_window)]
        if edt:
            routes.append(("host", lambda: host_route(edt, x, by_class, K), wall_window))
            got, ref = F.signed_distance_map(x, by_class, K)[0], host_route(edt, x, by_class, K)
            print(f"{name}: max |device - host route| {float((got - ref).abs().max()):.3g}", flush=True)
        reps, times = {}, {k: [] for k, _, _ in routes}
        for k, fn, win in routes:
            fn()
            reps[k] = max(1, int(a.seconds * 1e3 / max(win(fn, 1), 1e-3)))
        for _ in range(a.repeats):
            for k, fn, win in routes:
                times[k].append(win(fn, reps[k]))
        line = f"{name}: foreground {100 * frac.min():.1f}-{100 * frac.max():.1f} % of a plane"
        for k, _, _ in routes:
            t = times[k]
            line += f" | {k} {statistics.median(t):.4f} ({min(t):.4f}-{max(t):.4f}) ms"
        if edt:
            line += f" | host / device x{statistics.median(times['host']) / statistics.median(times['device']):.0f}"
        print(line, flush=True)


if __name__ == "__main__":
    main()
