"""Time of the volume kernels (csrc/edt3d.hip) against the host route for the same labels in the same process:
  sdf      ustrun.functional.signed_distance_map_3d  against  D2H + compute_sdf's two scipy.ndimage.distance_transform_edt calls and
           its normalisation per volume (utils/util.py:219-239) + H2D of the float32 map
  metrics  utils.metrics.volume_metrics (device records, host finish)  against  D2H + medpy's hd / hd95 / asd / assd restated
           with scipy (binary_erosion and distance_transform_edt with sampling=voxelspacing, two of each per part)

Inputs are nested ellipsoids (3-33 % foreground per volume), not noise: both searches run as far as the distance they find.  Shapes:
[4,1,32,256,256], [2,1,16,384,384] and a 3-class map [4,10,288,288].  Method (as tools/bench_sdf.py): every route of every shape is
warmed, then windows of at least --seconds each, the routes alternating over --repeats windows, median (min-max) per call; the device
sdf route is timed with device events, the routes that wait for the device by their nature with the wall clock.

Algorithmic bytes per pass are computed from the shapes here (the least each pass must move; the two searches read more, by as
much as the distances they find).  Per-pass kernel TIMES come from a run of their own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_volumes.py --loop 20

    python tools/bench_volumes.py [--repeats 7] [--seconds 0.25] [--no-host]
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ust-run_amd"))

import numpy as np  # noqa: E402

SPACING = (10.0, 1.25, 1.25)


def nested(rng, D, H, W, K, anis):
    """a class map [D,H,W] of K nested ellipsoids, class 1 outermost; `anis` squeezes them along z as thick slices do"""
    zz, yy, xx = np.mgrid[:D, :H, :W]
    cz, cy, cx = D / 2 + rng.uniform(-1, 1), H / 2 + rng.uniform(-H / 8, H / 8), W / 2 + rng.uniform(-W / 8, W / 8)
    r = rng.uniform(0.25, 0.35) * min(H, W)
    d2 = (anis * (zz - cz)) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2
    lab = np.zeros((D, H, W), np.int64)
    for c in range(K):
        lab[d2 <= (r * (1 - c / (K + 0.5))) ** 2] = c + 1
    return lab


def cases():
    rng = np.random.default_rng(28)
    out = []
    for N, D, S in ((4, 32, 256), (2, 16, 384)):
        m = np.stack([nested(rng, D, S, S, 1, S / (2.5 * D)) for _ in range(N)])[:, None].astype(np.float32)
        out.append((f"[{N},1,{D},{S},{S}] volumes", m, False, 1))
    lab = np.stack([nested(rng, 10, 288, 288, 3, 8.0) for _ in range(4)])
    out.append(("[4,10,288,288] class map, 3 classes", lab, True, 3))
    return out


def shifted(m):
    """a prediction for the ground truth m: the same labels moved by (1, 5, 3) voxels"""
    return np.roll(m, (1, 5, 3), axis=(-3, -2, -1))


def volumes(m, by_class, K):
    return np.stack([m == c + 1 for c in range(K)], axis=1) if by_class else m != 0


def host_sdf(ndi, dev_mask, by_class, K):
    import torch
    vol = volumes(dev_mask.cpu().numpy(), by_class, K)
    out = np.zeros(vol.shape, np.float64)
    for n in range(vol.shape[0]):
        for k in range(vol.shape[1]):
            pos = vol[n, k]
            if pos.any() and not pos.all():
                inside, outside = ndi.distance_transform_edt(pos), ndi.distance_transform_edt(~pos)
                sdf = outside / outside.max() - inside / inside.max()
                sdf[inside == 1] = 0
                out[n, k] = sdf
    return torch.from_numpy(out.astype(np.float32)).cuda()


def host_metrics(ndi, dev_pred, dev_gt, by_class, K):
    P, G = volumes(dev_pred.cpu().numpy(), by_class, K), volumes(dev_gt.cpu().numpy(), by_class, K)
    fp = ndi.generate_binary_structure(3, 1)
    out = {k: np.zeros(P.shape[:2]) for k in ("hd", "hd95", "asd", "assd")}
    for n in range(P.shape[0]):
        for k in range(P.shape[1]):
            pb, gb = P[n, k] ^ ndi.binary_erosion(P[n, k], fp), G[n, k] ^ ndi.binary_erosion(G[n, k], fp)
            a = ndi.distance_transform_edt(~gb, sampling=SPACING)[pb]
            b = ndi.distance_transform_edt(~pb, sampling=SPACING)[gb]
            out["hd"][n, k], out["hd95"][n, k] = max(a.max(), b.max()), np.percentile(np.hstack((a, b)), 95)
            out["asd"][n, k], out["assd"][n, k] = a.mean(), (a.mean() + b.mean()) / 2
    return out


def pass_bytes(N, K, D, H, W, mask_bytes_per_voxel):
    """the least bytes each launch moves, per call"""
    v = N * K * D * H * W
    sdf = [("seed", mask_bytes_per_voxel * v + 4 * v), ("column scan", 16 * v), ("row pass", 4 * v + 4 * v),
           ("z pass", 4 * v + 4 * v), ("maxima", 4 * v), ("normalise", 4 * v + 4 * v)]
    met = [("border", 2 * mask_bytes_per_voxel * v + 4 * v), ("column scan", 16 * v), ("row pass", 4 * v + 8 * v), ("z pass", 8 * v),
           ("select", 0)]
    return sdf, met


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
    ap.add_argument("--no-host", action="store_true", help="device routes alone")
    ap.add_argument("--loop", type=int, default=0, help="only call the device routes this many times per shape (for a profiler run)")
    a = ap.parse_args()
    import torch
    from ustrun import functional as F
    from utils import metrics
    if not torch.cuda.is_available():
        raise SystemExit("bench_volumes: no HIP device; nothing is measured on a CPU")
    try:
        from scipy import ndimage as ndi
    except ImportError:
        ndi = None
    if a.no_host or a.loop:
        ndi = None
    print(f"device {torch.cuda.get_device_name(0)}, {a.repeats} windows of >= {a.seconds} s each, median (min-max) ms per call; "
          + ("host routes: D2H + scipy per volume (+ H2D), wall clock" if ndi else "device routes alone"), flush=True)
    for name, m, by_class, K in cases():
        gt, pred = torch.from_numpy(m).cuda(), torch.from_numpy(shifted(m)).cuda()
        vol = volumes(m, by_class, K)
        N, D, H, W = vol.shape[0], vol.shape[2], vol.shape[3], vol.shape[4]
        frac = vol.reshape(N * K, -1).mean(axis=1)
        nc = dict(by_class=by_class, n_classes=K)
        routes = [("sdf device", lambda: F.signed_distance_map_3d(gt, by_class, K if by_class else None), dev_window),
                  ("s2 only", lambda: F.signed_dist2_3d(gt, by_class, K if by_class else None), dev_window),
                  ("records device", lambda: F.surface_metrics_3d(pred, gt, weights=(8, 1, 1), **nc), dev_window),
                  ("metrics device", lambda: metrics.volume_metrics(pred, gt, voxelspacing=SPACING, **nc), wall_window)]
        if a.loop:
            for _, fn, _ in routes:
                for _ in range(a.loop):
                    fn()
            torch.cuda.synchronize()
            continue
        if ndi:
            routes += [("sdf host", lambda: host_sdf(ndi, gt, by_class, K), wall_window),
                       ("metrics host", lambda: host_metrics(ndi, pred, gt, by_class, K), wall_window)]
            got, ref = F.signed_distance_map_3d(gt, by_class, K if by_class else None)[0], host_sdf(ndi, gt, by_class, K)
            gm, hm = metrics.volume_metrics(pred, gt, voxelspacing=SPACING, **nc), host_metrics(ndi, pred, gt, by_class, K)
            print(f"{name}: max |sdf device - host| {float((got - ref).abs().max()):.3g}; max relative metric difference "
                  f"{max(float(np.abs(gm[k] / hm[k] - 1).max()) for k in hm):.3g}", flush=True)
        reps, times = {}, {k: [] for k, _, _ in routes}
        for k, fn, win in routes:                          # every route of every shape is warmed before it is timed
            fn()
            reps[k] = max(1, int(a.seconds * 1e3 / max(win(fn, 1), 1e-3)))
        for _ in range(a.repeats):
            for k, fn, win in routes:
                times[k].append(win(fn, reps[k]))
        print(f"{name}: foreground {100 * frac.min():.1f}-{100 * frac.max():.1f} % of a volume", flush=True)
        med = {k: statistics.median(t) for k, t in times.items()}
        for k, _, _ in routes:
            print(f"    {k:15s} {med[k]:10.4f} ({min(times[k]):.4f}-{max(times[k]):.4f}) ms, {reps[k]} calls per window", flush=True)
        if ndi:
            print(f"    host / device: sdf x{med['sdf host'] / med['sdf device']:.0f}, metrics x{med['metrics host'] / med['metrics device']:.0f}",
                  flush=True)
        sdf_b, met_b = pass_bytes(N, K, D, H, W, 8.0 if by_class else 4.0)     # every volume of a class map reads the int64 map
        for label, rows, t in (("sdf", sdf_b, med["sdf device"]), ("records", met_b, med["records device"])):
            total = sum(b for _, b in rows)
            print(f"    {label}: least bytes per pass " + ", ".join(f"{n} {b / 1e6:.1f} MB" for n, b in rows)
                  + f"; total {total / 1e6:.1f} MB in {t:.4f} ms = {total / t / 1e9:.3f} TB/s", flush=True)


if __name__ == "__main__":
    main()
