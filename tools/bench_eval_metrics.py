"""Cost of the surface-distance metrics (dc / jc / hd95 / asd) in the validation path, prostate 384x384 and fundus 256x256.

Per workload and test_bs (1 and 16):
  * validation images/s with the metrics off and on (`ustrun.evaluate.validate`, host clock around runs that end in a device
    synchronise; off and on alternate, the median and the spread over --repeats are printed),
  * the time of `ustrun_surface_metrics` alone on a batch of 64 of that run's own predictions and labels (device events over
    back-to-back calls, the four launches and the counter memset together) and the shader clock held meanwhile,
  * if scipy imports: the same (sample, part) planes through the scipy.ndimage restatement of the reference's method
    (tools/gen_surface_goldens.py: two distance transforms and two erosions per hd95, again per asd, as medpy does) over
    --procs worker processes, as images/s.

    python tools/bench_eval_metrics.py [--dtype bf16] [--batches 64] [--repeats 5] [--procs 16]
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


def scipy_sample(args):
    """what the reference runs per (sample, part): binary.hd95 + binary.asd = three surface-distance calls"""
    from gen_surface_goldens import sds
    p, g = args
    if not p.any() or not g.any():
        return 100.0, 100.0
    hd = np.percentile(np.hstack((sds(p, g), sds(g, p))), 95)
    return float(hd), float(sds(p, g).mean())


def timed_validate(validate, dataset, model, loaders, on, coalesce):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    validate(dataset, model, loaders, log=None, coalesce=coalesce, surface_metrics=on)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batches", type=int, default=64, help="loader batches per run at test_bs 16 (x4 at test_bs 1)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--coalesce", type=int, default=64)
    a = ap.parse_args()
    import torch
    from clock_probe import clock_mhz, probe
    from networks.unet_model import UNet
    from ustrun import _lib as L
    from ustrun import functional as F
    from ustrun import synthetic
    from ustrun.evaluate import predict, validate
    from ustrun.trainer import DATASETS, decode_labels
    try:
        import scipy
        have_scipy = scipy.__version__
    except ImportError:
        have_scipy = None
    print(f"device {torch.cuda.get_device_name(0)}, dtype {a.dtype}, coalesce {a.coalesce}, scipy {have_scipy}", flush=True)
    lib = L.lib()
    for dataset in ("prostate", "fundus"):
        C, H, K = DATASETS[dataset][:3]
        torch.manual_seed(0)
        model = UNet(n_channels=C, n_classes=K, dtype=a.dtype).cuda()
        # predictions with real geometry: random weights predict all or nothing; centre the head on one batch's logits
        x0 = synthetic.test_loaders(dataset, 1, 1, 16, C, H, 3)[0][0][0].cuda()
        model.eval()
        with torch.no_grad():
            lg = model(x0).float()
            model.outc.conv.bias -= lg.transpose(0, 1).flatten(1).median(dim=1).values
        model.train()
        for bs in (1, 16):
            nb = a.batches * (4 if bs == 1 else 1)
            loaders = [[(x.cuda(), y.cuda()) for x, y in dom] for dom in synthetic.test_loaders(dataset, 1, nb, bs, C, H, 3)]
            for on in (False, True):                       # warm-up of every shape of the timed window
                timed_validate(validate, dataset, model, loaders, on, a.coalesce)
            t = {False: [], True: []}
            for _ in range(a.repeats):
                for on in (False, True):
                    t[on].append(timed_validate(validate, dataset, model, loaders, on, a.coalesce))
            n = bs * nb
            rate = {on: sorted(n / v for v in t[on]) for on in t}
            print(f"{dataset} {H}x{H} test_bs={bs:2d} ({n} images/run, {a.repeats} runs): "
                  f"metrics off {statistics.median(rate[False]):8.1f} images/s ({rate[False][0]:.1f}-{rate[False][-1]:.1f}), "
                  f"on {statistics.median(rate[True]):8.1f} images/s ({rate[True][0]:.1f}-{rate[True][-1]:.1f})", flush=True)
        # the kernels alone, 64 images of this model's predictions
        x, y = zip(*synthetic.test_loaders(dataset, 1, 4, 16, C, H, 3)[0])
        model.eval()
        with torch.no_grad():
            pred = predict(dataset, model(torch.cat(x).cuda()))
        model.train()
        mask = decode_labels(dataset, torch.cat(y).cuda())
        call = lambda: F.surface_metrics(pred, mask)
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 300
        pa = probe(lib)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        pb = probe(lib)
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        mhz, lo, hi, nx = clock_mhz(pa, pb)
        rec = call().cpu().numpy()
        parts = rec.shape[1]
        wb = lib.ustrun_surface_metrics_work_bytes(64, parts, H, H)
        print(f"{dataset} {H}x{H}: ustrun_surface_metrics on 64 images x {parts} part(s): {ms:.3f} ms per call "
              f"({64 / ms * 1e3:.0f} images/s), work buffer {wb / 2 ** 20:.1f} MiB, border pixels per plane "
              f"{rec[..., 0].mean():.0f} + {rec[..., 1].mean():.0f}; shader clock {mhz:.0f} MHz ({lo:.0f}-{hi:.0f} over {nx} XCDs)",
              flush=True)
        if have_scipy:
            p, g = pred.cpu().numpy(), mask.cpu().numpy()
            if p.ndim == 3:
                p, g = p[:, None], g[:, None]
            jobs = [(p[n, k] != 0, g[n, k] != 0) for n in range(len(p)) for k in range(parts)]
            with mp.get_context("spawn").Pool(a.procs) as pool:
                pool.map(scipy_sample, jobs[:a.procs])            # the workers import scipy before the clock starts
                t0 = time.perf_counter()
                pool.map(scipy_sample, jobs, chunksize=1)
                dt = time.perf_counter() - t0
            print(f"{dataset} {H}x{H}: scipy restatement of the reference's hd95 + asd, {a.procs} processes: {len(p) / dt:.1f} images/s "
                  f"({dt / len(jobs) * a.procs * 1e3:.1f} ms per (sample, part) per process)", flush=True)
        else:
            print(f"{dataset}: scipy does not import here: no CPU figure for the reference's method", flush=True)


if __name__ == "__main__":
    main()
