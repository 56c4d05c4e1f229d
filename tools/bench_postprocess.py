"""Cost of the post-processing (ustrun_post_process: holes filled, small components removed) alone and in the validation path.

  * `F.post_process` on 64 coalesced images of a model's own predictions, as planes/s: fundus 256x256 x 2 parts, M&Ms 288x288 x 3,
    BUSI 512x512 x 1 (device events over back-to-back calls, every launch and the work-buffer allocation from torch's cache
    included; the shader clock held meanwhile), with both steps, with the filling alone, with the removal alone and as the plain
    decode;
  * `validate(surface_metrics=True)` with and without `post_process=True` on the same loaders (host clock around runs that end in a
    device synchronise; the two alternate, the median and the spread over --repeats are printed);
  * if scipy imports: the scipy restatement of the reference's function (binary_fill_holes, label with the full 3x3 structure, the
    reference's loop) on the same planes over --procs worker processes;
  * `--loop WORKLOAD`: nothing but 200 calls of `F.post_process` on that workload, for a kernel trace taken in a run of its own
    (rocprofv3 --kernel-trace --stats -- python tools/bench_postprocess.py --loop fundus): the share of each launch.

    python tools/bench_postprocess.py [--dtype bf16] [--batches 16] [--repeats 5] [--procs 16]
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

WORKLOADS = {"fundus": ("fundus", 256), "MNMS": ("MNMS", 288), "BUSI": ("BUSI", 512)}


def scipy_plane(p):
    """the reference's post_processing, skimage's label restated with scipy's (full 3x3 structure)"""
    import scipy.ndimage as nd
    f = nd.binary_fill_holes(p)
    lab, n = nd.label(f, structure=np.ones((3, 3)))
    total = f.sum()
    for c in range(1, n + 1):
        one = lab == c
        if one.sum() / total < 0.2:
            f[one] = 0
    return int(f.sum())


def timed_validate(validate, dataset, model, loaders, post, coalesce):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    validate(dataset, model, loaders, log=None, coalesce=coalesce, surface_metrics=True, post_process=post)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def centred_model(dataset, C, H, K, dtype):
    """random weights predict all or nothing; the head bias centred on one batch's logits gives predictions with geometry"""
    import torch
    from networks.unet_model import UNet
    from ustrun import synthetic
    torch.manual_seed(0)
    model = UNet(n_channels=C, n_classes=K, dtype=dtype).cuda()
    x0 = synthetic.test_loaders(dataset, 1, 1, 8, C, H, 3)[0][0][0].cuda()
    model.eval()
    with torch.no_grad():
        lg = model(x0).float()
        model.outc.conv.bias -= lg.transpose(0, 1).flatten(1).median(dim=1).values
    model.train()
    return model


def predictions(dataset, model, C, H, n=64):
    import torch
    from ustrun import synthetic
    from ustrun.evaluate import predict
    x = torch.cat([b[0] for b in synthetic.test_loaders(dataset, 1, n // 8, 8, C, H, 3)[0]]).cuda()
    model.eval()
    with torch.no_grad():
        pred = torch.cat([predict(dataset, model(x[i:i + 16])) for i in range(0, n, 16)])
    model.train()
    return pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batches", type=int, default=16, help="loader batches of 16 per validate run")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--coalesce", type=int, default=64)
    ap.add_argument("--loop", default="", choices=[""] + list(WORKLOADS))
    a = ap.parse_args()
    import torch
    from clock_probe import clock_mhz, probe
    from ustrun import _lib as L
    from ustrun import functional as F
    from ustrun import synthetic
    from ustrun.evaluate import _part_kw, validate
    from ustrun.trainer import DATASETS
    lib = L.lib()
    try:
        import scipy
        have_scipy = scipy.__version__
    except ImportError:
        have_scipy = None
    print(f"device {torch.cuda.get_device_name(0)}, dtype {a.dtype}, coalesce {a.coalesce}, scipy {have_scipy}", flush=True)
    for name in ([a.loop] if a.loop else WORKLOADS):
        dataset, H = WORKLOADS[name]
        C, _, K = DATASETS[dataset][:3]
        model = centred_model(dataset, C, H, K, a.dtype)
        pred = predictions(dataset, model, C, H)
        kw = _part_kw(dataset)
        if a.loop:
            for _ in range(200):
                F.post_process(pred, **kw)
            torch.cuda.synchronize()
            print(f"{name}: 200 calls done", flush=True)
            return
        out = F.post_process(pred, **kw)
        plain = F.post_process(pred, fill_holes=False, min_share=None, **kw)
        filled = F.post_process(pred, min_share=None, **kw)
        parts, nplanes = out.shape[1], out.shape[0] * out.shape[1]
        print(f"{name} {H}x{H} x {parts} part(s), 64 images: foreground per plane {plain.sum().item() / nplanes:.0f} raw, "
              f"{filled.sum().item() / nplanes:.0f} filled, {out.sum().item() / nplanes:.0f} kept; "
              f"work buffer {lib.ustrun_post_process_work_bytes(64, parts, H, H) / 2 ** 20:.1f} MiB", flush=True)
        for label, opts in (("fill + removal", {}), ("fill only", dict(min_share=None)), ("removal only", dict(fill_holes=False)),
                            ("decode only", dict(fill_holes=False, min_share=None))):
            call = lambda: F.post_process(pred, **kw, **opts)
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
            print(f"{name} {H}x{H}: F.post_process, {label:14s}: {ms:.3f} ms per call of {nplanes} planes ({nplanes / ms * 1e3:.0f} planes/s, "
                  f"{64 / ms * 1e3:.0f} images/s); shader clock {mhz:.0f} MHz ({lo:.0f}-{hi:.0f} over {nx} XCDs)", flush=True)
        loaders = [[(x.cuda(), y.cuda()) for x, y in dom] for dom in synthetic.test_loaders(dataset, 1, a.batches, 16, C, H, 3)]
        for post in (False, True):
            timed_validate(validate, dataset, model, loaders, post, a.coalesce)
        t = {False: [], True: []}
        for _ in range(a.repeats):
            for post in (False, True):
                t[post].append(timed_validate(validate, dataset, model, loaders, post, a.coalesce))
        n = 16 * a.batches
        rate = {k: sorted(n / v for v in t[k]) for k in t}
        med = {k: statistics.median(t[k]) for k in t}
        print(f"{name} {H}x{H} validate(surface_metrics=True), test_bs 16 ({n} images/run, {a.repeats} runs): "
              f"post_process off {statistics.median(rate[False]):8.1f} images/s ({rate[False][0]:.1f}-{rate[False][-1]:.1f}), "
              f"on {statistics.median(rate[True]):8.1f} images/s ({rate[True][0]:.1f}-{rate[True][-1]:.1f}); "
              f"added {(med[True] - med[False]) / n * 1e6:.1f} us per image ({(med[True] / med[False] - 1) * 100:+.1f} %)", flush=True)
        if have_scipy:
            p = plain.cpu().numpy().astype(bool)
            jobs = [p[i, k] for i in range(len(p)) for k in range(parts)]
            with mp.get_context("spawn").Pool(a.procs) as pool:
                pool.map(scipy_plane, jobs[:a.procs])             # the workers import scipy before the clock starts
                t0 = time.perf_counter()
                pool.map(scipy_plane, jobs, chunksize=1)
                dt = time.perf_counter() - t0
            print(f"{name} {H}x{H}: scipy restatement of the reference's post_processing, {a.procs} processes: {len(jobs) / dt:.1f} planes/s "
                  f"({dt / len(jobs) * a.procs * 1e3:.1f} ms per plane per process)", flush=True)
        else:
            print(f"{name}: scipy does not import here: no CPU figure for the reference's method", flush=True)


if __name__ == "__main__":
    main()
