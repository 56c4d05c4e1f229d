"""Cost of `--save_img` in the validation path (ustrun.evaluate.validate(save_dir=...)), fundus 256x256 and prostate 384x384 on
the synthetic loaders, test_bs 16.

Per workload:
  * validation images/s without and with `save_dir` (host clock around runs that end in a device synchronise; the two alternate,
    the median and the spread over --repeats are printed); `--parent_module ustrun.NAME` times a second copy of the validation
    module (the parent commit's, placed beside evaluate.py for the run) in the same alternation,
  * the with-`save_dir` time of one coalesced batch of 64 split into its three parts: the render kernels (range + overlay,
    device events over back-to-back calls), the device-to-host copy of the uint8 [64,H,W,3] block (host clock, synchronised),
    the PNG encoding and file writes (host clock), for both picture modes, at PIL's default compress_level and at the one
    ustrun.render uses, one after the other and through ustrun.render.PngWriter's threads.

    python tools/bench_render.py [--dtype bf16] [--batches 16] [--repeats 5] [--parent_module ustrun.evaluate_parent]
"""
import argparse
import importlib
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ust-run_amd"))


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batches", type=int, default=16, help="loader batches of 16 per run")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--coalesce", type=int, default=64)
    ap.add_argument("--parent_module", default="", help="a second validation module to time beside ustrun.evaluate")
    a = ap.parse_args()
    import torch
    from networks.unet_model import UNet
    from ustrun import render, synthetic
    from ustrun.evaluate import PARTS, predict, validate
    from ustrun.trainer import DATASETS, decode_labels
    parent = importlib.import_module(a.parent_module).validate if a.parent_module else None
    print(f"device {torch.cuda.get_device_name(0)}, dtype {a.dtype}, coalesce {a.coalesce}, test_bs 16, {a.batches} batches/run, "
          f"compress_level {render.PNG_COMPRESS_LEVEL}", flush=True)
    for dataset in ("fundus", "prostate"):
        C, H, K = DATASETS[dataset][:3]
        torch.manual_seed(0)
        model = UNet(n_channels=C, n_classes=K, dtype=a.dtype).cuda()
        x0 = synthetic.test_loaders(dataset, 1, 1, 16, C, H, 3)[0][0][0].cuda()
        model.eval()
        with torch.no_grad():           # random weights predict all or nothing: centre the head on one batch's logits
            model.outc.conv.bias -= model(x0).float().transpose(0, 1).flatten(1).median(dim=1).values
        model.train()
        loaders = [[(x.cuda(), y.cuda()) for x, y in dom] for dom in synthetic.test_loaders(dataset, 1, a.batches, 16, C, H, 3)]
        n = 16 * a.batches
        with tempfile.TemporaryDirectory() as tmp:
            runs = {"without save_dir": lambda: validate(dataset, model, loaders, log=None, coalesce=a.coalesce),
                    "with save_dir (mask)": lambda: validate(dataset, model, loaders, log=None, coalesce=a.coalesce, save_dir=tmp),
                    "with save_dir (contour)": lambda: validate(dataset, model, loaders, log=None, coalesce=a.coalesce, save_dir=tmp,
                                                                save_mode="contour")}
            if parent:
                runs["parent commit's validate"] = lambda: parent(dataset, model, loaders, log=None, coalesce=a.coalesce)
            for fn in runs.values():
                timed(fn)
            t = {k: [] for k in runs}
            for _ in range(a.repeats):
                for k, fn in runs.items():
                    t[k].append(timed(fn))
            for k, v in t.items():
                r = sorted(n / s for s in v)
                print(f"{dataset} {H}x{H} validate {k:26s}: {statistics.median(r):8.1f} images/s ({r[0]:.1f}-{r[-1]:.1f}), "
                      f"{statistics.median(v) / n * 1e3:.3f} ms per image", flush=True)
            # the three parts on one coalesced batch of 64
            x, y = zip(*synthetic.test_loaders(dataset, 1, 4, 16, C, H, 3)[0])
            image = torch.cat(x).cuda()
            model.eval()
            with torch.no_grad():
                pred = predict(dataset, model(image))
            model.train()
            mask = decode_labels(dataset, torch.cat(y).cuda())
            parts = len(PARTS[dataset])
            for mode, call in (("mask", lambda: render.render_mask(image, pred, parts=parts)),
                               ("contour", lambda: render.render_contour(image, pred, mask, parts=parts))):
                for _ in range(10):
                    call()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                reps = 100
                torch.cuda.synchronize()
                e0.record()
                for _ in range(reps):
                    call()
                e1.record()
                torch.cuda.synchronize()
                k_ms = e0.elapsed_time(e1) / reps
                rgb = call()
                c_ms = statistics.median(timed(lambda: rgb.cpu()) for _ in range(9)) * 1e3
                host = rgb.cpu().numpy()
                enc = {}
                keep = render.PNG_COMPRESS_LEVEL
                for lvl in (6, keep):
                    render.PNG_COMPRESS_LEVEL = lvl
                    t0 = time.perf_counter()
                    for j in range(len(host)):
                        render.save_png(host[j], os.path.join(tmp, "b_%d.png" % j))
                    enc[lvl] = (time.perf_counter() - t0) * 1e3
                    size = sum(os.path.getsize(os.path.join(tmp, "b_%d.png" % j)) for j in range(len(host))) / len(host)
                    enc[lvl] = (enc[lvl], size)
                render.PNG_COMPRESS_LEVEL = keep
                t0 = time.perf_counter()
                w = render.PngWriter()
                for j in range(len(host)):
                    w.save(host[j], os.path.join(tmp, "b_%d.png" % j))
                threads = w.threads
                w.close()
                thr_ms = (time.perf_counter() - t0) * 1e3
                print(f"{dataset} {H}x{H} {mode:7s} 64 images: render kernels {k_ms:.3f} ms, device->host copy {c_ms:.3f} ms "
                      f"({host.nbytes / 2 ** 20:.1f} MiB), PNG encode + write level 6: {enc[6][0]:.1f} ms ({enc[6][1] / 1024:.0f} KiB/file), "
                      f"level {keep}: {enc[keep][0]:.1f} ms ({enc[keep][1] / 1024:.0f} KiB/file), level {keep} on {threads} threads (PngWriter, what validate uses): "
                      f"{thr_ms:.1f} ms", flush=True)


if __name__ == "__main__":
    main()
