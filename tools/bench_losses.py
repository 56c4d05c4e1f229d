"""Forward + backward time of the fused consistency / entropy / focal losses of utils/losses.py against the same expressions
composed from torch's own ROCm operators (what a user would otherwise write: softmax / log_softmax / kl_div / log, and the
focal expression of tests/losses_ref.py evaluated on the device), on the same device in the same process.

Per shape [N,K,H,W] and loss: the student's logits require a gradient, the teacher's do not (the Mean-Teacher form); the map
valued softmax_mse_loss is driven by a resident upstream map (`out.backward(gm)`), the scalars by backward().  Timing: device
events around `--reps` back-to-back iterations after a warm-up of each, the two implementations alternating over `--repeats`
windows; the median and the spread (min-max) of the per-iteration time are printed, then

    algorithmic bytes / time      the bytes the loss has to move (every operand read once per direction, every result written once)
    ... / 6.3 TB/s                that figure against the copy rate of MI355X_MICROARCH.md

with T the bytes of one [N,K,H,W] f32 tensor: softmax_mse_loss 7 T (forward a, b -> map; backward a, b, upstream map -> da),
softmax_kl_loss 5 T (a, b; a, b -> da), entropy_minmization 3 T (p; p -> dp), FocalLoss 3 T + 16 bytes per pixel (the int64 target).

    python tools/bench_losses.py [--repeats 7] [--shapes 16,2,256,256 64,4,512,512]
"""
import argparse
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ust-run_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

COPY_RATE = 6.3e12
SHAPES = ["16,2,256,256", "16,4,288,288", "16,2,512,512", "64,4,512,512"]


def window(fn, reps):
    """ms per iteration of `reps` back-to-back calls, device events"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.25, help="least length of a timed window")
    ap.add_argument("--shapes", nargs="*", default=SHAPES)
    a = ap.parse_args()
    import warnings

    import torch
    import torch.nn.functional as F
    import losses_ref as R
    from utils import losses
    warnings.filterwarnings("ignore", message="reduction: 'mean' divides")
    if not torch.cuda.is_available():
        raise SystemExit("bench_losses: no HIP device; nothing is measured on a CPU")
    print(f"device {torch.cuda.get_device_name(0)}, forward + backward, teacher detached, {a.repeats} windows of >= {a.seconds} s each, "
          f"median (min-max) ms per iteration", flush=True)
    focal_fused = losses.FocalLoss()
    for shape in a.shapes:
        N, K, H, W = (int(v) for v in shape.split(","))
        g = torch.Generator(device="cuda").manual_seed(N * K + H)
        x = (3 * torch.randn(N, K, H, W, device="cuda", generator=g)).requires_grad_(True)
        t = 3 * torch.randn(N, K, H, W, device="cuda", generator=g)
        gm = torch.randn(N, K, H, W, device="cuda", generator=g)
        p = torch.softmax(t, dim=1).requires_grad_(True)
        idx = torch.randint(0, K, (N, H, W), device="cuda", generator=g)
        T, npix = 4.0 * N * K * H * W, N * H * W

        def run(leaf, make, upstream=None):
            def go():
                leaf.grad = None
                out = make()
                out.backward(upstream) if upstream is not None else out.backward()
            return go

        cases = [
            ("softmax_mse_loss", 7 * T, run(x, lambda: losses.softmax_mse_loss(x, t), gm), run(x, lambda: (F.softmax(x, dim=1) - F.softmax(t, dim=1)) ** 2, gm)),
            ("softmax_kl_loss", 5 * T, run(x, lambda: losses.softmax_kl_loss(x, t)), run(x, lambda: F.kl_div(F.log_softmax(x, dim=1), F.softmax(t, dim=1), reduction="mean"))),
            ("entropy_minmization", 3 * T, run(p, lambda: losses.entropy_minmization(p)), run(p, lambda: (-(p * torch.log(p + 1e-6)).sum(dim=1)).mean())),
            ("FocalLoss", 3 * T + 16.0 * npix, run(x, lambda: focal_fused(x, idx)), run(x, lambda: R.focal_loss(x, idx))),
        ]
        for name, nbytes, fused, composed in cases:
            times = {"fused": [], "composed": []}
            reps = {}
            for k, fn in (("fused", fused), ("composed", composed)):
                for _ in range(3):
                    fn()
                reps[k] = max(5, int(a.seconds * 1e3 / max(window(fn, 5), 1e-3)))
            for _ in range(a.repeats):
                for k, fn in (("fused", fused), ("composed", composed)):
                    times[k].append(window(fn, reps[k]))
            f, c = statistics.median(times["fused"]), statistics.median(times["composed"])
            rate = nbytes / (f * 1e-3)
            print(f"[{shape}] {name:20s} fused {f:8.4f} ({min(times['fused']):.4f}-{max(times['fused']):.4f}) ms   "
                  f"composed {c:8.4f} ({min(times['composed']):.4f}-{max(times['composed']):.4f}) ms   x{c / f:5.2f}   "
                  f"{nbytes / 1e6:8.1f} MB algorithmic, {rate / 1e12:5.2f} TB/s = {100 * rate / COPY_RATE:4.1f}% of the copy rate", flush=True)
        del x, t, gm, p, idx
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
