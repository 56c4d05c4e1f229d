"""Time of the label-map losses and metrics of csrc/labelmap.hip against the same expressions composed from torch's own ROCm
operators (what a user would otherwise write), on the same device in the same process:

    ce_map              forward + backward of the class-weighted cross-entropy with ignore_index, against
                        F.cross_entropy(weight=, ignore_index=, reduction="sum") / (H*W*N)
    confusion + get_iou one confusion matrix per image and the IoU from it (a Python float: the call waits), against the
                        reference's loop of one compare-and-count pair with .item() per class and image, in the form it means
                        (logical and / or)
    Balanced_DiceLoss   forward + backward, against sigmoid and the reference's sums on channels 0 and 1

Timing as tools/bench_losses.py: device events around back-to-back iterations after a warm-up of each, the two implementations
alternating over `--repeats` windows; the median and the spread of the per-iteration time are printed, then the bytes the call has
to move (every operand read once per direction, every result written once) over the time, and that against the 6.3 TB/s copy
rate of MI355X_MICROARCH.md.  With T the bytes of the [N,K,H,W] f32 logits and P = N*H*W pixels:
    ce_map 3 T + 24 P (forward: logits, int64 target -> lse; backward: logits, target, lse -> dlogits)
    confusion 16 P (two int64 maps);  Balanced_DiceLoss 40 P (x, t of two channels read in both directions, their dx written)

    python tools/bench_labelmap.py [--repeats 7] [--shapes 16,21,512,512 16,2,512,512]
"""
import argparse
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ust-run_amd"))

COPY_RATE = 6.3e12
SHAPES = ["16,21,512,512", "16,2,512,512"]


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


def iou_loop(pred, gt, n_classes):
    """the reference's get_iou as it is meant: per image and class one intersection and one union, each fetched with .item()"""
    import torch
    total = 0.0
    for p, g in zip(pred, gt):
        vals = []
        for j in range(n_classes):
            it = torch.sum((p == j) & (g == j)).item()
            un = torch.sum((p == j) | (g == j)).item()
            if un:
                vals.append(it / un)
        total += sum(vals) / len(vals)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.25, help="least length of a timed window")
    ap.add_argument("--shapes", nargs="*", default=SHAPES)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as TF
    import dataloaders.utils as U
    from ustrun import functional as F
    from utils import metrics as M
    if not torch.cuda.is_available():
        raise SystemExit("bench_labelmap: no HIP device; nothing is measured on a CPU")
    print(f"device {torch.cuda.get_device_name(0)}, {a.repeats} windows of >= {a.seconds} s each, median (min-max) ms per iteration", flush=True)
    for shape in a.shapes:
        N, K, H, W = (int(v) for v in shape.split(","))
        g = torch.Generator(device="cuda").manual_seed(N * K + H)
        x = (3 * torch.randn(N, K, H, W, device="cuda", generator=g)).requires_grad_(True)
        t = torch.randint(0, K, (N, H, W), device="cuda", generator=g)
        t[torch.rand(N, H, W, device="cuda", generator=g) < 0.1] = 255
        w = 0.5 + torch.rand(K, device="cuda", generator=g)
        pred = torch.randint(0, K, (N, H, W), device="cuda", generator=g)
        gt = torch.where(torch.rand(N, H, W, device="cuda", generator=g) < 0.7, pred, torch.randint(0, K, (N, H, W), device="cuda", generator=g))
        bt = (torch.rand(N, K, H, W, device="cuda", generator=g) < 0.3).float()
        T, P = 4.0 * N * K * H * W, float(N * H * W)
        scale = 1.0 / (H * W * N)

        def fb(make):
            def go():
                x.grad = None
                make().backward()
            return go

        def composed_balanced():
            s = torch.sigmoid(x)
            d = lambda i, tt: 1 - (2.0 * (i.reshape(-1) * tt.reshape(-1)).sum() + 1.0) / (i.sum() + tt.sum() + 1.0)
            return 0.5 * (d(s[:, 0], bt[:, 0]) + d(s[:, 1], bt[:, 1]))

        assert abs(U.get_iou(pred, gt, K) - iou_loop(pred, gt, K)) < 1e-9
        cases = [
            ("ce_map fwd+bwd", 3 * T + 24 * P, fb(lambda: F.ce_map(x, t, weight=w, ignore_index=255, scale=scale)),
             fb(lambda: TF.cross_entropy(x, t, weight=w, ignore_index=255, reduction="sum") * scale)),
            ("confusion + get_iou", 16 * P, lambda: U.get_iou(pred, gt, K), lambda: iou_loop(pred, gt, K)),
            ("Balanced_DiceLoss fwd+bwd", 40 * P, fb(lambda: M.Balanced_DiceLoss(x, bt)), fb(composed_balanced)),
        ]
        for name, nbytes, fused, composed in cases:
            times = {"fused": [], "composed": []}
            reps = {}
            for k, fn in (("fused", fused), ("composed", composed)):
                for _ in range(3):
                    fn()
                reps[k] = max(3, int(a.seconds * 1e3 / max(window(fn, 3), 1e-3)))
            for _ in range(a.repeats):
                for k, fn in (("fused", fused), ("composed", composed)):
                    times[k].append(window(fn, reps[k]))
            f, c = statistics.median(times["fused"]), statistics.median(times["composed"])
            rate = nbytes / (f * 1e-3)
            print(f"[{shape}] {name:26s} fused {f:8.4f} ({min(times['fused']):.4f}-{max(times['fused']):.4f}) ms   "
                  f"composed {c:8.4f} ({min(times['composed']):.4f}-{max(times['composed']):.4f}) ms   x{c / f:6.2f}   "
                  f"{nbytes / 1e6:8.1f} MB algorithmic, {rate / 1e12:5.2f} TB/s = {100 * rate / COPY_RATE:4.1f}% of the copy rate", flush=True)
        del x, t, w, pred, gt, bt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
