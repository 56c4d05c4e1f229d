#!/usr/bin/env python3
"""Writes tests/golden/g19_losses_rest.npz: inputs, values and gradients of the thirteen functions of the reference's
utils/losses.py beside DiceLossWithMask, from the reference's OWN functions in float32 on the CPU, and the public names of that
file with their `inspect.signature` strings (classes: constructor and forward).

The reference's file is loaded in place by its path (`--reference DIR`, the directory that holds utils/).  `entropy_loss` and
`entropy_loss_map` call .cuda() and are not run: tests/losses_ref.py states them as entropy_minmization / entropy_map over ln C.

Shapes: N = 2, 9 x 13 pixels, K in {2, 4}, logits 3 * randn.  Scalar results are multiplied by losses_ref.UP = 0.7 before backward();
map results are contracted with a random map `gm` / `gm1`.  Keys: `<case>_K<K>_v` the value, `_ga` / `_gb` the gradients of
the first / second argument.  The case table is tests/losses_ref.py's `cases`, which the tests walk too.

    python tools/gen_losses_goldens.py --reference /path/to/reference
"""
import argparse
import importlib.util
import inspect
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import losses_ref as R  # noqa: E402


def inputs(K):
    """the tensors of one class count, float32 (int64 for the class map)"""
    g = torch.Generator().manual_seed(1900 + K)
    z = {"a": 3 * torch.randn(2, K, 9, 13, generator=g), "b": 3 * torch.randn(2, K, 9, 13, generator=g),
         "gm": torch.randn(2, K, 9, 13, generator=g), "gm1": torch.randn(2, 1, 9, 13, generator=g),
         "ra": 3 * torch.randn(7, 5, generator=g), "rb": 3 * torch.randn(7, 5, generator=g)}
    z["p"] = torch.softmax(3 * torch.randn(2, K, 9, 13, generator=g), dim=1)
    z["idx"] = torch.randint(0, K, (2, 1, 9, 13), generator=g)
    z["hot"] = torch.cat([z["idx"] == k for k in range(K)], dim=1).float()
    return z


def load_reference(root):
    path = os.path.join(os.path.abspath(root), "utils", "losses.py")
    spec = importlib.util.spec_from_file_location("reference_utils_losses", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def signatures(mod):
    out = []
    for name, obj in vars(mod).items():
        if name.startswith("_") or getattr(obj, "__module__", None) != mod.__name__:
            continue
        s = str(inspect.signature(obj))
        if inspect.isclass(obj):
            s += " forward" + str(inspect.signature(obj.forward))
        out.append((name, s))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's root directory (holds utils/losses.py)")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    out = {}
    sig = signatures(ref)
    out["names"] = np.array([n for n, _ in sig])
    out["signatures"] = np.array([s for _, s in sig])
    worst = 0.0
    for K in R.KS:
        z = inputs(K)
        for k, t in z.items():
            out["in_%s_K%d" % (k, K)] = t.numpy()
        mine = R.cases(K, R.Names)
        for name, case in R.cases(K, ref).items():
            v, ga, gb = R.evaluate(case, z)
            v64, ga64, gb64 = R.evaluate(mine[name], z, torch.float64)
            key = "%s_K%d" % (name, K)
            out[key + "_v"], out[key + "_ga"] = v.numpy(), ga.numpy()
            errs = [float((v - v64).abs().max() / v64.abs().max()), float((ga - ga64).abs().max() / ga64.abs().max())]
            if gb is not None:
                out[key + "_gb"] = gb.numpy()
                errs.append(float((gb - gb64).abs().max() / gb64.abs().max()))
            worst = max(worst, *errs[1:])
            print("%-28s value %.1e  gradients %s   (reference f32 against the restatement in f64, / max|.|)"
                  % (key, errs[0], " ".join("%.1e" % e for e in errs[1:])))
            assert errs[0] < 2e-5 and max(errs[1:]) < 2e-6, key
    print("worst gradient error / max|g|: %.1e" % worst)
    path = os.path.join(ROOT, "tests", "golden", "g19_losses_rest.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.normpath(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
