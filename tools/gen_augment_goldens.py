#!/usr/bin/env python3
"""Writes tests/golden/g16_augment_*.npz: one reference transform per record, on small noise images, with the transform's
random draws pinned and recorded (tests/test_gpu_augment.py, tests/test_datasets_host.py).

Runs only where the reference tree is on disk:

    python tools/gen_augment_goldens.py /path/to/reference

It imports the reference's dataloaders/custom_transforms.py in place and calls its transform classes; `torchvision.transforms`
and `cv2`, which that module imports and this environment may lack, are replaced by throw-away stubs: Compose, and
the minimal ToTensor / ToPILImage GaussianBlur needs (/ 255 to float CHW, mul(255).byte() back).  Draws are pinned by giving the
module a scripted stand-in for `random`; elastic_transform's unseeded RandomState(None) is replaced by a seeded one.  The files
hold data only: inputs, parameters, outputs and the exclusion masks (float64: image pixels whose source position lies within
1e-3 px of the edge where the fill value begins, label pixels whose source coordinate lies within 1e-3 of a nearest-neighbour
rounding boundary; at most 0.5 % of a case, asserted here).
"""
import math
import os
import random
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
EPS, CAP = 1e-3, 0.005


def install_stubs():
    import torch
    from PIL import Image

    class Compose:
        def __init__(self, ts):
            self.transforms = ts

        def __call__(self, x):
            for t in self.transforms:
                x = t(x)
            return x

    class ToTensor:
        def __call__(self, pic):
            a = np.array(pic)
            if a.ndim == 2:
                a = a[:, :, None]
            return torch.from_numpy(a.transpose(2, 0, 1).copy()).float().div(255)

    class ToPILImage:
        def __call__(self, t):
            a = t.mul(255).byte().numpy()
            if a.ndim == 3:
                a = a.transpose(1, 2, 0)
            return Image.fromarray(a)

    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tvt.Compose, tvt.ToTensor, tvt.ToPILImage = Compose, ToTensor, ToPILImage
    tv.transforms = tvt
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tvt)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))


class Script:
    """Stands in for the `random` module inside custom_transforms: hands out queued values, or draws from a seeded
    random.Random, and logs every call as (kind, value): 0 random(), 1 uniform(a, b), 2 randint(a, b)."""

    def __init__(self, queue=None, seed=None):
        self.q = list(queue or [])
        self.rng = random.Random(seed) if seed is not None else None
        self.log = []

    def _next(self):
        return self.q.pop(0)

    def random(self):
        v = self.rng.random() if self.rng else float(self._next())
        self.log.append((0, v))
        return v

    def uniform(self, a, b):
        v = self.rng.uniform(a, b) if self.rng else a + (b - a) * float(self._next())
        self.log.append((1, v))
        return v

    def randint(self, a, b):
        v = self.rng.randint(a, b) if self.rng else int(self._next())
        assert a <= v <= b, (a, v, b)
        self.log.append((2, v))
        return v


DATASETS = {   # patch, image channels, label values, label channels, (min_v, max_v), fillcolor: train.py:404-436, train_mnms.py:397-404
    "fundus": (256, 3, (0, 128, 255), 1, (0.5, 1.5), 255),
    "prostate": (384, 1, (0, 255), 1, (0.1, 2.0), 255),
    "BUSI": (256, 1, (0, 255), 1, (0.1, 2.0), 0),
    "MNMS": (288, 1, (0, 255), 3, (0.1, 2.0), 0),
}


def noise_image(rs, n, c):
    return rs.randint(0, 256, (n, n, c) if c == 3 else (n, n)).astype(np.uint8)


def noise_label(rs, n, values, cl):
    return np.asarray(values, np.uint8)[rs.randint(0, len(values), (n, n, cl) if cl == 3 else (n, n))]


def pil(a):
    from PIL import Image
    return Image.fromarray(a)


def arr(x):
    return np.array(x).astype(np.uint8)


def capped(mask, what):
    frac = float(mask.mean()) if mask.size else 0.0
    assert frac <= CAP, f"{what}: exclusion mask covers {frac:.4%} > {CAP:.1%}: pick another angle / offset"
    return mask.astype(np.uint8)


def near_int(v):
    return np.abs(v - np.round(v)) < EPS


def rotate_matrix(deg, W, H):
    """The affine matrix PIL's Image.rotate hands to its transform (no expand, centre of the image)."""
    a = -math.radians(deg % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2] + cx
    m[5] = m[3] * -cx + m[4] * -cy + m[5] + cy
    return m


def main():
    ref = sys.argv[1]
    sys.path.insert(0, ref)
    install_stubs()
    warnings.simplefilter("ignore")
    from dataloaders import custom_transforms as tr
    from scipy.ndimage import gaussian_filter
    real_random, real_RandomState, real_uniform = tr.random, np.random.RandomState, np.random.uniform
    rs = np.random.RandomState(16)
    stages, chain, big = {}, {}, {}

    # shared inputs: (64, 3 channels, fundus label values) and (40, 1 channel, MNMS three-channel label)
    inputs = {"a": (64, 3, (0, 128, 255), 1), "b": (40, 1, (0, 255), 3)}
    for k, (n, c, vals, cl) in inputs.items():
        stages[f"in_{k}_img"] = noise_image(rs, n, c)
        stages[f"in_{k}_lab"] = noise_label(rs, n, vals, cl)
    small = {"a": (noise_image(rs, 52, 3), noise_label(rs, 52, (0, 128, 255), 1)),       # sources smaller than the patch
             "b": (noise_image(rs, 33, 1), noise_label(rs, 33, (0, 255), 3))}
    for k in small:
        stages[f"in_{k}_small_img"], stages[f"in_{k}_small_lab"] = small[k]

    def sample(img, lab):
        return {"image": pil(img), "label": pil(lab), "img_name": "x", "dc": 1}

    # ---- scale-crop: gate off, gate on, padded branch -------------------------------------------------------------------
    def scale_crop_case(name, img, lab, patch, queue):
        s = Script(queue)
        tr.random = s
        out = tr.RandomScaleCrop(patch)(sample(img, lab))
        tr.random = real_random
        assert not s.q
        Hs, Ws = img.shape[:2]
        on = s.log[0][1] > 0.5
        w, h = (int(s.log[1][1] * Ws), int(s.log[2][1] * Hs)) if on else (Ws, Hs)
        pad = max((patch - w) // 2 + 5, (patch - h) // 2 + 5) if (w < patch or h < patch) else 0
        ints = [v for k, v in s.log if k == 2]
        x1, y1 = ints if ints else (0, 0)
        oi, ol = arr(out["image"]), arr(out["label"])
        assert oi.shape[:2] == (patch, patch)
        # no exclusions: the resize has no fill edge, and its nearest source index is PIL's running sum of in / out in double,
        # which is reproducible to the bit -- at an odd w the centre column's coordinate IS an integer, so a 1e-3 band around
        # the rounding boundaries could never stay under the cap at these sizes
        stages[f"sc_{name}_params"] = np.array([int(on), w, h, pad, x1, y1, patch], np.int64)
        stages[f"sc_{name}_img"], stages[f"sc_{name}_lab"] = oi, ol

    for k, (n, c, vals, cl) in inputs.items():
        img, lab = stages[f"in_{k}_img"], stages[f"in_{k}_lab"]
        scale_crop_case(f"{k}_off", img, lab, n, [0.3])
        u1, u2 = (0.37, 0.81) if k == "a" else (0.93, 0.12)
        w, h = int((1 + 0.5 * u1) * n), int((1 + 0.5 * u2) * n)
        scale_crop_case(f"{k}_on", img, lab, n, [0.8, u1, u2, (w - n) // 2 + 1, (h - n) // 3])
        simg, slab = small[k]
        m = simg.shape[0]
        pad = (n - m) // 2 + 5
        scale_crop_case(f"{k}_pad", simg, slab, n, [0.2, 3, 2 * pad + m - n - 1])

    # ---- rotate (+ flip) ------------------------------------------------------------------------------------------------
    def rotate_case(name, img, lab, deg, flip, fillcolor):
        s = Script([0.9, deg] if deg is not None else [0.1])
        tr.random = s
        mid = tr.RandomScaleRotate(fillcolor=fillcolor)(sample(img, lab))
        s.q = [0.2 if flip else 0.7]
        out = tr.RandomHorizontalFlip()(mid)
        tr.random = real_random
        H, W = img.shape[:2]
        oi, ol = arr(out["image"]), arr(out["label"])
        xi = np.zeros((H, W), bool)
        xl = np.zeros((H, W), bool)
        d = deg or 0
        if d % 360:
            m = rotate_matrix(d, W, H)
            yy, xx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
            xin, yin = m[0] * xx + m[1] * yy + m[2], m[3] * xx + m[4] * yy + m[5]
            xi = (np.abs(xin) < EPS) | (np.abs(xin - W) < EPS) | (np.abs(yin) < EPS) | (np.abs(yin - H) < EPS)
            # (the label has no exclusions: PIL's nearest rotation walks 16.16 fixed-point integers, reproducible to the bit,
            # and at 1 degree a 1e-3 band around its rounding boundaries covers more than the cap at these sizes)
            if flip:
                xi = xi[:, ::-1]
        stages[f"rot_{name}_params"] = np.array([d, int(flip), fillcolor], np.int64)
        stages[f"rot_{name}_img"], stages[f"rot_{name}_lab"] = oi, ol
        stages[f"rot_{name}_ximg"] = capped(xi, f"rot_{name} image")
        stages[f"rot_{name}_xlab"] = capped(xl, f"rot_{name} label")

    for k, fc in (("a", 255), ("b", 0)):
        img, lab = stages[f"in_{k}_img"], stages[f"in_{k}_lab"]
        for deg, flip in ((None, False), (None, True), (0, False), (1, False), (-1, True), (20, True), (-20, False), (7, False)):
            rotate_case(f"{k}_{'off' if deg is None else deg}_{int(flip)}", img, lab, deg, flip, fc)
    rotate_case("b_fill255_13", stages["in_b_img"], stages["in_b_lab"], 13, False, 255)      # integer colour on a 3-channel label

    # ---- elastic ----------------------------------------------------------------------------------------------------------
    def elastic_case(store, name, img, lab, on, seed):
        s = Script([0.9 if on else 0.1])
        tr.random = s
        np.random.RandomState = lambda _=None: real_RandomState(seed)
        out = tr.elastic_transform()(sample(img, lab))
        tr.random, np.random.RandomState = real_random, real_RandomState
        H, W = img.shape[:2]
        assert H == W
        oi, ol = arr(out["image"]), arr(out["label"])
        store[f"el_{name}_on"] = np.array([int(on)], np.int64)
        store[f"el_{name}_img"], store[f"el_{name}_lab"] = oi, ol
        if not on:
            return
        r = real_RandomState(seed)
        n0, n1 = r.rand(W, H) * 2 - 1, r.rand(W, H) * 2 - 1
        sigma, alpha = H * 0.08, H * 2
        f0 = gaussian_filter(n0, sigma, mode="constant", cval=0) * alpha
        f1 = gaussian_filter(n1, sigma, mode="constant", cval=0) * alpha
        ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        rr, cc = ii + f0, jj + f1
        xi = (np.abs(rr) < EPS) | (np.abs(rr - (H - 1)) < EPS) | (np.abs(cc) < EPS) | (np.abs(cc - (W - 1)) < EPS)
        xl = near_int(np.clip(rr, 0, H - 1) + 0.5) | near_int(np.clip(cc, 0, W - 1) + 0.5)
        store[f"el_{name}_noise"] = np.stack([n0, n1]).astype(np.float32)
        store[f"el_{name}_field"] = np.stack([f0, f1])
        store[f"el_{name}_ximg"] = capped(xi, f"el_{name} image")
        store[f"el_{name}_xlab"] = capped(xl, f"el_{name} label")

    for k in inputs:
        elastic_case(stages, f"{k}_off", stages[f"in_{k}_img"], stages[f"in_{k}_lab"], False, 0)
        elastic_case(stages, f"{k}_on", stages[f"in_{k}_img"], stages[f"in_{k}_lab"], True, 21 if k == "a" else 22)

    # ---- strong: brightness, contrast, blur -------------------------------------------------------------------------------
    def blur_of(img, sigma):
        c = 3 if img.ndim == 3 else 1
        np.random.uniform = lambda a, b: sigma
        out = tr.GaussianBlur(kernel_size=int(0.1 * img.shape[0] * 4), num_channels=c)(pil(img))     # r = 12 at 64, 8 at 40
        np.random.uniform = real_uniform
        return arr(out)

    for k, (n, c, vals, cl) in inputs.items():
        img = stages[f"in_{k}_img"]
        lo, hi = (0.5, 1.5) if k == "a" else (0.1, 2.0)
        for v in (lo, 1.0, hi):
            tr.random = Script([(v - lo) / (hi - lo)])
            stages[f"br_{k}_{v}"] = arr(tr.Brightness(lo, hi)(pil(img)))
            stages[f"br_{k}_{v}_v"] = np.array([tr.random.log[0][1] * (hi - lo) + lo])
            tr.random = Script([(v - lo) / (hi - lo)])
            stages[f"co_{k}_{v}"] = arr(tr.Contrast(lo, hi)(pil(img)))
            tr.random = real_random
        for sg in (0.1, 1.0, 2.0):
            stages[f"bl_{k}_{sg}"] = blur_of(img, sg)
    stages["blur_r"] = np.array([int(0.1 * 64 * 4) // 2, int(0.1 * 40 * 4) // 2], np.int64)

    # ---- one chain per dataset, every gate on: each stage's input and output ----------------------------------------------
    for di, (ds, (patch, c, vals, cl, (lo, hi), fc)) in enumerate(DATASETS.items()):
        n = 64 if di % 2 == 0 else 40
        img, lab = noise_image(rs, n, c), noise_label(rs, n, vals, cl)
        u1, u2, deg = 0.2 + 0.15 * di, 0.9 - 0.2 * di, (-11, 17, 5, -3)[di]
        w, h = int((1 + 0.5 * u1) * n), int((1 + 0.5 * u2) * n)
        s = Script([0.9, u1, u2, (w - n) // 2, (h - n) // 2 + 1, 0.8, deg, 0.1, 0.95, 0.25, 0.8])
        tr.random = s
        np.random.RandomState = lambda _=None: real_RandomState(100 + di)
        sg = 0.7 + 0.3 * di
        np.random.uniform = lambda a, b: sg
        x = sample(img, lab)
        chain[f"{ds}_s0_img"], chain[f"{ds}_s0_lab"] = img, lab
        ts = [tr.RandomScaleCrop(n), tr.RandomScaleRotate(fillcolor=fc), tr.RandomHorizontalFlip(), tr.elastic_transform()]
        for i, t in enumerate(ts):
            x = t(x)
            chain[f"{ds}_s{i + 1}_img"], chain[f"{ds}_s{i + 1}_lab"] = arr(x["image"]), arr(x["label"])
        weak = x["image"]
        r_blur = int(0.1 * n * 3) // 2
        y = weak
        for i, t in enumerate([tr.Brightness(lo, hi), tr.Contrast(lo, hi), tr.GaussianBlur(int(0.1 * n * 3), c)]):
            y = t(y)
            chain[f"{ds}_t{i + 1}_img"] = arr(y)
        tr.random, np.random.RandomState, np.random.uniform = real_random, real_RandomState, real_uniform
        assert not s.q
        r = real_RandomState(100 + di)
        n0, n1 = r.rand(n, n) * 2 - 1, r.rand(n, n) * 2 - 1
        f = np.stack([gaussian_filter(n0, n * 0.08, mode="constant", cval=0), gaussian_filter(n1, n * 0.08, mode="constant", cval=0)]) * (2 * n)
        ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        rr, cc = ii + f[0], jj + f[1]
        m = rotate_matrix(deg, n, n)
        yy, xx = np.meshgrid(np.arange(n) + 0.5, np.arange(n) + 0.5, indexing="ij")
        xin, yin = m[0] * xx + m[1] * yy + m[2], m[3] * xx + m[4] * yy + m[5]
        x1, y1 = (w - n) // 2, (h - n) // 2 + 1
        chain[f"{ds}_params"] = np.array([n, w, h, x1, y1, deg, 1, fc, r_blur], np.int64)
        chain[f"{ds}_strong"] = np.array([lo + (hi - lo) * 0.25, lo + (hi - lo) * 0.8, sg])
        chain[f"{ds}_field"] = f.astype(np.float32)             # (what the device's warp reads)
        chain[f"{ds}_x3_img"] = capped(((np.abs(xin) < EPS) | (np.abs(xin - n) < EPS) | (np.abs(yin) < EPS) | (np.abs(yin - n) < EPS))[:, ::-1], ds + " rot")
        chain[f"{ds}_x4_img"] = capped((np.abs(rr) < EPS) | (np.abs(rr - (n - 1)) < EPS) | (np.abs(cc) < EPS) | (np.abs(cc - (n - 1)) < EPS), ds + " warp")
        chain[f"{ds}_x4_lab"] = capped(near_int(np.clip(rr, 0, n - 1) + 0.5) | near_int(np.clip(cc, 0, n - 1) + 0.5), ds + " warp label")

    # ---- real extent: field smoothing at H = 256 (sigma 20.48), blur at r = 19 (H = 384); seeds + 4096 sampled values ----------
    r = real_RandomState(256)
    n0 = (r.rand(256, 256) * 2 - 1).astype(np.float32)            # the device reads f32 noise: smooth exactly that
    f0 = gaussian_filter(n0.astype(np.float64), 256 * 0.08, mode="constant", cval=0) * 512
    pick = real_RandomState(7).choice(256 * 256, 4096, replace=False)
    big["field_seed"], big["field_idx"], big["field_val"] = np.array([256]), pick.astype(np.int64), f0.reshape(-1)[pick]
    big["field_l2"] = np.array([np.sqrt((f0 ** 2).sum())])
    im = real_RandomState(384).randint(0, 256, (384, 384)).astype(np.uint8)
    np.random.uniform = lambda a, b: 1.3
    bl = arr(tr.GaussianBlur(kernel_size=int(0.1 * 384), num_channels=1)(pil(im)))
    np.random.uniform = real_uniform
    pick = real_RandomState(8).choice(384 * 384, 4096, replace=False)
    big["blur_seed"], big["blur_sigma"], big["blur_idx"], big["blur_val"] = np.array([384]), np.array([1.3]), pick.astype(np.int64), bl.reshape(-1)[pick]

    # ---- the draws of a seeded single-worker run: weak on labelled samples, weak + strong on unlabelled ones -----------------
    for ds, seed in (("fundus", 5), ("BUSI", 6)):
        patch, c, vals, cl, (lo, hi), fc = DATASETS[ds]
        n = 40
        s = Script(seed=seed)
        tr.random = s
        np.random.seed(seed)
        weak = sys.modules["torchvision.transforms"].Compose([tr.RandomScaleCrop(n), tr.RandomScaleRotate(fillcolor=fc),
                                                              tr.RandomHorizontalFlip(), tr.elastic_transform()])
        strong = sys.modules["torchvision.transforms"].Compose([tr.Brightness(lo, hi), tr.Contrast(lo, hi), tr.GaussianBlur(int(0.1 * n), c)])
        sig = []
        for step in range(3):
            for i in range(2):                                    # labelled batch
                weak(sample(noise_image(rs, n, c), noise_label(rs, n, vals, cl)))
            for i in range(2):                                    # unlabelled batch
                x = weak(sample(noise_image(rs, n, c), noise_label(rs, n, vals, cl)))
                st = np.random.get_state()
                strong(x["image"])
                np.random.set_state(st)
                sig.append(np.random.uniform(0.1, 2.0))           # the value GaussianBlur drew (its only numpy draw)
        tr.random = real_random
        big[f"sampler_trace_{ds}_kind"] = np.array([k for k, _ in s.log], np.int64)
        big[f"sampler_trace_{ds}_val"] = np.array([v for _, v in s.log], np.float64)
        big[f"sampler_trace_{ds}_sigma"] = np.array(sig, np.float64)
        big[f"sampler_trace_{ds}_cfg"] = np.array([seed, n, 2, 2, 3], np.int64)      # seed, patch, label_bs, unlabel_bs, steps

    ins = {k: v for k, v in stages.items() if k.startswith("in_")}
    geo = {k: v for k, v in stages.items() if k.startswith("sc_")}
    rot = {k: v for k, v in stages.items() if k.startswith("rot_")}
    ela = {k: v for k, v in stages.items() if k.startswith("el_")}
    tone = {k: v for k, v in stages.items() if k.startswith(("br_", "co_", "bl_", "blur_r"))}
    assert len(ins) + len(geo) + len(rot) + len(ela) + len(tone) == len(stages)
    total = 0
    for name, d in (("crop", {**ins, **geo}), ("rotate", {**ins, **rot}), ("elastic", {**ins, **ela}), ("tone", {**ins, **tone}),
                    ("chain", chain), ("big", big)):
        path = os.path.join(OUT, f"g16_augment_{name}.npz")
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        assert size < 300 * 1024, (path, size)
        total += size
        print(path, size, len(d))
    assert total < 1024 * 1024, total


if __name__ == "__main__":
    main()
