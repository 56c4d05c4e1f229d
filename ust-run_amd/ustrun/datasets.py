"""Training on image folders: the reference's four dataset layouts read once into resident uint8 pools, and its per-sample
PIL / scipy augmentation (dataloaders/dataloader.py, dataloaders/custom_transforms.py) done per batch on the device by the
ustrun_aug_* kernels (csrc/augment.hip).

Host side, once:  the file listing, the `selected_idxs` rule, the image -> mask path rule, the mode conversions and the one
resize per file of each reader, exactly as the reference's Dataset classes do them (PIL is imported here, lazily, and nowhere
else).  Per step: AugmentSampler draws every sample's parameters from its own random.Random / numpy RandomState in the call order
of the reference's transforms, ResidentLoader uploads that one int32 block and launches the stages.  Pixels never return to
the host."""
from __future__ import annotations

import glob as _glob
import math
import os
import random
import struct

import numpy as np
import torch

from . import _lib

# name: (reader kind, sub-directory of --data_root, domain names, patch, image channels, label channels, (min_v, max_v),
#        fillcolor, image resample)   train.py:404-436,464-471,966-971, train_mnms.py:397-404,882, dataloader.py
SPECS = {
    "fundus": dict(sub="Fundus", domains={1: "Domain1", 2: "Domain2", 3: "Domain3", 4: "Domain4"}, patch=256, C=3, Cl=1,
                   v=(0.5, 1.5), fill=255, values=(0, 128, 255)),
    "prostate": dict(sub="ProstateSlice", domains={1: "BIDMC", 2: "BMC", 3: "HK", 4: "I2CVB", 5: "RUNMC", 6: "UCL"}, patch=384, C=1,
                     Cl=1, v=(0.1, 2.0), fill=255, values=(0, 255)),
    "BUSI": dict(sub="Dataset_BUSI_with_GT", domains={1: "benign", 2: "malignant"}, patch=256, C=1, Cl=1, v=(0.1, 2.0), fill=0,
                 values=(0, 255)),
    "MNMS": dict(sub="mnms", domains={1: "vendorA", 2: "vendorB", 3: "vendorC", 4: "vendorD"}, patch=288, C=1, Cl=3, v=(0.1, 2.0),
                 fill=0, values=(0, 255)),
}
DOMAIN_LEN = {"fundus": [50, 99, 320, 320], "prostate": [225, 305, 136, 373, 338, 133], "BUSI": [350, 168],
              "MNMS": [1030, 1342, 525, 550]}       # train.py:466-471, train_mnms.py:436


def _pil():
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("reading image folders (--synthetic 0) needs Pillow, which is not installed; "
                           "run with --synthetic 1 for the seeded synthetic batches") from e
    return Image


# ---------------------------------------------------------------------------------------------------------------- listing
def _keep_selected(items, domain, splitid, selected_idxs):
    """dataloader.py:67-75: only the domain equal to splitid is thinned, to the indices in selected_idxs."""
    if splitid == domain and selected_idxs is not None:
        sel = set(selected_idxs)
        return [it for i, it in enumerate(items) if i in sel]
    return list(items)


def list_files(dataset, base_dir, phase, domains, splitid=-1, selected_idxs=None):
    """-> [(image path, [mask paths], domain code, name)] in the reference's order."""
    spec = SPECS[dataset]
    out = []
    for i in domains:
        dn = spec["domains"][i]
        if dataset == "fundus":                             # dataloader.py:55-83
            image_dir = os.path.join(base_dir, "Domain" + str(i), phase, "ROIs/image/")
            if phase == "train":
                with open(os.path.join(base_dir, f"Domain{i}_train.txt")) as f:
                    files = [line.strip() for line in f]
            else:
                files = sorted(_glob.glob(image_dir + "*.png"))
            items = [(p, [p.replace("image", "mask")], i, p.split("/")[-1]) for p in files]
        elif dataset in ("prostate", "MNMS"):               # :189-210, :293-314
            files = sorted(_glob.glob(os.path.join(base_dir, dn, phase, "image/") + "*.png"))
            items = [(p, [p.replace("image", "mask")], i, dn + "_" + p.split("/")[-1]) for p in files]
        else:                                               # BUSI :377-410: masks follow their image in the sorted listing
            groups = []
            for p in sorted(_glob.glob(os.path.join(base_dir, dn + "/") + "*.png")):
                if "mask" not in p:
                    groups.append([p])
                else:
                    groups[-1].append(p)
            n_test = int(len(groups) * 0.2)
            if phase == "test":
                groups = groups[-n_test:]
            elif phase == "train":
                groups = groups[:len(groups) - n_test]
            else:
                raise ValueError("Unknown split...")
            items = [(g[0], g[1:], i, dn + "_" + g[0].split("/")[-1]) for g in groups]
        out += _keep_selected(items, i, splitid, selected_idxs)
    return out


# ---------------------------------------------------------------------------------------------------------------- decoding
def _label_image(im):
    """The reference converts an RGB mask to L and leaves every other mode as it is (dataloader.py:99-100; its `mode is 'RGB'`
    is read as the equality it means); a mode numpy would not give bytes for is converted too."""
    if im.mode == "RGB" or im.mode not in ("L", "P"):
        im = im.convert("L")
    return im


def decode(dataset, item, patch, resolve=None):
    """One file pair -> (image uint8 [patch, patch(, 3)], label uint8 [patch, patch(, 3)]): dataloader.py:97-101 (fundus),
    :224-231 (prostate), :328-332 (MNMS), :418-433 (BUSI).  One resize per file: the image with the reader's filter, the mask
    with NEAREST."""
    Image = _pil()
    path, masks, _, _ = item
    opn = (lambda p: Image.open(resolve(p))) if resolve else Image.open
    size = (patch, patch)
    if dataset == "fundus":
        img = opn(path).convert("RGB").resize(size, Image.LANCZOS)
        lab = _label_image(opn(masks[0])).resize(size, Image.NEAREST)
    elif dataset == "prostate":                             # stored at patch size: the reference resizes nothing here; a file
        img, lab = opn(path), opn(masks[0])                 # of another size is brought to the patch the same way as the others
        if img.mode != "L":
            img = img.convert("L")
        lab = _label_image(lab)
        if img.size != size:
            img = img.resize(size, Image.LANCZOS)
        if lab.size != size:
            lab = lab.resize(size, Image.NEAREST)
    elif dataset == "MNMS":                                 # (this reader's image filter is BILINEAR)
        img = opn(path).resize(size, Image.BILINEAR)
        if img.mode != "L":
            img = img.convert("L")
        lab = opn(masks[0]).resize(size, Image.NEAREST)
        if lab.mode != "RGB":
            lab = lab.convert("RGB")
    else:
        img = opn(path).convert("L").resize(size, Image.LANCZOS)
        if len(masks) == 1:
            lab = opn(masks[0]).convert("L").resize(size, Image.NEAREST)
        else:
            comb = None
            for m in masks:
                a = np.array(opn(m).convert("L"))
                comb = a if comb is None else np.maximum(comb, a)
            lab = Image.fromarray(comb).convert("L").resize(size, Image.NEAREST)
    return np.asarray(img, dtype=np.uint8), np.asarray(lab, dtype=np.uint8)


class ResidentDataset:
    """images uint8 [n, H, W, C], labels uint8 [n, H, W, Cl], dc int32 [n] on `device`, names on the host."""

    def __init__(self, dataset, base_dir, phase="train", splitid=-1, domain=(1,), selected_idxs=None, patch=None, device="cuda"):
        spec = SPECS[dataset]
        self.dataset, self.phase = dataset, phase
        self.patch = patch or spec["patch"]
        self.items = list_files(dataset, base_dir, phase, list(domain), splitid, selected_idxs)
        if not self.items:
            raise RuntimeError(f"{dataset}: no {phase} images of domain(s) {list(domain)} under {base_dir}")

        def resolve(p):                                      # a list file's entry may be relative to the data directory
            return p if os.path.isabs(p) or os.path.exists(p) else os.path.join(base_dir, p)
        P, C, Cl = self.patch, spec["C"], spec["Cl"]
        imgs = np.empty((len(self.items), P, P, C), np.uint8)
        labs = np.empty((len(self.items), P, P, Cl), np.uint8)
        for n, it in enumerate(self.items):
            a, b = decode(dataset, it, P, resolve)
            imgs[n], labs[n] = a.reshape(P, P, C), b.reshape(P, P, Cl)
        self.images = torch.from_numpy(imgs).to(device)
        self.labels = torch.from_numpy(labs).to(device)
        self.dc = torch.tensor([it[2] for it in self.items], dtype=torch.int32, device=device)
        self.names = [it[3] for it in self.items]

    def __len__(self):
        return len(self.items)


# ------------------------------------------------------------------------------------------------------- parameter sampling
ROW = 40                                  # int32 words per sample
SC, ROT, EL, ST = 0, 8, 32, 33            # scale-crop {gate, w, h, pad, x1, y1, fill, 0}; rotate {gate, flip, fill, 0, 6 fixed, 6 doubles};
                                          # elastic {gate}; strong {gate, brightness, contrast, sigma}


def _f32_bits(v):
    return struct.unpack("<i", struct.pack("<f", v))[0]


def _fix16(v):
    v = v * 65536.0 + 0.5
    return int(math.floor(v)) if v < 0.0 else int(v)


def rotate_words(deg, W, H):
    """The affine matrix of PIL's Image.rotate(deg) (centre of the image, no expand) as the 18 words ustrun_aug_rotate reads:
    the 16.16 fixed-point coefficients of its nearest-neighbour walk, then the six doubles of its bilinear path."""
    a = -math.radians(deg % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2] + cx
    m[5] = m[3] * -cx + m[4] * -cy + m[5] + cy
    fixed = [_fix16(m[0]), _fix16(m[1]), _fix16(m[2] + m[0] * 0.5 + m[1] * 0.5),
             _fix16(m[3]), _fix16(m[4]), _fix16(m[5] + m[3] * 0.5 + m[4] * 0.5)]
    return fixed + list(struct.unpack("<12i", struct.pack("<6d", *m)))


def scale_crop_words(on, w, h, x1, y1, patch, fill):
    pad = max((patch - w) // 2 + 5, (patch - h) // 2 + 5) if (w < patch or h < patch) else 0      # custom_transforms.py:323-324
    return [int(on), w, h, pad, x1, y1, 255, 0]            # (RandomCrop pads the mask with 255 whatever the rotation's fillcolor)


class AugmentSampler:
    """Per-sample draws in the reference's call order: RandomScaleCrop (custom_transforms.py:542-550 with RandomCrop :322-338),
    RandomScaleRotate (:518-520), RandomHorizontalFlip (:391), elastic_transform (:212), then for a strong view Brightness
    (:66), Contrast (:75) and GaussianBlur's sigma (:103, from numpy).  `trace`, when a list, receives every draw as
    (kind, value): 0 random(), 1 uniform, 2 randint, 3 numpy uniform."""

    def __init__(self, dataset, patch, seed, trace=None):
        spec = SPECS[dataset]
        self.patch, self.v, self.fill = patch, spec["v"], spec["fill"]
        self.rng, self.np_rng, self.trace = random.Random(seed), np.random.RandomState(seed % (2 ** 32)), trace

    def _log(self, kind, v):
        if self.trace is not None:
            self.trace.append((kind, v))
        return v

    def _random(self):
        return self._log(0, self.rng.random())

    def _uniform(self, a, b):
        return self._log(1, self.rng.uniform(a, b))

    def _randint(self, a, b):
        return self._log(2, self.rng.randint(a, b))

    def weak(self, row, Hs, Ws):
        P = self.patch
        on = self._random() > 0.5
        w, h = (int(self._uniform(1, 1.5) * Ws), int(self._uniform(1, 1.5) * Hs)) if on else (Ws, Hs)
        words = scale_crop_words(on, w, h, 0, 0, P, self.fill)
        pw, ph = w + 2 * words[3], h + 2 * words[3]
        if not (pw == P and ph == P):
            words[4], words[5] = self._randint(0, pw - P), self._randint(0, ph - P)
        row[SC:SC + 8] = words
        deg = self._randint(-20, 20) if self._random() > 0.5 else 0
        flip = self._random() < 0.5
        row[ROT:ROT + 4] = [int(deg % 360 != 0), int(flip), self.fill, 0]
        if deg % 360:
            row[ROT + 4:ROT + 22] = rotate_words(deg, P, P)
        row[EL] = int(self._random() > 0.5)

    def strong(self, row):
        lo, hi = self.v
        vb = lo + float(hi - lo) * self._random()
        vc = lo + float(hi - lo) * self._random()
        sg = self._log(3, float(self.np_rng.uniform(0.1, 2.0)))
        row[ST:ST + 4] = [3, _f32_bits(vb), _f32_bits(vc), _f32_bits(sg)]

    def batch(self, n_lb, n_ulb, Hs=None, Ws=None):
        """-> int32 [n_lb + n_ulb, ROW]: the labelled samples (weak only), then the unlabelled ones (weak, then strong)."""
        Hs, Ws = Hs or self.patch, Ws or self.patch
        rows = np.zeros((n_lb + n_ulb, ROW), np.int64)
        for b in range(n_lb + n_ulb):
            self.weak(rows[b], Hs, Ws)
            if b >= n_lb:
                self.strong(rows[b])
        return rows.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ device stages
def _s():
    return torch.cuda.current_stream().cuda_stream


def _geom(img, lab):
    B, H, W, C = img.shape
    return B, H, W, C, lab.shape[3]


def stage_gather(images, labels, idx):
    B = idx.numel()
    img = torch.empty((B,) + tuple(images.shape[1:]), dtype=torch.uint8, device=images.device)
    lab = torch.empty((B,) + tuple(labels.shape[1:]), dtype=torch.uint8, device=images.device)
    _lib.check(_lib.lib().ustrun_aug_gather(images.data_ptr(), labels.data_ptr(), idx.data_ptr(), images.shape[0], B,
                                            images[0].numel(), labels[0].numel(), img.data_ptr(), lab.data_ptr(), _s()), "aug_gather")
    return img, lab


def stage_scale_crop(img, lab, params, patch):
    B, H, W, C, Cl = _geom(img, lab)
    oi = torch.empty((B, patch, patch, C), dtype=torch.uint8, device=img.device)
    ol = torch.empty((B, patch, patch, Cl), dtype=torch.uint8, device=img.device)
    _lib.check(_lib.lib().ustrun_aug_scale_crop(img.data_ptr(), lab.data_ptr(), params[:, SC:].data_ptr(), params.stride(0), B, H, W, C, Cl,
                                                patch, oi.data_ptr(), ol.data_ptr(), _s()), "aug_scale_crop")
    return oi, ol


def stage_rotate(img, lab, params):
    B, H, W, C, Cl = _geom(img, lab)
    oi, ol = torch.empty_like(img), torch.empty_like(lab)
    _lib.check(_lib.lib().ustrun_aug_rotate(img.data_ptr(), lab.data_ptr(), params[:, ROT:].data_ptr(), params.stride(0), B, H, W, C, Cl,
                                            oi.data_ptr(), ol.data_ptr(), _s()), "aug_rotate")
    return oi, ol


def stage_elastic_field(params, B, H, W, seed, noise=None, device=None):
    device = device or params.device
    field = torch.empty((B, 2, H, W), dtype=torch.float32, device=device)
    work = torch.empty_like(field)
    _lib.check(_lib.lib().ustrun_aug_elastic_field(None if noise is None else noise.data_ptr(), int(seed), params[:, EL:].data_ptr(),
                                                   params.stride(0), B, H, W, field.data_ptr(), work.data_ptr(), _s()), "aug_elastic_field")
    return field


def elastic_noise(B, H, W, seed, device="cuda"):
    """The generator's values on their own (tests): [B, 2, H, W]."""
    noise = torch.empty((B, 2, H, W), dtype=torch.float32, device=device)
    _lib.check(_lib.lib().ustrun_aug_elastic_noise(int(seed), B, H, W, noise.data_ptr(), _s()), "aug_elastic_noise")
    return noise


def stage_elastic_warp(img, lab, field, params):
    B, H, W, C, Cl = _geom(img, lab)
    oi, ol = torch.empty_like(img), torch.empty_like(lab)
    _lib.check(_lib.lib().ustrun_aug_elastic_warp(img.data_ptr(), lab.data_ptr(), field.data_ptr(), params[:, EL:].data_ptr(),
                                                  params.stride(0), B, H, W, C, Cl, oi.data_ptr(), ol.data_ptr(), _s()), "aug_elastic_warp")
    return oi, ol


def blur_radius(patch):
    return int(0.1 * patch) // 2                      # train.py:456 with custom_transforms.py:82


def stage_strong(img, params, r):
    B, H, W, C = img.shape
    out = torch.empty_like(img)
    nbytes = _lib.lib().ustrun_aug_strong_work_bytes(B, H, W, C)
    work = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
    _lib.check(_lib.lib().ustrun_aug_strong(img.data_ptr(), params[:, ST:].data_ptr(), params.stride(0), B, H, W, C, r, out.data_ptr(),
                                            work.data_ptr(), nbytes, _s()), "aug_strong")
    return out


def stage_finish(weak, strong, lab):
    B, H, W, C = weak.shape
    Cl = lab.shape[3]
    xw = torch.empty((B, C, H, W), dtype=torch.float32, device=weak.device)
    xs = torch.empty_like(xw) if strong is not None else None
    y = torch.empty((B, H, W, Cl) if Cl > 1 else (B, H, W), dtype=torch.float32, device=weak.device)
    _lib.check(_lib.lib().ustrun_aug_finish(weak.data_ptr(), None if strong is None else strong.data_ptr(), lab.data_ptr(), B, H, W, C, Cl,
                                            xw.data_ptr(), None if xs is None else xs.data_ptr(), y.data_ptr(), _s()), "aug_finish")
    return xw, xs, y


def weak_augment(img, lab, params, patch, seed, noise=None):
    """The reference's weak Compose (train.py:439-451) on a gathered batch: scale-crop, rotate (+ flip), elastic."""
    img, lab = stage_scale_crop(img, lab, params, patch)
    img, lab = stage_rotate(img, lab, params)
    field = stage_elastic_field(params, img.shape[0], patch, patch, seed, noise)
    return stage_elastic_warp(img, lab, field, params)


# ------------------------------------------------------------------------------------------------------------------- loader
class _Epochs:
    """The index stream of DataLoader(shuffle=True, drop_last=True) under the reference's `cycle` (train.py:95-107): a fresh
    permutation per epoch, batches of bs, the incomplete tail dropped."""

    def __init__(self, n, bs, gen):
        if n < bs:
            raise RuntimeError(f"a pool of {n} images cannot fill a batch of {bs} (drop_last)")
        self.n, self.bs, self.gen, self.perm, self.pos = n, bs, gen, None, 0

    def next(self):
        if self.perm is None or self.pos + self.bs > self.n:
            self.perm, self.pos = torch.randperm(self.n, generator=self.gen), 0
        idx = self.perm[self.pos:self.pos + self.bs]
        self.pos += self.bs
        return idx


class ResidentLoader:
    """Infinite iterator of (lb_x_w, lb_y, ulb_x_w, ulb_x_s, ulb_y) device tensors in the dtypes and value domains of
    synthetic.batch: images f32 NCHW on the grid k / 127.5 - 1, labels f32 holding byte values.  One permutation stream per
    pool; rank r draws from seed + 100003 r, as the synthetic path does."""

    def __init__(self, lb_ds, ulb_ds, label_bs, unlabel_bs, seed=1337, rank=0):
        assert lb_ds.dataset == ulb_ds.dataset and lb_ds.patch == ulb_ds.patch
        self.lb, self.ulb, self.n_lb, self.n_ulb = lb_ds, ulb_ds, label_bs, unlabel_bs
        self.patch = lb_ds.patch
        s = seed + 100003 * rank
        self.seed = s
        self.sampler = AugmentSampler(lb_ds.dataset, self.patch, s)
        self.lb_idx = _Epochs(len(lb_ds), label_bs, torch.Generator().manual_seed(s))
        self.ulb_idx = _Epochs(len(ulb_ds), unlabel_bs, torch.Generator().manual_seed(s + 1))
        self.step = 0
        self.last_idx = None

    def __iter__(self):
        return self

    def __next__(self):
        dev = self.lb.images.device
        li, ui = self.lb_idx.next(), self.ulb_idx.next()
        self.last_idx = (li, ui)
        rows = torch.from_numpy(self.sampler.batch(self.n_lb, self.n_ulb))
        block = torch.cat([rows.reshape(-1), li.to(torch.int32), ui.to(torch.int32)]).to(dev, non_blocking=True)   # the step's one upload
        n = self.n_lb + self.n_ulb
        params = block[:n * ROW].view(n, ROW)
        lidx, uidx = block[n * ROW:n * ROW + self.n_lb], block[n * ROW + self.n_lb:]
        out = []
        for ds, idx, p, strong in ((self.lb, lidx, params[:self.n_lb], False), (self.ulb, uidx, params[self.n_lb:], True)):
            img, lab = stage_gather(ds.images, ds.labels, idx)
            # elastic noise: a counter-based stream keyed by (seed, step, pool)
            img, lab = weak_augment(img, lab, p, self.patch, (self.seed << 20) + 2 * self.step + int(strong))
            s = stage_strong(img, p, blur_radius(self.patch)) if strong else None
            out.append(stage_finish(img, s, lab))
        self.step += 1
        (lx, _, ly), (ux, us, uy) = out
        return lx, ly, ux, us, uy


class _TestDomain:
    """One domain's test pool as a re-iterable of (image f32 NCHW, raw label f32) batches, in file order, no augmentation."""

    def __init__(self, ds, bs):
        self.ds, self.bs = ds, bs

    def __len__(self):
        return (len(self.ds) + self.bs - 1) // self.bs

    def __iter__(self):
        for o in range(0, len(self.ds), self.bs):
            xw, _, y = stage_finish(self.ds.images[o:o + self.bs], None, self.ds.labels[o:o + self.bs])
            yield xw, y


def test_loaders(ds_list, test_bs):
    """The shape synthetic.test_loaders returns: one iterable of (image, raw label) batches per domain (test.py:222-230)."""
    return [_TestDomain(ds, test_bs) for ds in ds_list]


# ------------------------------------------------------------------------------------------------------------------- wiring
def base_dir(args):
    return os.path.join(args.data_root, SPECS[args.dataset]["sub"])


def domain_count(args):
    return min(args.domain_num, len(SPECS[args.dataset]["domains"]))        # train.py:413-414,424-425,435-436


def train_datasets(args, patch, device):
    """The labelled / unlabelled split of the reference's train() (train.py:464-485, train_mnms.py:434-447)."""
    lens = DOMAIN_LEN[args.dataset]
    data_num = lens[args.lb_domain - 1]
    lb_num = int(sum(lens) * args.lb_ratio) if getattr(args, "lb_ratio", 0) > 0 else args.lb_num
    domains = list(range(1, domain_count(args) + 1))
    root = base_dir(args)
    lb = ResidentDataset(args.dataset, root, "train", args.lb_domain, [args.lb_domain], list(range(lb_num)), patch, device)
    ulb = ResidentDataset(args.dataset, root, "train", args.lb_domain, domains, list(range(lb_num, data_num)), patch, device)
    return lb, ulb


def test_datasets(args, patch, device):
    root = base_dir(args)
    return [ResidentDataset(args.dataset, root, "test", -1, [i], None, patch, device) for i in range(1, domain_count(args) + 1)]
