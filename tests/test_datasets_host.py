"""Host side of the image-folder pipeline (ust-run_amd/ustrun/datasets.py), no GPU: the four readers on tiny trees built in
tmp_path (listing order, the selected_idxs rule, image / mask pairing, domain codes, pools byte-identical to direct PIL
calls), AugmentSampler against the draws the reference's transforms made from the same seeds (g16_augment_big:
sampler_trace_*), and ResidentLoader's epoch rule."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from ustrun import datasets as D


def _png(path, a, mode=None, palette=False):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    im = Image.fromarray(a, mode) if mode else Image.fromarray(a)
    if palette:
        im = im.convert("P")
    im.save(path)


def _noise(rs, h, w, c=None):
    return rs.randint(0, 256, (h, w) if c is None else (h, w, c)).astype(np.uint8)


SIZES = [(37, 51), (64, 64), (45, 33), (70, 41), (39, 39), (52, 67), (31, 58), (66, 35)]


def build_tree(kind, root, rs, n=7, domains=(1, 2)):
    """-> {domain: [image paths in the order they were WRITTEN (shuffled names)]}"""
    spec = D.SPECS[kind]
    for d in domains:
        dn = spec["domains"][d]
        names = ["%s%02d.png" % ("gV"[d % 2], (i * 5) % 11) for i in range(n)]          # not written in sorted order
        for phase in ("train", "test"):
            listed = []
            for i, nm in enumerate(names if phase == "train" else names[:3]):
                h, w = SIZES[(i + d) % len(SIZES)]
                if kind == "fundus":
                    ip = os.path.join(root, f"Domain{d}", phase, "ROIs/image", nm)
                    _png(ip, _noise(rs, h, w, 3))
                    m = np.asarray((0, 128, 255), np.uint8)[rs.randint(0, 3, (h, w))]
                    if i == 1:
                        _png(ip.replace("image", "mask"), np.stack([m, m, m], 2))          # an RGB mask
                    elif i == 2:
                        _png(ip.replace("image", "mask"), m, palette=True)                 # a palette mask
                    else:
                        _png(ip.replace("image", "mask"), m)
                    listed.append(ip)
                elif kind in ("prostate", "MNMS"):
                    ip = os.path.join(root, dn, phase, "image", nm)
                    _png(ip, _noise(rs, h, w))
                    m = np.asarray((0, 255), np.uint8)[rs.randint(0, 2, (h, w, 3) if kind == "MNMS" else (h, w))]
                    _png(ip.replace("image", "mask"), m)
                if kind == "BUSI" and phase == "train":
                    ip = os.path.join(root, dn, "%s (%d).png" % (dn, i + 1))
                    _png(ip, _noise(rs, h, w, 3))
                    _png(ip[:-4] + "_mask.png", np.asarray((0, 255), np.uint8)[rs.randint(0, 2, (h, w))])
                    if i == 3:
                        _png(ip[:-4] + "_mask_1.png", np.asarray((0, 255), np.uint8)[rs.randint(0, 2, (h, w))])
            if kind == "fundus" and phase == "train":
                with open(os.path.join(root, f"Domain{d}_train.txt"), "w") as f:
                    f.write("\n".join(reversed(listed)) + "\n")                             # the list file's order rules, not the sort


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    pytest.importorskip("PIL")
    rs = np.random.RandomState(3)
    out = {}
    for kind in D.SPECS:
        root = str(tmp_path_factory.mktemp(kind))
        build_tree(kind, root, rs)
        out[kind] = root
    return out


def test_fundus_listing_follows_the_list_file_and_test_split_is_sorted(trees):
    root = trees["fundus"]
    tr = D.list_files("fundus", root, "train", [1, 2])
    want = [line.strip() for d in (1, 2) for line in open(os.path.join(root, f"Domain{d}_train.txt"))]
    assert [t[0] for t in tr] == want and want[:7] != sorted(want[:7])
    assert [t[2] for t in tr] == [1] * 7 + [2] * 7
    assert all(t[1] == [t[0].replace("image", "mask")] and os.path.exists(t[1][0]) for t in tr)
    assert all(t[3] == os.path.basename(t[0]) for t in tr)
    te = D.list_files("fundus", root, "test", [2])
    assert [t[0] for t in te] == sorted(t[0] for t in te) and len(te) == 3 and "/test/" in te[0][0]


@pytest.mark.parametrize("kind", ["prostate", "MNMS"])
def test_glob_layouts_sort_and_prefix_names(trees, kind):
    items = D.list_files(kind, trees[kind], "train", [1, 2])
    for d in (1, 2):
        sub = [t for t in items if t[2] == d]
        assert len(sub) == 7 and [t[0] for t in sub] == sorted(t[0] for t in sub)
        dn = D.SPECS[kind]["domains"][d]
        assert all(t[3] == dn + "_" + os.path.basename(t[0]) and f"/{dn}/train/image/" in t[0] for t in sub)
        assert all(t[1] == [t[0].replace("image", "mask")] for t in sub)


def test_busi_groups_masks_and_splits_the_tail(trees):
    tr = D.list_files("BUSI", trees["BUSI"], "train", [1, 2])
    te = D.list_files("BUSI", trees["BUSI"], "test", [1])
    assert len([t for t in tr if t[2] == 1]) == 6 and len(te) == 1          # int(7 * 0.2) = 1 from the tail
    allp = sorted(t[0] for t in tr if t[2] == 1) + [te[0][0]]
    assert allp == sorted(allp) and all("mask" not in t[0] for t in tr + te)
    multi = [t for t in tr + te if len(t[1]) == 2]
    assert len(multi) == 2 and all(m[1][0].endswith("_mask.png") and m[1][1].endswith("_mask_1.png") for m in multi)
    assert all(t[3].startswith("benign_benign (") for t in te)


@pytest.mark.parametrize("kind", list(D.SPECS))
def test_selected_idxs_thin_only_the_split_domain(trees, kind):
    full = D.list_files(kind, trees[kind], "train", [1, 2])
    n1 = len([t for t in full if t[2] == 1])
    lb = D.list_files(kind, trees[kind], "train", [1], splitid=1, selected_idxs=[0, 1, 2])
    ulb = D.list_files(kind, trees[kind], "train", [1, 2], splitid=1, selected_idxs=list(range(3, 50)))
    assert [t[0] for t in lb] == [t[0] for t in full[:3]]
    assert [t[0] for t in ulb] == [t[0] for t in full[3:]]                  # domain 1 minus its first three, domain 2 whole
    other = D.list_files(kind, trees[kind], "train", [1, 2], splitid=2, selected_idxs=[0])
    assert [t[0] for t in other] == [t[0] for t in full[:n1 + 1]]
    assert [t[0] for t in D.list_files(kind, trees[kind], "train", [1, 2], splitid=-1, selected_idxs=[0])] == [t[0] for t in full]


def test_pools_are_byte_identical_to_direct_pil_calls(trees):
    from PIL import Image
    P = 48
    ds = D.ResidentDataset("fundus", trees["fundus"], "train", 1, [1, 2], list(range(2, 9)), patch=P, device="cpu")
    assert ds.images.dtype == torch.uint8 and tuple(ds.images.shape) == (len(ds), P, P, 3) and tuple(ds.labels.shape) == (len(ds), P, P, 1)
    assert ds.dc.dtype == torch.int32 and ds.dc.tolist() == [1] * 5 + [2] * 7 and ds.names == [t[3] for t in ds.items]
    modes = set()
    for n, (ip, (mp,), _, _) in enumerate(ds.items):
        a = np.asarray(Image.open(ip).convert("RGB").resize((P, P), Image.LANCZOS))
        m = Image.open(mp)
        modes.add(m.mode)
        if m.mode == "RGB":
            m = m.convert("L")
        b = np.asarray(m.resize((P, P), Image.NEAREST))
        assert np.array_equal(ds.images[n].numpy(), a) and np.array_equal(ds.labels[n, :, :, 0].numpy(), b), ip
    assert {"RGB", "P", "L"} <= modes

    ds = D.ResidentDataset("MNMS", trees["MNMS"], "test", -1, [2], None, patch=P, device="cpu")
    assert tuple(ds.labels.shape) == (3, P, P, 3) and ds.dc.tolist() == [2] * 3
    for n, (ip, (mp,), _, _) in enumerate(ds.items):
        assert np.array_equal(ds.images[n, :, :, 0].numpy(), np.asarray(Image.open(ip).resize((P, P), Image.BILINEAR)))
        assert np.array_equal(ds.labels[n].numpy(), np.asarray(Image.open(mp).resize((P, P), Image.NEAREST)))

    ds = D.ResidentDataset("prostate", trees["prostate"], "train", -1, [1], None, patch=P, device="cpu")
    for n, (ip, (mp,), _, _) in enumerate(ds.items):
        assert np.array_equal(ds.images[n, :, :, 0].numpy(), np.asarray(Image.open(ip).resize((P, P), Image.LANCZOS)))
        assert np.array_equal(ds.labels[n, :, :, 0].numpy(), np.asarray(Image.open(mp).resize((P, P), Image.NEAREST)))

    ds = D.ResidentDataset("BUSI", trees["BUSI"], "train", -1, [1], None, patch=P, device="cpu")
    for n, (ip, ms, _, _) in enumerate(ds.items):
        assert np.array_equal(ds.images[n, :, :, 0].numpy(), np.asarray(Image.open(ip).convert("L").resize((P, P), Image.LANCZOS)))
        comb = np.maximum.reduce([np.asarray(Image.open(m).convert("L")) for m in ms])
        assert np.array_equal(ds.labels[n, :, :, 0].numpy(), np.asarray(Image.fromarray(comb).resize((P, P), Image.NEAREST)))


@pytest.mark.parametrize("ds", ["fundus", "BUSI"])
def test_sampler_draws_what_the_reference_drew(ds):
    g = load_golden("g16_augment_big")
    seed, patch, n_lb, n_ulb, steps = (int(v) for v in g[f"sampler_trace_{ds}_cfg"])
    trace = []
    s = D.AugmentSampler(ds, patch, seed, trace=trace)
    blocks = [s.batch(n_lb, n_ulb) for _ in range(steps)]
    mine = [(k, v) for k, v in trace if k != 3]
    assert [k for k, _ in mine] == g[f"sampler_trace_{ds}_kind"].tolist()
    assert [float(v) for _, v in mine] == g[f"sampler_trace_{ds}_val"].tolist()                    # the same calls: exact
    assert [v for k, v in trace if k == 3] == g[f"sampler_trace_{ds}_sigma"].tolist()
    b = blocks[0]
    assert b.dtype == np.int32 and b.shape == (n_lb + n_ulb, D.ROW)
    assert (b[:n_lb, D.ST] == 0).all() and (b[n_lb:, D.ST] == 3).all()
    on = b[:, D.SC] == 1
    assert ((b[on, D.SC + 1] >= patch) & (b[on, D.SC + 1] <= int(1.5 * patch))).all()
    assert (b[:, D.SC + 4] >= 0).all() and (b[:, D.SC + 4] <= np.where(on, b[:, D.SC + 1], patch) - patch).all()


def test_sampler_ranges_and_rotation_words():
    lo, hi = D.SPECS["prostate"]["v"]
    s = D.AugmentSampler("prostate", 64, 9)
    rows = np.concatenate([s.batch(0, 8) for _ in range(40)])
    f = rows[:, D.ST + 1:D.ST + 4].copy().view(np.float32)
    assert f[:, :2].min() >= lo and f[:, :2].max() <= hi and f[:, 2].min() >= 0.1 and f[:, 2].max() <= 2.0
    assert 0.3 < (rows[:, D.EL] == 1).mean() < 0.7 and 0.3 < (rows[:, D.ROT + 1] == 1).mean() < 0.7
    assert (rows[:, D.ROT + 2] == 255).all() and (D.AugmentSampler("BUSI", 64, 1).batch(4, 0)[:, D.ROT + 2] == 0).all()
    w = D.rotate_words(90, 64, 64)                               # x_in = y, y_in = 64 - x about the centre
    m = np.array(w[6:], np.int32).view(np.float64)
    assert np.allclose(m, [0, -1, 64, 1, 0, 0], atol=1e-12) or np.allclose(m, [0, 1, 0, -1, 0, 64], atol=1e-12)
    assert w[0] == 0 and abs(w[1]) == 65536


class _Pool:
    def __init__(self, n, patch=8):
        self.dataset, self.patch = "BUSI", patch
        self.images = torch.zeros(n, patch, patch, 1, dtype=torch.uint8)
        self.labels = torch.zeros(n, patch, patch, 1, dtype=torch.uint8)

    def __len__(self):
        return self.images.shape[0]


def test_loader_epochs_visit_every_index_once_and_drop_the_tail():
    ld = D.ResidentLoader(_Pool(7), _Pool(11), 2, 3, seed=5, rank=0)
    for stream, n, bs in ((ld.lb_idx, 7, 2), (ld.ulb_idx, 11, 3)):
        for epoch in range(3):
            seen = torch.cat([stream.next() for _ in range(n // bs)]).tolist()
            assert len(seen) == len(set(seen)) == (n // bs) * bs and all(0 <= i < n for i in seen)
    a = D.ResidentLoader(_Pool(64), _Pool(64), 4, 4, seed=5, rank=0)
    b = D.ResidentLoader(_Pool(64), _Pool(64), 4, 4, seed=5, rank=0)
    c = D.ResidentLoader(_Pool(64), _Pool(64), 4, 4, seed=5, rank=1)
    ia, ib, ic = (torch.cat([x.lb_idx.next() for _ in range(4)]).tolist() for x in (a, b, c))
    assert ia == ib and ia != ic and c.seed == 5 + 100003
    assert not np.array_equal(a.sampler.batch(4, 4), c.sampler.batch(4, 4))
    with pytest.raises(RuntimeError, match="cannot fill a batch"):
        D.ResidentLoader(_Pool(3), _Pool(64), 4, 4)


def test_missing_pil_names_the_synthetic_alternative(monkeypatch):
    import builtins
    real = builtins.__import__

    def fake(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("No module named 'PIL'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", fake)
    with pytest.raises(RuntimeError, match="--synthetic 1"):
        D._pil()
