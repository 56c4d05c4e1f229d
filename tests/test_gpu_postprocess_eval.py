"""`validate(..., post_process=True)`, `dataloaders.utils.post_processing` and `test.py --post_process 1`: the validation path with
the reference's post_processing (dataloaders/utils.py:193-204) on the device scores and draws exactly what it scores and draws
for predictions that were post-processed on the CPU by tests/postprocess_ref.py and uploaded as planes; switched off it is the
path it was."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import postprocess_ref as R
from test_gpu_surface_metrics import _model

pytestmark = pytest.mark.gpu

FORMS = [("fundus", 3, 2), ("MNMS", 1, 4)]
H = 64


@pytest.fixture(scope="module", params=FORMS, ids=[f[0] for f in FORMS])
def setup(request):
    from ustrun import synthetic
    dataset, c, k = request.param
    out = {}
    for bs in (1, 3):
        out[bs] = synthetic.test_loaders(dataset, 2, 3, bs, c, H, seed=5)
    return dataset, _model(dataset, c, k, out[3], base=16), out


def _cpu_processed(dataset, model, loader_batch):
    """(image, processed prediction planes, ground-truth planes) of one loader batch, the post-processing done on the CPU"""
    from ustrun.evaluate import PARTS, predict
    from ustrun.trainer import decode_labels
    image, label = loader_batch
    image, label = image.cuda(), label.cuda()
    kw = dict(by_class=True, K=3) if dataset == "MNMS" else dict(K=len(PARTS[dataset]))
    with torch.no_grad():
        pred = predict(dataset, model(image)).cpu().numpy()
    P = R.process_batch(pred, **kw)
    G = R.planes(decode_labels(dataset, label).cpu().numpy(), **kw).astype(np.float32)
    return image, torch.from_numpy(P).cuda(), torch.from_numpy(G).cuda(), pred


def _expected(dataset, model, loaders):
    """validate's averaging (per loader batch, per domain, over the domains) over metrics of the CPU-processed planes"""
    from ustrun import functional as F
    from ustrun.evaluate import PARTS
    from utils import metrics
    parts = len(PARTS[dataset])
    names = ("dice", "dc", "jc", "hd", "asd")
    val = {m: [0.0] * parts for m in names}
    per = {m: [] for m in names}
    changed = 0
    model.eval()
    for loader in loaders:
        dom = {m: [0.0] * parts for m in names}
        for batch in loader:
            image, P, G, raw = _cpu_processed(dataset, model, batch)
            changed += int((P.cpu().numpy() != R.planes(raw, dataset == "MNMS", parts)).any())
            c, r = F.dice_counts(P, G).cpu().numpy(), F.surface_metrics(P, G).cpu().numpy()
            cf = c.astype(np.float64)
            vals = (metrics.dice_from_counts(cf[..., 0], cf[..., 1], cf[..., 2]),) + tuple(metrics.surface_from_records(r, c))
            n = len(image)
            for m, v in zip(names, vals):
                for p in range(parts):
                    dom[m][p] += float(sum(v[:, p]) / n)
        for m in names:
            dom[m] = [d / max(len(loader), 1) for d in dom[m]]
            per[m].append(dom[m])
            for p in range(parts):
                val[m][p] += dom[m][p]
    model.train()
    for m in names:
        val[m] = [v / len(loaders) for v in val[m]]
    return val, per, changed


@pytest.mark.parametrize("bs", [1, 3])
def test_validate_with_post_process_equals_cpu_processed_planes(setup, bs):
    from ustrun.evaluate import validate
    dataset, model, loaders = setup
    val, per, changed = _expected(dataset, model, loaders[bs])
    assert changed > 0                                   # the post-processing did change some predictions
    for coalesce in (64, 1):
        got = validate(dataset, model, loaders[bs], epoch=3, log=None, coalesce=coalesce, surface_metrics=True, post_process=True)
        assert got[0] == val["dice"] and got[1] == per["dice"]
        for m in ("dc", "jc", "hd", "asd"):
            assert got[2][m]["val"] == val[m] and got[2][m]["per_domain"] == per[m], m
    assert model.training


def test_switched_off_it_is_the_path_it_was(setup):
    from ustrun.evaluate import validate
    dataset, model, loaders = setup
    a_lines, b_lines, c_lines = [], [], []
    a = validate(dataset, model, loaders[3], epoch=3, log=a_lines.append, surface_metrics=True)
    b = validate(dataset, model, loaders[3], epoch=3, log=b_lines.append, surface_metrics=True, post_process=False)
    assert a == b and a_lines == b_lines and len(a_lines) == 3
    c = validate(dataset, model, loaders[3], epoch=3, log=c_lines.append, surface_metrics=True, post_process=True)
    assert len(c_lines) == len(a_lines) and c != a        # the same lines, other numbers
    assert [t.split(":")[0] for t in c_lines] == [t.split(":")[0] for t in a_lines] and "_hd: " in c_lines[0]
    assert validate(dataset, model, loaders[3], log=None) == validate(dataset, model, loaders[3], log=None, post_process=False)


def test_saved_pictures_show_the_processed_planes(setup, tmp_path):
    from PIL import Image
    from ustrun import functional as F
    from ustrun import render
    from ustrun.evaluate import PARTS, validate
    from utils import metrics
    dataset, model, loaders = setup
    parts = len(PARTS[dataset])
    out = tmp_path / "pics"
    got = validate(dataset, model, loaders[3], log=None, save_dir=str(out), post_process=True)
    assert got == validate(dataset, model, loaders[3], log=None, post_process=True)
    names, pics, num = [], [], 0
    model.eval()
    for dom, loader in enumerate(loaders[3]):
        for batch in loader:
            image, P, G, _ = _cpu_processed(dataset, model, batch)
            cf = F.dice_counts(P, G).cpu().numpy().astype(np.float64)
            d = metrics.dice_from_counts(cf[..., 0], cf[..., 1], cf[..., 2])
            dice = [float(sum(d[:, p]) / len(d)) for p in range(parts)]
            rgb = render.render_mask(image, P, parts=parts).cpu().numpy()
            for j in range(len(image)):
                num += 1
                names.append("%d_%d_%s.png" % (dom + 1, num, round(sum(dice) / len(dice), 4)))
                pics.append(rgb[j])
    model.train()
    assert sorted(os.listdir(out)) == sorted(names) and len(names) == 18
    for n, p in zip(names, pics):
        with Image.open(out / n) as im:
            assert np.array_equal(np.asarray(im), p), n


def test_dataloaders_post_processing_keeps_the_reference_signature():
    from dataloaders.utils import post_processing
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[:50, :70]
    d2 = (yy - 25) ** 2 + (xx - 30) ** 2
    p = ((d2 <= 400) & (d2 >= 100)) | (rng.random((50, 70)) < 0.02)
    want = R.process(p)
    assert want.sum() > p.sum() * 1.2 and (p & ~want).any()                # a hole filled, specks removed
    got = post_processing(p.copy())
    assert isinstance(got, np.ndarray) and got.dtype == bool and np.array_equal(got, want)
    assert np.array_equal(post_processing(p.astype(np.uint8)), want)
    for t in (torch.from_numpy(p.astype(np.float32)), torch.from_numpy(p.astype(np.int64)).cuda(), torch.from_numpy(p)):
        g = post_processing(t)
        assert torch.is_tensor(g) and g.dtype == t.dtype and g.device == t.device and g.shape == t.shape
        assert np.array_equal(g.cpu().numpy() != 0, want)
    with pytest.raises(ValueError, match="2-D"):
        post_processing(np.zeros((2, 4, 4), bool))


def test_script_with_post_process_logs_the_surface_lines(tmp_path):
    from networks.unet_model import UNet
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ust-run_amd")
    torch.manual_seed(6)
    ck = tmp_path / "w.pth"
    torch.save(UNet(n_channels=1, n_classes=2).state_dict(), ck)
    cmd = [sys.executable, os.path.join(root, "test.py"), "--dataset", "prostate", "--post_process", "1", "--surface_metrics", "1",
           "--load_path", str(ck), "--test_bs", "2", "--test_batches", "1", "--domain_num", "2", "--image_size", "64"]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("val_base_hd: ") == 3 and r.stdout.count("val_base_dice: ") == 3 and "post_process=1" in r.stdout
