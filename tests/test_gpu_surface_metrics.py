"""GPU parity of the device surface-distance metrics (ustrun_surface_metrics -> utils.metrics.surface_from_records ->
ustrun.evaluate.validate(surface_metrics=True)) against the scipy-generated fixture g15 and the brute-force numpy restatement
of tests/surface_brute.py.  Bounds: every integer field (border sizes, both order statistics) and dc / jc (the same f64
quotient of integers) are EXACT; hd95 and asd are within 1e-9 relative -- everything before the square roots is exact integer
work, what remains is f64 rounding of sums of <= 1e5 terms (~1e-11) and the one-ulp variants of numpy's lerp."""
import os

import numpy as np
import pytest
import torch

import surface_brute as B
from test_gpu_eval import _weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "g15_surface_metrics.npz"), allow_pickle=False)
RTOL = 1e-9


def _device_records(pred, gt, by_class, K):
    from ustrun import functional as F
    rec = F.surface_metrics(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), by_class=by_class, n_classes=K)
    cnt = F.dice_counts(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), by_class=by_class, n_classes=K)
    assert rec.dtype == torch.int32 and rec.is_cuda and tuple(rec.shape[2:]) == (6,)
    return rec.cpu().numpy(), cnt.cpu().numpy()


def _check_against_brute(pred, gt, by_class, K):
    from utils import metrics
    rec, cnt = _device_records(pred, gt, by_class, K)
    want, wcnt = B.records(pred, gt, by_class, K)
    print("records: device\n", rec[..., :4].reshape(-1, 4), "\nbrute\n", want[..., :4].reshape(-1, 4))
    print("sums: device", B.record_sum(rec).ravel(), "brute", B.record_sum(want).ravel())
    assert np.array_equal(cnt, wcnt)
    assert np.array_equal(rec[..., :4], want[..., :4])
    np.testing.assert_allclose(B.record_sum(rec), B.record_sum(want), rtol=RTOL, atol=0)
    P, G = B.planes(pred, gt, by_class, K)
    ok = wcnt[..., 1] > 0                                   # samples the reference can score (non-empty ground truth)
    if ok.all():
        dc, jc, hd, asd = metrics.surface_from_records(rec, cnt)
        m = np.array([[B.metrics(P[n, k], G[n, k]) for k in range(P.shape[1])] for n in range(P.shape[0])])
        assert np.array_equal(dc, m[..., 0]) and np.array_equal(jc, m[..., 1])
        np.testing.assert_allclose(hd, m[..., 2], rtol=RTOL, atol=0)
        np.testing.assert_allclose(asd, m[..., 3], rtol=RTOL, atol=0)
    return rec


@pytest.mark.parametrize("name", B.fixture_cases(Z))
def test_fixture_parity(name):
    from utils import metrics
    pred, gt, by_class, K = B.fixture_inputs(Z, name)
    rec, cnt = _device_records(pred, gt, by_class, K)
    dc, jc, hd, asd = metrics.surface_from_records(rec, cnt)
    for key, got in (("hd95", hd), ("asd", asd)):
        w = Z[f"{name}_{key}"]
        print(name, key, "max rel err", float(np.max(np.abs(got - w) / np.maximum(np.abs(w), 1e-300))))
    assert np.array_equal(rec[..., 0:2], Z[name + "_nborder"])
    assert np.array_equal(rec[..., 2:4], Z[name + "_d2"])
    assert np.array_equal(dc, Z[name + "_dc"]) and np.array_equal(jc, Z[name + "_jc"])
    np.testing.assert_allclose(hd, Z[name + "_hd95"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(asd, Z[name + "_asd"], rtol=RTOL, atol=0)


def _random_masks(kind, density, H, W, seed, N=4):
    rng = np.random.default_rng(seed)
    if kind == "f32":                                       # {0,1} planes [N,2,H,W], the fundus layout
        mk = lambda: (rng.random((N, 2, H, W)) < density).astype(np.float32)
        return mk(), mk(), False, 2
    if kind == "i64":                                       # binary int64 maps [N,H,W], the prostate / BUSI layout
        mk = lambda: (rng.random((N, H, W)) < density).astype(np.int64)
        return mk(), mk(), False, 1
    mk = lambda: (rng.random((N, H, W)) < density) * rng.integers(1, 4, (N, H, W))      # class maps, the M&Ms layout
    return mk().astype(np.int64), mk().astype(np.int64), True, 3


@pytest.mark.parametrize("kind", ["f32", "i64", "i64_class"])
@pytest.mark.parametrize("H,W", [(64, 64), (33, 57)])
@pytest.mark.parametrize("density", [0.02, 0.3, 0.9])
def test_brute_force_parity_random_masks(kind, H, W, density):
    _check_against_brute(*_random_masks(kind, density, H, W, seed=int(density * 100) + H))


def test_brute_force_parity_mixed_input_types():
    """prediction int64, ground truth f32 (and the reverse): each side's type flag is its own"""
    p, g, by_class, K = _random_masks("i64", 0.3, 33, 57, seed=3)
    _check_against_brute(p, g.astype(np.float32), by_class, K)
    _check_against_brute(p.astype(np.float32), g, by_class, K)


@pytest.mark.parametrize("H,W", [(1024, 1024), (1024, 1000), (1, 1), (1, 7), (5, 1), (2, 1024), (1024, 3), (65, 129)])
def test_brute_force_parity_extreme_extents(H, W):
    """the limits of the accepted range (d2 up to 2 * 1023^2 < 2^21: opposite corners) and degenerate planes"""
    N = 4
    p, g = np.zeros((N, 1, H, W), np.float32), np.zeros((N, 1, H, W), np.float32)
    p[0, 0, 0, 0], g[0, 0, H - 1, W - 1] = 1, 1             # opposite corners
    p[1], g[1] = 1, 1                                       # both fill the frame
    g[1, 0, H // 2, W // 2] = 1
    yy, xx = np.mgrid[:H, :W]
    p[2, 0] = (yy - 0.4 * H) ** 2 + (xx - 0.45 * W) ** 2 <= (0.2 * min(H, W)) ** 2
    g[2, 0] = (yy - 0.5 * H) ** 2 + (xx - 0.5 * W) ** 2 <= (0.25 * min(H, W)) ** 2
    p[2, 0, 0, 0], g[2, 0, 0, 0] = 1, 1                     # never empty, whatever the extent
    p[3, 0, :, W - 1], g[3, 0, 0, :] = 1, 1                 # the last column against the first row
    _check_against_brute(p, g, False, 1)


def test_two_calls_give_identical_bits():
    from ustrun import functional as F
    for name in ("speckle_384", "rings_288_i64", "frame_40x72"):
        pred, gt, by_class, K = B.fixture_inputs(Z, name)
        p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
        a = F.surface_metrics(p, g, by_class=by_class, n_classes=K).cpu()
        b = F.surface_metrics(p, g, by_class=by_class, n_classes=K).cpu()
        assert torch.equal(a, b), name


def test_empty_prediction_scores_100():
    from ustrun.evaluate import sample_metrics
    g = torch.zeros(3, 40, 72, dtype=torch.int64)
    g[:, 10:20, 30:50] = 1
    p = g.clone()
    p[1] = 0
    dice, dc, jc, hd, asd = sample_metrics("prostate", p.cuda(), g.cuda())
    assert (hd[1, 0], asd[1, 0], dc[1, 0], jc[1, 0]) == (100.0, 100.0, 0.0, 0.0)
    assert (hd[0, 0], asd[0, 0], dc[0, 0], jc[0, 0]) == (0.0, 0.0, 1.0, 1.0)


def _model(dataset, c, k, loaders, base=8, seed=21):
    """The model of tests/test_gpu_eval.py, its head bias centred on the first batch's logits (CPU oracle): random weights
    otherwise predict all or nothing, and every score would be the empty-prediction rule's 100."""
    from networks.unet_model import UNet
    from oracle import unet_ref as U
    sd = _weights(c, k, base, seed=seed)
    with torch.no_grad():
        lg = U.unet_forward(loaders[0][0][0], sd, train=False)
    sd["outc.conv.bias"] = sd["outc.conv.bias"] - lg.transpose(0, 1).flatten(1).median(dim=1).values
    model = UNet(n_channels=c, n_classes=k, base_channels=base)
    model.load_state_dict({kk: v.detach().clone() for kk, v in sd.items()})
    return model.cuda()


def test_empty_ground_truth_raises_through_validate():
    from ustrun import synthetic
    from ustrun.evaluate import validate
    loaders = synthetic.test_loaders("prostate", 2, 3, 2, 1, 48, seed=5)
    model = _model("prostate", 1, 2, loaders)
    validate("prostate", model, loaders, log=None, surface_metrics=True)              # as generated: every sample has a label
    x, y = loaders[1][2]
    y = y.clone()
    y[1] = 255.0                                            # prostate foreground is label 0: sample 1 of this batch has none
    loaders[1][2] = (x, y)
    for coalesce in (64, 1):
        with pytest.raises(RuntimeError, match=r"domain 2, loader batch 2, sample 1, part 0"):
            validate("prostate", model, loaders, log=None, surface_metrics=True, coalesce=coalesce)
    assert validate("prostate", model, loaders, log=None)                             # the Dice alone still scores it


def _reference_average(dataset, model, loaders, parts):
    """train.py:306-346,368-375 on the host: per sample (brute force on predict()'s own output), per loader batch, per
    domain loader, over the domains."""
    from ustrun.evaluate import predict
    from ustrun.trainer import decode_labels
    kw = dict(by_class=True, n_classes=3) if dataset == "MNMS" else {}
    val = np.zeros((4, parts))
    per = []
    model.eval()
    for loader in loaders:
        dom = [[0.0] * parts for _ in range(4)]
        for image, label in loader:
            with torch.no_grad():
                pred = predict(dataset, model(image.cuda())).cpu().numpy()
            P, G = B.planes(pred, decode_labels(dataset, label).numpy(), **kw)
            acc = [[0.0] * parts for _ in range(4)]
            for j in range(len(image)):
                for i in range(parts):
                    for m, v in enumerate(B.metrics(P[j, i], G[j, i])):
                        acc[m][i] += v
            for m in range(4):
                for i in range(parts):
                    dom[m][i] += acc[m][i] / len(image)
        dom = [[v / len(loader) for v in row] for row in dom]
        per.append(dom)
        val += np.array(dom)
    model.train()
    return val / len(loaders), np.array(per)


@pytest.mark.parametrize("dataset,c,k", [("fundus", 3, 2), ("prostate", 1, 2), ("MNMS", 1, 4)])
def test_validate_end_to_end(dataset, c, k):
    from ustrun import synthetic
    from ustrun.evaluate import PARTS, validate
    loaders = synthetic.test_loaders(dataset, 2, 3, 2, c, 48, seed=5)
    model = _model(dataset, c, k, loaders)
    before = validate(dataset, model, loaders, epoch=3, log=None)                      # before the feature's path is touched
    off = validate(dataset, model, loaders, epoch=3, log=None, surface_metrics=False)
    assert isinstance(off, tuple) and len(off) == 2 and off == before
    parts = len(PARTS[dataset])
    want_val, want_per = _reference_average(dataset, model, loaders, parts)
    lines = []
    for coalesce in (64, 1):
        on = validate(dataset, model, loaders, epoch=3, log=lines.append, surface_metrics=True, coalesce=coalesce)
        assert len(on) == 3 and on[0] == before[0] and on[1] == before[1]
        extra = on[2]
        assert sorted(extra) == ["asd", "dc", "hd", "jc"]
        for m, name in enumerate(("dc", "jc", "hd", "asd")):
            got_val, got_per = np.array(extra[name]["val"]), np.array(extra[name]["per_domain"])
            assert got_val.shape == (parts,) and got_per.shape == (len(loaders), parts)
            print(dataset, coalesce, name, got_val, want_val[m])
            if name in ("dc", "jc"):
                assert np.array_equal(got_val, want_val[m]) and np.array_equal(got_per, want_per[:, m])
            else:
                np.testing.assert_allclose(got_val, want_val[m], rtol=RTOL, atol=0)
                np.testing.assert_allclose(got_per, want_per[:, m], rtol=RTOL, atol=0)
    assert (np.array(extra["hd"]["per_domain"]) < 100).all()             # real distances, not the empty-prediction rule
    assert model.training
    p0 = PARTS[dataset][0]
    assert len(lines) == 2 * (len(loaders) + 1)
    assert all(all("val_%s_%s: " % (p0, m) in t for m in ("dice", "dc", "jc", "hd", "asd")) for t in lines)
    plain = []
    validate(dataset, model, loaders, epoch=3, log=plain.append)
    assert all("_dc" not in t and "_hd" not in t for t in plain) and len(plain) == len(loaders) + 1


def test_extents_above_1024_are_an_error_not_a_launch():
    from ustrun import _lib
    from ustrun import functional as F
    from ustrun.engine import stream_ptr
    for H, W in ((1025, 8), (8, 1025)):
        p = torch.zeros(1, 1, H, W, device="cuda")
        with pytest.raises(RuntimeError, match="1..1024"):
            F.surface_metrics(p, p)
        work = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        out = torch.full((1, 1, 6), -7, dtype=torch.int32, device="cuda")
        rc = _lib.lib().ustrun_surface_metrics(p.data_ptr(), p.data_ptr(), 0, 0, 1, 1, 0, H, W, work.data_ptr(), work.numel(),
                                               out.data_ptr(), stream_ptr())
        assert rc != 0 and b"1..1024" in _lib.lib().ustrun_last_error()
        torch.cuda.synchronize()
        assert bool((out == -7).all())                      # nothing ran
    small = torch.empty(64, dtype=torch.uint8, device="cuda")
    p = torch.zeros(1, 1, 64, 64, device="cuda")
    out = torch.empty((1, 1, 6), dtype=torch.int32, device="cuda")
    rc = _lib.lib().ustrun_surface_metrics(p.data_ptr(), p.data_ptr(), 0, 0, 1, 1, 0, 64, 64, small.data_ptr(), small.numel(),
                                           out.data_ptr(), stream_ptr())
    assert rc != 0 and b"work buffer" in _lib.lib().ustrun_last_error()
