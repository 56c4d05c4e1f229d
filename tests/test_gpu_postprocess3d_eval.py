"""The public surface above ustrun_post_process_3d: ustrun.evaluate.validate_volumes(post_process=..., largest=...) cleans every
case's stacked prediction as a volume before utils.metrics.volume_metrics measures it, and is what it was without the keywords;
dataloaders.utils.post_processing_volume is the reference's post_processing handed a volume.  The expectation is
tests/postprocess3d_ref.py's output put through the same volume_metrics."""
import numpy as np
import pytest
import torch

import postprocess3d_ref as R

pytestmark = pytest.mark.gpu

NAMES = ["caseA_s0.png", "caseB_s0.png", "caseA_s1.png", "caseB_s1.png", "caseB_s2.png", "caseA_s2.png", "caseA_s3.png", "caseA_s4.png"]
PATTERN = r"(case[A-Z])_"


class _Pool:
    """what validate_volumes reads of a ustrun.datasets.ResidentDataset: images / labels uint8 [n,H,W,C] on the device, names"""

    def __init__(self, images, labels, names):
        self.images, self.labels, self.names = torch.from_numpy(images).cuda(), torch.from_numpy(labels).cuda(), names


class _ByIntensity(torch.nn.Module):
    """a stand-in network whose class follows the image's intensity, scaled to the image's own range (per image, so coalescing
    cannot matter): what is under test is the cleaning of the stacked prediction, not the network"""

    def __init__(self, k):
        super().__init__()
        self.k, self.dummy = k, torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        lo, hi = x.amin(dim=(1, 2, 3), keepdim=True), x.amax(dim=(1, 2, 3), keepdim=True)
        levels = torch.linspace(0.0, 1.0, self.k, device=x.device).view(1, self.k, 1, 1)
        return -((x - lo) / (hi - lo) - levels) ** 2


def _pool(dataset, parts):
    """nested discs per slice; what the image shows is the structure moved, with a cavity in the inner slices of a case and a
    stray blob of the outermost class in one slice of each case: the prediction errs the way post-processing mends"""
    rng = np.random.default_rng(30)
    n, H = len(NAMES), 48
    truth = np.zeros((n, H, H), np.int64)
    yy, xx = np.mgrid[:H, :H]
    for i in range(n):
        cy, cx, r = rng.integers(22, 26), rng.integers(22, 26), rng.integers(12, 16)
        for c in range(parts):
            truth[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= (r * (1 - c / (parts + 0.5))) ** 2] = c + 1
    seen = np.roll(truth, (2, -3), axis=(1, 2))
    for i in (2, 3, 5, 6):                               # inner slices of both cases: a cavity in the innermost class
        seen[i, 25:27, 21:23] = 0
    seen[2, 2:5, 3:6] = seen[4, 40:44, 40:43] = 1        # stray blobs
    images = (seen * (200 // parts) + 20 + rng.integers(0, 12, seen.shape)).astype(np.uint8)[..., None]
    if dataset == "prostate":
        labels = np.where(truth == 1, 0, 255).astype(np.uint8)[..., None]    # foreground is 0 (train.py:590-608)
    else:
        labels = np.stack([np.where(truth == c + 1, 255, 0) for c in range(3)], axis=-1).astype(np.uint8)
    return _Pool(images, labels, NAMES)


@pytest.mark.parametrize("dataset,k,spacing", [("prostate", 2, (2.5, 1, 1)), ("MNMS", 4, None)])
def test_validate_volumes_post_processes_each_case_as_a_volume(dataset, k, spacing):
    from ustrun import datasets
    from ustrun.evaluate import PARTS, case_groups, predict, validate_volumes
    from ustrun.trainer import decode_labels
    from utils import metrics
    parts = len(PARTS[dataset])
    pool, model = _pool(dataset, parts), _ByIntensity(k).cuda()
    plain = validate_volumes(dataset, model, [pool], PATTERN, voxelspacing=spacing, log=None, coalesce=3)
    model.eval()
    with torch.no_grad():
        x, _, y = datasets.stage_finish(pool.images, None, pool.labels)
        pred, mask = predict(dataset, model(x)).cpu().numpy(), decode_labels(dataset, y).cpu().numpy()
    model.train()
    groups = case_groups(NAMES, PATTERN)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    def mean_over_cases(measure):
        acc = {m: np.zeros(parts) for m in plain[0]}
        for _, idx in groups:
            one = measure(idx)
            for m in acc:
                acc[m] += one[m][0]
        return {m: acc[m] / len(groups) for m in acc}

    def expected(clean):
        return mean_over_cases(lambda idx: metrics.volume_metrics(
            dev(np.stack([clean(pred[idx] == c + 1) for c in range(parts)])[None]),
            dev(np.stack([mask[idx] == c + 1 for c in range(parts)])[None]), voxelspacing=spacing))

    # without the keywords: the path as it was -- the class maps themselves into volume_metrics --, bit for bit
    kw_parts = dict(by_class=True, n_classes=3) if dataset == "MNMS" else {}
    today = mean_over_cases(lambda idx: metrics.volume_metrics(torch.from_numpy(pred[idx][None]).cuda(), torch.from_numpy(mask[idx][None]).cuda(),
                                                               voxelspacing=spacing, **kw_parts))
    for m in today:
        assert np.array_equal(np.asarray(plain[0][m]), today[m]), m
    assert plain == validate_volumes(dataset, model, [pool], PATTERN, voxelspacing=spacing, log=None, coalesce=3, post_process=False,
                                     largest=False)
    changed = 0
    for kw in (dict(post_process=True), dict(largest=True), dict(post_process=True, largest=True)):
        lines = []
        got = validate_volumes(dataset, model, [pool], PATTERN, voxelspacing=spacing, log=lines.append, coalesce=3, **kw)
        assert model.training and len(got) == 1 and len(lines) == 1 and "vol_%s_hd95: " % PARTS[dataset][0] in lines[0]
        post, largest = kw.get("post_process", False), kw.get("largest", False)
        want = expected(lambda p: R.process(p, post, (1, 5) if post else None, largest))
        for m in want:
            print(dataset, kw, m, got[0][m], want[m].tolist(), plain[0][m])
            assert np.allclose(got[0][m], want[m], rtol=1e-12, atol=0), (kw, m)
        changed += any(got[0][m] != plain[0][m] for m in got[0])
    assert changed == 3                                      # every rule here removes the stray blobs: the keywords are live


def test_post_processing_volume_takes_numpy_and_tensors():
    from dataloaders import utils as U
    rng = np.random.default_rng(3)
    p = rng.random((6, 20, 70)) < 0.55
    want = R.process(p)
    assert 0 < want.sum() != p.sum()
    got = U.post_processing_volume(p)
    assert isinstance(got, np.ndarray) and got.dtype == bool and np.array_equal(got, want)
    assert np.array_equal(U.post_processing_volume(p.astype(np.uint8) * 255), want)
    for t in (torch.from_numpy(p.astype(np.float32)), torch.from_numpy(p.astype(np.int64)).cuda(), torch.from_numpy(p).cuda()):
        out = U.post_processing_volume(t)
        assert out.device == t.device and out.dtype == t.dtype and np.array_equal(out.cpu().numpy() != 0, want)
    with pytest.raises(ValueError, match="3-D volume"):
        U.post_processing_volume(p[0])
    with pytest.raises(ValueError, match="2-D plane"):       # the plane entry keeps refusing volumes
        U.post_processing(p)
