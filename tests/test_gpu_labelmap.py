"""csrc/labelmap.hip through ustrun.functional, utils.metrics and dataloaders.utils on the device against tests/labelmap_ref.py in
float64 and against the reference's own results (g21_labelmap.npz).

Bars, as tests/test_gpu_losses_rest.py.  Scalars: rtol 2e-5 against float64.  Maps and gradients: the restatement is also evaluated
in float32 on the CPU; its max-abs error against float64 is the yardstick, and the device's max-abs error must be
<= max(4 x yardstick, 8 * 2^-24 * max|expected|).  Counts, colours and zeros that must be exact are compared exactly.  Errors are
printed (pytest -s)."""
import numpy as np
import pytest
import torch

import labelmap_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu


def one_in(t):
    """the same values in a contiguous tensor whose storage starts one element past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size()
    return v


def check_scalar(label, got, want):
    got, want = float(got), float(want)
    print("%-40s got %.8e want %.8e" % (label, got, want))
    assert abs(got - want) <= 2e-5 * abs(want), (label, got, want)


def check_map(label, got, want64, yard32):
    assert got.shape == want64.shape and got.dtype == torch.float32 and torch.isfinite(got).all(), label
    err = float((got.double() - want64).abs().max())
    yard = float((yard32.double() - want64).abs().max())
    bar = max(4 * yard, 8 * 2.0 ** -24 * float(want64.abs().max()))
    print("%-40s err %.2e  yardstick %.2e  bar %.2e" % (label, err, yard, bar))
    assert err <= bar, (label, err, yard, bar)


# ---- ce_map --------------------------------------------------------------------------------------------------------------------
# name: (N, K, H, W), weights, keywords, what the targets hold besides classes, which operand sits one element into its buffer
CE = {
    "k1_hw3": ((2, 1, 3, 1), False, dict(), None, None),                                   # fewer pixels than a lane's vector
    "k2_odd": ((2, 2, 9, 13), True, dict(ignore_index=255, by_weight=True), "ignore", None),
    "k21_odd": ((2, 21, 9, 13), True, dict(ignore_negative=True, by_weight=True, by_count=True), "negative", None),
    "k21_vec": ((2, 21, 16, 16), True, dict(ignore_index=255, scale=1.0 / 512), "ignore", None),        # the 16-byte path
    "k256_vec": ((1, 256, 16, 16), False, dict(ignore_index=255, by_count=True), "ignore", None),
    "k256_hw3": ((1, 256, 3, 1), True, dict(by_weight=True), None, None),
    "view_logits": ((2, 2, 16, 16), True, dict(ignore_index=255, by_weight=True), "ignore", "logits"),
    "view_target": ((2, 2, 16, 16), True, dict(ignore_index=255, by_weight=True), "ignore", "target"),
    "view_weight": ((2, 2, 16, 16), True, dict(ignore_index=255, by_weight=True), "ignore", "weight"),
    "image_ignored": ((2, 21, 16, 16), True, dict(ignore_index=255, by_weight=True), "second image", None),
    "negative_kept": ((2, 2, 9, 13), False, dict(ignore_index=255), "negative", None),         # flag off: out of range, counted
    "out_of_range": ((2, 21, 9, 13), True, dict(ignore_index=255, by_weight=True), "beyond", None),
    "pm60": ((1, 21, 16, 16), False, dict(by_count=True), "pm60", None),
    "grid_wrap": ((1, 2, 1025, 1027), False, dict(ignore_index=255, by_count=True), "ignore", None),   # > 1024 blocks x 256 lanes x 4 items
}
_ce_cache = {}


def ce_inputs(name):
    if name in _ce_cache:
        return _ce_cache[name]
    (N, K, H, W), weights, kw, special, _ = CE[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = 3 * torch.randn(N, K, H, W, generator=g)
    t = torch.randint(0, K, (N, H, W), generator=g)
    r = torch.rand(N, H, W, generator=g)
    if special == "ignore":
        t[r < 0.2] = 255
    elif special == "negative":
        t[r < 0.2] = -1
        t[(r >= 0.2) & (r < 0.25)] = -7
    elif special == "second image":
        t[1] = 255
    elif special == "beyond":
        t[r < 0.1] = K
        t[(r >= 0.1) & (r < 0.15)] = -2
        t[(r >= 0.15) & (r < 0.2)] = 255
        t[(r >= 0.2) & (r < 0.22)] = 1 << 40
    elif special == "pm60":
        x = 60.0 * torch.sign(x)
    w = 0.25 + 2 * torch.rand(K, generator=g) if weights else None
    want = R.ce_map(x, t, w, dtype=torch.float64, **kw)
    yard = R.ce_map(x, t, w, dtype=torch.float32, **kw)
    _ce_cache[name] = (x, t, w, kw, want, yard)
    return _ce_cache[name]


def ce_on_device(name):
    from ustrun import functional as F
    x, t, w, kw, _, _ = ce_inputs(name)
    shift = CE[name][4]
    xd, td, wd = x.cuda(), t.cuda(), None if w is None else w.cuda()
    xd = (one_in(xd) if shift == "logits" else xd.clone()).requires_grad_(True)
    td = one_in(td) if shift == "target" else td
    wd = one_in(wd) if shift == "weight" else wd
    loss = F.ce_map(xd, td, weight=wd, **kw)
    (loss * R.UP).backward()
    out, lse = F.ce_map_stats(xd, td, weight=wd, **kw)
    return loss.detach().cpu(), xd.grad.cpu(), out.cpu(), lse.cpu()


@pytest.mark.parametrize("name", list(CE))
def test_ce_map_against_float64(name):
    x, t, w, kw, want, yard = ce_inputs(name)
    loss, grad, out, lse = ce_on_device(name)
    assert float(loss) == float(out[0])
    for i, part in enumerate(("loss", "S", "sum w")):
        check_scalar("%s %s" % (name, part), out[i], want["out"][i])
    assert float(out[3]) == float(want["out"][3]) and float(out[4]) == float(want["out"][4]), (name, out, want["out"])
    check_map(name + " lse", lse, want["lse"], yard["lse"])
    check_map(name + " grad", grad, want["grad"], yard["grad"])
    off = ~want["valid"].reshape(t.shape)[:, None].expand_as(grad)
    assert not grad[off].any()                                   # exactly 0 on ignored and out-of-range pixels
    if name == "out_of_range":
        assert float(out[4]) > 20
    if name == "negative_kept":
        assert float(out[4]) == float((t < 0).sum()) > 0


@pytest.mark.parametrize("shape", [(2, 21, 9, 13), (1, 2, 16, 16)])
def test_ce_map_without_a_valid_pixel(shape):
    from ustrun import functional as F
    N, K, H, W = shape
    x = torch.randn(shape, device="cuda")
    t = torch.full((N, H, W), 255, device="cuda")
    t[0, 0, 0] = -1
    for kw, is_nan in ((dict(by_weight=True), True), (dict(by_count=True), True), (dict(), False)):
        xd = x.clone().requires_grad_(True)
        loss = F.ce_map(xd, t, ignore_index=255, ignore_negative=True, **kw)
        loss.backward()
        loss = loss.detach()
        assert bool(torch.isnan(loss)) == is_nan and (is_nan or float(loss) == 0.0)
        assert not xd.grad.any()                                 # exactly 0, whatever the divisor was
        out, _ = F.ce_map_stats(x, t, ignore_index=255, ignore_negative=True, **kw)
        assert out[1:].tolist() == [0.0, 0.0, 0.0, 0.0]


def test_ce_map_twice_is_bit_identical():
    a, b = ce_on_device("k21_vec"), ce_on_device("k21_vec")
    c, d = ce_on_device("grid_wrap"), ce_on_device("grid_wrap")
    for u, v in zip(a + c, b + d):
        assert torch.equal(u, v)


def test_ce_map_matches_the_reference_functions():
    """utils.metrics.cross_entropy2d and dataloaders.utils.cross_entropy2d against the reference's own values and gradients"""
    import dataloaders.utils as U
    from utils import metrics as M
    gold = load_golden("g21_labelmap")

    def vg(fn, x):
        xd = torch.from_numpy(x).cuda().requires_grad_(True)
        v = fn(xd)
        (v * R.UP).backward()
        return v.detach().cpu(), xd.grad.cpu()

    for K in (2, 21):
        x, tn, t255, w = (gold[f"ce{K}_{n}"] for n in ("logits", "t_neg", "t_255", "weight"))
        tn_d, t255_d, w_d = torch.from_numpy(tn).cuda(), torch.from_numpy(t255).cuda(), torch.from_numpy(w).cuda()
        runs = [(f"ce{K}_metrics_w{wt}_sa{sa}", lambda xd, wt=wt, sa=sa: M.cross_entropy2d(xd, tn_d, weight=w_d if wt else None, size_average=bool(sa)))
                for wt in (0, 1) for sa in (0, 1)]
        runs += [(f"ce{K}_utils_s{sa}_b{ba}", lambda xd, sa=sa, ba=ba: U.cross_entropy2d(xd, t255_d[:, None], size_average=bool(sa), batch_average=bool(ba)))
                 for sa in (0, 1) for ba in (0, 1)]
        runs += [(f"ce{K}_utils_weighted", lambda xd: U.cross_entropy2d(xd, t255_d, weight=w.tolist()))]
        for key, fn in runs:
            v, g = vg(fn, x)
            check_scalar(key, v, gold[key])
            if key + "_grad" in gold:
                ref = torch.from_numpy(gold[key + "_grad"])
                assert float((g - ref).abs().max()) <= 2e-5 * float(ref.abs().max()), key       # the reference's own f32 result


# ---- confusion -----------------------------------------------------------------------------------------------------------------
def conf_case(N, H, W, K, seed, as_float=(False, False)):
    g = torch.Generator().manual_seed(seed)
    p, q = torch.randint(0, K, (N, H, W), generator=g), torch.randint(0, K, (N, H, W), generator=g)
    return (p.float() if as_float[0] else p), (q.float() if as_float[1] else q)


def conf_check(p, q, K, ignore_index=None):
    from ustrun import functional as F
    counts, skipped = F.confusion(p.cuda(), q.cuda(), K, ignore_index)
    again = F.confusion(p.cuda(), q.cuda(), K, ignore_index)
    want, wskip = R.confusion(p.numpy(), q.numpy(), K, ignore_index)
    assert counts.dtype == torch.int32 and skipped.dtype == torch.int32
    assert np.array_equal(counts.cpu().numpy(), want) and np.array_equal(skipped.cpu().numpy(), wskip)
    assert torch.equal(again[0], counts) and torch.equal(again[1], skipped)
    return want, wskip


@pytest.mark.parametrize("K", [1, 2, 21, 32])
@pytest.mark.parametrize("plane", [(1, 1), (1, 7), (33, 47)])
def test_confusion_counts_exact(plane, K):
    H, W = plane
    want, skip = conf_check(*conf_case(3, H, W, K, 100 * K + H), K)           # N = 3 with different content per image
    assert want.sum() == 3 * H * W and not skip.any()


def test_confusion_single_class_images():
    p = torch.full((2, 33, 47), 20)
    q = torch.full((2, 33, 47), 20)
    q[1] = 3
    want, _ = conf_check(p, q, 21)
    assert want[0, 20, 20] == 33 * 47 and want[1, 3, 20] == 33 * 47 and (want != 0).sum() == 2
    big = torch.full((1, 512, 512), 31)
    want, _ = conf_check(big, big.float(), 32)
    assert want[0, 31, 31] == 262144 and (want != 0).sum() == 1              # far past any 16-bit counter


@pytest.mark.parametrize("as_float", [(False, False), (True, False), (False, True), (True, True)])
def test_confusion_label_types_ignore_and_out_of_range(as_float):
    p, q = conf_case(3, 33, 47, 21, 7, as_float)
    q[0, :5] = 255
    q[1, 0, :4] = -1
    q[2, 3, 3] = 21
    p[1, 7, :9] = 21
    p[2, 9, 1] = -3
    if as_float[0]:
        p[0, 20, 20] = 2.5                                                # no integer: out of range
    want, skip = conf_check(p, q, 21, ignore_index=255)
    assert list(skip) == [5 * 47 + int(as_float[0]), 13, 2]
    _, skip = conf_check(p, q, 21)                                           # without ignore_index 255 is out of range all the same
    assert list(skip) == [5 * 47 + int(as_float[0]), 13, 2]


def test_metrics_from_the_confusion_matrix():
    import dataloaders.utils as U
    from utils import metrics as M
    gold = load_golden("g21_labelmap")
    pred, gt = gold["lab_pred"], gold["lab_gt"]
    c21, _ = R.confusion(pred, gt, 21)
    for a, b in ((pred, gt), (torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()), (torch.from_numpy(pred).float().cuda(), torch.from_numpy(gt))):
        iou, dice = U.get_iou(a, b, 21), U.get_dice(a, b)
        assert isinstance(iou, float) and isinstance(dice, float)
        assert abs(iou - R.iou_from_counts(c21)) <= 1e-12 and abs(iou - float(gold["iou_intended"])) <= 1e-12
        assert abs(dice - float(gold["get_dice"])) <= 1e-12
    assert abs(U.get_iou(torch.from_numpy(pred), torch.from_numpy(pred)) - 2.0) <= 1e-12
    cd = M.cal_dice(pred % 5, gt % 5, 5)
    assert cd.dtype == np.float64 and np.abs(cd - gold["cal_dice_5"]).max() <= 1e-12
    assert np.isnan(M.cal_dice(np.zeros((4, 4), int), np.zeros((4, 4), int), 3)).all()       # 0 / 0, as the reference's formula
    with pytest.raises(ValueError, match="get_iou: sample 1"):
        U.get_iou(pred, np.where(np.arange(2)[:, None, None] == 1, 21, gt), 21)
    with pytest.raises(ValueError, match="get_dice"):
        U.get_dice(pred + 32, gt)
    with pytest.raises(ZeroDivisionError):
        U.get_dice(np.zeros((1, 3, 3), int), np.zeros((1, 3, 3), int))


# ---- plane_sums and the losses on it -----------------------------------------------------------------------------------------------
# the shape set of consistency.hip's tests: the 16-byte path, odd HW, K = 1 with HW < 4, an operand one float into its buffer
PS = {"vec": (3, 2, 40, 40), "odd": (2, 4, 33, 37), "k1": (2, 1, 3, 1), "kmax": (1, 8, 5, 7), "view_x": (2, 2, 8, 12), "view_t": (2, 2, 8, 12),
      "pm60": (1, 2, 4, 8)}


def ps_inputs(tag):
    N, K, H, W = PS[tag]
    g = torch.Generator().manual_seed(sum(map(ord, tag)))
    x = 3 * torch.randn(N, K, H, W, generator=g)
    if tag == "pm60":
        x = 60.0 * torch.sign(x)
    t = (torch.rand(N, K, H, W, generator=g) < 0.4).float()
    t[torch.rand(N, K, H, W, generator=g) < 0.1] = 255.0
    return x, t, torch.rand(K, 4, generator=g) + 0.5


@pytest.mark.parametrize("ignore", [None, 255.0])
@pytest.mark.parametrize("act", ["none", "sigmoid"])
@pytest.mark.parametrize("tag", list(PS))
def test_plane_sums_and_gradient(tag, act, ignore):
    from ustrun import functional as F
    x, t, G = ps_inputs(tag)
    if ignore is None:
        t = torch.where(t == 255.0, torch.zeros_like(t), t)
    if act == "none":
        x = torch.sigmoid(x)               # the callers' operand without an activation is a probability map: every sum is of one sign
    res = {}
    for dtype in (torch.float64, torch.float32):
        xx = x.detach().clone().to(dtype).requires_grad_(True)
        s = R.plane_sums(xx, t, act, ignore, dtype)
        g, = torch.autograd.grad((s * G.to(dtype)).sum(), xx)
        res[dtype] = (s.detach(), g)
    xd, td = x.cuda(), t.cuda()
    xd = (one_in(xd) if tag == "view_x" else xd.clone()).requires_grad_(True)
    td = one_in(td) if tag == "view_t" else td
    s = F.plane_sums(xd, td, act, ignore)
    (s * G.cuda()).sum().backward()
    assert torch.equal(F.plane_sums(xd.detach(), td, act, ignore), s)             # two calls bit-identical
    s, want = s.detach().cpu(), res[torch.float64][0]
    for k in range(x.shape[1]):
        for j in range(4):
            if act == "none" and j == 3:
                assert float(s[k, j]) == 0.0
            elif float(want[k, j]) == 0.0:
                assert float(s[k, j]) == 0.0
            else:
                check_scalar("%s %s plane %d col %d" % (tag, act, k, j), s[k, j], want[k, j])
    check_map("%s %s grad" % (tag, act), xd.grad.cpu(), res[torch.float64][1], res[torch.float32][1])
    if ignore is not None:
        assert not xd.grad.cpu()[t == ignore].any()


def _loss_cases():
    from utils import metrics as M
    return {"DiceLoss": (M.DiceLoss, R.DiceLoss, "p", {}), "dice": (M.dice, R.dice, "p", {}),
            "dice_ignore": (M.dice, R.dice, "p", {"ignore_index": 255.0}), "Balanced_DiceLoss": (M.Balanced_DiceLoss, R.Balanced_DiceLoss, "x", {}),
            "WatershedCrossEntropy": (M.WatershedCrossEntropy, R.WatershedCrossEntropy, "x", {})}


@pytest.mark.parametrize("name", ["DiceLoss", "dice", "dice_ignore", "Balanced_DiceLoss", "WatershedCrossEntropy"])
@pytest.mark.parametrize("tag", ["vec", "odd", "view_x", "pm60", "golden"])
def test_sigmoid_map_losses(tag, name):
    fn, ref, operand, kw = _loss_cases()[name]
    gold = load_golden("g21_labelmap")
    if tag == "golden":
        x, t = torch.from_numpy(gold["map_logits"]), torch.from_numpy(gold["map_target_ignore" if name == "dice_ignore" else "map_target"])
    else:
        x, t, _ = ps_inputs(tag)
        if name != "dice_ignore":
            t = torch.where(t == 255.0, torch.zeros_like(t), t)
    a = torch.sigmoid(x) if operand == "p" else x
    want, gwant = R.value_and_grad(ref, a, t, dtype=torch.float64, **kw)
    _, gyard = R.value_and_grad(ref, a, t, dtype=torch.float32, **kw)
    ad = a.cuda()
    ad = (one_in(ad) if tag == "view_x" else ad.clone()).requires_grad_(True)
    v = fn(ad, t.cuda(), **kw)
    (v * R.UP).backward()
    assert v.is_cuda and v.dim() == 0
    v = v.detach()
    check_scalar("%s %s" % (name, tag), v, want)
    check_map("%s %s grad" % (name, tag), ad.grad.cpu(), gwant, gyard)
    if tag == "golden":
        check_scalar("%s against the reference" % name, v, gold[name])
        ref_g = torch.from_numpy(gold[name + "_grad"])
        assert float((ad.grad.cpu() - ref_g).abs().max()) <= 2e-5 * float(ref_g.abs().max())


def test_watershed_with_an_empty_plane_is_finite():
    from utils import metrics as M
    x, t, _ = ps_inputs("vec")
    t = torch.where(t == 255.0, torch.zeros_like(t), t)
    t[:, 1] = 0
    xd = x.cuda().requires_grad_(True)
    v = M.WatershedCrossEntropy(xd, t.cuda())
    v.backward()
    want, gwant = R.value_and_grad(R.WatershedCrossEntropy, x, t, up=1.0)
    assert torch.isfinite(v) and torch.isfinite(xd.grad).all()
    check_scalar("watershed, empty plane", v, want)
    check_map("watershed, empty plane, grad", xd.grad.cpu(), gwant, R.value_and_grad(R.WatershedCrossEntropy, x, t, dtype=torch.float32, up=1.0)[1])


# ---- colorize ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds", ["pascal", "cityscapes"])
def test_colorize_exact(ds):
    import dataloaders.utils as U
    from ustrun import functional as F
    gold = load_golden("g21_labelmap")
    labels, pal = gold["colour_labels"], gold[f"{ds}_labels"]
    labels = np.concatenate([labels, np.array([[-1, -300, 20, 18] + [0] * 9] * 9)[None]])        # negative labels too
    want = R.colorize(labels, pal)                                         # float64 [N,H,W,3]
    assert np.array_equal(want[:2], gold[f"decode_{ds}"])
    want32 = want.astype(np.float32).transpose(0, 3, 1, 2)
    for t in (torch.from_numpy(labels).cuda(), torch.from_numpy(labels).float().cuda(), one_in(torch.from_numpy(labels).cuda())):
        out = F.colorize(t, pal)
        assert out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), want32)
    seq = U.decode_seg_map_sequence(labels, ds)
    assert seq.dtype == torch.float64 and not seq.is_cuda and np.array_equal(seq.numpy(), want.transpose(0, 3, 1, 2))
    dev = U.decode_seg_map_sequence(torch.from_numpy(labels).cuda(), ds)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want32)
    one = U.decode_segmap(labels[0], ds)
    assert isinstance(one, np.ndarray) and one.dtype == np.float64 and np.array_equal(one, gold[f"decode_{ds}"][0])
    one = U.decode_segmap(torch.from_numpy(labels[0]).cuda(), ds)
    assert one.is_cuda and tuple(one.shape) == (9, 13, 3) and np.array_equal(one.cpu().numpy(), want32[0].transpose(1, 2, 0))
    with pytest.raises(NotImplementedError):
        U.decode_segmap(labels[0], "coco")


# ---- refusals: the message names the entry, and nothing is launched (the outputs keep their fill) --------------------------------
def _raw():
    from ustrun import _lib as L
    lib = L.lib()
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device="cuda")
    t = dict(x=z(4096), t=z(4096, torch.int64), w=z(256), pal=z(768, torch.uint8), part=z(lib.ustrun_loss_partials_bytes(1, 1, 1) // 4),
             out=torch.full((64,), 77.0, device="cuda"), big=torch.full((4096,), 77.0, device="cuda"),
             cnt=torch.full((4096,), 77, dtype=torch.int32, device="cuda"), skip=torch.full((8,), 77, dtype=torch.int32, device="cuda"))
    return lib, t, lib.ustrun_loss_partials_bytes(1, 1, 1)


def _err(lib):
    return lib.ustrun_last_error().decode()


def _untouched(t):
    torch.cuda.synchronize()
    return bool((t["out"] == 77.0).all() and (t["big"] == 77.0).all() and (t["cnt"] == 77).all() and (t["skip"] == 77).all())


def _calls(lib, t, nb):
    p = {k: v.data_ptr() for k, v in t.items()}
    return {
        "ce_map_fwd": (lib.ustrun_ce_map_fwd, [p["x"], p["t"], p["w"], 1, 2, 16, 1, 255, 0, 1.0, 0, 0, p["out"], p["big"], p["part"], nb, None], 4, 256, (0, 1, 12, 14), 15),
        "ce_map_bwd": (lib.ustrun_ce_map_bwd, [p["x"], p["t"], p["w"], p["x"], 1, 2, 16, 1, 255, 0, 1.0, 0, 0, p["x"], p["x"], p["big"], None], 5, 256, (0, 1, 3, 13, 14, 15), None),
        "confusion": (lib.ustrun_confusion, [p["t"], p["t"], 1, 1, 1, 2, 16, 0, 0, p["cnt"], p["skip"], None], 5, 32, (0, 1, 9, 10), None),
        "plane_sums_fwd": (lib.ustrun_plane_sums_fwd, [p["x"], p["x"], 1, 2, 16, 1, 0, 0.0, p["out"], p["part"], nb, None], 3, 8, (0, 1, 8, 9), 10),
        "plane_sums_bwd": (lib.ustrun_plane_sums_bwd, [p["x"], p["x"], 1, 2, 16, 1, 0, 0.0, p["x"], p["big"], None], 3, 8, (0, 1, 8, 9), None),
        "colorize": (lib.ustrun_colorize, [p["t"], 1, 1, 16, p["pal"], 21, p["big"], None], 5, 256, (0, 4, 6), None),
    }


@pytest.mark.parametrize("entry", ["ce_map_fwd", "ce_map_bwd", "confusion", "plane_sums_fwd", "plane_sums_bwd", "colorize"])
def test_bad_arguments_are_refused(entry):
    lib, t, nb = _raw()
    fn, args, k_at, k_max, pointers, bytes_at = _calls(lib, t, nb)[entry]
    for K in (0, k_max + 1):
        a = list(args)
        a[k_at] = K
        assert fn(*a) != 0 and _err(lib).startswith(entry + ":") and f"{K} " in _err(lib) and f"1..{k_max}" in _err(lib), _err(lib)
    for i in pointers:
        a = list(args)
        a[i] = None
        assert fn(*a) != 0 and (f"{entry}: null pointer" in _err(lib) or f"{entry}: partials too small" in _err(lib)), (i, _err(lib))
    if bytes_at is not None:
        a = list(args)
        a[bytes_at] = nb - 1
        assert fn(*a) != 0 and _err(lib) == f"{entry}: partials too small"
    assert _untouched(t)
    assert fn(*args) == 0                                          # and the call as it stands goes through
    torch.cuda.synchronize()


def test_confusion_refuses_planes_of_2_to_the_31():
    lib, t, _ = _raw()
    for HW in (1 << 31, 1 << 40, 0, -1):
        rc = lib.ustrun_confusion(t["t"].data_ptr(), t["t"].data_ptr(), 1, 1, 1, 2, HW, 0, 0, t["cnt"].data_ptr(), t["skip"].data_ptr(), None)
        assert rc != 0 and _err(lib).startswith("confusion: HW %d" % HW)
    assert _untouched(t)


def test_python_surface_refuses_what_it_cannot_read():
    from ustrun import functional as F
    x, t = torch.zeros(1, 2, 4, 4, device="cuda"), torch.zeros(1, 4, 4, dtype=torch.int64, device="cuda")
    for bad in (x.half(), x.bfloat16()):
        with pytest.raises(RuntimeError, match="float32"):
            F.ce_map(bad, t)
        with pytest.raises(RuntimeError, match="float32"):
            F.plane_sums(bad, bad)
        with pytest.raises(RuntimeError, match="int64 or float32"):
            F.confusion(bad[:, 0], t, 2)
        with pytest.raises(RuntimeError, match="int64 or float32"):
            F.colorize(bad[:, 0], np.zeros((2, 3), np.uint8))
    with pytest.raises(RuntimeError, match="target must be an int64"):
        F.ce_map(x, t.int())
    with pytest.raises(RuntimeError, match="weight has 3 entries"):
        F.ce_map(x, t, weight=torch.ones(3, device="cuda"))
    with pytest.raises(RuntimeError, match=r"confusion: 33 classes \(1\.\.32\)"):
        F.confusion(t, t, 33)
    with pytest.raises(RuntimeError, match=r"ce_map_fwd: 257 classes"):
        F.ce_map(torch.zeros(1, 257, 2, 2, device="cuda"), torch.zeros(1, 2, 2, dtype=torch.int64, device="cuda"))
    with pytest.raises(RuntimeError, match="palette must be"):
        F.colorize(t, np.zeros((2, 3), np.int64))
