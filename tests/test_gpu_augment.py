"""The augmentation kernels (csrc/augment.hip) against the g16 goldens: one reference transform per record, on uniform noise
images, its random draws pinned (tools/gen_augment_goldens.py).

Bars.  Image outputs: |device - golden| <= 1 grey level at every pixel the golden does not exclude -- both are the same real
value, the reference's perturbed by at most half a level of intermediate rounding, each rounded or truncated once, and the
float error (at most 165-tap f32 sums of values <= 255) is far below a level.  Label outputs: exact.  Exclusions come from
the golden (float64, never the code under test) and cover at most 0.5 % of a case; the resize and the rotation of the LABEL
carry none, PIL's nearest paths being integer / running-sum arithmetic that the kernels repeat to the bit.  The share of
exactly equal pixels is printed per case (profiles/augment.md): a finding, not a gate.

Measured on an MI355X, every case here: image outputs of scale-crop, rotate, elastic warp, brightness, contrast and blur
are equal to the golden at every pixel (share 1.0), labels exact; the field's rel-L2 is 1.3e-7 to 3.0e-7."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
CAP = 0.005


@pytest.fixture(scope="module")
def D():
    from ustrun import datasets
    return datasets


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def img4(a):
    """[H, W] or [H, W, C] -> uint8 device [1, H, W, C]"""
    a = np.asarray(a)
    return dev(a.reshape(1, a.shape[0], a.shape[1], -1))


def rows(D, n=1):
    return np.zeros((n, D.ROW), np.int64)


def close_image(got, want, excl, what):
    got, want = got.cpu().numpy().reshape(want.shape).astype(np.int64), want.astype(np.int64)
    keep = np.ones(want.shape[:2], bool) if excl is None else excl == 0
    assert keep.mean() >= 1 - CAP, f"{what}: exclusion mask covers {1 - keep.mean():.4f}"
    d = np.abs(got - want)[keep]
    print(f"{what}: max |d| {d.max()}, share equal {(d == 0).mean():.4f}, excluded {1 - keep.mean():.4f}")
    assert d.max() <= 1, what


def equal_label(got, want, excl, what):
    got = got.cpu().numpy().reshape(want.shape)
    keep = np.ones(want.shape[:2], bool) if excl is None else excl == 0
    assert keep.mean() >= 1 - CAP, f"{what}: exclusion mask covers {1 - keep.mean():.4f}"
    assert np.array_equal(got[keep], want[keep]), f"{what}: {(got[keep] != want[keep]).sum()} label values differ"


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert torch.equal(x, y)                     # every reduction has a fixed order
    return a


# ------------------------------------------------------------------------------------------------------------- scale-crop
@pytest.mark.parametrize("case", ["a_off", "a_on", "a_pad", "b_off", "b_on", "b_pad"])
def test_scale_crop(D, case):
    g = load_golden("g16_augment_crop")
    k = case[0]
    src = f"in_{k}_small" if case.endswith("pad") else f"in_{k}"
    on, w, h, pad, x1, y1, patch = (int(v) for v in g[f"sc_{case}_params"])
    r = rows(D)
    r[0, D.SC:D.SC + 8] = D.scale_crop_words(on, w, h, x1, y1, patch, 0)
    assert r[0, D.SC + 3] == pad
    p = dev(r.astype(np.int32))
    img, lab = img4(g[src + "_img"]), img4(g[src + "_lab"])
    oi, ol = twice(lambda: D.stage_scale_crop(img, lab, p, patch))
    close_image(oi, g[f"sc_{case}_img"], None, "scale_crop " + case)
    equal_label(ol, g[f"sc_{case}_lab"], None, "scale_crop " + case)
    if case.endswith("off"):
        assert torch.equal(oi, img) and torch.equal(ol, lab)             # gate off, source at patch size: a byte copy


# ---------------------------------------------------------------------------------------------------------- rotate + flip
ROT_CASES = [f"{k}_{d}_{f}" for k in "ab" for d, f in (("off", 0), ("off", 1), (0, 0), (1, 0), (-1, 1), (20, 1), (-20, 0), (7, 0))] + ["b_fill255_13"]


@pytest.mark.parametrize("case", ROT_CASES)
def test_rotate_and_flip(D, case):
    g = load_golden("g16_augment_rotate")
    k = case[0]
    deg, flip, fill = (int(v) for v in g[f"rot_{case}_params"])
    img, lab = img4(g[f"in_{k}_img"]), img4(g[f"in_{k}_lab"])
    H, W = img.shape[1:3]
    r = rows(D)
    r[0, D.ROT:D.ROT + 4] = [int(deg % 360 != 0), flip, fill, 0]
    if deg % 360:
        r[0, D.ROT + 4:D.ROT + 22] = D.rotate_words(deg, W, H)
    p = dev(r.astype(np.int32))
    oi, ol = twice(lambda: D.stage_rotate(img, lab, p))
    close_image(oi, g[f"rot_{case}_img"], g[f"rot_{case}_ximg"], "rotate " + case)
    equal_label(ol, g[f"rot_{case}_lab"], g[f"rot_{case}_xlab"] if f"rot_{case}_xlab" in g.files else None, "rotate " + case)
    if deg % 360 == 0 and not flip:
        assert torch.equal(oi, img) and torch.equal(ol, lab)


# ---------------------------------------------------------------------------------------------------------------- elastic
@pytest.mark.parametrize("k", ["a", "b"])
def test_elastic_warp_and_gate(D, k):
    g = load_golden("g16_augment_elastic")
    img, lab = img4(g[f"in_{k}_img"]), img4(g[f"in_{k}_lab"])
    r = rows(D)
    p0 = dev(r.astype(np.int32))
    r[0, D.EL] = 1
    p1 = dev(r.astype(np.int32))
    field = dev(g[f"el_{k}_on_field"].astype(np.float32)[None])
    oi, ol = twice(lambda: D.stage_elastic_warp(img, lab, field, p1))
    close_image(oi, g[f"el_{k}_on_img"], g[f"el_{k}_on_ximg"], "elastic warp " + k)
    equal_label(ol, g[f"el_{k}_on_lab"], g[f"el_{k}_on_xlab"], "elastic warp " + k)
    oi, ol = D.stage_elastic_warp(img, lab, field, p0)
    assert torch.equal(oi, img) and torch.equal(ol, lab)
    assert np.array_equal(g[f"el_{k}_off_img"], g[f"in_{k}_img"]) and np.array_equal(g[f"el_{k}_off_lab"], g[f"in_{k}_lab"])


def field_bars(got, want, alpha, what):
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    mx = np.abs(got - want).max()
    print(f"{what}: rel-L2 {rel:.3e}, max-abs {mx:.3e} (bar {1e-4 * alpha:.3e})")
    assert rel <= 1e-5 and mx <= 1e-4 * alpha, what


@pytest.mark.parametrize("k", ["a", "b"])
def test_elastic_field_from_given_noise(D, k):
    g = load_golden("g16_augment_elastic")
    noise = g[f"el_{k}_on_noise"]
    H = noise.shape[1]
    r = rows(D)
    r[0, D.EL] = 1
    p = dev(r.astype(np.int32))
    (f,) = twice(lambda: (D.stage_elastic_field(p, 1, H, H, 0, dev(noise[None])),))
    field_bars(f[0].cpu().numpy().astype(np.float64), g[f"el_{k}_on_field"], 2 * H, "field " + k)


def test_elastic_field_at_real_extent(D):
    g = load_golden("g16_augment_big")
    rs = np.random.RandomState(int(g["field_seed"][0]))
    noise = (rs.rand(256, 256) * 2 - 1).astype(np.float32)
    r = rows(D, 2)
    r[:, D.EL] = 1
    p = dev(r.astype(np.int32))
    f = D.stage_elastic_field(p, 2, 256, 256, 0, dev(np.stack([np.stack([noise, noise]), np.stack([noise[::-1], noise])])))
    f = f.cpu().numpy().astype(np.float64)
    got, want = f[0, 0].reshape(-1)[g["field_idx"]], g["field_val"]              # 4096 sampled positions
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"field 256: rel-L2 {rel:.3e}, max-abs {np.abs(got - want).max():.3e}")
    assert rel <= 1e-5 and np.abs(got - want).max() <= 1e-4 * 512
    assert np.array_equal(f[0, 0], f[0, 1]) and np.array_equal(f[0, 0], f[1, 1]) and not np.array_equal(f[0, 0], f[1, 0])


def test_elastic_generator(D):
    """The on-device noise: mean and variance within 4 standard errors of uniform(-1, 1) at 64 x 64 (n = 4096: se of the mean
    sqrt(1 / 3n), of the variance sqrt((1 / 5 - 1 / 9) / n)); the same seed repeats to the bit; two samples of a batch, and
    the two fields of a sample, differ; the field entry smooths exactly these values; a gated-off sample is not written."""
    H, n = 64, 64 * 64
    a, b, c = D.elastic_noise(3, H, H, 1234), D.elastic_noise(3, H, H, 1234), D.elastic_noise(3, H, H, 1235)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[0, 0], a[0, 1])
    for plane in a.reshape(6, -1).cpu().numpy().astype(np.float64):
        assert plane.min() >= -1 and plane.max() < 1
        assert abs(plane.mean()) <= 4 * np.sqrt(1 / 3 / n), plane.mean()
        assert abs(plane.var() - 1 / 3) <= 4 * np.sqrt((1 / 5 - 1 / 9) / n), plane.var()
    r = rows(D, 3)
    r[:2, D.EL] = 1
    p = dev(r.astype(np.int32))
    f0, f1 = D.stage_elastic_field(p, 3, H, H, 1234), D.stage_elastic_field(p, 3, H, H, 1234, a)
    assert torch.equal(f0[:2], f1[:2]) and torch.isfinite(f0[:2]).all()
    marked = torch.full((3, 2, H, H), 7.0, device="cuda")
    from ustrun import _lib
    work = torch.empty_like(marked)
    _lib.check(_lib.lib().ustrun_aug_elastic_field(None, 1234, p[:, D.EL:].data_ptr(), D.ROW, 3, H, H, marked.data_ptr(), work.data_ptr(), None))
    assert torch.equal(marked[:2], f0[:2]) and bool((marked[2] == 7.0).all())


def test_elastic_refuses_non_square(D):
    from ustrun import _lib
    h = _lib.lib()
    x = torch.zeros(1, 2, 40, 48, device="cuda")
    u = torch.zeros(1, 40, 48, 1, dtype=torch.uint8, device="cuda")
    p = torch.zeros(1, D.ROW, dtype=torch.int32, device="cuda")
    rc = h.ustrun_aug_elastic_field(None, 0, p.data_ptr(), D.ROW, 1, 40, 48, x.data_ptr(), x.data_ptr(), None)
    assert rc != 0 and b"square" in h.ustrun_last_error()
    rc = h.ustrun_aug_elastic_warp(u.data_ptr(), u.data_ptr(), x.data_ptr(), p.data_ptr(), D.ROW, 1, 40, 48, 1, 1, u.data_ptr(),
                                   u.data_ptr(), None)
    assert rc != 0 and b"square" in h.ustrun_last_error()


# ----------------------------------------------------------------------------------------------------------------- strong
def strong_row(D, gate, vb, vc, sg):
    r = rows(D)
    r[0, D.ST:D.ST + 4] = [gate, D._f32_bits(vb), D._f32_bits(vc), D._f32_bits(sg)]
    return dev(r.astype(np.int32))


@pytest.mark.parametrize("k,v", [("a", 0.5), ("a", 1.0), ("a", 1.5), ("b", 0.1), ("b", 1.0), ("b", 2.0)])
def test_brightness_and_contrast(D, k, v):
    g = load_golden("g16_augment_tone")
    img = img4(g[f"in_{k}_img"])
    vv = float(g[f"br_{k}_{v}_v"][0])
    (o,) = twice(lambda: (D.stage_strong(img, strong_row(D, 1, vv, 1.0, 1.0), 3),))
    close_image(o, g[f"br_{k}_{v}"], None, f"brightness {k} {v}")
    o = D.stage_strong(img, strong_row(D, 1, 1.0, vv, 1.0), 3)
    close_image(o, g[f"co_{k}_{v}"], None, f"contrast {k} {v}")
    assert torch.equal(D.stage_strong(img, strong_row(D, 0, vv, vv, 1.0), 3), img)       # gate off: a byte copy


@pytest.mark.parametrize("k,sg", [(k, s) for k in "ab" for s in (0.1, 1.0, 2.0)])
def test_blur(D, k, sg):
    g = load_golden("g16_augment_tone")
    img = img4(g[f"in_{k}_img"])
    r = int(g["blur_r"][0 if k == "a" else 1])
    (o,) = twice(lambda: (D.stage_strong(img, strong_row(D, 2, 1.0, 1.0, sg), r),))
    close_image(o, g[f"bl_{k}_{sg}"], None, f"blur {k} {sg}")


def test_blur_at_real_extent(D):
    g = load_golden("g16_augment_big")
    im = np.random.RandomState(int(g["blur_seed"][0])).randint(0, 256, (384, 384)).astype(np.uint8)
    o = D.stage_strong(img4(im), strong_row(D, 2, 1.0, 1.0, float(g["blur_sigma"][0])), D.blur_radius(384))
    assert D.blur_radius(384) == 19 and D.blur_radius(256) == 12 and D.blur_radius(288) == 14
    d = np.abs(o.cpu().numpy().reshape(-1)[g["blur_idx"]].astype(np.int64) - g["blur_val"].astype(np.int64))
    print(f"blur 384, r 19: max |d| {d.max()}, share equal {(d == 0).mean():.4f}")
    assert d.max() <= 1


# ------------------------------------------------------------------------------------------------------------------ chains
@pytest.mark.parametrize("ds", ["fundus", "prostate", "BUSI", "MNMS"])
def test_chain_stage_by_stage(D, ds):
    """Every stage fed the golden's input of that stage, so one stage's +-1 does not move the next one's nearest decisions."""
    g = load_golden("g16_augment_chain")
    n, w, h, x1, y1, deg, flip, fill, r_blur = (int(v) for v in g[f"{ds}_params"])
    vb, vc, sg = (float(v) for v in g[f"{ds}_strong"])
    r = rows(D)
    r[0, D.SC:D.SC + 8] = D.scale_crop_words(1, w, h, x1, y1, n, fill)
    r[0, D.ROT:D.ROT + 4] = [1, flip, fill, 0]
    r[0, D.ROT + 4:D.ROT + 22] = D.rotate_words(deg, n, n)
    r[0, D.EL] = 1
    r[0, D.ST:D.ST + 4] = [3, D._f32_bits(vb), D._f32_bits(vc), D._f32_bits(sg)]
    p = dev(r.astype(np.int32))
    S = lambda i, what: img4(g[f"{ds}_s{i}_{what}"])
    oi, ol = D.stage_scale_crop(S(0, "img"), S(0, "lab"), p, n)
    close_image(oi, g[f"{ds}_s1_img"], None, ds + " crop")
    equal_label(ol, g[f"{ds}_s1_lab"], None, ds + " crop")
    oi, ol = D.stage_rotate(S(1, "img"), S(1, "lab"), p)                                # rotate + flip: against the flip's output
    close_image(oi, g[f"{ds}_s3_img"], g[f"{ds}_x3_img"], ds + " rotate+flip")
    equal_label(ol, g[f"{ds}_s3_lab"], None, ds + " rotate+flip")
    oi, ol = D.stage_elastic_warp(S(3, "img"), S(3, "lab"), dev(g[f"{ds}_field"][None]), p)
    close_image(oi, g[f"{ds}_s4_img"], g[f"{ds}_x4_img"], ds + " warp")
    equal_label(ol, g[f"{ds}_s4_lab"], g[f"{ds}_x4_lab"], ds + " warp")
    weak = S(4, "img")
    o = D.stage_strong(weak, p, r_blur)                                                  # brightness, contrast, blur in one entry
    close_image(o, g[f"{ds}_t3_img"], None, ds + " strong")
    xw, xs, y = D.stage_finish(weak, o, S(4, "lab"))
    C = weak.shape[3]
    want = torch.from_numpy(g[f"{ds}_s4_img"].reshape(n, n, C).astype(np.float32)).permute(2, 0, 1) / 127.5 - 1
    assert torch.equal(xw[0].cpu(), want) and xw.shape == (1, C, n, n) and xs.shape == xw.shape
    assert torch.equal(y[0].cpu(), torch.from_numpy(g[f"{ds}_s4_lab"].astype(np.float32)))
    assert y.dim() == (4 if ds == "MNMS" else 3)


def test_composed_entry_runs_the_stages_in_the_reference_order(D):
    """Free-running: weak_augment equals the device's own scale-crop -> rotate(+flip) -> field -> warp."""
    g = load_golden("g16_augment_crop")
    B = 3
    img = torch.cat([img4(g["in_a_img"])] * B)
    lab = torch.cat([img4(g["in_a_lab"])] * B)
    s = D.AugmentSampler("fundus", 64, 11)
    r = s.batch(0, B)
    r[0, D.SC], r[0, D.ROT], r[0, D.EL] = 1, 1, 1                      # at least one sample with every gate on
    r[0, D.SC + 1:D.SC + 6] = [80, 90, 0, 7, 9]
    r[0, D.ROT + 4:D.ROT + 22] = D.rotate_words(-13, 64, 64)
    p = dev(r)
    wi, wl = D.weak_augment(img, lab, p, 64, 77)
    a = D.stage_scale_crop(img, lab, p, 64)
    b = D.stage_rotate(*a, p)
    f = D.stage_elastic_field(p, B, 64, 64, 77)
    c = D.stage_elastic_warp(*b, f, p)
    assert torch.equal(wi, c[0]) and torch.equal(wl, c[1])
    assert not torch.equal(c[0][0], b[0][0]) and not torch.equal(b[0][0], a[0][0]) and not torch.equal(a[0][0], img[0])


def test_gather(D):
    rs = np.random.RandomState(2)
    pool_i, pool_l = dev(rs.randint(0, 256, (9, 40, 40, 3)).astype(np.uint8)), dev(rs.randint(0, 256, (9, 40, 40, 1)).astype(np.uint8))
    idx = torch.tensor([8, 0, 3, 3, 5], dtype=torch.int32, device="cuda")
    gi, gl = D.stage_gather(pool_i, pool_l, idx)
    assert torch.equal(gi, pool_i[idx.long()]) and torch.equal(gl, pool_l[idx.long()])
    odd_i, odd_l = pool_i[:, :37, :39].contiguous(), pool_l[:, :37, :39].contiguous()      # sizes no multiple of 16 bytes
    gi, gl = D.stage_gather(odd_i, odd_l, idx)
    assert torch.equal(gi, odd_i[idx.long()]) and torch.equal(gl, odd_l[idx.long()])
