"""ustrun.functional.signed_dist2 / signed_distance_map (csrc/distmap.hip) and the wrappers utils.util.compute_sdf and
utils.metrics.distance_transform against tests/distmap_ref.py (pinned on the host by tests/test_distmap_ref_host.py) and the
g20 fixture.

The squared distances are integers: every comparison of them is bit equality.  The normalised map is compared with the float64
restatement within 2^-24 absolute.  Derivation: the kernel forms each pixel's quotient sqrt(d2) / sqrt(max d2) in float64 (error
of a few 2^-53, as the restatement's) and rounds it to float32 once; the quotient is at most 1 in magnitude, where a float32
ulp is at most 2^-24 and rounding to nearest moves a value by at most half of it, 2^-25; there is no subtraction, since one of
the map's two terms is 0 at every pixel.  2^-25 + 2^-50 < 2^-24.  (Three float32 roundings and a subtraction would have needed
7 * 2^-24.)"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import distmap_ref as R

pytestmark = pytest.mark.gpu

SDF_TOL = 2.0 ** -24


def _one(H, W, y, x):
    p = np.zeros((H, W), bool)
    p[y, x] = True
    return p


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (planes bool [N,K,H,W], s2 int32, flags int32, sdf float64): the inputs and the restatement's results, computed once"""
    rng = np.random.default_rng(2020)
    yy, xx = np.mgrid[:31, :70]
    c = {
        "1x1_foreground": np.ones((1, 1), bool),
        "1x1_background": np.zeros((1, 1), bool),
        "1x7": np.array([[0, 1, 1, 0, 0, 0, 1]], bool),
        "7x1": np.array([[0, 1, 1, 0, 0, 0, 1]], bool).T,
        "5x5_single_pixel": _one(5, 5, 1, 3),
        "5x5_all_but_one": ~_one(5, 5, 1, 3),
        "33x47_blobs": R.blobs(rng, 33, 47),                   # no multiple of 64 lanes, 4 rows per block or the 8-row column chunk
        "33x47_noisy_blobs": R.blobs(rng, 33, 47, flip=0.03),
        "64x130_blobs": R.blobs(rng, 64, 130),                 # W spans three lane chunks
        "9x1024_blobs": R.blobs(rng, 9, 1024, n=6),            # both limits
        "1024x3_blobs": R.blobs(rng, 1024, 3, n=6),
        "40x40_all_but_a_corner": ~_one(40, 40, 39, 39),       # the longest search: 39^2 + 39^2 from the opposite corner
        "checkerboard": (yy + xx) % 2 == 0,
    }
    c = {k: v[None, None] for k, v in c.items()}
    batch = np.stack([np.stack([R.blobs(rng, 33, 47), np.zeros((33, 47), bool)]),
                      np.stack([np.ones((33, 47), bool), R.blobs(rng, 33, 47, flip=0.02)]),
                      np.stack([~_one(33, 47, 0, 46), _one(33, 47, 32, 0)])])
    c["batch_3x2_empty_full_mixed"] = batch
    out = {}
    for k, p in c.items():
        s2, flags = R.signed_dist2_batch(p.astype(np.float32))
        sdf, _ = R.sdf_batch(p.astype(np.float32))
        out[k] = (p, s2, flags, sdf)
    return out


NAMES = ["1x1_foreground", "1x1_background", "1x7", "7x1", "5x5_single_pixel", "5x5_all_but_one", "33x47_blobs",
         "33x47_noisy_blobs", "64x130_blobs", "9x1024_blobs", "1024x3_blobs", "40x40_all_but_a_corner", "checkerboard",
         "batch_3x2_empty_full_mixed"]


def _dev(p):
    return torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).cuda()


def _report(name, got, want):
    bad = int((got != want).sum())
    print(name, tuple(want.shape), "differing pixels", bad, "of", want.size)
    return bad


@pytest.mark.parametrize("name", NAMES)
def test_signed_dist2_is_bit_equal(name):
    from ustrun import functional as F
    p, s2, flags, _ = cases()[name]
    got, gflags = F.signed_dist2(_dev(p))
    assert got.dtype == torch.int32 and gflags.dtype == torch.int32 and got.is_cuda and gflags.is_cuda
    assert got.shape == p.shape and gflags.shape == p.shape[:2]
    assert np.array_equal(gflags.cpu().numpy(), flags), (gflags.cpu().numpy(), flags)
    assert _report(name, got.cpu().numpy(), s2) == 0


def test_fixed_flags_and_values_of_the_smallest_planes():
    from ustrun import functional as F
    s2, flags = F.signed_dist2(_dev(cases()["1x1_foreground"][0]))
    assert flags.item() == F.PLANE_FULL and s2.item() == -F.DIST_NONE
    s2, flags = F.signed_dist2(_dev(cases()["1x1_background"][0]))
    assert flags.item() == F.PLANE_EMPTY and s2.item() == F.DIST_NONE
    s2, flags = F.signed_dist2(_dev(cases()["40x40_all_but_a_corner"][0]))
    assert flags.item() == F.PLANE_MIXED and s2[0, 0, 0, 0].item() == -2 * 39 * 39 and s2[0, 0, 39, 39].item() == 1
    s2, _ = F.signed_dist2(_dev(cases()["1x7"][0]))
    assert s2[0, 0, 0].tolist() == [1, -1, -1, 1, 4, 1, -1]


@pytest.mark.parametrize("dtype", [np.int64, np.float32])
def test_class_maps(dtype):
    from ustrun import functional as F
    rng = np.random.default_rng(5)
    m = np.zeros((3, 33, 47), np.int64)
    for n in range(2):                                   # sample 2 stays empty; 4 is a value above K: it belongs to no plane
        for c in (1, 2, 3, 4):
            m[n][R.blobs(rng, 33, 47, n=1)] = c
    m = m.astype(dtype)
    got, gflags = F.signed_dist2(torch.from_numpy(m).cuda(), by_class=True, num_classes=3)
    want, wflags = R.signed_dist2_batch(m, by_class=True, K=3)
    assert got.shape == (3, 3, 33, 47) and (m == 4).any() and (wflags[2] == R.EMPTY).all() and (wflags[:2] == R.MIXED).any()
    assert np.array_equal(gflags.cpu().numpy(), wflags) and _report("by_class", got.cpu().numpy(), want) == 0


def test_mask_values_outside_0_1_and_three_dimensional_masks():
    from ustrun import functional as F
    p, s2, flags, _ = cases()["batch_3x2_empty_full_mixed"]
    rng = np.random.default_rng(1)
    v = np.where(p, rng.choice([1.0, 0.25, -3.0, 1e-30, np.inf], p.shape), 0.0).astype(np.float32)          # binarised as x != 0
    got, gflags = F.signed_dist2(torch.from_numpy(v).cuda())
    assert np.array_equal(gflags.cpu().numpy(), flags) and np.array_equal(got.cpu().numpy(), s2)
    got3, _ = F.signed_dist2(_dev(p[:, 0]))              # [N,H,W]: one plane per sample
    assert got3.shape == (3, 1, 33, 47) and np.array_equal(got3.cpu().numpy()[:, 0], s2[:, 0])


def test_a_view_one_element_into_its_buffer():
    from ustrun import functional as F
    p, s2, flags, _ = cases()["33x47_blobs"]
    buf = torch.zeros(p.size + 1, device="cuda")
    buf[0] = 1.0
    buf[1:] = _dev(p).flatten()
    view = buf[1:].view(p.shape)
    assert view.data_ptr() == buf.data_ptr() + 4 and view.is_contiguous()
    got, gflags = F.signed_dist2(view)
    assert np.array_equal(got.cpu().numpy(), s2) and np.array_equal(gflags.cpu().numpy(), flags)
    lab = torch.zeros(p.size + 1, dtype=torch.int64, device="cuda")
    lab[1:] = torch.from_numpy(p.astype(np.int64)).cuda().flatten()
    got, _ = F.signed_dist2(lab[1:].view(1, 33, 47), by_class=True, num_classes=1)
    assert np.array_equal(got.cpu().numpy(), s2)


def test_g20_reference_fixture():
    from ustrun import functional as F
    for m, to_fg, to_bg, sdf in R.load_golden(R.GOLDEN):
        s2, flags = F.signed_dist2(_dev(m[None, None]))
        got, _ = F.signed_distance_map(_dev(m[None, None]))
        s2, got = s2.cpu().numpy()[0, 0], got.cpu().numpy()[0, 0]
        if m.any():
            assert flags.item() == R.MIXED and np.array_equal(s2, to_fg - to_bg)
        else:
            assert flags.item() == R.EMPTY and (s2 == R.DIST_NONE).all()
        err = float(np.abs(got.astype(np.float64) - sdf).max())
        print(m.shape, "max |sdf - reference|", err)
        assert err <= SDF_TOL and np.array_equal(got == 0, sdf == 0)


def test_two_calls_give_identical_bits():
    from ustrun import functional as F
    x = _dev(cases()["batch_3x2_empty_full_mixed"][0])
    a, fa = F.signed_dist2(x)
    b, fb = F.signed_dist2(x)
    sa, _ = F.signed_distance_map(x)
    sb, _ = F.signed_distance_map(x)
    assert torch.equal(a, b) and torch.equal(fa, fb) and torch.equal(sa, sb)


@pytest.mark.parametrize("name", NAMES)
def test_signed_distance_map_against_float64(name):
    from ustrun import functional as F
    p, s2, flags, sdf = cases()[name]
    got, gflags = F.signed_distance_map(_dev(p))
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == p.shape and not got.requires_grad
    got = got.cpu().numpy()
    assert np.array_equal(gflags.cpu().numpy(), flags)
    err = float(np.abs(got.astype(np.float64) - sdf).max())
    print(name, "max |sdf - float64|", err, "bound", SDF_TOL)
    assert err <= SDF_TOL
    assert (got[s2 == -1] == 0).all()                                        # the inner boundary, exactly
    for n in range(p.shape[0]):
        for k in range(p.shape[1]):
            if flags[n, k] == R.MIXED:                                       # the deepest pixels, exactly
                assert got[n, k].min() == -1.0 or (s2[n, k][p[n, k]] == -1).all()
                assert got[n, k].max() == 1.0
                assert (got[n, k][p[n, k]] <= 0).all() and (got[n, k][~p[n, k]] > 0).all()
            else:                                                            # empty and full planes, exactly
                assert not got[n, k].any()


def test_deepest_pixels_are_exactly_minus_one_and_one():
    from ustrun import functional as F
    p, s2, flags, sdf = cases()["33x47_blobs"]
    assert s2.min() < -1
    got, _ = F.signed_distance_map(_dev(p))
    got = got.cpu().numpy()
    assert got.min() == -1.0 and got.max() == 1.0
    assert np.array_equal(got == -1.0, s2 == s2.min()) and np.array_equal(got == 1.0, s2 == s2.max())


def test_compute_sdf_wrapper():
    from utils.util import compute_sdf
    p, s2, flags, sdf = cases()["batch_3x2_empty_full_mixed"]
    gt = (p[:, 1] * 7).astype(np.int16)                   # planes empty / mixed / mixed; any integer dtype, binarised as != 0
    for shape in ((3, 33, 47), (3, 1, 33, 47)):
        out = compute_sdf(gt, shape)
        assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == shape
        assert np.array_equal(out.reshape(3, 33, 47), sdf[:, 1])             # float64 of the exact integers: the restatement's values
        dev = compute_sdf(torch.from_numpy(gt).cuda(), shape)
        assert torch.is_tensor(dev) and dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == shape
        assert float(np.abs(dev.cpu().numpy().reshape(3, 33, 47) - sdf[:, 1]).max()) <= SDF_TOL
    assert compute_sdf(p[:, 1], (3, 33, 47)).dtype == np.float64             # bool in
    with pytest.raises(ValueError, match="sample 1"):
        compute_sdf(p[:, 0].astype(np.uint8), (3, 33, 47))                   # plane 0 of sample 1 is full
    assert not compute_sdf(torch.from_numpy(p[1:2, 0]).cuda(), (1, 33, 47)).any()         # tensor route: zeros, no exception


def test_distance_transform_wrapper():
    from utils.metrics import distance_transform
    p, s2, flags, _ = cases()["batch_3x2_empty_full_mixed"]
    for col in (0, 1):
        bitmap = p[:, col]
        want = np.where(s2[:, col] == R.DIST_NONE, np.inf, np.sqrt(np.maximum(s2[:, col], 0).astype(np.float64)))
        out = distance_transform(bitmap)
        assert out.dtype == np.float64 and out.shape == bitmap.shape and np.array_equal(out, want)
        dev = distance_transform(torch.from_numpy(bitmap).cuda())
        assert dev.is_cuda and dev.dtype == torch.float32 and np.array_equal(dev.cpu().numpy(), want.astype(np.float32))
    assert np.isinf(distance_transform(p[:, 1])[0]).all() and not distance_transform(p[:, 0])[1].any()     # empty: inf; full: 0


# ---- refusals: the message names the entry, and nothing is launched (the outputs keep their fill) ----

def _raw(H=8, W=8, N=1, K=1):
    from ustrun import _lib as L
    lib = L.lib()
    dev = "cuda"
    t = dict(mask=torch.ones(N * K * max(H, 1) * max(W, 1), device=dev), work=torch.zeros(1 << 16, dtype=torch.uint8, device=dev),
             s2=torch.full((N * K * 64,), 77, dtype=torch.int32, device=dev), flags=torch.full((N * K,), 77, dtype=torch.int32, device=dev),
             sdf=torch.full((N * K * 64,), 77.0, device=dev))
    return lib, t


def _err(lib):
    return lib.ustrun_last_error().decode()


def _untouched(t):
    torch.cuda.synchronize()
    return bool((t["s2"] == 77).all() and (t["flags"] == 77).all() and (t["sdf"] == 77.0).all())


@pytest.mark.parametrize("H,W", [(0, 8), (8, 0), (1025, 8), (8, 1025)])
def test_sizes_out_of_range_are_refused(H, W):
    from ustrun import functional as F
    lib, t = _raw()
    assert lib.ustrun_signed_dist2_work_bytes(1, 1, H, W) == -1 and "signed_dist2_work_bytes" in _err(lib) and "1024" in _err(lib)
    assert lib.ustrun_sdf_from_dist2_work_bytes(1, 1, H, W) == -1 and "sdf_from_dist2_work_bytes" in _err(lib)
    rc = lib.ustrun_signed_dist2(t["mask"].data_ptr(), 0, 1, 1, 0, H, W, t["work"].data_ptr(), 1 << 16, t["s2"].data_ptr(),
                                 t["flags"].data_ptr(), None)
    assert rc != 0 and _err(lib).startswith("signed_dist2:") and f"H {H} W {W}" in _err(lib)
    rc = lib.ustrun_sdf_from_dist2(t["s2"].data_ptr(), t["flags"].data_ptr(), 1, 1, H, W, t["work"].data_ptr(), 1 << 16,
                                   t["sdf"].data_ptr(), None)
    assert rc != 0 and _err(lib).startswith("sdf_from_dist2:") and f"H {H} W {W}" in _err(lib)
    assert _untouched(t)
    if H and W:
        with pytest.raises(RuntimeError, match="ustrun_signed_dist2_work_bytes.*1024"):
            F.signed_dist2(torch.zeros(1, 1, H, W, device="cuda"))
        with pytest.raises(RuntimeError, match="ustrun_signed_dist2_work_bytes.*1024"):
            F.signed_distance_map(torch.zeros(1, 1, H, W, device="cuda"))


def test_null_pointers_are_refused():
    lib, t = _raw()
    a = [t["mask"].data_ptr(), 0, 1, 1, 0, 8, 8, t["work"].data_ptr(), 1 << 16, t["s2"].data_ptr(), t["flags"].data_ptr(), None]
    for i in (0, 7, 9, 10):
        b = list(a)
        b[i] = None
        assert lib.ustrun_signed_dist2(*b) != 0 and "signed_dist2: null pointer" in _err(lib)
    a = [t["s2"].data_ptr(), t["flags"].data_ptr(), 1, 1, 8, 8, t["work"].data_ptr(), 1 << 16, t["sdf"].data_ptr(), None]
    for i in (0, 1, 6, 8):
        b = list(a)
        b[i] = None
        assert lib.ustrun_sdf_from_dist2(*b) != 0 and "sdf_from_dist2: null pointer" in _err(lib)
    assert _untouched(t)


def test_scratch_one_byte_short_is_refused():
    lib, t = _raw()
    need = lib.ustrun_signed_dist2_work_bytes(1, 1, 8, 8)
    assert need == 2 * 8 * 8 * 2
    rc = lib.ustrun_signed_dist2(t["mask"].data_ptr(), 0, 1, 1, 0, 8, 8, t["work"].data_ptr(), need - 1, t["s2"].data_ptr(),
                                 t["flags"].data_ptr(), None)
    assert rc != 0 and _err(lib) == f"signed_dist2: work buffer of {need - 1} bytes, needs {need}"
    need = lib.ustrun_sdf_from_dist2_work_bytes(1, 1, 8, 8)
    assert need == 16
    rc = lib.ustrun_sdf_from_dist2(t["s2"].data_ptr(), t["flags"].data_ptr(), 1, 1, 8, 8, t["work"].data_ptr(), need - 1,
                                   t["sdf"].data_ptr(), None)
    assert rc != 0 and _err(lib) == f"sdf_from_dist2: work buffer of {need - 1} bytes, needs {need}"
    assert _untouched(t)
    # with exactly the bytes asked for, both run
    assert lib.ustrun_signed_dist2(t["mask"].data_ptr(), 0, 1, 1, 0, 8, 8, t["work"].data_ptr(), 2 * 8 * 8 * 2, t["s2"].data_ptr(),
                                   t["flags"].data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert t["flags"].item() == 2 and (t["s2"] == -0x7fffffff).all()


def test_python_surface_refuses_what_it_cannot_read():
    from ustrun import functional as F
    with pytest.raises(RuntimeError, match="signed_dist2: mask must be"):
        F.signed_dist2(torch.zeros(1, 1, 8, 8))
    with pytest.raises(RuntimeError, match="signed_dist2: mask must be"):
        F.signed_dist2(torch.zeros(1, 1, 8, 8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="by_class"):
        F.signed_dist2(torch.zeros(1, 8, 8, dtype=torch.int64, device="cuda"), by_class=True)
    with pytest.raises(RuntimeError, match="by_class"):
        F.signed_dist2(torch.zeros(1, 8, 8, dtype=torch.int64, device="cuda"))
