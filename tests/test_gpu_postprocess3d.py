"""ustrun.functional.post_process_3d (ustrun_post_process_3d: cavities filled, small 26-connected components removed, largest
component kept, per VOLUME on the device) against tests/postprocess3d_ref.py and the reference's own results in the g22 fixture.
Everything is integer work on a unique partition: every comparison is exact, at every voxel of every volume.

A labelling fault shows only through the filter, so every shape runs under several shares -- (1, 5) is the reference's, (1, 1) keeps
a volume only if it is ONE component, None shows the filling alone -- and under largest-only, each with the filling on and off.
The shapes are the smallest where the kernel can still go wrong: 5 x 19 x 70 has two tile rows and two tile columns, neither a
multiple of the 16 x 64 tile, and interior and face slices; 3 x 16 x 64 is exactly one tile, 2 x 17 x 65 one pixel past it; and one
batch has more slices (N K D = 67584) than a grid's y extent or the folded tile grid holds.

None of this exists on the parent commit: there the symbol and the function are missing and every test here fails."""
import functools
import os

import numpy as np
import pytest
import torch

import postprocess3d_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_postprocess3d.npz")
SIZES = [(5, 19, 70), (3, 16, 64), (2, 17, 65), (1, 1, 1), (1, 5, 5)]
RULES = [((1, 5), False), ((1, 2), False), ((1, 1), False), (None, False), (None, True)]          # (share, largest)
TILE_H, TILE_W = 16, 64


def shapes(D, H, W):
    zz, yy, xx = np.mgrid[:D, :H, :W]
    s = {"empty": np.zeros((D, H, W), bool), "full": np.ones((D, H, W), bool)}
    rng = np.random.default_rng((D * 1000 + H) * 1000 + W)
    for density in (0.15, 0.3, 0.5):
        s["random_%d" % round(density * 100)] = rng.random((D, H, W)) < density
    s["checkerboard"] = (zz + yy + xx) % 2 == 1          # everything connects under 26-connectivity
    for name, a, b, A, B in (("tube_z", yy, xx, H, W), ("tube_y", zz, xx, D, W), ("tube_x", zz, yy, D, H)):
        inside = (a >= 1) & (b >= 1) & (a <= A - 2) & (b <= B - 2)
        s[name] = inside & ((a == 1) | (b == 1) | (a == A - 2) | (b == B - 2))     # a ring in every cross-section, open at both ends
    depth = np.minimum.reduce([zz, yy, xx, D - 1 - zz, H - 1 - yy, W - 1 - xx])
    s["nested_shells"] = depth % 2 == 1
    box = depth == 0                                     # a closed box around the whole interior, one voxel inside
    if min(D, H, W) > 2:
        box[D // 2, H // 2, W // 2] = True
    s["closed_box"] = box
    plane = (yy % 2 == 0) | (xx == np.where((yy // 2) % 2 == 1, 0, W - 1))
    link = np.where((zz // 2) % 2 == 1, (yy == 0) & (xx == 0), (yy == H - 1) & (xx == W - 1))
    s["serpentine"] = np.where(zz % 2 == 0, plane, link)     # the plane serpentine in every other slice, joined at alternating corners
    spiral = np.zeros((D, H, W), bool)                   # a broken row per slice that moves round, joined by edges and corners
    for z in range(D):
        y = (3 * z) % H
        spiral[z, y, z % 2:] = (np.arange(z % 2, W) // 3 + z) % 2 == 0
        spiral[z, (y + 1) % H, (7 * z) % W] = True
    s["spiral"] = spiral
    corner = np.zeros((D, H, W), bool)                   # voxels that touch only by a corner across a tile corner and a slice
    for z in range(D):
        for y, x in ((TILE_H - 1 + (z & 1), TILE_W - 1 + (z & 1)), (TILE_H - (z & 1), TILE_W - 1 + (z & 1)), (1 + (z & 1), 1 + (z & 1))):
            if y < H and x < W:
                corner[z, y, x] = True
    corner[D - 1, H - 1, W - 1] = True
    s["corner_touch"] = corner
    five = np.zeros((D, H, W), bool)
    if H >= 4 and W >= 17:
        for k in range(5):
            five[0, 1:3, 1 + 3 * k:3 + 3 * k] = True
    s["five_squares"] = five
    s["five_squares_plus_one"] = five.copy()
    s["five_squares_plus_one"][D - 1, H - 1, W - 1] = five.any()
    return s


@functools.lru_cache(maxsize=None)
def _shape_batch(D, H, W):
    s = shapes(D, H, W)
    return tuple(s), np.stack(list(s.values()))


@functools.lru_cache(maxsize=None)
def _labelled(D, H, W, fill):
    """every shape's filled volume and its components, computed once and shared by all rules"""
    out = []
    for p in _shape_batch(D, H, W)[1]:
        f = R.fill(p) if fill else p
        out.append((f, R.components(f)))
    return out


def _run(vols, **kw):
    from ustrun import functional as F
    out = F.post_process_3d(torch.from_numpy(np.ascontiguousarray(vols, dtype=np.float32)).cuda(), **kw)
    assert out.dtype == torch.float32 and out.is_cuda
    return out.cpu().numpy()


@pytest.mark.parametrize("fill", [True, False])
@pytest.mark.parametrize("D,H,W", SIZES)
def test_shapes_equal_the_flood_fill(D, H, W, fill):
    names, batch = _shape_batch(D, H, W)
    for share, largest in RULES:
        got = _run(batch[:, None], fill_holes=fill, min_share=share, largest=largest)
        assert got.shape == (len(names), 1, D, H, W)
        for k, name in enumerate(names):
            f, comps = _labelled(D, H, W, fill)[k]
            want = R.select(f, comps, share, largest)
            print(D, H, W, fill, share, largest, name, "components", len(comps), "gained", int(f.sum() - batch[k].sum()),
                  "kept", int(want.sum()), "differing voxels", int((got[k, 0] != want).sum()))
            assert np.array_equal(got[k, 0], want.astype(np.float32)), (name, fill, share, largest)


def test_all_three_regimes_occur():
    """many components, a few, hardly more than one; no cavity, a few, many: the random volumes of 5 x 19 x 70 cover them"""
    names, _ = _shape_batch(5, 19, 70)
    comps = [len(_labelled(5, 19, 70, True)[names.index("random_%d" % d)][1]) for d in (15, 30, 50)]
    holes = [int(_labelled(5, 19, 70, True)[names.index("random_%d" % d)][0].sum() - _shape_batch(5, 19, 70)[1][names.index("random_%d" % d)].sum())
             for d in (15, 30, 50)]
    print("components", comps, "hole voxels", holes)
    assert comps[0] > 20 > comps[1] > comps[2] >= 1 and holes[0] == 0 and holes[2] > 10


@functools.lru_cache(maxsize=None)
def _long_columns():
    """six volumes of 1024 x 3 x 5 and, per filling, their labelled forms"""
    D, H, W = 1024, 3, 5
    zz, yy, xx = np.mgrid[:D, :H, :W]
    rng = np.random.default_rng(1024)
    rim = (yy != 1) | (xx == 0) | (xx == W - 1)
    capped = rim | (zz == 0) | (zz == D - 1)
    capped[D // 2, 1, 2] = True                            # a voxel inside the cavity: its own component until the cavity is filled
    vols = [rng.random((D, H, W)) < 0.3, rng.random((D, H, W)) < 0.6, rim, capped,
            (zz % 2 == 0) & ((xx + yy) % 2 == 0) | (zz % 2 == 1) & (yy == 1) & (xx == (zz // 2) % 2 * 2 + 1),
            (zz + yy + xx) % 2 == 0]
    lab = {}
    for fill in (True, False):
        fs = [R.fill(p) if fill else p for p in vols]
        lab[fill] = [(f, R.components(f)) for f in fs]
    return np.stack(vols), lab


@pytest.mark.parametrize("fill", [True, False])
def test_more_slices_than_a_grid_extent(fill):
    """2 x 33 volumes of 1024 x 3 x 5: 67584 slices, one tile each -- past 65535 and past the folded tile grid, so blocks walk
    more than one tile; six different volumes take turns, so a slice or a volume read from its neighbour's place shows."""
    vols, lab = _long_columns()
    N, K = 2, 33
    pick = np.arange(N * K) % len(vols)
    batch = vols[pick].reshape(N, K, *vols.shape[1:])
    assert N * K * vols.shape[1] > 65535
    assert int(lab[True][3][0].sum() - vols[3].sum()) == 3 * 1022 - 1 and int(lab[True][2][0].sum()) == int(vols[2].sum())
    x = torch.from_numpy(batch.astype(np.float32)).cuda()
    from ustrun import functional as F
    for share, largest in RULES:
        got = F.post_process_3d(x, fill_holes=fill, min_share=share, largest=largest).cpu().numpy().reshape(N * K, *vols.shape[1:])
        want = [R.select(f, comps, share, largest).astype(np.float32) for f, comps in lab[fill]]
        for v in range(N * K):
            assert np.array_equal(got[v], want[pick[v]]), (v, fill, share, largest)


def test_g22_reference_fixture():
    for inp, out in R.load_golden(GOLDEN):
        got = _run(inp[:, None])
        assert np.array_equal(got[:, 0], out.astype(np.float32)), inp.shape


@pytest.mark.parametrize("N,K", [(1, 1), (3, 2), (2, 3)])
def test_volume_batches(N, K):
    rng = np.random.default_rng(10 * N + K)
    p = rng.random((N, K, 4, 17, 65)) < np.array([0.15, 0.3, 0.5, 0.6])[rng.integers(0, 4, (N, K, 1, 1, 1))]
    v = p.astype(np.float32) * rng.choice([1.0, 0.25, -3.0], p.shape).astype(np.float32)         # binarised as x != 0
    assert np.array_equal(_run(v), R.process_batch(v))
    assert np.array_equal(_run(v, largest=True), R.process_batch(v, largest=True))
    if K == 1:
        assert np.array_equal(_run(v[:, 0]), R.process_batch(v))                                 # [N,D,H,W] is K = 1


@pytest.mark.parametrize("dtype", [np.int64, np.float32])
@pytest.mark.parametrize("K", [1, 3])
def test_class_maps(K, dtype):
    from ustrun import functional as F
    rng = np.random.default_rng(K)
    m = (rng.integers(0, K + 2, (2, 4, 20, 70)) * (rng.random((2, 4, 20, 70)) < 0.7)).astype(dtype)   # K + 1 belongs to no part
    got = F.post_process_3d(torch.from_numpy(m).cuda(), by_class=True, n_classes=K).cpu().numpy()
    assert got.shape == (2, K, 4, 20, 70) and (m == K + 1).any()
    assert np.array_equal(got, R.process_batch(m, True, K))
    plain = F.post_process_3d(torch.from_numpy(m).cuda(), by_class=True, n_classes=K, fill_holes=False, min_share=None).cpu().numpy()
    assert np.array_equal(plain, R.volumes(m, True, K).astype(np.float32))


def test_the_plain_decode():
    _, batch = _shape_batch(5, 19, 70)
    assert np.array_equal(_run(batch[:, None], fill_holes=False, min_share=None)[:, 0], batch.astype(np.float32))
    assert np.array_equal(_run(batch[:, None], fill_holes=False, min_share=(0, 1))[:, 0], batch.astype(np.float32))


def test_the_result_does_not_depend_on_the_pruning_of_z_pairs():
    from ustrun import _lib as L
    from ustrun import functional as F
    _, batch = _shape_batch(5, 19, 70)
    x = torch.from_numpy(batch[:, None].astype(np.float32)).cuda()
    a = F.post_process_3d(x, min_share=(1, 2), largest=True)
    old = L.lib().ustrun_debug_flags2(128)                 # every z-pair unites
    try:
        b = F.post_process_3d(x, min_share=(1, 2), largest=True)
    finally:
        L.lib().ustrun_debug_flags2(old)
    assert torch.equal(a, b)


def test_two_calls_give_equal_bits_and_a_side_stream_the_same_result():
    from ustrun import functional as F
    _, batch = _shape_batch(5, 19, 70)
    x = torch.from_numpy(batch[:, None].astype(np.float32)).cuda()
    a, b = F.post_process_3d(x, largest=True), F.post_process_3d(x, largest=True)
    assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = F.post_process_3d(x, largest=True)
        junk = torch.zeros(1 << 20, device="cuda")      # other work queued behind it on the same stream
        for _ in range(4):
            junk = junk * 1.5 + 1.0
    side.synchronize()
    assert torch.equal(a, c)


def test_errors_name_the_entry_point():
    from ustrun import _lib as L
    from ustrun import functional as F
    lib = L.lib()
    assert lib.ustrun_pack_conv_elems_dtype(8, 8, 9, L.F16) > 0             # the calling thread used the IEEE-half build last:
                                                                            # the message must still come from the build that failed
    with pytest.raises(RuntimeError, match="ustrun_post_process_3d_work_bytes.*1\\.\\.1024.*D 1025"):
        F.post_process_3d(torch.zeros(1, 1, 1025, 2, 2, device="cuda"))
    for args, msg in (((1, 1, 1024, 1024, 129), "exceed 2\\^27"), ((32768, 1, 1, 1, 1), "N \\* K <= 32767"), ((1, 1, 0, 4, 4), "D 0")):
        assert lib.ustrun_post_process_3d_work_bytes(*args) == -1
        with pytest.raises(RuntimeError, match="post_process_3d_work_bytes.*" + msg):
            L.check(1, "ustrun_post_process_3d_work_bytes")
    x = torch.zeros(1, 1, 3, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="ustrun_post_process_3d.*share_den"):
        F.post_process_3d(x, min_share=(1, 0))
    with pytest.raises(RuntimeError, match="ustrun_post_process_3d.*share_num"):
        F.post_process_3d(x, min_share=(-1, 5))
    with pytest.raises(RuntimeError, match="post_process_3d: pred .* must be"):
        F.post_process_3d(torch.zeros(3, 8, 8, device="cuda"))
    with pytest.raises(RuntimeError, match="post_process_3d: pred .* must be"):
        F.post_process_3d(x, by_class=True)
    with pytest.raises(RuntimeError, match="float32 or int64 HIP tensor"):
        F.post_process_3d(x.cpu())
    # the C entry itself: null pointers, a short and a misaligned work buffer, a misaligned out -- refused before any launch
    nb = lib.ustrun_post_process_3d_work_bytes(1, 1, 3, 8, 8)
    work, out = torch.zeros(nb + 16, dtype=torch.uint8, device="cuda"), torch.full((3 * 8 * 8 + 1,), 7.0, device="cuda")
    call = lambda p, w, n, o: lib.ustrun_post_process_3d(p, 0, 1, 1, 0, 3, 8, 8, 1, 1, 5, 0, w, n, o, None)
    for bad, msg in (((None, work.data_ptr(), nb, out.data_ptr()), "null pointer"), ((x.data_ptr(), None, nb, out.data_ptr()), "null pointer"),
                     ((x.data_ptr(), work.data_ptr(), nb, None), "null pointer"),
                     ((x.data_ptr(), work.data_ptr(), nb - 1, out.data_ptr()), "work buffer of %d bytes, needs %d" % (nb - 1, nb)),
                     ((x.data_ptr(), work.data_ptr() + 8, nb, out.data_ptr()), "16-byte"),
                     ((x.data_ptr(), work.data_ptr(), nb, out.data_ptr() + 2), "4-byte aligned")):
        assert call(*bad) != 0
        with pytest.raises(RuntimeError, match="post_process_3d: .*" + msg):
            L.check(1, "ustrun_post_process_3d")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                        # nothing was launched
    assert call(x.data_ptr(), work.data_ptr(), nb, out.data_ptr()) == 0
