"""ustrun.functional.post_process (ustrun_post_process: holes filled, small 8-connected components removed, on the device)
against tests/postprocess_ref.py and the reference's own results in the g18 fixture.  Everything is integer work on a unique
partition: every comparison is exact, at every pixel of every plane.

A labelling fault shows only through the filter, so every shape runs under several shares: (1, 5) is the reference's, (1, 1) keeps a
plane only if it is ONE component (any split empties it, any wrong merge keeps what must go), and None shows the filling alone."""
import functools
import os

import numpy as np
import pytest
import torch

import postprocess_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_postprocess.npz")
SIZES = [(1, 1), (1, 37), (37, 1), (16, 16), (17, 23), (33, 65), (64, 64), (96, 136), (130, 70)]
SHARES = [(1, 5), (1, 2), (1, 1), None]


def _blobs(rng, H, W, flip):
    yy, xx = np.mgrid[:H, :W]
    p = np.zeros((H, W), bool)
    for _ in range(3):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(1, max(2, max(H, W) // 3))
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        p |= (d2 <= r * r) & (d2 >= (r // 2) ** 2)
    return p ^ (rng.random((H, W)) < flip)


def _spiral(H, W):
    """one-pixel-wide square spiral, its arms two pixels apart: one component, one long chain through every tile"""
    p = np.zeros((H, W), bool)
    y0, x0, y1, x1 = 0, 0, H - 1, W - 1
    while y0 <= y1 and x0 <= x1:
        p[y0, x0:x1 + 1] = True
        p[y0:y1 + 1, x1] = True
        if y1 - y0 < 2 or x1 - x0 < 2:
            break
        p[y1, x0 + 2:x1 + 1] = True
        p[y0 + 2:y1 + 1, x0 + 2] = True
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
        p[y0, x0] = True
    return p


def shapes(H, W):
    yy, xx = np.mgrid[:H, :W]
    s = {"empty": np.zeros((H, W), bool), "full": np.ones((H, W), bool)}
    s["checkerboard"] = (yy + xx) % 2 == 1               # one 8-connected component; every interior background pixel its own hole
    s["serpentine"] = (yy % 2 == 0) | (xx == np.where((yy // 2) % 2 == 1, 0, W - 1))
    s["comb"] = (yy == 0) | (xx % 2 == 0)
    s["spiral"] = _spiral(H, W)
    bars = np.zeros((H, W), bool)                        # bars separated by ONE background column, on every 8th column (any tile edge)
    bars[1:H - 1, 1:W - 1] = True
    bars[:, 8::8] = False
    s["bars_one_column_apart"] = bars
    b = min(H, W) - 2
    for closed in (0, 1):                                # a box that leaks through a one-pixel gap; the same with the gap closed diagonally
        p = np.zeros((H, W), bool)
        if b >= 4:
            p[1, 1:b + 1] = p[b, 1:b + 1] = True
            p[1:b + 1, 1] = p[1:b + 1, b] = True
            p[1, b // 2] = False
            if closed:
                p[0, :] = True
                p[0, b // 2 + 1] = False
        s["gap_closed" if closed else "gap_open"] = p
    d = np.maximum(abs(yy - H // 2), abs(xx - W // 2))
    s["nested_rings"] = (d % 4 == 1) & (d < min(H, W) // 2)
    five = np.zeros((H, W), bool)
    if H >= 4 and W >= 17:
        for k in range(5):
            five[1:3, 1 + 3 * k:3 + 3 * k] = True
    s["five_squares"] = five
    s["five_squares_plus_one"] = five.copy()
    s["five_squares_plus_one"][H - 1, W - 1] = five.any()
    rng = np.random.default_rng(H * 1000 + W)
    for flip in (0.0, 0.02, 0.3):
        s["blobs_%d" % round(flip * 100)] = _blobs(rng, H, W, flip)
    return s


def corner_pairs(H, W):
    """Pairs of pixels that touch only diagonally across every crossing of the 8-pixel grid (so across every tile corner, whatever
    the tile), both diagonals in turn -> (plane, number of pairs).  Under share (1, pairs) every pair stays exactly when it is ONE
    component of two pixels."""
    p = np.zeros((H, W), bool)
    n = 0
    for a in range(1, (H - 1) // 8 + 1):
        for b in range(1, (W - 1) // 8 + 1):
            y, x = 8 * a, 8 * b
            if (a + b) % 2:
                p[y - 1, x - 1] = p[y, x] = True
            else:
                p[y - 1, x] = p[y, x - 1] = True
            n += 1
    return p, n


@functools.lru_cache(maxsize=None)
def _shape_batch(H, W):
    s = shapes(H, W)
    return tuple(s), np.stack(list(s.values()))


def _run(planes, **kw):
    from ustrun import functional as F
    out = F.post_process(torch.from_numpy(np.ascontiguousarray(planes, dtype=np.float32)).cuda(), **kw)
    assert out.dtype == torch.float32 and out.is_cuda
    return out.cpu().numpy()


@pytest.mark.parametrize("H,W", SIZES)
def test_shapes_equal_the_flood_fill(H, W):
    names, batch = _shape_batch(H, W)
    for share in SHARES:
        got = _run(batch[:, None], min_share=share)
        assert got.shape == (len(names), 1, H, W)
        for k, name in enumerate(names):
            want = R.process(batch[k], True, share)
            diff = int((got[k, 0] != want).sum())
            print(H, W, share, name, "foreground", int(want.sum()), "differing pixels", diff)
            assert np.array_equal(got[k, 0], want.astype(np.float32)), (name, share)


@pytest.mark.parametrize("H,W", [s for s in SIZES if min(s) > 8])
def test_diagonal_touch_across_every_grid_corner_is_one_component(H, W):
    p, n = corner_pairs(H, W)
    got = _run(p[None, None], fill_holes=False, min_share=(1, n))
    assert p.sum() == 2 * n and np.array_equal(got[0, 0], p.astype(np.float32))       # a split pair (2 x one pixel) would be removed
    if n > 1:                                            # one notch stricter and every pair goes: the threshold is live
        assert not _run(p[None, None], fill_holes=False, min_share=(1, n - 1)).any()
    assert np.array_equal(got[0, 0], R.process(p, False, (1, n)).astype(np.float32))


def test_256():
    H = W = 256
    rng = np.random.default_rng(256)
    batch = np.stack([_spiral(H, W), _blobs(rng, H, W, 0.02), shapes(H, W)["serpentine"]])
    for share in ((1, 5), (1, 1)):
        got = _run(batch[:, None], min_share=share)
        for k in range(len(batch)):
            assert np.array_equal(got[k, 0], R.process(batch[k], True, share).astype(np.float32)), (k, share)


def test_g18_reference_fixture():
    for inp, out in R.load_golden(GOLDEN):
        got = _run(inp[:, None])
        assert np.array_equal(got[:, 0], out.astype(np.float32)), inp.shape


@pytest.mark.parametrize("N,K", [(1, 1), (3, 2), (5, 3)])
def test_plane_batches(N, K):
    rng = np.random.default_rng(10 * N + K)
    p = np.stack([np.stack([_blobs(rng, 33, 65, (0.0, 0.02, 0.3)[(n + k) % 3]) for k in range(K)]) for n in range(N)])
    v = p.astype(np.float32) * rng.choice([1.0, 0.25, -3.0], p.shape).astype(np.float32)         # binarised as x != 0
    assert np.array_equal(_run(v), R.process_batch(v))


@pytest.mark.parametrize("dtype", [np.int64, np.float32])
@pytest.mark.parametrize("K", [1, 3])
def test_class_maps(K, dtype):
    from ustrun import functional as F
    rng = np.random.default_rng(K)
    m = np.zeros((3, 40, 72), np.int64)
    for n in range(3):
        for c in range(1, K + 2):                        # K + 1 is a value above K: it belongs to no part
            m[n][_blobs(rng, 40, 72, 0.01)] = c
    m = m.astype(dtype)
    got = F.post_process(torch.from_numpy(m).cuda(), by_class=True, n_classes=K).cpu().numpy()
    assert got.shape == (3, K, 40, 72) and (m == K + 1).any()
    assert np.array_equal(got, R.process_batch(m, True, K))
    plain = F.post_process(torch.from_numpy(m).cuda(), by_class=True, n_classes=K, fill_holes=False, min_share=None).cpu().numpy()
    assert np.array_equal(plain, R.planes(m, True, K).astype(np.float32))


def test_switches():
    names, batch = _shape_batch(33, 65)
    for fill, share in ((False, (1, 5)), (True, None), (False, None), (True, (1, 2)), (True, (1, 1)), (False, (1, 1))):
        got = _run(batch[:, None], fill_holes=fill, min_share=share)
        want = np.stack([R.process(p, fill, share) for p in batch]).astype(np.float32)
        assert np.array_equal(got[:, 0], want), (fill, share)
    assert np.array_equal(_run(batch[:, None], fill_holes=False, min_share=None)[:, 0], batch.astype(np.float32))   # the plain decode


def test_two_calls_give_equal_bits_and_a_side_stream_the_same_result():
    from ustrun import functional as F
    names, batch = _shape_batch(96, 136)
    x = torch.from_numpy(batch[:, None].astype(np.float32)).cuda()
    a, b = F.post_process(x), F.post_process(x)
    assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = F.post_process(x)
        junk = torch.zeros(1 << 20, device="cuda")      # other work queued behind it on the same stream
        for _ in range(4):
            junk = junk * 1.5 + 1.0
    side.synchronize()
    assert torch.equal(a, c)


def test_errors_name_the_entry_point():
    from ustrun import _lib as L
    from ustrun import functional as F
    assert L.lib().ustrun_pack_conv_elems_dtype(8, 8, 9, L.F16) > 0         # the calling thread used the IEEE-half build last:
                                                                            # the message must still come from the build that failed
    with pytest.raises(RuntimeError, match="ustrun_post_process_work_bytes.*1025"):
        F.post_process(torch.zeros(1, 1, 1025, 4, device="cuda"))
    with pytest.raises(RuntimeError, match="ustrun_post_process.*share_den"):
        F.post_process(torch.zeros(1, 1, 8, 8, device="cuda"), min_share=(1, 0))
    with pytest.raises(RuntimeError, match="ustrun_post_process.*share_num"):
        F.post_process(torch.zeros(1, 1, 8, 8, device="cuda"), min_share=(-1, 5))
