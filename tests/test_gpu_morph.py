"""The chamfer-distance and binary-morphology kernels (csrc/morph.hip: ustrun_chamfer_dist, ustrun_morph) and the Python surface
on top of them (ustrun.functional.chamfer_distance / distance_transform_cdt / binary_* / boundary_band,
dataloaders.custom_transforms.GetBoundary) against tests/morph_ref.py, which tests/test_morph_ref_host.py pins to scipy.ndimage and
to a brute force, and against the reference's own GetBoundary outputs (tests/golden/g23_morph.npz).

Everything is integers: every comparison is equality at every element.  The shapes are the ones at which the kernels can go
wrong -- single rows and columns, rows of one, two and five 64-pixel chunks with a ragged end, more rows than a block's four
waves, volumes of one slice -- not workload shapes; each case sends all its calls before it reads any result back."""
import functools

import numpy as np
import pytest
import torch

import morph_ref as M

pytestmark = pytest.mark.gpu

DENSITIES = (0.0, 0.03, 0.3, 0.9, 1.0)
WIDTHS = (1, 2, 3, 5, 300)
PLANES = ((1, 1), (1, 7), (7, 1), (9, 13), (64, 64), (65, 130), (33, 257))
VOLUMES = ((1, 5, 6), (2, 9, 4), (5, 6, 7), (3, 65, 70), (17, 33, 40))
METRIC_NAMES = {M.L1: "taxicab", M.LINF: "chessboard"}


def _dev(p):
    return torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).cuda()


def _corners(box):
    out = []
    for c in np.ndindex(*(2,) * len(box)):
        p = np.zeros(box, bool)
        p[tuple((n - 1) * b for n, b in zip(box, c))] = True
        out.append(p)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def batches(box):
    """name -> bool parts [N,K,*box]: the five densities and one more random part as N * K = 3 * 2; one pixel in each corner as
    [2^rank,1]; one part alone, N * K = 1"""
    rng = np.random.default_rng(hash(box) % 1000 + 31)
    six = np.stack([rng.random(box) < d for d in DENSITIES + (0.5,)]).reshape((3, 2) + box)
    return {"densities_3x2": six, "corners": _corners(box)[:, None], "single_1x1": (rng.random(box) < 0.3)[None, None]}


class Ref:
    """the unclipped distances of one batch, formed once: every op at every width is a threshold of them (morph_ref's identities)"""

    def __init__(self, parts, rank):
        self.parts, self.rank = parts, rank
        self.d = functools.lru_cache(maxsize=None)(self._d)

    def _d(self, metric, kind, outside):
        return M.dist_sep(self.parts if kind == 0 else ~self.parts, metric, self.rank, outside)

    def morph(self, metric, op, w, b):
        dil, ero = self.d(metric, 0, b == 1) <= w, self.d(metric, 1, b == 0) > w
        if op == M.DILATE:
            return dil
        if op == M.ERODE:
            return ero
        if op == M.BAND:
            return dil & ~ero
        if op == M.OPEN:
            return M.dist_sep(ero, metric, self.rank, b == 1) <= w
        return M.dist_sep(dil == 0, metric, self.rank, b == 0) > w

    def chamfer(self, metric, outside):
        d_fg, d_bg = self.d(metric, 0, outside == 2), self.d(metric, 1, outside == 1)
        d_fg, d_bg = np.where(d_fg >= M.INF, M.DIST_NONE, d_fg), np.where(d_bg >= M.INF, M.DIST_NONE, d_bg)
        return np.where(self.parts, -d_bg, d_fg)

    def flags(self):
        ax = tuple(range(2, self.parts.ndim))
        return np.where(self.parts.any(ax), np.where((~self.parts).any(ax), 1, 2), 0)


def _run_batch(parts, rank, widths=WIDTHS, ops=(M.DILATE, M.ERODE, M.OPEN, M.CLOSE, M.BAND), mask=None, **kw):
    """all chamfer codes and all op x width x metric x border x reduce combinations of one batch; returns the differing elements"""
    from ustrun import functional as F
    ref = Ref(parts, rank)
    mask = _dev(parts) if mask is None else mask
    got, want, names = [], [], []
    for metric in (M.L1, M.LINF):
        for outside in (0, 1, 2):
            sd, flags = F.chamfer_distance(mask, METRIC_NAMES[metric], outside, **kw)
            assert sd.dtype == torch.int32 and flags.dtype == torch.int32 and sd.is_cuda and tuple(sd.shape) == parts.shape
            if metric == M.LINF and outside == 0:
                first_linf = len(got)
            got += [sd.flatten(), flags.flatten()]
            want += [ref.chamfer(metric, outside).ravel(), ref.flags().ravel()]
            names += [f"chamfer m{metric} o{outside}", f"flags m{metric} o{outside}"]
        for op in ops:
            for w in widths:
                for b in (0, 1):
                    r = ref.morph(metric, op, w, b)
                    for reduce in (0, 1):
                        o = F._morph(mask, op, metric, w, b, reduce, kw.get("by_class", False), kw.get("num_classes"), "test")
                        assert o.dtype == torch.uint8 and tuple(o.shape) == ((parts.shape[0],) + parts.shape[2:] if reduce else parts.shape)
                        if (metric, op, w, b, reduce) == (M.L1, M.BAND, widths[0], 0, 1):
                            first_band = len(got)
                        got.append(o.flatten().to(torch.int32))
                        want.append((r.any(1) if reduce else r).ravel())
                        names.append(f"op{op} w{w} m{metric} b{b} reduce{reduce}")
    # a second call gives identical bits
    sd2, _ = F.chamfer_distance(mask, "chessboard", 0, **kw)
    again = F._morph(mask, M.BAND, M.L1, widths[0], 0, 1, kw.get("by_class", False), kw.get("num_classes"), "test")
    same = torch.equal(sd2.flatten(), got[first_linf]) and torch.equal(again.flatten().to(torch.int32), got[first_band])
    sizes = [g.numel() for g in got]
    flat = torch.cat([g.to(torch.int32) for g in got]).cpu().numpy()
    bad, at = [], 0
    for n, w, name in zip(sizes, want, names):
        diff = int((flat[at:at + n] != w.astype(np.int64)).sum())
        if diff:
            bad.append((name, diff, n))
        at += n
    print(parts.shape, len(names), "results,", len(bad), "differ", bad[:8])
    assert same
    return bad


@pytest.mark.parametrize("box", PLANES, ids=lambda b: "x".join(map(str, b)))
def test_planes_every_op_width_metric_border(box):
    for name, parts in batches(box).items():
        full = name == "densities_3x2"
        bad = _run_batch(parts, 2, WIDTHS if full else (1, 300), (M.DILATE, M.ERODE, M.OPEN, M.CLOSE, M.BAND) if full else (M.CLOSE, M.BAND))
        assert not bad, (name, bad[:8])


@pytest.mark.parametrize("box", VOLUMES, ids=lambda b: "x".join(map(str, b)))
def test_volumes_every_op_width_metric_border(box):
    for name, parts in batches(box).items():
        full = name == "densities_3x2"
        bad = _run_batch(parts, 3, WIDTHS if full else (1, 300), (M.DILATE, M.ERODE, M.OPEN, M.CLOSE, M.BAND) if full else (M.OPEN, M.BAND))
        assert not bad, (name, bad[:8])


@pytest.mark.parametrize("dtype", [torch.int64, torch.float32], ids=["int64", "float32"])
@pytest.mark.parametrize("box", [(9, 13), (65, 130), (5, 6, 7)], ids=lambda b: "x".join(map(str, b)))
def test_class_maps(box, dtype):
    rng = np.random.default_rng(7)
    cmap = rng.integers(0, 4, (3,) + box)                # classes 1 and 2 are the parts, 0 and 3 belong to neither
    parts = M.decode(cmap, True, 2)
    bad = _run_batch(parts, len(box), (1, 3), (M.ERODE, M.CLOSE, M.BAND), mask=torch.from_numpy(cmap).to(dtype).cuda(), by_class=True,
                     num_classes=2)
    assert not bad, bad[:8]


def test_one_slice_volume_is_not_a_plane():
    """rank 3 with D = 1: every voxel is 1 from the outside along z; rank 2: the slice axis is no axis"""
    from ustrun import functional as F
    p = np.ones((1, 1, 1, 6, 7), bool)
    sd3, _ = F.chamfer_distance(_dev(p), "taxicab", 1)
    sd2, _ = F.chamfer_distance(_dev(p[:, :, 0]), "taxicab", 1)
    assert (sd3.cpu().numpy() == -1).all()
    assert np.array_equal(sd2.cpu().numpy(), M.chamfer(p[:, :, 0], M.L1, 2, 1)[0]) and sd2.min().item() == -3
    assert not F.binary_erosion(_dev(p)).any().item() and F.binary_erosion(_dev(p[:, :, 0])).any().item()


def test_grid_fold_past_65535_slices():
    """N * K = 300 volumes of 250 slices: 75000 slices, more than a grid's y extent holds; six distinct volumes repeated"""
    from ustrun import functional as F
    rng = np.random.default_rng(11)
    six = np.stack([rng.random((250, 8, 8)) < d for d in (0.0, 0.002, 0.03, 0.3, 0.97, 1.0)])
    ref = Ref(six[:, None], 3)
    mask = _dev(six).repeat(50, 1, 1, 1).view(150, 2, 250, 8, 8)
    for metric in (M.L1, M.LINF):
        sd, flags = F.chamfer_distance(mask, METRIC_NAMES[metric], 0)
        band = F._morph(mask, M.BAND, metric, 2, 0, 0, False, None, "test")
        closed = F._morph(mask, M.CLOSE, metric, 1, 1, 1, False, None, "test")
        sd, flags, band, closed = sd.cpu().numpy(), flags.cpu().numpy(), band.cpu().numpy(), closed.cpu().numpy()
        want = ref.chamfer(metric, 0)[:, 0]
        assert np.array_equal(sd.reshape(50, 6, 250, 8, 8), np.broadcast_to(want, (50,) + want.shape))
        assert np.array_equal(flags.reshape(50, 6), np.broadcast_to(ref.flags()[:, 0], (50, 6)))
        want = ref.morph(metric, M.BAND, 2, 0)[:, 0]
        assert np.array_equal(band.reshape(50, 6, 250, 8, 8), np.broadcast_to(want, (50,) + want.shape))
        want = ref.morph(metric, M.CLOSE, 1, 1)[:, 0].reshape(3, 2, 250, 8, 8).any(1)
        assert np.array_equal(closed.reshape(50, 3, 250, 8, 8), np.broadcast_to(want, (50,) + want.shape))


def test_python_surface_types_and_errors():
    from ustrun import functional as F
    rng = np.random.default_rng(3)
    p = rng.random((2, 2, 9, 13)) < 0.4
    v = rng.random((1, 2, 4, 5, 6)) < 0.4
    for parts, rank in ((p, 2), (v, 3)):
        m = _dev(parts)
        for fn, op in ((F.binary_dilation, M.DILATE), (F.binary_erosion, M.ERODE), (F.binary_opening, M.OPEN), (F.binary_closing, M.CLOSE)):
            for structure, metric in ((None, M.L1), (1, M.L1), ("cross", M.L1), (rank, M.LINF), ("full", M.LINF)):
                out = fn(m, structure, 2, 1)
                assert out.dtype == torch.bool and out.is_cuda
                assert np.array_equal(out.cpu().numpy(), M.morph(parts, metric, rank, op, 2, 1))
        assert np.array_equal(F.binary_dilation(m, iterations=100000).cpu().numpy(), M.morph(parts, M.L1, rank, M.DILATE, 100000))
        band = F.boundary_band(m, 2, "full")
        assert band.dtype == torch.uint8 and np.array_equal(band.cpu().numpy(), M.band(parts, M.LINF, rank, 2).any(1))
        for metric, name in ((M.L1, "taxicab"), (M.LINF, "chessboard")):
            cdt = F.distance_transform_cdt(m, name)
            assert cdt.dtype == torch.int32
            for n in range(parts.shape[0]):
                for k in range(parts.shape[1]):
                    assert np.array_equal(cdt[n, k].cpu().numpy(), M.distance_transform_cdt(parts[n, k], metric, rank))
    full = F.distance_transform_cdt(_dev(np.ones((1, 2, 3, 4), bool)))
    assert (full.cpu().numpy() == -1).all()
    mixed = np.stack([np.ones((3, 4), bool), np.eye(3, 4, dtype=bool)])[None]
    got = F.distance_transform_cdt(_dev(mixed)).cpu().numpy()
    assert (got[0, 0] == -1).all() and np.array_equal(got[0, 1], M.distance_transform_cdt(mixed[0, 1], M.LINF, 2))
    with pytest.raises(RuntimeError, match="connectivity 2"):
        F.binary_dilation(_dev(v), structure=2)
    for bad in (3, "ball", np.ones((3, 3)), 0, True):
        with pytest.raises(RuntimeError, match="structure"):
            F.binary_erosion(_dev(p), structure=bad)
    with pytest.raises(RuntimeError, match="iterations"):
        F.binary_dilation(_dev(p), iterations=0)
    with pytest.raises(RuntimeError, match="border_value"):
        F.binary_dilation(_dev(p), border_value=2)
    with pytest.raises(RuntimeError, match="metric"):
        F.chamfer_distance(_dev(p), "euclidean")
    with pytest.raises(RuntimeError, match="outside"):
        F.chamfer_distance(_dev(p), "taxicab", 3)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        F.binary_dilation(torch.zeros(1, 1, 4, 4))


def test_every_refusal_launches_nothing():
    from ustrun import _lib as L
    lib = L.lib()
    N, K, H, W = 2, 2, 9, 13
    mask = _dev(np.random.default_rng(5).random((N, K, H, W)) < 0.3)
    nb = lib.ustrun_morph_work_bytes(N, K, 2, 1, H, W, M.CLOSE)
    nbc = lib.ustrun_chamfer_dist_work_bytes(N, K, 2, 1, H, W)
    assert nb > 0 and nbc > 0 and nb % 16 == 0 and nbc % 16 == 0
    work = torch.full((nb + 16,), 0x5a, dtype=torch.uint8, device="cuda")
    out = torch.full((N, K, H, W), 7, dtype=torch.uint8, device="cuda")
    sd = torch.full((N, K, H, W), 7, dtype=torch.int32, device="cuda")
    flags = torch.full((N, K), 7, dtype=torch.int32, device="cuda")
    s = None

    def morph(mask_p=mask.data_ptr(), n=N, k=K, rank=2, d=1, h=H, w=W, metric=0, op=0, width=1, border=0, work_p=work.data_ptr(),
              work_bytes=nb, out_p=out.data_ptr()):
        return lib.ustrun_morph(mask_p, 0, n, k, 0, rank, d, h, w, metric, op, width, border, 0, work_p, work_bytes, out_p, s)

    def chamfer(mask_p=mask.data_ptr(), n=N, k=K, rank=2, d=1, h=H, w=W, metric=0, outside=0, work_p=work.data_ptr(), work_bytes=nbc,
                sd_p=sd.data_ptr(), flags_p=flags.data_ptr()):
        return lib.ustrun_chamfer_dist(mask_p, 0, n, k, 0, rank, d, h, w, metric, outside, work_p, work_bytes, sd_p, flags_p, s)

    refused = [
        (morph, dict(rank=1), b"rank"), (morph, dict(rank=4), b"rank"), (morph, dict(d=2), b"D must be 1"),
        (morph, dict(h=0), b"1..1024"), (morph, dict(w=1025), b"1..1024"), (morph, dict(rank=3, d=1025), b"1..1024"),
        (morph, dict(n=0), b"N, K > 0"), (morph, dict(n=32768, k=1), b"32767"), (morph, dict(rank=3, d=1024, h=1024, w=1024), b"2^27"),
        (morph, dict(width=0), b"width"), (morph, dict(width=-3), b"width"), (morph, dict(width=4096), b"width"),
        (morph, dict(metric=2), b"metric"), (morph, dict(metric=-1), b"metric"), (morph, dict(op=5), b"op"), (morph, dict(op=-1), b"op"),
        (morph, dict(border=2), b"border_value"), (morph, dict(mask_p=None), b"null"), (morph, dict(work_p=None), b"null"),
        (morph, dict(out_p=None), b"null"), (morph, dict(op=M.CLOSE, work_bytes=nb - 1), b"needs"), (morph, dict(work_bytes=0), b"needs"),
        (morph, dict(work_p=work.data_ptr() + 8), b"aligned"),
        (chamfer, dict(rank=0), b"rank"), (chamfer, dict(d=3), b"D must be 1"), (chamfer, dict(h=2000), b"1..1024"),
        (chamfer, dict(k=20000), b"32767"), (chamfer, dict(metric=7), b"metric"), (chamfer, dict(outside=3), b"outside"),
        (chamfer, dict(outside=-1), b"outside"), (chamfer, dict(mask_p=None), b"null"), (chamfer, dict(sd_p=None), b"null"),
        (chamfer, dict(flags_p=None), b"null"), (chamfer, dict(work_p=None), b"null"), (chamfer, dict(work_bytes=nbc - 16), b"needs"),
        (chamfer, dict(work_p=work.data_ptr() + 4), b"aligned"), (chamfer, dict(sd_p=sd.data_ptr() + 2), b"aligned"),
    ]
    for fn, kw, word in refused:
        assert fn(**kw) != 0, kw
        assert word in lib.ustrun_last_error(), (kw, lib.ustrun_last_error())
    for args, word in (((N, K, 5, 1, H, W, 0), b"rank"), ((N, K, 2, 2, H, W, 0), b"D must be 1"), ((N, K, 2, 1, H, 4000, 0), b"1..1024"),
                       ((N, K, 2, 1, H, W, 9), b"op")):
        assert lib.ustrun_morph_work_bytes(*args) == -1 and word in lib.ustrun_last_error()
        if args[-1] == 0:
            assert lib.ustrun_chamfer_dist_work_bytes(*args[:-1]) == -1 and word in lib.ustrun_last_error()
    torch.cuda.synchronize()
    assert (work == 0x5a).all().item() and (out == 7).all().item() and (sd == 7).all().item() and (flags == 7).all().item()
    assert morph(op=M.CLOSE) == 0 and chamfer() == 0          # and the same arguments, unspoilt, are accepted
    torch.cuda.synchronize()
    assert out.max().item() <= 1 and sd.abs().max().item() < 30 and flags.max().item() <= 2


def test_get_boundary_equals_the_reference_goldens(golden):
    from dataloaders.custom_transforms import GetBoundary
    g = golden("g23_morph")
    names = [str(n) for n in g["names"]]
    by_shape = {}
    for name in names:
        by_shape.setdefault(g[f"{name}_mask"].shape, []).append(name)
    assert len(names) >= 5 and len(by_shape) == 2
    for w in (1, 3, 5):
        for name in names:                               # numpy in, the reference's numpy array out
            got = GetBoundary(width=w)(g[f"{name}_mask"])
            assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, g[f"{name}_w{w}"]), (name, w)
        for shape, group in by_shape.items():            # a device batch [N,K,H,W] in, [N,H,W] on the device out
            batch = torch.from_numpy(np.stack([g[f"{n}_mask"].transpose(2, 0, 1) for n in group]).astype(np.float32)).cuda()
            got = GetBoundary(width=w)(batch)
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (len(group),) + shape[:2]
            assert np.array_equal(got.cpu().numpy(), np.stack([g[f"{n}_w{w}"] for n in group])), (shape, w)
    assert GetBoundary().width == 5
