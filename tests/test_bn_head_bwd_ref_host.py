"""CPU pin of tests/bn_head_bwd_ref.py (the float64 references of tests/test_gpu_bn_head_bwd_ops.py) against torch's float64 autograd:
F.batch_norm(training=True) -> relu (-> max_pool2d(2)) for the BatchNorm backward, F.conv2d with a 1x1 weight and bias for the head --
odd extents, the dp-only case, planted ties and K in {1, 3, 8} included.  It also runs the input generator of every GPU case in all four
storage types and asserts what the GPU tests rely on: both margins hold with no element left out, the planted ties are exact and reach
every pair of window positions."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_head_bwd_ref as R

TIGHT = dict(rtol=1e-12, atol=1e-13)       # float64 against float64: only the order of a few operations differs


def nchw(a):           # numpy NHWC -> torch NCHW float64
    return torch.from_numpy(np.ascontiguousarray(a)).double().permute(0, 3, 1, 2).contiguous()


def nhwc(t):           # torch NCHW -> numpy NHWC
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def test_torch_max_pool_keeps_the_first_maximum():
    """what the planted-tie comparisons below rest on"""
    for vals, first in (([1.0, 1.0, 1.0, 1.0], 0), ([0.0, 2.0, 2.0, 1.0], 1), ([2.0, 1.0, 1.0, 2.0], 0), ([0.0, 0.0, 3.0, 3.0], 2)):
        x = torch.tensor(vals, dtype=torch.float64).view(1, 1, 2, 2).requires_grad_(True)
        F.max_pool2d(x, 2).sum().backward()
        want = [1.0 if i == first else 0.0 for i in range(4)]
        assert x.grad.flatten().tolist() == want, (vals, x.grad)
        got = R.F.routed(np.ones((1, 1, 1, 1)), np.array(vals).reshape(1, 2, 2, 1))
        assert got.flatten().tolist() == want


def autograd_bn(y, da, dp, gamma, beta, eps=1e-5):
    """float64 autograd through batch_norm(training) -> relu (-> max_pool2d): dy, dgamma, dbeta and the statistics used"""
    yt = nchw(y).requires_grad_(True)
    g, b = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
    act = torch.relu(F.batch_norm(yt, None, None, g, b, True, 0.0, eps))
    obj = 0.0
    if da is not None:
        obj = obj + (act * nchw(da)).sum()
    if dp is not None:
        obj = obj + (F.max_pool2d(act, 2) * nchw(dp)).sum()
    obj.backward()
    flat = y.reshape(-1, y.shape[3])
    mean, rstd = flat.mean(0), 1.0 / np.sqrt(flat.var(0) + eps)
    return nhwc(yt.grad), g.grad.numpy(), b.grad.numpy(), mean, rstd


BN_HOST = [(2, 4, 6, 5), (3, 5, 7, 4), (1, 2, 2, 8), (2, 6, 3, 3), (1, 3, 3, 2)]


@pytest.mark.parametrize("n,h,w,c,mode", [s + (m,) for s in BN_HOST for m in ("da", "da+dp", "dp")] + [(2, 1, 1, 4, "da"), (1, 1, 3, 4, "da")])
def test_bn_backward_equals_autograd(n, h, w, c, mode):
    """dz -> sums -> finalize -> apply with the batch statistics of y itself is autograd's gradient with respect to y, gamma and beta;
    every window holds a planted tie pattern (bn_head_bwd_ref.plant_ties), the dp-only case and odd extents included."""
    rng = np.random.default_rng(100 * h + 10 * w + c)
    y = rng.normal(size=(n, h, w, c)) * 2 + 0.5
    gamma = (1 + 0.3 * rng.normal(size=c)) * rng.choice([-1.0, 1.0], size=c)
    beta = 0.3 * rng.normal(size=c)
    flat = y.reshape(-1, c)
    if mode != "da":       # ties in the normalised activation: planted through the constants of the y as drawn, then taken as they fall
        s0 = gamma / np.sqrt(flat.var(0) + 1e-5)
        R.plant_ties(y, s0, beta - flat.mean(0) * s0, rng, "f32")
    da = rng.normal(size=(n, h, w, c)) if "da" in mode else None
    dp = rng.normal(size=(n, h // 2, w // 2, c)) if "dp" in mode else None
    dy, dg, db, mean, rstd = autograd_bn(y, da, dp, gamma, beta)
    scale = gamma * rstd
    shift = beta - mean * scale
    z, zero, gap = R.dz(da, dp, y, scale, shift)
    assert zero > 0 and gap > 0
    s1, s2 = R.bn_bwd_sums(z, y)
    dgamma, dbeta, coef = R.bn_bwd_finalize(s1, s2, n * h * w, gamma, mean, rstd)
    np.testing.assert_allclose(dbeta, db, **TIGHT)
    np.testing.assert_allclose(dgamma, dg, **TIGHT)
    np.testing.assert_allclose(R.bn_bwd_apply(z, y, coef), dy, **TIGHT)
    m1, m2 = R.bn_bwd_sums_magnitude(z, y)
    assert (m1 >= np.abs(s1)).all() and (m2 >= np.abs(s2) * (1 - 1e-15)).all()
    assert (R.bn_bwd_apply_magnitude(z, y, coef) >= np.abs(R.bn_bwd_apply(z, y, coef)) * (1 - 1e-15)).all()
    if dp is not None:     # same y in one channel -> the same normalised activation: the planted ties survive batch_norm
        win = np.stack(R._quads(np.maximum(y * scale + shift, 0.0)))
        assert ((win == win.max(0)).sum(0) > 1).any()


def test_dz_routes_to_the_first_maximum_and_skips_hanging_windows():
    y = np.zeros((1, 3, 3, 1))
    y[0, :, :, 0] = [[1.0, 2.0, 9.0], [2.0, 2.0, 9.0], [9.0, 9.0, 9.0]]
    dp = np.full((1, 1, 1, 1), 5.0)
    z, _, gap = R.dz(None, dp, y, [1.0], [0.0])
    want = np.zeros((3, 3))
    want[0, 1] = 5.0                                   # the first of the three 2.0; row 2 and column 2 belong to no window
    assert np.array_equal(z[0, :, :, 0], want) and gap == 1.0 / 3.0
    z, _, _ = R.dz(np.ones_like(y), dp, y, [-1.0], [0.5])         # all four activations <= 0: routed to position 0, then masked
    assert not z.any()
    z, zero, gap = R.dz(np.ones_like(y), dp, y, [0.0], [1.0])       # the all-ones mask: a four-way tie goes to position 0
    assert z[0, 0, 0, 0] == 6.0 and z.sum() == 14.0 and zero == 1.0 and gap == np.inf


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("n,h,w,c", [(1, 1, 1, 4), (3, 5, 7, 12)])
def test_head_equals_conv2d(n, h, w, c, k, affine):
    rng = np.random.default_rng(10 * c + k)
    y = rng.normal(size=(n, h, w, c))
    s, b = R.B_table(rng, c) if affine else (None, None)
    wt, bias, dl = rng.normal(size=(k, c)), rng.normal(size=k), rng.normal(size=(n, k, h, w))
    a = torch.from_numpy(R.head_act(y, s, b)).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    if affine:
        assert (a >= 0).all() and (a == 0).any()
    else:
        assert (a < 0).any()
    wq, bq = torch.from_numpy(wt).view(k, c, 1, 1).requires_grad_(True), torch.from_numpy(bias).requires_grad_(True)
    out = F.conv2d(a, wq, bq)
    out.backward(torch.from_numpy(dl))
    np.testing.assert_allclose(R.head_fwd(y, s, b, wt, bias), out.detach().numpy(), **TIGHT)
    da, dw, db = R.head_bwd(dl, y, s, b, wt)
    np.testing.assert_allclose(da, nhwc(a.grad), **TIGHT)
    np.testing.assert_allclose(dw, wq.grad.view(k, c).numpy(), **TIGHT)
    np.testing.assert_allclose(db, bq.grad.numpy(), **TIGHT)
    maw, mw = R.head_fwd_magnitude(y, s, b, wt)
    assert (maw >= np.abs(R.head_fwd(y, s, b, wt, np.zeros(k))) * (1 - 1e-15)).all() and ((mw > 0) == affine).all()
    mda, mdw, mdwa, mdb = R.head_bwd_magnitude(dl, y, s, b, wt)
    assert (mda >= np.abs(da) * (1 - 1e-15)).all() and (mdw >= np.abs(dw) * (1 - 1e-15)).all() and (mdb >= np.abs(db)).all()
    assert ((mdwa > 0) == affine).all()


def test_finalize_rows_sums_the_table():
    stat, count, gamma, mean, rstd, _, _ = R.finalize_stat_case(7, 8, 2, 16)
    assert np.isnan(mean[8:16]).all() and abs(mean[R.HI] * rstd[R.HI]) == pytest.approx(1e3, rel=1e-6)
    dg, db, coef = R.finalize_rows(stat[1], count, gamma, mean[16:24], rstd[16:24])
    s1 = stat[1, :, 0].astype(np.float64).sum(0)
    np.testing.assert_allclose(db, s1, **TIGHT)
    assert coef[0, R.G0] == 0 and coef[1, R.G0] == 0 and coef[2, R.G0] == 0 and coef[0, R.GNEG] < 0


def test_storage_rounding_in_numpy_equals_torch():
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.normal(size=4096) * 10.0 ** rng.integers(-6, 4, size=4096), [0.0, 1.0, 1.00390625, 1.01171875]])
    for name, tdt in (("f32", torch.float32), ("bf16", torch.bfloat16), ("f16", torch.float16)):
        want = torch.from_numpy(a).to(torch.float32).to(tdt).double().numpy() if name == "bf16" else torch.from_numpy(a).to(tdt).double().numpy()
        got = R.rounded(a, name)
        assert np.array_equal(got, want), name
        away = np.where(got < 0, -1.0, 1.0) * R.spacing(got, name)  # one spacing further from zero is the next value of the type
        assert (np.abs(R.rounded(got + away, name)) > np.abs(got)).all() and np.array_equal(R.rounded(got + 0.49 * away, name), got), name


@pytest.mark.parametrize("name", R.TYPES)
@pytest.mark.parametrize("n,c,h,w,pooled", R.BN_SHAPES)
def test_gpu_case_generators_meet_the_margins(n, c, h, w, pooled, name):
    """Every BatchNorm-backward case of the GPU file: the settling loop terminates, both margins hold over ALL elements, the values are
    of the storage type, and (pooled) the planted ties are exact, the maximum's tie reaches every pair of positions -- (0, 3) across
    smaller values included -- and some window has all four activations <= 0."""
    k = R.bn_case(name, n, c, h, w, pooled)
    z, zero, gap = R.dz(k["da"], k["dp"], k["y"], k["scale"], k["shift"])
    assert zero >= R.MARGIN and gap >= R.MARGIN and k["rounds"] <= R.ROUNDS
    for v in ("y", "da") + (("dp",) if pooled else ()):
        assert np.array_equal(k[v], R.rounded(k[v], name))
    if not pooled:
        return
    a = np.maximum(k["y"] * k["scale"] + k["shift"], 0.0)
    win, pat = np.stack(R._quads(a)), k["pattern"]
    top = win.max(0)
    for p, (i, j) in enumerate(R.PAIRS):
        sel = pat == p
        assert sel.any(), p
        others = [q for q in range(4) if q not in (i, j)]
        assert (win[i][sel] == top[sel]).all() and (win[j][sel] == top[sel]).all() and (top[sel] > 0).all(), p
        assert all((win[q][sel] < top[sel]).all() for q in others), p
        assert (R.winners(k["y"], k["scale"], k["shift"])[sel] == i).all()
    assert (pat == 6).any() and (top[pat == 6] == 0).all()
    if pat.size >= 64:
        assert set(np.unique(R.winners(k["y"], k["scale"], k["shift"])).tolist()) == {0, 1, 2, 3}
    zd, _, _ = R.dz(None, k["dp"], k["y"], k["scale"], k["shift"])          # dp alone: the same margins, by construction
    assert np.abs(zd).sum() > 0


@pytest.mark.parametrize("name", R.TYPES)
@pytest.mark.parametrize("n,c,h,w,pooled", R.MASK_ALL_SHAPES)
def test_gpu_case_generators_mask_all_ones(n, c, h, w, pooled, name):
    k = R.bn_case(name, n, c, h, w, pooled, mask_all=True)
    z, zero, gap = R.dz(k["da"], k["dp"], k["y"], k["scale"], k["shift"])
    assert zero == 1.0 and gap == np.inf
    if pooled:
        assert (R.winners(k["y"], k["scale"], k["shift"]) == 0).all()
    assert (z != 0).mean() > 0.99


def test_plans_restate_the_launchers():
    """the figures the shapes' comments in bn_head_bwd_ref.BN_SHAPES claim"""
    p = R.bn_bwd_plan("f32", 1, 4, 1, 1, False)
    assert (p["G"], p["PL"], p["blocks"], p["T"]) == (1, 256, 1, 1)
    p = R.bn_bwd_plan("f32", 3, 24, 9, 7, False)
    assert (p["G"], p["PL"], p["blocks"], p["T"]) == (8, 32, 1, 6)
    p = R.bn_bwd_plan("bf16", 3, 64, 9, 7, False)
    assert p["x8"] and (p["G"], p["PL"], p["blocks"], p["T"]) == (8, 32, 1, 6)
    assert not R.bn_bwd_plan("bf16", 3, 64, 9, 7, False, four=True)["x8"] and not R.bn_bwd_plan("f16", 2, 96, 8, 8, False)["x8"]
    p = R.bn_bwd_plan("f16", 2, 2048, 3, 5, False)
    assert p["x8"] and (p["G"], p["PL"], p["blocks"], p["T"]) == (256, 1, 4, 8)
    p = R.bn_bwd_plan("f32", 1, 1032, 4, 6, True)
    assert (p["G"], p["PL"], p["T"]) == (256, 1, 24) and p["even"]
    assert R.bn_bwd_plan("bf16", 2, 64, 11, 15, True)["code"] == 0x424E0000 | 2 << 4 | 2
    assert R.head_plan(189, 64) == (16, 16, 1, 12) and R.head_plan(189, 264) == (64, 4, 3, 16) and R.head_plan(1, 4) == (1, 256, 1, 1)
