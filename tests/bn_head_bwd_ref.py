"""Float64 restatement, in plain numpy, of the BatchNorm + ReLU (+ MaxPool2d(2) routing) backward in train mode (csrc/bn.hip, kernels in
csrc/bn_bwd.h) and of the 1x1 classification head (csrc/head.hip), as include/ustrun.h documents them, for
tests/test_gpu_bn_head_bwd_ops.py.  No GPU, no torch, nothing from oracle/.  tests/test_bn_head_bwd_ref_host.py pins every function to
torch's float64 autograd on the CPU.

Layouts are the kernels': NHWC activations [N, H, W, C], NCHW logits / dlogits [N, K, H, W], coef[3][C] (coef[pass][3][C] for several
passes), statistics rows [pass][rows][2][C].  Every function converts what it is given to float64 and never modifies it.

The second half holds the INPUT GENERATORS of the GPU tests (rounding to a storage type in numpy, the planted arg-max ties, and the
loop that moves pre-activations away from the ReLU's kink and window values away from each other), here so that the host test can run
them without a GPU.
"""
import math

import numpy as np

import bn_ops_ref as B
import frozen_bn_ref as F

TYPES = ("f32", "f32x3", "bf16", "f16")
MARGIN = 4 * 2.0 ** -22          # what both margins of dz() must reach, in units of |y scale| + |shift|


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _quads(a):
    """the four positions (0,0) (0,1) (1,0) (1,1) of every COMPLETE 2x2 window of a [N, H, W, C]: four views [N, H//2, W//2, C]"""
    hp, wp = a.shape[1] // 2, a.shape[2] // 2
    return [a[:, (q >> 1):2 * hp:2, (q & 1):2 * wp:2] for q in range(4)]


# ---- BatchNorm + ReLU (+ pool) backward ------------------------------------------------------------------------------------------------
def margins(y, scale, shift, pooled):
    """(zero, gap), both in units of the f32 evaluation's error scale |y scale| + |shift|:
    zero: the smallest |y scale + shift| over elements where it is not 0;
    gap:  the smallest difference between a window's maximum of relu(.) and a DIFFERENT value of the window, over the sum of the two
          elements' scales (an element with a <= 0 counts 0: its relu is exactly 0 once `zero` holds).  inf where there is none."""
    y, s, b = _f64(y), _f64(scale), _f64(shift)
    a = y * s + b
    mag = np.abs(y * s) + np.abs(b)
    nz = a != 0
    zero = float((np.abs(a[nz]) / mag[nz]).min()) if nz.any() else math.inf
    gap = math.inf
    if pooled and y.shape[1] >= 2 and y.shape[2] >= 2:
        r = np.stack(_quads(np.maximum(a, 0.0)))
        m = np.stack(_quads(np.where(a > 0, mag, 0.0)))
        top = r.max(axis=0)
        mtop = np.where(r == top, m, 0.0).max(axis=0)
        diff = r != top
        if diff.any():
            gap = float(((top - r)[diff] / (mtop + m)[diff]).min())
    return zero, gap


def dz(da, dp, y, scale, shift):
    """a = relu(y scale + shift); dp [N, H//2, W//2, C] goes to the FIRST maximum of a over each complete 2x2 window in the order (0,0)
    (0,1) (1,0) (1,1) (frozen_bn_ref.routed), windows that hang over an odd edge take none; dz = (da + routed) [a > 0].  da or dp may
    be None.  -> (dz, zero margin, gap margin) (see margins())"""
    y, s, b = _f64(y), _f64(scale), _f64(shift)
    a = y * s + b
    g = np.zeros_like(y) if da is None else _f64(da).copy()
    if dp is not None:
        g = g + F.routed(_f64(dp), a)
    zero, gap = margins(y, s, b, dp is not None)
    return g * (a > 0), zero, gap


def bn_bwd_sums(dz_, y):
    """-> sum dz, sum dz y per channel"""
    dz_, y = _f64(dz_), _f64(y)
    return dz_.sum((0, 1, 2)), (dz_ * y).sum((0, 1, 2))


def bn_bwd_sums_magnitude(dz_, y):
    """-> sum |dz|, sum |dz y| per channel: what the rounding errors of the two sums are proportional to"""
    dz_, y = _f64(dz_), _f64(y)
    return np.abs(dz_).sum((0, 1, 2)), np.abs(dz_ * y).sum((0, 1, 2))


def bn_bwd_finalize(s1, s2, count, gamma, mean, rstd):
    """bn_bwd_finalize_kernel: dbeta = s1, dgamma = rstd (s2 - mean s1), c0 = gamma rstd, c1 = -c0 (dgamma / count) rstd,
    c2 = -c0 (dbeta / count) - c1 mean.  -> dgamma [C], dbeta [C], coef [3, C]"""
    s1, s2, gamma, mean, rstd = (_f64(v) for v in (s1, s2, gamma, mean, rstd))
    count = float(count)
    dbeta = s1
    dgamma = rstd * (s2 - mean * s1)
    c0 = gamma * rstd
    c1 = -c0 * (dgamma / count) * rstd
    c2 = -c0 * (dbeta / count) - c1 * mean
    return dgamma, dbeta, np.stack([c0, c1, c2])


def bn_bwd_apply(dz_, y, coef):
    """dy = c0 dz + c1 y + c2"""
    c = _f64(coef)
    return c[0] * _f64(dz_) + c[1] * _f64(y) + c[2]


def bn_bwd_apply_magnitude(dz_, y, coef):
    """|c0 dz| + |c1 y| + |c2|"""
    c = _f64(coef)
    return np.abs(c[0] * _f64(dz_)) + np.abs(c[1] * _f64(y)) + np.abs(c[2])


def finalize_rows(stat, count, gamma, mean, rstd):
    """ustrun_bn_bwd_finalize_stat on one pass's rows [rows, 2, C]: the columns summed exactly (bn_ops_ref.stat_sums), then
    bn_bwd_finalize"""
    s1, s2 = B.stat_sums(stat)
    return bn_bwd_finalize(s1, s2, count, gamma, mean, rstd)


# ---- 1x1 head --------------------------------------------------------------------------------------------------------------------------
def head_act(y, scale, shift):
    """the head's input: relu(y scale + shift), or y itself (NO ReLU) when scale is None"""
    return B.act(y, scale, shift, relu=scale is not None)


def head_fwd(y, scale, shift, w, bias):
    """logits [N, K, H, W] = sum_c a[n, h, w, c] w[k, c] + bias[k]"""
    return np.einsum("nhwc,kc->nkhw", head_act(y, scale, shift), _f64(w)) + _f64(bias)[None, :, None, None]


def head_fwd_magnitude(y, scale, shift, w):
    """-> sum_c |a w| and sum_c |w| (|y scale| + |shift|), both [N, K, H, W]"""
    w = np.abs(_f64(w))
    return (np.einsum("nhwc,kc->nkhw", np.abs(head_act(y, scale, shift)), w),
            np.einsum("nhwc,kc->nkhw", B.act_magnitude(y, scale, shift), w))


def head_bwd(dl, y, scale, shift, w):
    """da [N, H, W, C] = sum_k dl[n, k, h, w] w[k, c] (the gradient of the ACTIVATED input: no mask), dw [K, C] = sum_p dl a, db [K] =
    sum_p dl"""
    dl = _f64(dl)
    return (np.einsum("nkhw,kc->nhwc", dl, _f64(w)), np.einsum("nkhw,nhwc->kc", dl, head_act(y, scale, shift)), dl.sum((0, 2, 3)))


def head_bwd_magnitude(dl, y, scale, shift, w):
    """-> sum_k |dl w| [N, H, W, C], sum_p |dl a| [K, C], sum_p |dl| (|y scale| + |shift|) [K, C], sum_p |dl| [K]"""
    dl = np.abs(_f64(dl))
    return (np.einsum("nkhw,kc->nhwc", dl, np.abs(_f64(w))), np.einsum("nkhw,nhwc->kc", dl, np.abs(head_act(y, scale, shift))),
            np.einsum("nkhw,nhwc->kc", dl, B.act_magnitude(y, scale, shift)), dl.sum((0, 2, 3)))


# ---- the storage types, in numpy -------------------------------------------------------------------------------------------------------
def rounded(a, name):
    """a rounded to nearest-even in the storage type of `name`, as float64"""
    a = _f64(a)
    if name in ("f32", "f32x3"):
        return a.astype(np.float32).astype(np.float64)
    if name == "f16":
        return a.astype(np.float16).astype(np.float64)
    x = np.ascontiguousarray(a.astype(np.float32)).view(np.uint32)
    x = (x + (((x >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    return x.view(np.float32).astype(np.float64)


def spacing(a, name):
    """the distance from |a| to the next larger value of the storage type"""
    a = np.abs(_f64(a))
    if name in ("f32", "f32x3"):
        return np.spacing(a.astype(np.float32)).astype(np.float64)
    if name == "f16":
        return np.spacing(a.astype(np.float16)).astype(np.float64)
    _, e = np.frexp(np.maximum(a, 2.0 ** -126))
    return np.ldexp(1.0, e - 1 - 7)


def f32(a):
    return rounded(a, "f32")


# ---- input generators ------------------------------------------------------------------------------------------------------------------
# (n, c, h, w, pooled): the smallest shapes that reach each path of bn_bwd_plan / bn_bwd_stream4 / bn_bwd_stream8
BN_SHAPES = [
    (1, 4, 1, 1, False),        # G = 1, one window, 255 idle pixel lanes in the fold
    (3, 24, 9, 7, False),       # G = 8 with two idle group lanes; 189 windows over 2 blocks: a four-window trip plus a remainder per lane
    (3, 64, 9, 7, False),       # 16-bit: the 8-channel kernels (G8 = 8), main trip + remainder
    (2, 96, 8, 8, False),       # 12 octets, not a power of two -> the 4-channel kernels for 16-bit
    (2, 2048, 3, 5, False),     # G8 = 256: one pixel lane per block
    (1, 1032, 3, 5, False),     # two channel rounds
    (1, 1032, 4, 6, True),      # two channel rounds, pooled
    (2, 64, 12, 16, True),      # EVEN
    (2, 8, 2, 2, True),         # EVEN, one window per image
    (2, 64, 11, 15, True),      # general form, both edges ragged
    (2, 24, 12, 7, True),       # general form, only W odd
    (2, 24, 5, 8, True),        # general form, only H odd
    (1, 8, 3, 3, True),         # general form
]
MASK_ALL_SHAPES = [(3, 24, 9, 7, False), (2, 64, 11, 15, True)]      # scale = 0, shift = 1
ROUNDS = 8
NPATTERN = 8                    # 0..5: a tie of the maximum between two positions; 6: all four <= 0; 7: left as drawn
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def plant_ties(y, s, b, rng, name):
    """Planted EXACT ties, in place: window slot i (flat over image, window row, window column, channel) takes pattern i % 8 in every
    other run of eight slots, the rest stay as drawn.  0..5: positions PAIRS[p] hold the same stored y with a clearly positive activation, the other two smaller ones (one may be
    negative) -- (0, 3) is the tie across a smaller value between; 6: all four activations negative.  -> the pattern of every slot"""
    q = _quads(y)
    shape = q[0].shape
    idx = np.arange(q[0].size).reshape(shape)
    pat = np.where((idx // NPATTERN) % 2 == 0, idx % NPATTERN, NPATTERN - 1)
    sb = np.broadcast_to(s, shape)
    bb = np.broadcast_to(b, shape)
    ok = sb != 0
    inv = lambda a: rounded((a - bb) / np.where(ok, sb, 1.0), name)
    hi = 0.5 + np.abs(rng.normal(size=shape))
    lo = [hi * rng.uniform(-0.6, 0.6, size=shape) for _ in range(4)]
    neg = [-(0.2 + np.abs(rng.normal(size=shape))) for _ in range(4)]
    for p, pair in enumerate(PAIRS):
        sel = ok & (pat == p)
        for k in range(4):
            q[k][sel] = (inv(hi) if k in pair else inv(lo[k]))[sel]
    sel = ok & (pat == 6)
    for k in range(4):
        q[k][sel] = inv(neg[k])[sel]
    return pat


def settle(y, s, b, name, pooled):
    """Moves, in place, every y whose pre-activation is within MARGIN of zero away from it, and every window value within MARGIN of
    its window's (different) maximum down, by a few units of the storage type's spacing; equal values of a window move together, so
    planted ties stay exact.  A bounded number of rounds; -> the rounds it took.  Raises when the margins do not hold after ROUNDS."""
    for rnd in range(ROUNDS + 1):
        zero, gap = margins(y, s, b, pooled)
        if zero >= MARGIN and gap >= MARGIN:
            return rnd
        if rnd == ROUNDS:
            break
        a = y * s + b
        mag = np.abs(y * s) + np.abs(b)
        sgn = np.where(s < 0, -1.0, 1.0) * np.ones_like(y)
        step = (4 + 4 * rnd) * spacing(y, name)
        near = (a != 0) & (np.abs(a) < MARGIN * mag)
        y[near] = rounded(y + np.where(a > 0, 1.0, -1.0) * sgn * step, name)[near]
        if pooled:
            a = y * s + b
            qy, qs = _quads(y), _quads(sgn)
            r = np.stack(_quads(np.maximum(a, 0.0)))
            m = np.stack(_quads(np.where(a > 0, np.abs(y * s) + np.abs(b), 0.0)))
            top = r.max(axis=0)
            mtop = np.where(r == top, m, 0.0).max(axis=0)
            close = (r != top) & (top - r < MARGIN * (mtop + m))
            for k in range(4):
                down = rounded(qy[k] - qs[k] * (4 + 4 * rnd) * spacing(qy[k], name), name)
                qy[k][close[k]] = down[close[k]]
    raise AssertionError(f"margins {margins(y, s, b, pooled)} below {MARGIN} after {ROUNDS} rounds")


def bn_case(name, n, c, h, w, pooled, mask_all=False):
    """The inputs of one BatchNorm-backward case, every array float64 holding values of its storage type (activations: `name`;
    constants: f32).  mean / rstd are the batch statistics of y as drawn (before ties are planted), rounded to f32; scale = gamma rstd,
    shift = beta - mean scale (or 0 and 1 with mask_all).  Both margins of dz() are at least MARGIN with no element left out."""
    rng = np.random.default_rng(7919 * c + 131 * h + 17 * w + n + (1 if mask_all else 0))
    y = rounded(rng.normal(size=(n, h, w, c)) * 2.0 + 0.5, name)
    da = rounded(rng.normal(size=(n, h, w, c)), name)
    dp = rounded(rng.normal(size=(n, h // 2, w // 2, c)), name) if pooled else None
    flat = y.reshape(-1, c)
    mean = f32(flat.mean(0))
    rstd = f32(1.0 / np.sqrt(flat.var(0) + 1e-5))
    gamma = f32((1.0 + 0.3 * rng.normal(size=c)) * rng.choice([-1.0, 1.0], size=c, p=[0.25, 0.75]))
    beta = 0.3 * rng.normal(size=c)
    if mask_all:
        scale, shift = np.zeros(c), np.ones(c)
    else:
        scale = f32(gamma * rstd)
        shift = f32(beta - mean * scale)
    pat = plant_ties(y, scale, shift, rng, name) if pooled else None
    rounds = settle(y, scale, shift, name, pooled)
    assert np.array_equal(y, rounded(y, name))
    return dict(y=y, da=da, dp=dp, scale=scale, shift=shift, mean=mean, rstd=rstd, gamma=gamma, pattern=pat, rounds=rounds)


def winners(y, scale, shift):
    """the position 0..3 each complete window's dp goes to, [N, H//2, W//2, C]"""
    a = np.maximum(_f64(y) * _f64(scale) + _f64(shift), 0.0)
    return np.argmax(np.stack(_quads(a)), axis=0)


def bn_bwd_plan(name, n, c, h, w, pooled, has_da=True, four=False):
    """bn_bwd_plan / reduce_blocks of csrc/bn.hip, restated: which build serves the call and how long a lane's f32 chain is.
    four: ustrun_debug_flags bit 12 (the 4-channel kernels on 16-bit data).  -> dict(x8, even, G, PL, blocks, T, code)"""
    wide = name in ("bf16", "f16")
    g8 = c // 8
    x8 = wide and not pooled and not four and has_da and c % 8 == 0 and 1 <= g8 <= 256 and (g8 & (g8 - 1)) == 0
    if x8:
        G = g8
    else:
        G = 1
        while G < c // 4 and G < 256:
            G <<= 1
    PL = 256 // G
    nwin = n * ((h + 1) // 2) * ((w + 1) // 2) if pooled else n * h * w
    blocks = min(max(-(-nwin // (PL * 8)), 1), 1024)
    T = -(-nwin // (blocks * PL)) * (4 if pooled else 1)         # elements a lane adds up: windows per lane x pixels per window
    even = pooled and h % 2 == 0 and w % 2 == 0
    code = 0x424E0000 | (2 if wide else 4) << 4 | (4 if even else 0) | (2 if pooled else 0) | (1 if x8 else 0)
    return dict(x8=x8, even=even, G=G, PL=PL, blocks=blocks, T=T, code=code)


def head_plan(npix, c):
    """lanes_per_pixel / head_blocks of csrc/head.hip: -> (LPP, PPB, blocks, T = pixels a lane adds up)"""
    lpp = 1
    while lpp < c // 4 and lpp < 64:
        lpp <<= 1
    ppb = 256 // lpp
    blocks = min(max(-(-npix // (ppb * 16)), 1), 1024)
    return lpp, ppb, blocks, -(-npix // (blocks * ppb))


# (C, K) of the head cases and their extents (n, h, w)
HEAD_CK = [(4, 1), (8, 1), (8, 2), (16, 3), (24, 4), (64, 1), (64, 2), (64, 3), (64, 4), (64, 5), (64, 8), (264, 2), (512, 4), (1024, 2)]
HEAD_EXTENTS = [(1, 1, 1), (3, 9, 7)]


def head_case(name, c, k, n, h, w):
    """The inputs of one head case: y in the storage type; scale, shift, w, bias, dl in f32.  No margin is needed (header of the GPU
    test): relu enters only through max(., 0)."""
    rng = np.random.default_rng(977 * c + 31 * k + 7 * h + w)
    y = rounded(rng.normal(size=(n, h, w, c)), name)
    s, b = B_table(rng, c)
    return dict(y=y, scale=f32(s), shift=f32(b), w=f32(rng.normal(size=(k, c)) / 8), bias=f32(rng.normal(size=k)),
                dl=f32(rng.normal(size=(n, k, h, w))), dw0=f32(rng.normal(size=(k, c))), db0=f32(rng.normal(size=k)))


def B_table(rng, c):
    """scale / shift of one pass: |scale| >= 0.05, three in ten negative (as the sibling's table())"""
    return ((0.05 + np.abs(rng.normal(size=c))) * rng.choice([-1.0, 1.0], size=c, p=[0.3, 0.7]), rng.normal(size=c) * 0.5)


# ---- ustrun_bn_bwd_finalize_stat: synthetic row tables ---------------------------------------------------------------------------------
HI, G0, GNEG = 0, 2, 3            # channels: |mean| rstd = 1e3; gamma = 0; gamma < 0


def finalize_stat_case(rows, c, passes, aff_stride):
    """`passes` synthetic (dz, y)[count, C] in float64, each split into `rows` ragged chunks whose sums {sum dz, sum dz y} are rounded
    once to float32 (as bn_ops_ref's sibling builds its forward table): stat [passes, rows, 2, C] f32; mean / rstd [passes] tables
    aff_stride floats apart with NaN between the passes' constants; gamma [C]."""
    rng = np.random.default_rng(1000 * rows + 10 * c + passes)
    sizes = rng.integers(2, 6, size=rows)
    count = int(sizes.sum())
    edges = np.concatenate([[0], np.cumsum(sizes)])
    stat = np.empty((passes, rows, 2, c), dtype=np.float32)
    nt = (passes - 1) * aff_stride + c
    mean, rstd = np.full(nt, np.nan), np.full(nt, np.nan)
    for p in range(passes):
        sd = rng.uniform(0.5, 2.0, c)
        mu = rng.normal(size=c)
        mu[HI] = 1e3 * sd[HI]
        y = rng.normal(size=(count, c)) * sd + mu
        d = rng.normal(size=(count, c)) * (rng.random(size=(count, c)) < 0.6)
        for r, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
            stat[p, r, 0], stat[p, r, 1] = d[a:b].sum(0), (d[a:b] * y[a:b]).sum(0)
        mean[p * aff_stride:p * aff_stride + c] = f32(mu)
        rstd[p * aff_stride:p * aff_stride + c] = f32(1.0 / sd)
    gamma = f32(rng.normal(size=c))
    gamma[G0 % c], gamma[GNEG % c] = 0.0, -1.5
    return stat, count, gamma, mean, rstd, f32(rng.normal(size=c)), f32(rng.normal(size=c))
