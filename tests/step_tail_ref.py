"""Plain numpy restatement of the kernels of the step's tail (csrc/loss.hip, csrc/fftmix.hip), with the layouts of include/ustrun.h:
logits (N, K, HW); softmax targets / masks (N, HW); sigmoid targets / masks (N, K, HW).  Everything is float64 unless a function takes
`dt`: then the TERMS are evaluated in that type (np.float32: what float32 arithmetic costs at these inputs, the yardstick of the GPU
tests) and only the sums over them are float64.  Pinned to torch, oracle/ and utils.metrics by tests/test_step_tail_ref_host.py.
"""
import numpy as np

KMAX = 8
SMOOTH = float(np.float32(1e-10))          # the kernels' constant is a float
U = 2.0 ** -24
SOFTMAX, SIGMOID = 0, 1
BBOX_BLOCKS = 64


def nsums(K):
    """USTRUN_LOSS_NSUMS(K)"""
    return 4 + 3 * K


def stream_blocks(items):
    """the grid of a streaming kernel (csrc/stream_reduce.h): four items per thread, 1024 blocks at the most"""
    return int(min(max((items + 1023) // 1024, 1), 1024))


def trips(items):
    """the most items one thread of that grid sums"""
    return -(-items // (stream_blocks(items) * 256))


def f32(x):
    return float(np.float32(x))


def softmax(x, dt=np.float64):
    """over axis 1 of (N, K, HW), in the kernels' order: exp(l - max), the sum, one reciprocal"""
    x = x.astype(dt)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    se = e[:, :1].copy()
    for k in range(1, x.shape[1]):
        se = se + e[:, k:k + 1]
    return e * (dt(1) / se), se


def sigmoid(x, dt=np.float64):
    x = x.astype(dt)
    ea = np.exp(-np.abs(x))
    return np.where(x >= 0, dt(1) / (dt(1) + ea), ea / (dt(1) + ea)), ea


# ---- seg_loss -----------------------------------------------------------------------------------------------------------------------
def seg_loss_terms(logits, target, mask, mode, dt=np.float64):
    """(ce, I, Z, Y): the per-item terms of the sums; ce (items,), the others (kk, items) with kk = K (softmax) or 1 (sigmoid)"""
    N, K, HW = logits.shape
    if mode == SOFTMAX:
        p, se = softmax(logits, dt)
        x = logits.astype(dt)
        m = np.ones((N, HW), dt) if mask is None else mask.astype(dt)
        m1 = np.ones((N, HW), dt) if mask is None else (mask == 1).astype(dt)
        lt = np.take_along_axis(x - x.max(axis=1, keepdims=True), target[:, None, :], 1)[:, 0]
        ce = (np.log(se[:, 0]) - lt) * m
        tk = (target[:, None, :] == np.arange(K)[None, :, None]).astype(dt)
        mk = np.stack([np.ones((N, HW), dt) if k == 0 else m1 for k in range(K)], 1)
        flat = lambda a: np.moveaxis(a, 1, 0).reshape(K, -1)
        return ce.reshape(-1), flat(p * tk * mk), flat(p * p * mk), flat(tk * mk)
    p, ea = sigmoid(logits, dt)
    x, t = logits.astype(dt), target.astype(dt)
    m = np.ones_like(x) if mask is None else mask.astype(dt)
    ce = (np.maximum(x, dt(0)) - x * t + np.log1p(ea)) * m
    return ce.reshape(-1), (p * t * m).reshape(1, -1), (p * p * m).reshape(1, -1), (t * t * m).reshape(1, -1)


def dice_of(I, Z, Y, smooth=SMOOTH):
    return 1.0 - (2.0 * I + smooth) / (Z + Y + smooth)


def seg_loss_fwd(logits, target, mask, mode):
    """out[USTRUN_LOSS_NSUMS(K)]: {ce mean, dice, ce sum, I[kk], Z[kk], Y[kk]}; the floats behind 3 + 3 kk are not written (NaN here)"""
    N, K, HW = logits.shape
    ce, I, Z, Y = (a.astype(np.float64) for a in seg_loss_terms(logits, target, mask, mode))
    kk = len(I)
    out = np.full(nsums(K), np.nan)
    out[0], out[2] = ce.sum() / ce.size, ce.sum()
    out[1] = sum(dice_of(I[k].sum(), Z[k].sum(), Y[k].sum()) for k in range(kk)) / kk
    out[3:3 + kk], out[3 + kk:3 + 2 * kk], out[3 + 2 * kk:3 + 3 * kk] = I.sum(1), Z.sum(1), Y.sum(1)
    return out


def seg_loss_bwd(logits, target, mask, mode, sums, gdev=None, gscale=1.0, cw=1.0, dw=1.0, dt=np.float64):
    """dlogits (N, K, HW) of gscale (cw g0 ce + dw g1 dice) from the stored sums of the forward"""
    N, K, HW = logits.shape
    s = np.asarray(sums).astype(dt)
    sm, gs = dt(SMOOTH), dt(gscale)
    cw, dw = dt(cw) * dt(1 if gdev is None else gdev[0]), dt(dw) * dt(1 if gdev is None else gdev[1])
    if mode == SOFTMAX:
        p, _ = softmax(logits, dt)
        m = np.ones((N, HW), dt) if mask is None else mask.astype(dt)
        m1 = np.ones((N, HW), dt) if mask is None else (mask == 1).astype(dt)
        cen = cw / dt(N * HW)
        G = np.empty_like(p)
        gp = np.zeros((N, HW), dt)
        tk = (target[:, None, :] == np.arange(K)[None, :, None]).astype(dt)
        for k in range(K):
            I, D = s[3 + k], s[3 + K + k] + s[3 + 2 * K + k] + sm
            A, Bc = dt(-2) / D / dt(K), dt(2) * (dt(2) * I + sm) / (D * D) / dt(K)
            mk = np.ones((N, HW), dt) if k == 0 else m1
            G[:, k] = dw * (A * tk[:, k] * mk + Bc * p[:, k] * mk)
            gp = gp + G[:, k] * p[:, k]
        return gs * (cen * m[:, None] * (p - tk) + p * (G - gp[:, None]))
    p, _ = sigmoid(logits, dt)
    t = target.astype(dt)
    m = np.ones_like(p) if mask is None else mask.astype(dt)
    I, D = s[3], s[4] + s[5] + sm
    A, Bc = dt(-2) / D, dt(2) * (dt(2) * I + sm) / (D * D)
    cen = cw / dt(N * K * HW)
    G = dw * (A * t * m + Bc * p * m)
    return gs * (cen * m * (p - t) + G * p * (dt(1) - p))


# ---- dice (DiceLossWithMask in every mode combination) -------------------------------------------------------------------------------
def dice_ptm(logits, target, mask, act, multi, tper, mper, dt=np.float64):
    """(p, t, m, yonce), each (N, K, HW): what dice_pixel hands the two kernels"""
    N, K, HW = logits.shape
    p = logits.astype(dt) if act == 0 else softmax(logits, dt)[0] if act == 1 else sigmoid(logits, dt)[0]
    if not multi:
        tv = target.astype(np.float64)                            # (N, HW) class indices, int64 or float
        t = (tv[:, None, :] == np.arange(K)[None, :, None]).astype(dt)
        m1 = np.ones((N, HW), dt) if mask is None else (mask == 1).astype(dt)
        m = np.stack([np.ones((N, HW), dt) if k == 0 else m1 for k in range(K)], 1)
        return p, t, m, False
    t = np.broadcast_to(target[:, None, :] if tper else target, (N, K, HW)).astype(dt)
    m = np.ones((N, K, HW), dt) if mask is None else np.broadcast_to(mask[:, None, :] if mper else mask, (N, K, HW)).astype(dt)
    return p, t, m, bool(tper and (mper or mask is None))


def dice_terms(logits, target, mask, act, multi, tper, mper, dt=np.float64):
    """(I, Z, Y) terms, each (K, items).  A per-pixel target under a per-pixel (or no) mask is counted ONCE in Y, not once per class
    (dice_fwd_kernel, utils/losses.py:229): its terms of the classes behind the first are zero."""
    p, t, m, yonce = dice_ptm(logits, target, mask, act, multi, tper, mper, dt)
    K = p.shape[1]
    flat = lambda a: np.moveaxis(a, 1, 0).reshape(K, -1)
    Y = t * t * m
    if yonce:
        Y = Y.copy()
        Y[:, 1:] = 0
    return flat(p * t * m), flat(p * p * m), flat(Y)


def dice_fwd(logits, target, mask, act, multi, tper, mper, weight=None, smooth=SMOOTH):
    """out[1 + 3K]: {loss, I[K], Z[K], Y[K]}; multi: the totals in k = 0, zeros behind"""
    K = logits.shape[1]
    I, Z, Y = (a.astype(np.float64).sum(1) for a in dice_terms(logits, target, mask, act, multi, tper, mper))
    w = np.ones(K) if weight is None else np.asarray(weight, np.float64)
    smooth = f32(smooth)
    out = np.zeros(1 + 3 * K)
    if multi:
        out[0] = dice_of(I.sum(), Z.sum(), Y.sum(), smooth)
        out[1], out[1 + K], out[1 + 2 * K] = I.sum(), Z.sum(), Y.sum()
    else:
        out[0] = sum(w[k] * dice_of(I[k], Z[k], Y[k], smooth) for k in range(K)) / K
        out[1:1 + K], out[1 + K:1 + 2 * K], out[1 + 2 * K:] = I, Z, Y
    return out


def dice_bwd(logits, target, mask, act, multi, tper, mper, sums, weight=None, smooth=SMOOTH, gdev=None, gscale=1.0, dt=np.float64):
    p, t, m, _ = dice_ptm(logits, target, mask, act, multi, tper, mper, dt)
    N, K, HW = p.shape
    s = np.asarray(sums).astype(dt)
    sm = dt(np.float32(smooth))
    gs = dt(gscale) * dt(1 if gdev is None else gdev[0])
    G = np.empty_like(p)
    gp = np.zeros((N, HW), dt)
    for k in range(K):
        kk = 0 if multi else k
        I, D = s[1 + kk], s[1 + K + kk] + s[1 + 2 * K + kk] + sm
        wk = dt(1) if multi else dt(np.float32(1 if weight is None else weight[k])) / dt(K)
        A, Bc = dt(-2) / D * wk, dt(2) * (dt(2) * I + sm) / (D * D) * wk
        G[:, k] = (A * t[:, k] + Bc * p[:, k]) * m[:, k]
        gp = gp + G[:, k] * p[:, k]
    d = p * (G - gp[:, None]) if act == 1 else G * p * (dt(1) - p) if act == 2 else G
    return gs * d


# ---- pseudo labels -------------------------------------------------------------------------------------------------------------------
def pseudo_label(logits, threshold, mode):
    """(label, mask, p): softmax: label (N, HW) int64 = the FIRST index of the largest probability, mask = (max p > th), p (N, K, HW);
    sigmoid: label = (p >= 0.5), mask = (p >= th) + (p <= 1 - th), all (N, K, HW).  The threshold and 1 - th are the kernel's floats."""
    th = f32(threshold)
    if mode == SOFTMAX:
        p, _ = softmax(logits)
        return np.argmax(p, 1).astype(np.int64), (p.max(1) > th).astype(np.float64), p
    x = logits.astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-x))
    lo = float(np.float32(1) - np.float32(threshold))
    return (p >= 0.5).astype(np.float64), (p >= th).astype(np.float64) + (p <= lo), p


def pseudo_label_p_err(logits, p, mode):
    """What float32 arithmetic can move a probability by.  softmax: l - max is rounded once (u |d| in the exponent = a relative u |d| of
    the exponential, |d| <= 104: beyond it the float exponential is 0), expf is within 2 ulp, the sum of K terms adds K - 1 roundings,
    the quotient one: relative (2 (u d + 2u) + K u) for numerator and denominator together, plus the subnormal floor.  K = 1: p = 1 / 1,
    exact.
    sigmoid: expf (2 ulp), 1 + e, the quotient: relative 4u, taken as 5u."""
    if mode == SOFTMAX:
        K = logits.shape[1]
        if K == 1:
            return np.zeros_like(p)
        x = logits.astype(np.float64)
        d = np.minimum(x.max(1, keepdims=True) - x.min(1, keepdims=True), 104.0)
        return p * U * (2 * d + K + 6) + K * 2.0 ** -148
    return 5 * U * p + 2.0 ** -148


PSEUDO_SHAPES = [(1, 1, 1), (2, 3, 77), (4, 2, 4096), (1, 8, 515)]
PSEUDO_THRESHOLDS = [0.95, 0.5, 0.0, 1.0]
PSEUDO_ZONE_CAP = 1e-3


def pseudo_label_case(N, K, HW, seed=0):
    """(float32 logits (N, K, HW), planted (N, HW)): 2 x normal logits (at that scale fewer than 0.1 % of the probabilities lie within
    float32's reach of any of the thresholds, 1 included) and, where the plane is long enough, planted pixels at the head of
    sample 0: four of all-equal logits (0: the sigmoid probability is exactly 0.5), four whose first and last planes are equal
    and above the rest, four of +-60."""
    rng = np.random.default_rng(1000 * K + HW + seed)
    x = (2.0 * rng.normal(size=(N, K, HW))).astype(np.float32)
    planted = np.zeros((N, HW), bool)
    if HW >= 12:
        x[0, :, 0:4] = 0.0
        x[0, :, 4:8] = np.minimum(x[0, :, 4:8], 1.0)
        x[0, 0, 4:8] = x[0, K - 1, 4:8] = 1.5
        x[0, :, 8:12] = 60.0 * (-1.0) ** np.arange(K)[:, None]
        planted[0, :12] = True
    return x, planted


def pseudo_label_accept(logits, threshold, mode, label, mask):
    """Which elements of a device result are acceptable: equal to the float64 result, OR the float64 probability lies within
    pseudo_label_p_err of the decision boundary (labels, softmax: the probability of the class chosen is within the two errors of the
    largest).  -> (label_ok, mask_ok, label_zone, mask_zone): the zones are the elements where a second answer is acceptable."""
    rl, rm, p = pseudo_label(logits, threshold, mode)
    e = pseudo_label_p_err(logits, p, mode)
    th = f32(threshold)
    if mode == SOFTMAX:
        best = np.take_along_axis(p, rl[:, None], 1)[:, 0]
        ebest = np.take_along_axis(e, rl[:, None], 1)[:, 0]
        got = np.clip(label, 0, p.shape[1] - 1)
        pg, eg = np.take_along_axis(p, got[:, None], 1)[:, 0], np.take_along_axis(e, got[:, None], 1)[:, 0]
        label_ok = (label == rl) | ((label == got) & (best - pg <= ebest + eg))
        srt = np.sort(p, 1)
        label_zone = (best - srt[:, -2] <= 2 * ebest) if p.shape[1] > 1 else np.zeros_like(rl, bool)
        mask_zone = (np.abs(best - th) <= ebest) & (ebest > 0)
        mask_ok = (mask == rm) | (mask_zone & ((mask == 0) | (mask == 1)))
        return label_ok, mask_ok, label_zone, mask_zone
    lo = float(np.float32(1) - np.float32(threshold))
    label_zone = np.abs(p - 0.5) <= e
    label_ok = (label == rl) | (label_zone & ((label == 0) | (label == 1)))
    zh, zl = np.abs(p - th) <= e, np.abs(p - lo) <= e
    hi, low = (p >= th).astype(np.float64), (p <= lo).astype(np.float64)
    mask_ok = mask == hi + low
    mask_ok |= zh & (mask == (1 - hi) + low)
    mask_ok |= zl & (mask == hi + (1 - low))
    mask_ok |= zh & zl & (mask == (1 - hi) + (1 - low))
    return label_ok, mask_ok, label_zone, zh | zl


# ---- target algebra ------------------------------------------------------------------------------------------------------------------
def mix_targets(mode, box, pl, mask, plwul, mwul, plwlu, mwlu, cutl, cutm):
    """-> (pl_w, mask_w, pl_ul, mask_ul, pl_lu, mask_lu); box (N, HW); softmax: labels int64 (N, HW), masks (N, HW); sigmoid: all
    float (N, K, HW).  The label blends truncate towards zero as the kernel's casts do."""
    b = box.astype(np.float64)
    if mode == SIGMOID:
        b = b[:, None, :]
    nb = 1.0 - b
    lab = lambda a: np.trunc(a).astype(np.int64 if mode == SOFTMAX else np.float64)
    plw = lab(plwul * nb + plwlu * b)
    mw = mwul.astype(np.float64) * nb + mwlu * b
    mw = np.where((plw == pl) * mask.astype(np.float64) == 0, 0.0, mw)
    shape = mask.shape
    return (plw, mw, lab(pl * nb + cutl * b), np.where(np.broadcast_to(b, shape) == 1, cutm, mask),
            lab(cutl * nb + pl * b), np.where(np.broadcast_to(b, shape) == 0, cutm, mask))


def box_mix(a, b, box):
    """a (1 - box) + b box, box (N, HW) over the channels of (N, C, HW): (value, |a (1 - box)| + |b box|)"""
    bx = box.astype(np.float64)[:, None, :]
    x, y = a.astype(np.float64) * (1.0 - bx), b.astype(np.float64) * bx
    return x + y, np.abs(x) + np.abs(y)


def decode_labels(y, kind):
    """kind 0: (N, HW) -> float (N, 2, HW) {y == 0, y <= 128}; 1: int64 (y == 0); 2: int64 (y == 255); 3: (N, HW, 3) -> the class of
    the LAST channel that is 255"""
    if kind == 0:
        return np.stack([y == 0, y <= 128], 1).astype(np.float64)
    if kind == 1:
        return (y == 0).astype(np.int64)
    if kind == 2:
        return (y == 255).astype(np.int64)
    return np.where(y[..., 2] == 255, 3, np.where(y[..., 1] == 255, 2, np.where(y[..., 0] == 255, 1, 0))).astype(np.int64)


def region_bbox(planes, H, W):
    """the int32 [64, 4] table of region_bbox_kernel: block b sees the elements e with (e // 256) % 64 == b and reports {min y, max y,
    min x, max x} of the non-zero ones of ANY plane, {H, -1, W, -1} where it sees none"""
    nz = np.zeros(H * W, bool)
    for p in planes:
        nz |= np.asarray(p).reshape(-1) != 0
    e = np.arange(H * W)
    blk, y, x = (e // 256) % BBOX_BLOCKS, e // W, e % W
    out = np.tile(np.array([H, -1, W, -1], np.int32), (BBOX_BLOCKS, 1))
    for b in np.unique(blk[nz]):
        s = nz & (blk == b)
        out[b] = [y[s].min(), y[s].max(), x[s].min(), x[s].max()]
    return out


def fold_bbox(table):
    """the rectangle {y0, y1, x0, x1} with exclusive ends of the table's 64 rows, None for an empty region"""
    if table[:, 1].max() < 0:
        return None
    return (int(table[:, 0].min()), int(table[:, 1].max()) + 1, int(table[:, 2].min()), int(table[:, 3].max()) + 1)


def rect_masks(rects, H, W):
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    return np.stack([((y >= r[0]) & (y < r[1]) & (x >= r[2]) & (x < r[3])).astype(np.float64) for r in rects])


def dice_split(N, K, HW):
    """how many blocks ustrun_dice_counts spreads one (sample, part) plane over; above 1 it clears `counts` and adds atomically"""
    split = 1
    while N * K * split < 512 and HW // (split * 2) >= 2048:
        split *= 2
    return split


def dice_counts(pred, gt, K, by_class):
    """int32 (N, K, 3) {|pred|, |gt|, |pred & gt|}; by_class: pred / gt (N, HW) class maps, part c is class c + 1 (floats truncate);
    else (N, K, HW), non-zero = set"""
    if by_class:
        pv, gv = np.trunc(pred).astype(np.int64), np.trunc(gt).astype(np.int64)
        pb = np.stack([pv == c + 1 for c in range(K)], 1)
        gb = np.stack([gv == c + 1 for c in range(K)], 1)
    else:
        pb, gb = pred != 0, gt != 0
    return np.stack([pb.sum(-1), gb.sum(-1), (pb & gb).sum(-1)], -1).astype(np.int32)


# ---- optimizer and loss scale --------------------------------------------------------------------------------------------------------
def sgd_ema(p, g, v, t, lr, mu, wd, first, alpha, gsc, scale=None, skip=False):
    """torch.optim.SGD(momentum, weight_decay) + the EMA line on the values the kernel sees (every scalar a float): returns
    ((p, v, t), (ep, ev, et)) -- the float64 results and bounds on what float32 evaluation of the kernel's expression
    can differ by: one 2^-24 rounding per operation, propagated (tests/test_gpu_step_tail_ops.py derives them).  scale: the loss scale
    the gradient is divided by (sgd_ema_scaled); skip: found_inf set, p and v stay, t moves."""
    lr, mu, wd, alpha, gsc = (f32(a) for a in (lr, mu, wd, alpha, gsc))
    p, g, v = (a.astype(np.float64) for a in (p, g, v))
    R = 1.0 + 2.0 ** -20                                            # the second-order terms
    if skip:
        pn, ep, vn, ev = p, np.zeros_like(p), v, np.zeros_like(v)
    else:
        c, ec = gsc, 0.0
        if scale is not None:
            c = gsc / f32(scale)
            ec = U * abs(c)                                         # the quotient, rounded once
        a, b = g * c, wd * p
        gv = a + b
        egv = np.abs(g) * ec + U * np.abs(a) + U * np.abs(b) + U * np.abs(gv)
        if first:
            vn, ev = gv, egv
        else:
            mv = mu * v
            vn = mv + gv
            ev = U * np.abs(mv) + egv + U * np.abs(vn)
        lv = lr * vn
        pn = p - lv
        ep = lr * ev + U * np.abs(lv) + U * np.abs(pn)
        ev, ep = ev * R, ep * R
    if t is None:
        return (pn, vn, None), (ep, ev, None)
    t = t.astype(np.float64)
    om = float(np.float32(1) - np.float32(alpha))                   # the kernel's 1.f - alpha, rounded once
    x, y = alpha * t, om * pn
    tn = x + y
    et = (U * np.abs(x) + om * ep + U * np.abs(y) + U * np.abs(tn)) * R
    return (pn, vn, tn), (ep, ev, et)


def amp_update(state, growth, backoff, interval):
    """GradScaler.update() on the eight state floats {scale, scale, tracker, found_inf, skipped, seen, -, -}, in float arithmetic"""
    s = np.array(state, np.float32)
    scale, tracker = s[0], s[2]
    s[5] += np.float32(1)
    if s[3] != 0:
        scale, tracker = scale * np.float32(backoff), np.float32(0)
        s[4] += np.float32(1)
    else:
        tracker = tracker + np.float32(1)
        if tracker >= np.float32(interval):
            scale, tracker = scale * np.float32(growth), np.float32(0)
    s[0], s[1], s[2], s[3] = scale, scale, tracker, 0
    return s


def amp_check(g):
    """found_inf of a gradient buffer"""
    return 0.0 if np.isfinite(g).all() else 1.0


# ---- amplitude mix -------------------------------------------------------------------------------------------------------------------
def freq_mix(src, trg, ratios, b):
    """src, trg (n, C, H, W) in [-1, 1]; the full numpy.fft form of oracle/host_ref.freq_mix with the window half-width given (H != W
    allowed), on the 0..255 scale the reference works in, clipped and scaled back"""
    S, T = (src.astype(np.float64) + 1.0) * 127.5, (trg.astype(np.float64) + 1.0) * 127.5
    f = np.fft.fft2(S, axes=(-2, -1))
    amp = np.abs(f)
    pha = np.where(amp == 0, 0.0, np.angle(f))      # np.angle(0) = 0; a transform of zeros may hold -0.0, whose angle would be pi
    a_s = np.fft.fftshift(amp, axes=(-2, -1))
    a_t = np.fft.fftshift(np.abs(np.fft.fft2(T, axes=(-2, -1))), axes=(-2, -1))
    h, w = S.shape[-2:]
    ch, cw = h // 2, w // 2
    r = np.asarray(ratios, np.float32).astype(np.float64)[:, None, None, None]
    sl = (slice(None), slice(None), slice(ch - b, ch + b + 1), slice(cw - b, cw + b + 1))
    a_s[sl] = a_s[sl] * (1 - r) + a_t[sl] * r
    a_s = np.fft.ifftshift(a_s, axes=(-2, -1))
    out = np.real(np.fft.ifft2(a_s * np.exp(1j * pha), axes=(-2, -1)))
    return np.clip(out, 0, 255) / 127.5 - 1.0


def freq_mix_two_stage(src, trg, ratios, b, dt=np.float32):
    """The kernel's form: a direct (2b+1)^2-bin DFT of both images, then out = src + Re sum coef e^{+j..} per pixel with
    coef = r (|F_trg| - |F_src|) e^{j arg F_src} / HW (phase (1, 0) where |F_src| = 0).  dt = np.float32: complex64 throughout (the
    yardstick); np.float64: the same algebra in double."""
    ct = np.complex64 if dt == np.float32 else np.complex128
    n, C, H, W = src.shape
    S, T = (src.astype(dt) + dt(1)) * dt(127.5), (trg.astype(dt) + dt(1)) * dt(127.5)
    fr = np.arange(-b, b + 1)

    def tw(n_, sign):
        k = np.fmod(fr[:, None] * np.arange(n_)[None, :], n_).astype(dt)
        ang = dt(sign) * dt(6.283185307179586) * k / dt(n_)
        return (np.cos(ang) + 1j * np.sin(ang)).astype(ct)

    fwd = lambda X: np.einsum("uy,ncyx,vx->ncuv", tw(H, -1), X.astype(ct), tw(W, -1)).astype(ct)
    fs, ft = fwd(S), fwd(T)
    a_s, a_t = np.abs(fs).astype(dt), np.abs(ft).astype(dt)
    ph = np.where(a_s > 0, fs / np.where(a_s > 0, a_s, dt(1)), ct(1)).astype(ct)
    g = np.asarray(ratios, np.float32).astype(dt)[:, None, None, None] * (a_t - a_s) * (dt(1) / (dt(H) * dt(W)))
    corr = np.real(np.einsum("ncuv,uy,vx->ncyx", (g * ph).astype(ct), tw(H, 1), tw(W, 1))).astype(dt)
    return np.clip(S + corr, dt(0), dt(255)) / dt(127.5) - dt(1)
