"""GPU: the backward in eval mode -- through BatchNorm frozen on its running statistics.

1-3  the one-pass operator ustrun_bn_bwd_frozen against tests/frozen_bn_ref.py (float64; pinned to torch's autograd by
     tests/test_frozen_bn_ref_host.py): exact on small integers, bounded on real values, and its contracts;
4-8  UNet in eval mode (reference networks/unet_model.py:25-39 under model.eval(): an ordinary autograd module) against
     oracle/unet_ref.py with train=False, and the plan's variants;
9    the stand-alone blocks."""
import copy
import functools

import numpy as np
import pytest
import torch

from frozen_bn_ref import frozen_bn_bwd
from oracle import unet_ref as U
from test_gpu_input_grad import LOSSES, _inputs
from test_gpu_unet import YARD_X, build_model, rel_l2

pytestmark = pytest.mark.gpu

_ST = {"f32": (torch.float32, 0, 0.0), "bf16": (torch.bfloat16, 1, 2.0 ** -8), "f16": (torch.float16, 2, 2.0 ** -11),
       "f32x3": (torch.float32, 3, 0.0)}            # torch type, USTRUN_* code, unit roundoff of the storage type
U32 = 2.0 ** -24


def _stream():
    return torch.cuda.current_stream().cuda_stream


def frozen(da, dp, y, consts, dtype, sums=True, accumulate=0, dy=None, dg=None, db=None, part=None, passes=1):
    """ustrun_bn_bwd_frozen (passes == 1) / _passes on device tensors: da, y [passes * N, H, W, C] in the storage type, dp
    [passes * N, H // 2, W // 2, C] or None, consts [passes, 4, C] f32 = scale, shift, mean, rstd.  dy: the output tensor (da itself
    for the in-place form; default a NaN-filled one).  -> dy, dgamma, dbeta, partials"""
    from ustrun import _lib as L
    lib = L.lib()
    nn, h, w, c = y.shape
    n = nn // passes
    if dy is None:
        dy = torch.full_like(y, float("nan"))
    nb = lib.ustrun_bn_bwd_partials_bytes(n * h * w, c)
    if part is None:
        part = torch.full((nb // 4,), float("nan"), device=y.device)
    if sums and dg is None:
        dg, db = torch.full((c,), float("nan"), device=y.device), torch.full((c,), float("nan"), device=y.device)
    k = consts
    args = (L.ptr(da), L.ptr(dp), y.data_ptr(), k[0, 0].data_ptr(), k[0, 1].data_ptr(), k[0, 2].data_ptr(), k[0, 3].data_ptr(),
            n, h, w, c, dy.data_ptr(), L.ptr(dg) if sums else None, L.ptr(db) if sums else None, accumulate, part.data_ptr(), nb,
            _ST[dtype][1])
    if passes == 1:
        L.check(lib.ustrun_bn_bwd_frozen(*args, _stream()), "ustrun_bn_bwd_frozen")
    else:
        L.check(lib.ustrun_bn_bwd_frozen_passes(*args, passes, 4 * c, _stream()), "ustrun_bn_bwd_frozen_passes")
    return dy, dg, db, part


def _ref(da, dp, y, consts):
    k = consts.double().cpu().numpy()
    f = lambda t: None if t is None else t.double().cpu().numpy()
    return frozen_bn_bwd(f(da), f(dp), f(y), k[0], k[1], k[2], k[3])


def _integer_case(n, h, w, c, pooled, dtype, g, with_da=True):
    """integers in -2..2, scale = +-2^k, shift and mean small integers, rstd 2^k: a = y scale + shift, g, scale g, every partial sum
    (|.| <= 8 N H W) and rstd (sum g y - mean sum g) are exact in f32 and in every storage type"""
    st = _ST[dtype][0]
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)
    y = ri(-2, 2, (n, h, w, c)).to(st).cuda()
    da = ri(-2, 2, (n, h, w, c)).to(st).cuda() if with_da else None
    dp = ri(-2, 2, (n, h // 2, w // 2, c)).to(st).cuda() if pooled else None
    scale = (2.0 ** ri(-2, 1, (c,)).float()) * (2 * ri(0, 1, (c,)).float() - 1)
    consts = torch.stack([scale, ri(-1, 1, (c,)).float(), ri(-1, 1, (c,)).float(), 2.0 ** ri(-1, 1, (c,)).float()])[None].contiguous().cuda()
    return da, dp, y, consts


# ---- 1. the operator, exact ----------------------------------------------------------------------------------------------------
# (3, 5, 7): 105 pixels, no multiple of any block's pixel lanes (256 / G, G = 1 .. 64); (2, 16, 16) at C = 4: one block of 256
# pixel lanes walks 512 pixels, the grid-stride loop twice, and at C = 256 the launch has 8 (16-bit) / 16 (f32) blocks; pooled
# (2, 5, 7): odd extents, the last row / column in a partial window; (1, 6, 4): even extents, the all-pixels-exist build
SHAPES = [(1, 1, 1, False), (2, 16, 16, False), (3, 5, 7, False), (2, 5, 7, True), (1, 6, 4, True)]


@pytest.mark.parametrize("n,h,w,pooled", SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_operator_exact_on_small_integers(dtype, n, h, w, pooled):
    g = torch.Generator().manual_seed(500 + 31 * h + w)
    for c in (4, 8, 24, 64, 256, 1032):
        for with_da in ((True, False) if pooled else (True,)):
            da, dp, y, consts = _integer_case(n, h, w, c, pooled, dtype, g, with_da)
            dy, dg, db, _ = frozen(da, dp, y, consts, dtype)
            rdy, rdg, rdb = _ref(da, dp, y, consts[0])
            assert torch.equal(dy.double().cpu(), torch.from_numpy(rdy)), (c, with_da)
            assert torch.equal(dg.double().cpu(), torch.from_numpy(rdg)), (c, with_da, dg.cpu(), rdg)
            assert torch.equal(db.double().cpu(), torch.from_numpy(rdb)), (c, with_da)
            dy2, _, _, part = frozen(da, dp, y, consts, dtype, sums=False)       # frozen parameters: the same dy, nothing else
            assert torch.equal(dy2.double().cpu(), torch.from_numpy(rdy)) and bool(torch.isnan(part).all()), c


# ---- 2. the operator, real values -------------------------------------------------------------------------------------------------
def _chain_depth(n, h, w, c, pooled, dtype):
    """additions in the longest f32 chain of one row of the sums, from the launcher's plan (bn.hip, bn_bwd_frozen_passes): a thread
    owns a channel group and every (blocks * lanes)-th window; the block then adds its lanes in order"""
    x8 = dtype != "f32" and not pooled and c % 8 == 0 and (c // 8) & (c // 8 - 1) == 0 and c // 8 <= 256
    if x8:
        G = c // 8
    else:
        G = 1
        while G < c // 4 and G < 256:
            G *= 2
    lanes = 256 // G
    nwin = n * ((h + 1) // 2) * ((w + 1) // 2) if pooled else n * h * w
    blocks = min(max(-(-nwin // (lanes * 8)), 1), 1024)
    return -(-nwin // (blocks * lanes)) * (4 if pooled else 1) + lanes


@pytest.mark.parametrize("n,h,w,c,pooled", [(2, 16, 16, 64, False), (3, 5, 7, 24, False), (4, 32, 32, 8, False), (2, 5, 7, 8, True),
                                            (2, 16, 16, 64, True)])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_operator_real_values_within_derived_bounds(dtype, n, h, w, c, pooled):
    """Bounds, derived as DESIGN.md 19 derives its own (u = 2^-24, u_s = the storage type's unit roundoff: 0 / 2^-8 / 2^-11), against
    float64 on the operands AS STORED:
      dy = fl_s(fl(scale * fl(da + dp))): two f32 roundings and the storage rounding -> |dy - ref| <= (3 u + 1.001 u_s) |ref| + t_s,
      t_s = half the spacing of the storage type's subnormals (f16: 2^-25 below 2^-14; bf16 and f32 share f32's exponent range: 0);
      a row of the sums is an f32 chain of at most d additions (_chain_depth) over terms that carry one rounding (g = fl(da + dp))
      or two (fl(g y), unless fused): |S1 - sum g| <= (d + 1) u sum |g|, |S2 - sum g y| <= (d + 2) u sum |g y|; the rows are added
      in f64 (2^-53 per addition: nothing beside u) and the results rounded to f32 once:
      |dbeta - ref| <= E1 + u |ref|,  |dgamma - ref| <= rstd (E2 + |mean| E1) + u |ref|, each with 1 % for the second-order terms.
    The ReLU mask is kept away from a rounding decision: pre-activations within 1e-2 of zero are moved to 1."""
    st, _, us = _ST[dtype]
    g = torch.Generator().manual_seed(900 + 7 * h + c)
    gamma = 1 + 0.5 * torch.randn(c, generator=g)
    gamma[0] = -gamma[0].abs()
    rstd = 1.0 / torch.sqrt(0.5 + 1.5 * torch.rand(c, generator=g) + 1e-5)
    mean = 0.3 * torch.randn(c, generator=g)
    scale = gamma * rstd
    shift = 0.2 * torch.randn(c, generator=g) - mean * scale
    y = torch.randn(n, h, w, c, generator=g).to(st).float()
    near = (y * scale + shift).abs() < 1e-2
    y = torch.where(near, ((1 - shift) / scale).expand_as(y), y).to(st)
    assert float((y.double() * scale.double() + shift.double()).abs().min()) > 4e-3
    y = y.cuda()
    da = torch.randn(n, h, w, c, generator=g).to(st).cuda()
    dp = torch.randn(n, h // 2, w // 2, c, generator=g).to(st).cuda() if pooled else None
    consts = torch.stack([scale, shift, mean, rstd])[None].contiguous().cuda()
    dy, dg, db, _ = frozen(da, dp, y, consts, dtype)
    rdy, rdg, rdb = _ref(da, dp, y, consts[0])
    k = consts[0].double().cpu().numpy()
    gq = rdy / k[0]                                                 # g, float64
    yq = y.double().cpu().numpy()
    d = _chain_depth(n, h, w, c, pooled, dtype)
    e1 = (d + 1) * U32 * np.abs(gq).sum((0, 1, 2))
    e2 = (d + 2) * U32 * np.abs(gq * yq).sum((0, 1, 2))
    bound_db = 1.01 * (e1 + U32 * np.abs(rdb))
    bound_dg = 1.01 * (k[3] * (e2 + np.abs(k[2]) * e1) + U32 * np.abs(rdg))
    err_dy = np.abs(dy.double().cpu().numpy() - rdy)
    bound_dy = (3 * U32 + 1.001 * us) * np.abs(rdy) + (2.0 ** -25 if dtype == "f16" else 0.0)
    err_dg, err_db = np.abs(dg.double().cpu().numpy() - rdg), np.abs(db.double().cpu().numpy() - rdb)
    rel = lambda e, b: float((e / np.maximum(b, 1e-300)).max())
    print(f"bn_bwd_frozen {dtype} {(n, h, w, c)}{' pooled' if pooled else ''}: chain depth {d}; error / bound: dy {rel(err_dy, bound_dy):.3f}, "
          f"dgamma {rel(err_dg, bound_dg):.3f}, dbeta {rel(err_db, bound_db):.3f}; max |dy err| {err_dy.max():.2e}, "
          f"max dgamma rel {rel(err_dg, np.abs(rdg)):.2e}, max dbeta rel {rel(err_db, np.abs(rdb)):.2e}")
    assert (err_dy <= bound_dy).all(), rel(err_dy, bound_dy)
    assert (err_dg <= bound_dg).all(), rel(err_dg, bound_dg)
    assert (err_db <= bound_db).all(), rel(err_db, bound_db)


# ---- 3. the operator's contracts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,c,pooled", [(2, 16, 16, 64, False), (3, 5, 7, 24, False), (2, 5, 7, 8, True), (2, 8, 12, 16, True)])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_operator_contracts(dtype, n, h, w, c, pooled):
    st = _ST[dtype][0]
    g = torch.Generator().manual_seed(33 + c)
    P = 3
    y = torch.randn(P * n, h, w, c, generator=g).to(st).cuda()
    da = torch.randn(P * n, h, w, c, generator=g).to(st).cuda()
    dp = torch.randn(P * n, h // 2, w // 2, c, generator=g).to(st).cuda() if pooled else None
    consts = torch.randn(P, 4, c, generator=g).cuda()
    consts[:, 3] = consts[:, 3].abs() + 0.5
    y0, da0, dp0, k0 = y[:n], da[:n], (dp[:n] if pooled else None), consts[:1]
    dy, dg, db, _ = frozen(da0, dp0, y0, k0, dtype)
    # two launches: the same bits
    dy_b, dg_b, db_b, _ = frozen(da0, dp0, y0, k0, dtype)
    assert torch.equal(dy, dy_b) and torch.equal(dg, dg_b) and torch.equal(db, db_b)
    # in place (dy == da) == out of place
    buf = da0.clone()
    dy_i, dg_i, db_i, _ = frozen(buf, dp0, y0, k0, dtype, dy=buf)
    assert dy_i.data_ptr() == buf.data_ptr()
    assert torch.equal(dy_i, dy) and torch.equal(dg_i, dg) and torch.equal(db_i, db)
    # accumulate = 1 adds to what is there (one f32 addition per channel)
    pre_g, pre_b = torch.randn(c, generator=g).cuda(), torch.randn(c, generator=g).cuda()
    _, dg_a, db_a, _ = frozen(da0, dp0, y0, k0, dtype, accumulate=1, dg=pre_g.clone(), db=pre_b.clone())
    assert torch.equal(dg_a, pre_g + dg) and torch.equal(db_a, pre_b + db)
    # dgamma == NULL: the same dy, the partials scratch untouched
    dy_n, none_g, none_b, part = frozen(da0, dp0, y0, k0, dtype, sums=False)
    assert none_g is None and none_b is None
    assert torch.equal(dy_n, dy) and bool(torch.isnan(part).all())
    # the per-pass form with 3 passes == three single calls (the passes' dgamma / dbeta added in order)
    dy_p, dg_p, db_p, _ = frozen(da, dp, y, consts, dtype, passes=P)
    dg_s = db_s = None
    for q in range(P):
        sl = slice(q * n, (q + 1) * n)
        dy_q, dg_s, db_s, _ = frozen(da[sl], dp[sl] if pooled else None, y[sl], consts[q:q + 1], dtype, accumulate=int(q > 0), dg=dg_s, db=db_s)
        assert torch.equal(dy_p[sl], dy_q), q
    assert torch.equal(dg_p, dg_s) and torch.equal(db_p, db_s)
    dy_pn, _, _, part = frozen(da, dp, y, consts, dtype, passes=P, sums=False)
    assert torch.equal(dy_pn, dy_p) and bool(torch.isnan(part).all())


def test_operator_refuses_bad_arguments():
    from ustrun import _lib as L
    lib = L.lib()
    t = torch.zeros(1, 4, 4, 8).cuda()
    k = torch.ones(4, 8).cuda()
    p = torch.zeros(2048 * 8).cuda()
    a = lambda dg, db, c: lib.ustrun_bn_bwd_frozen(t.data_ptr(), None, t.data_ptr(), k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(),
                                                   k[3].data_ptr(), 1, 4, 4, c, t.data_ptr(), dg, db, 0, p.data_ptr(), 1024 * 2 * 8 * 4, 0, None)
    assert a(k[0].data_ptr(), None, 8) != 0 and b"come together" in lib.ustrun_last_error()
    assert a(None, None, 6) != 0 and b"multiple of 4" in lib.ustrun_last_error()


# ---- 4. the network against the oracle ---------------------------------------------------------------------------------------------
def _eval_inputs(c, k, n, h, w, base, seed, bilinear=False):
    """test_gpu_input_grad._inputs, plus non-trivial running buffers: running_mean = 0.3 randn, running_var uniform in [0.5, 2], an
    arbitrary num_batches_tracked"""
    sd, x = _inputs(c, k, n, h, w, base, seed, bilinear)
    g = torch.Generator().manual_seed(seed + 2)
    for key in sd:
        if key.endswith("running_mean"):
            sd[key] = 0.3 * torch.randn(sd[key].shape, generator=g)
        elif key.endswith("running_var"):
            sd[key] = 0.5 + 1.5 * torch.rand(sd[key].shape, generator=g)
        elif key.endswith("num_batches_tracked"):
            sd[key] = torch.tensor(37, dtype=torch.long)
    return sd, x


@functools.lru_cache(maxsize=None)
def oracle_eval_grads(c, k, n, h, w, base, seed, bilinear=False):
    """{loss: {parameter key or 'x': (f32 CPU gradient, f64 gradient)}} of oracle/unet_ref.py with train=False: one f32 and one f64
    forward per shape, a backward per loss, shared by the tests below and left unchanged"""
    sd, x = _eval_inputs(c, k, n, h, w, base, seed, bilinear)
    per = []
    for dt in (torch.float32, torch.float64):
        s = {kk: (v.to(dt) if v.is_floating_point() else v.clone()) for kk, v in sd.items()}
        keys = U.param_keys(s)
        for kk in keys:
            s[kk].requires_grad_(True)
        xx = x.to(dt).requires_grad_(True)
        lg, ft = U.unet_forward(xx, s, train=False, bilinear=bilinear, feature=True)
        leaves = [s[kk] for kk in keys] + [xx]
        gr = {}
        for name, fn in LOSSES.items():
            gs = torch.autograd.grad(fn(lg, ft), leaves, retain_graph=True, allow_unused=True)
            gr[name] = {kk: (torch.zeros_like(l) if g_ is None else g_).detach() for kk, l, g_ in zip(keys + ["x"], leaves, gs)}
        per.append(gr)
    return {name: {kk: (per[0][name][kk], per[1][name][kk]) for kk in per[0][name]} for name in LOSSES}


def eval_grads(model, x, loss, x_grad=True, **kw):
    for p in model.parameters():
        p.grad = None
    xg = x.cuda().requires_grad_(x_grad)
    lg, ft = model(xg, feature=True, **kw)
    LOSSES[loss](lg, ft).backward()
    return {kk: p.grad for kk, p in model.named_parameters()}, xg.grad, lg.detach(), ft.detach()


def _buffers(model):
    return {kk: v.clone() for kk, v in model.state_dict().items() if "running_" in kk or "num_batches" in kk}


def _eval_model(c, k, n, h, w, base, seed, bilinear=False, dtype="f32"):
    sd, x = _eval_inputs(c, k, n, h, w, base, seed, bilinear)
    if bilinear:
        from networks.unet_model import UNet
        model = UNet(c, k, bilinear=True, base_channels=base, dtype=dtype)
        model.load_state_dict({kk: v.detach().clone() for kk, v in sd.items()})
        model = model.cuda()
    else:
        model = build_model(sd, c, k, base, dtype)
    model.eval_backward = True
    return model.eval(), x


def check_eval_against_oracle(c, k, n, h, w, base, seed, loss, bilinear=False):
    """test_gpu_input_grad.check_against_oracle's rule in eval mode: err_hip < max(5 err_cpu_f32, floor) against the f64 oracle for
    every parameter gradient and x.grad, floor 2e-4 (base < 64) / 1e-2 (base 64); the outputs are the existing eval forward's bit for
    bit, no running buffer and no num_batches_tracked moves, the model stays in eval mode"""
    model, x = _eval_model(c, k, n, h, w, base, seed, bilinear)
    before = _buffers(model)
    with torch.no_grad():
        lg0, ft0 = model(x.cuda(), feature=True)
    want = oracle_eval_grads(c, k, n, h, w, base, seed, bilinear)[loss]
    pg, xg, lg, ft = eval_grads(model, x, loss)
    assert torch.equal(lg, lg0) and torch.equal(ft, ft0)
    assert not model.training
    after = _buffers(model)
    assert before.keys() == after.keys() and all(torch.equal(before[kk], after[kk]) for kk in before)
    assert int(model.inc.double_conv[1].num_batches_tracked) == 37
    assert xg is not None and xg.shape == x.shape
    got = dict(pg, x=xg)
    floor = 2e-4 if base < 64 else 1e-2
    worst = (0.0, "", 0.0)
    for key, (g32, g64) in want.items():
        if float(g64.norm()) == 0.0:                     # (the head under the features-only loss)
            assert got[key] is not None and float(got[key].abs().max()) == 0.0, key
            continue
        err_hip, err_cpu = rel_l2(got[key].cpu(), g64), rel_l2(g32, g64)
        worst = max(worst, (err_hip / max(5 * err_cpu, floor), key, err_hip, err_cpu))
        if key == "x":
            print(f"eval x.grad [{loss}] {(c, k, n, h, w, base)}{' bilinear' if bilinear else ''}: HIP {err_hip:.2e}, CPU f32 {err_cpu:.2e} "
                  f"against the f64 oracle")
        assert err_hip < max(5 * err_cpu, floor), (key, err_hip, err_cpu)
    print(f"eval worst parameter [{loss}] {(c, k, n, h, w, base)}: {worst[1]} HIP {worst[2]:.2e}, CPU f32 {worst[3]:.2e} ({worst[0]:.2f} of the bar)")
    return model, x, pg, xg


NET_SHAPES = [(3, 2, 2, 32, 32, 8, 5), (1, 4, 3, 48, 32, 8, 5), (3, 2, 1, 50, 38, 8, 5), (3, 2, 2, 64, 48, 64, 12)]


@pytest.mark.parametrize("loss", ["logits", "feat", "both"])
@pytest.mark.parametrize("c,k,n,h,w,base,seed", NET_SHAPES)
def test_eval_gradients_vs_oracle(c, k, n, h, w, base, seed, loss):
    model, x, pg, xg = check_eval_against_oracle(c, k, n, h, w, base, seed, loss)
    if loss == "feat":
        assert float(pg["outc.conv.weight"].abs().max()) == 0.0 and float(pg["outc.conv.bias"].abs().max()) == 0.0


# ---- 5. parameters that require grad, an input that does not ---------------------------------------------------------------------
@pytest.mark.parametrize("train", [False, True])
def test_parameter_gradients_without_input_gradient(train):
    """parameters require grad, x does not: the node is recorded for the parameters alone -- eval mode used to return logits
    without a grad_fn, silently -- and the gradients are those of the call with x.requires_grad, bit for bit"""
    def run(x_grad):
        model, x = _eval_model(3, 2, 2, 32, 32, 8, 5)          # a fresh model: the same running buffers in front of both calls
        model.train(train)
        xg = x.cuda().requires_grad_(x_grad)
        lg, ft = model(xg, feature=True)
        assert lg.requires_grad and ft.requires_grad and lg.grad_fn is not None
        LOSSES["both"](lg, ft).backward()
        return {kk: p.grad for kk, p in model.named_parameters()}, xg.grad

    with_x, xg = run(True)
    plain, none = run(False)
    assert xg is not None and none is None
    for kk in with_x:
        assert plain[kk] is not None and torch.equal(with_x[kk], plain[kk]), kk


def test_eval_backward_is_opt_in():
    """a model that did not set eval_backward keeps the eval-mode call it had: no node for parameters that require grad, and an
    input that requires grad is refused with the switch's name; the switch changes no forward bit"""
    model, x = _eval_model(3, 2, 2, 32, 32, 8, 5)
    on = model(x.cuda())
    assert on.requires_grad
    model.eval_backward = False
    off = model(x.cuda())
    assert not off.requires_grad and torch.equal(on.detach(), off)
    with pytest.raises(NotImplementedError, match="eval_backward = True"):
        model(x.cuda().requires_grad_())
    model.train()
    assert model(x.cuda().requires_grad_()).requires_grad          # train mode never needed it


# ---- 6. frozen parameters ----------------------------------------------------------------------------------------------------------------
def _weight_gradient_tags(fn):
    """the launch profiler's records of one call of fn: how many carry a weight-gradient tag (200 + i: 3x3 layer i, 220 + j:
    ConvTranspose j), how many records in all"""
    from ustrun import _lib as L
    lib = L.lib()
    for kind in (0, 1):
        lib.ustrun_profile_collect(kind, None, None, None, None)          # start from an empty table
    lib.ustrun_profile_stream(None, 0)
    lib.ustrun_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.ustrun_profile_enable(0)
    buf = (L.ProfRec * 4096)()
    n = lib.ustrun_profile_records(buf, 4096)
    for kind in (0, 1):
        lib.ustrun_profile_collect(kind, None, None, None, None)
    assert n >= 0
    return sum(1 for r in buf[:n] if 200 <= r.tag < 224), n


@pytest.mark.parametrize("train", [False, True])
def test_frozen_parameters_input_gradient_only(train):
    """every parameter frozen, x requires grad (grads == NULL in the C ABI): x.grad is the run with parameter gradients' bit for
    bit, every p.grad stays None, and no launch carries a weight-gradient tag"""
    model, x = _eval_model(3, 2, 2, 32, 32, 8, 5)
    model.train(train)
    state = copy.deepcopy(model.state_dict())
    _, xg_full, lg_full, _ = eval_grads(model, x, "both")
    tagged, total = _weight_gradient_tags(lambda: eval_grads(model, x, "both"))
    readable = tagged > 0                               # the tags are readable from here: the full backward shows its own
    model.load_state_dict(state)                        # (train mode: the running buffers the first call started from)
    for p in model.parameters():
        p.requires_grad_(False)
    res = []
    tagged0, total0 = _weight_gradient_tags(lambda: res.append(eval_grads(model, x, "both")))
    _, xg, lg, _ = res[0]
    assert torch.equal(lg, lg_full)
    assert xg is not None and torch.equal(xg, xg_full)
    assert all(p.grad is None for p in model.parameters())
    print(f"input-only backward ({'train' if train else 'eval'}): {tagged0} weight-gradient launches of {total0} profiled "
          f"(with parameter gradients: {tagged} of {total})")
    if readable:
        assert tagged0 == 0 and 0 < total0 < total


def test_c_abi_refuses_a_backward_with_nothing_to_compute():
    """grads == NULL needs dx or a part that ends before layer 0 (1 or 3); with dx it runs, in eval mode and in train mode"""
    import ctypes as C
    from ustrun import _lib as L
    from ustrun import engine
    lib = L.lib()
    for train in (False, True):
        model, x = _eval_model(3, 2, 2, 32, 32, 8, 5)
        model.train(train)
        xc = x.cuda()
        with torch.no_grad():
            logits, _, ws, d = engine._run_forward(model, xc, False)
        dl = torch.ones_like(logits)
        scratch = torch.empty(lib.ustrun_unet_bwd_scratch_bytes(C.byref(d)), dtype=torch.uint8, device="cuda")
        call = lambda part, dx: lib.ustrun_unet_backward_io(C.byref(d), xc.data_ptr(), dl.data_ptr(), None, ws.data_ptr(), scratch.data_ptr(),
                                                           None, 0, part, L.ptr(dx), _stream())
        assert call(0, None) != 0 and b"nothing to compute" in lib.ustrun_last_error()
        assert call(2, None) != 0 and b"nothing to compute" in lib.ustrun_last_error()
        dx = torch.full_like(xc, float("nan"))
        assert call(1, None) == 0 and call(2, dx) == 0          # head + decoder, then the encoder down to dx
        dx0 = torch.full_like(xc, float("nan"))
        assert call(0, dx0) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dx0).all()) and torch.equal(dx, dx0)


# ---- 7. 16-bit storage and f32x3 in eval mode against the f32 network in eval mode -------------------------------------------
def _calibrated(c, k, base, dtype, sd, x):
    """the network with running statistics = the batch's own (one train-mode forward at momentum 1): a trained model's situation"""
    from networks.unet_model import UNet
    m = UNet(c, k, base_channels=base, dtype=dtype)
    m.load_state_dict({kk: v.clone() for kk, v in sd.items()})
    m = m.cuda().train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.momentum = 1.0
    with torch.no_grad():
        m(x.cuda())
    m.eval_backward = True
    return m.eval()


@functools.lru_cache(maxsize=None)
def f32_eval_reference(c, k, n, h, w, base):
    """(state dict with calibrated running buffers, x, the f32 eval network's x.grad, its x.grad at the input rounded to bf16):
    test_gpu_input_grad.f32_reference's construction in eval mode"""
    torch.manual_seed(21)
    sd = U.make_state_dict(c, k, base=base)
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(22))
    m = _calibrated(c, k, base, "f32", sd, x)
    sd = {kk: v.detach().cpu().clone() for kk, v in m.state_dict().items()}
    res = []
    for xin in (x, x.to(torch.bfloat16).float()):
        xg = xin.cuda().requires_grad_()
        m(xg).square().mean().backward()
        res.append(xg.grad.cpu())
    return sd, x, res[0], res[1]


@pytest.mark.parametrize("c,k,n,h,w,base", [(3, 2, 2, 64, 64, 64), (1, 4, 2, 48, 32, 16)])
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32x3"])
def test_low_precision_eval_input_gradient_tracks_f32(dtype, c, k, n, h, w, base):
    """test_low_precision_input_gradient_tracks_f32's rule in eval mode: x.grad against the f32 HIP network on the same weights and
    running buffers, held to that network's own response to ONE bf16 rounding of the input: max(YARD_X * yardstick, 3e-3)"""
    from networks.unet_model import UNet
    sd, x, g32, g32r = f32_eval_reference(c, k, n, h, w, base)
    m = UNet(c, k, base_channels=base, dtype=dtype)
    m.load_state_dict({kk: v.clone() for kk, v in sd.items()})
    m = m.cuda().eval()
    m.eval_backward = True
    xg = x.cuda().requires_grad_()
    m(xg).square().mean().backward()
    err, yard = rel_l2(xg.grad.cpu(), g32), rel_l2(g32r, g32)
    print(f"eval x.grad {dtype} vs f32 {(c, k, n, h, w, base)}: error {err:.3e}, yardstick {yard:.3e}, ratio {err / max(yard, 1e-30):.2f}")
    assert err < max(YARD_X * yard, 3e-3), (err, yard)


# ---- 8. plan variants in eval mode ---------------------------------------------------------------------------------------------------
def _randomise_buffers(model, g):
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(0.3 * torch.randn(mod.num_features, generator=g))
                mod.running_var.copy_(0.5 + 1.5 * torch.rand(mod.num_features, generator=g))
                mod.weight.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.num_features, generator=g) * 0.1)


def test_eval_backward_in_parts_equals_one_call():
    """parts 1 | 3 | 4 with dfeat and dx == the single call, bit for bit (bf16, base 16, 32 x 32)"""
    from networks.unet_model import UNet
    torch.manual_seed(7)
    m1 = UNet(3, 2, base_channels=16, dtype="bf16")
    _randomise_buffers(m1, torch.Generator().manual_seed(3))
    m1 = m1.cuda().eval()
    m1.eval_backward = True
    m2 = copy.deepcopy(m1)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 32, 32, generator=g).cuda()
    dl = torch.randn(2, 2, 32, 32, generator=g).cuda()
    df = torch.randn(2, 16, 32, 32, generator=g).cuda()
    fired = []
    m2._ustrun_backward_split_hook = lambda: fired.append(1)
    m2._ustrun_backward_mid_hook = lambda: fired.append(3)
    grads = []
    for m in (m1, m2):
        xg = x.clone().requires_grad_()
        lg, ft = m(xg, feature=True)
        torch.autograd.backward([lg, ft], [dl, df])
        grads.append(xg.grad)
    assert fired == [1, 3]
    assert torch.equal(grads[0], grads[1])
    for (kk, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert p1.grad is not None and torch.equal(p1.grad, p2.grad), kk


def test_eval_passes_with_lead_and_tail():
    """forward_batched(groups = 3, lead = 1, tail = 1) in eval mode: the gradient passes' rows of dx equal separate calls to 1e-5,
    the leading and the tail rows are zero; the parameter gradients are the two passes' sum"""
    from networks.unet_model import UNet
    torch.manual_seed(29)
    m1 = UNet(3, 2, base_channels=16, dtype="f32")
    _randomise_buffers(m1, torch.Generator().manual_seed(4))
    m1 = m1.cuda().eval()
    m1.eval_backward = True
    m2 = copy.deepcopy(m1)
    g = torch.Generator().manual_seed(12)
    n = 2
    x = torch.randn(3 * n + 1, 3, 40, 40, generator=g).cuda()
    dl = torch.randn(3 * n, 2, 40, 40, generator=g).cuda()
    xg = x.clone().requires_grad_()
    lg = m1.forward_batched(xg, 3, tail=1, lead=1)
    assert lg.shape[0] == 3 * n
    lg.backward(dl)
    assert xg.grad.shape == x.shape
    assert float(xg.grad[:n].abs().max()) == 0.0 and float(xg.grad[3 * n:].abs().max()) == 0.0
    for q in (1, 2):
        xs = x[q * n:(q + 1) * n].clone().requires_grad_()
        out = m2(xs)
        assert rel_l2(lg[q * n:(q + 1) * n].detach().cpu(), out.detach().cpu()) < 1e-5
        out.backward(dl[q * n:(q + 1) * n])
        e = rel_l2(xg.grad[q * n:(q + 1) * n].cpu(), xs.grad.cpu())
        assert e < 1e-5, (q, e)
    for (kk, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert rel_l2(p1.grad.cpu(), p2.grad.cpu()) < 1e-5, kk


def test_eval_bilinear_vs_oracle():
    check_eval_against_oracle(3, 2, 2, 32, 48, 8, 11, "both", bilinear=True)


def test_eval_domain_specific_batchnorm():
    """UNet(num_domains = 2) in eval mode, domain_label = 1: the call's domain selects the running statistics, its members get the
    gradients, domain 0's stay None, and every value is the plain network's carrying domain 1's members and buffers, bit for bit"""
    from networks.unet_model import UNet
    torch.manual_seed(41)
    plain = UNet(3, 2, base_channels=16)
    torch.manual_seed(41)
    ds = UNet(3, 2, base_channels=16, num_domains=2)
    g = torch.Generator().manual_seed(8)
    _randomise_buffers(ds, g)
    sd = {}
    for kk, v in ds.state_dict().items():
        if ".bns." in kk:
            head, rest = kk.split(".bns.")
            d_, name = rest.split(".", 1)
            if int(d_) == 1:
                sd[f"{head}.{name}"] = v.clone()
        else:
            sd[kk] = v.clone()
    plain.load_state_dict(sd)
    plain, ds = plain.cuda().eval(), ds.cuda().eval()
    plain.eval_backward = ds.eval_backward = True
    before = _buffers(ds)
    x = torch.randn(2, 3, 32, 32, generator=g).cuda()
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    la, fa = plain(xa, feature=True)
    (la.square().mean() + fa.square().mean()).backward()
    lb, fb = ds(xb, feature=True, domain_label=torch.tensor([1, 0]))
    (lb.square().mean() + fb.square().mean()).backward()
    assert torch.equal(la, lb) and torch.equal(fa, fb) and torch.equal(xa.grad, xb.grad)
    got = dict(ds.named_parameters())
    seen = 0
    for kk, p in plain.named_parameters():
        parts = kk.split(".")
        if parts[-2] in ("1", "4") and "double_conv" in kk:            # a BatchNorm: domain 1's member carries the gradient
            k1 = ".".join(parts[:-1] + ["bns", "1", parts[-1]])
            k0 = ".".join(parts[:-1] + ["bns", "0", parts[-1]])
            assert got[k0].grad is None, k0
            assert torch.equal(p.grad, got[k1].grad), kk
            seen += 1
        else:
            assert torch.equal(p.grad, got[kk].grad), kk
    assert seen == 36
    after = _buffers(ds)
    assert all(torch.equal(before[kk], after[kk]) for kk in before) and not ds.training


# ---- 9. the stand-alone blocks ---------------------------------------------------------------------------------------------------------
def _block_reference(m, ins):
    """the same torch modules in float64 on the CPU, eval mode, through their ATen forward (unet_parts.py:8-68)"""
    import torch.nn.functional as F
    from networks.unet_parts import DoubleConv, Down
    r = copy.deepcopy(m).cpu().double().eval()
    xs = [t.detach().cpu().double().requires_grad_(True) for t in ins]
    if isinstance(r, DoubleConv):
        out = r.double_conv(xs[0])
    elif isinstance(r, Down):
        out = r.maxpool_conv[1].double_conv(r.maxpool_conv[0](xs[0]))
    else:
        x1 = r.up(xs[0])
        dy_, dx_ = xs[1].shape[2] - x1.shape[2], xs[1].shape[3] - x1.shape[3]
        x1 = F.pad(x1, [dx_ // 2, dx_ - dx_ // 2, dy_ // 2, dy_ - dy_ // 2])
        out = r.conv.double_conv(torch.cat([xs[1], x1], 1))
    out.square().mean().backward()
    return r, xs, out


@pytest.mark.parametrize("name", ["doubleconv_3_8", "down_8_16_odd", "up_16_8"])
def test_block_eval_backward(name):
    """eval-mode backward of DoubleConv(3, 8), Down(8, 16) at an odd extent and Up(16, 8) against the same torch modules in float64 on
    the CPU, at the tolerances tests/test_gpu_blocks.py holds their train-mode twins to (output rtol 2e-4 / atol 2e-5, input
    gradients rtol 2e-3 / atol 2e-6, parameter gradients rtol 2e-3 / atol 5e-6)"""
    from networks.unet_parts import DoubleConv, Down, Up
    from test_gpu_blocks import close
    torch.manual_seed(17)
    g = torch.Generator().manual_seed(18)
    if name == "doubleconv_3_8":
        m, ins = DoubleConv(3, 8), [torch.randn(2, 3, 12, 10, generator=g)]
    elif name == "down_8_16_odd":
        m, ins = Down(8, 16), [torch.randn(2, 8, 13, 11, generator=g)]
    else:
        m, ins = Up(16, 8, bilinear=False), [torch.randn(2, 16, 6, 5, generator=g), torch.randn(2, 8, 13, 11, generator=g)]
    _randomise_buffers(m, g)
    m = m.cuda().eval()
    before = _buffers(m)
    ref, rxs, rout = _block_reference(m, ins)
    xs = [t.cuda().requires_grad_(True) for t in ins]
    out = m(*xs)
    close(out, rout.detach().numpy())
    out.square().mean().backward()
    for x, rx in zip(xs, rxs):
        close(x.grad, rx.grad.numpy(), rtol=2e-3, atol=2e-6)
    for (kk, p), (_, rp) in zip(m.named_parameters(), ref.named_parameters()):
        close(p.grad, rp.grad.numpy(), rtol=2e-3, atol=5e-6)
    after = _buffers(m)
    assert all(torch.equal(before[kk], after[kk]) for kk in before) and not m.training
