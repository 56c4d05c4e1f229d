"""A skipped step of the f16 trainer, through the real kernels: the backward overflows under a loss scale of 2^40, ustrun_amp_check
finds it in flat_g, the optimizer step is skipped (parameters and momentum keep their bits, the EMA line still runs, the scale
halves), and the NEXT step is an ordinary one -- nothing of the overflow survives in flat_g, the gradient sink, the split-K slabs or
the statistics rows.  Both routes of the student's backward: the batched call and the four accumulating calls (batch_passes=False).

Special values reach only floating operands here (the scaled loss gradient and what the backward makes of it): the forward, and with
it every pseudo-label and class index, is the clean one.  The one borrowed bar is that of ustrun_sgd_ema_scaled in
tests/test_gpu_step_tail_ops.py (step_tail_ref.sgd_ema), for the momentum buffer of the step after the skip (and, from the same
call of that reference, its parameters and EMA teacher); everything else is bit equality or an exact count."""
import random

import numpy as np
import pytest
import torch

import step_tail_ref as R
from test_gpu_bn_forward_ops import hold
from test_gpu_step import synth

pytestmark = pytest.mark.gpu

B, H, C, K, BASE = 2, 32, 3, 2, 8
KW = dict(max_iterations=300, threshold=0.52, patch_size=H, num_eval_iter=2)


def _trainer(batch_passes):
    from networks.unet_model import UNet
    from oracle import unet_ref as U
    from ustrun.trainer import SSLTrainer
    torch.manual_seed(1)
    sd_s, sd_t = U.make_state_dict(C, K, base=BASE), U.make_state_dict(C, K, base=BASE)
    stu, tea = UNet(C, K, base_channels=BASE, dtype="f16"), UNet(C, K, base_channels=BASE, dtype="f16")
    stu.load_state_dict({k: v.clone() for k, v in sd_s.items()})
    tea.load_state_dict({k: v.clone() for k, v in sd_t.items()})
    tr = SSLTrainer("fundus", stu.cuda(), tea.cuda(), batch_passes=batch_passes, **KW)
    assert tr.scaler is not None and tr.batch_passes == batch_passes
    return tr


def _bits(t):
    return t.detach().clone().view(torch.int32)


@pytest.mark.parametrize("batch_passes", [True, False], ids=["batched", "unbatched"])
def test_overflowing_backward_skips_one_step_and_leaves_nothing_behind(batch_passes):
    batches = [[t.cuda() for t in synth("fundus", B, C, H, 100 + s)] for s in range(2)]
    # the twin: the same first batch under the default scale (its step is an ordinary one)
    twin = _trainer(batch_passes)
    random.seed(7); np.random.seed(7)
    twin.step(*batches[0], epoch_start=True)
    twin_loss = twin.scalars()["loss"]
    assert twin.scaler.skipped_steps() == (0, 1)

    tr = _trainer(batch_passes)
    tr.scaler.state[:2] = 2.0 ** 40
    p0, v0, t0 = tr.flat_p.clone(), tr.flat_v.clone(), tr.flat_t.clone()
    alpha1 = min(1 - 1 / (tr.iter_num + 1), tr.ema_decay)
    random.seed(7); np.random.seed(7)
    tr.step(*batches[0], epoch_start=True)

    # ---- step 1: found, skipped
    assert not bool(torch.isfinite(tr.flat_g).all()), "a backward scaled by 2^40 left a finite flat_g: the overflow was saturated or dropped"
    assert tr.scaler.skipped_steps() == (1, 1)
    st = tr.scaler.state.cpu()
    assert float(st[0]) == 2.0 ** 39 and float(st[1]) == 2.0 ** 39 and float(st[3]) == 0.0
    assert torch.equal(_bits(tr.flat_p), _bits(p0)) and torch.equal(_bits(tr.flat_v), _bits(v0))
    # the EMA line still runs on the unchanged p: t' = alpha t + (1 - alpha) p in float32, bit for bit.  At the trainer's first
    # iteration alpha = min(1 - 1 / 1, decay) = 0, so every float32 operation of the kernel's expression is exact: fl(0 t) = 0,
    # fl(1 p) = p, fl(0 + p) = p (t finite)
    assert alpha1 == 0.0 and bool(torch.isfinite(t0).all())
    a32 = torch.tensor(alpha1, dtype=torch.float32)
    want_t = a32 * t0.cpu() + (torch.tensor(1.0) - a32) * p0.cpu()
    assert torch.equal(tr.flat_t.cpu(), want_t) and torch.equal(want_t, p0.cpu())
    loss1 = tr.scalars()["loss"]
    assert np.isfinite(loss1) and loss1 == twin_loss, (loss1, twin_loss)

    # ---- step 2: an ordinary step
    tr.scaler.state[:2] = 65536.0
    lr2, alpha2 = tr.lr, min(1 - 1 / (tr.iter_num + 1), tr.ema_decay)
    p1, t1 = tr.flat_p.clone(), tr.flat_t.clone()
    tr.step(*batches[1], epoch_start=False)
    assert tr.scaler.skipped_steps() == (1, 2)
    assert bool(torch.isfinite(tr.flat_g).all()), "%d non-finite gradients after the skipped step" % int((~torch.isfinite(tr.flat_g)).sum())
    assert float(tr.flat_g.abs().max()) > 0 and not torch.equal(tr.flat_p, p1)
    assert float(tr.scaler.state[0]) == 65536.0 and np.isfinite(tr.scalars()["loss"])
    # torch's SGD after ITS first step holds v = g / scale + wd p; first_step was cleared by the skipped step, so the kernel
    # computes mu * v0 + that with the untouched v0 = 0
    assert not tr.first_step and not bool(v0.any())
    (rp, rv, rtt), (ep, ev, ett) = R.sgd_ema(p1.cpu().numpy(), tr.flat_g.cpu().numpy(), v0.cpu().numpy(), t1.cpu().numpy(), lr2,
                                             tr.momentum, tr.wd, 0, alpha2, 1.0, scale=65536.0)
    g64 = tr.flat_g.double().cpu().numpy() * (np.float32(1.0) / np.float32(65536.0))
    np.testing.assert_array_equal(rv, g64 + np.float64(np.float32(tr.wd)) * p1.double().cpu().numpy())     # = torch's first step
    hold("step after the skip: momentum", tr.flat_v.double().cpu().numpy(), rv, ev)
    hold("step after the skip: parameters", tr.flat_p.double().cpu().numpy(), rp, ep)
    hold("step after the skip: EMA teacher", tr.flat_t.double().cpu().numpy(), rtt, ett)
