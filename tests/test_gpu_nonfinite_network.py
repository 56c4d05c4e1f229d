"""f16 overflow through the whole engine: it is FOUND (a value that leaves half's range poisons flat_g, where ustrun_amp_check
looks), and it leaves NOTHING BEHIND (the gradient sink is overwritten, not `0 * old + new`; no workspace, split-K slab or statistics
row carries a NaN into the next call).

U-Net (base_channels 64 at 2 x 3 x 32 x 32: the production kernel families), train mode, loss = (logits * R).sum() with a fixed finite
R, so no label logic ever sees a special value; gradients go to a flat sink laid out as ustrun.trainer.flat_like lays it out
(model._ustrun_grad_sink), found_inf is read by ustrun_amp_check on that sink.  Every comparison is bit equality between two runs
of the same code, or the 0 / 1 of found_inf.

The premise of each forward-overflow case is checked on the CPU: oracle.unet_ref in float64 on the half-rounded weights, every
convolution's output tapped; the poisoned layer's weight is scaled by the smallest power of two that takes that output past
2 x 65504 (a power of two scales a float64 convolution exactly, so one clean oracle run serves all layers) while the scaled weight
itself still fits half.  Expected, by the reference's semantics (a half convolution output of inf, BatchNorm of it NaN, GradScaler
skips): found_inf == 1.

"Sink overwrite" pre-fills every PARAMETER's view of the sink with NaN; the alignment gaps between the views keep flat_like's zeros
(no kernel may write there, and a NaN there would make amp_check skip every step) and are part of the bit comparison."""
import math

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

N, CIN, K, HW = 2, 3, 2, 32
BASE = 64
HALF_MAX = 65504.0
FORWARD_LAYERS = ["inc.double_conv.0.weight", "inc.double_conv.3.weight", "down4.maxpool_conv.1.double_conv.3.weight", "up1.up.weight",
                  "up4.conv.double_conv.0.weight"]


def _inputs():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, CIN, HW, HW, generator=g)
    R = torch.randn(N, K, HW, HW, generator=g)
    return x, R


class _Tap:
    """torch.nn.functional with the two convolutions recording max |output| under the weight tensor's identity"""

    def __init__(self):
        self.peak = {}

    def __getattr__(self, name):
        return getattr(TF, name)

    def conv2d(self, x, w, *a, **k):
        y = TF.conv2d(x, w, *a, **k)
        self.peak[id(w)] = float(y.detach().abs().max())
        return y

    def conv_transpose2d(self, x, w, *a, **k):
        y = TF.conv_transpose2d(x, w, *a, **k)
        self.peak[id(w)] = float(y.detach().abs().max())
        return y


_ORACLE = {}


def _oracle_peaks(base):
    """{weight key: max |that convolution's output|} of the clean float64 forward on half-rounded weights and input, and the
    state_dict (float32) both sides start from"""
    if base not in _ORACLE:
        from oracle import unet_ref as U
        torch.manual_seed(1)
        sd = U.make_state_dict(CIN, K, base=base)
        x, _ = _inputs()
        sd64 = {k: (v.half().double() if v.is_floating_point() and v.dim() == 4 else v.double() if v.is_floating_point() else v.clone())
                for k, v in sd.items()}
        tap, keep = _Tap(), U.F
        U.F = tap
        try:
            with torch.no_grad():
                U.unet_forward(x.half().double(), sd64, train=True)
        finally:
            U.F = keep
        _ORACLE[base] = (sd, {k: tap.peak[id(v)] for k, v in sd64.items() if id(v) in tap.peak})
    return _ORACLE[base]


class Net:
    """one model object, its flat gradient sink, and clean / poisoned runs on it"""

    def __init__(self, dtype, base=BASE):
        from networks.unet_model import UNet
        from ustrun.trainer import flat_like
        self.sd, self.peaks = _oracle_peaks(base)
        m = UNet(CIN, K, base_channels=base, dtype=dtype)
        m.load_state_dict({k: v.clone() for k, v in self.sd.items()})
        self.model = m.cuda().train()
        self.saved = {k: v.clone() for k, v in self.model.state_dict().items()}
        params = list(self.model.parameters())
        total = sum((p.numel() + 3) // 4 * 4 for p in params)
        self.flat, self.views = flat_like(torch.empty(total, dtype=torch.float32, device="cuda"), params)
        self.gap = torch.ones(total, dtype=torch.bool, device="cuda")
        o = 0
        for p in params:
            self.gap[o:o + p.numel()] = False
            o += (p.numel() + 3) // 4 * 4
        assert bool(self.gap.any()), "this layout has no alignment gap: the sink test would not see one written"
        self.model._ustrun_grad_sink = self.views
        x, R = _inputs()
        self.x, self.R = x.cuda(), R.cuda()

    def restore(self):
        from ustrun import engine
        self.model.load_state_dict(self.saved)            # weights and the BatchNorm running buffers
        engine.invalidate_packed(self.model)

    def run(self, x=None, R=None, scale_weight=None, prefill=None):
        """-> (logits, flat gradient sink, found_inf), after restoring weights and running buffers"""
        from ustrun import engine
        self.restore()
        if scale_weight is not None:
            key, factor = scale_weight
            with torch.no_grad():
                self.model.get_parameter(key).mul_(factor)
            engine.invalidate_packed(self.model)
        if prefill is not None:
            self.flat.zero_()
            for v in self.views:
                v.fill_(prefill)
        self.model._ustrun_sink_fresh = True
        logits = self.model(self.x if x is None else x)
        (logits * (self.R if R is None else R)).sum().backward()
        return logits.detach().clone(), self.flat.clone(), found_inf(self.flat)


def found_inf(flat):
    from ustrun import _lib as L
    state = torch.zeros(8, dtype=torch.float32, device="cuda")
    L.check(L.lib().ustrun_amp_check(flat.data_ptr(), flat.numel(), state.data_ptr(), torch.cuda.current_stream().cuda_stream),
            "ustrun_amp_check")
    return int(state[3].item())


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


_NETS = {}


def net(dtype):
    if dtype not in _NETS:
        _NETS[dtype] = Net(dtype)
    return _NETS[dtype]


def overflow_factor(n, key):
    """the smallest power of two that takes the layer's float64 output past 2 x 65504; the scaled weight must still fit half"""
    k = math.floor(math.log2(2 * HALF_MAX / n.peaks[key])) + 1
    assert n.peaks[key] * 2.0 ** k > 2 * HALF_MAX
    assert float(n.sd[key].abs().max()) * 2.0 ** k < HALF_MAX, "the scaled weight itself would overflow half"
    return 2.0 ** k


def test_clean_runs_are_deterministic_and_finite():
    n = net("f16")
    la, ga, fa = n.run()
    lb, gb, fb = n.run()
    assert fa == 0 and fb == 0 and bool(torch.isfinite(la).all())
    assert same_bits(la, lb), "two clean forwards differ"
    assert same_bits(ga, gb), "two clean backwards differ in %d gradients" % int((ga.view(torch.int32) != gb.view(torch.int32)).sum())
    assert not bool(ga[n.gap].any())


@pytest.mark.parametrize("key", FORWARD_LAYERS)
def test_forward_overflow_is_found(key):
    n = net("f16")
    f = overflow_factor(n, key)
    logits, g, found = n.run(scale_weight=(key, f))
    print("%s x %g: oracle peak %.4g, %d non-finite logits, %d non-finite gradients" %
          (key, f, n.peaks[key] * f, int((~torch.isfinite(logits)).sum()), int((~torch.isfinite(g)).sum())))
    assert found == 1, "a convolution output past 2 x 65504 in half left a finite flat_g: the step would not be skipped"


def test_backward_overflow_is_found():
    n = net("f16")
    logits, g, found = n.run(R=n.R * 2.0 ** 40)
    assert bool(torch.isfinite(logits).all())
    assert found == 1


def test_sink_is_overwritten_not_scaled():
    n = net("f16")
    _, g0, f0 = n.run(prefill=0.0)
    _, g1, f1 = n.run(prefill=float("nan"))
    assert f0 == 0
    assert not bool(g1[n.gap].any()), "an alignment gap of the sink was written"
    assert f1 == 0 and same_bits(g0, g1), "%d sink entries differ after a NaN pre-fill" % int((g0.view(torch.int32) != g1.view(torch.int32)).sum())


def _residue(n, poisoned):
    la, ga, fa = n.run()
    assert fa == 0
    for kw in poisoned:
        assert n.run(**kw)[2] == 1
    lb, gb, fb = n.run()
    assert fb == 0, "NaN left behind by a poisoned run: %d non-finite gradients" % int((~torch.isfinite(gb)).sum())
    assert same_bits(la, lb), "the logits after the poisoned runs differ from those before"
    assert same_bits(ga, gb), "%d gradients after the poisoned runs differ from those before" % int((ga.view(torch.int32) != gb.view(torch.int32)).sum())


def test_nothing_left_behind_f16():
    n = net("f16")
    key = FORWARD_LAYERS[0]
    _residue(n, [dict(scale_weight=(key, overflow_factor(n, key))), dict(R=n.R * 2.0 ** 40)])


def test_nothing_left_behind_bf16():
    """bf16 overflows at 3.4e38: an inf in the input image (a floating operand of the first convolution) instead of a scaled weight,
    and an inf in the logits' gradient (a floating operand of the head's backward) instead of a scaled R"""
    n = net("bf16")
    x, R = n.x.clone(), n.R.clone()
    x[1, 2, 17, 5] = float("inf")
    R[0, 1, 9, 30] = float("inf")
    _residue(n, [dict(x=x), dict(R=R)])


# ---- DeepLabV2 through resnet_engine: its own sink logic (foreach copy / add), weight gradients on a side stream -------------------------
class DeepLab:
    def __init__(self):
        from networks.deeplabv2 import DeepLabV2
        from ustrun.trainer import flat_like
        torch.manual_seed(5)
        self.model = DeepLabV2("resnet50", K, pretrained=False, dtype="f16").cuda().train()
        self.saved = {k: v.clone() for k, v in self.model.state_dict().items()}
        params = list(self.model.parameters())
        total = sum((p.numel() + 3) // 4 * 4 for p in params)
        self.flat, self.views = flat_like(torch.empty(total, dtype=torch.float32, device="cuda"), params)
        self.gap = torch.ones(total, dtype=torch.bool, device="cuda")
        o = 0
        for p in params:
            self.gap[o:o + p.numel()] = False
            o += (p.numel() + 3) // 4 * 4
        self.model._ustrun_grad_sink = self.views
        g = torch.Generator().manual_seed(12)
        self.x = torch.randn(2, 3, 64, 64, generator=g).cuda()
        # (a sum-reduced loss through fifty default-init residual blocks overflows half near |R| = 64, tests/test_gpu_deeplab_bwd.py)
        self.R = (torch.randn(2, K, 64, 64, generator=g) / 256).cuda()

    def run(self, R=None, prefill=None, x=None):
        from ustrun import engine
        self.model.load_state_dict(self.saved)
        engine.invalidate_packed(self.model)
        if prefill is not None:
            self.flat.zero_()
            for v in self.views:
                v.fill_(prefill)
        self.model._ustrun_sink_fresh = True
        out = self.model(self.x if x is None else x)
        (out * (self.R if R is None else R)).sum().backward()
        torch.cuda.synchronize()
        return out.detach().clone(), self.flat.clone(), found_inf(self.flat)


def test_deeplab_sink_overwrite_and_nothing_left_behind():
    n = DeepLab()
    la, ga, fa = n.run(prefill=0.0)
    lb, gb, fb = n.run(prefill=0.0)
    assert fa == 0 and fb == 0, "the clean DeepLabV2 backward is not finite at |R| / 256: the premise of this case fails"
    assert same_bits(la, lb) and same_bits(ga, gb), "two clean DeepLabV2 runs differ"
    _, g1, f1 = n.run(prefill=float("nan"))
    assert f1 == 0 and same_bits(ga, g1), "%d sink entries differ after a NaN pre-fill" % int((ga.view(torch.int32) != g1.view(torch.int32)).sum())
    assert not bool(ga[n.gap].any()) and not bool(g1[n.gap].any()), "an alignment gap of the sink was written"
    x = n.x.clone()
    x[1, 2, 33, 5] = float("inf")                 # the forward group: an inf in the image, a floating operand of the stem convolution
    assert n.run(x=x)[2] == 1, "an inf in the image left a finite flat_g"
    assert n.run(R=n.R * 2.0 ** 40)[2] == 1
    lc, gc, fc = n.run()
    assert fc == 0 and same_bits(la, lc) and same_bits(ga, gc), "the run after an overflowing backward differs from the one before"
