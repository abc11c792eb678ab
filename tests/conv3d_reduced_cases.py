"""Shared by tests/test_conv3d_reduced_cpu.py, tests/test_gpu_conv3d_reduced.py and tests/golden/make_golden_conv3d_reduced.py (a plain
module, no fixtures): the cases, the seeded parameters and inputs, a torch restatement of FoundationStereo's Conv3dNormActReduced
(foundationstereo/core/submodule.py:87-112, fast_foundationstereo/core/submodule.py:90-115) and the tolerance rule.

The restatement keeps the reference's attribute names (conv1 and conv2: a Sequential of convolution, norm and ReLU each), so its state_dict
keys are the reference's and the engine's mirror grafts onto it.  It also runs in float64.

The tolerance rule, as in tests/disparity_attention_cases.py: err(X) = max |X - float64 restatement| on the same inputs, and the kernel must
satisfy err(X) <= 8 * err(float32 restatement); both numbers are printed.  The factor 8 is the one the project uses for kernels that sum in
another order (here: the channels of every tap in the order 0-3, 8-11, .. | 4-7, 12-15, .. of the matrix unit's two lane halves, tap after tap).

A test of this module passes vacuously when a ReLU never clips or always does, or when the hidden planes outside [0, D) might as well be
relu(t1) as zero, so reference() asserts on the float64 run of every case: between 20 % and 80 % of the pre-activations of either ReLU are
negative, and at least a quarter of the hidden channels have relu(t1) > 0.1, t1 being what the first norm makes of a zero convolution sum
plus bias -- the value a wrong disparity padding would put there.

Seeds: conv weights ~ 1.25 N(0,1) / sqrt(fan_in), conv biases ~ 0.5 N(0,1), BatchNorm weight ~ U(0.5, 2), bias and running mean
~ 0.5 N(0,1), running variance ~ U(0.5, 2), in the order of module.modules() from one generator per case; x ~ N(0,1).
"""
import math
import os

import torch
import torch.nn as nn

FACTOR = 8.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv3d_reduced.npz")

# case: (B, Ci, Ch, Co, ks, kd, D, H, W)
CASES = {
    "fs": (2, 28, 28, 28, 3, 17, 20, 5, 9),                # the model's block; batch stride; channel padding; ragged tile
    "short": (1, 28, 28, 28, 3, 17, 5, 3, 4),              # the window never fills
    "d1": (1, 28, 28, 28, 3, 17, 1, 2, 3),                 # one plane
    "full": (1, 32, 32, 32, 3, 17, 17, 8, 16),             # no padding anywhere; exactly one tile
    "plus1": (1, 8, 20, 12, 3, 5, 7, 9, 17),               # unequal channels; kd = 5; one pixel past a tile in both directions
    "k1": (1, 16, 16, 16, 1, 3, 4, 2, 2),                  # ks = 1
    "long": (1, 28, 28, 28, 3, 17, 104, 2, 3),             # the model's D; D cut into segments
    "many": (1, 28, 28, 28, 3, 17, 18, 33, 130),           # many tiles in both directions
}
GOLDEN_CASES = ("fs", "short", "plus1")
SEED = 20261021


class Conv3dNormActReduced(nn.Module):
    def __init__(self, C_in, C_out, hidden=None, kernel_size=3, kernel_disp=None, stride=1, norm=nn.BatchNorm3d):
        super().__init__()
        kernel_disp = kernel_size if kernel_disp is None else kernel_disp
        hidden = C_out if hidden is None else hidden
        self.conv1 = nn.Sequential(nn.Conv3d(C_in, hidden, kernel_size=(1, kernel_size, kernel_size), padding=(0, kernel_size // 2, kernel_size // 2), stride=(1, stride, stride)),
                                   norm(hidden), nn.ReLU())
        self.conv2 = nn.Sequential(nn.Conv3d(hidden, C_out, kernel_size=(kernel_disp, 1, 1), padding=(kernel_disp // 2, 0, 0), stride=(stride, 1, 1)), norm(C_out), nn.ReLU())

    def forward(self, x):
        return self.conv2(self.conv1(x))


def seed_parameters(module, g):
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.Conv3d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 1.25 / math.sqrt(m.in_channels * math.prod(m.kernel_size)))
                m.bias.copy_(0.5 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, nn.BatchNorm3d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 1.5 + 0.5)
                m.bias.copy_(0.5 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.5 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 1.5 + 0.5)
    return module


def _generator(case):
    return torch.Generator().manual_seed(SEED + list(CASES).index(case))


def ctor_args(case):
    B, Ci, Ch, Co, ks, kd, D, H, W = CASES[case]
    return dict(C_in=Ci, C_out=Co, hidden=Ch, kernel_size=ks, kernel_disp=kd)


def make_module(case, dtype=torch.float32, **kw):
    """the seeded restatement of the case in eval mode (kw overrides constructor arguments: the parameters are drawn in the same order)"""
    return seed_parameters(Conv3dNormActReduced(**{**ctor_args(case), **kw}), _generator(case)).to(dtype).eval()


def make_input(case, dtype=torch.float32):
    B, Ci, Ch, Co, ks, kd, D, H, W = CASES[case]
    g = _generator(case)
    g.manual_seed(g.initial_seed() + 1000)
    return torch.randn((B, Ci, D, H, W), generator=g).to(dtype)


def out_shape(case):
    B, Ci, Ch, Co, ks, kd, D, H, W = CASES[case]
    return (B, Co, D, H, W)


def _assert_not_vacuous(case, mod, x):
    neg = []
    hooks = [seq[2].register_forward_pre_hook(lambda m, a: neg.append(float((a[0] < 0).double().mean()))) for seq in (mod.conv1, mod.conv2)]
    with torch.no_grad():
        y = mod(x)
        t1 = torch.relu(mod.conv1[1](mod.conv1[0].bias.reshape(1, -1, 1, 1, 1))).flatten()     # the hidden value of a zero convolution sum
    for h in hooks:
        h.remove()
    share = float((t1 > 0.1).double().mean())
    print(f"{case}: {neg[0]:.1%} and {neg[1]:.1%} of the pre-activations negative, relu(t1) > 0.1 on {share:.1%} of the hidden channels")
    assert all(0.2 <= n <= 0.8 for n in neg), f"{case}: {neg[0]:.1%} / {neg[1]:.1%} of the pre-activations of the two ReLUs are negative (wanted 20 % .. 80 %)"
    assert share >= 0.25, f"{case}: relu(t1) > 0.1 on {share:.1%} of the hidden channels only: a wrong disparity padding would hardly show"
    return y


_cache = {}


def reference(case, dtype):
    """-> the restatement's output in `dtype`, [B,Co,D,H,W] contiguous; computed once per (case, dtype) and not modified by the tests"""
    key = (case, dtype)
    if key not in _cache:
        mod, x = make_module(case, dtype), make_input(case, dtype)
        if dtype == torch.float64:
            _cache[key] = _assert_not_vacuous(case, mod, x).contiguous()
        else:
            with torch.no_grad():
                _cache[key] = mod(x).contiguous()
    return _cache[key]


def err(x, ref64):
    return float((x.detach().double().cpu() - ref64).abs().max())


def check(what, x, ref64, ref32):
    """the tolerance rule; both numbers in the message"""
    assert tuple(x.shape) == tuple(ref64.shape), f"{what}: shape {tuple(x.shape)}, expected {tuple(ref64.shape)}"
    e, e32 = err(x, ref64), err(ref32, ref64)
    print(f"{what}: err {e:.3e}, fp32 restatement {e32:.3e}")
    assert e <= FACTOR * e32, f"{what}: err {e:.3e} > {FACTOR:g} x {e32:.3e} (the fp32 restatement's error)"


def pack_args(mod):
    """the arguments osa_native.conv3d_reduced_pack takes: weights, biases and the eval-mode BatchNorm folds"""
    from openstereo_amd.engine import bn_scale_shift
    (c1, n1, _), (c2, n2, _) = mod.conv1, mod.conv2
    return (c1.weight, c1.bias, *bn_scale_shift(n1), c2.weight, c2.bias, *bn_scale_shift(n2))


class Entered:
    """counts how often `module.conv1` was entered: the torch composition ran"""

    def __init__(self, module):
        self.n = 0
        self.hook = module.conv1.register_forward_pre_hook(self._hit)

    def _hit(self, *a):
        self.n += 1

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.hook.remove()
