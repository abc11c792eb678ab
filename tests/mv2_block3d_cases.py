"""Shared by tests/test_mv2_block3d_cpu.py, tests/test_gpu_mv2_block3d.py and tests/golden/make_golden_msnet3d.py (a plain module, no
fixtures): the cases of MobileStereoNet's 3-D inverted-residual block, their seeded parameters and inputs, and a torch restatement of the
block (stereo/modeling/models/msnet/submodule.py:136-173) with the reference's `self.conv` Sequential layout, so that state_dict keys match:

    conv = [Conv3d(inp, hid, 1), BN, ReLU6, Conv3d(hid, hid, 3, stride, 1, groups=hid), BN, ReLU6, Conv3d(hid, oup, 1), BN]
    y = conv(x) (+ x when stride == 1 and inp == oup)

The tolerance rule: err(X) = max |X - float64 restatement| on the same inputs, and every checked tensor X must satisfy
err(X) <= 8 * err(float32 restatement).  The factor 8, as in tests/mr_volume_cases.py: the engine sums K in another order (two halves of
every 8 channels interleaved on the matrix unit, the 27 taps row by row), and a maximum over thousands of elements is noisy.

A test of this block passes vacuously when ReLU6 never clamps or when relu6(shift1) is zero (the padding of the hidden tensor could then
be taken for a padding of x), so reference() asserts for the float64 run: outside the two degenerate cases at least 5 % of each hidden
pre-activation lies below 0 and at least 5 % above 6; in every case at least 25 % of the expansion's folded shifts are positive.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msnet3d_blocks.npz")
FACTOR = 8.0

# case -> (B, Cin, Cout, stride, ratio, D, H, W): the smallest shapes at which the kernel can still go wrong
CASES = {
    "res": (2, 32, 32, 1, 2, 5, 11, 19),      # residual, batch stride, more planes than ring slots, more than one tile along w, ragged tiles
    "g40": (1, 40, 32, 1, 3, 4, 9, 17),       # Cin = 40 and Chid = 120: the K and N edges of the matrix tiles
    "s2odd": (1, 32, 64, 2, 2, 7, 13, 21),    # stride 2 on odd sizes, zero plane D
    "s2even": (1, 64, 128, 2, 2, 6, 12, 20),  # stride 2 on even sizes
    "wide": (1, 128, 128, 1, 2, 3, 5, 9),     # Chid = 256, the largest ring
    "tiny": (1, 32, 32, 1, 2, 2, 3, 3),       # a volume smaller than one tile, D < 3
    "s2one": (1, 32, 64, 2, 2, 1, 4, 5),      # D = 1
    # beyond the issue's seven: the launcher cuts d into chunks of at least 8 output planes once there are 16, and a chunk re-expands the
    # input planes below its first output plane
    "chunk": (1, 32, 32, 1, 2, 17, 5, 9),     # two chunks of 9 and 8 planes, residual
    "s2chunk": (1, 32, 64, 2, 2, 33, 4, 5),   # stride 2: 17 output planes in two chunks
}
GOLDEN_CASES = ("g40", "s2odd")
DEGENERATE = ("tiny", "s2one")


class Block(nn.Module):
    """submodule.py:136-173 restated; `stride` is the int MSNet3D.py passes.  (The reference compares it with (1, 1, 1), so its own blocks
    never add x; the restatement adds x at stride 1 and equal channels, which is what the engine's `residual` argument is tested with.)"""

    def __init__(self, inp, oup, stride, ratio):
        super().__init__()
        self.stride = stride
        hid = round(inp * ratio)
        self.use_res_connect = stride == 1 and inp == oup
        dw = [nn.Conv3d(hid, hid, 3, stride, 1, groups=hid, bias=False), nn.BatchNorm3d(hid), nn.ReLU6(inplace=True),
              nn.Conv3d(hid, oup, 1, 1, 0, bias=False), nn.BatchNorm3d(oup)]
        self.conv = nn.Sequential(*dw) if ratio == 1 else nn.Sequential(nn.Conv3d(inp, hid, 1, 1, 0, bias=False), nn.BatchNorm3d(hid), nn.ReLU6(inplace=True), *dw)

    def forward(self, x):
        return x + self.conv(x) if self.use_res_connect else self.conv(x)


def seed_parameters(module, g):
    """conv weights ~ N(0,1) * 1.5 * sqrt(2 / fan_in), BN weight ~ U(0.5, 2), bias ~ N(0,1), running mean ~ 0.5 N(0,1), running var ~ U(0.5, 2):
    in the order of module.modules(), from the generator g"""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (nn.Conv3d, nn.ConvTranspose3d)):
                fan_in = m.weight[0].numel() if isinstance(m, nn.Conv3d) else m.weight[:, 0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 1.5 * (2.0 / fan_in) ** 0.5)
            elif isinstance(m, nn.BatchNorm3d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 1.5 + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.5 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) * 1.5 + 0.5)
    return module


def make_block(case, dtype=torch.float32):
    """the case's block with its seeded parameters, in eval mode on the CPU"""
    B, Ci, Co, stride, ratio, D, H, W = CASES[case]
    g = torch.Generator().manual_seed(3000 + list(CASES).index(case))
    return seed_parameters(Block(Ci, Co, stride, ratio), g).to(dtype).eval()


def make_input(case, dtype=torch.float32):
    """seeded x ~ 2 N(0,1), contiguous NCDHW on the CPU"""
    B, Ci, Co, stride, ratio, D, H, W = CASES[case]
    g = torch.Generator().manual_seed(4000 + list(CASES).index(case))
    return (2.0 * torch.randn(B, Ci, D, H, W, generator=g)).to(dtype)


def out_shape(case):
    B, Ci, Co, stride, ratio, D, H, W = CASES[case]
    o = lambda n: (n - 1) // stride + 1
    return (B, Co, o(D), o(H), o(W))


def _assert_not_vacuous(case, blk, x):
    pre = []
    hooks = [blk.conv[i].register_forward_hook(lambda m, a, out: pre.append(out.detach().clone())) for i in (1, 4)]   # before the in-place ReLU6
    with torch.no_grad():
        y = blk(x)
    for h in hooks:
        h.remove()
    bn = blk.conv[1]
    shift = bn.bias - bn.running_mean * bn.weight / torch.sqrt(bn.running_var + bn.eps)
    assert float((shift > 0).double().mean()) >= 0.25, f"{case}: too few positive expansion shifts"
    if case not in DEGENERATE:
        for i, t in enumerate(pre):
            lo, hi = float((t < 0).double().mean()), float((t > 6).double().mean())
            assert lo >= 0.05 and hi >= 0.05, f"{case}: hidden pre-activation {i} has {lo:.1%} below 0 and {hi:.1%} above 6"
    return y


_cache = {}


def reference(case, dtype, x=None):
    """-> the restatement's output in `dtype` on the case's input (or on x); the case's own run is computed once and not modified by the tests"""
    if x is not None:
        with torch.no_grad():
            return make_block(case, dtype)(x.to(dtype))
    key = (case, dtype)
    if key not in _cache:
        blk, xin = make_block(case, dtype), make_input(case, dtype)
        if dtype == torch.float64:
            _cache[key] = _assert_not_vacuous(case, blk, xin)
        else:
            with torch.no_grad():
                _cache[key] = blk(xin)
    return _cache[key]


def err(x, ref64):
    return float((x.detach().double().cpu() - ref64).abs().max())


def check(what, x, ref64, ref32):
    """the tolerance rule; both numbers in the message"""
    assert tuple(x.shape) == tuple(ref64.shape), f"{what}: shape {tuple(x.shape)}, expected {tuple(ref64.shape)}"
    e, e32 = err(x, ref64), err(ref32, ref64)
    print(f"{what}: err {e:.3e}, fp32 restatement {e32:.3e}")
    assert e <= FACTOR * e32, f"{what}: err {e:.3e} > {FACTOR:g} x {e32:.3e} (the fp32 restatement's error)"
