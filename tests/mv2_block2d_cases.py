"""Shared by tests/test_mv2_block2d_cpu.py, tests/test_gpu_mv2_block2d.py and tests/golden/make_golden_msnet2d.py (a plain module, no
fixtures): the cases of MobileStereoNet's 2-D inverted-residual block, their seeded parameters and inputs, and a torch restatement of the
block (stereo/modeling/models/msnet/submodule.py:94-133) with the reference's `self.conv` Sequential layout, so that state_dict keys match:

    conv = [Conv2d(inp, hid, 1), BN, ReLU6, Conv2d(hid, hid, 3, stride, dilation, dilation, groups=hid), BN, ReLU6, Conv2d(hid, oup, 1), BN]
    y = conv(x) (+ x when stride == 1 and inp == oup)

reference() also restates the two epilogues with which MSNet2D follows a block (MSNet2D.py:42-43, 86-93): y + addend, then relu.

The tolerance rule: err(X) = max |X - float64 restatement| on the same inputs, and every checked tensor X must satisfy
err(X) <= 8 * err(float32 restatement).  The factor 8, as in tests/mv2_block3d_cases.py: the engine sums K in another order (four quarters
of every 16 channels interleaved on the matrix unit, the hidden channels in chunks of 48), and a maximum over thousands of elements is
noisy.

A test of this block passes vacuously when ReLU6 never clamps or when relu6(shift1) is zero (the padding of the hidden tensor could then
be taken for a padding of x), so reference() asserts for the float64 run: outside the degenerate cases at least 5 % of each hidden
pre-activation lies below 0 and at least 5 % above 6; in every case at least 25 % of the expansion's folded shifts are positive.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msnet2d_blocks.npz")
FACTOR = 8.0

# case -> (B, Cin, Cout, stride, ratio, H, W): the smallest shapes at which the kernel can still go wrong.  The kernel's tiles are 8 x 16,
# 4 x 8 and 4 x 4 outputs at stride 1, 4 x 8 and 4 x 4 at stride 2; it takes the largest that leaves at least 128 workgroups, else 4 x 4;
# the hidden channels go in chunks of 48.
CASES = {
    "dres": (2, 48, 48, 1, 3, 11, 19),        # residual, batch stride, Ch = 144 (not a multiple of 32), ragged tiles, more than one tile along w
    "g40": (1, 40, 32, 1, 3, 9, 17),          # Ci = 40, Ch = 120: K and N edges, a last hidden chunk (24) that is not full
    "s2odd": (1, 48, 96, 2, 2, 13, 21),       # stride 2 on odd sizes
    "s2even": (1, 96, 192, 2, 2, 12, 20),     # stride 2 on even sizes; the bottom / right zero row is never read
    "wide": (1, 192, 192, 1, 2, 5, 9),        # Ch = 384, the limits, residual
    "first": (1, 32, 32, 1, 3, 6, 37),        # firstconv's shape, several tiles along w
    "tall": (1, 48, 48, 1, 2, 37, 5),         # more rows than any tile or chunk of rows
    "tiny": (1, 48, 48, 1, 2, 3, 3),          # a map smaller than one tile
    "s2one": (1, 48, 96, 2, 2, 1, 5),         # H = 1
    "s2two": (1, 48, 96, 2, 2, 2, 2),         # a 1 x 1 output
    # beyond the issue's ten: the cases above all have fewer than 128 tiles of any size and so run on 4 x 4 tiles; each larger tile needs
    # a map with at least 128 of them
    "t8x16": (1, 32, 32, 1, 3, 67, 261),      # 9 x 17 = 153 tiles of 8 x 16, ragged on both axes, residual, two hidden chunks
    "t4x8": (1, 40, 40, 1, 2, 37, 101),       # 35 tiles of 8 x 16 but 10 x 13 = 130 of 4 x 8, residual, Ch = 80: chunks of 48 and 32
    "s2t4x8": (1, 32, 40, 2, 2, 73, 203),     # stride 2: 37 x 102 outputs in 10 x 13 = 130 tiles of 4 x 8, odd sizes
}
GOLDEN_CASES = ("g40", "s2odd")
DEGENERATE = ("tiny", "s2one", "s2two")


class Block(nn.Module):
    """submodule.py:94-133 restated"""

    def __init__(self, inp, oup, stride, ratio, dilation=1):
        super().__init__()
        self.stride = stride
        hid = int(inp * ratio)
        self.use_res_connect = stride == 1 and inp == oup
        dw = [nn.Conv2d(hid, hid, 3, stride, dilation, dilation=dilation, groups=hid, bias=False), nn.BatchNorm2d(hid), nn.ReLU6(inplace=True),
              nn.Conv2d(hid, oup, 1, 1, 0, bias=False), nn.BatchNorm2d(oup)]
        self.conv = nn.Sequential(*dw) if ratio == 1 else nn.Sequential(nn.Conv2d(inp, hid, 1, 1, 0, bias=False), nn.BatchNorm2d(hid), nn.ReLU6(inplace=True), *dw)

    def forward(self, x):
        return x + self.conv(x) if self.use_res_connect else self.conv(x)


def seed_parameters(module, g):
    """conv weights ~ N(0,1) * 1.5 * sqrt(2 / fan_in), BN weight ~ U(0.5, 2), bias ~ N(0,1), running mean ~ 0.5 N(0,1), running var ~ U(0.5, 2):
    in the order of module.modules(), from the generator g"""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                fan_in = m.weight[0].numel() if isinstance(m, nn.Conv2d) else m.weight[:, 0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 1.5 * (2.0 / fan_in) ** 0.5)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 1.5 + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.5 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) * 1.5 + 0.5)
    return module


def make_block(case, dtype=torch.float32):
    """the case's block with its seeded parameters, in eval mode on the CPU"""
    B, Ci, Co, stride, ratio, H, W = CASES[case]
    g = torch.Generator().manual_seed(3100 + list(CASES).index(case))
    return seed_parameters(Block(Ci, Co, stride, ratio), g).to(dtype).eval()


def make_input(case, dtype=torch.float32):
    """seeded x ~ 2 N(0,1), contiguous NCHW on the CPU"""
    B, Ci, Co, stride, ratio, H, W = CASES[case]
    g = torch.Generator().manual_seed(4100 + list(CASES).index(case))
    return (2.0 * torch.randn(B, Ci, H, W, generator=g)).to(dtype)


def out_shape(case):
    B, Ci, Co, stride, ratio, H, W = CASES[case]
    o = lambda n: (n - 1) // stride + 1
    return (B, Co, o(H), o(W))


def make_addend(case, dtype=torch.float32):
    """seeded addend ~ 4 N(0,1) of the output's shape (of the output's magnitude, so that the ReLU behind the sum clips a good part)"""
    g = torch.Generator().manual_seed(5100 + list(CASES).index(case))
    return (4.0 * torch.randn(*out_shape(case), generator=g)).to(dtype)


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


def reference(case, dtype, x=None, addend=None, relu=False):
    """-> the restatement's relu?(block(x) (+ addend)) in `dtype` on the case's input (or on x); the case's own run is computed once and not
    modified by the tests (the epilogues make new tensors)"""
    if x is not None:
        with torch.no_grad():
            y = make_block(case, dtype)(x.to(dtype))
    else:
        key = (case, dtype)
        if key not in _cache:
            blk, xin = make_block(case, dtype), make_input(case, dtype)
            if dtype == torch.float64:
                _cache[key] = _assert_not_vacuous(case, blk, xin)
            else:
                with torch.no_grad():
                    _cache[key] = blk(xin)
        y = _cache[key]
    if addend is not None:
        y = y + addend.to(dtype)
    return torch.relu(y) if relu else y


def err(x, ref64):
    return float((x.detach().double().cpu() - ref64).abs().max())


def check(what, x, ref64, ref32):
    """the tolerance rule; both numbers in the message"""
    assert tuple(x.shape) == tuple(ref64.shape), f"{what}: shape {tuple(x.shape)}, expected {tuple(ref64.shape)}"
    e, e32 = err(x, ref64), err(ref32, ref64)
    print(f"{what}: err {e:.3e}, fp32 restatement {e32:.3e}")
    assert e <= FACTOR * e32, f"{what}: err {e:.3e} > {FACTOR:g} x {e32:.3e} (the fp32 restatement's error)"
