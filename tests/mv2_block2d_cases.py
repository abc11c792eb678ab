"""Shared by tests/test_mv2_block2d_cpu.py, tests/test_gpu_mv2_block2d.py and tests/golden/make_golden_msnet2d.py (a plain module, no
fixtures): the cases of MobileStereoNet's 2-D inverted-residual block, their seeded parameters and inputs, and a torch restatement of the
block (stereo/modeling/models/msnet/submodule.py:94-133) with the reference's `self.conv` Sequential layout, so that state_dict keys match:

    conv = [Conv2d(inp, hid, 1), BN, ReLU6, Conv2d(hid, hid, 3, stride, dilation, dilation, groups=hid), BN, ReLU6, Conv2d(hid, oup, 1), BN]
    y = conv(x) (+ x when stride == 1 and inp == oup)

reference() also restates the two epilogues with which MSNet2D follows a block (MSNet2D.py:42-43, 86-93): y + addend, then relu.

The tolerance rule, what reference() asserts about the cases, and everything else that does not depend on the rank: tests/mv2_cases_common.py.
"""
from __future__ import annotations

import os
import sys

import torch
import torch.nn as nn

from mv2_cases_common import FACTOR, check, err, seed_parameters  # noqa: F401  (the tests and tools reach them through this module)
import mv2_cases_common as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msnet2d_blocks.npz")

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


def reference(case, dtype, x=None, addend=None, relu=False):
    """-> the restatement's relu?(block(x) (+ addend)) in `dtype` on the case's input (or on x); the case's own run is computed once and not
    modified by the tests (the epilogues make new tensors)"""
    y = C.reference(sys.modules[__name__], case, dtype, x)
    if addend is not None:
        y = y + addend.to(dtype)
    return torch.relu(y) if relu else y
