"""Shared by tests/test_mv2_block3d_cpu.py, tests/test_gpu_mv2_block3d.py and tests/golden/make_golden_msnet3d.py (a plain module, no
fixtures): the cases of MobileStereoNet's 3-D inverted-residual block, their seeded parameters and inputs, and a torch restatement of the
block (stereo/modeling/models/msnet/submodule.py:136-173) with the reference's `self.conv` Sequential layout, so that state_dict keys match:

    conv = [Conv3d(inp, hid, 1), BN, ReLU6, Conv3d(hid, hid, 3, stride, 1, groups=hid), BN, ReLU6, Conv3d(hid, oup, 1), BN]
    y = conv(x) (+ x when stride == 1 and inp == oup)

The tolerance rule, what reference() asserts about the cases, and everything else that does not depend on the rank: tests/mv2_cases_common.py.
"""
from __future__ import annotations

import os
import sys

import torch
import torch.nn as nn

from mv2_cases_common import FACTOR, check, err, seed_parameters  # noqa: F401  (the tests and tools reach them through this module)
import mv2_cases_common as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msnet3d_blocks.npz")

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


def reference(case, dtype, x=None):
    """-> the restatement's output in `dtype` on the case's input (or on x); the case's own run is computed once and not modified by the tests"""
    return C.reference(sys.modules[__name__], case, dtype, x)
