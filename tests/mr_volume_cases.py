"""Shared by tests/test_mr_volume_cpu.py, tests/test_gpu_mr_volume.py and tests/golden/make_golden_mr_volume.py (a plain module, no
fixtures): the cases of IGEV++'s multi-range cost volumes, their seeded inputs and a torch restatement of the composition they replace,

    gwc[b,g,d,h,w] = (1/K) sum_k L[b,gK+k,h,w] R[b,gK+k,h,w-d]     (w >= d, else 0)
    V0 = gwc[:, :, :S]     V1 = conv3d(gwc[:, :, :M], P0, stride (k0,1,1))     V2 = conv3d(gwc, P1, stride (k1,1,1))

written from these formulas as a slice-assign loop plus F.conv3d, in float32 or float64.

The tolerance rule: err(X) = max |X - float64 restatement| on the same inputs, and every checked tensor X must satisfy
err(X) <= 8 * err(float32 restatement), per output.  The factor 8: the engine sums in another order (the k chain inside a group, then g,
then j), and a maximum over a few thousand elements is noisy.  V0 is not under the rule: it equals gwc_volume(L, R, D, 8)[:, :, :S] bit
for bit.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "igevpp_volumes.npz")
G = 8
FACTOR = 8.0

# case -> (B, C, H, W, D, S, M, k0, k1): the smallest shapes at which the kernels can still go wrong
CASES = {
    "small": (2, 96, 3, 40, 32, 8, 16, 2, 4),     # K = 12, batch stride, the masked edge w = k d' + j crossing a patch
    "narrow": (1, 32, 2, 13, 24, 6, 12, 2, 4),    # W < D: whole planes and whole patches zero, one partial pixel tile
    "equal": (1, 32, 2, 37, 16, 16, 16, 2, 4),    # S = M = D, odd width
    "k44": (1, 8, 2, 21, 16, 4, 8, 4, 4),         # K = 1, both patches of size 4, S < k
    "tile": (1, 32, 1, 70, 48, 12, 24, 2, 4),     # more than one pixel tile per row, ring wrap over 48 planes
    "k3": (1, 24, 2, 21, 12, 4, 8, 2, 2),         # a K the kernels have no register form for (neither 4 nor 12), k1 = 2, D < one step of 16 planes
}
GOLDEN_CASES = ("small", "narrow")
NAMES = ("V0", "V1", "V2")
GRAD_NAMES = ("dL", "dR", "dP0", "dP1")


def inputs(case, dtype=torch.float32):
    """seeded (L, R, P0, P1) on the CPU: features ~ N(0, 1), patch weights ~ N(0, 1) / sqrt(8 k) (a Conv3d's scale)"""
    B, C, H, W, D, S, M, k0, k1 = CASES[case]
    g = torch.Generator().manual_seed(1000 + list(CASES).index(case))
    L, R = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    P0 = torch.randn(G, G, k0, 1, 1, generator=g) / (G * k0) ** 0.5
    P1 = torch.randn(G, G, k1, 1, 1, generator=g) / (G * k1) ** 0.5
    return tuple(t.to(dtype) for t in (L, R, P0, P1))


def out_grads(case, dtype=torch.float32):
    """seeded gradients of the three outputs"""
    B, C, H, W, D, S, M, k0, k1 = CASES[case]
    g = torch.Generator().manual_seed(2000 + list(CASES).index(case))
    return tuple(torch.randn(B, G, n, H, W, generator=g).to(dtype) for n in (S, M // k0, D // k1))


def gwc(L, R, D):
    B, C, H, W = L.shape
    K = C // G
    vol = L.new_zeros(B, G, D, H, W)
    for d in range(min(D, W)):
        vol[:, :, d, :, d:] = (L[..., d:] * R[..., :W - d]).view(B, G, K, H, W - d).mean(2)
    return vol


def restatement(L, R, P0, P1, D, S, M):
    """the composition in the tensors' dtype -> (V0, V1, V2)"""
    vol = gwc(L, R, D)
    k0, k1 = P0.shape[2], P1.shape[2]
    return vol[:, :, :S].contiguous(), F.conv3d(vol[:, :, :M], P0, stride=(k0, 1, 1)), F.conv3d(vol, P1, stride=(k1, 1, 1))


_cache = {}


def reference(case, dtype):
    """-> (outputs, gradients) of the restatement in `dtype` on the case's inputs, the gradients through autograd for out_grads(case) over
    all three outputs; computed once per (case, dtype) and not modified by the tests"""
    key = (case, dtype)
    if key not in _cache:
        B, C, H, W, D, S, M, k0, k1 = CASES[case]
        leaves = [t.clone().requires_grad_() for t in inputs(case, dtype)]
        outs = restatement(*leaves, D, S, M)
        grads = torch.autograd.grad(outs, leaves, out_grads(case, dtype))
        _cache[key] = (tuple(o.detach() for o in outs), tuple(grads))
    return _cache[key]


def err(x, ref64):
    return float((x.detach().double().cpu() - ref64).abs().max())


def check(what, x, ref64, ref32):
    """the tolerance rule; both numbers in the message"""
    assert tuple(x.shape) == tuple(ref64.shape), f"{what}: shape {tuple(x.shape)}, expected {tuple(ref64.shape)}"
    e, e32 = err(x, ref64), err(ref32, ref64)
    print(f"{what}: err {e:.3e}, fp32 restatement {e32:.3e}")
    assert e <= FACTOR * e32, f"{what}: err {e:.3e} > {FACTOR:g} x {e32:.3e} (the fp32 restatement's error)"
