"""Cases, inputs and fp64 references of the disparity-variance heads, shared by tests/golden/make_golden_variance.py (which measures the
reference's own fp32 error on them and stores it), tests/test_variance_head_cpu.py and tests/test_gpu_variance_head.py.

The measure is the reference's `disparity_variance(x, maxdisp, disparity)` (models/cfnet/submodule.py:128-134 ==
models/igevpp/submodule.py:153-159): sum_d x[:, d] * (d - disparity)^2, keepdim.  `regression` / `variance` below are that arithmetic in
torch, so that the tests run where the reference is not mounted; the generator checks them against the reference's functions bit for bit.

A case is one input shape of one head form.  Its three cost distributions share one `randn` base (stored once):
  flat   the base
  mid    one plane per pixel raised by 8, anywhere in the range
  sharp  one plane per pixel raised by 40, in the top sixth of the range -- the variance is small and sits at a large disparity: the
         regime in which E[d^2] - E[d]^2 in fp32 loses five digits
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disparity_variance.npz")
DISTS = {"flat": 0.0, "mid": 8.0, "sharp": 40.0}

# fused upsample form: name -> (cost shape [B,Dl,Hl,Wl], (D, h, w), align_corners)
FUSED = {
    "x4": ((2, 48, 5, 18), (192, 20, 72), False),          # x4 streaming kernel: a partial 64-wide tile, five row tiles, two batches
    "x4_dl1": ((1, 1, 3, 17), (4, 12, 68), False),         # first plane is the last plane
    "x4_dl2": ((1, 2, 3, 17), (8, 12, 68), False),
    "x4_dl3": ((1, 3, 3, 17), (12, 12, 68), False),
    "gen_ac": ((2, 16, 6, 19), (64, 23, 70), True),        # generic (LDS) kernel, PSMNet's align_corners=True
    "gen_nac": ((1, 12, 5, 9), (40, 17, 31), False),       # generic kernel at a size that is no multiple of the input
}
# logits form and (through softmax in fp64, rounded to fp32) probabilities form: name -> cost shape [B,D,H,W]
PLAIN = {"d48": (2, 48, 7, 33), "d5": (1, 5, 3, 65)}


def case_seed(name):
    return 1000 + sorted(list(FUSED) + list(PLAIN)).index(name)


def make_inputs(name):
    """-> dict of the arrays a case stores: the cost base, the raised plane per pixel for `mid` / `sharp`, the loss weights a, b, and for
    the probabilities form a disparity map that is not the mean plus an unnormalised volume."""
    shape = FUSED[name][0] if name in FUSED else PLAIN[name]
    B, D, H, W = shape
    r = np.random.default_rng(case_seed(name))
    out = {"base": r.normal(0, 1, shape).astype(np.float32),
           "idx_mid": r.integers(0, D, (B, 1, H, W)).astype(np.int64),
           "idx_sharp": r.integers(D - max(1, D // 6), D, (B, 1, H, W)).astype(np.int64)}
    oh, ow = FUSED[name][1][1:] if name in FUSED else (H, W)
    out["a"] = r.normal(0, 1, (B, oh, ow)).astype(np.float32)
    out["b"] = r.normal(0, 1, (B, oh, ow)).astype(np.float32)
    if name in PLAIN:
        out["given_disp"] = r.uniform(0, D - 1, (B, 1, H, W)).astype(np.float32)
        out["prob_unnorm"] = r.uniform(0, 2, shape).astype(np.float32)
    return out


def cost_of(arrs, dist):
    """the fp32 cost of one distribution from a case's stored arrays (exact: one fp32 addition per raised element)"""
    c = torch.from_numpy(np.asarray(arrs["base"])).clone()
    if DISTS[dist]:
        c.scatter_add_(1, torch.from_numpy(np.asarray(arrs["idx_" + dist])), torch.full((1,), DISTS[dist]).expand(c.shape[0], 1, *c.shape[2:]).contiguous())
    return c


def prob_of(cost):
    """probabilities-form input of a distribution: the fp64 softmax of its cost, rounded to fp32"""
    return torch.softmax(cost.double(), 1).float()


def own_mean(prob):
    """the given disparity of the probabilities-form distribution cases: the volume's fp64 mean, rounded to fp32, [B,1,H,W]"""
    return regression(prob.double(), prob.shape[1]).float().unsqueeze(1)


def regression(x, maxdisp):
    """cfnet/submodule.py:121-125"""
    d = torch.arange(0, maxdisp, dtype=x.dtype, device=x.device).view(1, maxdisp, 1, 1)
    return torch.sum(x * d, 1, keepdim=False)


def variance(x, maxdisp, disparity):
    """cfnet/submodule.py:128-134; disparity [B,1,H,W] -> [B,1,H,W]"""
    d = torch.arange(0, maxdisp, dtype=x.dtype, device=x.device).view(1, maxdisp, 1, 1)
    return torch.sum(x * (d - disparity) ** 2, 1, keepdim=True)


def compose_fused(cost, D, h, w, align, regression=regression, variance=variance):
    """F.interpolate(trilinear) -> softmax -> regression / variance, in cost's dtype -> (disp, var) [B,h,w]"""
    p = F.softmax(F.interpolate(cost[:, None], [D, h, w], mode="trilinear", align_corners=align).squeeze(1), dim=1)
    disp = regression(p, D)
    return disp, variance(p, D, disp.unsqueeze(1)).squeeze(1)


def compose_logits(cost, regression=regression, variance=variance):
    p = F.softmax(cost, dim=1)
    disp = regression(p, cost.shape[1])
    return disp, variance(p, cost.shape[1], disp.unsqueeze(1)).squeeze(1)


def compose_prob(prob, disparity, regression=regression, variance=variance):
    return regression(prob, prob.shape[1]), variance(prob, prob.shape[1], disparity).squeeze(1)


def var_err(var, var64):
    """the issue's metric: max over ALL pixels |var - var64| / (1 + var64)"""
    return float(((var.double() - var64).abs() / (1.0 + var64)).max())


def grad_err(g, g64):
    return float((g.double() - g64).abs().max() / g64.abs().max())


def bar(e_ref):
    """variance bar: 4 x the reference's own fp32 error; fp32 rounding of the result alone reaches 1e-7, so never below 4e-7"""
    return 4.0 * max(float(e_ref), 1e-7)


def grad_bar(e_ref_grad):
    """gradient bar: 4 x the reference's own fp32 autograd error, with no floor"""
    return 4.0 * float(e_ref_grad)


def loss_grads(fn, leaves, a, b):
    """gradients of sum(a * disp) + sum(b * var) w.r.t. `leaves` (fresh leaf copies)"""
    xs = [t.detach().clone().requires_grad_() for t in leaves]
    disp, var = fn(*xs)
    (torch.sum(a.to(disp.dtype) * disp) + torch.sum(b.to(var.dtype) * var)).backward()
    return [x.grad for x in xs]


def load_golden():
    return np.load(GOLDEN)
