"""IGEV++'s multi-range lookup (osa_geo_lookup_mr_f32 / _nhwc_f32 / _bwd_acc_f32) at the IGEV++ evaluation map -- B = 1, 136 x 240 at 1/4,
C = 8, D0 = D1 = D2 = 48, two levels, radius 4 -- against two baselines on the same GPU in the same process:
  (a) the torch composition of the lookup (2 L + 2 grid_sample calls, their coordinate tensors, the concatenations; autograd for the backward),
  (b) what the single-pyramid kernel allows: three geo_lookup calls on fake pyramids (volume 0 + corr; volume 1 as a fake level 1; volume 2 as
      a fake level 2) and the slicing that produces the same four tensors; for the backward three geo_lookup_bwd_acc calls on the same fake
      pyramids with the upstream gradients scattered into their interleaved layout.
Every variant is warmed up, then timed in alternating rounds (device events around CALLS calls each); the table gives the median round and the
spread.  (b) must equal the one-launch results bit for bit, and the one launch the float64 composition within the lookup / gradient tolerances, at
this size, or the script fails.
    python tools/bench_lookup_multirange.py [--rounds 7] [--calls 200] [--out FILE.md]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from openstereo_amd import _ext                 # noqa: E402
import multirange_cases as M                    # noqa: E402  (the contract in torch: M.lookup)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_lookup_multirange: no GPU visible; there is nothing to time without one")

dev = "cuda"
B, H, W, C, D, L, r = 1, 136, 240, 8, 48, 2, 4
T = 2 * r + 1
g = torch.Generator().manual_seed(0)
rn = lambda *s: torch.randn(*s, generator=g).to(dev)
geo0 = [rn(B, H, W, C, D >> l) for l in range(L)]
v1, v2 = rn(B, H, W, C, D), rn(B, H, W, C, D)
cor = [rn(B, H, W, W >> l) * 0.4 for l in range(L)]
src = geo0 + [v1, v2] + cor
disp = (torch.rand(B, H, W, generator=g) * 4 * D).to(dev)               # reaches the ends of all three ranges (disp / 4 < D2)
cx = torch.arange(W).float().view(1, 1, W).repeat(B, H, 1).to(dev)
counts = (L * C * T, C * T, C * T, L * T)
douts = [rn(B, n, H, W) for n in counts]
ext = _ext.load()
per = (C + 1) * T

# ---- forward variants
outs = [torch.empty(B, n, H, W, device=dev) for n in counts]
cls = [torch.empty(B, H, W, (n + 3) // 4 * 4, device=dev) for n in counts]
o1, o2, o3 = (torch.empty(B, per * n, H, W, device=dev) for n in (L, 2, 3))


def fwd_mr():
    ext.geo_lookup_mr(src, disp, cx, outs, C, r)
    return outs


def fwd_mr_cl():
    ext.geo_lookup_mr_nhwc(src, disp, cx, cls, [t.shape[-1] for t in cls], [B, H, W], C, r)
    return cls


def fwd_three():
    ext.geo_lookup(geo0 + cor, disp, cx, o1, C, r)
    ext.geo_lookup([geo0[0], v1, cor[0], cor[1]], disp, cx, o2, C, r)
    ext.geo_lookup([geo0[0], geo0[1], v2, cor[0], cor[1], cor[1]], disp, cx, o3, C, r)
    a = o1.view(B, L, per, H, W)
    return (a[:, :, :C * T].reshape(B, L * C * T, H, W), o2[:, per:per + C * T].contiguous(), o3[:, 2 * per:2 * per + C * T].contiguous(),
            a[:, :, C * T:].reshape(B, L * T, H, W))


def fwd_torch():
    with torch.no_grad():
        return M.lookup(src, disp.view(B, 1, H, W), cx.view(B, H, W, 1), L, r)


# ---- backward variants (gradients of all 2 L + 2 sources, accumulated)
acc = [torch.zeros_like(t) for t in src]
acc_b = [torch.zeros_like(t) for t in src]
dummy = [torch.zeros_like(t) for t in (geo0[0], geo0[1], cor[0], cor[1], cor[1])]        # what the fake levels of (b) receive and nobody wants
d2, d3 = torch.zeros(B, per * 2, H, W, device=dev), torch.zeros(B, per * 3, H, W, device=dev)
leaves = [t.clone().requires_grad_() for t in src]


def bwd_mr():
    ext.geo_lookup_mr_bwd_acc(acc, disp, cx, douts, C, r)
    return acc


def bwd_three():
    d1 = torch.cat([douts[0].view(B, L, C * T, H, W), douts[3].view(B, L, T, H, W)], dim=2).reshape(B, L * per, H, W)
    d2[:, per:per + C * T] = douts[1]
    d3[:, 2 * per:2 * per + C * T] = douts[2]
    ext.geo_lookup_bwd_acc(acc_b[:L] + acc_b[L + 2:], disp, cx, d1, C, r)
    ext.geo_lookup_bwd_acc([dummy[0], acc_b[L], dummy[2], dummy[3]], disp, cx, d2, C, r)
    ext.geo_lookup_bwd_acc([dummy[0], dummy[1], acc_b[L + 1], dummy[2], dummy[3], dummy[4]], disp, cx, d3, C, r)
    return acc_b


def fwdbwd_torch():
    o = M.lookup(leaves, disp.view(B, 1, H, W), cx.view(B, H, W, 1), L, r)
    return torch.autograd.grad(sum((a * w).sum() for a, w in zip(o, douts)), leaves)


# ---- results must not differ
ref = [t.clone() for t in fwd_mr()]
for t, c_, n in zip(ref, fwd_mr_cl(), counts):
    assert torch.equal(c_[..., :n].permute(0, 3, 1, 2), t) and not c_[..., n:].any(), "channels-last != NCHW"
for t, b_ in zip(ref, fwd_three()):
    assert torch.equal(t, b_), "three single-pyramid launches differ from the one launch"
# the composition in float64 on the same (float32) inputs is the yardstick, at the tolerances of tests/test_gpu_multirange_lookup.py; the float32
# composition that is timed carries the same kind of rounding error as the kernels and is not compared with them
src64 = [t.double().requires_grad_() for t in src]
out64 = M.lookup(src64, disp.view(B, 1, H, W), cx.view(B, H, W, 1), L, r)
for t, a_ in zip(ref, out64):
    torch.testing.assert_close(t.double(), a_.detach(), rtol=1e-5, atol=2e-5)
gm, gb = [t.clone() for t in bwd_mr()], [t.clone() for t in bwd_three()]
g64 = torch.autograd.grad(sum((a * w).sum() for a, w in zip(out64, douts)), src64)
for q, (x, y, z) in enumerate(zip(gm, gb, g64)):
    assert torch.equal(x, y), f"source {q}: three accumulating launches differ from the one launch"
    torch.testing.assert_close(x.double(), z, rtol=1e-4, atol=1e-4 * float(z.abs().max()))
del src64, out64, g64

VARIANTS = [("forward, one launch, NCHW (geo_lookup_mr)", fwd_mr), ("forward, one launch, channels-last (geo_lookup_mr_nhwc)", fwd_mr_cl),
            ("forward, (b) three geo_lookup launches + slicing", fwd_three), ("forward, (a) torch composition", fwd_torch),
            ("backward, one launch (geo_lookup_mr_bwd_acc)", bwd_mr), ("backward, (b) three geo_lookup_bwd_acc launches + scatter of the gradients", bwd_three),
            ("forward + backward, (a) torch composition with autograd", fwdbwd_torch)]
times = {name: [] for name, _ in VARIANTS}
for name, fn in VARIANTS:
    for _ in range(10):
        fn()
torch.cuda.synchronize()
for _ in range(args.rounds):
    for name, fn in VARIANTS:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) / args.calls * 1000)

lines = [f"| variant | us per call (median of {args.rounds} rounds of {args.calls} calls) | min .. max |", "|---|---|---|"]
for name, _ in VARIANTS:
    t = times[name]
    lines.append(f"| {name} | {statistics.median(t):.1f} | {min(t):.1f} .. {max(t):.1f} |")
med = lambda n: statistics.median(times[VARIANTS[n][0]])
lines += ["", f"one-launch NCHW forward vs (b): {med(2) / med(0):.2f}x, vs (a): {med(3) / med(0):.2f}x; channels-last vs (b): {med(2) / med(1):.2f}x; "
              f"backward vs (b): {med(5) / med(4):.2f}x",
          f"one-launch forward {'is not slower than' if med(0) <= med(2) else 'IS SLOWER THAN'} baseline (b)",
          f"output bytes of one forward: {sum(counts) * B * H * W * 4 / 1e6:.1f} MB; device: {torch.cuda.get_device_name(0)}"]
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
