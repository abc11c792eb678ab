"""What the per-pixel variance costs on the fused soft-argmin head (HIP events, inputs resident, GPU only).

Three ways to the final maps of one forward, per shape:
  head        ops.upsample_softargmin(cost)                         the disparity-only head (unchanged kernel: the baseline)
  head+var    ops.upsample_softargmin(cost, return_variance=True)   disparity and variance from one kernel
  torch       F.interpolate(trilinear) -> softmax -> sum p d, sum p (d - disp)^2 in torch: what a user had to run for the same two maps
Shapes: GwcNet 9 x [48,136,240] -> [192,544,960], align_corners=False (the x4 streaming kernel, the sub-batch of the headline benchmark) and
PSMNet [16,64,128] -> [64,256,512], align_corners=True (the generic LDS kernel).

The variants alternate inside every round (other work shares the machine); the figure is the median over the rounds of the mean time of
`--iters` back-to-back launches.  Writes one markdown table to stdout (and to --out).

    python tools/bench_head_variance.py [--rounds 7] [--iters 20] [--out profiles/round7/head_variance.md]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from openstereo_amd import ops  # noqa: E402

DEV = "cuda:0"
SHAPES = [("GwcNet", (9, 48, 136, 240), (192, 544, 960), False), ("PSMNet", (1, 16, 64, 128), (64, 256, 512), True)]


def torch_composition(cost, D, h, w, align):
    p = F.softmax(F.interpolate(cost[:, None], [D, h, w], mode="trilinear", align_corners=align).squeeze(1), dim=1)
    d = torch.arange(D, dtype=p.dtype, device=p.device).view(1, D, 1, 1)
    disp = torch.sum(p * d, 1)
    return disp, torch.sum(p * (d - disp.unsqueeze(1)) ** 2, 1)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"# Fused head with and without the variance ({torch.cuda.get_device_name(0)}; median of {a.rounds} rounds x {a.iters} launches, variants alternating)", "",
             "| shape | head (ms) | head + var (ms) | ratio | torch composition (ms) | min .. max head | min .. max head + var | algorithmic GB/s head + var |",
             "|---|---|---|---|---|---|---|---|"]
    for name, shape, (D, h, w), align in SHAPES:
        torch.manual_seed(0)
        cost = torch.randn(shape, device=DEV) * 3
        variants = {"head": lambda: ops.upsample_softargmin(cost, D, h, w, align),
                    "var": lambda: ops.upsample_softargmin(cost, D, h, w, align, return_variance=True),
                    "torch": lambda: torch_composition(cost, D, h, w, align)}
        with torch.no_grad():
            want, (disp, var), (tdisp, tvar) = variants["head"](), variants["var"](), variants["torch"]()
            assert torch.equal(want, disp), "the disparity moved"
            err = float(((var - tvar).abs() / (1 + tvar)).max())
            for fn in variants.values():                      # warm-up of every shape the timed window uses
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in variants}
            for _ in range(a.rounds):
                for k, fn in variants.items():
                    ms[k].append(timed(fn, a.iters if k != "torch" else max(2, a.iters // 5)))
        med = {k: statistics.median(v) for k, v in ms.items()}
        nbytes = cost.numel() * 4 + 2 * shape[0] * h * w * 4
        lines.append(f"| {name} {shape[0]} x {list(shape[1:])} -> {[D, h, w]}, align_corners={align} | {med['head']:.4f} | {med['var']:.4f} | {med['var'] / med['head']:.3f} | "
                     f"{med['torch']:.3f} | {min(ms['head']):.4f} .. {max(ms['head']):.4f} | {min(ms['var']):.4f} .. {max(ms['var']):.4f} | {nbytes / med['var'] / 1e6:.0f} |")
        lines.append(f"|   disparity bit-identical: {torch.equal(want, disp)}; max abs(var - torch fp32 var) / (1 + var) = {err:.2e} | | | | | | | |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
