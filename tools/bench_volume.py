"""Micro-benchmark of the NDHWC volume builder (GwcNet shape, HIP events, inputs resident, GPU only).

Modes (VOL_MODES or --modes, comma separated):
  quads       the chunked quad-lane kernel (build_volume_quads_kernel)
  perchannel  the per-channel kernel where the quad lanes would run (OSA_VOL_PERCHANNEL: experiments build only, the shipped library ignores it)
  walk8 / walk4            the d-walking form, 8 / 4 disparities per step, fp32 output
  walk8split / walk4split  ... the volume written as a split tensor (f16x3 chains)
VOL_B: pairs per launch (default 1).

The modes alternate inside every round (other work shares the machine); per mode the figure is the median over the rounds of the mean time of
`--iters` back-to-back launches, printed with the minimum and the maximum.  Ends with the bit-identity of the fp32 forms against `quads`.

    VOL_B=3 python tools/bench_volume.py --modes quads,walk8,walk4split [--rounds 7] [--iters 20]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from openstereo_amd import _lib, ops, ranges  # noqa: E402

DEV = "cuda:0"
MODES = "quads,perchannel,walk8,walk4,walk8split,walk4split"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default=os.environ.get("VOL_MODES", MODES))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    modes = a.modes.split(",")
    B, H, W, D = int(os.environ.get("VOL_B", 1)), 136, 240, 48
    gf = ops.empty_cl(2 * B, 320, 1, H, W, DEV); gf.normal_()
    cf = ops.empty_cl(2 * B, 12, 1, H, W, DEV); cf.normal_()
    ranges.ensure_meta(gf); ranges.ensure_meta(cf)          # (the split form derives its scale from the features' range blocks)
    lib = _lib.load()

    def run(mode):
        lib.osa_volume_walk_step(int(mode[4:5]) if mode.startswith("walk") else 0)      # 0: the chunked kernels
        os.environ.pop("OSA_VOL_PERCHANNEL", None)
        if mode == "perchannel":
            os.environ["OSA_VOL_PERCHANNEL"] = "1"
        return ops.build_cost_volume_from_cl(gf, 40, cf, B, D, out_split=mode.endswith("split"))

    def timed(mode):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            run(mode)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    outs = {}
    for mode in modes:                                       # warm-up of every mode the timed window uses
        for _ in range(3):
            v = run(mode)
        torch.cuda.synchronize()
        outs[mode] = v.clone()
    ms = {mode: [] for mode in modes}
    for _ in range(a.rounds):
        for mode in modes:
            ms[mode].append(timed(mode))
    print(f"# volume builder, {B} x [{D},{H},{W}] ({torch.cuda.get_device_name(0)}; median of {a.rounds} rounds x {a.iters} launches, modes alternating)")
    for mode in modes:
        med = statistics.median(ms[mode])
        print(f"{mode}: median {med:.4f} ms  min {min(ms[mode]):.4f}  max {max(ms[mode]):.4f}  {(487.8e6 * B / med / 1e9):.2f} TB/s (algorithmic 487.8 MB per pair)")
    for m in ("perchannel", "walk8", "walk4"):
        if m in outs and "quads" in outs:
            print(f"quads vs {m} bit-identical:", torch.equal(outs["quads"], outs[m]))


if __name__ == "__main__":
    main()
