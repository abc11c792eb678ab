"""Timing-only ablations of the fused stride-2 transposed conv (GwcNet hourglass conv6 + redir1 / conv5 + redir2) in the form the
model runs it: split input, split redir input, split output.  GPU only; needs the experiments build for OSA_DBG
(tools/build_variant.sh exp -DOSA_EXPERIMENTS; OSA_LIB_PATH=openstereo_amd/lib/variants/exp/libopenstereo_amd.so).

    python tools/bench_deconv.py [--batch 2] [--dbgs 0,8,32,64,1]

--ab (shipped library, no experiments build): brick form against the output-plane-walking form (csrc/conv_deconv_walk.h, switched through
osa_deconv_walk) of conv5 and conv6, interleaved in ONE process on one device -- 20 warm-up launches per form, then `--rounds` rounds of
`--iters` launches per form, random inputs, HIP events, 3 and 9 pairs per launch; median, min and max - min spread over the rounds.
`--planes 1,2,4` adds the walking form with that many output planes per segment (osa_deconv_walk_segment_planes) to the rotation.

    python tools/bench_deconv.py --ab [--batches 3,9] [--rounds 7] [--iters 20] [--planes 1,2,4,8]
"""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from openstereo_amd import ops, ranges, engine  # noqa: E402
from openstereo_amd.engine import PackedConv3d, ACT_NONE, ACT_RELU  # noqa: E402


def split_of(C, dims, B, dev):
    """A split tensor with C channels: output of a 1x1x1 engine conv."""
    x = ops.empty_cl(B, C, *dims, dev)
    x.normal_()
    ranges.ensure_meta(x)
    ident = PackedConv3d(nn.Conv3d(C, C, 1, bias=False).to(dev), None, ACT_NONE)
    return ident(x, out_split=True), x


def ab(args, dev):
    """brick and walking form of the two fused transposed layers, alternating round by round"""
    import statistics
    from openstereo_amd import _lib
    lib = _lib.load()
    V0, V1, V2 = (48, 136, 240), (24, 68, 120), (12, 34, 60)
    shipped = lib.osa_deconv_walk(0)
    lib.osa_deconv_walk(shipped)
    print(f"device {torch.cuda.get_device_name(0)}; shipped osa_deconv_walk default = {shipped} (bit 0: conv6 class, bit 1: conv5 class)")
    for B in [int(v) for v in args.batches.split(",")]:
        for name, Ci, Co, din, dout in (("conv6+redir1 64->32 V1->V0", 64, 32, V1, V0), ("conv5+redir2 128->64 V2->V1", 128, 64, V2, V1)):
            xs, _ = split_of(Ci, din, B, dev)
            rs, _ = split_of(Co, dout, B, dev)
            dc = PackedConv3d(nn.ConvTranspose3d(Ci, Co, 3, stride=2, padding=1, output_padding=1, bias=False).to(dev), nn.BatchNorm3d(Co).to(dev).eval(), ACT_RELU)
            rl = PackedConv3d(nn.Conv3d(Co, Co, 1, bias=False).to(dev), nn.BatchNorm3d(Co).to(dev).eval(), ACT_NONE)
            out = ops.empty_cl(B, Co, *dout, dev)
            fn = lambda: dc(xs, redir=(rl, rs), out=out, out_split=True)
            traffic = 4 * B * (Ci * din[0] * din[1] * din[2] + 2 * Co * dout[0] * dout[1] * dout[2])
            forms = [("brick", 0, 0), ("walk", 3, 0)] + [(f"walk/{n}pl", 3, n) for n in (int(v) for v in args.planes.split(",") if v)]
            times = {f[0]: [] for f in forms}
            for form, sw, pl in forms:                                  # warm-up of every form; the counter proves which one runs
                lib.osa_deconv_walk(sw)
                lib.osa_deconv_walk_segment_planes(pl)
                n0 = lib.osa_deconv3d_walk_launches()
                for _ in range(20):
                    fn()
                assert lib.osa_deconv3d_walk_launches() - n0 == (20 if sw else 0), form
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for form, sw, pl in forms:
                    lib.osa_deconv_walk(sw)
                    lib.osa_deconv_walk_segment_planes(pl)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    times[form].append(e0.elapsed_time(e1) / args.iters)
            lib.osa_deconv_walk(shipped)
            lib.osa_deconv_walk_segment_planes(0)
            line = f"{B} pairs  {name:28s}"
            for form in times:
                t = times[form]
                med = statistics.median(t)
                line += f" | {form}: median {med:6.3f} min {min(t):6.3f} spread {max(t) - min(t):5.3f} ms ({traffic / med / 1e9:4.2f} TB/s)"
            print(line + f" | walk / brick (medians) {statistics.median(times['walk']) / statistics.median(times['brick']):5.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", action="store_true", help="brick form vs walking form, interleaved (see the module docstring)")
    ap.add_argument("--batches", default="3,9")
    ap.add_argument("--planes", default="", help="--ab: also time the walking form with these output planes per segment")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dbgs", default="0,8,32,64,1,9")
    args = ap.parse_args()
    dev = "cuda:0"
    engine.set_precision("f16x3")
    if args.ab:
        return ab(args, dev)
    V0, V1, V2 = (48, 136, 240), (24, 68, 120), (12, 34, 60)
    for name, Ci, Co, din, dout in (("conv6+redir1 64->32 V1->V0", 64, 32, V1, V0), ("conv5+redir2 128->64 V2->V1", 128, 64, V2, V1)):
        xs, xp = split_of(Ci, din, args.batch, dev)
        rs, rp = split_of(Co, dout, args.batch, dev)
        dc = PackedConv3d(nn.ConvTranspose3d(Ci, Co, 3, stride=2, padding=1, output_padding=1, bias=False).to(dev), nn.BatchNorm3d(Co).to(dev).eval(), ACT_RELU)
        rl = PackedConv3d(nn.Conv3d(Co, Co, 1, bias=False).to(dev), nn.BatchNorm3d(Co).to(dev).eval(), ACT_NONE)
        out_bytes = args.batch * Co * dout[0] * dout[1] * dout[2] * 4
        in_bytes = args.batch * Ci * din[0] * din[1] * din[2] * 4
        forms = {"fused split": lambda: dc(xs, redir=(rl, rs), out_split=True),
                 "plain (no redir, fp32 tensors)": lambda: dc(xp)}
        for fname, fn in forms.items():
            traffic = in_bytes + out_bytes * (2 if "fused" in fname else 1)
            line = f"{name:28s} {fname:32s}"
            for d in [int(v) for v in args.dbgs.split(",")]:
                os.environ["OSA_DBG"] = str(d)
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / args.iters
                line += f" | dbg {d}: {ms:6.3f} ms"
                if d == 0:
                    line += f" ({traffic / ms / 1e9:5.2f} TB/s)"
            os.environ.pop("OSA_DBG", None)
            print(line, flush=True)


if __name__ == "__main__":
    main()
