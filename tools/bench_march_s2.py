"""Rounds of the stride-2 hourglass convolutions (conv1 32 -> 64 at V0, conv3 64 -> 128 at V1; f16x3, split tensors in and out) on the
library in use, for A/B sessions that alternate two builds process by process (OSA_LIB_PATH variant directories).  GPU only.

    python tools/bench_march_s2.py [--batches 9,3] [--rounds 6] [--iters 30] [--planes 0,4,8] [--tag new] >> rounds.txt
    python tools/bench_march_s2.py --summarize rounds.txt

A round is `--iters` launches between two HIP events after 20 warm-up launches per layer; `--planes` rotates
osa_conv_march_s2_segment_planes inside every round (0 = the launcher's cost model).  One line per (layer, pairs, planes, round);
--summarize prints median / min / max - min per (tag, layer, pairs, planes) and TF/s, TB/s of the median from the algorithmic work."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

V0, V1 = (48, 136, 240), (24, 68, 120)
LAYERS = {"conv1": (32, 64, V0), "conv3": (64, 128, V1)}


def work(layer, pairs):
    """(GFLOP, GB) per launch: 2 x MACs; split input + split output, 4 bytes per element (hi | lo halves)"""
    ci, co, (d, h, w) = LAYERS[layer]
    od, oh, ow = d // 2, h // 2, w // 2
    return 2 * pairs * ci * co * 27 * od * oh * ow / 1e9, pairs * 4 * (ci * d * h * w + co * od * oh * ow) / 1e9


def summarize(path):
    rows = {}
    for line in open(path):
        f = dict(kv.split("=") for kv in line.split() if "=" in kv)
        if "ms" in f:
            rows.setdefault((f["tag"], f["layer"], int(f["pairs"]), int(f["planes"])), []).append(float(f["ms"]))
    print("| build | layer | pairs | planes | rounds | median ms | min ms | max - min | TF/s | TB/s |\n|---|---|---|---|---|---|---|---|---|---|")
    for (tag, layer, pairs, planes), v in sorted(rows.items(), key=lambda kv: (kv[0][1], -kv[0][2], kv[0][3], kv[0][0])):
        med, (gf, gb) = statistics.median(v), work(layer, pairs)
        print(f"| {tag} | {layer} | {pairs} | {planes or 'model'} | {len(v)} | {med:.4f} | {min(v):.4f} | {max(v) - min(v):.4f} | {gf / med:.1f} | {gb / med:.2f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="9,3")
    ap.add_argument("--layers", default="conv1,conv3")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--planes", default="0")
    ap.add_argument("--tag", default="lib")
    ap.add_argument("--summarize", default="")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    import torch
    import torch.nn as nn
    from openstereo_amd import _lib, ops, ranges
    from openstereo_amd.engine import PackedConv3d
    dev, lib = "cuda:0", _lib.load()
    setter = getattr(lib, "osa_conv_march_s2_segment_planes", None)
    planes = [int(p) for p in args.planes.split(",")]
    assert setter is not None or planes == [0], "this library has no segment setter"
    for pairs in [int(b) for b in args.batches.split(",")]:
        for name in args.layers.split(","):
            ci, co, dims = LAYERS[name]
            x = ops.empty_cl(pairs, ci, *dims, dev)
            x.normal_()
            ranges.ensure_meta(x)
            idm = nn.Conv3d(ci, ci, 1, bias=False).to(dev)
            idm.weight.data = torch.eye(ci, device=dev).reshape(ci, ci, 1, 1, 1).clone()
            x = PackedConv3d(idm, None, 0, precision="f16x3")(x, out_split=True)
            layer = PackedConv3d(nn.Conv3d(ci, co, 3, 2, 1, bias=False).to(dev), nn.BatchNorm3d(co).to(dev).eval(), 1, precision="f16x3")
            n0 = lib.osa_conv3d_march_s2_launches()
            try:
                for pl in planes:
                    if setter:
                        setter(pl)
                    for _ in range(20):
                        layer(x, out_split=True)
                form = "march" if lib.osa_conv3d_march_s2_launches() > n0 else "brick"
                for r in range(args.rounds):
                    for pl in planes:
                        if setter:
                            setter(pl)
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(args.iters):
                            layer(x, out_split=True)
                        e1.record()
                        torch.cuda.synchronize()
                        print(f"tag={args.tag} layer={name} pairs={pairs} planes={pl} form={form} round={r} ms={e0.elapsed_time(e1) / args.iters:.4f}", flush=True)
            finally:
                if setter:
                    setter(0)
            del x, layer


if __name__ == "__main__":
    main()
