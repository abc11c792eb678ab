"""The interlaced cost volume as one launch (osa_native.interlaced_volume; csrc/interlaced_volume.hip) against what it replaces, on the same
seeded parameters and inputs in the same process:

  (a) torch   the torch composition, i.e. the reference's per-disparity loop (the restatements of tests/interlaced_volume_cases.py)
  (b) parent  StereoBase shapes only: the eval path of models/interlaced.py before this op existed -- per disparity a host-side interweave,
              four fused conv + BN + ReLU launches of the engine's 2-D kernels (PackedConv3d) and five layout conversions

Shapes (B = 1, D = 48): MSNet2D (C = 32, F = 1) at the evaluation map 136 x 240 and the training crop 64 x 128; StereoBase (C = 96, F = 8) at
136 x 240 and 80 x 184.  The variants alternate inside every round; per variant the figure is the median over the rounds of the mean time of
up to `--iters` back-to-back calls (rounds are sized to about 0.2 s), printed with the minimum and the maximum, beside the peak memory a call
allocates and the fused launch's algorithmic rate (55,312 MAC per valid voxel for MSNet2D, 152,192 for StereoBase, sum_i H (W - i) valid
voxels) against the fp32 matrix peak.
    python tools/bench_interlaced_volume.py [--rounds 7] [--iters 20] [--out FILE.md]"""
import argparse
import os
import statistics
import subprocess
import sys

import torch
import torch.nn as nn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from openstereo_amd.engine import ACT_RELU, PackedConv3d          # noqa: E402
from openstereo_amd.models.interlaced import interlaced_volume    # noqa: E402
from openstereo_amd.ops import to_cl, to_ncdhw                    # noqa: E402
import interlaced_volume_cases as M                               # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_interlaced_volume: no GPU visible; there is nothing to time without one")

dev = "cuda"
F32_MATRIX_PEAK = 157.3e12                      # FLOP / s, spec (MI355X): 64 FLOP per clock and SIMD on the f32-input MFMA
MAC = {"ms": 55312, "sb": 152192}               # per valid voxel: 8*9*16 per A1 group + k2*16*9*32 per A2 group + k3*32*9*16 + 16 F
SHAPES = (("ms", 1, 136, 240), ("ms", 1, 64, 128), ("sb", 8, 136, 240), ("sb", 8, 80, 184))
D = 48


def parent_path(m, feat_l, feat_r, maxdisp):
    """models/interlaced.py's eval path before the fused op: every Conv3d with depth stride == depth kernel as a 2-D layer over kd * Cin
    channels (depth tap outermost), four engine launches and five layout conversions per disparity"""
    if not hasattr(m, "_parent_packs"):
        def flat(conv, bn):
            Co, Ci, kd = conv.weight.shape[:3]
            c2 = nn.Conv2d(Ci * kd, Co, 3, padding=1, bias=False).to(conv.weight.device)
            c2.weight.data = conv.weight.detach().permute(0, 2, 1, 3, 4).reshape(Co, kd * Ci, 3, 3).contiguous()
            return PackedConv3d(c2, bn, ACT_RELU)
        layers = m.layers()
        m._parent_packs = [flat(c, b) for c, b in layers[:3]] + [PackedConv3d(*layers[3], ACT_RELU)]
    e = m._parent_packs
    B, C, H, W = feat_l.shape
    volume = feat_l.new_zeros([B, m.num_features, maxdisp, H, W])
    for i in range(min(maxdisp, W)):
        Wc = W - i
        x = torch.stack((feat_l[:, :, :, i:], feat_r[:, :, :, :Wc]), 2).reshape(B, 2 * C, H, Wc)
        x = e[0](to_cl(x.reshape(B * 24, 8, 1, H, Wc)))
        x = e[1](to_cl(to_ncdhw(x, 16).reshape(B * 3, 128, 1, H, Wc)))
        x = e[3](e[2](to_cl(to_ncdhw(x, 32).reshape(B, 96, 1, H, Wc))))
        volume[:, :, i, :, i:] = to_ncdhw(x, m.num_features)[:, :, 0]
    return volume


lines = [f"device: {torch.cuda.get_device_name(0)}; median of {args.rounds} rounds of up to {args.iters} calls, device events, variants alternating", ""]
try:
    lines.insert(0, "commit: " + subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip() + " + this change")
except Exception:
    pass
lines += ["| config, map (D = 48) | fused ms (min .. max) | torch ms (min .. max) | parent ms (min .. max) | vs torch | vs parent | beyond the spread | peak MB fused / torch / parent | GMAC | TFLOP/s | % of 157.3 |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]


def emit():
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return text


for cfg, Fo, H, W in SHAPES:
    g = torch.Generator().manual_seed(H * 1000 + W)
    m = M.SBVolume(Fo) if cfg == "sb" else M.MSVolume()
    M.seed_volume_parameters(m.layers(), g)
    m = m.to(dev).eval()
    C = M.CONFIGS[cfg][0]
    fl, fr = torch.randn(1, C, H, W, generator=g).to(dev), torch.randn(1, C, H, W, generator=g).to(dev)
    convs, bns = zip(*m.layers())
    VARIANTS = [("fused", lambda: interlaced_volume(m, list(convs), list(bns), fl, fr, D)), ("torch", lambda: m(fl, fr, D))]
    if cfg == "sb":
        VARIANTS.append(("parent", lambda: parent_path(m, fl, fr, D)))
    with torch.no_grad():
        iters, times, peak = {}, {n: [] for n, _ in VARIANTS}, {}
        want = None
        for name, fn in VARIANTS:                                    # warm-up (MIOpen picks its kernels per crop width here), then size the rounds
            y = fn()
            if name == "fused":
                want = y
            else:
                torch.testing.assert_close(want, y, rtol=1e-4, atol=1e-5 * float(y.abs().max()))
            del y
            fn()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            peak[name] = (torch.cuda.max_memory_allocated() - base) / 1e6
            iters[name] = max(1, min(args.iters, int(200.0 / max(e0.elapsed_time(e1), 1e-3))))
            print(f"# {cfg} {H} x {W}: {name} warmed up, {e0.elapsed_time(e1):.2f} ms, {iters[name]} calls per round", flush=True)
        del want
        for _ in range(args.rounds):
            for name, fn in VARIANTS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters[name]):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / iters[name])
    med = {n: statistics.median(t) for n, t in times.items()}
    cell = lambda n: f"{med[n]:.3f} ({min(times[n]):.3f} .. {max(times[n]):.3f})" if n in med else "-"
    others = [n for n in med if n != "fused"]
    beyond = "yes" if all(max(times["fused"]) < min(times[n]) for n in others) else ("LOSES" if any(med["fused"] >= med[n] for n in others) else "no")
    gmac = MAC[cfg] * sum(H * (W - i) for i in range(min(D, W))) / 1e9
    tf = 2 * gmac * 1e9 / (med["fused"] * 1e-3) / 1e12
    lines.append(f"| {cfg}, {H} x {W} | {cell('fused')} | {cell('torch')} | {cell('parent')} | {med['torch'] / med['fused']:.1f}x | "
                 + (f"{med['parent'] / med['fused']:.1f}x" if "parent" in med else "-")
                 + f" | {beyond} | {peak['fused']:.0f} / {peak['torch']:.0f} / " + (f"{peak['parent']:.0f}" if "parent" in peak else "-")
                 + f" | {gmac:.1f} | {tf:.1f} | {tf * 1e12 / F32_MATRIX_PEAK * 100:.1f} |")
    print(lines[-1], flush=True)
    emit()
    del m, fl, fr
    torch.cuda.empty_cache()
lines += ["", "Times are call times on an otherwise idle stream (launch overhead included), not kernel times.",
          "\"beyond the spread\": the slowest fused round is faster than the fastest round of every baseline."]
print(emit())
