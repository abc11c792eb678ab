"""MobileStereoNet's 3-D inverted-residual block as one launch (osa_native.mv2_block3d; csrc/mv2_block3d.hip) against the torch composition
it replaces (the block's eight operators in eval mode, contiguous and channels_last_3d, the faster of the two is the baseline), on the same
inputs in the same process, at the seven MSNet3D shapes (B = 1; 48 x 136 x 240 at 1/4, 24 x 68 x 120 at 1/8, 12 x 34 x 60 at 1/16).  Each
figure is a median of event-timed rounds after warm-up with the variants alternating; the fused launch's algorithmic bytes (x read once, y
written once) over its time are set against the HBM peak.  The results are compared first (fused against the torch composition).
    python tools/bench_mv2_block3d.py [--rounds 7] [--calls 20] [--out FILE.md]"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from openstereo_amd import _ext                 # noqa: E402
from openstereo_amd.engine import bn_scale_shift  # noqa: E402
import mv2_block3d_cases as M                   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_mv2_block3d: no GPU visible; there is nothing to time without one")

dev = "cuda"
ns = _ext.load()
HBM_PEAK = 8.0e12                               # bytes / s, spec (MI355X)
L4, L8, L16 = (48, 136, 240), (24, 68, 120), (12, 34, 60)
# (Cin, Cout, stride, ratio, input map): dres0.0, dres0.1 / dres1 / redir1, then the hourglass (MSNet3D.py:10-45, 62-69)
SHAPES = ((40, 32, 1, 3, L4), (32, 32, 1, 3, L4), (32, 32, 1, 2, L4), (32, 64, 2, 2, L4), (64, 64, 1, 2, L8), (64, 128, 2, 2, L8), (128, 128, 1, 2, L16))
CL = torch.channels_last_3d

lines = [f"device: {torch.cuda.get_device_name(0)}; median of {args.rounds} rounds of up to {args.calls} calls, device events, variants alternating", ""]
try:
    lines.insert(0, "commit: " + subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip() + " + this change")
except Exception:
    pass
lines += ["| Cin -> Chid -> Cout, stride, input map | fused us (min .. max) | torch contiguous us (min .. max) | torch channels_last_3d us (min .. max) | speed-up | beyond the spread | x + y MB | TB/s | % of 8 TB/s |",
          "|---|---|---|---|---|---|---|---|---|"]


def emit():
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return text


for Ci, Co, stride, ratio, (D, H, W) in SHAPES:
    g = torch.Generator().manual_seed(Ci * 1000 + Co * 10 + stride)
    blk = M.seed_parameters(M.Block(Ci, Co, stride, ratio), g).to(dev).eval()
    blk_cl = M.seed_parameters(M.Block(Ci, Co, stride, ratio), torch.Generator().manual_seed(Ci * 1000 + Co * 10 + stride)).to(dev).eval().to(memory_format=CL)
    c = blk.conv
    Ch = c[3].out_channels
    x = (2.0 * torch.randn(1, Ci, D, H, W, generator=g)).to(dev)
    x_cl = x.contiguous(memory_format=CL)
    pk = ns.mv2_block3d_pack(c[0].weight, c[3].weight, c[6].weight, *bn_scale_shift(c[1]), *bn_scale_shift(c[4]), *bn_scale_shift(c[7]))
    VARIANTS = [("fused", lambda: ns.mv2_block3d(x_cl, pk, Ch, Co, stride, blk.use_res_connect)), ("torch", lambda: blk(x)), ("torch_cl", lambda: blk_cl(x_cl))]
    with torch.no_grad():
        y, want = VARIANTS[0][1](), VARIANTS[1][1]()
        torch.testing.assert_close(y, want, rtol=1e-4, atol=1e-5 * float(want.abs().max()))
        alg = (x.numel() + y.numel()) * 4
        del y, want
        calls, times = {}, {n: [] for n, _ in VARIANTS}
        for name, fn in VARIANTS:                                    # warm-up (MIOpen picks its kernels here), then size the rounds: about 0.1 s each
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            calls[name] = max(1, min(args.calls, int(100.0 / max(e0.elapsed_time(e1), 1e-3))))
        for _ in range(args.rounds):
            for name, fn in VARIANTS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls[name]):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / calls[name] * 1000)
    med = {n: statistics.median(t) for n, t in times.items()}
    base = min(("torch", "torch_cl"), key=lambda n: med[n])
    cell = lambda n: f"{med[n]:.1f} ({min(times[n]):.1f} .. {max(times[n]):.1f})"
    beyond = "yes" if max(times["fused"]) < min(times[base]) else ("LOSES" if med["fused"] >= med[base] else "no")
    f = med["fused"] * 1e-6
    lines.append(f"| {Ci} -> {Ch} -> {Co}, s{stride}, {D} x {H} x {W} | {cell('fused')} | {cell('torch')} | {cell('torch_cl')} | {med[base] / med['fused']:.2f}x | {beyond} | "
                 f"{alg / 1e6:.1f} | {alg / f / 1e12:.2f} | {alg / f / HBM_PEAK * 100:.1f} |")
    print(lines[-1], flush=True)
    emit()
    del blk, blk_cl, x, x_cl, pk
    torch.cuda.empty_cache()
lines += ["", "Times are call times on an otherwise idle stream (launch overhead included), not kernel times."]
print(emit())
