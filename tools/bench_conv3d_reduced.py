"""FoundationStereo's Conv3dNormActReduced as one launch (models/foundationstereo.py -> osa_native.conv3d_reduced; csrc/conv3d_reduced.hip)
against what it replaces, on the same inputs in the same process:
  (a) the reference composition on torch (the restatement of tests/conv3d_reduced_cases.py: two convolutions, two BatchNorms, two ReLUs),
      with contiguous and with channels-last tensors; the faster of the two is the baseline the routing rule of the mirror rests on;
  (b) two launches of the brick engine (engine.PackedConv3d, BatchNorm and ReLU in the epilogue, the hidden tensor in HBM), in the f32 and in
      the f16x3 mode, where it takes the (1,3,3) and the (17,1,1) layer; for information.
`fused` is the whole forward of a module of a grafted class: the cache look-up of the packed parameters and the launch.  The 28-channel
block (ks 3, kd 17) at D x H x W = 104 x 136 x 240 and 48 x 136 x 240 (the quarter-resolution volume of a 544 x 960 pair at max_disp 416 and
192) and 104 x 68 x 120, for one pair and for nine.  Each figure is a median of event-timed rounds after warm-up with the variants
alternating, with the spread of the rounds beside it; the peak memory of a call and the share of the 157 TFLOP/s fp32 matrix peak the fused
call reaches (real channels, 2 flops per multiply-add) are reported too.  The results are compared first.
    python tools/bench_conv3d_reduced.py [--rounds 5] [--calls 10] [--shapes 0,1,2,3,4,5] [--out FILE.md]"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from openstereo_amd import attach, ops           # noqa: E402
from openstereo_amd.engine import PackedConv3d, ACT_RELU  # noqa: E402
from openstereo_amd.models import foundationstereo as FS  # noqa: E402
import conv3d_reduced_cases as M                 # noqa: E402

SHAPES = ((104, 136, 240, 1), (104, 136, 240, 9), (48, 136, 240, 1), (48, 136, 240, 9), (104, 68, 120, 1), (104, 68, 120, 9))     # (D, H, W, B)
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--shapes", default=",".join(str(i) for i in range(len(SHAPES))))
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_conv3d_reduced: no GPU visible; there is nothing to time without one")

dev = "cuda"
C, KS, KD, PEAK = 28, 3, 17, 157e12

lines = [f"device: {torch.cuda.get_device_name(0)}; median of {args.rounds} rounds of up to {args.calls} calls, device events, variants alternating", ""]
try:
    lines.insert(0, "commit: " + subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip() + " + this change")
except Exception:
    pass
lines += ["| D x H x W, pairs | fused us (min .. max) | torch us (min .. max) | torch channels-last us (min .. max) | brick f32 us | brick f16x3 us | speed-up | beyond the spread | "
          "share of fp32 peak | peak MiB fused / torch | max abs difference |", "|---|---|---|---|---|---|---|---|---|---|---|"]


def emit():
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return text


def time_variants(variants, budget_ms=150.0):
    """-> {name: [us per call, one per round]}: warm-up, rounds sized to about budget_ms, variants alternating"""
    calls, times = {}, {n: [] for n, _ in variants}
    for name, fn in variants:
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        calls[name] = max(1, min(args.calls, int(budget_ms / max(e0.elapsed_time(e1), 1e-3))))
    for _ in range(args.rounds):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls[name]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / calls[name] * 1000)
    return times


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def verdict(fused, base):
    return "yes" if max(fused) < min(base) else ("LOSES" if statistics.median(fused) >= statistics.median(base) else "no")


class Grafted(M.Conv3dNormActReduced):
    """the class the mirror is grafted onto, so that the restatement's own class keeps its forward for the baselines"""
    forward = M.Conv3dNormActReduced.forward


attach._graft(Grafted, FS.Conv3dNormActReduced, ("forward", "reset_engine"), True)


def module(cls):
    return M.seed_parameters(cls(C, C, hidden=C, kernel_size=KS, kernel_disp=KD), torch.Generator().manual_seed(7)).to(dev).eval()


def brick(mod, precision):
    """the block as two brick-engine launches on NDHWC tensors, or None where the engine does not take a layer"""
    try:
        l1, l2 = (PackedConv3d(s[0], s[1], ACT_RELU, precision=precision) for s in (mod.conv1, mod.conv2))
        fn = lambda t: l2(l1(t))
        fn(ops.to_cl(torch.randn(1, C, 3, 8, 16, device=dev)))
        return fn
    except Exception as ex:
        print(f"brick engine, {precision}: {type(ex).__name__}: {str(ex)[:200]}", flush=True)
        return None


plain, eng = module(M.Conv3dNormActReduced), module(Grafted)
bricks = {p: brick(plain, p) for p in ("f32", "f16x3")}
for D, H, W, B in (SHAPES[int(i)] for i in args.shapes.split(",")):
    x = torch.randn(B, C, D, H, W, generator=torch.Generator().manual_seed(B)).to(dev)
    xcl = x.contiguous(memory_format=torch.channels_last_3d)
    xe = ops.to_cl(x)
    variants = [("fused", lambda: eng(x)), ("torch", lambda: plain(x)), ("torch_cl", lambda: plain(xcl))] + [(p, (lambda f: lambda: f(xe))(f)) for p, f in bricks.items() if f]
    with torch.no_grad():
        with M.Entered(eng) as entered:
            y = eng(x)
        assert entered.n == 0, "the torch composition ran instead of the fused kernel"
        want = plain(x)
        diff = float((y - want).abs().max())
        torch.testing.assert_close(y, want, rtol=1e-4, atol=1e-4)
        del y, want
        mem = peak_mib(lambda: eng(x)), peak_mib(lambda: plain(x))
        times = time_variants(variants)
    med = {n: statistics.median(t) for n, t in times.items()}
    base = min(("torch", "torch_cl"), key=lambda n: med[n])
    cell = lambda n: f"{med[n]:.0f} ({min(times[n]):.0f} .. {max(times[n]):.0f})" if n in med else "n/a"
    flops = 2.0 * B * D * H * W * C * C * (KS * KS + KD)
    lines.append(f"| {D} x {H} x {W}, {B} | {cell('fused')} | {cell('torch')} | {cell('torch_cl')} | {cell('f32')} | {cell('f16x3')} | {med[base] / med['fused']:.2f}x | "
                 f"{verdict(times['fused'], times[base])} | {flops / (med['fused'] * 1e-6) / PEAK:.1%} | {mem[0]:.0f} / {mem[1]:.0f} | {diff:.1e} |")
    print(lines[-1], flush=True)
    emit()
    del x, xcl, xe
    torch.cuda.empty_cache()
lines += ["", "Times are call times on an otherwise idle stream (launch overhead and the Python of the module's forward included), not kernel times."]
print(emit())
