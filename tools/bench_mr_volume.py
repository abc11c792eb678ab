"""IGEV++'s multi-range cost volumes (osa_native.mr_volume: V0, V1, V2 from one launch; csrc/mr_volume.h) against the composition they
replace -- osa_native.gwc_volume over the full range, two F.conv3d patch convolutions and the dense slice -- on the same inputs in the same
process, at two maps: the IGEV++ evaluation map (B = 1, C = 96, 136 x 240 at 1/4, D = 192, S = 48, M = 96, k = (2, 4)) and the training crop
(64 x 192, same ranges).  For each map: forward, forward + backward (gradients of both features and both patch weights), each a median of
event-timed rounds after warm-up with the variants alternating; torch.cuda.max_memory_allocated of one training step of either form; the
achieved fraction of the fused forward's algorithmic bytes (features read once, three volumes written once) over time against the HBM peak;
and the two numbers of the tests' tolerance rule at that map (err vs the float64 composition: fused, float32 composition).
    python tools/bench_mr_volume.py [--rounds 7] [--calls 20] [--out FILE.md]"""
import argparse
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from openstereo_amd import _ext                 # noqa: E402
import mr_volume_cases as M                     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_mr_volume: no GPU visible; there is nothing to time without one")

dev = "cuda"
ext = _ext.load()
HBM_PEAK = 8.0e12                               # bytes / s, spec (MI355X)
B, C, D, S, Mr, k0, k1 = 1, 96, 192, 48, 96, 2, 4
MAPS = (("evaluation map 136 x 240", 136, 240), ("training crop 64 x 192", 64, 192))


def composition(l, r, p0, p1):
    vol = ext.gwc_volume(l, r, D, 8)
    return vol[:, :, :S].contiguous(), F.conv3d(vol[:, :, :Mr], p0, stride=(k0, 1, 1)), F.conv3d(vol, p1, stride=(k1, 1, 1))


def fused(l, r, p0, p1):
    return ext.mr_volume(l, r, p0, p1, D, S, Mr, False)


def fused_cl(l, r, p0, p1):
    return ext.mr_volume(l, r, p0, p1, D, S, Mr, True)


lines = [f"device: {torch.cuda.get_device_name(0)}; median of {args.rounds} rounds of {args.calls} calls, device events, variants alternating", ""]
try:
    lines.insert(0, "commit: " + subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip() + " + this change")
except Exception:
    pass
for title, H, W in MAPS:
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    l, r = rn(B, C, H, W), rn(B, C, H, W)
    p0, p1 = rn(8, 8, k0, 1, 1) / (8 * k0) ** 0.5, rn(8, 8, k1, 1, 1) / (8 * k1) ** 0.5
    dv = [rn(B, 8, n, H, W) for n in (S, Mr // k0, D // k1)]
    leaves = [t.clone().requires_grad_() for t in (l, r, p0, p1)]

    def step(fn):
        return torch.autograd.grad(fn(*leaves), leaves, dv)

    # ---- results must not differ: the rule of tests/mr_volume_cases.py at this size (float64 composition on the CPU)
    with torch.no_grad():
        mine, comp = fused(l, r, p0, p1), composition(l, r, p0, p1)
        assert all(torch.equal(a, b_) for a, b_ in zip(mine, fused_cl(l, r, p0, p1))), "NDHWC != NCDHW"
        assert torch.equal(mine[0], comp[0]), "V0 differs from gwc_volume's planes"
        r64 = M.restatement(*(t.double().cpu() for t in (l, r, p0, p1)), D, S, Mr)
    rule = []
    for name, a, b_, c in zip(M.NAMES[1:], mine[1:], comp[1:], r64[1:]):
        e, e32 = M.err(a, c), M.err(b_, c)
        rule.append(f"{name}: fused {e:.2e}, float32 composition {e32:.2e}")
        assert e <= M.FACTOR * e32, (name, e, e32)
    for a, b_ in zip(step(fused), step(composition)):
        torch.testing.assert_close(a, b_, rtol=1e-4, atol=1e-4 * float(b_.abs().max()))
    del mine, comp, r64

    def peak(fn):
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(fn)
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 1e6

    nograd = lambda fn: (lambda: fn(l, r, p0, p1))
    VARIANTS = [("forward, fused, NCDHW", nograd(fused)), ("forward, fused, NDHWC", nograd(fused_cl)), ("forward, composition", nograd(composition)),
                ("forward + backward, fused", lambda: step(fused)), ("forward + backward, composition", lambda: step(composition))]
    times = {name: [] for name, _ in VARIANTS}
    for name, fn in VARIANTS:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in VARIANTS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.set_grad_enabled("backward" in name):
                e0.record()
                for _ in range(args.calls):
                    fn()
                e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.calls * 1000)
    med = {n: statistics.median(t) for n, t in times.items()}
    alg = (2 * B * C * H * W + B * 8 * (S + Mr // k0 + D // k1) * H * W) * 4
    full = B * 8 * D * H * W * 4
    lines += [f"## {title} (B = {B}, C = {C}, D = {D}, S = {S}, M = {Mr}, k = ({k0}, {k1}))", "",
              "| variant | us per call (median) | min .. max |", "|---|---|---|"]
    lines += [f"| {n} | {med[n]:.1f} | {min(times[n]):.1f} .. {max(times[n]):.1f} |" for n, _ in VARIANTS]
    f, c = med["forward, fused, NCDHW"], med["forward, composition"]
    fb, cb = med["forward + backward, fused"], med["forward + backward, composition"]
    lines += ["", f"forward: fused {'is faster than' if f < c else 'IS NOT FASTER THAN'} the composition ({c / f:.2f}x); "
                  f"forward + backward: fused {'is faster than' if fb < cb else 'IS NOT FASTER THAN'} the composition ({cb / fb:.2f}x)",
              f"algorithmic bytes of the fused forward: {alg / 1e6:.1f} MB -> {alg / (f * 1e-6) / 1e12:.2f} TB/s = {alg / (f * 1e-6) / HBM_PEAK * 100:.1f} % of the "
              f"{HBM_PEAK / 1e12:.1f} TB/s HBM peak (call time, not kernel time)",
              f"peak memory of one training step above the inputs: fused {peak(fused):.1f} MB, composition {peak(composition):.1f} MB "
              f"(the full-range volume is {full / 1e6:.1f} MB)",
              "tolerance rule (max error against the float64 composition): " + "; ".join(rule), ""]
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
