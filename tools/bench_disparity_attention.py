"""FoundationStereo's disparity transformer as one launch (models/foundationstereo.py -> osa_native.disparity_attention;
csrc/disparity_attention.hip) against the torch composition it replaces, on the same inputs in the same process: the restatement of
tests/disparity_attention_cases.py as it is (softmax(q k^T / sqrt(dh)) v as torch operators) and with F.scaled_dot_product_attention in
its place, which is what the reference calls for fp32 tensors (foundationstereo/core/submodule.py:195-225); the faster of the two is the
baseline.  `fused` is the whole forward of a module of a grafted class: the cache look-up of the packed parameters, the position table from the module's
own pos_embed0 and the launch.  Shapes: C = 28, 4 heads, ff = 28, 4 layers; L = 26 (max_disp 416) and L = 12 (max_disp 192) on the 1/16 map
34 x 60 of a 544 x 960 pair, for one pair and for the nine pairs the headline step batches.  Each figure is a median of event-timed rounds
after warm-up with the variants alternating, with the spread of the rounds beside it.  The results are compared first.
    python tools/bench_disparity_attention.py [--rounds 7] [--calls 20] [--out FILE.md]"""
import argparse
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from openstereo_amd import attach               # noqa: E402
from openstereo_amd.models import foundationstereo as FS  # noqa: E402
import disparity_attention_cases as M           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_disparity_attention: no GPU visible; there is nothing to time without one")

dev = "cuda"
C, NHEAD, FF, LAYERS, H, W = 28, 4, 28, 4, 34, 60
SHAPES = ((26, 1), (26, 9), (12, 1), (12, 9))     # (L, B)


class SdpaAttention(M.Attention):
    """the restatement's attention through F.scaled_dot_product_attention, as the reference runs fp32 tensors"""

    def forward(self, query, key, value, attn_mask=None, window_size=(-1, -1)):
        B, L, _ = query.shape
        q, k, v = (p(t).view(B, L, self.num_heads, self.head_dim).transpose(1, 2) for p, t in ((self.q_proj, query), (self.k_proj, key), (self.v_proj, value)))
        return self.out_proj(F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, L, -1))


lines = [f"device: {torch.cuda.get_device_name(0)}; median of {args.rounds} rounds of up to {args.calls} calls, device events, variants alternating", ""]
try:
    lines.insert(0, "commit: " + subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip() + " + this change")
except Exception:
    pass
lines += ["| L, B x 34 x 60 | sequences | fused us (min .. max) | torch softmax us (min .. max) | torch SDPA us (min .. max) | speed-up | beyond the spread | max abs difference |",
          "|---|---|---|---|---|---|---|---|"]


def emit():
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return text


def time_variants(variants, budget_ms=100.0):
    """-> {name: [us per call, one per round]}: warm-up, rounds sized to about budget_ms, variants alternating"""
    calls, times = {}, {n: [] for n, _ in variants}
    for name, fn in variants:
        for _ in range(3):
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


def verdict(fused, base):
    return "yes" if max(fused) < min(base) else ("LOSES" if statistics.median(fused) >= statistics.median(base) else "no")


class Grafted(M.CostVolumeDisparityAttention):
    """the class the mirror is grafted onto, so that the restatement's own class keeps its forward for the baselines"""
    forward = M.CostVolumeDisparityAttention.forward


attach._graft(Grafted, FS.CostVolumeDisparityAttention, ("forward", "reset_engine"), True)


def module(L, attention=None, cls=M.CostVolumeDisparityAttention):
    g = torch.Generator().manual_seed(L)
    mod = cls(C, NHEAD, FF, num_transformer=LAYERS, max_len=L)
    if attention is not None:                               # before the seeding: the parameters are drawn in the same order
        for layer in mod.sa:
            layer.self_attn = attention(C, NHEAD)
    return M.seed_parameters(mod, g).to(dev).eval()


for L, B in SHAPES:
    plain, sdpa, eng = module(L), module(L, SdpaAttention), module(L, cls=Grafted)
    x = torch.randn(B, C, L, H, W, generator=torch.Generator().manual_seed(B)).to(dev)

    VARIANTS = [("fused", lambda: eng(x)), ("torch", lambda: plain(x)), ("sdpa", lambda: sdpa(x))]
    with torch.no_grad():
        with M.Entered(eng) as entered:
            y, want = eng(x), plain(x)
        assert entered.n == 0, "the torch composition ran instead of the fused kernel"
        diff = float((y - want).abs().max())
        torch.testing.assert_close(y, want, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(sdpa(x), want, rtol=1e-4, atol=1e-4)
        del y, want
        times = time_variants(VARIANTS)
    med = {n: statistics.median(t) for n, t in times.items()}
    base = min(("torch", "sdpa"), key=lambda n: med[n])
    cell = lambda n: f"{med[n]:.1f} ({min(times[n]):.1f} .. {max(times[n]):.1f})"
    lines.append(f"| {L}, {B} x {H} x {W} | {B * H * W} | {cell('fused')} | {cell('torch')} | {cell('sdpa')} | {med[base] / med['fused']:.2f}x | "
                 f"{verdict(times['fused'], times[base])} | {diff:.1e} |")
    print(lines[-1], flush=True)
    emit()
    del plain, sdpa, eng, x
    torch.cuda.empty_cache()
lines += ["", "Times are call times on an otherwise idle stream (launch overhead and the Python of the module's forward included), not kernel times."]
print(emit())
