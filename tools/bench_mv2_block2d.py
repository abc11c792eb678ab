"""MobileStereoNet's 2-D inverted-residual block as one launch (osa_native.mv2_block2d; csrc/mv2_block2d.hip) against the torch composition
it replaces (the block's eight operators in eval mode, contiguous and channels_last, the faster of the two is the baseline), on the same
inputs in the same process, at the block shapes of MSNet2D (B = 1; 136 x 240 at 1/4, 68 x 120 at 1/8, 34 x 60 at 1/16 of a 544 x 960 pair,
272 x 480 for `firstconv`).  Then the whole grafted MSNet2D eval forward at 544 x 960, D = 192, against the forward of the commit before
the fused block: `parent_forward` below is that commit's MSNet2D mirror, line for line, on the same instance with the block class not
grafted (so every MobileV2_Residual runs its eight torch operators, the sums and the ReLUs after them as the reference's modules).
Each figure is a median of event-timed rounds after warm-up with the variants alternating; the fused launch's algorithmic bytes (x read
once, y written once) over its time are set against the HBM peak.  The results are compared first (fused against the torch composition).
    python tools/bench_mv2_block2d.py [--rounds 7] [--calls 20] [--out FILE.md] [--no-model]"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from openstereo_amd import _ext, attach, ops    # noqa: E402
from openstereo_amd.engine import bn_scale_shift  # noqa: E402
from openstereo_amd.models import msnet as MS   # noqa: E402
from openstereo_amd.models.interlaced import interlaced_volume  # noqa: E402
import interlaced_volume_cases as IV            # noqa: E402
import mv2_block2d_cases as M                   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--out", default=None)
ap.add_argument("--no-model", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_mv2_block2d: no GPU visible; there is nothing to time without one")

dev = "cuda"
ns = _ext.load()
HBM_PEAK = 8.0e12                               # bytes / s, spec (MI355X)
L2, L4, L8, L16 = (272, 480), (136, 240), (68, 120), (34, 60)
# (Cin, Cout, stride, ratio, input map): dres0 / dres1, redir1, conv1; conv2 / redir2, conv3; conv4; firstconv[2], [4]  (MSNet2D.py:10-45, 86-93)
SHAPES = ((48, 48, 1, 3, L4), (48, 48, 1, 2, L4), (48, 96, 2, 2, L4), (96, 96, 1, 2, L8), (96, 192, 2, 2, L8), (192, 192, 1, 2, L16), (32, 32, 1, 3, L2))
CL = torch.channels_last

lines = [f"device: {torch.cuda.get_device_name(0)}; median of {args.rounds} rounds of up to {args.calls} calls, device events, variants alternating", ""]
try:
    lines.insert(0, "commit: " + subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip() + " + this change")
except Exception:
    pass
lines += ["| Cin -> Chid -> Cout, stride, input map | fused us (min .. max) | torch contiguous us (min .. max) | torch channels_last us (min .. max) | speed-up | beyond the spread | x + y MB | TB/s | % of 8 TB/s |",
          "|---|---|---|---|---|---|---|---|---|"]


def emit():
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return text


def time_variants(variants, budget_ms=100.0):
    """-> {name: [us per call, one per round]}: warm-up (MIOpen picks its kernels here), rounds sized to about budget_ms, variants alternating"""
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


for Ci, Co, stride, ratio, (H, W) in SHAPES:
    seed = Ci * 1000 + Co * 10 + stride
    blk = M.seed_parameters(M.Block(Ci, Co, stride, ratio), torch.Generator().manual_seed(seed)).to(dev).eval()
    blk_cl = M.seed_parameters(M.Block(Ci, Co, stride, ratio), torch.Generator().manual_seed(seed)).to(dev).eval().to(memory_format=CL)
    c = blk.conv
    Ch = c[3].out_channels
    x = (2.0 * torch.randn(1, Ci, H, W, generator=torch.Generator().manual_seed(seed + 1))).to(dev)
    x_cl = x.contiguous(memory_format=CL)
    pk = ns.mv2_block2d_pack(c[0].weight, c[3].weight, c[6].weight, *bn_scale_shift(c[1]), *bn_scale_shift(c[4]), *bn_scale_shift(c[7]))
    VARIANTS = [("fused", lambda: ns.mv2_block2d(x_cl, pk, Ch, Co, stride, blk.use_res_connect, None, False)), ("torch", lambda: blk(x)), ("torch_cl", lambda: blk_cl(x_cl))]
    with torch.no_grad():
        y, want = VARIANTS[0][1](), VARIANTS[1][1]()
        torch.testing.assert_close(y, want, rtol=1e-4, atol=1e-5 * float(want.abs().max()))
        alg = (x.numel() + y.numel()) * 4
        del y, want
        times = time_variants(VARIANTS)
    med = {n: statistics.median(t) for n, t in times.items()}
    base = min(("torch", "torch_cl"), key=lambda n: med[n])
    cell = lambda n: f"{med[n]:.1f} ({min(times[n]):.1f} .. {max(times[n]):.1f})"
    f = med["fused"] * 1e-6
    lines.append(f"| {Ci} -> {Ch} -> {Co}, s{stride}, {H} x {W} | {cell('fused')} | {cell('torch')} | {cell('torch_cl')} | {med[base] / med['fused']:.2f}x | "
                 f"{verdict(times['fused'], times[base])} | {alg / 1e6:.1f} | {alg / f / 1e12:.2f} | {alg / f / HBM_PEAK * 100:.1f} |")
    print(lines[-1], flush=True)
    emit()
    del blk, blk_cl, x, x_cl, pk
    torch.cuda.empty_cache()
lines += ["", "Times are call times on an otherwise idle stream (launch overhead included), not kernel times."]


def parent_forward(net, data):
    """MSNet2D.forward of openstereo_amd/models/msnet.py in the commit before the fused 2-D block"""
    L, R = data["left"], data["right"]
    fl, fr = net.preconv11(net.feature_extraction(L)), net.preconv11(net.feature_extraction(R))
    volume = interlaced_volume(net, [*net.conv3d[0::3], net.volume11[0][0]], [*net.conv3d[1::3], net.volume11[0][1]], fl, fr, net.volume_size)[:, 0]
    cost0 = net.dres0(volume)
    cost0 = net.dres1(cost0) + cost0
    cost3 = net.classif3(net.encoder_decoder3(net.encoder_decoder2(net.encoder_decoder1(cost0))))
    return {"disp_pred": ops.upsample_softargmin(cost3, net.maxdisp, L.shape[2], L.shape[3])}


if not args.no_model:
    from openstereo_amd.utils.weights import synth_images
    net = IV.make_msnet2d().to(dev)
    data = dict(zip(("left", "right"), (t.to(dev) for t in synth_images(1, 544, 960, seed=IV.E2E_SEED, max_shift=24.0))))

    def fused_model():
        # both mirrors grafted for the call only, so that `parent_forward` sees the block class as the parent commit left it
        attach._graft(IV.MV2, MS.MobileV2Residual2D, ("forward", "reset_engine"), True)
        attach._graft(IV.MSNet2D, MS.MSNet2D, ("forward", "reset_engine"), True)
        try:
            return net(data)["disp_pred"]
        finally:
            attach.unpatch_reference()

    with torch.no_grad():
        d, want = fused_model(), parent_forward(net, data)["disp_pred"]
        epe = float((d - want).abs().mean())
        assert epe < 1e-3, epe
        times = time_variants([("fused", fused_model), ("parent", lambda: parent_forward(net, data))], budget_ms=400.0)
    med = {n: statistics.median(t) / 1000 for n, t in times.items()}
    cell = lambda n: f"{med[n]:.2f} ms ({min(times[n]) / 1000:.2f} .. {max(times[n]) / 1000:.2f})"
    lines += ["", f"Whole MSNet2D eval forward, 1 x 3 x 544 x 960, D = 192 (EPE between the two {epe:.1e} px): fused blocks {cell('fused')}, parent commit's forward {cell('parent')}, "
                  f"{med['parent'] / med['fused']:.2f}x, beyond the spread: {verdict(times['fused'], times['parent'])}"]
print(emit())
