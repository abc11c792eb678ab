"""The single-pyramid geometry-encoding lookup through the C ABI (_lib.call): osa_geo_lookup_f32 (NCHW, the training path),
osa_geo_lookup_nhwc_f32 (channel stride rounded up to 4, the engine's GRU loop), osa_geo_lookup_bwd_acc_f32 and the dense
osa_geo_lookup_bwd_f32, at the StereoBase training map (1 x 80 x 184: the 320x736 crop at 1/4) and at IGEV x 32 with 4 pairs
(4 x 136 x 240: 544 x 960 at 1/4), both with C = 8, D = 48, radius 4.
Per shape: warm-up, then rounds in which the entry points alternate, device events around CALLS calls each; the table gives the median round
with min .. max.  The ABI does not change between library versions, so the same script times any of them:
    python tools/bench_lookup.py [--rounds 7] [--calls 50] [--levels 2] [--out FILE.md]
    OSA_LIB_PATH=openstereo_amd/lib/variants/NAME/libopenstereo_amd.so python tools/bench_lookup.py
The second table is the dense backward in its two forms (one wave per (pixel, level), and the thread-per-element gather form the host
falls back to for radius > 4), compared bit for bit; the form switch OSA_GEO_BWD_FORM exists in the experiments build only
(bash tools/build_one_variant.sh exp_geo geometry -DOSA_EXPERIMENTS): the shipped library always runs the rows form."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from openstereo_amd import _lib     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--levels", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_lookup: no GPU visible; there is nothing to time without one")

dev = "cuda"
C, D, r, L = int(os.environ.get("LOOKUP_C", "8")), 48, 4, args.levels      # LOOKUP_C: geometry channels (IGEV 8)
nch = (C + 1) * (2 * r + 1) * L
Cs = (nch + 3) // 4 * 4
st = torch.cuda.current_stream().cuda_stream
lines = []


def timed(call, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1000


def problem(B, H, W):
    g = torch.Generator().manual_seed(0)
    p = {"disp": (torch.rand(B, H, W, generator=g) * 40).to(dev), "cx": torch.arange(W).float().view(1, 1, W).repeat(B, H, 1).to(dev),
         "dout": torch.randn(B, nch, H, W, generator=g).to(dev)}
    p["shapes"] = [(B, H, W, C, D >> l) for l in range(L)] + [(B, H, W, W >> l) for l in range(L)]
    p["levels"] = [torch.randn(s, generator=g).to(dev) for s in p["shapes"]]
    p["len"] = ((ctypes.c_int * L)(*[s[-1] for s in p["shapes"][:L]]), (ctypes.c_int * L)(*[s[-1] for s in p["shapes"][L:]]))
    return p


def pointers(ts):
    return (ctypes.c_void_p * L)(*[t.data_ptr() for t in ts[:L]]), (ctypes.c_void_p * L)(*[t.data_ptr() for t in ts[L:]])


for B, H, W in ((1, 80, 184), (4, 136, 240)):
    p = problem(B, H, W)
    gl, cl = p["len"]
    d, cx, dout = p["disp"].data_ptr(), p["cx"].data_ptr(), p["dout"].data_ptr()
    gp, cp = pointers(p["levels"])
    out, out_cl = torch.empty(B, nch, H, W, device=dev), torch.empty(B, H, W, Cs, device=dev)
    acc, grads = [torch.zeros(s, device=dev) for s in p["shapes"]], [torch.empty(s, device=dev) for s in p["shapes"]]
    ap_, acp = pointers(acc)
    dp_, dcp = pointers(grads)
    entries = [("osa_geo_lookup_f32", lambda: _lib.call("osa_geo_lookup_f32", gp, cp, gl, cl, L, d, cx, out.data_ptr(), B, H, W, C, r, st)),
               ("osa_geo_lookup_nhwc_f32", lambda: _lib.call("osa_geo_lookup_nhwc_f32", gp, cp, gl, cl, L, d, cx, out_cl.data_ptr(), Cs, B, H, W, C, r, st)),
               ("osa_geo_lookup_bwd_acc_f32", lambda: _lib.call("osa_geo_lookup_bwd_acc_f32", ap_, acp, gl, cl, L, d, cx, dout, B, H, W, C, r, st)),
               ("osa_geo_lookup_bwd_f32", lambda: _lib.call("osa_geo_lookup_bwd_f32", dp_, dcp, gl, cl, L, d, cx, dout, B, H, W, C, r, st))]
    for _, call in entries:
        for _ in range(10):
            call()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in entries}
    for _ in range(args.rounds):
        for name, call in entries:
            times[name].append(timed(call, args.calls))
    assert torch.equal(out_cl[..., :nch].permute(0, 3, 1, 2), out) and not out_cl[..., nch:].any(), "channels-last != NCHW"
    lines += [f"{B} x {H} x {W}, C = {C}, D = {D}, {L} levels, radius {r}", "",
              f"| entry point | us per call (median of {args.rounds} rounds of {args.calls} calls) | min .. max |", "|---|---|---|"]
    for name, _ in entries:
        t = times[name]
        lines.append(f"| `{name}` | {statistics.median(t):.1f} | {min(t):.1f} .. {max(t):.1f} |")
    lines.append("")

# the dense backward's two forms at the training map
B, H, W = 1, 80, 184
p = problem(B, H, W)
ref = None
for form in ("gather", "rows"):
    os.environ["OSA_GEO_BWD_FORM"] = "1" if form == "gather" else "2"
    grads = [torch.full(s, float("nan"), device=dev) for s in p["shapes"]]
    gp, cp = pointers(grads)
    call = lambda: _lib.call("osa_geo_lookup_bwd_f32", gp, cp, *p["len"], L, p["disp"].data_ptr(), p["cx"].data_ptr(), p["dout"].data_ptr(), B, H, W, C, r, st)
    for _ in range(5):
        call()
    us = timed(call, args.calls)
    same = "" if ref is None else f"; bit-identical to the gather form: {all(torch.equal(a, b) for a, b in zip(grads, ref))}"
    ref = ref or grads
    nbytes = sum(t.numel() for t in grads) * 4 + p["dout"].numel() * 4
    lines.append(f"[lookup bwd, OSA_GEO_BWD_FORM {form:6s}] {us:7.1f} us per call ({nbytes / us / 1e6:.2f} TB/s of written + read bytes){same}")
lines.append(f"device: {torch.cuda.get_device_name(0)}; library: {_lib.LIB_PATH}")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
