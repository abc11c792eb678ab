"""Stride-2 convolution and stride-2 transposed convolution geometries that training admits (autograd._shape_eligible): Conv3d k3/s2/p1 on
even dims, ConvTranspose3d and ConvTranspose2d with stride 2 as k3/p1/op1 and k4/p1/op0 -- the table, the float64 reference, the error
bounds and deliberately wrong results.  A plain module (no fixtures, no GPU) shared by tests/test_strided_conv_cases_cpu.py and
tests/test_gpu_strided_conv.py; the stride-1 companion is tests/conv_geometry_cases.py, whose bounds are used here unchanged.

Operands (the distribution of the stride-1 table): x, dy ~ N(0,1), w = synth_tensor * 3, bias = N(0,1) * 0.5 + 0.25, batch 2.  The
reference is F.conv3d(.., stride 2) / F.conv_transpose3d / F.conv_transpose2d and its autograd on the CPU in float64 from the same float32
values, computed once per case and never modified (`reference(case)`); S comes from one more pass on the absolute values.

Term counts K (upper bounds everywhere: padding, and taps that are absent from an output position's parity class, contribute exact zeros)
    y  = bias + sum over (ci, tap) of x * w           K = Ci * T          (T = k^3, flat layers k^2)
    dx = sum over (co, tap) of dy * w                 K = Co * T
    dw = sum over (b, position) of dy * x             K = B * the positions the tap is accumulated over: OUTPUT positions of a convolution,
                                                          INPUT positions of a transposed layer (each input position meets a tap once)
    db = sum over (b, output position) of dy          K = B * output positions

Bounds (conv_geometry_cases.bound_f32 / bound_f16x3 / stored_f16, derived there from the number formats)
    f32     bound_f32 = 2 (K + 1) u S for y, dx, dw, db.  The transposed layers add their bias after the launch (autograd._AddBias), one
            more fp32 rounding of a value that is at most (sum of products) + |bias| <= S: one more term of the sum, and S includes |bias|, so
            the K + 1 of 2 (K + 1) u S covers it (the convolution adds its bias in the epilogue, as the stride-1 layers do).
    f16x3   bound_f16x3 for y and dx.  dw: with the shipped default (autograd.WGRAD_F16X3_CLASS off) the exact fp32 class-mode kernel runs:
            bound_f32; with the switch on and a layer the split kernel covers: bound_f16x3 (`bounds(.., dw_split=True)`).  db: a plain fp32
            sum, bound_f32 always.
    f16     the native fp16 mode rounds x, w, dy to fp16 and accumulates exact products in fp32: bound_f32 against float64 on the ROUNDED
            operands (`reference(case, rounded=True)`), + stored_f16 where a result is stored in fp16.

A misplaced tap, exchanged parity classes, a dropped output_padding, an unflipped axis or swapped k = 4 tap pairs are errors of order S
itself; `wrong_results` builds such results in float64 (all of them through torch's own float64 functions on altered operands: there is no
tap-wise restatement to validate, only the per-axis list of live taps, which is checked against the zeros of S[dw]), and the CPU test
shows that each leaves the wider of the two bounds by more than a factor 100 on every case it applies to."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from conv_geometry_cases import U, ratio, bound_f32, bound_f16x3, stored_f16, _rn     # noqa: F401  (carried over unchanged; re-exported)
from openstereo_amd.utils.weights import synth_tensor

Case = namedtuple("Case", "id kind k pad opad ci co dims must_see")
# kind: conv3d_s2 (w [Co, Ci, k, k, k]) | deconv3d (w [Ci, Co, k, k, k]) | deconv2d (w [Ci, Co, k, k]); dims: the layer's INPUT map, (D, H, W) or (H, W)
_S2 = ("kernel_unflipped_d", "kernel_unflipped_h", "kernel_unflipped_w", "stride_phase_d", "stride_phase_h", "stride_phase_w", "edge_clamped", "tap_zeroed")
_T3 = ("kernel_unflipped_d", "kernel_unflipped_h", "kernel_unflipped_w", "dx_unflipped_d", "dx_unflipped_h", "dx_unflipped_w",
       "parity_exchanged_d", "parity_exchanged_h", "parity_exchanged_w", "tap_zeroed")
_T2 = ("kernel_unflipped_h", "kernel_unflipped_w", "dx_unflipped_h", "dx_unflipped_w", "parity_exchanged_h", "parity_exchanged_w", "tap_zeroed")
_K4_3 = ("k4_pairs_exchanged_d", "k4_pairs_exchanged_h", "k4_pairs_exchanged_w")
_K4_2 = ("k4_pairs_exchanged_h", "k4_pairs_exchanged_w")
CASES = [
    Case("s2_32_64", "conv3d_s2", 3, 1, None, 32, 64, (8, 12, 16), _S2 + ("dw_taps_exchanged", "shifted", "dx_shifted")),
    Case("s2_smallest", "conv3d_s2", 3, 1, None, 8, 8, (2, 2, 2), _S2 + ("dw_taps_exchanged",)),
    Case("s2_ragged_ch", "conv3d_s2", 3, 1, None, 6, 5, (6, 10, 18), _S2 + ("dw_taps_exchanged", "shifted", "dx_shifted")),
    Case("s2_two_ntiles", "conv3d_s2", 3, 1, None, 16, 72, (2, 4, 36), _S2 + ("shifted", "dx_shifted")),
    Case("s2_64_128", "conv3d_s2", 3, 1, None, 64, 128, (4, 6, 10), _S2 + ("dw_taps_exchanged",)),
    Case("t3_k3_64_32", "deconv3d", 3, 1, 1, 64, 32, (3, 5, 7), _T3 + ("opad_dropped", "edge_clamped", "dw_taps_exchanged", "shifted", "dx_shifted")),
    Case("t3_k3_one_voxel", "deconv3d", 3, 1, 1, 8, 8, (1, 1, 1), _T3 + ("opad_dropped", "edge_clamped", "dw_taps_exchanged")),
    Case("t3_k3_d1", "deconv3d", 3, 1, 1, 16, 12, (1, 9, 11), _T3 + ("opad_dropped", "edge_clamped", "shifted", "dx_shifted")),
    Case("t3_k3_ragged_ch", "deconv3d", 3, 1, 1, 20, 6, (5, 6, 9), _T3 + ("opad_dropped", "edge_clamped", "dw_taps_exchanged")),
    Case("t3_k3_two_ntiles", "deconv3d", 3, 1, 1, 24, 40, (2, 3, 10), _T3 + ("opad_dropped", "edge_clamped", "shifted")),
    Case("t3_k4_48_24", "deconv3d", 4, 1, 0, 48, 24, (4, 5, 9), _T3 + _K4_3 + ("edge_clamped", "dw_taps_exchanged", "shifted", "dx_shifted")),
    Case("t3_k4_one_voxel", "deconv3d", 4, 1, 0, 8, 8, (1, 1, 1), _T3 + _K4_3 + ("edge_clamped", "dw_taps_exchanged")),
    Case("t3_k4_ragged_ch", "deconv3d", 4, 1, 0, 6, 5, (3, 7, 5), _T3 + _K4_3 + ("edge_clamped", "dw_taps_exchanged")),
    Case("t2_k4_64_9", "deconv2d", 4, 1, 0, 64, 9, (11, 21), _T2 + _K4_2 + ("edge_clamped", "dw_taps_exchanged", "shifted", "dx_shifted")),
    Case("t2_k4_one_row", "deconv2d", 4, 1, 0, 12, 5, (1, 19), _T2 + _K4_2 + ("edge_clamped", "dw_taps_exchanged", "shifted")),
    Case("t2_k4_one_col", "deconv2d", 4, 1, 0, 12, 5, (9, 1), _T2 + _K4_2 + ("edge_clamped", "dw_taps_exchanged", "dx_shifted")),
    Case("t2_k3_32_32", "deconv2d", 3, 1, 1, 32, 32, (9, 17), _T2 + ("opad_dropped", "edge_clamped", "dw_taps_exchanged", "shifted", "dx_shifted")),
    Case("t2_k3_one_pixel", "deconv2d", 3, 1, 1, 4, 4, (1, 1), _T2 + ("opad_dropped", "edge_clamped", "dw_taps_exchanged")),
    Case("t2_k3_40_out", "deconv2d", 3, 1, 1, 8, 40, (5, 18), _T2 + ("opad_dropped", "edge_clamped", "shifted")),
]
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
BATCH = 2
F16_IDS = ["s2_32_64", "s2_ragged_ch", "t3_k3_64_32", "t3_k4_ragged_ch", "t2_k4_64_9", "t2_k3_one_pixel"]     # the native f16 mode runs on these

# Layers outside the admitted domain: (id, module constructor arguments (kind, Ci, Co, k, stride, pad, output_padding | None, dilation), input shape).
# All of them are declined by autograd._shape_eligible; the first three are also run on the GPU (they stay torch modules inside engine_convs).
DECLINED = [
    ("conv3d_s2_odd_dim", ("Conv3d", 8, 8, 3, 2, 1, None, 1), (1, 8, 5, 8, 10)),
    ("deconv3d_k3_op0", ("ConvTranspose3d", 8, 8, 3, 2, 1, 0, 1), (1, 8, 3, 4, 5)),
    ("conv2d_s2", ("Conv2d", 8, 8, 3, 2, 1, None, 1), (1, 8, 8, 10)),
    ("conv3d_s2_k5", ("Conv3d", 8, 8, 5, 2, 2, None, 1), (1, 8, 4, 8, 10)),
    ("conv3d_s2_pad0", ("Conv3d", 8, 8, 3, 2, 0, None, 1), (1, 8, 4, 8, 10)),
    ("conv3d_s2_dil2", ("Conv3d", 8, 8, 3, 2, 1, None, 2), (1, 8, 4, 8, 10)),
    ("conv3d_s122", ("Conv3d", 8, 8, 3, (1, 2, 2), 1, None, 1), (1, 8, 4, 8, 10)),
    ("deconv3d_k4_op1", ("ConvTranspose3d", 8, 8, 4, 2, 1, 1, 1), (1, 8, 3, 4, 5)),
    ("deconv3d_k2_p0", ("ConvTranspose3d", 8, 8, 2, 2, 0, 0, 1), (1, 8, 3, 4, 5)),
    ("deconv3d_dil2", ("ConvTranspose3d", 8, 8, 3, 2, 1, 1, 2), (1, 8, 3, 4, 5)),
    ("deconv2d_3ch", ("ConvTranspose2d", 3, 8, 4, 2, 1, 0, 1), (1, 3, 6, 7)),
]
GPU_DECLINED = ["conv3d_s2_odd_dim", "deconv3d_k3_op0", "conv2d_s2"]


def make_module(kind, ci, co, k, s, p, op, d):
    ctor = getattr(torch.nn, kind)
    return ctor(ci, co, k, s, p, op, 1, True, d) if "Transpose" in kind else ctor(ci, co, k, s, p, d)


def module_of(case):
    """the nn module of the case (with bias)"""
    kind = {"conv3d_s2": "Conv3d", "deconv3d": "ConvTranspose3d", "deconv2d": "ConvTranspose2d"}[case.kind]
    return make_module(kind, case.ci, case.co, case.k, 2, case.pad, case.opad, 1)


def transposed(case):
    return case.kind != "conv3d_s2"


def nd(case):
    return len(case.dims)


def out_dims(case):
    if transposed(case):
        return tuple((n - 1) * 2 - 2 * case.pad + case.k + case.opad for n in case.dims)
    return tuple((n + 2 * case.pad - case.k) // 2 + 1 for n in case.dims)


def taps(case):
    return case.k ** nd(case)


def wshape(case):
    io = (case.ci, case.co) if transposed(case) else (case.co, case.ci)
    return io + (case.k,) * nd(case)


def op(case, x, w, b=None, opad=None):
    """the layer, in the dtype of its operands"""
    if case.kind == "conv3d_s2":
        return F.conv3d(x, w, b, 2, case.pad)
    f = F.conv_transpose3d if case.kind == "deconv3d" else F.conv_transpose2d
    return f(x, w, b, 2, case.pad, case.opad if opad is None else opad)


def inputs(case, salt=0):
    """float32 x, w, bias, dy of the case (salt: further inputs for the same weight)"""
    x = _rn((BATCH, case.ci) + case.dims, 1000 + 7 * salt)
    w = synth_tensor(case.id + ".w", wshape(case), 1) * 3.0
    b = _rn((case.co,), 3) * 0.5 + 0.25
    dy = _rn((BATCH, case.co) + out_dims(case), 2000 + 7 * salt)
    return x, w, b, dy


def grads(case, x, w, b, dy):
    x, w, b = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    y = op(case, x, w, b)
    y.backward(dy)
    return {"y": y.detach(), "dx": x.grad, "dw": w.grad, "db": b.grad}


def exact_and_sums(case, x, w, b, dy):
    """float64 results {y, dx, dw, db} and the sums of absolute products S of the same, from float32 (or any) operands"""
    d = lambda t: t.detach().double().cpu()
    x, w, b, dy = d(x), d(w), d(b), d(dy)
    return grads(case, x, w, b, dy), grads(case, x.abs(), w.abs(), b.abs(), dy.abs())


Ref = namedtuple("Ref", "x w b dy exact sums")
_cache = {}


def reference(case, salt=0, rounded=False):
    """the case's operands and its float64 reference, computed once.  rounded: on the operands of the native f16 mode (x, w, dy rounded to
    fp16; the bias stays fp32)"""
    key = (case.id, salt, rounded)
    if key not in _cache:
        x, w, b, dy = inputs(case, salt)
        r16 = (lambda t: t.half().float()) if rounded else (lambda t: t)
        _cache[key] = Ref(x, w, b, dy, *exact_and_sums(case, r16(x), r16(w), b, r16(dy)))
    return _cache[key]


def terms(case, what):
    """K: the number of products summed into one element of `what` (an upper bound)"""
    if what == "y":
        return case.ci * taps(case)
    if what == "dx":
        return case.co * taps(case)
    if what == "dw":
        return BATCH * int(np.prod(case.dims if transposed(case) else out_dims(case)))
    return BATCH * int(np.prod(out_dims(case)))


def bounds(case, ref, precision, dw_split=False):
    """-> {y, dx, dw, db: elementwise bound tensor} of the arithmetic mode for fp32 tensors ("f32", "f16x3"; "f16": bound_f32, to be used
    with reference(case, rounded=True)).  dw_split: the f16x3 class-mode weight-gradient kernel ran (WGRAD_F16X3_CLASS on and the layer covered)"""
    S = ref.sums
    out = {}
    for what in ("y", "dx", "dw", "db"):
        K = terms(case, what)
        if precision == "f16x3" and (what in ("y", "dx") or (what == "dw" and dw_split)):
            a, bb = {"y": (ref.x, ref.w), "dx": (ref.dy, ref.w), "dw": (ref.dy, ref.x)}[what]
            out[what] = bound_f16x3(S[what], K, a.abs().max(), bb.abs().max())
        else:
            out[what] = bound_f32(S[what], K)
    return out


# ----------------------------------------------------------------------------- deliberately wrong results
def live_taps(case):
    """per spatial axis: the kernel indices that meet the map at all.  A transposed layer's tap t carries input i to output 2 i + t - pad; a
    convolution's tap t reads input 2 o + t - pad for output o."""
    out = []
    for n, no in zip(case.dims, out_dims(case)):
        if transposed(case):
            out.append([t for t in range(case.k) if any(0 <= 2 * i + t - case.pad < no for i in range(n))])
        else:
            out.append([t for t in range(case.k) if any(0 <= 2 * o + t - case.pad < n for o in range(no))])
    return out


def _edge_extended(x, n):
    """x with its edge replicated by one position on each side of its last n axes"""
    for a in range(x.dim() - n, x.dim()):
        x = torch.cat([x.narrow(a, 0, 1), x, x.narrow(a, x.shape[a] - 1, 1)], a)
    return x


def _shift_down(x, a):
    """x read one position further along axis a (zero behind the end)"""
    return torch.cat([x.narrow(a, 1, x.shape[a] - 1), torch.zeros_like(x.narrow(a, 0, 1))], a)


def wrong_results(case):
    """-> {name: (which of y / dx / dw, a float64 tensor of the right shape that is NOT the result)}: what a kernel with one defect would
    return.  Only the defects the geometry can show: a flip or a roll along an axis of length 1, or a flip that maps the live taps of an
    axis onto themselves, changes nothing and is left out."""
    ref = reference(case)
    n = nd(case)
    x, w, b, dy = ref.x.double(), ref.w.double(), ref.b.double(), ref.dy.double()
    tr = transposed(case)
    names = ("d", "h", "w")[3 - n:]
    live = live_taps(case)
    # the live-tap lists are this module's own restatement of the geometry: a tap is live exactly where S[dw] is not zero
    met = ref.sums["dw"].sum((0, 1)) > 0
    mine = torch.zeros_like(met)
    mine[torch.meshgrid(*[torch.tensor(l) for l in live], indexing="ij")] = True
    assert torch.equal(met, mine), (case.id, live)
    assert all(bool((ref.exact["dw"][(slice(None), slice(None)) + tuple(idx.tolist())] == 0).all()) for idx in (~met).nonzero())
    out = {}
    for i, name in enumerate(names):
        ax = 2 + i
        if any(case.k - 1 - t != t for t in live[i]):
            g = grads(case, x, w.flip(ax), b, dy)
            # the parity kernel's result (y of a transposed layer, dx of the convolution) and the stride-2 convolution kernel's result (dx of
            # a transposed layer, y of the convolution) with the kernel read in the other order along this axis
            out["kernel_unflipped_" + name] = ("y", g["y"]) if tr else ("dx", g["dx"])
            out[("dx_unflipped_" if tr else "y_unflipped_") + name] = ("dx", g["dx"]) if tr else ("y", g["y"])
        if tr:
            y = ref.exact["y"]
            sh = list(y.shape)
            pairs = y.reshape(sh[:ax] + [sh[ax] // 2, 2] + sh[ax + 1:]).flip(ax + 1).reshape(sh)
            out["parity_exchanged_" + name] = ("y", pairs)
            if case.k == 4:
                wx = w.index_select(ax, torch.tensor([2, 3, 0, 1]))
                out["k4_pairs_exchanged_" + name] = ("y", op(case, x, wx, b))
        else:
            out["stride_phase_" + name] = ("y", op(case, _shift_down(x, ax), w, b))
    if tr and case.k == 3:
        short = op(case, x, w, b, opad=0)
        out["opad_dropped"] = ("y", F.pad(short, (0, 1) * n))
    # the input edge-replicated by one position where the layer reads zeros
    xe = _edge_extended(x, n)
    if tr:
        crop = (slice(None), slice(None)) + tuple(slice(2, 2 + no) for no in out_dims(case))
        out["edge_clamped"] = ("y", op(case, xe, w, b)[crop])
    else:
        out["edge_clamped"] = ("y", F.conv3d(xe, w, b, 2, 0))
    first, last = (tuple(l[e] for l in live) for e in (0, -1))
    sel = lambda t: (slice(None), slice(None)) + t
    wz = w.clone()
    wz[sel(last)] = 0
    out["tap_zeroed"] = ("y", op(case, x, wz, b))
    if first != last:
        dw = ref.exact["dw"].clone()
        dw[sel(first)], dw[sel(last)] = ref.exact["dw"][sel(last)], ref.exact["dw"][sel(first)]
        out["dw_taps_exchanged"] = ("dw", dw)
    if ref.exact["y"].shape[-1] > 1:
        out["shifted"] = ("y", torch.roll(ref.exact["y"], 1, -1))
    if ref.exact["dx"].shape[-2] > 1:
        out["dx_shifted"] = ("dx", torch.roll(ref.exact["dx"], 1, -2))
    return out


# ----------------------------------------------------------------------------- a small hourglass (module-level test)
NET_IN = (BATCH, 16, 4, 8, 12)


def make_net():
    """Conv3d(16,24,3,2,1), ReLU, Conv3d(24,40,3,2,1), ReLU, ConvTranspose3d(40,24,3,2,1,1), ReLU, ConvTranspose3d(24,16,4,2,1,0): all with
    bias, in-place ReLUs; weights synth_tensor * 1.5, biases N(0,1) * 0.3"""
    nn = torch.nn
    convs = [nn.Conv3d(16, 24, 3, 2, 1), nn.Conv3d(24, 40, 3, 2, 1), nn.ConvTranspose3d(40, 24, 3, 2, 1, 1), nn.ConvTranspose3d(24, 16, 4, 2, 1, 0)]
    layers = []
    for i, m in enumerate(convs):
        with torch.no_grad():
            m.weight.copy_(synth_tensor(f"stridednet.{i}.w", tuple(m.weight.shape), 1) * 1.5)
            m.bias.copy_(_rn(tuple(m.bias.shape), 60 + i) * 0.3)
        layers += [m, nn.ReLU(inplace=True)]
    return nn.Sequential(*layers[:-1])


def net_inputs():
    return _rn(NET_IN, 87), _rn(NET_IN, 88)


def case_of_module(name, m, dims):
    """the Case of an admitted nn.Conv3d (stride 2) / nn.ConvTranspose3d / nn.ConvTranspose2d module on an input map `dims`"""
    kind = {torch.nn.Conv3d: "conv3d_s2", torch.nn.ConvTranspose3d: "deconv3d", torch.nn.ConvTranspose2d: "deconv2d"}[type(m)]
    return Case(name, kind, m.kernel_size[0], m.padding[0], m.output_padding[0] if kind != "conv3d_s2" else None, m.in_channels, m.out_channels,
                tuple(dims), ())
