"""Stride-1 convolution geometries that training admits (autograd._eligible) beyond isotropic "same" 3x3: the table, the float64
reference, the error bound and deliberately wrong results.  A plain module (no fixtures, no GPU) shared by tests/test_conv_geometry_cpu.py
and tests/test_gpu_conv_geometry.py.

Operands (the distribution of CONV_BWD in tests/test_gpu_autograd.py): x ~ N(0,1), w = synth_tensor * 3, dy ~ N(0,1), a non-zero bias.
The reference is F.conv2d / F.conv3d and its autograd on the CPU in float64 from the same float32 values, computed once per case and
never modified (`reference(case)`).

The bound -- derived from the number formats, elementwise, never from what a kernel returned
-------------------------------------------------------------------------------------------
Every checked element r is a sum of K products a_i * b_i (plus the bias in y):
    y  [b,co,p]  = bias[co] + sum over (ci, tap) of x * w           K = Ci * T          (T = kd * kh * kw)
    dx [b,ci,p]  = sum over (co, tap) of dy * w                     K = Co * T
    dw [co,ci,t] = sum over (b, output position) of dy * x          K = B * Do * Ho * Wo
    db [co]      = sum over (b, output position) of dy              K = B * Do * Ho * Wo
Taps that fall into the padding contribute exact zeros, so K is an upper bound of the term count everywhere.  S is the same sum over
|a_i| * |b_i| (+ |bias|): the same convolution applied to |x|, |w|, |dy| in float64 -- one more autograd pass on the absolute values gives
S for y, dx, dw and db at once.  With u = 2^-24 (fp32 unit roundoff):

  f32     Products are rounded once (relative u), and a sum of K + 1 terms accumulated in fp32 in ANY order is within (K + 1) u S of the exact
          sum to first order (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  The matrix instruction may round its
          products and its internal partial sums separately, hence a factor 2:
              bound_f32 = 2 (K + 1) u S.
          The same bound serves torch's own float32 convolution on the CPU (test_conv_geometry_cpu.py shows that the reference is inside it).

  f16x3   Each fp32 operand is multiplied by a power of two s (exact) that brings the tensor's max |.| into [2^14, 2^15)
          (pow2_scale, csrc/osa_common.h; the range blocks of openstereo_amd/ranges.py) and split hi + lo in fp16: hi is the truncated
          value, lo = x s - hi is exact in fp32 and is rounded to fp16, which leaves a representation error of at most 2^-22 relative
          (22 significant bits) as long as lo is a normal fp16 number.  The products hi*hi, hi*lo and lo*hi of 11-bit significands are exact in
          the fp32 accumulator; lo*lo is dropped (at most 2^-22 |a||b|); three times as many terms are accumulated.  Together
              (3 K + 16) u S.
          Absolute term: a lo half below 2^-14 (after scaling) is subnormal in fp16, spaced 2^-24, so its rounding error is at most 2^-25 / s
          <= 2^-39 max|a| instead of relative (the same holds for a hi half that is itself subnormal: the remainder goes to lo exactly).
          Each of the K products then carries at most 2^-39 (max|a| |b_i| + max|b| |a_i|) <= 2 * 2^-39 max|a| max|b|:
              bound_f16x3 = (3 K + 16) u S + 2 K 2^-39 max|a| max|b|.
          The bias is added in fp32 in the epilogue and is part of S.  Where the f16x3 mode runs the exact fp32 weight-gradient kernel (dilated
          layers, more than 3 taps on a plane axis: `wgrad_is_split`) dw is held to bound_f32, and db (a plain fp32 sum) always is.

  f16     The native fp16 mode rounds x, w and dy to fp16 (nearest even) and accumulates their exact products in fp32: against float64 on the
          ROUNDED operands that is the f32 situation, bound_f32.  Two refinements, both from the formats:
          * a result that is STORED in fp16 (the fp16-tensor path writes dx, and y where the channel count allows, as fp16) is rounded once
            more: + 2^-11 (|r| + bound_f32) + 2^-25 (fp16 half-ulp of a normal value; half the subnormal spacing);
          * a layer the fp16 weight-gradient kernel declines takes the exact fp32 kernel on the tensors as they are (autograd._wgrad): with fp32
            tensors dw is then the gradient of the UNROUNDED x and dy, and is compared with float64 on those.

These bounds are worst case and sit one to two orders above the observed error.  A misplaced, dropped or mis-flipped tap is an error of
order S itself; `wrong_results` builds such results in float64, and the CPU test shows that every one of them leaves the widest bound
(f16x3) on every case it applies to.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from openstereo_amd.utils.weights import synth_tensor

U = 2.0 ** -24

Case = namedtuple("Case", "id k pad dil ci co dims must_see")
# k / pad / dil: (h, w) for the flat cases (AG.conv2d; dims = (H, W)), (d, h, w) for the volume cases (AG.conv3d; dims = (D, H, W)).
# must_see: the wrong results this case is there to tell from the truth (every applicable one is checked anyway).
CASES = [
    # ---- flat
    Case("a_1x5_gru_row", (1, 5), (0, 2), (1, 1), 80, 48, (13, 37), ("pad_swapped", "dx_unflipped_w", "tap_zeroed", "dw_taps_exchanged", "shifted")),
    Case("b_5x1_gru_col", (5, 1), (2, 0), (1, 1), 80, 48, (13, 37), ("pad_swapped", "dx_unflipped_h", "tap_zeroed", "dw_taps_exchanged", "shifted")),
    Case("c_7x7_49taps", (7, 7), (3, 3), (1, 1), 8, 24, (19, 21), ("tap_zeroed", "dw_taps_exchanged", "dx_unflipped_h", "dx_unflipped_w")),
    Case("d_3x3_dil2", (3, 3), (2, 2), (2, 2), 32, 32, (17, 23), ("dilation_ignored_h", "dilation_ignored_w", "tap_zeroed")),
    Case("e_3x3_dil4", (3, 3), (4, 4), (4, 4), 32, 20, (17, 23), ("dilation_ignored_h", "dilation_ignored_w", "tap_zeroed")),
    Case("e_3x3_dil4_map_in_halo", (3, 3), (4, 4), (4, 4), 32, 20, (3, 5), ("tap_zeroed", "shifted")),
    Case("f_3x3_valid", (3, 3), (0, 0), (1, 1), 16, 20, (9, 18), ("shifted", "dx_unflipped_h", "dx_unflipped_w", "tap_zeroed")),
    Case("g_3x3_overpadded", (3, 3), (2, 2), (1, 1), 16, 12, (6, 11), ("shifted", "dx_unflipped_h", "dx_unflipped_w")),
    Case("h_3x3_pad_0_1", (3, 3), (0, 1), (1, 1), 12, 16, (8, 19), ("pad_swapped", "shifted")),
    Case("i_1x1_pad1", (1, 1), (1, 1), (1, 1), 16, 16, (5, 9), ("shifted",)),
    Case("j_2x2_valid", (2, 2), (0, 0), (1, 1), 16, 8, (7, 10), ("dx_unflipped_h", "dx_unflipped_w", "shifted", "dw_taps_exchanged")),
    Case("j_2x2_pad1", (2, 2), (1, 1), (1, 1), 16, 8, (7, 10), ("dx_unflipped_h", "dx_unflipped_w", "shifted", "dw_taps_exchanged")),
    Case("k_4x4_pad1", (4, 4), (1, 1), (1, 1), 8, 8, (9, 12), ("dx_unflipped_h", "dx_unflipped_w", "tap_zeroed")),
    Case("l_3x2_anisotropic", (3, 2), (1, 0), (2, 1), 6, 10, (11, 14), ("pad_swapped", "dilation_ignored_h", "dx_unflipped_h", "dx_unflipped_w")),
    # ---- volumes
    Case("m_1x3x3", (1, 3, 3), (0, 1, 1), (1, 1, 1), 24, 16, (5, 9, 12), ("tap_zeroed", "dx_unflipped_h", "dx_unflipped_w")),
    Case("n_3x1x1", (3, 1, 1), (1, 0, 0), (1, 1, 1), 24, 16, (5, 9, 12), ("tap_zeroed", "dx_unflipped_d")),
    Case("o_3x3x3_valid", (3, 3, 3), (0, 0, 0), (1, 1, 1), 16, 16, (3, 7, 10), ("shifted", "dx_unflipped_d", "dx_unflipped_h", "dx_unflipped_w")),
    Case("p_3x3x3_dilated_planes", (3, 3, 3), (1, 2, 2), (1, 2, 2), 16, 16, (4, 9, 11), ("dilation_ignored_h", "dilation_ignored_w", "dx_unflipped_d")),
    Case("q_2x2x2_valid", (2, 2, 2), (0, 0, 0), (1, 1, 1), 8, 12, (4, 6, 9), ("dx_unflipped_d", "dx_unflipped_h", "dx_unflipped_w")),
    Case("r_3x3x3_pad_2_0_1", (3, 3, 3), (2, 0, 1), (1, 1, 1), 8, 8, (4, 8, 9), ("pad_swapped", "shifted", "dx_unflipped_d")),
]
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
BATCH = 2

# Layers the kernels cannot take (part 4 of the test plan: the edge of the admitted domain): (id, module constructor arguments, input shape)
DECLINED = [
    ("conv2d_9x9_81taps", ("Conv2d", 8, 8, 9, 1, 4, 1), (2, 8, 12, 14)),
    ("conv3d_5x5x5_125taps", ("Conv3d", 8, 8, 5, 1, 2, 1), (1, 8, 6, 7, 9)),
    ("conv2d_3x3_dil12_128ch", ("Conv2d", 128, 128, 3, 1, 12, 12), (1, 128, 30, 34)),
    ("conv3d_3x3x3_dil2", ("Conv3d", 8, 8, 3, 1, 2, 2), (1, 8, 6, 9, 10)),
]


def flat(case):
    return len(case.k) == 2


def lift(case):
    """-> k, pad, dil as (d, h, w) triples: a flat case is the D = 1 case of the volume kernels"""
    if flat(case):
        return (1,) + case.k, (0,) + case.pad, (1,) + case.dil
    return case.k, case.pad, case.dil


def out_dims(case):
    return tuple(n + 2 * p - d * (k - 1) for n, k, p, d in zip(case.dims, case.k, case.pad, case.dil))


def taps(case):
    return int(np.prod(case.k))


def wgrad_is_split(case):
    """the split-precision / native fp16 weight-gradient kernel covers the case (csrc/wgrad.hip wgrad_impl: unit dilation, at most 3 taps on
    each plane axis); otherwise the exact fp32 kernel runs in every mode"""
    k, _, dil = lift(case)
    return all(d == 1 for d in dil) and k[1] <= 3 and k[2] <= 3


def _rn(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).normal(0, 1, shape).astype(np.float32))


def conv(case, x, w, b=None):
    return (F.conv2d if flat(case) else F.conv3d)(x, w, b, 1, case.pad, case.dil)


def inputs(case, salt=0):
    """float32 x, w, bias, dy of the case (salt: further inputs for the same weight)"""
    x = _rn((BATCH, case.ci) + case.dims, 1000 + 7 * salt)
    w = synth_tensor(case.id + ".w", (case.co, case.ci) + case.k, 1) * 3.0
    b = _rn((case.co,), 3) * 0.5 + 0.25
    dy = _rn((BATCH, case.co) + out_dims(case), 2000 + 7 * salt)
    return x, w, b, dy


def _grads(case, x, w, b, dy):
    x, w, b = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    y = conv(case, x, w, b)
    y.backward(dy)
    return {"y": y.detach(), "dx": x.grad, "dw": w.grad, "db": b.grad}


def exact_and_sums(case, x, w, b, dy):
    """float64 results {y, dx, dw, db} and the sums of absolute products S of the same, from float32 (or any) operands"""
    d = lambda t: t.detach().double().cpu()
    x, w, b, dy = d(x), d(w), d(b), d(dy)
    return _grads(case, x, w, b, dy), _grads(case, x.abs(), w.abs(), b.abs(), dy.abs())


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
    """K: the number of products summed into one element of `what`"""
    if what == "y":
        return case.ci * taps(case)
    if what == "dx":
        return case.co * taps(case)
    return BATCH * int(np.prod(out_dims(case)))


def bound_f32(S, K):
    return 2.0 * (K + 1) * U * S


def bound_f16x3(S, K, amax_a, amax_b):
    return (3.0 * K + 16.0) * U * S + 2.0 * K * 2.0 ** -39 * float(amax_a) * float(amax_b)


def stored_f16(bound, exact):
    """the bound of a result that is rounded to fp16 when it is stored"""
    return bound + 2.0 ** -11 * (exact.abs() + bound) + 2.0 ** -25


def bounds(case, ref, precision):
    """-> {y, dx, dw, db: elementwise bound tensor} of the arithmetic mode for fp32 tensors ("f32", "f16x3"; "f16": bound_f32, to be used with
    reference(case, rounded=True))"""
    S = ref.sums
    out = {}
    for what in ("y", "dx", "dw", "db"):
        K = terms(case, what)
        split = precision == "f16x3" and what != "db" and (what != "dw" or wgrad_is_split(case))
        if split:
            a, bb = {"y": (ref.x, ref.w), "dx": (ref.dy, ref.w), "dw": (ref.dy, ref.x)}[what]
            out[what] = bound_f16x3(S[what], K, a.abs().max(), bb.abs().max())
        else:
            out[what] = bound_f32(S[what], K)
    return out


def ratio(got, exact, bound):
    """max over the elements of |got - exact| / bound: <= 1 passes.  An element whose bound is zero (a tap that never meets the map: no
    products at all) must be exact: 0 there if it is, inf if not."""
    assert tuple(got.shape) == tuple(exact.shape), (tuple(got.shape), tuple(exact.shape))
    err = (got.detach().double().cpu() - exact).abs()
    assert bool(torch.isfinite(err).all())
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


# ----------------------------------------------------------------------------- deliberately wrong results
def _shifted(t, offs, margin):
    """t [B, C, D, H, W] zero-padded by `margin` on every side and read at position + offs: the tensor a tap sees"""
    D, H, W = t.shape[2:]
    tp = F.pad(t, (margin,) * 6)
    o = [margin + v for v in offs]
    return tp[:, :, o[0]:o[0] + D, o[1]:o[1] + H, o[2]:o[2] + W]


def conv_by_taps(x5, w5, offsets, osize):
    """y[b, co, p] = sum over taps t of w5[co, :, t] . x5[b, :, p + offsets[t]] on the output grid `osize`, zeros outside x5.  The tap
    offsets are given, so a wrong kernel is one with wrong offsets or wrong weights.  float64."""
    B, Ci = x5.shape[:2]
    margin = max(max(abs(v) for v in o) for o in offsets) + max(osize)
    big = F.pad(x5, (margin,) * 6)
    y = torch.zeros((B, w5.shape[0]) + tuple(osize), dtype=x5.dtype)
    wt = w5.reshape(w5.shape[0], Ci, -1)
    for t, o in enumerate(offsets):
        s = [margin + v for v in o]
        win = big[:, :, s[0]:s[0] + osize[0], s[1]:s[1] + osize[1], s[2]:s[2] + osize[2]]
        y += torch.einsum("oc,bcdhw->bodhw", wt[:, :, t], win)
    return y


def tap_offsets(k, pad, dil):
    return [(z * dil[0] - pad[0], y * dil[1] - pad[1], xx * dil[2] - pad[2]) for z in range(k[0]) for y in range(k[1]) for xx in range(k[2])]


def wrong_results(case):
    """-> {name: (which of y / dx / dw, a float64 tensor of the right shape that is NOT the result)}: what a kernel with one defect would
    return.  Only the defects that apply to the geometry (a swap of equal paddings changes nothing and is left out)."""
    ref = reference(case)
    k, pad, dil = lift(case)
    five = (lambda t: t.unsqueeze(2)) if flat(case) else (lambda t: t)
    back = (lambda t: t.squeeze(2)) if flat(case) else (lambda t: t)
    x5, w5, dy5 = five(ref.x.double()), five(ref.w.double()), five(ref.dy.double())
    bias = ref.b.double().view(1, -1, 1, 1, 1)
    osize = tuple(dy5.shape[2:])
    isize = tuple(x5.shape[2:])
    fwd = lambda offs, w=w5: back(conv_by_taps(x5, w, offs, osize) + bias)
    # dx[b, ci, p] = sum_t w[:, ci, t] . dy[b, :, p - off_t]
    dgrad = lambda w: back(conv_by_taps(dy5, w.transpose(0, 1), [tuple(-v for v in o) for o in tap_offsets(k, pad, dil)], isize))
    axis = {"d": 0, "h": 1, "w": 2}
    out = {}
    # the restatement itself must be right before its variants mean anything
    assert ratio(fwd(tap_offsets(k, pad, dil)), ref.exact["y"], bound_f32(ref.sums["y"], terms(case, "y"))) <= 1.0
    assert ratio(dgrad(w5), ref.exact["dx"], bound_f32(ref.sums["dx"], terms(case, "dx"))) <= 1.0
    # kernel indices along an axis whose taps can meet the map at all (a 3-row map under dilation 4 only ever sees the centre row of taps)
    live = [[i for i in range(k[a]) if -osize[a] < i * dil[a] - pad[a] < isize[a]] for a in range(3)]
    for name, a in axis.items():
        if any(k[a] - 1 - i != i for i in live[a]):
            out["dx_unflipped_" + name] = ("dx", dgrad(w5.flip(2 + a)))          # the data gradient read the kernel in forward order along this axis
        if k[a] > 1 and dil[a] > 1:
            d2 = list(dil)
            d2[a] = 1
            out["dilation_ignored_" + name] = ("y", fwd(tap_offsets(k, pad, d2)))
    if pad[1] != pad[2]:
        out["pad_swapped"] = ("y", fwd(tap_offsets(k, (pad[0], pad[2], pad[1]), dil)))
    T = taps(case)
    first, last = ((live[0][e] * k[1] + live[1][e]) * k[2] + live[2][e] for e in (0, -1))      # the first and the last tap that meet the map
    wz = w5.clone().reshape(case.co, case.ci, T)
    wz[:, :, last] = 0                                                             # (7x7: a tap of the partial last group)
    out["tap_zeroed"] = ("y", fwd(tap_offsets(k, pad, dil), wz.reshape(w5.shape)))
    if first != last:
        dw = five(ref.exact["dw"]).clone().reshape(case.co, case.ci, T)
        dw[:, :, [first, last]] = dw[:, :, [last, first]]
        out["dw_taps_exchanged"] = ("dw", back(dw.reshape(w5.shape)))
    out["shifted"] = ("y", torch.roll(ref.exact["y"], 1, -1))
    out["dx_shifted"] = ("dx", torch.roll(ref.exact["dx"], 1, -2))
    return out


# ----------------------------------------------------------------------------- a small network (module-level test)
NET = [  # geometry of cases a, b, d, e, f on a chain of channels: (Ci, Co, k, pad, dil)
    (80, 48, (1, 5), (0, 2), (1, 1)),
    (48, 32, (5, 1), (2, 0), (1, 1)),
    (32, 32, (3, 3), (2, 2), (2, 2)),
    (32, 20, (3, 3), (4, 4), (4, 4)),
    (20, 16, (3, 3), (0, 0), (1, 1)),
]
NET_IN = (BATCH, 80, 13, 37)


def make_net(dtype=torch.float32):
    """Conv2d layers of NET with an in-place ReLU between them (none behind the last); weights synth_tensor * 1.5, biases N(0,1) * 0.3"""
    layers = []
    for i, (ci, co, k, p, d) in enumerate(NET):
        m = torch.nn.Conv2d(ci, co, k, 1, p, d)
        with torch.no_grad():
            m.weight.copy_(synth_tensor(f"geomnet.{i}.w", (co, ci) + k, 1) * 1.5)
            m.bias.copy_(_rn((co,), 50 + i) * 0.3)
        layers += [m, torch.nn.ReLU(inplace=True)]
    return torch.nn.Sequential(*layers[:-1]).to(dtype)


def net_inputs():
    x = _rn(NET_IN, 77)
    H, W = NET_IN[2] - 2, NET_IN[3] - 2
    return x, _rn((BATCH, NET[-1][1], H, W), 78)


def net_reference(mode="f32"):
    """float64 run of make_net: loss = mean(out * g), every parameter gradient, and a first-order bound of what a run in arithmetic `mode`
    ("f32" | "f16x3") may differ by -- the SUM of the layers' own bounds carried through the network:
      forward   e_l = conv(|w_l|, e_{l-1}) + bound_l(S_l, K_l)          (ReLU is 1-Lipschitz)
      backward  eg_{l-1} = mask * (convT(|w_l|, eg_l) + bound(dgrad_l)); where a pre-activation lies within its e_l of zero the ReLU mask
                may come out either way, and the whole gradient through that element is uncertain: eg = |convT(w_l, g_l)| + the above
                (a handful of elements; their share of a dw bound is one product, still far below a misplaced tap)
      dw_l      bound(wgrad_l) + corr(|a_{l-1}|, eg_l) + corr(e_{l-1}, |g_l|);   db_l: bound(sum) + sum eg_l
      loss      sum |g| e_L / N + (N + 1) u sum |out g| / N               (the mean is an fp32 sum of N terms)
    -> loss, {name: grad}, loss_bound, {name: bound}"""
    net = make_net(torch.float64)
    x, g = net_inputs()
    x, g = x.double(), g.double()
    convs = [m for m in net if isinstance(m, torch.nn.Conv2d)]
    N = g.numel()

    def bnd(S, K, a, b, split):
        return bound_f16x3(S, K, a.abs().max(), b.abs().max()) if split else bound_f32(S, K)
    x3 = mode == "f16x3"
    acts, pres, errs, uncertain = [x], [], [torch.zeros_like(x)], []
    for i, m in enumerate(convs):
        a, w = acts[-1], m.weight.detach()
        cv = lambda t, ww, bb=None: F.conv2d(t, ww, bb, 1, m.padding, m.dilation)
        pre = cv(a, w, m.bias.detach())
        S = cv(a.abs(), w.abs(), m.bias.detach().abs())
        e = cv(errs[-1], w.abs()) + bnd(S, m.in_channels * w[0, 0].numel(), a, w, x3)
        last = i == len(convs) - 1
        pres.append(pre)
        uncertain.append(pre.abs() <= e)
        errs.append(e)
        acts.append(pre if last else pre.clamp_min(0))
    out = acts[-1]
    loss = float((out * g).sum() / N)
    loss_bound = float(((g.abs() * errs[-1]).sum() + (N + 1) * U * (out * g).abs().sum()) / N)
    grads, gbounds = {}, {}
    gy, eg = g / N, torch.zeros_like(g)
    eg = eg + U * gy.abs()                                   # g / N is formed in fp32
    for i in reversed(range(len(convs))):
        m = convs[i]
        a, ea, w = acts[i], errs[i], m.weight.detach()
        K = gy.numel() // gy.shape[1]

        def wgrad(inp, up):
            ww = w.clone().requires_grad_()
            F.conv2d(inp, ww, None, 1, m.padding, m.dilation).backward(up)
            return ww.grad

        def dgrad(up, ww):
            xx = torch.zeros_like(a).requires_grad_()
            F.conv2d(xx, ww, None, 1, m.padding, m.dilation).backward(up)
            return xx.grad
        split_w = x3 and all(d == 1 for d in m.dilation) and max(m.kernel_size) <= 3
        grads[f"{2 * i}.weight"] = wgrad(a, gy)
        gbounds[f"{2 * i}.weight"] = bnd(wgrad(a.abs(), gy.abs()), K, gy, a, split_w) + wgrad(a.abs(), eg) + wgrad(ea, gy.abs())
        grads[f"{2 * i}.bias"] = gy.sum((0, 2, 3))
        gbounds[f"{2 * i}.bias"] = bound_f32(gy.abs().sum((0, 2, 3)), K) + eg.sum((0, 2, 3))
        if i:
            mask = (pres[i - 1] > 0).double()
            raw = dgrad(gy, w)
            eraw = dgrad(eg, w.abs()) + bnd(dgrad(gy.abs(), w.abs()), m.out_channels * w[0, 0].numel(), gy, w, x3)
            eg = torch.where(uncertain[i - 1], raw.abs() + eraw, mask * eraw)
            gy = mask * raw
    return loss, grads, loss_bound, gbounds
