"""Case tables and pure-torch helpers of the range-block tests (tests/test_range_block_cases_cpu.py, tests/test_gpu_range_blocks.py).

The f16x3 mode rests on two facts about range blocks (include/openstereo_amd.h, osa_f16x3_ranges):
  1. every producer folds max |y| of WHAT IT WROTE into meta[16 * s] -- the next layer derives its operand scale from it;
  2. a split writer chooses the scale of its hi / lo halves from the bound  coef[0] * max|x| + coef[1] (+ max|residual|) (+ redir terms)
     through pow2_scale(bound * 1.0625), so that bound * 1.0625 * meta[1] lies in [2^14, 2^15).
Nothing here calls an engine kernel or needs a GPU: the module builds inputs that ATTAIN the bound (worst_case), inputs whose output maximum
sits where a kernel could lose it (spike), reads split tensors from the documented bytes (decode_split) and states the comparison rules
(check_recorded_max, scale_window)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from openstereo_amd.utils.weights import synth_tensor

MS = [2.0 ** -10, 1.0, 2.0 ** 10]          # operand magnitudes of the bound tests


# ----------------------------------------------------------------------------- the storage format
def decode_split(t, meta, channels=None):
    """A split NDHWC tensor (logical [B, C, D, H, W], channels innermost in memory) read from its documented bytes: the storage viewed as
    fp16, every 16-channel chunk = [16 x fp16 hi | 16 x fp16 lo] at the scale meta[1]; value = (hi + lo) / meta[1] in fp64.
    Returns a contiguous fp64 [B, C, D, H, W] tensor on the CPU (channels = (first, count) selects a 16-aligned slice).  Shares nothing
    with the engine's reader (join_f16 of conv_kernel.h)."""
    assert t.dim() == 5 and t.dtype == torch.float32 and t.shape[1] % 16 == 0, "a split tensor has the bytes of fp32 and whole 16-channel chunks"
    rows = t.detach().permute(0, 2, 3, 4, 1)
    assert rows.is_contiguous(), "NDHWC storage"
    scale = float(meta[1])
    assert scale > 0.0 and np.isfinite(scale)
    B, D, H, W, C = rows.shape
    halves = rows.cpu().contiguous().view(torch.float16).reshape(B, D, H, W, C // 16, 2, 16).to(torch.float64)
    val = ((halves[..., 0, :] + halves[..., 1, :]) / scale).reshape(B, D, H, W, C).permute(0, 4, 1, 2, 3)
    if channels is not None:
        assert channels[0] % 16 == 0 and channels[1] % 16 == 0
        val = val[:, channels[0]:channels[0] + channels[1]]
    return val.contiguous()


def encode_split(values, scale):
    """hand-built bytes for the decoder's test: fp64 [B, C, D, H, W] -> (fp32-typed split tensor, hi, lo); hi = fp16(v * scale) rounded to
    nearest, lo = fp16(v * scale - hi).  Not the kernels' split (they truncate hi): only the layout matters here."""
    B, C, D, H, W = values.shape
    assert C % 16 == 0
    v = (values.to(torch.float64) * scale).permute(0, 2, 3, 4, 1).reshape(B, D, H, W, C // 16, 16)
    hi = v.to(torch.float16)
    lo = (v - hi.to(torch.float64)).to(torch.float16)
    raw = torch.stack([hi, lo], dim=-2).reshape(B, D, H, W, 2 * C).contiguous().view(torch.float32)
    return raw.permute(0, 4, 1, 2, 3), hi, lo


# ----------------------------------------------------------------------------- comparison rules
def check_recorded_max(amax, y, kind, what="", src_amax=None):
    """The recorded maximum against the maximum of the kernel's OWN output `y` (read back by the caller: directly for fp32 / fp16, through
    decode_split for split tensors).
      "f32"     the kernel takes the maximum from the fp32 values it stores: equal bit for bit;
      "split"   |amax - max|decoded|| <= 2^-21 * amax: twice the split's documented error (osa_common.h: lo rounded to nearest, 2^-22 |x|;
                the lo half is normal at the maximum, which sits in the top binades of the scale);
      "f16"     <= 2^-11 * amax (one rounding to fp16);
      "inherit" pool2x / bilinear resize share the source's block: max|y| * (1 - 4 * 2^-24) <= amax <= src_amax (4 ulp for the interpolation's roundings)."""
    amax = float(amax)
    ymax = float(y.detach().abs().max()) if y.numel() else 0.0
    assert np.isfinite(amax) and np.isfinite(ymax), f"{what}: recorded {amax}, stored maximum {ymax}"
    if kind == "f32":
        assert amax == ymax, f"{what}: recorded maximum {amax!r} != maximum of the stored values {ymax!r} (ratio {amax / ymax if ymax else float('inf'):.6f})"
    elif kind == "split":
        assert abs(amax - ymax) <= 2.0 ** -21 * amax, f"{what}: recorded maximum {amax!r} vs decoded maximum {ymax!r} (ratio {amax / ymax if ymax else float('inf'):.8f})"
    elif kind == "f16":
        assert abs(amax - ymax) <= 2.0 ** -11 * amax, f"{what}: recorded maximum {amax!r} vs fp16 maximum {ymax!r}"
    elif kind == "inherit":
        assert src_amax is not None
        assert ymax * (1.0 - 4 * 2.0 ** -24) <= amax <= float(src_amax), f"{what}: inherited maximum {amax!r}, output {ymax!r}, source {float(src_amax)!r}"
    else:
        raise ValueError(kind)


def is_pow2(s):
    m, _ = np.frexp(float(s))
    return float(s) > 0 and np.isfinite(float(s)) and m == 0.5


def scale_window(frac):
    """[lo, hi) for max|decoded| * meta[1] of a split tensor whose maximum attains `frac` of its bound: pow2_scale(bound * 1.0625) places
    bound * 1.0625 * meta[1] in [2^14, 2^15), so frac * bound * meta[1] lies in [frac * 2^14 / 1.0625, 2^15 / 1.0625) -- a subset of the
    window the tests assert, [frac * 2^14 / 1.0625, 2^15)."""
    return frac * 2.0 ** 14 / 1.0625, 2.0 ** 15


# ----------------------------------------------------------------------------- layers
@dataclass(frozen=True)
class Layer:
    """One conv / transposed-conv layer of the tables below (weights: synth_tensor(name + ...))."""
    name: str
    kind: str = "conv"            # "conv" | "deconv3d" | "deconv2d"
    ci: int = 32
    co: int = 32
    k: int = 3
    stride: int = 1
    pad: int = 1
    dil: int = 1
    opad: int = 0
    bias: bool = False
    bn: bool = False
    act: str = "none"             # none | relu | leaky | relu6 | sigmoid | tanh
    slope: float = 0.25           # leaky (a power of two: the scaled maximum is exact)
    redir: bool = False           # transposed 3-D: fused 1x1x1 redir branch (Conv3d(co, co, 1) + BN) on the output-resolution tensor


ACT_CODE = {"none": 0, "relu": 1, "leaky": 2, "relu6": 3, "sigmoid": 4, "tanh": 5}


def _bn(c, name, dims):
    bn = (nn.BatchNorm3d if dims == 3 else nn.BatchNorm2d)(c)
    bn.load_state_dict({k: synth_tensor(f"{name}.{k}", v.shape, 2) for k, v in bn.state_dict().items()})
    return bn.eval()


def modules(layer: Layer):
    """(conv, bn or None, redir conv or None, redir bn or None): CPU torch modules of a Layer, seeded by its name"""
    n = layer.name
    if layer.kind == "conv":
        conv = nn.Conv3d(layer.ci, layer.co, layer.k, layer.stride, layer.pad, layer.dil, bias=layer.bias)
    elif layer.kind == "deconv3d":
        conv = nn.ConvTranspose3d(layer.ci, layer.co, layer.k, stride=2, padding=layer.pad, output_padding=layer.opad, bias=layer.bias)
    else:
        conv = nn.ConvTranspose2d(layer.ci, layer.co, layer.k, stride=2, padding=layer.pad, output_padding=layer.opad, bias=layer.bias)
    conv.weight.data = synth_tensor(n + ".w", conv.weight.shape, 1)
    if layer.bias:
        conv.bias.data = synth_tensor(n + ".bias", conv.bias.shape, 1)
    dims = 2 if layer.kind == "deconv2d" else 3
    bn = _bn(layer.co, n + ".bn", dims) if layer.bn else None
    rc = rbn = None
    if layer.redir:
        rc = nn.Conv3d(layer.co, layer.co, 1, bias=False)
        rc.weight.data = synth_tensor(n + ".rw", rc.weight.shape, 1)
        rbn = _bn(layer.co, n + ".rbn", 3)
    return conv, bn, rc, rbn


def activation(layer: Layer):
    return {"none": lambda t: t, "relu": F.relu, "leaky": lambda t: F.leaky_relu(t, layer.slope), "relu6": F.relu6,
            "sigmoid": torch.sigmoid, "tanh": torch.tanh}[layer.act]


def fold(conv, bn, dtype=torch.float64):
    """(scale, shift) per output channel of conv (+ bias) (+ eval BatchNorm): y = conv_nobias(x) * scale + shift"""
    co = conv.out_channels
    scale, shift = torch.ones(co, dtype=dtype), torch.zeros(co, dtype=dtype)
    if bn is not None:
        scale = bn.weight.detach().to(dtype) / torch.sqrt(bn.running_var.detach().to(dtype) + bn.eps)
        shift = bn.bias.detach().to(dtype) - bn.running_mean.detach().to(dtype) * scale
    if conv.bias is not None:
        shift = shift + conv.bias.detach().to(dtype) * scale
    return scale, shift


def bound_coef(conv, bn):
    """(gain, smax) as the engine computes them (PackedConv3d.__init__): max_co |bn scale| * sum|w_co| and max_co |shift|, in fp64.
    The output-channel axis of a transposed weight is dim 1."""
    w = conv.weight.detach().to(torch.float64)
    transposed = isinstance(conv, (nn.ConvTranspose3d, nn.ConvTranspose2d))
    red = [d for d in range(w.dim()) if d != (1 if transposed else 0)]
    scale, shift = fold(conv, bn)
    return float((w.abs().sum(dim=red) * scale.abs()).max()), float(shift.abs().max())


def reference(layer: Layer, mods, x, residual=None, rx=None, dtype=torch.float64):
    """the layer as torch computes it on the CPU in `dtype`: act(BN(conv(x)) (+ residual) (+ BN_r(conv_r(rx))))"""
    import copy
    conv, bn, rc, rbn = (None if m is None else copy.deepcopy(m).to(dtype) for m in mods)
    with torch.no_grad():
        y = conv(x.to(dtype))
        if bn is not None:
            y = bn(y)
        if residual is not None:
            y = y + residual.to(dtype)
        if rc is not None:
            y = y + rbn(rc(rx.to(dtype)))
        return activation(layer)(y)


def out_dims(layer: Layer, dims):
    if layer.kind == "conv":
        return tuple((n + 2 * layer.pad - layer.dil * (layer.k - 1) - 1) // layer.stride + 1 for n in dims)
    return tuple((n - 1) * 2 - 2 * layer.pad + layer.k + layer.opad for n in dims)


def taps_of(layer: Layer, o, n_in):
    """[(kernel index, input index)] of the taps that reach output index `o` from inside an input dimension of size n_in"""
    out = []
    for kk in range(layer.k):
        if layer.kind == "conv":
            i = o * layer.stride - layer.pad + kk * layer.dil
        else:                                      # transposed, stride 2: o = 2 i - pad + kk
            if (o + layer.pad - kk) % 2:
                continue
            i = (o + layer.pad - kk) // 2
        if 0 <= i < n_in:
            out.append((kk, i))
    return out


def within_reach(layer: Layer, in_voxel, out_voxel, in_dims):
    """does the receptive field of output voxel (spatial tuple) contain input voxel (spatial tuple)?"""
    return all(any(i == iv for _, i in taps_of(layer, ov, n)) for iv, ov, n in zip(in_voxel, out_voxel, in_dims))


# ----------------------------------------------------------------------------- inputs that attain the bound
def _uniform(shape, seed):
    """uniform in [-1, 1), fp32, seeded"""
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32))


def worst_case(layer: Layer, mods, M, shape, voxel=None, residual_amax=0.0, redir_amax=0.0, background=1.0, negate=False, seed=11):
    """Input of `layer` (input shape = (B, *spatial)) whose output at one voxel attains the layer's bound as closely as one voxel can.

    co* = argmax_co (|scale_co| * S_co * M + |shift_co + rshift_co|), S_co = sum |w_co| over the taps that reach `voxel` -- for M large or
    no shift this is the argmax of |scale| * sum|w_co|; with a BatchNorm and a tiny M the shift decides, as it does in the bound.
    The receptive field of `voxel` is M * sign(w[co*]) * sign(scale[co*]) * sgn, sgn = the sign of the shift at co* (so the terms add up);
    every other element is uniform in [-M, M] * background.  residual_amax = R > 0: a residual, uniform in [-R/2, R/2] with sgn * R at
    (co*, voxel).  redir_amax = Mr > 0 (layers with a fused redir): the redir input, +-Mr along its channels at `voxel` with the signs of
    the redir weights of co*, uniform in [-Mr, Mr] * background elsewhere.  negate: flip the planted pattern (the extreme value of the
    pre-activation comes out with the sign OPPOSITE to the shift; for the activation tests).
    Transposed layers: an output voxel sees one parity class of taps per dimension; `voxel` = None picks an interior voxel of the class
    with the largest sum, a given voxel is snapped to that class.  Plain layers: `voxel` = None picks the centre.

    Returns a dict: x, residual, rx (fp32 CPU tensors, NC(D)HW), voxel (b, *spatial) and co of the planted maximum, bound = gain * M + smax
    (+ R) (+ rgain * Mr + rsmax) -- the engine's formula --, attain = the value the planted voxel reaches (same terms for co* and its taps),
    frac = attain / bound, gain, smax."""
    conv, bn, rc, rbn = mods
    B, *sp = shape
    nd = len(sp)
    w = conv.weight.detach().to(torch.float64)
    if layer.kind != "conv":
        w = w.transpose(0, 1)                                    # [Co, Ci, k...]
    scale, shift = fold(conv, bn)
    rscale = rshift = rw = None
    tot_shift = shift.clone()
    if rc is not None:
        rscale, rshift = fold(rc, rbn)
        rw = rc.weight.detach().to(torch.float64).reshape(layer.co, layer.co)
        tot_shift = tot_shift + rshift
    od = out_dims(layer, sp)
    if voxel is None:
        voxel = (B - 1,) + tuple(n // 2 for n in od)
    voxel = list(voxel)
    if layer.kind != "conv":
        # parity class per dimension with the largest tap sum; classes factor over dimensions only in the index sets, so search all 2^nd
        best = None
        for cls in range(2 ** nd):
            par = [(cls >> d) & 1 for d in range(nd)]
            idx = [[kk for kk in range(layer.k) if (p + layer.pad - kk) % 2 == 0] for p in par]
            sub = w
            for d in range(nd):
                sub = sub.index_select(2 + d, torch.tensor(idx[d]))
            val = float((sub.abs().sum(dim=tuple(range(1, 2 + nd))) * scale.abs()).max())
            if best is None or val > best[0]:
                best = (val, par)
        for d in range(nd):                                      # nearest voxel of that parity whose taps all lie inside the input
            cand = [c for c in range(od[d]) if c % 2 == best[1][d]]
            voxel[1 + d] = min(cand, key=lambda c: (-len(taps_of(layer, c, sp[d])), abs(c - voxel[1 + d])))
    b = voxel[0]
    taps = [taps_of(layer, voxel[1 + d], sp[d]) for d in range(nd)]
    sub = w
    for d in range(nd):
        sub = sub.index_select(2 + d, torch.tensor([kk for kk, _ in taps[d]]))
    S = sub.abs().sum(dim=tuple(range(1, 2 + nd)))               # per co: the tap sum that reaches the voxel
    score = scale.abs() * S * M + tot_shift.abs() + (float(residual_amax)) + ((rscale.abs() * rw.abs().sum(1) * redir_amax) if rc is not None else 0.0)
    co = int(score.argmax())
    sgn = 1.0 if float(tot_shift[co]) >= 0 else -1.0
    plant = -sgn if negate else sgn
    x = _uniform((B, layer.ci, *sp), seed) * float(background)
    sc = 1.0 if float(scale[co]) >= 0 else -1.0
    ws = torch.where(sub[co] >= 0, 1.0, -1.0).to(torch.float32) * (sc * plant)      # [Ci, taps...]
    grid = torch.meshgrid(*[torch.tensor([i for _, i in taps[d]]) for d in range(nd)], indexing="ij")
    x[b][(slice(None),) + tuple(grid)] = ws                      # (adjacent index tensors: the result keeps [Ci, taps...] order)
    x = x * float(M)
    residual = rx = None
    R = float(residual_amax)
    if R > 0:
        residual = _uniform((B, layer.co, *od), seed + 1) * 0.5
        residual[(b, co) + tuple(voxel[1:])] = plant
        residual = residual * R
    Mr = float(redir_amax)
    if rc is not None:
        assert Mr > 0, "a fused redir branch needs an input"
        rx = _uniform((B, layer.co, *od), seed + 2) * float(background)
        rsc = 1.0 if float(rscale[co]) >= 0 else -1.0
        rx[(b, slice(None)) + tuple(voxel[1:])] = torch.where(rw[co] >= 0, 1.0, -1.0).to(torch.float32) * (rsc * plant)
        rx = rx * Mr
    gain, smax = bound_coef(conv, bn)
    bound = gain * M + smax + R
    attain = float(scale[co].abs() * S[co]) * M + R
    if rc is not None:
        rgain, rsmax = bound_coef(rc, rbn)
        bound += rgain * Mr + rsmax
        attain += float(rscale[co].abs() * rw[co].abs().sum()) * Mr
    attain = attain + abs(float(tot_shift[co])) if not negate else attain - abs(float(tot_shift[co]))
    return dict(x=x, residual=residual, rx=rx, voxel=tuple(voxel), co=co, bound=bound, attain=attain, frac=attain / bound, gain=gain, smax=smax)


def spike(x, voxel, value):
    """`x` with every channel of one voxel set to `value` (voxel = (b, *spatial) of x; in place, returns x): the maximum of a layer's
    output then lies within the layer's reach of that voxel"""
    x[(voxel[0], slice(None)) + tuple(voxel[1:])] = value
    return x


def background(shape, seed=5, amp=2.0 ** -6):
    """small uniform values around a spike"""
    return _uniform(shape, seed) * amp


# ----------------------------------------------------------------------------- case tables
@dataclass(frozen=True)
class ConvCase:
    """One producer form of PackedConv3d in the f16x3 mode.  form: which kernel must run, proven by the launch counters
    (osa_conv3d_march_launches / osa_conv3d_march_s2_launches / osa_deconv3d_walk_launches: +1 for the named form, unchanged for the brick
    form).  tile: (TD, TH, TW) of the form in OUTPUT voxels (0 = the form does not tile that dimension); segment: planes per D segment set
    through the library's debug setter (forms that cut D)."""
    layer: Layer
    shape: tuple                  # (B, D, H, W) of the input
    form: str                     # brick | march | march_s2 | walk
    tile: tuple
    in_split: bool = False
    out_split: bool = False
    res: str = "none"             # none | plain | split
    segment: int = 0
    note: str = ""

    @property
    def id(self):
        return self.layer.name


# Tile sizes: csrc/conv_cfgs.def through pick_cfg (csrc/conv3d.hip): 3-D stride-1 layers of small volumes take tile 3 / 4 (brick 4 x 4 x 8),
# stride-2 layers tile 15 / 5 (2 x 4 x 8), the transposed 3-D kernels own 4 x 4 x 8 INPUT positions x 8 parity classes = 8 x 8 x 16 output
# voxels, the 2-D transposed kernel 8 x 16 input pixels = 16 x 32 output pixels; the marching forms own pixel columns (stride 1: 16 x 16 or
# 8 x 32 -- 16 covers both; stride 2: 4 x 32; walking transposed: 4 x 32 or 8 x 32 input pixels = up to 16 x 64 output pixels) and cut D
# into segments.
CONV_CASES = [
    ConvCase(Layer("brick whole tiles (fast epilogue)", ci=32, co=64), (2, 4, 8, 8), "brick", (4, 4, 8),
             note="every workgroup's brick lies inside the tensor: conv_kernel.h `fast`"),
    ConvCase(Layer("brick ragged", ci=32, co=64, bn=True, act="relu"), (2, 5, 7, 37), "brick", (4, 4, 8)),
    ConvCase(Layer("brick Co % 4 != 0", ci=16, co=30, bias=True), (2, 5, 6, 11), "brick", (4, 4, 8), note="scalar stores, quads with padded lanes"),
    ConvCase(Layer("brick stride 2", ci=32, co=64, stride=2, bn=True, act="relu"), (1, 5, 7, 5), "brick", (2, 4, 8), note="fp32 tensors keep the brick form"),
    ConvCase(Layer("brick dilated", ci=32, co=32, dil=2, pad=2), (1, 5, 7, 11), "brick", (4, 4, 8)),
    ConvCase(Layer("brick k = 1", ci=32, co=32, k=1, pad=0, bn=True), (2, 3, 5, 9), "brick", (4, 4, 8)),
    ConvCase(Layer("brick split out", ci=32, co=64, bn=True), (2, 5, 7, 13), "brick", (4, 4, 8), out_split=True),
    ConvCase(Layer("march fp32 in and out", ci=32, co=32, bn=True, act="relu"), (2, 5, 7, 37), "march", (0, 16, 16)),
    ConvCase(Layer("march split chain, split residual", ci=32, co=32, bn=True), (2, 7, 11, 21), "march", (0, 16, 16), in_split=True, out_split=True, res="split"),
    ConvCase(Layer("march_s2", ci=32, co=64, stride=2, bn=True, act="leaky"), (2, 5, 7, 5), "march_s2", (0, 4, 32), in_split=True, out_split=True, segment=2),
    ConvCase(Layer("march_s2 two column tiles", ci=32, co=64, stride=2, bn=True), (1, 4, 9, 66), "march_s2", (0, 4, 32), in_split=True, out_split=True, segment=1),
    ConvCase(Layer("deconv3d k3 brick", kind="deconv3d", ci=64, co=32, k=3, pad=1, opad=1, bn=True, act="relu"), (1, 2, 5, 7), "brick", (8, 8, 16)),
    ConvCase(Layer("deconv3d k4 brick", kind="deconv3d", ci=32, co=16, k=4, pad=1, opad=0, bn=True), (2, 2, 5, 9), "brick", (8, 8, 16)),
    ConvCase(Layer("deconv3d redir brick", kind="deconv3d", ci=64, co=32, k=3, pad=1, opad=1, bn=True, act="relu", redir=True), (1, 2, 5, 7), "brick",
             (8, 8, 16), in_split=True, out_split=True),
    ConvCase(Layer("deconv3d redir walk", kind="deconv3d", ci=64, co=32, k=3, pad=1, opad=1, bn=True, act="relu", redir=True), (2, 2, 5, 7), "walk",
             (0, 16, 64), in_split=True, out_split=True, segment=2),
    ConvCase(Layer("deconv2d", kind="deconv2d", ci=32, co=32, k=3, pad=1, opad=1, bn=True, act="relu"), (2, 1, 9, 19), "brick", (0, 16, 32)),
]


def spike_targets(case: ConvCase):
    """{label: OUTPUT voxel (b, d, h, w)} the maximum is steered to.  "last D / H / W": a voxel of the last partial tile along that dimension
    (test_range_block_cases_cpu.py checks it lies past the last whole tile of case.tile); "segment": the two planes either side of the first
    D-segment boundary of a form that cuts D."""
    B = case.shape[0]
    sp = case.shape[1:]
    flat = case.layer.kind == "deconv2d"
    od = out_dims(case.layer, sp[1:]) if flat else out_dims(case.layer, sp)
    if flat:
        od = (1,) + od
    t = {"first": (0, 0, 0, 0), "last": (B - 1, od[0] - 1, od[1] - 1, od[2] - 1)}
    for d, label in enumerate(("last D", "last H", "last W")):
        if case.tile[d] and od[d] % case.tile[d]:
            v = [0, 0, 0, 0]
            v[1 + d] = od[d] - 1
            t[label] = tuple(v)
    if case.form == "march":                       # the launcher's cost model cuts D (no setter): one run per plane covers every boundary
        for d in range(od[0]):
            t[f"plane {d}"] = (B - 1, d, od[1] // 2, od[2] // 2)
    if case.segment and case.segment < od[0]:
        t["segment lower"] = (B - 1, case.segment - 1, od[1] // 2, od[2] // 2)
        t["segment upper"] = (B - 1, case.segment, od[1] // 2, od[2] // 2)
    return t


def input_voxel_for(layer: Layer, out_voxel, in_dims):
    """an input voxel (b, *spatial) inside the receptive field of an output voxel: per dimension the tap nearest the kernel's centre"""
    v = [out_voxel[0]]
    for o, n in zip(out_voxel[1:], in_dims):
        taps = taps_of(layer, o, n)
        assert taps, "an output voxel with no tap inside the tensor"
        v.append(min(taps, key=lambda t: abs(t[0] - (layer.k - 1) / 2))[1])
    return tuple(v)


# Split-output writers of the bound tests (part B): run at every M of MS with out_split=True, activation none.
BOUND_CASES = [
    ConvCase(Layer("bound brick plain", ci=32, co=64), (1, 5, 7, 13), "brick", (4, 4, 8), out_split=True),
    ConvCase(Layer("bound brick bn", ci=32, co=64, bn=True), (1, 5, 7, 13), "brick", (4, 4, 8), out_split=True),
    ConvCase(Layer("bound brick bias bn", ci=32, co=64, bias=True, bn=True), (1, 5, 7, 13), "brick", (4, 4, 8), out_split=True),
    # (a split output with an fp32 residual does not exist: the launchers refuse it -- "a split output takes a split residual";
    #  test_gpu_range_blocks.py::test_split_output_refuses_an_fp32_residual)
    ConvCase(Layer("bound brick bn split residual", ci=32, co=64, bn=True), (1, 5, 7, 13), "brick", (4, 4, 8), out_split=True, res="split"),
    ConvCase(Layer("bound march", ci=32, co=32, bn=True), (2, 5, 7, 37), "march", (0, 16, 16), in_split=True, out_split=True),
    ConvCase(Layer("bound march split residual", ci=32, co=32, bn=True), (2, 5, 7, 37), "march", (0, 16, 16), in_split=True, out_split=True, res="split"),
    ConvCase(Layer("bound march_s2", ci=32, co=64, stride=2, bn=True), (1, 5, 7, 5), "march_s2", (0, 4, 32), in_split=True, out_split=True),
    ConvCase(Layer("bound deconv redir brick", kind="deconv3d", ci=64, co=32, k=3, pad=1, opad=1, bn=True, redir=True), (1, 2, 5, 7), "brick", (8, 8, 16),
             in_split=True, out_split=True),
    ConvCase(Layer("bound deconv redir walk", kind="deconv3d", ci=64, co=32, k=3, pad=1, opad=1, bn=True, redir=True), (1, 2, 5, 7), "walk", (0, 16, 64),
             in_split=True, out_split=True),
]
# the same construction on a k = 4 transposed layer (CPU only: what one parity class can reach; no split writer of the engine's chains is k = 4)
TRANSPOSED_CPU_CASES = [c for c in BOUND_CASES if c.layer.kind != "conv"] + [
    ConvCase(Layer("bound deconv k4", kind="deconv3d", ci=32, co=16, k=4, pad=1, opad=0, bn=True), (1, 3, 5, 6), "brick", (8, 8, 16)),
    ConvCase(Layer("bound deconv2d", kind="deconv2d", ci=32, co=32, k=3, pad=1, opad=1, bn=True), (1, 1, 6, 9), "brick", (0, 16, 32)),
]


def bound_inputs(case: ConvCase, M):
    """worst_case of a bound case: the residual at the input's magnitude times 4 (it must matter next to gain * M), the redir input at M"""
    mods = modules(case.layer)
    shape = case.shape if case.layer.kind != "deconv2d" else (case.shape[0],) + tuple(case.shape[2:])
    wc = worst_case(case.layer, mods, M, shape, residual_amax=(4.0 * M if case.res != "none" else 0.0), redir_amax=(M if case.layer.redir else 0.0))
    return mods, wc


# Depthwise producers (shapes of test_gpu_parity.DW_CASES, smaller maps): name, C, (kh, kw), stride, (ph, pw), (H, W), bias, bn, act, fp16 io
DW_CASES = [
    ("dw3x3 s1 bn relu6", 16, (3, 3), 1, (1, 1), (13, 22), False, True, "relu6", False),
    ("dw3x3 s2 bn relu6", 16, (3, 3), 2, (1, 1), (14, 21), False, True, "relu6", False),
    ("row strip 1x7 bias", 16, (1, 7), 1, (0, 3), (9, 30), True, False, "none", False),
    ("column strip 7x1 bias", 16, (7, 1), 1, (3, 0), (10, 13), True, False, "none", False),
    ("dw3x3 s1 fp16 io", 16, (3, 3), 1, (1, 1), (13, 22), False, True, "relu6", True),
]

# InstanceNorm producers: name, C, Cs of the input, activation code (0 none, 1 relu, 2 leaky), (out channels, out_off) or None
IN_CASES = [
    ("none", 8, 8, 0, None),
    ("relu", 8, 8, 1, None),
    ("leaky", 8, 8, 2, None),
    ("C % 4 != 0", 6, 8, 2, None),
    ("channel slice", 8, 8, 2, (24, 8)),
]
