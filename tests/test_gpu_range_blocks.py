"""GPU: range blocks of the f16x3 mode (include/openstereo_amd.h, osa_f16x3_ranges).

Part A -- the recorded maximum IS the maximum.  Every producer runs on a fresh zeroed block; its output is read back (fp32 directly, split
tensors from their documented bytes through range_block_cases.decode_split) and ranges.amax_of(meta) is compared with the maximum of the
kernel's OWN output under range_block_cases.check_recorded_max: bit for bit for fp32 outputs, 2^-21 relative for split outputs, 2^-11 for
fp16 outputs, the inherit rule for pool2x / resize.  One spike per run steers the maximum to the places a kernel could lose it: first
voxel, last voxel of the last batch item, last partial tile along D / H / W, either side of a D-segment boundary, the last real channel of
a ragged quad.  The launch counters prove which form ran.

Part B -- the bound of split outputs is rigorous and not loose.  Every split writer runs on range_block_cases.worst_case inputs at
M in {2^-10, 1, 2^10}; the decoded output must be finite, meta[1] a power of two, max|decoded| * meta[1] inside
[(frac - 2^-19) * 2^14 / 1.0625, 2^15) with frac the attained share of the bound computed on the CPU, the values within
4 * max|ref32 - ref64| + 2^-20 * bound of the fp64 reference, and a real 3x3x3 f16x3 consumer must read the tensor to the same bar.
(The 2^-19 under frac: the accuracy bar allows the decoded maximum 2^-20 of the bound below the reference's, and the kernel evaluates the
bound in fp32 from fp32 coefficients -- four roundings of 2^-24.)"""
import contextlib
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import range_block_cases as R
from openstereo_amd.utils.weights import synth_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ----------------------------------------------------------------------------- plumbing
def _eye(c):
    m = nn.Conv3d(c, c, 1, bias=False)
    m.weight.data = torch.eye(c).reshape(c, c, 1, 1, 1).clone()
    return m


@functools.lru_cache(maxsize=None)
def _ident(c):
    from openstereo_amd.engine import PackedConv3d
    return PackedConv3d(_eye(c).to(DEV), None, 0, precision="f16x3")


def _cl(t):
    """fp32 NC(D)HW on the CPU -> NDHWC engine tensor on the GPU"""
    from openstereo_amd import ops
    if t.dim() == 4:
        t = t[:, :, None]
    return ops.to_cl(t.to(DEV).contiguous())


def _split(t):
    """... -> split NDHWC tensor (a 1x1x1 identity layer writes it: exact for values of <= 22 significant bits)"""
    return _ident(t.shape[1])(_cl(t), out_split=True)


def _amax(t):
    from openstereo_amd import ranges
    return float(ranges.amax_of(ranges.meta_of(t)))


def _read(y, co, split):
    """the kernel's own output on the CPU: fp64 [B, co, D, H, W]"""
    from openstereo_amd import ranges
    torch.cuda.synchronize()
    if split:
        return R.decode_split(y, ranges.meta_of(y).cpu())[:, :co]
    return y[:, :co].detach().cpu().double()


@functools.lru_cache(maxsize=None)
def _engine(layer):
    """(CPU torch modules, engine layer, engine redir layer or None) of a Layer"""
    from openstereo_amd.engine import PackedConv3d
    mods = R.modules(layer)
    gpu = lambda m: None if m is None else copy.deepcopy(m).to(DEV)
    with torch.no_grad():
        pc = PackedConv3d(gpu(mods[0]), gpu(mods[1]), R.ACT_CODE[layer.act], layer.slope, precision="f16x3")
        prl = PackedConv3d(gpu(mods[2]), gpu(mods[3]), 0, precision="f16x3") if layer.redir else None
    return mods, pc, prl


EXPECT = {"brick": (0, 0, 0), "march": (1, 0, 0), "march_s2": (0, 1, 0), "walk": (0, 0, 1)}


@contextlib.contextmanager
def _form(lib, case):
    """select the form of `case` (the switches are restored) and hand out a runner that proves it by the launch counters"""
    counters = lambda: (lib.osa_conv3d_march_launches(), lib.osa_conv3d_march_s2_launches(), lib.osa_deconv3d_walk_launches())
    prev_walk = lib.osa_deconv_walk(3 if case.form == "walk" else 0)
    prev_wp = lib.osa_deconv_walk_segment_planes(case.segment if case.form == "walk" else 0)
    prev_s2 = lib.osa_conv_march_s2_segment_planes(case.segment if case.form == "march_s2" else 0)

    def run(fn):
        n0 = counters()
        y = fn()
        got = tuple(a - b for a, b in zip(counters(), n0))
        assert got == EXPECT[case.form], f"[{case.id}] expected the {case.form} form, launch counters moved by {got} (march, march_s2, walk)"
        return y
    try:
        yield run
    finally:
        lib.osa_deconv_walk(prev_walk)
        lib.osa_deconv_walk_segment_planes(prev_wp)
        lib.osa_conv_march_s2_segment_planes(prev_s2)


def _launch(case, run, x, residual=None, rx=None, out=None, out_off=0, out_split=None):
    """one launch of the case's layer on CPU inputs; returns (y, the engine's input tensors)"""
    _, pc, prl = _engine(case.layer)
    xs = _split(x) if case.in_split else _cl(x)
    rs = None
    if residual is not None:
        rs = _split(residual) if case.res == "split" else _cl(residual)
    kw = dict(out_split=case.out_split if out_split is None else out_split)
    if out is not None:
        kw.update(out=out, out_off=out_off)
    if case.layer.redir:
        rxs = _split(rx) if case.in_split else _cl(rx)
        y = run(lambda: pc(xs, redir=(prl, rxs), **kw))
        return y, (xs, rs, rxs)
    y = run(lambda: pc(xs, residual=rs, **kw))
    return y, (xs, rs, None)


def _shapes(case):
    """(input shape without channels, output spatial dims) as the CPU modules see them (2-D layers: no D)"""
    flat = case.layer.kind == "deconv2d"
    shape = (case.shape[0],) + tuple(case.shape[2:] if flat else case.shape[1:])
    return flat, shape, R.out_dims(case.layer, shape[1:])


def _argmax(t):
    return tuple(int(i) for i in np.unravel_index(int(t.abs().argmax()), t.shape))


# ============================================================================= part A: the recorded maximum
@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c.id)
def test_conv_recorded_maximum_follows_the_spike(case, lib):
    """PackedConv3d in every form of the table: one spike per run; the recorded maximum equals the maximum of the stored values and the
    stored maximum lies within the layer's reach of the spike."""
    lay = case.layer
    flat, shape, od = _shapes(case)
    B = shape[0]
    with torch.no_grad(), _form(lib, case) as run:
        for label, ov in R.spike_targets(case).items():
            ovs = (ov[0],) + tuple(ov[2:] if flat else ov[1:])
            iv = R.input_voxel_for(lay, ovs, shape[1:])
            x = R.spike(R.background((B, lay.ci) + shape[1:]), iv, 4.0)
            res = R.background((B, lay.co) + od, seed=6) if case.res != "none" else None
            rx = R.background((B, lay.co) + od, seed=7) if lay.redir else None
            y, _ = _launch(case, run, x, res, rx)
            got = _read(y, lay.co, case.out_split)
            what = f"[{case.id}] spike -> {label} {ov}"
            R.check_recorded_max(_amax(y), got, "split" if case.out_split else "f32", what)
            am = _argmax(got)
            pos = am[3:] if flat else am[2:]
            assert am[0] == iv[0] and R.within_reach(lay, iv[1:], pos, shape[1:]), f"{what}: the stored maximum sits at {am}, out of reach of the spike at {iv}"


def _ragged_layer(act, bias_value):
    """16 -> 30 channels (a last quad with two padded lanes), the last real channel's weights 8x the others"""
    from openstereo_amd.engine import PackedConv3d
    conv = nn.Conv3d(16, 30, 3, 1, 1, bias=True)
    conv.weight.data = synth_tensor("ragged quad.w", conv.weight.shape, 1)
    conv.weight.data[29] *= 8.0
    conv.bias.data = torch.full((30,), float(bias_value))
    with torch.no_grad():
        return conv, PackedConv3d(copy.deepcopy(conv).to(DEV), None, R.ACT_CODE[act], precision="f16x3")


def test_last_real_channel_of_a_ragged_quad(lib):
    """Co % 4 != 0: the maximum in the last real channel (29 of 30) is recorded exactly"""
    conv, pc = _ragged_layer("none", 0.0)
    x = R.spike(R.background((2, 16, 5, 6, 11)), (1, 4, 5, 10), 4.0)
    with torch.no_grad():
        y = pc(_cl(x))
    got = _read(y, 30, False)
    assert float(y[:, 30:].abs().max()) == 0.0, "padded channels of a fresh output are zero"
    R.check_recorded_max(_amax(y), got, "f32", "Co = 30, maximum in channel 29")
    assert _argmax(got)[1] == 29


@pytest.mark.parametrize("act", ["sigmoid", "tanh", "relu"])
def test_padded_lanes_of_a_ragged_quad_do_not_count(act, lib):
    """Co % 4 != 0 with every real output far below what a padded lane would give: the pre-activation of every real channel is about -8
    (sigmoid: 3e-4, tanh: -1, relu: 0) while a padded lane holds act(0) (sigmoid: 0.5).  Only stored values may be folded."""
    conv, pc = _ragged_layer(act, -8.0)
    x = R.background((1, 16, 5, 6, 11))
    with torch.no_grad():
        y = pc(_cl(x))
    got = _read(y, 30, False)
    R.check_recorded_max(_amax(y), got, "f32", f"Co = 30, {act}, bias -8")


EPILOGUE_FORMS = [
    R.ConvCase(R.Layer("epilogue brick", ci=32, co=64), (2, 5, 7, 13), "brick", (4, 4, 8)),
    R.ConvCase(R.Layer("epilogue brick whole tiles", ci=32, co=64), (1, 4, 8, 8), "brick", (4, 4, 8)),
    R.ConvCase(R.Layer("epilogue march", ci=32, co=32), (2, 5, 7, 21), "march", (0, 16, 16)),
]
# (the marching form takes none / relu / leaky only, conv_march.hip: ReLU6 and sigmoid layers of its geometry run as bricks)
EPILOGUES = [(b, v) for b in EPILOGUE_FORMS for v in ("residual only", "relu", "leaky", "relu6", "sigmoid") if not (b.form == "march" and v in ("relu6", "sigmoid"))]


@pytest.mark.parametrize("base,variant", EPILOGUES, ids=[f"{b.id}-{v}" for b, v in EPILOGUES])
def test_epilogue_variants_record_the_stored_value(base, variant, lib):
    """The maximum is taken AFTER the residual and the activation: a residual-only maximum (conv input near 0); ReLU / LeakyReLU / sigmoid
    with the largest pre-activation magnitude negative (ReLU: it must not count; leaky: the scaled value counts); ReLU6 saturated."""
    import dataclasses
    act = "none" if variant == "residual only" else variant
    lay = dataclasses.replace(base.layer, name=f"{base.layer.name} {variant}", act=act)
    case = dataclasses.replace(base, layer=lay, res="plain" if variant == "residual only" else "none")
    mods, _, _ = _engine(lay)
    B, *sp = case.shape
    with torch.no_grad(), _form(lib, case) as run:
        if variant == "residual only":
            x = R.background((B, lay.ci, *sp), amp=2.0 ** -20)
            voxel = (B - 1, sp[0] - 1, sp[1] - 1, sp[2] - 1)
            res = R.spike(R.background((B, lay.co, *sp), seed=6), voxel, -5.0)
            y, _ = _launch(case, run, x, res)
            got = _read(y, lay.co, False)
            R.check_recorded_max(_amax(y), got, "f32", f"[{case.id}]")
            am = _argmax(got)
            assert (am[0],) + am[2:] == voxel and abs(float(got.abs().max()) - 5.0) < 1e-3
            return
        wc = R.worst_case(lay, mods, 1.0, case.shape, background=2.0 ** -4, negate=variant != "relu6")
        y, _ = _launch(case, run, wc["x"])
        got = _read(y, lay.co, False)
        top = float(got.abs().max())
        print(f"[{case.id}] pre-activation extreme {wc['attain']:.4g}, stored maximum {top:.6g}, recorded {_amax(y):.6g}")
        R.check_recorded_max(_amax(y), got, "f32", f"[{case.id}]")
        planted = (wc["voxel"][0], wc["co"]) + tuple(wc["voxel"][1:])
        if variant == "relu":
            assert float(got[planted]) == 0.0 and top < 0.5 * wc["attain"], "the negative extreme must be cut, the maximum lies elsewhere"
        elif variant == "leaky":
            assert _argmax(got) == planted and float(got[planted]) < 0 and abs(top - lay.slope * wc["attain"]) <= 1e-4 * top
        elif variant == "relu6":
            assert top == 6.0 and float(got[planted]) == 6.0 and wc["attain"] > 12.0
        else:
            assert 0.0 < top < 1.0 and float(got[planted]) < 1e-6


def _slice_layer(form):
    if form == "march":
        return R.ConvCase(R.Layer("slice march", ci=32, co=32, bn=True), (1, 5, 7, 21), "march", (0, 16, 16), in_split=True, out_split=True)
    if form == "split":
        return R.ConvCase(R.Layer("slice brick split", ci=32, co=16, bn=True), (1, 5, 7, 13), "brick", (4, 4, 8), out_split=True)
    return R.ConvCase(R.Layer("slice brick", ci=32, co=16, bn=True), (1, 5, 7, 13), "brick", (4, 4, 8))


@pytest.mark.parametrize("form", ["fp32", "split", "march"])
def test_block_lifecycle_running_maximum_slices_and_preloaded_slots(form, lib):
    """Channel-slice outputs (out_off, wider yCs): the untouched channels -- filled with 1e30 -- do not count; a second producer writing
    another slice of the same buffer, first with smaller, then with larger values, leaves the running maximum of everything written;
    a slot pre-loaded below / above the true maximum (what the early peek reads) gives max(old, true) in every slot arrangement."""
    from openstereo_amd import ops, ranges
    case = _slice_layer(form)
    lay = case.layer
    co, split = lay.co, case.out_split
    B, *sp = case.shape
    wide = 3 * co if co == 16 else 2 * co + 32                    # 48 or 96 channels: slices at 16-aligned offsets
    offs = (co, 0)
    x = R.background((B, lay.ci, *sp), amp=1.0)
    with torch.no_grad(), _form(lib, case) as run:
        out = ops.empty_cl(B, wide, *sp, torch.device(DEV))
        out.fill_(1e30)
        y, _ = _launch(case, run, x, out=out, out_off=offs[0])
        assert y is out
        meta = ranges.meta_of(out)
        rd = lambda off: (R.decode_split(out, meta.cpu(), channels=(off, co)) if split else out[:, off:off + co].cpu().double())
        torch.cuda.synchronize()
        a_first = rd(offs[0])
        kind = "split" if split else "f32"
        R.check_recorded_max(_amax(out), a_first, kind, f"[{case.id}] slice at {offs[0]} of {wide} channels")
        untouched = torch.cat([out[:, :offs[0]], out[:, offs[0] + co:]], 1)
        assert bool((untouched == 1e30).all()), "channels outside the output slice were written"
        if split:
            return      # (a split buffer has ONE scale: two split writers of one buffer do not occur -- the running maximum is tested on fp32 slices)
        # second producer, smaller values: the maximum stays; then larger values: it moves
        _launch(case, run, x * 2.0 ** -4, out=out, out_off=offs[1])
        torch.cuda.synchronize()
        both = torch.cat([rd(offs[0]), rd(offs[1])], 1)
        R.check_recorded_max(_amax(out), both, kind, f"[{case.id}] second slice, smaller values")
        assert float(both.abs().max()) == float(a_first.abs().max())
        _launch(case, run, x * 2.0 ** 4, out=out, out_off=offs[1])
        torch.cuda.synchronize()
        both = torch.cat([rd(offs[0]), rd(offs[1])], 1)
        R.check_recorded_max(_amax(out), both, kind, f"[{case.id}] second slice, larger values")
        assert float(both.abs().max()) > 8.0 * float(a_first.abs().max())
        # pre-loaded slots
        true = float(a_first.abs().max())
        for old in (true * 0.25, true * 4.0):
            fresh = ops.empty_cl(B, wide, *sp, torch.device(DEV))
            m = ranges.attach_meta(fresh)
            m[0:ranges.META_FLOATS:16] = old
            _launch(case, run, x, out=fresh, out_off=offs[0])
            torch.cuda.synchronize()
            assert _amax(fresh) == max(old, true), f"[{case.id}] slot pre-loaded with {old!r}: recorded {_amax(fresh)!r}, true maximum {true!r}"
            slots = m[0:ranges.META_FLOATS:16].cpu()
            assert bool((slots >= old).all()) and bool((slots <= max(old, true)).all())


@pytest.mark.parametrize("case", R.DW_CASES, ids=[c[0] for c in R.DW_CASES])
def test_depthwise_recorded_maximum(case):
    from openstereo_amd.engine import DepthwiseConv2d
    name, C, k, s, p, (H, W), bias, use_bn, act, f16 = case
    conv = nn.Conv2d(C, C, k, s, p, groups=C, bias=bias)
    conv.weight.data = synth_tensor(name + ".w", conv.weight.shape, 1)
    if bias:
        conv.bias.data = synth_tensor(name + ".bias", conv.bias.shape, 1)
    bn = R._bn(C, name + ".bn", 2) if use_bn else None
    with torch.no_grad():
        dw = DepthwiseConv2d(conv.to(DEV), None if bn is None else bn.to(DEV), {"none": 0, "relu6": 3}[act])
        for label, voxel in (("first", (0, 0, 0)), ("last", (1, H - 1, W - 1)), ("last row", (0, H - 1, 0)), ("last column", (0, 0, W - 1))):
            x = R.spike(R.background((2, C, H, W), amp=0.25), voxel, 2.0)
            x[voxel[0], C - 1, voxel[1], voxel[2]] = -3.0                      # the last channel carries the largest value
            xc = _cl(x)
            y = dw(xc.half() if f16 else xc, out_f16=f16) if f16 else dw(xc)
            torch.cuda.synchronize()
            assert y.dtype == (torch.float16 if f16 else torch.float32)
            got = y.float().cpu()
            R.check_recorded_max(_amax(y), got, "f16" if f16 else "f32", f"[{name}] spike at {label}")
            am = _argmax(got)
            assert am[0] == voxel[0] and abs(am[3] * s - voxel[1]) <= k[0] // 2 + s - 1 and abs(am[4] * s - voxel[2]) <= k[1] // 2 + s - 1, (label, am)


@pytest.mark.parametrize("case", R.IN_CASES, ids=[c[0] for c in R.IN_CASES])
def test_instance_norm_recorded_maximum(case):
    from openstereo_amd import ops, ranges
    from openstereo_amd.models.feature_pyramid import instance_norm_act_cl
    name, C, Cs, act, sl = case
    B, H, W = 2, 9, 13
    with torch.no_grad():
        for label, voxel in (("first", (0, 0, 0)), ("last", (1, H - 1, W - 1))):
            x = R.background((B, Cs, H, W), amp=1.0)
            x[:, C:] = 0.0
            x[voxel[0], C - 1, voxel[1], voxel[2]] = -40.0 if act == 2 else 40.0     # leaky: the scaled negative value is the maximum
            x[voxel[0], 0, voxel[1], voxel[2]] = -60.0 if act == 1 else 0.0          # relu: a larger negative value must not count
            xc = _cl(x)
            ranges.ensure_meta(xc)
            out, off = None, 0
            if sl is not None:
                out = ops.empty_cl(B, sl[0], 1, H, W, torch.device(DEV))
                out.fill_(1e30)
                off = sl[1]
            y = instance_norm_act_cl(xc, C, act=act, slope=0.5, out=out, out_off=off)
            torch.cuda.synchronize()
            got = y[:, off:off + C].cpu()
            R.check_recorded_max(_amax(y), got, "f32", f"[instnorm {name}] spike at {label}")
            am = _argmax(got)
            assert (am[0], am[3], am[4]) == voxel and am[1] == C - 1, (label, am)
            if sl is not None:
                assert bool((y[:, :off] == 1e30).all()) and bool((y[:, off + (C + 3) // 4 * 4:] == 1e30).all())


def test_gru_loop_helpers_recorded_maximum():
    """gru_combine (running maximum of the level buffer), pool2x and the bilinear resize through _resample_into (inherit the source's
    block), disp_update (two blocks)."""
    from openstereo_amd import _ext, ops, ranges
    from openstereo_amd.models.igev_update import _resample_into, interp, pool2x
    ext = _ext.load()
    dev = torch.device(DEV)
    B, H, W, hd, cx = 2, 9, 13, 8, 8
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        # ---- gru_combine: T = [h | x | r*h | z], h <- (1 - z) h + z q
        for label, px, first_max in (("first", (0, 0, 0), 0.0), ("last", (B - 1, H - 1, W - 1), 0.0), ("running", (0, 4, 6), 50.0)):
            T = ops.empty_cl(B, 3 * hd + cx, 1, H, W, dev)
            T.copy_(torch.rand(T.shape, generator=g).to(dev))
            q = ops.empty_cl(B, hd, 1, H, W, dev)
            q.copy_((torch.rand(q.shape, generator=g) * 2 - 1).to(dev))
            q[px[0], hd - 1, 0, px[1], px[2]] = -9.0
            T[px[0], 2 * hd + cx + hd - 1, 0, px[1], px[2]] = 1.0           # z = 1 there: h takes q
            m = ranges.attach_meta(T)
            m[16] = first_max                                                # what an earlier producer of the buffer left
            ext.gru_combine(T, 2 * hd + cx, q, T, T, [B * H * W, hd, T.shape[1], q.shape[1], T.shape[1], T.shape[1]], m)
            torch.cuda.synchronize()
            hnew = T[:, :hd].cpu()
            assert float(hnew.abs().max()) == 9.0 and _argmax(hnew) == (px[0], hd - 1, 0, px[1], px[2])
            assert _amax(T) == max(9.0, first_max), f"gru_combine [{label}]: recorded {_amax(T)!r}"
        # ---- pool2x / resize: the destination inherits the source's maximum
        for label, px in (("first", (0, 0, 0)), ("last", (B - 1, H - 1, W - 1))):
            x = R.spike(R.background((B, 8, H, W), amp=1.0), px, -7.0)
            xc = _cl(x)
            ranges.ensure_meta(xc)
            src = _amax(xc)
            assert src == 7.0
            y = pool2x(xc)
            torch.cuda.synchronize()
            R.check_recorded_max(_amax(y), y.cpu(), "inherit", f"pool2x [{label}]", src_amax=src)
            dest = ops.empty_cl(B, 8, 1, 2 * H - 1, 2 * W - 1, dev)
            y = interp(xc, dest)
            torch.cuda.synchronize()
            assert float(y.abs().max()) == 7.0, "align_corners resize to 2n - 1 reproduces the source pixels"
            R.check_recorded_max(_amax(y), y.cpu(), "inherit", f"resize [{label}]", src_amax=src)
            # into a channel slice of a level buffer that has a block of its own
            lvl = ops.empty_cl(B, 24, 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1, dev)
            lvl.zero_()
            ranges.attach_meta(lvl)
            _resample_into("pool", xc, 8, lvl, 8)
            torch.cuda.synchronize()
            R.check_recorded_max(_amax(lvl), lvl.cpu(), "inherit", f"pool2x into a slice [{label}]", src_amax=src)
            assert float(lvl[:, :8].abs().max()) == 0.0 and float(lvl[:, 16:].abs().max()) == 0.0
        # ---- disp_update: disp += delta; copies in an NHWC [disp, 0, 0, 0] map and one channel of the level buffer; two blocks
        n = B * H * W
        for label, i in (("first", 0), ("last", n - 1)):
            disp = torch.rand(B, 1, H, W, generator=g).to(dev)
            delta = ops.empty_cl(B, 4, 1, H, W, dev)
            delta.copy_((torch.rand(delta.shape, generator=g) - 0.5).to(dev))
            delta.permute(0, 2, 3, 4, 1).reshape(n, 4)[i, 0] = -33.0
            disp4 = ops.empty_cl(B, 4, 1, H, W, dev)
            lvl = ops.empty_cl(B, 16, 1, H, W, dev)
            lvl.fill_(0.5)
            m4, ml = ranges.attach_meta(disp4), ranges.attach_meta(lvl)
            ml[0] = 0.5
            ext.disp_update(disp, delta, 4, disp4, lvl, 11, 16, n, m4, ml)
            torch.cuda.synchronize()
            R.check_recorded_max(_amax(disp4), disp4.cpu(), "f32", f"disp_update map [{label}]")
            R.check_recorded_max(_amax(lvl), lvl.cpu(), "f32", f"disp_update level slot [{label}]")
            assert torch.equal(disp4[:, 0], lvl[:, 11]) and torch.equal(disp4[:, 0, 0], disp[:, 0]) and float(disp4[:, 1:].abs().max()) == 0.0
            assert int(disp.flatten().abs().argmax()) == i


def test_layout_recorded_maximum():
    """ops.to_cl output entering an f16x3 layer: its block comes from osa_amax_f32 (ranges.ENGINE_AMAX) or torch's norm -- exact either way,
    also with the maximum in the first / last element and in a channel-padded tensor."""
    from openstereo_amd import ranges
    old = ranges.ENGINE_AMAX
    try:
        for use_kernel in (False, True):
            ranges.ENGINE_AMAX = use_kernel
            for C in (32, 7):
                for px in ((0, 0, 0, 0), (1, 2, 4, 6)):
                    x = R.background((2, C, 3, 5, 7), amp=1.0)
                    x[px[0], C - 1 if px[0] else 0, px[1], px[2], px[3]] = -11.0
                    xc = _cl(x)
                    assert _argmax(xc.cpu()) == (px[0], C - 1 if px[0] else 0) + px[1:]
                    got = float(ranges.amax_of(ranges.input_meta(xc)))
                    assert got == 11.0 == float(xc.abs().max()), (use_kernel, C, px, got)
    finally:
        ranges.ENGINE_AMAX = old


VOLUME_CASES = [
    # name, B, gwc channels, groups, concat channels, H, W, D
    ("gwcnet ragged", 2, 320, 40, 12, 5, 75, 21),
    ("concat only", 1, 0, 0, 16, 4, 130, 12),
]


def _volume_features(case, M=1.0, signs=False, spike_at=None):
    """channels-last feature pair (left images first).  signs: every channel of a pixel is +M or -M (one sign per pixel): the group-wise
    correlation then attains max|f|^2 and the concatenation max|f_cat|."""
    from openstereo_amd import ops, ranges
    name, B, C, G, Cc, H, W, D = case
    rng = np.random.default_rng(5)
    mk = lambda ch: (np.sign(rng.uniform(-1, 1, (2 * B, 1, 1, H, W))) * np.ones((1, ch, 1, 1, 1)) if signs
                     else rng.uniform(-1, 1, (2 * B, ch, 1, H, W))).astype(np.float32) * M
    gf = ops.empty_cl(2 * B, max(C, 4), 1, H, W, torch.device(DEV))
    cf = ops.empty_cl(2 * B, Cc, 1, H, W, torch.device(DEV))
    g, c = torch.from_numpy(mk(max(C, 4))), torch.from_numpy(mk(Cc))
    if spike_at is not None:
        b, h, w = spike_at
        for t in (g, c):
            t[b, :, 0, h, w] = 8.0 * M                     # left image ...
            t[B + b, :, 0, h, w] = 8.0 * M                 # ... and the right image's pixel that disparity 0 pairs it with
    gf.copy_(g.to(DEV)); cf.copy_(c.to(DEV))
    ranges.ensure_meta(gf); ranges.ensure_meta(cf)
    return gf, cf


@pytest.mark.parametrize("form", ["fp32", "walking", "split"])
@pytest.mark.parametrize("case", VOLUME_CASES, ids=lambda c: c[0])
def test_volume_builder_recorded_maximum(case, form, lib):
    from openstereo_amd import ops, ranges
    from openstereo_amd.engine import is_split
    name, B, C, G, Cc, H, W, D = case
    prev = lib.osa_volume_walk_step(0) if form == "fp32" else None          # (0: the chunked kernel; the other forms run as shipped)
    try:
        for label, px in (("first", (0, 0, 0)), ("last", (B - 1, H - 1, W - 1))):
            gf, cf = _volume_features(case, spike_at=px)
            n0 = lib.osa_volume_walk_launches()
            v = ops.build_cost_volume_from_cl(gf, G, cf, B, D, gwc_channels=C, out_split=form == "split")
            torch.cuda.synchronize()
            if form == "fp32":
                assert lib.osa_volume_walk_launches() == n0, "the chunked kernel was asked for"
            elif form == "walking":
                assert lib.osa_volume_walk_launches() == n0 + 1, "the walking form did not run"
            assert is_split(v) == (form == "split"), "the call qualifies for the split form"
            nch = G + 2 * Cc
            got = _read(v, nch, form == "split")
            R.check_recorded_max(_amax(v), got, "split" if form == "split" else "f32", f"[volume {name} {form}] spike at {label}")
            am = _argmax(got)
            assert (am[0], am[3], am[4]) == px, (label, am)
    finally:
        if prev is not None:
            lib.osa_volume_walk_step(prev)


# ============================================================================= part B: the bound of split outputs
def _consumer(ci):
    from openstereo_amd.engine import PackedConv3d
    conv = nn.Conv3d(ci, 32, 3, 1, 1, bias=False)
    conv.weight.data = synth_tensor(f"consumer{ci}.w", conv.weight.shape, 1)
    with torch.no_grad():
        return conv, PackedConv3d(copy.deepcopy(conv).to(DEV), None, 0, precision="f16x3")


def _check_split_tensor(what, y, dec, frac, bound, ref64, ref32):
    """the assertions every split writer must meet (module docstring, part B); prints the figures"""
    from openstereo_amd import ranges
    s = float(ranges.meta_of(y)[1])
    top = float(dec.abs().max())
    err = float((dec - ref64).abs().max())
    own = float((ref32.double() - ref64).abs().max())
    bar = 4.0 * own + 2.0 ** -20 * bound
    lo, hi = R.scale_window(frac - 2.0 ** -19)
    print(f"{what}: frac = {frac:.4f}, bound = {bound:.6g}, meta[1] = 2^{np.log2(s):.0f}, max|decoded| * meta[1] = {top * s:.1f} in [{lo:.1f}, {hi:.0f}); "
          f"error {err:.3e} <= 4 * {own:.3e} + 2^-20 * bound = {bar:.3e}")
    assert bool(torch.isfinite(dec).all()), f"{what}: the split output overflowed"
    assert R.is_pow2(s), f"{what}: meta[1] = {s!r} is not a power of two"
    assert lo <= top * s < hi, f"{what}: max|decoded| * meta[1] = {top * s!r} outside [{lo!r}, {hi!r})"
    assert err <= bar, f"{what}: error {err:.3e} above the bar {bar:.3e}"


def _check_consumer(what, y, dec):
    """a real 3x3x3 f16x3 layer reads the split tensor: against fp64 on the decoded values, same bar"""
    from openstereo_amd import ranges
    conv, pc = _consumer(y.shape[1])
    with torch.no_grad():
        z = pc(y)
        torch.cuda.synchronize()
        full = R.decode_split(y, ranges.meta_of(y).cpu())
        ref64 = copy.deepcopy(conv).double()(full)
        ref32 = conv(full.float())
    gain, _ = R.bound_coef(conv, None)
    bound = gain * _amax(y)
    err = float((z[:, :32].cpu().double() - ref64).abs().max())
    own = float((ref32.double() - ref64).abs().max())
    bar = 4.0 * own + 2.0 ** -20 * bound
    print(f"{what}: consumer error {err:.3e} <= 4 * {own:.3e} + 2^-20 * {bound:.6g} = {bar:.3e}")
    assert bool(torch.isfinite(z).all()) and err <= bar, f"{what}: the consumer is off by {err:.3e} (bar {bar:.3e})"
    R.check_recorded_max(_amax(z), z[:, :32].cpu(), "f32", what + " consumer")


@pytest.mark.parametrize("M", R.MS, ids=lambda m: f"M=2^{int(np.log2(m))}")
@pytest.mark.parametrize("case", R.BOUND_CASES, ids=lambda c: c.id)
def test_split_output_bound_is_rigorous_and_tight(case, M, lib):
    from openstereo_amd import ranges
    lay = case.layer
    mods, wc = R.bound_inputs(case, M)
    _, pc, prl = _engine(lay)
    # the coefficients the kernel multiplies are the formula's
    coef = pc.coef.cpu().double()
    assert abs(float(coef[0]) - wc["gain"]) <= 2.0 ** -22 * wc["gain"] and abs(float(coef[1]) - wc["smax"]) <= 2.0 ** -22 * max(wc["smax"], 1e-30)
    with torch.no_grad(), _form(lib, case) as run:
        y, (xs, rs, rxs) = _launch(case, run, wc["x"], wc["residual"], wc["rx"])
        torch.cuda.synchronize()
        assert (_amax(xs) if case.in_split else float(xs.abs().max())) == M, "the operand's maximum is M"
        # the values the kernel really read (split operands carry 22 bits)
        dec_of = lambda t, s: None if t is None else (R.decode_split(t, ranges.meta_of(t).cpu()) if s else t.cpu().double())
        x64, r64, rx64 = dec_of(xs, case.in_split), dec_of(rs, case.res == "split"), dec_of(rxs, case.in_split)
        ref64 = R.reference(lay, mods, x64, r64, rx64)
        ref32 = R.reference(lay, mods, x64.float(), None if r64 is None else r64.float(), None if rx64 is None else rx64.float(), dtype=torch.float32)
        dec = _read(y, lay.co, True)
        what = f"[{case.id}] M = {M:g}"
        frac = float(ref64.abs().max()) / wc["bound"]
        assert abs(frac - wc["frac"]) <= 2.0 ** -20, "the operands the kernel read attain what the CPU case attains"
        _check_split_tensor(what, y, dec, wc["frac"], wc["bound"], ref64, ref32)
        R.check_recorded_max(_amax(y), dec, "split", what)
        planted = (wc["voxel"][0], wc["co"]) + tuple(wc["voxel"][1:])
        assert _argmax(dec) == planted
        _check_consumer(what, y, dec)


def test_split_output_refuses_an_fp32_residual(lib):
    """The split epilogue reads its residual as hi / lo halves: an fp32 residual must be refused loudly, never misread (so the
    `+ max|residual|` term of the bound only ever meets split residuals)."""
    case = R.ConvCase(R.Layer("bound brick bn split residual", ci=32, co=64, bn=True), (1, 5, 7, 13), "brick", (4, 4, 8), out_split=True, res="plain")
    x, res = R.background((1, 32, 5, 7, 13)), R.background((1, 64, 5, 7, 13), seed=6)
    with torch.no_grad(), pytest.raises(Exception, match="split residual"):
        _launch(case, lambda fn: fn(), x, res)


@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
def test_sigmoid_and_tanh_split_outputs_of_a_tiny_input(act, lib):
    """coef[0] * 2^-10 + coef[1] is below what sigmoid (0.5 and more everywhere) gives, and the activations are bounded by 1 whatever the
    coefficients say: the kernel's `bound = 1` rule must hold the output."""
    case = R.ConvCase(R.Layer(f"tiny {act}", ci=32, co=32, bias=True, act=act), (1, 5, 7, 13), "brick", (4, 4, 8), out_split=True)
    lay = case.layer
    mods, pc, _ = _engine(lay)
    M = 2.0 ** -10
    wc = R.worst_case(lay, mods, M, case.shape)
    with torch.no_grad(), _form(lib, case) as run:
        y, _ = _launch(case, run, wc["x"])
        ref64 = R.reference(lay, mods, wc["x"].double())
        ref32 = R.reference(lay, mods, wc["x"], dtype=torch.float32)
        dec = _read(y, lay.co, True)
    assert wc["bound"] < 0.45, "the coefficient bound alone would be too small"
    top = float(ref64.abs().max())
    _check_split_tensor(f"[tiny {act}]", y, dec, top / 1.0, 1.0, ref64, ref32)
    R.check_recorded_max(_amax(y), dec, "split", f"[tiny {act}]")
    _check_consumer(f"[tiny {act}]", y, dec)


@pytest.mark.parametrize("M", R.MS, ids=lambda m: f"M=2^{int(np.log2(m))}")
@pytest.mark.parametrize("case", VOLUME_CASES, ids=lambda c: c[0])
def test_split_volume_bound(case, M, lib):
    """The split volume builder: |gwc| <= max|f|^2, |concat| <= max|f_cat|, attained by constant-sign feature rows at +-M (frac = 1)."""
    from openstereo_amd import ops, ranges
    from openstereo_amd.engine import is_split
    name, B, C, G, Cc, H, W, D = case
    gf, cf = _volume_features(case, M=M, signs=True)
    v32 = ops.build_cost_volume_from_cl(gf, G, cf, B, D, gwc_channels=C)
    vs = ops.build_cost_volume_from_cl(gf, G, cf, B, D, gwc_channels=C, out_split=True)
    torch.cuda.synchronize()
    assert is_split(vs) and not is_split(v32)
    bound = max(M * M if C else 0.0, M)
    nch = G + 2 * Cc
    dec = _read(vs, nch, True)
    ref32 = v32[:, :nch].cpu()
    ref64 = ref32.double()                  # products and means of +-M, M a power of two: the fp32 volume is exact
    assert float(ref64.abs().max()) == bound
    _check_split_tensor(f"[split volume {name}] M = {M:g}", vs, dec, 1.0, bound, ref64, ref32)
    R.check_recorded_max(_amax(vs), dec, "split", f"[split volume {name}]")
    if nch % 16 == 0:
        _check_consumer(f"[split volume {name}] M = {M:g}", vs, dec)
