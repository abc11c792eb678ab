"""CPU: the inputs and readers of tests/test_gpu_range_blocks.py do what they claim, so the GPU tests cannot pass vacuously.

* worst_case() inputs make the fp64 torch reference attain >= 0.9 of the bound the engine formula gives (conv layers), or of what the best
  single parity class can reach (stride-2 transposed layers), and the maximum sits at the planted (channel, voxel);
* decode_split() reads hand-built bytes;
* the voxels the spike tests call "last partial tile" lie past the last whole tile of the form's stated tile size, and a spike's maximum
  lies within the layer's reach of it."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import range_block_cases as R

CONV_BOUND = [c for c in R.BOUND_CASES if c.layer.kind == "conv"]


def _engine_formula(conv, bn):
    """PackedConv3d.__init__ (engine.py, "output bound of this layer"): wsum over every dim but the output channels' -- dim 0 of a transposed
    weight is the INPUT channel axis --, gain = max(wsum * |scale|), smax = max |shift| with the bias folded as bias * scale + shift."""
    w = conv.weight.detach().double()
    transposed = isinstance(conv, (nn.ConvTranspose3d, nn.ConvTranspose2d))
    wsum = w.abs().sum(dim=(0, 2, 3, 4) if (transposed and w.dim() == 5) else ((0, 2, 3) if transposed else (1, 2, 3, 4)))
    scale = shift = None
    if bn is not None:
        scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        shift = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
    if conv.bias is not None:
        b = conv.bias.detach().double()
        if bn is None:
            shift, scale = b, torch.ones_like(b)
        else:
            shift = shift + b * scale
    gain = float((wsum * scale.abs()).max()) if scale is not None else float(wsum.max())
    smax = float(shift.abs().max()) if shift is not None else 0.0
    return gain, smax


def _argmax(t):
    return tuple(int(i) for i in np.unravel_index(int(t.abs().argmax()), t.shape))


@pytest.mark.parametrize("M", R.MS, ids=lambda m: f"M=2^{int(np.log2(m))}")
@pytest.mark.parametrize("case", CONV_BOUND, ids=lambda c: c.id)
def test_conv_worst_case_reaches_the_bound(case, M):
    mods, wc = R.bound_inputs(case, M)
    gain, smax = _engine_formula(mods[0], mods[1])
    bound = gain * M + smax + (4.0 * M if case.res != "none" else 0.0)
    assert bound == pytest.approx(wc["bound"], rel=1e-12), "the helper's bound is not the engine formula"
    ref = R.reference(case.layer, mods, wc["x"], wc["residual"])
    assert float(wc["x"].abs().max()) == M and (wc["residual"] is None or float(wc["residual"].abs().max()) == 4.0 * M)
    top = float(ref.abs().max())
    print(f"[{case.id}] M = {M:g}: max|ref| = {top:.6g}, bound = {bound:.6g}, frac = {top / bound:.4f}")
    assert top <= bound * (1 + 1e-12), "the bound is not a bound"
    assert top >= 0.9 * bound
    assert top == pytest.approx(wc["attain"], rel=1e-9)
    assert _argmax(ref) == (wc["voxel"][0], wc["co"]) + tuple(wc["voxel"][1:])


@pytest.mark.parametrize("M", R.MS, ids=lambda m: f"M=2^{int(np.log2(m))}")
@pytest.mark.parametrize("case", R.TRANSPOSED_CPU_CASES, ids=lambda c: c.id)
def test_transposed_worst_case_reaches_its_parity_class(case, M):
    """One output voxel of a stride-2 transposed layer sees one parity class of taps: the reference attains >= 0.9 of the best single
    class's value (+ shift + redir terms) -- and stays under the engine's bound, which sums every class."""
    mods, wc = R.bound_inputs(case, M)
    lay, (conv, bn, rc, rbn) = case.layer, mods
    gain, smax = _engine_formula(conv, bn)
    assert gain == pytest.approx(wc["gain"], rel=1e-12) and smax == pytest.approx(wc["smax"], rel=1e-12)
    # best class, recomputed here: kernel indices of one parity per dimension
    w = conv.weight.detach().double().transpose(0, 1)
    scale, shift = R.fold(conv, bn)
    nd = w.dim() - 2
    best = 0.0
    for cls in range(2 ** nd):
        sub = w
        for d in range(nd):
            sub = sub.index_select(2 + d, torch.tensor([kk for kk in range(lay.k) if (kk - lay.pad - ((cls >> d) & 1)) % 2 == 0]))
        best = max(best, float((sub.abs().sum(dim=tuple(range(1, 2 + nd))) * scale.abs()).max()))
    share = best / gain
    ref = R.reference(lay, mods, wc["x"], None, wc["rx"])
    top = float(ref.abs().max())
    print(f"[{case.id}] M = {M:g}: best class holds {share:.3f} of sum|w|; max|ref| = {top:.6g}, bound = {wc['bound']:.6g}, frac = {top / wc['bound']:.4f}")
    assert top <= wc["bound"] * (1 + 1e-12)
    assert top == pytest.approx(wc["attain"], rel=1e-9)
    assert top >= 0.9 * (best * M), "the planted voxel does not reach what the best parity class can reach"
    assert _argmax(ref) == (wc["voxel"][0], wc["co"]) + tuple(wc["voxel"][1:])
    if lay.k == 4:
        assert 0.10 < share < 0.20
    else:
        assert 0.25 < share < 0.50


def test_decode_split_reads_hand_built_bytes():
    """Known hi / lo halves at a known scale: three chunks (48 channels), a value whose lo half is zero, a negative value, a value below
    the scale's normal range; the decoder must return (hi + lo) / scale from the [16 hi | 16 lo] chunk layout."""
    scale = 2.0 ** 7
    g = torch.Generator().manual_seed(1)
    v = (torch.rand(2, 48, 2, 3, 5, generator=g, dtype=torch.float64) - 0.5) * 200.0
    v[0, 0, 0, 0, 0] = 1.5                      # 1.5 * 128 = 192: exact in fp16, lo = 0
    v[1, 47, 1, 2, 4] = -255.99
    v[0, 17, 1, 0, 0] = 2.0 ** -20
    t, hi, lo = R.encode_split(v, scale)
    meta = torch.zeros(128)
    meta[1] = scale
    assert float(lo[0, 0, 0, 0, 0, 0]) == 0.0 and float(hi[0, 0, 0, 0, 0, 0]) == 192.0
    dec = R.decode_split(t, meta)
    assert dec.dtype == torch.float64 and tuple(dec.shape) == tuple(v.shape)
    want = ((hi.double() + lo.double()) / scale).reshape(2, 2, 3, 5, 48).permute(0, 4, 1, 2, 3)
    assert torch.equal(dec, want)
    assert float(dec[0, 0, 0, 0, 0]) == 1.5
    assert float((dec - v).abs().max()) <= 2.0 ** -21 * 256.0
    # the layout, spelled out on raw halves: chunk c of a voxel = halves [32 c, 32 c + 16) hi, [32 c + 16, 32 c + 32) lo
    raw = t.permute(0, 2, 3, 4, 1).contiguous().view(torch.float16)
    assert float(raw[1, 1, 2, 4, 32 * 2 + 15]) == float(hi[1, 1, 2, 4, 2, 15]) and float(raw[1, 1, 2, 4, 32 * 2 + 16 + 15]) == float(lo[1, 1, 2, 4, 2, 15])
    assert torch.equal(R.decode_split(t, meta, channels=(16, 32)), want[:, 16:48])


@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c.id)
def test_spike_targets_are_real(case):
    """"last D / H / W" voxels lie past the last whole tile of the stated tile size; segment voxels straddle the first boundary; every
    target has an input voxel in reach, and the reference's maximum lies within reach of the spike."""
    lay = case.layer
    flat = lay.kind == "deconv2d"
    sp = case.shape[1:]
    od = ((1,) + R.out_dims(lay, sp[1:])) if flat else R.out_dims(lay, sp)
    targets = R.spike_targets(case)
    assert {"first", "last"} <= set(targets)
    ragged = [d for d in range(3) if case.tile[d] and od[d] % case.tile[d]]
    assert len(targets) >= 2 + len(ragged)
    for d, label in enumerate(("last D", "last H", "last W")):
        if label in targets:
            whole = od[d] // case.tile[d] * case.tile[d]
            assert whole <= targets[label][1 + d] < od[d], f"{label} is not inside the last partial tile"
    if "segment upper" in targets:
        assert targets["segment upper"][1] == case.segment == targets["segment lower"][1] + 1
    mods = R.modules(lay)
    shape = (case.shape[0],) + tuple(sp[1:] if flat else sp)
    for label, ov in targets.items():
        ovs = (ov[0],) + tuple(ov[2:] if flat else ov[1:])
        iv = R.input_voxel_for(lay, ovs, shape[1:])
        assert R.within_reach(lay, iv[1:], ovs[1:], shape[1:])
    # one full reference run per case: the argmax of the output lies within reach of the spike (the residual and redir inputs are small)
    ov = targets["last"]
    ovs = (ov[0],) + tuple(ov[2:] if flat else ov[1:])
    iv = R.input_voxel_for(lay, ovs, shape[1:])
    x = R.spike(R.background((shape[0], lay.ci) + shape[1:]), iv, 1.0)
    odims = tuple(od[1:] if flat else od)
    res = R.background((shape[0], lay.co) + odims, seed=6) if case.res != "none" else None
    rx = R.background((shape[0], lay.co) + odims, seed=7) if lay.redir else None
    ref = R.reference(lay, mods, x, res, rx)
    am = _argmax(ref)
    assert am[0] == iv[0] and R.within_reach(lay, iv[1:], am[2:], shape[1:]), f"maximum at {am}, spike at {iv}"
