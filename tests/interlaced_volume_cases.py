"""Shared by tests/test_interlaced_volume_cpu.py, tests/test_gpu_interlaced_volume.py and tests/golden/make_golden_interlaced_volume.py (a
plain module, no fixtures): the cases of the interlaced cost volume, their seeded parameters and inputs, and torch restatements of both
constructs with the reference's module layouts, so that state_dict keys match:

    sb: StereoBase's InterlacedVolume (stereo/modeling/cost_volume/cost_volume.py:120-169): `conv3d` = three blocks whose `block` is
        [Conv3d (no bias), BatchNorm3d, ReLU] with depth kernels = depth strides (8, 8, 3), `volume11.block` = [Conv2d 1x1, BatchNorm2d, ReLU]
    ms: MSNet2D (stereo/modeling/models/msnet/MSNet2D.py:48-212): `conv3d` = [Conv3d (WITH bias), BatchNorm3d, ReLU] x 3 flat in one
        Sequential with depth kernels (8, 4, 2), `volume11` = [[Conv2d 1x1 (no bias), BatchNorm2d], ReLU]; MSNet2D below restates the whole
        model (feature extraction, the 2-D hourglasses, the trilinear soft-argmin head) for the end-to-end test.

Per plane i < min(D, W) both crop the left features to x >= i and the right ones to x < W - i, interweave the channels (left even, right
odd), run the three Conv3d on the one-channel volume and the 1x1 head, and write the result to V[:, :, i, :, i:]; the rest of V is zero
(the reference fails for planes i >= W; the restatement leaves them zero).

The tolerance rule (as in tests/mv2_cases_common.py and tests/mr_volume_cases.py): err(X) = max |X - float64 restatement| on the same
inputs, and every checked tensor X must satisfy err(X) <= 8 * err(float32 restatement).

A test of this construct passes vacuously when a ReLU never clips, when relu(shift) is zero (zero padding of an intermediate could then be
taken for padding of its input) or when the conv biases of `ms` vanish, so reference() asserts for the float64 run of every case: in each
of the four layers at least 5 % of the pre-activations are negative and at least 5 % positive, in each layer at least 25 % of the folded
shifts (shift + scale * bias) are positive, and the `ms` biases are non-zero.  SEEDS holds the first seed offset per case for which that
holds.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interlaced_volume.npz")
FACTOR = 8.0

CONFIGS = {"ms": (32, (8, 4, 2)), "sb": (96, (8, 8, 3))}          # feature channels, depth kernels
# case -> (config, B, H, W, D, F): the smallest shapes at which the kernel can still go wrong (the kernel's tile is 8 x 16 pixels of one
# plane of one batch item; it tiles or chunks on no further axis)
CASES = {
    "ms": ("ms", 2, 7, 19, 6, 1),            # batch stride, ragged tile
    "sb": ("sb", 2, 7, 19, 6, 8),            # the shape of the `interlaced_alone` golden
    "ms_seams": ("ms", 1, 21, 37, 5, 1),     # more than one tile along h and w: the three halos cross tile seams
    "ms_narrow": ("ms", 1, 3, 5, 8, 1),      # D > W: planes 5..7 zero, crop widths down to 1
    "ms_row": ("ms", 1, 1, 9, 3, 1),         # H = 1: every vertical neighbour is padding
    "sb_f3": ("sb", 1, 5, 11, 4, 3),         # odd F
    "ms_deep": ("ms", 1, 3, 50, 48, 1),      # the workload's plane count, last plane 3 columns wide
}
SEEDS = {"ms": 0, "sb": 0, "ms_seams": 1, "ms_narrow": 0, "ms_row": 0, "sb_f3": 0, "ms_deep": 0}
# the fixture: the reference's InterlacedVolume on the `sb` case; the reference's MSNet2D on a 32 x 208 image pair (volume_size 48 on a
# 52 pixels wide map) with the volume parameters of E2E_VOLUME_CASE: its preconv11 outputs, its dres0 input and its disp_pred
GOLDEN_KEYS = ("sb__vol", "ms__featL", "ms__featR", "ms__vol", "e2e__disp_pred")
E2E_VOLUME_CASE, E2E_SEED, E2E_IMAGE, E2E_MAXDISP = "ms_deep", 61, (32, 208), 192


# ----------------------------------------------------------------------------- the volume, restated
def volume_forward(conv3d, volume11, features, feat_l, feat_r, maxdisp):
    B, C, H, W = feat_l.shape
    vol = feat_l.new_zeros(B, features, maxdisp, H, W)
    for i in range(min(maxdisp, W)):
        x = torch.stack((feat_l[..., i:], feat_r[..., :W - i]), 2).reshape(B, 1, 2 * C, H, W - i)      # left at even, right at odd depth
        vol[:, :, i, :, i:] = volume11(conv3d(x).squeeze(2))
    return vol


class _Block(nn.Module):
    def __init__(self, *layers):
        super().__init__()
        self.block = nn.Sequential(*layers)

    def forward(self, x):
        return self.block(x)


def _c3(i, o, k, bias):
    return [nn.Conv3d(i, o, (k, 3, 3), (k, 1, 1), (0, 1, 1), bias=bias), nn.BatchNorm3d(o), nn.ReLU()]


class SBVolume(nn.Module):
    def __init__(self, num_features=8):
        super().__init__()
        self.num_features = num_features
        self.conv3d = nn.Sequential(_Block(*_c3(1, 16, 8, False)), _Block(*_c3(16, 32, 8, False)), _Block(*_c3(32, 16, 3, False)))
        self.volume11 = _Block(nn.Conv2d(16, num_features, 1, bias=False), nn.BatchNorm2d(num_features), nn.ReLU())

    def layers(self):
        return [(b.block[0], b.block[1]) for b in self.conv3d] + [(self.volume11.block[0], self.volume11.block[1])]

    def forward(self, feat_l, feat_r, maxdisp):
        return volume_forward(self.conv3d, self.volume11, self.num_features, feat_l, feat_r, maxdisp)


def _convbn(i, o, k=1, stride=1, pad=0, dilation=1, groups=1):
    return nn.Sequential(nn.Conv2d(i, o, k, stride, dilation if dilation > 1 else pad, dilation, groups, bias=False), nn.BatchNorm2d(o))


class MSVolume(nn.Module):
    """the volume part of MSNet2D: `conv3d`, `volume11`, `volume_size`"""

    def __init__(self):
        super().__init__()
        self.volume_size = 48
        self.conv3d = nn.Sequential(*_c3(1, 16, 8, True), *_c3(16, 32, 4, True), *_c3(32, 16, 2, True))
        self.volume11 = nn.Sequential(_convbn(16, 1), nn.ReLU(inplace=True))

    def layers(self):
        return [(self.conv3d[3 * j], self.conv3d[3 * j + 1]) for j in range(3)] + [(self.volume11[0][0], self.volume11[0][1])]

    def volume(self, feat_l, feat_r, maxdisp):
        return volume_forward(self.conv3d, self.volume11, 1, feat_l, feat_r, maxdisp)

    def forward(self, feat_l, feat_r, maxdisp):
        return self.volume(feat_l, feat_r, maxdisp)


# ----------------------------------------------------------------------------- the rest of MSNet2D, restated (submodule.py:29-134, 183-234)
class MV2(nn.Module):
    def __init__(self, inp, oup, stride, ratio):
        super().__init__()
        hid = int(inp * ratio)
        self.use_res_connect = stride == 1 and inp == oup
        self.conv = nn.Sequential(*_convbn(inp, hid), nn.ReLU6(inplace=True), *_convbn(hid, hid, 3, stride, 1, groups=hid), nn.ReLU6(inplace=True), *_convbn(hid, oup))

    def forward(self, x):
        return x + self.conv(x) if self.use_res_connect else self.conv(x)


def _dws(inp, oup, stride, pad, dilation, second_relu):
    tail = [nn.ReLU6(inplace=False)] if second_relu else []
    return nn.Sequential(*_convbn(inp, inp, 3, stride, pad, dilation, groups=inp), nn.ReLU6(inplace=True), *_convbn(inp, oup), *tail)


class MV1(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample, pad, dilation):
        super().__init__()
        self.downsample = downsample
        self.conv1, self.conv2 = _dws(inplanes, planes, stride, pad, dilation, True), _dws(planes, planes, 1, pad, dilation, False)

    def forward(self, x):
        return self.conv2(self.conv1(x)) + (x if self.downsample is None else self.downsample(x))


class Features(nn.Module):
    def __init__(self):
        super().__init__()
        self.firstconv = nn.Sequential(MV2(3, 32, 2, 3), nn.ReLU(inplace=True), MV2(32, 32, 1, 3), nn.ReLU(inplace=True), MV2(32, 32, 1, 3), nn.ReLU(inplace=True))
        self.inplanes = 32
        self.layer1, self.layer2 = self._layer(32, 3, 1, 1), self._layer(64, 16, 2, 1)
        self.layer3, self.layer4 = self._layer(128, 3, 1, 1), self._layer(128, 3, 1, 2)

    def _layer(self, planes, blocks, stride, dilation):
        down = _convbn(self.inplanes, planes, 1, stride) if stride != 1 or self.inplanes != planes else None
        layers = [MV1(self.inplanes, planes, stride, down, 1, dilation)] + [MV1(planes, planes, 1, None, 1, dilation) for _ in range(1, blocks)]
        self.inplanes = planes
        return nn.Sequential(*layers)

    def forward(self, x):
        l2 = self.layer2(self.layer1(self.firstconv(x)))
        l3 = self.layer3(l2)
        return torch.cat((l2, l3, self.layer4(l3)), 1)


class Hourglass2D(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv1, self.conv2, self.conv3, self.conv4 = MV2(c, c * 2, 2, 2), MV2(c * 2, c * 2, 1, 2), MV2(c * 2, c * 4, 2, 2), MV2(c * 4, c * 4, 1, 2)
        self.conv5 = nn.Sequential(nn.ConvTranspose2d(c * 4, c * 2, 3, padding=1, output_padding=1, stride=2, bias=False), nn.BatchNorm2d(c * 2))
        self.conv6 = nn.Sequential(nn.ConvTranspose2d(c * 2, c, 3, padding=1, output_padding=1, stride=2, bias=False), nn.BatchNorm2d(c))
        self.redir1, self.redir2 = MV2(c, c, 1, 2), MV2(c * 2, c * 2, 1, 2)

    def forward(self, x):
        conv2 = self.conv2(self.conv1(x))
        conv5 = F.relu(self.conv5(self.conv4(self.conv3(conv2))) + self.redir2(conv2), inplace=True)
        return F.relu(self.conv6(conv5) + self.redir1(x), inplace=True)


class MSNet2D(MSVolume):
    """MSNet2D.py:48-212 with the reference's attribute layout; `forward` is its eval branch (the training branch adds three more heads)"""

    def __init__(self, maxdisp=E2E_MAXDISP):
        super().__init__()
        self.maxdisp, c = maxdisp, 48
        self.feature_extraction = Features()
        self.preconv11 = nn.Sequential(_convbn(320, 256), nn.ReLU(inplace=True), _convbn(256, 128), nn.ReLU(inplace=True), _convbn(128, 64), nn.ReLU(inplace=True),
                                       nn.Conv2d(64, 32, 1, 1, 0, 1))
        self.dres0 = nn.Sequential(MV2(c, c, 1, 3), nn.ReLU(inplace=True), MV2(c, c, 1, 3), nn.ReLU(inplace=True))
        self.dres1 = nn.Sequential(MV2(c, c, 1, 3), nn.ReLU(inplace=True), MV2(c, c, 1, 3))
        self.encoder_decoder1, self.encoder_decoder2, self.encoder_decoder3 = Hourglass2D(c), Hourglass2D(c), Hourglass2D(c)
        for n in range(4):
            setattr(self, f"classif{n}", nn.Sequential(_convbn(c, c, 3, 1, 1), nn.ReLU(inplace=True), nn.Conv2d(c, c, 3, 1, 1, bias=False)))

    def forward(self, data):
        L, R = data["left"], data["right"]
        fl, fr = self.preconv11(self.feature_extraction(L)), self.preconv11(self.feature_extraction(R))
        cost0 = self.dres0(self.volume(fl, fr, self.volume_size)[:, 0])
        cost0 = self.dres1(cost0) + cost0
        cost3 = self.classif3(self.encoder_decoder3(self.encoder_decoder2(self.encoder_decoder1(cost0))))
        cost3 = F.interpolate(cost3.unsqueeze(1), [self.maxdisp, L.shape[2], L.shape[3]], mode="trilinear").squeeze(1)
        disp = torch.arange(self.maxdisp, dtype=cost3.dtype, device=cost3.device).view(1, -1, 1, 1)
        return {"disp_pred": (F.softmax(cost3, 1) * disp).sum(1)}


# ----------------------------------------------------------------------------- seeded parameters and inputs
def seed_volume_parameters(layers, g):
    """conv weights ~ N(0,1) * 1.5 * sqrt(2 / fan_in), conv bias ~ 0.5 N(0,1), BN weight ~ U(0.5, 2), bias ~ N(0,1), running mean ~ 0.5 N(0,1),
    running var ~ U(0.5, 2): layer by layer from the generator g"""
    with torch.no_grad():
        for conv, bn in layers:
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 1.5 * (2.0 / conv.weight[0].numel()) ** 0.5)
            if conv.bias is not None:
                conv.bias.copy_(0.5 * torch.randn(conv.bias.shape, generator=g))
            bn.weight.copy_(torch.rand(bn.weight.shape, generator=g) * 1.5 + 0.5)
            bn.bias.copy_(torch.randn(bn.bias.shape, generator=g))
            bn.running_mean.copy_(0.5 * torch.randn(bn.bias.shape, generator=g))
            bn.running_var.copy_(torch.rand(bn.bias.shape, generator=g) * 1.5 + 0.5)


def make_volume(case, dtype=torch.float32):
    """the case's module (SBVolume or MSVolume) with its seeded parameters, in eval mode on the CPU"""
    cfg, B, H, W, D, Fo = CASES[case]
    m = SBVolume(Fo) if cfg == "sb" else MSVolume()
    seed_volume_parameters(m.layers(), torch.Generator().manual_seed(7000 + 100 * list(CASES).index(case) + SEEDS[case]))
    return m.to(dtype).eval()


def make_inputs(case, dtype=torch.float32):
    """seeded featL, featR ~ N(0,1), contiguous NCHW on the CPU"""
    cfg, B, H, W, D, Fo = CASES[case]
    g = torch.Generator().manual_seed(8000 + list(CASES).index(case))
    C = CONFIGS[cfg][0]
    return torch.randn(B, C, H, W, generator=g).to(dtype), torch.randn(B, C, H, W, generator=g).to(dtype)


def make_msnet2d(dtype=torch.float32):
    """the whole-model restatement: synthetic parameters by name (openstereo_amd.utils.weights), the volume's from E2E_VOLUME_CASE"""
    from openstereo_amd.utils.weights import synth_state_dict
    m = MSNet2D()
    m.load_state_dict(synth_state_dict(m, seed=E2E_SEED))
    vol = make_volume(E2E_VOLUME_CASE)
    m.conv3d.load_state_dict(vol.conv3d.state_dict())
    m.volume11.load_state_dict(vol.volume11.state_dict())
    return m.to(dtype).eval()


def e2e_images():
    from openstereo_amd.utils.weights import synth_images
    return synth_images(1, *E2E_IMAGE, seed=E2E_SEED, max_shift=24.0)


def out_shape(case):
    cfg, B, H, W, D, Fo = CASES[case]
    return (B, Fo, D, H, W)


def folded_shifts(m):
    """per layer: shift + scale * bias of the eval-mode BatchNorm behind the convolution"""
    out = []
    for conv, bn in m.layers():
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        shift = bn.bias - bn.running_mean * scale
        out.append((scale, shift if conv.bias is None else shift + scale * conv.bias))
    return out


def preactivations(m, feat_l, feat_r, maxdisp):
    """-> (volume, the four layers' BatchNorm outputs over all planes, flattened)"""
    pre = [[] for _ in range(4)]
    hooks = [bn.register_forward_hook(lambda mod, a, out, j=j: pre[j].append(out.detach().flatten().clone())) for j, (_, bn) in enumerate(m.layers())]
    with torch.no_grad():
        y = m(feat_l, feat_r, maxdisp)
    for h in hooks:
        h.remove()
    return y, [torch.cat(p) for p in pre]


def not_vacuous(case, m, feat_l, feat_r, maxdisp):
    """-> (volume, None) or (volume, reason why a test on this run would be vacuous)"""
    y, pre = preactivations(m, feat_l, feat_r, maxdisp)
    why = None
    for j, (v, (_, t)) in enumerate(zip(pre, folded_shifts(m))):
        lo, hi = float((v < 0).double().mean()), float((v > 0).double().mean())
        if lo < 0.05 or hi < 0.05:
            why = why or f"{case}: layer {j + 1} has {lo:.1%} negative and {hi:.1%} positive pre-activations"
        if float((t > 0).double().mean()) < 0.25:
            why = why or f"{case}: layer {j + 1} has too few positive folded shifts"
    if CASES[case][0] == "ms" and not all(conv.bias is not None and bool((conv.bias != 0).all()) for conv, _ in m.layers()[:3]):
        why = why or f"{case}: a conv bias is zero"
    return y, why


_cache = {}


def reference(case, dtype, feats=None):
    """-> the restatement's volume in `dtype` on the case's inputs (or on feats = (featL, featR)); the case's own run is computed once and
    not modified by the tests"""
    D = CASES[case][4]
    if feats is not None:
        with torch.no_grad():
            return make_volume(case, dtype)(feats[0].to(dtype), feats[1].to(dtype), D)
    key = (case, dtype)
    if key not in _cache:
        m, (fl, fr) = make_volume(case, dtype), make_inputs(case, dtype)
        if dtype == torch.float64:
            _cache[key], why = not_vacuous(case, m, fl, fr, D)
            assert why is None, why
        else:
            with torch.no_grad():
                _cache[key] = m(fl, fr, D)
    return _cache[key]


def err(x, ref64):
    return float((x.detach().double().cpu() - ref64).abs().max())


def check(what, x, ref64, ref32):
    """the tolerance rule; both numbers in the message"""
    assert tuple(x.shape) == tuple(ref64.shape), f"{what}: shape {tuple(x.shape)}, expected {tuple(ref64.shape)}"
    e, e32 = err(x, ref64), err(ref32, ref64)
    print(f"{what}: err {e:.3e}, fp32 restatement {e32:.3e}")
    assert e <= FACTOR * e32, f"{what}: err {e:.3e} > {FACTOR:g} x {e32:.3e} (the fp32 restatement's error)"
