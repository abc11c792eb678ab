"""End-to-end model classes for BASELINE configs [2]-[4]: StereoBase, IGEVStereo, LightStereo.

What is the engine's and what is not.  The hot path of SURVEY 8a -- cost volume, 3-D / 2-D aggregation, classifier,
soft-argmin, geometry-encoding lookup, ConvGRU update block, convex (context) upsampling -- runs on the gfx950 engine
through the stage modules of igev_style.py / lightstereo.py / igev_update.py, under the reference's attribute names
(`cost_agg`, `classifier`, `corr_stem`, `corr_feature_att`, `update_block`), so those checkpoint keys load.

The 2-D feature side is out of the path (SURVEY 8 "out of scope": timm MobileNetV2 / EfficientNet pyramids with
pretrained weights, MultiBasicEncoder).  The small 2-D heads around it (stem_2, stem_4, conv, desc, concat_conv, spx*,
context_zqr_convs, refine_*) are ordinary PyTorch-ROCm modules with the reference's names and shapes; the two large
pieces are *injectable*: `feature` / `backbone` (timm: pass the reference's own module, or leave the shape-compatible stand-in
StubFeature, a strided conv pyramid with the documented channel counts and strides) and `cnet` (default since r3: the engine mirror of the
reference's MultiBasicEncoder, models/context_encoder.py; StubContext is a light stand-in).  With the stand-ins the classes run offline end to end, which is what the tests and `bench.py` use; the
numbers they produce are hot-path numbers, never accuracy claims.

To accelerate the reference's *own* model objects (timm present), use `openstereo_amd.attach.patch_reference_modules()`
instead: it grafts the same engine forwards onto the reference's classes.

Reference: stereo/modeling/models/stereobase/stereobase_gru.py:14-213, models/igev/igev_stereo.py:78-218,
models/lightstereo/lightstereo.py:13-71.
"""
from __future__ import annotations

from functools import partial
from types import SimpleNamespace

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..ops import on_engine
from .igev_style import conv_block, BasicConv2d, BasicConv, IGEVFeatureAtt, StereoBaseCostStage, hourglass, _pack_igev
from .igev_update import BasicMultiUpdateBlock, run_refinement
from .context_encoder import MultiBasicEncoder
from .interlaced import InterlacedVolume
from .lightstereo import LightStereoCostStage
from ..engine import cached_pack, SmallCoConv3d


# ----------------------------------------------------------------------------- 2-D helper blocks (torch modules)
class BasicDeconv2d(nn.Module):
    """common/basic_block_2d.py:24-39"""

    def __init__(self, cin, cout, kernel_size, stride=1, padding=0, bias=False, norm_layer=None, act_layer=None, **kw):
        super().__init__()
        self.block = conv_block(nn.ConvTranspose2d(cin, cout, kernel_size=kernel_size, stride=stride, padding=padding, bias=bias, **kw), cout, norm_layer, act_layer)

    def forward(self, x):
        return self.block(x)


class Conv2xUp(nn.Module):
    """stereobase/igev_blocks.py:10-32: deconv x2 -> concat with the skip -> 3x3 conv."""

    def __init__(self, cin, cout, norm_layer, concat=True):
        super().__init__()
        self.concat = concat
        self.conv1 = BasicDeconv2d(cin, cout, norm_layer=norm_layer, act_layer=nn.LeakyReLU, kernel_size=4, stride=2, padding=1)
        self.conv2 = BasicConv2d(cout * 2, cout * 2, norm_layer=norm_layer, act_layer=nn.LeakyReLU, kernel_size=3, stride=1, padding=1)

    def forward(self, x, rem):
        x = self.conv1(x)
        if x.shape != rem.shape:
            x = F.interpolate(x, size=rem.shape[-2:], mode="nearest")
        return self.conv2(torch.cat((x, rem), 1) if self.concat else x + rem)


class FPNLayer(nn.Module):
    """lightstereo/backbone.py:11-26"""

    def __init__(self, chan_low, chan_high):
        super().__init__()
        act = partial(nn.LeakyReLU, negative_slope=0.2, inplace=True)
        self.deconv = BasicDeconv2d(chan_low, chan_high, kernel_size=4, stride=2, padding=1, norm_layer=nn.BatchNorm2d, act_layer=act)
        self.conv = BasicConv2d(chan_high * 2, chan_high, kernel_size=3, padding=1, norm_layer=nn.BatchNorm2d, act_layer=act)

    def forward(self, low, high):
        return self.conv(torch.cat([high, self.deconv(low)], 1))


class BasicConvIN(nn.Module):
    """models/igev/submodule.py:83-110 (`.conv` / `.IN` unit names; InstanceNorm2d without affine parameters, LeakyReLU(0.01))."""

    def __init__(self, cin, cout, deconv=False, IN=True, relu=True, **kw):
        super().__init__()
        self.relu, self.use_in = relu, IN
        self.conv = (nn.ConvTranspose2d if deconv else nn.Conv2d)(cin, cout, bias=False, **kw)
        self.IN = nn.InstanceNorm2d(cout)

    def forward(self, x):
        x = self.conv(x)
        if self.use_in:
            x = self.IN(x)
        return F.leaky_relu(x, 0.01) if self.relu else x


class Conv2xIGEV(nn.Module):
    """models/igev/submodule.py:35-78 (`Conv2x`, norm="bn") and :113-157 (`Conv2x_IN`, norm="in") in the one configuration IGEV-Stereo
    uses for its upsampling heads (igev_stereo.py:104,112): deconv k4 s2 p1 -> concat with the skip -> 3x3 conv keeping 2 x cout channels.
    Unit names `.conv1.conv` / `.conv1.bn|IN` / `.conv2.conv` / `.conv2.bn|IN` as in the reference's checkpoints."""

    def __init__(self, cin, cout, norm="bn"):
        super().__init__()
        unit = BasicConv if norm == "bn" else BasicConvIN
        self.concat = True
        self.conv1 = unit(cin, cout, deconv=True, kernel_size=4, stride=2, padding=1)
        self.conv2 = unit(cout * 2, cout * 2, kernel_size=3, stride=1, padding=1)

    def forward(self, x, rem):
        x = self.conv1(x)
        if x.shape != rem.shape:
            x = F.interpolate(x, size=rem.shape[-2:], mode="nearest")
        return self.conv2(torch.cat((x, rem), 1))


def _pyramid_step(cin, cout, stride):
    return nn.Sequential(nn.Conv2d(cin, cout, 3, stride, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))


class StubFeature(nn.Module):
    """Shape-compatible stand-in for the timm feature pyramid (stereobase/igev `Feature`, lightstereo `Backbone`):
    image [B,3,H,W] -> [1/4, 1/8, 1/16, 1/32] maps with `channels`.  NOT the reference's backbone (8 "out of scope")."""

    def __init__(self, channels=(48, 64, 192, 160)):
        super().__init__()
        self.output_channels = list(channels)
        self.stem = nn.Sequential(_pyramid_step(3, 16, 2), _pyramid_step(16, channels[0], 2))
        self.down = nn.ModuleList([_pyramid_step(channels[i], channels[i + 1], 2) for i in range(3)])

    def forward(self, x):
        out = [self.stem(x)]
        for d in self.down:
            out.append(d(out[-1]))
        return out


def _pick_feature(feature, which):
    """The 2-D feature pyramid of an end-to-end class: a module (the reference's own, or any shape-compatible one), None = the light
    5-conv stand-in the round-2/3 fixtures were generated with (`StubFeature`), or "mobilenetv2" = the reference's pyramid --
    feature_pyramid.Feature / IGEVFeature / LightStereoBackbone: MobileNetV2-100 trunk mirror (unpinned: timm absent) + the reference's FPN
    decoder (pinned), full `feature.*` / `backbone.*` checkpoint keys."""
    if isinstance(feature, str):
        if feature != "mobilenetv2":
            raise ValueError(f"unknown feature pyramid '{feature}' (only 'mobilenetv2')")
        from . import feature_pyramid as FP
        return {"stereobase": FP.Feature, "igev": FP.IGEVFeature, "lightstereo": FP.LightStereoBackbone}[which]()
    if feature is not None:
        return feature
    return StubFeature((24, 32, 96, 160) if which == "lightstereo" else (48, 64, 192, 160))


class StubContext(nn.Module):
    """Shape-compatible stand-in for MultiBasicEncoder (stereobase/gru_blocks.py, igev/extractor.py): image ->
    [(net, inp)] at 1/4, 1/8, 1/16 with hidden_dims / context_dims channels.  `forward(x, num_layers)` like the reference."""

    def __init__(self, hidden_dims=(128, 128, 128), context_dims=(128, 128, 128)):
        super().__init__()
        self.stem = nn.Sequential(_pyramid_step(3, 32, 2), _pyramid_step(32, 64, 2))
        self.down = nn.ModuleList([_pyramid_step(64, 64, 2), _pyramid_step(64, 64, 2)])
        # the reference orders hidden_dims coarse -> fine ([2] is the 1/4 level)
        self.heads = nn.ModuleList([nn.ModuleList([nn.Conv2d(64, hidden_dims[2 - i], 3, padding=1), nn.Conv2d(64, context_dims[2 - i], 3, padding=1)])
                                    for i in range(3)])

    def forward(self, x, num_layers=3):
        f = self.stem(x)
        out = []
        for i in range(num_layers):
            if i:
                f = self.down[i - 1](f)
            out.append((self.heads[i][0](f), self.heads[i][1](f)))
        return out


def _context_lists(cnet, zqr_convs, image, n_layers):
    """igev_stereo.py:175-179 / stereobase_gru.py:167-171"""
    cnet_list = cnet(image, num_layers=n_layers)
    net_list = [torch.tanh(x[0]) for x in cnet_list]
    inp_list = [torch.relu(x[1]) for x in cnet_list]
    inp_list = [list(conv(i).split(split_size=conv.out_channels // 3, dim=1)) for i, conv in zip(inp_list, zqr_convs)]
    return net_list, inp_list


FUSED_UPSAMPLE_TRAIN = os.environ.get("OSA_FUSED_UPSAMPLE_TRAIN", "1") != "0"


def _gru_train_loop(model, a, s, init_disp, geo, iters, n_layers, slow_fast):
    """The GRU loop of stereobase_gru.py:177-203 / igev_stereo.py:181-208 in training mode: lookup (forward + backward on the engine),
    update block (engine convs through autograd), convex upsampling of every iteration's disparity (the loss needs them all)."""
    from ..attach import context_upsample as ctx_up              # differentiable form (torch composition when gradients flow)
    from ..geometry import CombinedGeoEncodingVolume
    from .. import autograd as AG
    geo_fn = CombinedGeoEncodingVolume(s["match_left"].float(), s["match_right"].float(), geo.float(), radius=a.CORR_RADIUS, num_levels=a.CORR_LEVELS)
    b, _, h, w = s["match_left"].shape
    coords = torch.arange(w, device=init_disp.device).float().reshape(1, 1, w, 1).repeat(b, h, 1, 1)
    net_list, inp_list = s["net_list"], s["inp_list"]
    n3, n2 = n_layers == 3, n_layers >= 2
    disp, disp_preds = init_disp, []
    for _ in range(iters):
        disp = disp.detach()
        geo_feat = geo_fn(disp, coords)
        if n3 and slow_fast:
            net_list = model.update_block(net_list, inp_list, iter16=True, iter08=False, iter04=False, update=False)
        if n2 and slow_fast:
            net_list = model.update_block(net_list, inp_list, iter16=n3, iter08=True, iter04=False, update=False)
        net_list, mask_feat_4, delta_disp = model.update_block(net_list, inp_list, geo_feat, disp, iter16=n3, iter08=n2)
        disp = disp + delta_disp.float()     # (same values as the promoting add; fp32 + fp16 takes torch's templated mixed-dtype kernel: 88 us for 14720 elements)
        with AG.engine_convs():              # the k = 4 ConvTranspose2d heads: engine deconv / strided conv / class-mode wgrad
            logits = model.spx_gru(model.spx_2_gru(mask_feat_4, s["stem_2x"]))
        if FUSED_UPSAMPLE_TRAIN and logits.is_cuda and logits.shape[1] == 9:
            disp_preds.append(AG.context_upsample_logits(disp, logits, 4, 4.0).unsqueeze(1))      # softmax + x4 gain + convex combination, one kernel each way (r6)
        else:
            disp_preds.append(ctx_up(disp * 4.0, F.softmax(logits, 1)).unsqueeze(1))
    return disp_preds


def _masked_mean(x, valid):
    """mean of x over `valid` with static shapes: sum(x * valid) / count -- the value of `x[valid].mean()` (up to summation order) without
    the boolean-mask gather, whose output size is a host synchronisation (it cannot be captured in a hipGraph)."""
    v = valid.to(x.dtype)
    return (x * v).sum() / v.sum()


def _sequence_loss(model_pred, disp_gt, max_disp, static=False):
    """stereobase_gru.py:215-243 == igev_stereo.py:209-240: smooth-L1 on the initial disparity + gamma-weighted L1 over the GRU predictions.
    static=True: the same loss written with static shapes and no `.item()` (see _masked_mean) so that a whole training step can be replayed
    as a hipGraph; the info dict then holds the loss tensor."""
    valid = ((disp_gt < max_disp) & (disp_gt > 0)).unsqueeze(1)
    disp_gt = disp_gt.unsqueeze(1)
    mean = (lambda x: _masked_mean(x, valid)) if static else (lambda x: x[valid].mean())
    loss = mean(F.smooth_l1_loss(model_pred["init_disp"], disp_gt, reduction="none")) if static else \
        F.smooth_l1_loss(model_pred["init_disp"][valid], disp_gt[valid], reduction="mean")
    preds = model_pred["disp_preds"]
    n = len(preds)
    for i, pr in enumerate(preds):
        gamma = 0.9 ** (15 / (n - 1)) if n > 1 else 1.0
        loss = loss + gamma ** (n - i - 1) * mean((pr - disp_gt).abs())
    return loss, {"scalar/train/loss_disp": loss.detach() if static else float(loss.detach())}


def _require_engine(x, who):
    if not on_engine(x):
        raise RuntimeError(f"openstereo_amd {who} runs on the GPU engine only (no CPU path)")


# ----------------------------------------------------------------------------- StereoBase (BASELINE configs[2])
class StereoBase(StereoBaseCostStage):
    """stereobase_gru.py:14-213.  Every volume switch of the reference is honoured: USE_GWC_VOLUME / USE_CONCAT_VOLUME (the fused NDHWC
    builder), and the two dormant variants no shipped config enables -- USE_SUB_VOLUME (ops.build_sub_volume, 1 channel) and
    USE_INTERLACED_VOLUME (models/interlaced.py, INTERLACED_CHANNELS) -- appended behind the fused channels in the reference's order.

    `cfgs`: attribute namespace with the reference's keys (MAX_DISP, NUM_GROUPS, USE_CONCAT_VOLUME, CONCAT_CHANNELS,
    HIDDEN_DIMS, N_GRU_LAYERS, CORR_RADIUS, CORR_LEVELS, SLOW_FAST_GRU, EVAL_ITERS, TRAIN_ITERS)."""

    def __init__(self, cfgs, feature=None, cnet=None):
        g = lambda k, d: getattr(cfgs, k, d)
        self_concat = g("CONCAT_CHANNELS", 12) if g("USE_CONCAT_VOLUME", False) else 0
        groups = g("NUM_GROUPS", 8) if g("USE_GWC_VOLUME", True) else 0
        use_sub, use_inter = bool(g("USE_SUB_VOLUME", False)), bool(g("USE_INTERLACED_VOLUME", False))
        inter_ch = g("INTERLACED_CHANNELS", 8) if use_inter else 0
        if groups + self_concat + use_sub + inter_ch == 0:
            raise ValueError("StereoBase: every volume switch is off (USE_GWC_VOLUME / USE_CONCAT_VOLUME / USE_SUB_VOLUME / USE_INTERLACED_VOLUME)")
        feature = _pick_feature(feature, "stereobase")
        bc = list(getattr(feature, "output_channels", (48, 64, 192, 160)))
        bc[0] += 48
        super().__init__(max_disp=cfgs.MAX_DISP, num_groups=groups, concat_channels=self_concat, backbone_channels=bc,
                         extra_channels=int(use_sub) + inter_ch)
        self.use_sub_volume, self.use_interlaced_volume = use_sub, use_inter
        if use_inter:
            self.build_interlaced_volume = InterlacedVolume(inter_ch)
        self.cfgs = cfgs
        self.n_gru_layers, self.slow_fast_gru = cfgs.N_GRU_LAYERS, cfgs.SLOW_FAST_GRU
        hd = list(cfgs.HIDDEN_DIMS)
        volume_channel = self.num_groups + 2 * self_concat + self.extra_channels
        IN, BN, LR = nn.InstanceNorm2d, nn.BatchNorm2d, nn.LeakyReLU
        self.feature = feature
        # r3: the reference's context network itself (plain PyTorch there, engine mirror here, `cnet.*` checkpoint keys); StubContext stays
        # available as a light stand-in (pass cnet=StubContext(hd, hd))
        self.cnet = cnet if cnet is not None else MultiBasicEncoder(output_dim=[hd, hd], norm_fn="batch", downsample=g("N_DOWNSAMPLE", 2))
        args = SimpleNamespace(N_GRU_LAYERS=cfgs.N_GRU_LAYERS, CORR_LEVELS=cfgs.CORR_LEVELS, CORR_RADIUS=cfgs.CORR_RADIUS,
                               SLOW_FAST_GRU=cfgs.SLOW_FAST_GRU)
        self._loop_args = args
        cor_planes = cfgs.CORR_LEVELS * (2 * cfgs.CORR_RADIUS + 1) * (volume_channel + 1)          # gru_blocks.py:236
        self.update_block = BasicMultiUpdateBlock(args, hidden_dims=hd, cor_planes=cor_planes)
        self.context_zqr_convs = nn.ModuleList([nn.Conv2d(hd[i], hd[i] * 3, 3, padding=1) for i in range(self.n_gru_layers)])
        self.spx_2_gru = Conv2xUp(32, 32, norm_layer=BN)
        self.spx_gru = nn.Sequential(nn.ConvTranspose2d(2 * 32, 9, kernel_size=4, stride=2, padding=1))
        self.stem_2 = nn.Sequential(BasicConv2d(3, 32, norm_layer=IN, act_layer=LR, kernel_size=3, stride=2, padding=1),
                                    BasicConv2d(32, 32, norm_layer=IN, act_layer=nn.ReLU, kernel_size=3, stride=1, padding=1))
        self.stem_4 = nn.Sequential(BasicConv2d(32, 48, norm_layer=IN, act_layer=LR, kernel_size=3, stride=2, padding=1),
                                    BasicConv2d(48, 48, norm_layer=IN, act_layer=nn.ReLU, kernel_size=3, stride=1, padding=1))
        self.spx = nn.Sequential(nn.ConvTranspose2d(2 * 32, 9, kernel_size=4, stride=2, padding=1))
        self.spx_2 = Conv2xUp(24, 32, norm_layer=IN, concat=True)
        self.spx_4 = nn.Sequential(BasicConv2d(bc[0], 24, norm_layer=IN, act_layer=LR, kernel_size=3, stride=1, padding=1),
                                   BasicConv2d(24, 24, norm_layer=IN, act_layer=nn.ReLU, kernel_size=3, stride=1, padding=1))
        self.conv = BasicConv2d(bc[0], bc[0], norm_layer=IN, act_layer=LR, kernel_size=3, stride=1, padding=1)
        self.desc = nn.Conv2d(bc[0], bc[0], kernel_size=1, padding=0, stride=1)
        if self_concat:
            self.concat_conv = nn.Sequential(BasicConv2d(bc[0], 32, norm_layer=BN, act_layer=nn.ReLU, kernel_size=3, stride=1, padding=1),
                                             nn.Conv2d(32, self_concat, kernel_size=1, padding=0, stride=1, bias=False))

    # -- 2-D side (torch modules): everything the hot path consumes ---------------------------------------------------
    def side(self, image1, image2):
        fl, fr = self.feature(image1), self.feature(image2)
        stem_2x = self.stem_2(image1)
        fl[0] = torch.cat((fl[0], self.stem_4(stem_2x)), 1)
        fr[0] = torch.cat((fr[0], self.stem_4(self.stem_2(image2))), 1)
        ml, mr = self.desc(self.conv(fl[0])), self.desc(self.conv(fr[0]))
        cl = cr = None
        if self.concat_channels:
            cl, cr = self.concat_conv(ml), self.concat_conv(mr)
        net_list, inp_list = _context_lists(self.cnet, self.context_zqr_convs, image1, self.n_gru_layers)
        spx_logits = self.spx(self.spx_2(self.spx_4(fl[0]), stem_2x))
        return dict(features_left=fl, match_left=ml, match_right=mr, concat_left=cl, concat_right=cr, stem_2x=stem_2x,
                    net_list=net_list, inp_list=inp_list, spx_logits=spx_logits)

    def _extra_volumes(self, ml, mr):
        """stereobase_gru.py:152-159: the dormant volume variants, NCDHW, in the reference's concatenation order."""
        D4, out = self.max_disp // 4, []
        if self.use_sub_volume:
            if ml.requires_grad or mr.requires_grad:             # differentiable torch form of cost_volume.py:108-117 (the engine op has no backward)
                W = ml.shape[3]
                sub = torch.stack([torch.cat((ml[..., :i].abs().sum(1), (ml[..., i:] - mr[..., :W - i]).abs().sum(1)), -1) for i in range(D4)], 1)
            else:
                sub = ops.build_sub_volume(ml, mr, D4)
            out.append(sub.unsqueeze(1))
        if self.use_interlaced_volume:
            out.append(self.build_interlaced_volume(ml, mr, D4))
        return out

    def upsample_disp(self, disp, mask_feat_4, stem_2x):
        """stereobase_gru.py:114-119 with softmax, x4 gain and the 3x3 convex combination in one kernel."""
        logits = self.spx_gru(self.spx_2_gru(mask_feat_4, stem_2x))
        return ops.context_upsample(disp, logits, 4, softmax_weights=True, gain=4.0).unsqueeze(1)

    def forward(self, data):
        image1, image2 = data["left"], data["right"]
        _require_engine(image1, "StereoBase")
        if self.training:
            return self._train(image1, image2)
        with torch.no_grad():
            return self._infer(image1, image2)

    def _train(self, image1, image2):
        """stereobase_gru.py:121-213, training mode: every hot-path op forward AND backward on the engine -- volumes, hourglass convs,
        classifier, fused softmax regression (StereoBaseCostStage.forward_train), geometry-encoding lookup (geometry._Lookup), update
        block convs (BasicMultiUpdateBlock.forward_train); BatchNorm / activations / the small 2-D heads are torch modules."""
        from ..attach import context_upsample as ctx_up
        s = self.side(image1, image2)
        st = StereoBaseCostStage.forward(self, s["match_left"], s["match_right"], s["concat_left"], s["concat_right"], s["features_left"],
                                         self._extra_volumes(s["match_left"], s["match_right"]))
        disp_preds = _gru_train_loop(self, self.cfgs, s, st["init_disp"], st["geo_encoding_volume"], self.cfgs.TRAIN_ITERS,
                                     self.n_gru_layers, self.slow_fast_gru)
        init_up = ctx_up(st["init_disp"] * 4.0, F.softmax(s["spx_logits"], 1).float()).unsqueeze(1)
        return {"init_disp": init_up, "disp_preds": disp_preds, "disp_pred": disp_preds[-1]}

    def get_loss(self, model_pred, input_data, static=False):
        return _sequence_loss(model_pred, input_data["disp"], self.max_disp, static)

    def _infer(self, image1, image2):
        s = self.side(image1, image2)
        st = StereoBaseCostStage.forward(self, s["match_left"], s["match_right"], s["concat_left"], s["concat_right"], s["features_left"],
                                         self._extra_volumes(s["match_left"], s["match_right"]))
        r = run_refinement(self.update_block, self._loop_args, s["match_left"], s["match_right"], st["geo_encoding_volume"],
                           s["net_list"], s["inp_list"], st["init_disp"], self.cfgs.EVAL_ITERS)
        disp_up = self.upsample_disp(r["disp"], r["mask_feat_4"], s["stem_2x"])
        init_up = ops.context_upsample(st["init_disp"], s["spx_logits"].float(), 4, softmax_weights=True, gain=4.0).unsqueeze(1)
        # the reference also upsamples after every iteration (disp_preds, used by the training loss only)
        return {"init_disp": init_up, "disp_preds": [disp_up], "disp_pred": disp_up}


# ----------------------------------------------------------------------------- IGEV-Stereo (BASELINE configs[4])
class IGEVCostStage(nn.Module):
    """igev_stereo.py:158-168: gwc(8) volume -> corr_stem (Conv3d+BN+LeakyReLU) with the corr_feature_att gate fused into its
    epilogue -> hourglass -> classifier -> softmax -> regression, reference attribute names."""

    def __init__(self, max_disp=192):
        super().__init__()
        self.max_disp = max_disp
        self.corr_stem = BasicConv(8, 8, is_3d=True, kernel_size=3, stride=1, padding=1)
        self.corr_feature_att = IGEVFeatureAtt(8, 96)
        self.cost_agg = hourglass(8)
        self.classifier = nn.Conv3d(8, 1, 3, 1, 1, bias=False)
        self._stem = self._cls = None

    def reset_engine(self):
        self._stem = self._cls = None
        self.cost_agg.reset_engine()

    def cost_stage(self, match_left, match_right, features_left):
        D4 = self.max_disp // 4
        vol = ops.build_cost_volume_cl(match_left, match_right, 8, None, None, maxdisp=D4)
        stem = cached_pack(self, "_stem", lambda: _pack_igev(self.corr_stem), mods=(self.corr_stem,))
        vol = stem(vol, gate=self.corr_feature_att.logits(features_left[0]))
        geo = self.cost_agg.forward_cl(vol, features_left)
        cost = cached_pack(self, "_cls", lambda: SmallCoConv3d(self.classifier), mods=(self.classifier,))(geo)
        init_disp, prob = ops.softmax_disparity_regression(cost[:, 0], D4, keepdim=True, return_prob=True)
        return {"init_disp": init_disp, "prob": prob, "geo_encoding_volume": geo}

    def cost_stage_train(self, match_left, match_right, features_left):
        """igev_stereo.py:158-168 with differentiable engine ops (volume, convolutions, fused softmax regression)."""
        from .. import autograd as A
        D4 = self.max_disp // 4
        vol = A.build_gwc_volume(match_left, match_right, D4, 8)
        vol = self.cost_agg._unit_train(self.corr_stem, vol)
        vol = torch.sigmoid(self.corr_feature_att.feat_att(features_left[0]).unsqueeze(2)) * vol
        geo = self.cost_agg.forward_train(vol, features_left)
        cost = A.conv_module(self.classifier, geo).squeeze(1)
        init_disp = A.softmax_disparity_regression(cost, keepdim=True)
        return {"init_disp": init_disp, "prob": torch.softmax(cost, dim=1), "geo_encoding_volume": geo}

    def forward(self, match_left, match_right, features_left):
        _require_engine(match_left, "IGEVCostStage")
        if self.training or (torch.is_grad_enabled() and (match_left.requires_grad or any(p.requires_grad for p in self.parameters()))):
            return self.cost_stage_train(match_left, match_right, features_left)
        return self.cost_stage(match_left, match_right, features_left)


class IGEVStereo(IGEVCostStage):
    """igev_stereo.py:78-218, test mode.  `args`: MAX_DISP, HIDDEN_DIMS, N_GRU_LAYERS, CORR_RADIUS, CORR_LEVELS, SLOW_FAST_GRU,
    VALID_ITERS, TRAIN_ITERS.  Every parameter / buffer outside `feature.` / `cnet.` has the reference's name and shape (the small 2-D heads are
    the reference's `.conv` / `.IN` / `.bn` units, igev/submodule.py:6-157), so an IGEV-Stereo checkpoint loads completely."""

    def __init__(self, args, feature=None, cnet=None):
        super().__init__(max_disp=args.MAX_DISP)
        self.args = args
        hd = list(args.HIDDEN_DIMS)
        IN, LR = nn.InstanceNorm2d, nn.LeakyReLU
        self.feature = _pick_feature(feature, "igev")
        self.cnet = cnet if cnet is not None else MultiBasicEncoder(output_dim=[hd, hd], norm_fn="batch", downsample=getattr(args, "N_DOWNSAMPLE", 2))
        self.update_block = BasicMultiUpdateBlock(args, hidden_dims=hd)
        self.context_zqr_convs = nn.ModuleList([nn.Conv2d(hd[i], hd[i] * 3, 3, padding=1) for i in range(args.N_GRU_LAYERS)])
        self.stem_2 = nn.Sequential(BasicConvIN(3, 32, kernel_size=3, stride=2, padding=1),
                                    nn.Conv2d(32, 32, 3, 1, 1, bias=False), IN(32), nn.ReLU())
        self.stem_4 = nn.Sequential(BasicConvIN(32, 48, kernel_size=3, stride=2, padding=1),
                                    nn.Conv2d(48, 48, 3, 1, 1, bias=False), IN(48), nn.ReLU())
        self.spx_2_gru = Conv2xIGEV(32, 32, norm="bn")
        self.spx_gru = nn.Sequential(nn.ConvTranspose2d(2 * 32, 9, kernel_size=4, stride=2, padding=1))
        self.spx = nn.Sequential(nn.ConvTranspose2d(2 * 32, 9, kernel_size=4, stride=2, padding=1))      # init_disp head (training only)
        self.spx_2 = Conv2xIGEV(24, 32, norm="in")
        self.spx_4 = nn.Sequential(BasicConvIN(96, 24, kernel_size=3, stride=1, padding=1),
                                   nn.Conv2d(24, 24, 3, 1, 1, bias=False), IN(24), nn.ReLU())
        self.conv = BasicConvIN(96, 96, kernel_size=3, padding=1, stride=1)
        self.desc = nn.Conv2d(96, 96, kernel_size=1, padding=0, stride=1)

    def side(self, image1, image2):
        image1 = (2 * (image1 / 255.0) - 1.0).contiguous()                    # igev_stereo.py:144-145
        image2 = (2 * (image2 / 255.0) - 1.0).contiguous()
        fl, fr = self.feature(image1), self.feature(image2)
        stem_2x = self.stem_2(image1)
        fl[0] = torch.cat((fl[0], self.stem_4(stem_2x)), 1)
        fr[0] = torch.cat((fr[0], self.stem_4(self.stem_2(image2))), 1)
        ml, mr = self.desc(self.conv(fl[0])), self.desc(self.conv(fr[0]))
        net_list, inp_list = _context_lists(self.cnet, self.context_zqr_convs, image1, self.args.N_GRU_LAYERS)
        return dict(features_left=fl, match_left=ml, match_right=mr, stem_2x=stem_2x, net_list=net_list, inp_list=inp_list)

    def upsample_disp(self, disp, mask_feat_4, stem_2x):
        logits = self.spx_gru(self.spx_2_gru(mask_feat_4, stem_2x))
        return ops.context_upsample(disp, logits, 4, softmax_weights=True, gain=4.0).unsqueeze(1)

    def forward(self, data):
        image1, image2 = data["left"], data["right"]
        _require_engine(image1, "IGEVStereo")
        if self.training:
            return self._train(image1, image2)
        with torch.no_grad():
            return self._infer(image1, image2)

    def _train(self, image1, image2):
        """igev_stereo.py:139-218, training mode (TRAIN_ITERS iterations, every prediction upsampled, init_disp through spx_4 / spx_2 / spx)."""
        from ..attach import context_upsample as ctx_up
        s = self.side(image1, image2)
        st = self.cost_stage_train(s["match_left"], s["match_right"], s["features_left"])
        disp_preds = _gru_train_loop(self, self.args, s, st["init_disp"], st["geo_encoding_volume"], self.args.TRAIN_ITERS,
                                     self.args.N_GRU_LAYERS, self.args.SLOW_FAST_GRU)
        spx_pred = F.softmax(self.spx(self.spx_2(self.spx_4(s["features_left"][0]), s["stem_2x"])), 1)
        init_up = ctx_up(st["init_disp"] * 4.0, spx_pred.float()).unsqueeze(1)
        return {"init_disp": init_up, "disp_preds": disp_preds, "disp_pred": disp_preds[-1]}

    def get_loss(self, model_pred, input_data, static=False):
        return _sequence_loss(model_pred, input_data["disp"], self.max_disp, static)

    def _infer(self, image1, image2):
        s = self.side(image1, image2)
        st = self.cost_stage(s["match_left"], s["match_right"], s["features_left"])
        r = run_refinement(self.update_block, self.args, s["match_left"], s["match_right"], st["geo_encoding_volume"],
                           s["net_list"], s["inp_list"], st["init_disp"], self.args.VALID_ITERS)
        return {"disp_pred": self.upsample_disp(r["disp"], r["mask_feat_4"], s["stem_2x"])}


# ----------------------------------------------------------------------------- LightStereo (BASELINE configs[3])
class LightStereo(LightStereoCostStage):
    """lightstereo.py:13-71.  `cfgs`: MAX_DISP, LEFT_ATT, AGGREGATION_BLOCKS, EXPANSE_RATIO."""

    def __init__(self, cfgs, backbone=None):
        backbone = _pick_feature(backbone, "lightstereo")
        oc = list(backbone.output_channels)
        super().__init__(max_disp=cfgs.MAX_DISP, left_att=cfgs.LEFT_ATT, blocks=tuple(cfgs.AGGREGATION_BLOCKS),
                         expanse_ratio=cfgs.EXPANSE_RATIO, backbone_channels=oc)
        self.backbone = backbone
        IN, BN, LR = nn.InstanceNorm2d, nn.BatchNorm2d, nn.LeakyReLU
        self.refine_1 = nn.Sequential(BasicConv2d(oc[0], 24, kernel_size=3, stride=1, padding=1, norm_layer=IN, act_layer=LR),
                                      BasicConv2d(24, 24, kernel_size=3, stride=1, padding=1, norm_layer=IN, act_layer=nn.ReLU))
        self.stem_2 = nn.Sequential(BasicConv2d(3, 16, kernel_size=3, stride=2, padding=1, norm_layer=BN, act_layer=LR),
                                    BasicConv2d(16, 16, kernel_size=3, stride=1, padding=1, norm_layer=BN, act_layer=nn.ReLU))
        self.refine_2 = FPNLayer(24, 16)
        self.refine_3 = BasicDeconv2d(16, 9, kernel_size=4, stride=2, padding=1)

    def side(self, image1, image2):
        fl, fr = self.backbone(image1), self.backbone(image2)
        spx_logits = self.refine_3(self.refine_2(self.refine_1(fl[0]), self.stem_2(image1)))
        return dict(features_left=fl, feature_right=fr[0], spx_logits=spx_logits)

    def forward(self, data):
        image1, image2 = data["left"], data["right"]
        _require_engine(image1, "LightStereo")
        if self.training:
            return self._train(image1, image2)
        with torch.no_grad():
            return self._infer(image1, image2)

    def _train(self, image1, image2):
        """lightstereo.py:44-71, training mode: correlation volume, aggregation convs and the fused softmax regression forward and backward on
        the engine; disp_4 (bilinear x4 of the quarter-resolution disparity) for the auxiliary loss."""
        from ..attach import context_upsample as ctx_up
        from .. import autograd as A
        s = self.side(image1, image2)
        D4 = self.max_disp // 4
        vol = A.correlation_volume(s["features_left"][0], s["feature_right"], D4)
        enc = self.cost_agg(vol, s["features_left"])[0]
        cost = enc.reshape(enc.size(0), -1, enc.size(2), enc.size(3))
        init_disp = A.softmax_disparity_regression(cost, keepdim=True)
        disp_pred = ctx_up(init_disp * 4.0, F.softmax(s["spx_logits"], 1).float()).unsqueeze(1)
        disp_4 = F.interpolate(init_disp, image1.shape[2:], mode="bilinear", align_corners=False) * 4
        return {"disp_pred": disp_pred, "disp_4": disp_4}

    def get_loss(self, model_pred, input_data, static=False):
        """lightstereo.py:72-85 (static: static-shape form for hipGraph capture, see _sequence_loss)"""
        disp_gt = input_data["disp"].unsqueeze(1)
        mask = (disp_gt < self.max_disp) & (disp_gt > 0)
        if static:
            sl1 = lambda p: _masked_mean(F.smooth_l1_loss(p, disp_gt, reduction="none"), mask)
            loss = sl1(model_pred["disp_pred"]) + 0.3 * sl1(model_pred["disp_4"])
            return loss, {"scalar/train/loss_disp": loss.detach()}
        loss = F.smooth_l1_loss(model_pred["disp_pred"][mask], disp_gt[mask], reduction="mean") \
            + 0.3 * F.smooth_l1_loss(model_pred["disp_4"][mask], disp_gt[mask], reduction="mean")
        return loss, {"scalar/train/loss_disp": float(loss.detach())}

    def _infer(self, image1, image2):
        s = self.side(image1, image2)
        st = LightStereoCostStage.forward(self, s["features_left"], s["feature_right"])
        disp = ops.context_upsample(st["init_disp"], s["spx_logits"].float(), 4, softmax_weights=True, gain=4.0).unsqueeze(1)
        return {"disp_pred": disp}
