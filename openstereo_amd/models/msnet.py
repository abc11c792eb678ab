"""MobileStereoNet on the gfx950 engine: the 3-D inverted-residual block (csrc/mv2_block3d.hip) and MSNet2D's interlaced cost volume
(csrc/interlaced_volume.hip) in eval mode as ONE launch each.

Mirrors of stereo/modeling/models/msnet/submodule.py:136-173 and MSNet2D.py:48-212 for attach._graft: they read the reference's attribute
layout and have no constructors of their own.  Training keeps the reference's forward (attach: train_fallback)."""
import torch

from .. import _ext, ops
from ..engine import bn_scale_shift, cached_pack
from .interlaced import interlaced_volume


class MobileV2Residual3D(torch.nn.Module):
    def reset_engine(self):
        self._eng = None

    def forward(self, x):
        c = self.conv
        if len(c) != 8 or x.dim() != 5 or not x.is_cuda or x.dtype != torch.float32 or torch.is_autocast_enabled():
            y = c(x)                                     # the block's own composition: expanse_ratio == 1, CPU, other dtypes, autocast
            return x + y if self.use_res_connect else y
        ns = _ext.load()
        pk = cached_pack(self, "_eng", lambda: ns.mv2_block3d_pack(c[0].weight, c[3].weight, c[6].weight, *bn_scale_shift(c[1]), *bn_scale_shift(c[4]), *bn_scale_shift(c[7])))
        return ns.mv2_block3d(x, pk, c[3].out_channels, c[6].out_channels, c[3].stride[0], bool(self.use_res_connect))


class MSNet2D(torch.nn.Module):
    def reset_engine(self):
        self._eng = None

    def forward(self, data):
        L, R = data["left"], data["right"]
        if not (L.is_cuda and R.is_cuda and L.dtype == R.dtype == torch.float32) or torch.is_autocast_enabled() or (torch.is_grad_enabled() and (L.requires_grad or R.requires_grad)):
            return self._ref_forward(data)                # MSNet2D.py:134-212 as it is (attach._graft keeps it on the class)
        fl, fr = self.preconv11(self.feature_extraction(L)), self.preconv11(self.feature_extraction(R))
        volume = interlaced_volume(self, [*self.conv3d[0::3], self.volume11[0][0]], [*self.conv3d[1::3], self.volume11[0][1]], fl, fr, self.volume_size)[:, 0]
        cost0 = self.dres0(volume)
        cost0 = self.dres1(cost0) + cost0
        cost3 = self.classif3(self.encoder_decoder3(self.encoder_decoder2(self.encoder_decoder1(cost0))))
        return {"disp_pred": ops.upsample_softargmin(cost3, self.maxdisp, L.shape[2], L.shape[3])}
