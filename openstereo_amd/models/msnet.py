"""MobileStereoNet's 3-D inverted-residual block on the gfx950 engine: eval mode as ONE launch (csrc/mv2_block3d.hip).

Mirror of stereo/modeling/models/msnet/submodule.py:136-173 for attach._graft: it reads the reference's attribute layout
(`self.conv`, `self.use_res_connect`) and has no constructor of its own.  Training keeps the reference's forward (attach: train_fallback)."""
import torch

from .. import _ext
from ..engine import bn_scale_shift, cached_pack


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
