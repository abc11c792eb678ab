"""FoundationStereo on the gfx950 engine, each in eval mode as ONE launch: the disparity transformer `CostVolumeDisparityAttention` (foundationstereo/core/submodule.py:540-562,
fast_foundationstereo/core/submodule.py:581-603; csrc/disparity_attention.hip) and the hourglass's block `Conv3dNormActReduced` (:87-112 and :90-115;
csrc/conv3d_reduced.hip).  Mirrors for attach._graft: the reference's attribute layout, no constructors; training keeps the reference's forward (train_fallback)."""
import torch

from .. import _ext
from ..engine import bn_scale_shift, cached_pack, PackedMirror


def _eval_f32(mod, x):             # what both fused launches need: eval mode and a CUDA fp32 tensor, outside autocast, that records no gradient
    return not (mod.training or not x.is_cuda or x.dtype != torch.float32 or torch.is_autocast_enabled() or (torch.is_grad_enabled() and x.requires_grad))


class CostVolumeDisparityAttention(PackedMirror):
    def forward(self, cv, window_size=(-1, -1)):
        sa, at, nn = self.sa, self.sa[0].self_attn, torch.nn
        C, nh, ff, L, mods = at.embed_dim, at.num_heads, sa[0].linear1.out_features, cv.shape[2], lambda l: (l.self_attn.q_proj, l.self_attn.k_proj, l.self_attn.v_proj, l.self_attn.out_proj, l.linear1, l.linear2, l.norm1, l.norm2)
        if (not _eval_f32(self, cv) or tuple(window_size) != (-1, -1)
                or not (0 < L <= 32 and C <= 32 and ff <= 32 and C % 4 == ff % 4 == C % nh == 0 and len(sa) <= 8 and cv.shape[1] == C)       # the range of the kernel
                or any(type(n) is not nn.LayerNorm or n.eps != 1e-5 or n.weight is None or n.bias is None for l in sa for n in (l.norm1, l.norm2))
                or any(type(l.act) is not nn.GELU or l.act.approximate != "none" for l in sa)):
            return self._ref_forward(cv, window_size=window_size)        # the reference's composition as it is (attach._graft keeps it on the class)
        ns = _ext.load()
        pk = cached_pack(self, "_eng", lambda: ns.disparity_attention_pack([t for l in sa for m in mods(l) for t in (m.weight, m.bias)], nh))
        pe = self.pos_embed0(cv.new_zeros(1, L, C), resize_embed=self.resize_embed)    # the module's own table and resize rule; RuntimeError when L > max_len without resize
        return ns.disparity_attention(cv, pe, pk, C, nh, ff, len(sa))


class Conv3dNormActReduced(PackedMirror):
    def forward(self, x):
        (c1, n1, a1), (c2, n2, a2), nn, one, ks, kd = self.conv1, self.conv2, torch.nn, (1, 1, 1), self.conv1[0].kernel_size[1], self.conv2[0].kernel_size[0]
        if (not _eval_f32(self, x) or x.dim() != 5 or x.shape[1] != c1.in_channels or x.numel() == 0
                or any(type(n) is not nn.BatchNorm3d or n.running_mean is None for n in (n1, n2)) or type(a1) is not nn.ReLU or type(a2) is not nn.ReLU
                or (c1.kernel_size, c1.padding, c2.kernel_size, c2.padding) != ((1, ks, ks), (0, ks // 2, ks // 2), (kd, 1, 1), (kd // 2, 0, 0))      # the block's own
                or any((c.stride, c.dilation, c.groups, c.padding_mode) != (one, one, 1, "zeros") or c.bias is None for c in (c1, c2))
                or not (ks in (1, 3) and kd % 2 and kd <= 17 and all(0 < n <= 32 and n % 4 == 0 for n in (c1.in_channels, c1.out_channels, c2.out_channels)))):   # the range of the kernel
            return self._ref_forward(x)                                  # wider blocks (56 .. 168 channels), strides, other norms: the reference's composition
        ns = _ext.load()
        pk = cached_pack(self, "_eng", lambda: ns.conv3d_reduced_pack(c1.weight, c1.bias, *bn_scale_shift(n1), c2.weight, c2.bias, *bn_scale_shift(n2)))
        return ns.conv3d_reduced(x, pk, c1.out_channels, c2.out_channels, ks, kd)
