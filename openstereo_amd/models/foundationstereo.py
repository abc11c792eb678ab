"""FoundationStereo on the gfx950 engine: the disparity transformer `CostVolumeDisparityAttention` (foundationstereo/core/submodule.py:540-562 and
fast_foundationstereo/core/submodule.py:581-603) in eval mode as ONE launch (csrc/disparity_attention.hip).  A mirror for attach._graft:
it reads the reference's attribute layout and has no constructor.  Training keeps the reference's forward (attach: train_fallback)."""
import torch

from .. import _ext
from ..engine import cached_pack, PackedMirror


class CostVolumeDisparityAttention(PackedMirror):
    def forward(self, cv, window_size=(-1, -1)):
        sa, at, nn = self.sa, self.sa[0].self_attn, torch.nn
        C, nh, ff, L, mods = at.embed_dim, at.num_heads, sa[0].linear1.out_features, cv.shape[2], lambda l: (l.self_attn.q_proj, l.self_attn.k_proj, l.self_attn.v_proj, l.self_attn.out_proj, l.linear1, l.linear2, l.norm1, l.norm2)
        if (self.training or not cv.is_cuda or cv.dtype != torch.float32 or torch.is_autocast_enabled() or (torch.is_grad_enabled() and cv.requires_grad) or tuple(window_size) != (-1, -1)
                or not (0 < L <= 32 and C <= 32 and ff <= 32 and C % 4 == ff % 4 == C % nh == 0 and len(sa) <= 8 and cv.shape[1] == C)       # the range of the kernel
                or any(type(n) is not nn.LayerNorm or n.eps != 1e-5 or n.weight is None or n.bias is None for l in sa for n in (l.norm1, l.norm2))
                or any(type(l.act) is not nn.GELU or l.act.approximate != "none" for l in sa)):
            return self._ref_forward(cv, window_size=window_size)        # the reference's composition as it is (attach._graft keeps it on the class)
        ns = _ext.load()
        pk = cached_pack(self, "_eng", lambda: ns.disparity_attention_pack([t for l in sa for m in mods(l) for t in (m.weight, m.bias)], nh))
        pe = self.pos_embed0(cv.new_zeros(1, L, C), resize_embed=self.resize_embed)    # the module's own table and resize rule; RuntimeError when L > max_len without resize
        return ns.disparity_attention(cv, pe, pk, C, nh, ff, len(sa))
