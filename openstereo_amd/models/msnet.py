"""MobileStereoNet on the gfx950 engine: the 3-D and the 2-D inverted-residual block (csrc/mv2_block3d.hip, csrc/mv2_block2d.hip) and
MSNet2D's interlaced cost volume (csrc/interlaced_volume.hip) in eval mode as ONE launch each.

Mirrors of stereo/modeling/models/msnet/submodule.py:94-173 and MSNet2D.py:48-212 for attach._graft: they read the reference's attribute
layout and have no constructors of their own.  Training keeps the reference's forward (attach: train_fallback)."""
import torch

from .. import _ext, ops
from ..engine import bn_scale_shift, cached_pack, PackedMirror
from .interlaced import interlaced_volume

def mv2_block(blk, x, addend=None, relu=False, rank=2):
    """relu?(blk(x) (+ addend)) for a MobileV2_Residual (rank 2) or MobileV2_Residual_3D (rank 3) `blk` (submodule.py:94-173: `conv` of eight entries, `use_res_connect`): one
    fused launch where csrc/mv2_block2d.hip / mv2_block3d.hip applies, else the block's own composition; the sum and the ReLU are the 2-D kernel's epilogue, else torch operators"""
    c, one, ts, dw = blk.conv, (1,) * rank, [t for t in (x, addend) if t is not None], blk.conv[3] if len(blk.conv) == 8 else None   # expanse_ratio == 1: five entries, no dw
    tops = {2: (192, 384, 192), 3: (128, 256, 128)}[rank]     # the most input, hidden and output channels csrc/mv2_block2d.hip / mv2_block3d.hip take
    if (dw is None or blk.training or torch.is_autocast_enabled() or any(t.dim() != rank + 2 or not t.is_cuda or t.dtype != torch.float32 for t in ts)
            or (torch.is_grad_enabled() and any(t.requires_grad for t in (*ts, *c.parameters())))        # an inference op: it records no gradient
            or (dw.kernel_size, dw.padding, dw.dilation) != ((3,) * rank, one, one) or dw.stride not in (one, (2,) * rank)
            or any(n % 8 or n > top for n, top in zip((c[0].in_channels, dw.out_channels, c[6].out_channels), tops))):
        y = x + c(x) if blk.use_res_connect else c(x)
    else:
        ns = _ext.load()
        pk = cached_pack(blk, "_eng", lambda: getattr(ns, f"mv2_block{rank}d_pack")(c[0].weight, dw.weight, c[6].weight, *bn_scale_shift(c[1]), *bn_scale_shift(c[4]), *bn_scale_shift(c[7])))
        args = (x, pk, dw.out_channels, c[6].out_channels, dw.stride[0], bool(blk.use_res_connect))
        if rank == 2:
            return ns.mv2_block2d(*args, addend, bool(relu))
        y = ns.mv2_block3d(*args)
    y = y if addend is None else y + addend
    return torch.relu(y) if relu else y


mv2_block2d = mv2_block                                      # the name of the 2-D form (rank 2 is the default)


def mv2_sequential(seq, x, addend=None):
    """Sequential of MobileV2_Residual blocks and ReLUs (MSNet2D.py:86-93) (+ addend): a ReLU behind a block, or the addend behind a last block, is its epilogue"""
    mods, blocks = list(seq), [hasattr(m, "use_res_connect") for m in seq]
    for i, m in enumerate(mods):
        if blocks[i]:
            x = mv2_block2d(m, x, addend if i + 1 == len(mods) else None, i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.ReLU))
        elif not (i and blocks[i - 1] and isinstance(m, torch.nn.ReLU)):
            x = m(x)
    return x if addend is None or blocks[-1] else x + addend


def hourglass2d(hg, x):
    """hourglass2D.forward (MSNet2D.py:35-45), relu(deconv + redir(.)) as the redir block's epilogue (a + b == b + a); torch's deconvs get contiguous input"""
    conv2 = mv2_block2d(hg.conv2, mv2_block2d(hg.conv1, x))
    conv4 = mv2_block2d(hg.conv4, mv2_block2d(hg.conv3, conv2))
    conv5 = mv2_block2d(hg.redir2, conv2, hg.conv5(conv4.contiguous()), True)
    return mv2_block2d(hg.redir1, x, hg.conv6(conv5.contiguous()), True)


class MobileV2Residual3D(PackedMirror):
    def forward(self, x):
        return mv2_block(self, x, rank=3)


class MobileV2Residual2D(MobileV2Residual3D):                # reset_engine as above
    def forward(self, x):
        return mv2_block2d(self, x)


class MSNet2D(torch.nn.Module):
    reset_engine = PackedMirror.reset_engine

    def forward(self, data):
        L, R = data["left"], data["right"]
        if not (L.is_cuda and R.is_cuda and L.dtype == R.dtype == torch.float32) or torch.is_autocast_enabled() or (torch.is_grad_enabled() and (L.requires_grad or R.requires_grad)):
            return self._ref_forward(data)                # MSNet2D.py:134-212 as it is (attach._graft keeps it on the class)
        fe = self.feature_extraction                      # submodule.py:225-234, firstconv's ReLUs fused; the MobileV1 layers stay torch, on contiguous input
        l2 = [fe.layer2(fe.layer1(mv2_sequential(fe.firstconv, im).contiguous())) for im in (L, R)]
        l3 = [fe.layer3(t) for t in l2]
        fl, fr = (self.preconv11(torch.cat((a, b, fe.layer4(b)), 1)) for a, b in zip(l2, l3))
        volume = interlaced_volume(self, [*self.conv3d[0::3], self.volume11[0][0]], [*self.conv3d[1::3], self.volume11[0][1]], fl, fr, self.volume_size)[:, 0]
        cost0 = mv2_sequential(self.dres0, volume)
        cost0 = mv2_sequential(self.dres1, cost0, addend=cost0)
        cost3 = self.classif3(hourglass2d(self.encoder_decoder3, hourglass2d(self.encoder_decoder2, hourglass2d(self.encoder_decoder1, cost0))).contiguous())
        return {"disp_pred": ops.upsample_softargmin(cost3, self.maxdisp, L.shape[2], L.shape[3])}
