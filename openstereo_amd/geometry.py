"""CombinedGeoEncodingVolume on the engine.

Same constructor / call contract as models/stereobase/gru_blocks.py:170-229 and
models/igev/geometry.py:7-66: built once per forward from the matching features and the aggregated
geometry volume, then called once per GRU iteration with the current disparity.  The engine keeps the
volume as per-pixel rows ([B,H,W,C,D], D contiguous) plus an averaged pyramid, and one fused kernel per
iteration produces the reference's [B,(C+1)*(2r+1)*levels,H,W] tensor (replacing 2*levels grid_sample
calls, their coordinate tensors and the concatenations).
MultiRangeGeoEncodingVolume is IGEV++'s lookup (models/igevpp/geometry.py:6-87): three volumes of different disparity ranges + the correlation
pyramid -> (geo_feat0, geo_feat1, geo_feat2, init_corr) from one launch per iteration."""
import os

import torch

from . import _ext, ops, timing
from .ops import _f32c, is_cl

ACC_LOOKUP_BWD = os.environ.get("OSA_LOOKUP_BWD_ACC", "1") != "0"


def _channels(mr, C, radius, L):
    """channel counts of a lookup's results: one interleaved tensor, or IGEV++'s geo_feat0, geo_feat1, geo_feat2, init_corr"""
    T = 2 * radius + 1
    return (L * C * T, C * T, C * T, L * T) if mr else ((C + 1) * T * L,)


def _launch(mr, form, levels, d, cx, outs, *rest):
    """geo_lookup<form> (geo levels + corr levels -> 1 tensor) or geo_lookup_mr<form> (volume-0 levels, volume 1, volume 2, corr levels -> 4); rest: [stride(s), bhw,] C, radius"""
    getattr(_ext.load(), ("geo_lookup_mr" if mr else "geo_lookup") + form)(levels, d, cx, outs if mr else outs[0], *rest)


class _LevelAcc:
    """gradient accumulators of one pyramid (one CombinedGeoEncodingVolume = one forward): zero-filled by the first lookup backward of a
    backward pass, added to by every lookup backward (osa_geo_lookup_bwd_acc_f32), handed to autograd ONCE by _LevelJoin.backward"""
    __slots__ = ("acc",)

    def __init__(self):
        self.acc = None


class _SourceAcc(_LevelAcc):
    """the accumulators of IGEV++'s 2 L + 2 sources: a _Lookup that carries them is the multi-range one (four results, osa_geo_lookup_mr_*_f32)"""


class _LevelJoin(torch.autograd.Function):
    """Identity on the pyramid levels, applied once when the pyramid is built -- i.e. BEFORE every lookup, so its backward node runs after
    all lookup backward nodes of the running backward pass (autograd's own dependency count: also right for a backward pass that reaches
    only some of the iterations).  The lookups return no level gradients of their own; this node returns the accumulated ones."""

    @staticmethod
    def forward(ctx, state, *levels):
        ctx.state = state
        ctx.set_materialize_grads(False)
        return tuple(t.view_as(t) for t in levels)

    @staticmethod
    def backward(ctx, *grads):
        acc, ctx.state.acc = ctx.state.acc, None
        if acc is None:
            return (None, *grads)
        return (None, *[a if g is None else a + g for a, g in zip(acc, grads)])


class _Lookup(torch.autograd.Function):
    """out = lookup(disp, coords; geo levels, corr levels) with gradients for the levels (osa_geo_lookup_bwd_f32).  The disparity is
    detached in the reference's loop (igev_stereo.py:190, stereobase_gru.py:186), so it gets none.
    The kernels take fp32 rows: inside an autocast region the levels arrive cast to fp32 (custom_fwd) and every tensor is passed through
    `_f32c` -- handing the raw pointer of an fp16 pyramid level to the kernel reads past its end (found by tests/test_gpu_autocast.py)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, d, cx, C, radius, state, *levels):
        d, cx, levels = _f32c(d), _f32c(cx), tuple(_f32c(t) for t in levels)
        ctx.state, mr = state, isinstance(state, _SourceAcc)
        B, H, W = d.shape
        L = (len(levels) - 2) // 2 if mr else len(levels) // 2
        outs = [torch.empty((B, n, H, W), device=d.device, dtype=torch.float32) for n in _channels(mr, C, radius, L)]
        _launch(mr, "", list(levels), d, cx, outs, C, radius)                # the pyramid as a tensor list
        ctx.save_for_backward(d, cx)
        ctx.meta = (C, radius, [tuple(t.shape) for t in levels])
        return tuple(outs) if mr else outs[0]

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, *douts):
        d, cx = ctx.saved_tensors
        C, radius, shapes = ctx.meta
        st, douts = ctx.state, [_f32c(g) for g in douts]
        if st is not None:
            # accumulate into the pyramid's gradient buffers; _LevelJoin delivers them (r6)
            if st.acc is None:
                st.acc = [torch.zeros(s, device=d.device, dtype=torch.float32) for s in shapes]
            _launch(isinstance(st, _SourceAcc), "_bwd_acc", st.acc, d, cx, douts, C, radius)
            return (None, None, None, None, None, *([None] * len(shapes)))
        grads = [torch.empty(s, device=d.device, dtype=torch.float32) for s in shapes]
        _ext.load().geo_lookup_bwd(grads, d, cx, douts[0], C, radius)
        return (None, None, None, None, None, *grads)


class CombinedGeoEncodingVolume:
    MR = False

    def __init__(self, init_fmap1, init_fmap2, geo_volume, num_levels=2, radius=4):
        self._build([geo_volume], init_fmap1, init_fmap2, num_levels, radius)

    def _build(self, vols, init_fmap1, init_fmap2, num_levels, radius):
        """vols[0] and the all-pairs correlation get an averaged pyramid of num_levels levels; further volumes (IGEV++) stay single rows"""
        assert 1 <= num_levels <= 4
        self.num_levels, self.radius = num_levels, radius
        self.train_path = torch.is_grad_enabled() and any(t.requires_grad for t in (init_fmap1, init_fmap2, *vols))
        if self.train_path:
            # Training: the pyramid is built from differentiable torch ops (a permutation, an einsum, two average pools: once per
            # forward), the per-iteration lookup and its gradient run on the engine (_Lookup).
            # fp32 throughout, whatever autocast region surrounds the call: the reference casts its inputs to fp32 here too
            # (`match_left.float()`, igev_stereo.py:184) but its einsum / pooling still run in the autocast dtype; the engine keeps the
            # pyramid in fp32 -- no fp16 overflow of the 96-term correlation sums, and the levels are what _Lookup's kernels read.
            # The pooling is written as a strided add (exactly F.avg_pool2d(x, [1, 2], stride=[1, 2]): (a + b) / 2, a trailing odd
            # element dropped) on fp32 tensors; a memory-access fault first blamed on F.avg_pool1d with fp16 rows turned out to be _Lookup's kernels
            # being handed fp16 levels (no custom_fwd cast at the time; tools/diag_lookup_ac.py) -- the fp32 pyramid is what fixed it.
            with torch.autocast("cuda", enabled=False):
                f1, f2 = init_fmap1.float(), init_fmap2.float()
                rows = [v.float().permute(0, 3, 4, 1, 2).contiguous() for v in vols]             # [B,H,W,C,D]
                B, H, W1, C, _ = rows[0].shape
                corr = torch.einsum("aijk,aijh->ajkh", f1, f2).contiguous()                       # [B,H,W1,W2]
                geo, cor = [rows[0]], [corr]
                half = lambda t: ((t[..., 0:t.shape[-1] // 2 * 2:2] + t[..., 1::2]) * 0.5).contiguous()
                for _ in range(num_levels - 1):
                    geo.append(half(geo[-1])); cor.append(half(cor[-1]))
        else:
            f1, f2 = _f32c(init_fmap1), _f32c(init_fmap2)
            B, _, H, W1 = f1.shape
            dev = f1.device
            corr = torch.empty((B, H, W1, f2.shape[3]), device=dev, dtype=torch.float32)
            ext = _ext.load()
            ext.allpairs_corr(f1, f2, corr)
            rows = []
            for v in vols:
                gv = v if is_cl(v) and v.dtype == torch.float32 else ops.to_cl(v.float(), pad_to=1)
                _, Cs, D, Hg, Wg = gv.shape
                C = v.shape[1] if not is_cl(v) else Cs
                assert (Hg, Wg) == (H, W1) and (not rows or rows[0].shape[3] == C)      # one map size, one channel count
                rows.append(torch.empty((B, H, W1, C, D), device=dev, dtype=torch.float32))
                ext.geo_rows(gv, rows[-1], C)
            geo, cor = [rows[0]], [corr]
            for _ in range(num_levels - 1):
                for pyr in (geo, cor):
                    pyr.append(torch.empty(pyr[-1].shape[:-1] + (pyr[-1].shape[-1] // 2,), device=dev, dtype=torch.float32))
                    ext.avgpool_rows(pyr[-2], pyr[-1])
        self.C, self.shape = C, (B, H, W1)
        self.sources, self._acc = geo + rows[1:] + cor, None                                      # the kernels' order
        if self.train_path and (self.MR or ACC_LOOKUP_BWD):
            self._acc = _SourceAcc() if self.MR else _LevelAcc()
            self.sources = list(_LevelJoin.apply(self._acc, *self.sources))
        self.geo_volume_pyramid, self.init_corr_pyramid = self.sources[:num_levels], self.sources[-num_levels:]
        # range block of every lookup result (f16x3 consumers; IGEV++: one per result): taps are convex combinations of volume entries or zero,
        # the coarser pyramid levels are averages -> bounded by max |level 0|; measured once here, not once per iteration
        from .ranges import new_meta
        tops = [t.detach().abs().amax().reshape(1) for t in (*rows, corr)]
        self.metas = [new_meta(corr.device) for _ in (tops if self.MR else tops[:1])]
        for m, t in zip(self.metas, tops if self.MR else [torch.maximum(*tops)]):
            m[0:1] = t
        self.meta = self.metas[0]

    def __call__(self, disp, coords):
        """disp [B,1,H,W] (quarter-res disparity), coords [B,H,W,1] (x coordinate grid) ->
        [B,(C+1)*(2r+1)*levels,H,W] float32 (IGEV++: the four tensors of MultiRangeGeoEncodingVolume)."""
        B, H, W = self.shape
        d, cx = _f32c(disp).reshape(B, H, W), _f32c(coords).reshape(B, H, W)
        if self.train_path:
            return _Lookup.apply(d.detach(), cx.detach(), self.C, self.radius, self._acc, *self.sources)
        outs = [torch.empty((B, n, H, W), device=d.device, dtype=torch.float32) for n in _channels(self.MR, self.C, self.radius, self.num_levels)]
        with timing.span("geo_lookup_mr" if self.MR else "geo_lookup", self.C, self.num_levels, self.radius, H, W):
            _launch(self.MR, "", self.sources, d, cx, outs, self.C, self.radius)
        return tuple(outs) if self.MR else outs[0]

    def lookup_cl(self, disp, coords):
        """The same lookup as NHWC engine tensor(s) [B, Cpad4, 1, H, W] (padding channels zero) for the engine's GRU loop (osa_geo_lookup[_mr]_nhwc_f32):
        what the motion encoder's 1x1 convc1 (IGEV++: GeoEncoder's convg1 / convc1, igevpp/update.py:72-80) reads, without a transpose per iteration.
        disp / coords: fp32, [B,1,H,W] / [B,H,W,1] (or any shape with B*H*W elements), contiguous.  Inference path only."""
        assert not self.train_path
        B, H, W = self.shape
        outs = [ops.empty_cl(B, (n + 3) // 4 * 4, 1, H, W, disp.device) for n in _channels(self.MR, self.C, self.radius, self.num_levels)]
        d, cx = _f32c(disp), _f32c(coords)
        assert d.numel() == B * H * W and cx.numel() == B * H * W
        cs = [o.shape[1] for o in outs]
        with timing.span("geo_lookup_mr" if self.MR else "geo_lookup", self.C, self.num_levels, self.radius, H, W):
            _launch(self.MR, "_nhwc", self.sources, d, cx, outs, cs if self.MR else cs[0], [B, H, W], self.C, self.radius)
        for o, m in zip(outs, self.metas):
            o._osa_meta = m                        # taps interpolate / zero-pad the volumes: bounded by their max |.|
        return tuple(outs) if self.MR else outs[0]

    @staticmethod
    def corr(fmap1, fmap2):
        """einsum('aijk,aijh->ajkh') -> [B,H,W1,1,W2] (gru_blocks.py:221-229)."""
        f1, f2 = _f32c(fmap1), _f32c(fmap2)
        B, _, H, W1 = f1.shape
        out = torch.empty((B, H, W1, 1, f2.shape[3]), device=f1.device, dtype=torch.float32)
        _ext.load().allpairs_corr(f1, f2, out)
        return out


class MultiRangeGeoEncodingVolume(CombinedGeoEncodingVolume):
    """IGEV++'s Combined_Geo_Encoding_Volume (models/igevpp/geometry.py:6-87), the reference's constructor order: geo_volume0 [B,C,D0,H,W] and
    the correlation get the pyramid (sampled at disp / 2^l), geo_volume1 / 2 [B,C,D1|D2,H,W] are sampled at disp / 2 and disp / 4.  __call__ and
    lookup_cl return (geo_feat0 [B,L*C*T,H,W], geo_feat1 [B,C*T,H,W], geo_feat2 [B,C*T,H,W], init_corr [B,L*T,H,W]), T = 2r + 1."""
    MR = True

    def __init__(self, geo_volume0, geo_volume1, geo_volume2, init_fmap1, init_fmap2, radius=4, num_levels=2):
        self._build([geo_volume0, geo_volume1, geo_volume2], init_fmap1, init_fmap2, num_levels, radius)


Combined_Geo_Encoding_Volume = CombinedGeoEncodingVolume      # IGEV's name (models/igev/geometry.py:7)
Combined_Geo_Encoding_Volume_PP = MultiRangeGeoEncodingVolume  # IGEV++'s class of the same name (models/igevpp/geometry.py:6)
