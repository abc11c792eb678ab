"""Shared by tests/test_disparity_attention_cpu.py, tests/test_gpu_disparity_attention.py and tests/golden/make_golden_disparity_attention.py
(a plain module, no fixtures): the cases, the seeded parameters and inputs, a torch restatement of FoundationStereo's disparity transformer
(foundationstereo/core/submodule.py:195-291, 506-562, CostVolumeDisparityAttention) and the tolerance rule.

The restatement keeps the reference's attribute names (sa[i].self_attn.{q,k,v,out}_proj, linear1/2, norm1/2, act, pos_embed0, resize_embed),
so its state_dict keys are the reference's and the engine's mirror grafts onto it.  Attention is the plain softmax(q k^T / sqrt(dh)) v, which
also runs in float64.

The tolerance rule, as in tests/mv2_cases_common.py: err(X) = max |X - float64 restatement| on the same inputs, and the kernel must satisfy
err(X) <= 8 * err(float32 restatement); both numbers are printed.  The factor 8 is the one the project uses for kernels that sum in another
order (here: the channels of every product in the order 0-3, 8-11, .. | 4-7, 12-15, .. of the matrix unit's two lane halves).

A test of this module passes vacuously when the softmax is uniform or one-hot, or when GELU sees only its linear or only its zero branch, so
reference() asserts on the float64 run of every case outside DEGENERATE, per layer: the mean over rows of the largest attention probability
lies in [1.5 / L, 0.9], and at least 10 % of the feed-forward pre-activations lie below -1 and at least 10 % above +1.

Seeds: Linear weights ~ 1.25 N(0,1) / sqrt(fan_in), Linear biases ~ 0.5 N(0,1), LayerNorm weight ~ U(0.5, 2), LayerNorm bias ~ 0.5 N(0,1),
in the order of module.modules() from one generator per case; cv ~ N(0,1).
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

FACTOR = 8.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disparity_attention.npz")

# case: (B, C, nhead, ff, layers, L, max_len, resize, H, W)
CASES = {
    "fs416": (2, 28, 4, 28, 4, 26, 26, False, 3, 5),       # the model's configuration; batch stride; 30 sequences: a ragged last workgroup; pad rows and channels
    "fs192": (1, 28, 4, 28, 4, 12, 12, False, 2, 7),       # the max_disp 192 configs; L below 16
    "full": (1, 32, 4, 32, 2, 32, 32, False, 2, 3),        # no padding in either dimension
    "heads8": (1, 24, 8, 16, 1, 5, 8, False, 1, 2),        # dh = 3 (odd K); ff != C; L < max_len; fewer sequences than one workgroup
    "one": (1, 28, 4, 28, 4, 1, 26, False, 2, 2),          # L = 1: softmax over one key
    "resize": (1, 28, 4, 28, 2, 30, 26, True, 2, 3),       # interpolated position table
    "many": (1, 28, 4, 28, 1, 26, 26, False, 9, 129),      # 1161 sequences: every workgroup of the grid walks more than one group
}
DEGENERATE = ("one",)
GOLDEN_CASES = ("fs416", "heads8", "resize")
SEED = 20261020


class PositionalEmbedding(nn.Module):
    """sinusoidal table [1, max_len, d_model], a plain attribute as in the reference; linearly resized when the sequence is longer and
    resize_embed is set (align_corners: False in foundationstereo, True in fast_foundationstereo)"""

    def __init__(self, d_model, max_len=512, align_corners=False):
        super().__init__()
        pos = torch.arange(max_len, dtype=torch.float32)[:, None]
        freq = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float32) * (-math.log(10000.0) / d_model))[None]
        pe = torch.zeros(max_len, d_model)
        pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * freq), torch.cos(pos * freq)
        self.pe, self.align_corners = pe[None], align_corners

    def forward(self, x, resize_embed=False):
        self.pe = pe = self.pe.to(x.device).to(x.dtype)
        if pe.shape[1] < x.shape[1]:
            if not resize_embed:
                raise RuntimeError(f"x:{x.shape}, pe:{pe.shape}")
            pe = F.interpolate(pe.permute(0, 2, 1), size=x.shape[1], mode="linear", align_corners=self.align_corners).permute(0, 2, 1)
        return x + pe[:, :x.size(1)]


class Attention(nn.Module):
    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.num_heads, self.embed_dim, self.head_dim = num_heads, embed_dim, embed_dim // num_heads
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = (nn.Linear(embed_dim, embed_dim) for _ in range(4))
        self.stats = None                                    # a list: forward appends the mean over rows of the largest probability

    def forward(self, query, key, value, attn_mask=None, window_size=(-1, -1)):
        if tuple(window_size) != (-1, -1):
            raise NotImplementedError(f"window_size = {window_size}")
        B, L, _ = query.shape
        q, k, v = (p(t).view(B, L, self.num_heads, self.head_dim).transpose(1, 2) for p, t in ((self.q_proj, query), (self.k_proj, key), (self.v_proj, value)))
        prob = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(self.head_dim), dim=-1)
        if self.stats is not None:
            self.stats.append(float(prob.max(-1).values.double().mean()))
        return self.out_proj((prob @ v).transpose(1, 2).reshape(B, L, -1))


class EncoderLayer(nn.Module):
    def __init__(self, embed_dim, num_heads, dim_feedforward, dropout=0.1, act=nn.GELU, norm=nn.LayerNorm):
        super().__init__()
        self.self_attn, self.act = Attention(embed_dim, num_heads), act()
        self.linear1, self.dropout, self.linear2 = nn.Linear(embed_dim, dim_feedforward), nn.Dropout(dropout), nn.Linear(dim_feedforward, embed_dim)
        self.norm1, self.norm2, self.dropout1, self.dropout2 = norm(embed_dim), norm(embed_dim), nn.Dropout(dropout), nn.Dropout(dropout)
        self.stats = None                                    # a list: forward appends the shares of pre-activations below -1 and above +1

    def forward(self, src, src_mask=None, window_size=(-1, -1)):
        src = self.norm1(src + self.dropout1(self.self_attn(src, src, src, src_mask, window_size=window_size)))
        pre = self.linear1(src)
        if self.stats is not None:
            self.stats.append((float((pre < -1).double().mean()), float((pre > 1).double().mean())))
        return self.norm2(src + self.dropout2(self.linear2(self.dropout(self.act(pre)))))


class CostVolumeDisparityAttention(nn.Module):
    def __init__(self, d_model, nhead, dim_feedforward, dropout=0.1, act=nn.GELU, num_transformer=6, max_len=512, resize_embed=False, align_corners=False):
        super().__init__()
        self.resize_embed = resize_embed
        self.sa = nn.ModuleList(EncoderLayer(d_model, nhead, dim_feedforward, dropout, act) for _ in range(num_transformer))
        self.pos_embed0 = PositionalEmbedding(d_model, max_len, align_corners)

    def forward(self, cv, window_size=(-1, -1)):
        B, C, D, H, W = cv.shape
        x = self.pos_embed0(cv.permute(0, 3, 4, 2, 1).reshape(B * H * W, D, C), resize_embed=self.resize_embed)
        for layer in self.sa:
            x = layer(x, window_size=window_size)
        return x.reshape(B, H, W, D, C).permute(0, 4, 3, 1, 2)


def seed_parameters(module, g):
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 1.25 / math.sqrt(m.in_features))
                m.bias.copy_(0.5 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, nn.LayerNorm):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 1.5 + 0.5)
                m.bias.copy_(0.5 * torch.randn(m.bias.shape, generator=g))
    return module


def _generator(case):
    return torch.Generator().manual_seed(SEED + list(CASES).index(case))


def make_module(case, dtype=torch.float32, align_corners=False, **kw):
    """the seeded restatement of the case in eval mode (kw overrides constructor arguments: the parameters are drawn in the same order)"""
    B, C, nhead, ff, layers, L, max_len, resize, H, W = CASES[case]
    args = dict(d_model=C, nhead=nhead, dim_feedforward=ff, num_transformer=layers, max_len=max_len, resize_embed=resize, align_corners=align_corners)
    return seed_parameters(CostVolumeDisparityAttention(**{**args, **kw}), _generator(case)).to(dtype).eval()


def make_input(case, dtype=torch.float32):
    B, C, nhead, ff, layers, L, max_len, resize, H, W = CASES[case]
    g = _generator(case)
    g.manual_seed(g.initial_seed() + 1000)
    return torch.randn((B, C, L, H, W), generator=g).to(dtype)


def out_shape(case):
    B, C, nhead, ff, layers, L, max_len, resize, H, W = CASES[case]
    return (B, C, L, H, W)


def _assert_not_vacuous(case, mod, x):
    for layer in mod.sa:
        layer.stats, layer.self_attn.stats = [], []
    with torch.no_grad():
        y = mod(x)
    L = x.shape[2]
    for i, layer in enumerate(mod.sa):
        (top,), ((lo, hi),) = layer.self_attn.stats, layer.stats
        print(f"{case} layer {i}: largest probability {top:.3f} (1.5 / L = {1.5 / L:.3f}), pre-activations {lo:.1%} below -1, {hi:.1%} above +1")
        if case not in DEGENERATE:
            assert 1.5 / L <= top <= 0.9, f"{case} layer {i}: mean largest attention probability {top:.3f} outside [{1.5 / L:.3f}, 0.9]"
            assert lo >= 0.10 and hi >= 0.10, f"{case} layer {i}: {lo:.1%} of the feed-forward pre-activations below -1, {hi:.1%} above +1"
        layer.stats = layer.self_attn.stats = None
    return y


_cache = {}


def reference(case, dtype, align_corners=False):
    """-> the restatement's output in `dtype`, [B,C,L,H,W] contiguous; computed once per (case, dtype, align_corners) and not modified by the tests"""
    key = (case, dtype, align_corners)
    if key not in _cache:
        mod, x = make_module(case, dtype, align_corners), make_input(case, dtype)
        if dtype == torch.float64:
            _cache[key] = _assert_not_vacuous(case, mod, x).contiguous()
        else:
            with torch.no_grad():
                _cache[key] = mod(x).contiguous()
    return _cache[key]


def err(x, ref64):
    return float((x.detach().double().cpu() - ref64).abs().max())


def check(what, x, ref64, ref32):
    """the tolerance rule; both numbers in the message"""
    assert tuple(x.shape) == tuple(ref64.shape), f"{what}: shape {tuple(x.shape)}, expected {tuple(ref64.shape)}"
    e, e32 = err(x, ref64), err(ref32, ref64)
    print(f"{what}: err {e:.3e}, fp32 restatement {e32:.3e}")
    assert e <= FACTOR * e32, f"{what}: err {e:.3e} > {FACTOR:g} x {e32:.3e} (the fp32 restatement's error)"


def layer_params(mod):
    """the parameter list osa_native.disparity_attention_pack takes"""
    return [t for l in mod.sa for m in (l.self_attn.q_proj, l.self_attn.k_proj, l.self_attn.v_proj, l.self_attn.out_proj, l.linear1, l.linear2, l.norm1, l.norm2)
            for t in (m.weight, m.bias)]


class Entered:
    """counts how often an encoder layer sa[i] of `module` was entered: the torch composition ran"""

    def __init__(self, module):
        self.n = 0
        self.hooks = [l.register_forward_pre_hook(self._hit) for l in module.sa]
        assert self.hooks

    def _hit(self, *a):
        self.n += 1

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for h in self.hooks:
            h.remove()
