"""Shared by tests/test_multirange_lookup_cpu.py and tests/test_gpu_multirange_lookup.py: the cases, the disparity sets, the float64
reference of IGEV++'s multi-range lookup (the contract written with F.grid_sample(align_corners=True), zero padding; gradients by torch
autograd) and the kernels' float32 tap positions per source.  `spread`, `tap_x0` and `count_anomalies` come from geo_lookup_cases.
No GPU needed by anything here.

A lookup has 2 L + 2 SOURCES, always in this order: the L levels of volume 0 (sampled at dx + disp / 2^l), volume 1 (dx + disp / 2),
volume 2 (dx + disp / 4), the L levels of the all-pairs correlation (coords / 2^l - disp / 2^l + dx); and four outputs: geo_feat0
[B, L*C*T, H, W] (channel l*C*T + c*T + k), geo_feat1 and geo_feat2 [B, C*T, H, W] (c*T + k), init_corr [B, L*T, H, W] (l*T + k), T = 2r + 1."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from geo_lookup_cases import count_anomalies, spread, tap_x0  # noqa: F401  (re-exported to the tests)

# (B, C, D0, D1, D2, H, W, Cf, L, r)
CASES = {
    # odd D0 pooled (13 -> 6), three different lengths, 138 pixels, channels-last paddings 144 / 72 / 72 / 18 -> 20
    "odd": (2, 8, 13, 10, 7, 3, 23, 16, 2, 4),
    # W > 64; channel counts 54 / 27 / 27 / 18: every output has padding
    "wide": (1, 3, 24, 12, 6, 2, 70, 5, 2, 4),
    # generic kernels
    "radius5": (2, 4, 12, 12, 12, 3, 21, 8, 2, 5),
    # taps < 9, n - 1 not a power of two
    "radius1": (1, 2, 10, 6, 5, 2, 18, 8, 2, 1),
    # three levels
    "deep": (1, 2, 24, 6, 5, 2, 19, 8, 3, 4),
}
SETS = ("a", "b", "c", "d", "e", "f")
LATTICE_SETS = ("a", "b", "c", "d")
COORDS = ("grid", "half")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "igevpp_geometry.npz")
GOLDEN_CASES, GOLDEN_SETS = ("odd", "radius1"), ("a", "d", "e")          # with `grid` coordinates
# The fixture keeps batch element 0 of every output only ([:1]; `odd` has B = 2): the whole of `odd` is 127k full-mantissa floats, 310 kB
# compressed, and the fixture is to stay below tests/golden/geo_encoding.npz (199 kB).  Batch element 0 holds the low half of each
# disparity set's sweep; the out-of-range end of the sweep is checked against the float64 contract, not against the fixture.


def channels(case):
    B, C, D0, D1, D2, H, W, Cf, L, r = CASES[case]
    T = 2 * r + 1
    return (L * C * T, C * T, C * T, L * T)


def inputs(case):
    """fp32 CPU tensors: geo_volume0/1/2 [B,C,Dk,H,W], init_fmap1/2 [B,Cf,H,W] (the reference's constructor order) and the upstream
    gradients of the four outputs."""
    B, C, D0, D1, D2, H, W, Cf, L, r = CASES[case]
    g = torch.Generator().manual_seed(2000 + list(CASES).index(case))
    rn = lambda *s: torch.randn(*s, generator=g)
    fs = (0.4 / Cf ** 0.5) ** 0.5             # correlation entries of standard deviation 0.4 (see geo_lookup_cases.inputs)
    vols = [rn(B, C, D, H, W) for D in (D0, D1, D2)]
    f1, f2 = rn(B, Cf, H, W) * fs, rn(B, Cf, H, W) * fs
    return (*vols, f1, f2), [rn(B, n, H, W) for n in channels(case)]


def disparity_sets(case):
    """name -> float32 [B,1,H,W]: the sets of geo_lookup_cases.disparity_sets over [-3, max(D0, 2 D1, 4 D2) + 3], so that disp / 2 and
    disp / 4 also land on, one ulp beside and outside the lattices of volumes 1 and 2.  No NaN / inf anywhere."""
    B, C, D0, D1, D2, H, W, Cf, L, r = CASES[case]
    n, M = B * H * W, max(D0, 2 * D1, 4 * D2)
    ints = np.arange(-2, M + 3, dtype=np.float32)
    near = np.empty(2 * len(ints), np.float32)
    near[0::2] = np.nextafter(ints, np.float32(-np.inf))
    near[1::2] = np.nextafter(ints, np.float32(np.inf))
    rng = np.random.default_rng(177 + list(CASES).index(case))
    sets = {
        "a": spread(np.arange(-3, M + 3.5, 0.25), n),
        "b": spread(ints, n),
        "c": np.zeros(n, np.float32),
        "d": spread(near, n),
        "e": np.abs(rng.normal(0, 1, n)).astype(np.float32) * np.float32(5),
        "f": np.full(n, 1e4, np.float32),                              # every tap out of range
    }
    for v in sets.values():
        assert v.dtype == np.float32 and np.isfinite(v).all()
    return {k: torch.from_numpy(v.copy()).reshape(B, 1, H, W) for k, v in sets.items()}


def coords(case, variant):
    B, C, D0, D1, D2, H, W, Cf, L, r = CASES[case]
    c = torch.arange(W).float().reshape(1, 1, W, 1).repeat(B, H, 1, 1)
    return c + 0.5 if variant == "half" else c


# ----------------------------------------------------------------------------- the contract in torch
def scales(L):
    """(scale, is_corr) of the 2 L + 2 sources"""
    return [(0.5 ** l, False) for l in range(L)] + [(0.5, False), (0.25, False)] + [(0.5 ** l, True) for l in range(L)]


def build_sources(v0, v1, v2, f1, f2, L):
    """the 2 L + 2 sources as rows ([B,H,W,C,n] / [B,H,W,n]) in the dtype of the inputs, differentiable"""
    rows = [v.permute(0, 3, 4, 1, 2) for v in (v0, v1, v2)]
    geo0, cor = [rows[0]], [torch.einsum("aijk,aijh->ajkh", f1, f2)]
    for _ in range(L - 1):
        for pyr in (geo0, cor):
            t = pyr[-1]
            m = t.shape[-1] // 2 * 2                                       # a trailing odd element is dropped
            pyr.append(F.avg_pool1d(t[..., :m].reshape(-1, 1, m), 2, 2).reshape(*t.shape[:-1], m // 2))
    return geo0 + [rows[1], rows[2]] + cor


def _sample(rows, x):
    """rows [N,R,1,n], x [N,1,T,1] (pixel positions) -> [N,R,1,T]: 1-D linear, zero padding"""
    n = rows.shape[-1]
    grid = torch.cat([2 * x / (n - 1) - 1, torch.zeros_like(x)], dim=-1)
    return F.grid_sample(rows, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def lookup(sources, disp, cx, L, r):
    """the four outputs of one lookup from the 2 L + 2 sources; disp [B,1,H,W], cx [B,H,W,1]; dtype of the sources"""
    dt = sources[0].dtype
    B, H, W = sources[0].shape[:3]
    N = B * H * W
    d, c = disp.to(dt).reshape(N, 1, 1, 1), cx.to(dt).reshape(N, 1, 1, 1)
    dx = torch.arange(-r, r + 1, dtype=dt, device=sources[0].device).reshape(1, 1, 2 * r + 1, 1)
    per = []
    for t, (scale, is_corr) in zip(sources, scales(L)):
        x = (c * scale - d * scale + dx) if is_corr else (dx + d * scale)
        per.append(_sample(t.reshape(N, -1, 1, t.shape[-1]), x).reshape(B, H, W, -1))
    cat = lambda ts: torch.cat(ts, dim=-1).permute(0, 3, 1, 2).contiguous()
    return cat(per[:L]), cat([per[L]]), cat([per[L + 1]]), cat(per[L + 2:])


class Reference:
    """The contract on copies of a case's inputs in `dtype`.  Everything is computed once and kept; nothing is written to."""

    def __init__(self, case, dtype=torch.float64):
        self.case, self.dtype = case, dtype
        B, C, D0, D1, D2, H, W, Cf, L, r = CASES[case]
        self.leaves, self.douts = inputs(case)
        self.disp = disparity_sets(case)
        with torch.no_grad():
            self.sources = [t.contiguous() for t in build_sources(*[t.to(dtype) for t in self.leaves], L)]
        self._cache = {}

    def _run(self, s, cv):
        if (s, cv) not in self._cache:
            B, C, D0, D1, D2, H, W, Cf, L, r = CASES[self.case]
            leaves = [t.clone().requires_grad_() for t in self.sources]
            outs = lookup(leaves, self.disp[s], coords(self.case, cv), L, r)
            grads = torch.autograd.grad(sum((o * w).sum() for o, w in zip(outs, self.douts)), leaves)
            self._cache[(s, cv)] = ([o.detach() for o in outs], list(grads))
        return self._cache[(s, cv)]

    def out(self, s, cv):
        """the four outputs"""
        return self._run(s, cv)[0]

    def source_grads(self, s, cv):
        """gradient of sum_i sum(out_i * dout_i) with respect to every source on its own (detached from each other, as the kernel sees them)"""
        return self._run(s, cv)[1]

    def leaf_grads(self, lookups, douts):
        """gradients of sum_i sum_q sum(out_q(lookup i) * douts[i][q]) w.r.t. geo_volume0/1/2, init_fmap1/2: one pyramid, len(lookups) lookups"""
        B, C, D0, D1, D2, H, W, Cf, L, r = CASES[self.case]
        leaves = [t.to(self.dtype).requires_grad_() for t in self.leaves]
        src = build_sources(*leaves, L)
        loss = 0
        for (s, cv), ws in zip(lookups, douts):
            loss = loss + sum((o * w).sum() for o, w in zip(lookup(src, self.disp[s], coords(self.case, cv), L, r), ws))
        return list(torch.autograd.grad(loss, leaves))


@functools.lru_cache(maxsize=None)
def reference(case, dtype=torch.float64):
    return Reference(case, dtype)


# ----------------------------------------------------------------------------- the kernels' tap positions
def tap_positions(case, s, cv):
    """per source: (float32 tap positions [pixels, taps] with the kernels' operand order -- dx + d * scale, (cx * scale - d * scale) + dx --,
    row length)"""
    B, C, D0, D1, D2, H, W, Cf, L, r = CASES[case]
    f = np.float32
    d = disparity_sets(case)[s].numpy().reshape(-1, 1).astype(f)
    cx = coords(case, cv).numpy().reshape(-1, 1).astype(f)
    dx = np.arange(-r, r + 1, dtype=f).reshape(1, -1)
    lens = [D0 >> l for l in range(L)] + [D1, D2] + [W >> l for l in range(L)]
    out = []
    for n, (scale, is_corr) in zip(lens, scales(L)):
        sc = f(scale)
        out.append(((cx * sc - d * sc) + dx if is_corr else dx + d * sc, n))
    return out


def unreached(case, s, cv):
    """per source: boolean [pixels, n], True where no tap comes within 1.001 of the position -- whatever the rounding of a tap's position, it
    has no weight there, so the lookup's backward must leave the entry alone"""
    out = []
    for x, n in tap_positions(case, s, cv):
        j = np.arange(n, dtype=np.float64).reshape(1, 1, n)
        out.append(torch.from_numpy((np.abs(x.astype(np.float64)[:, :, None] - j) > 1.001).all(1)))
    return out
