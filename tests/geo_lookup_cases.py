"""Shared by tests/test_geo_lookup_positions_cpu.py and tests/test_gpu_geo_lookup_edges.py: the cases, the disparity sets, the float64
reference (oracle.torch_ref.GeoEncodingVolume on float64 inputs: F.grid_sample(align_corners=True), zero padding, torch autograd) and a
numpy float32 emulation of the kernels' tap_of() (openstereo_amd/csrc/geometry.hip).  No GPU needed by anything here."""
import functools

import numpy as np
import torch

# (B, C, D, H, W, Cf, levels, radius): the smallest shapes at which each kernel form and edge is reached
CASES = {
    # odd D and W pooled twice (13 -> 6 -> 3, 23 -> 11 -> 5); 138 pixels: no multiple of 4 or 256; 81 upstream gradients per (pixel, level):
    # two registers per lane of the rows backward; NHWC with 243 channels: one zero-filled padding channel
    "odd_3lv": (2, 8, 13, 3, 23, 16, 3, 4),
    # 4 levels; W = 70 > 64: the lane loop of the rows backward takes a second trip; odd feature count; W no multiple of 16 in allpairs_corr
    "wide_4lv": (1, 3, 24, 2, 70, 5, 4, 4),
    # (C + 1) * 9 = 252: all four registers of the readlane staging, the last one ragged
    "stage252": (1, 27, 12, 2, 19, 8, 2, 4),
    # (C + 1) * 9 = 288 > 256: the gather backward
    "gather288": (1, 31, 12, 2, 19, 8, 2, 4),
    # radius 5: generic NHWC kernel and gather backward
    "radius5": (2, 4, 12, 3, 21, 8, 2, 5),
    # one level, radius 1: generic NHWC kernel, rows backward with taps < 9.  First drafted with D = 9 / W = 17: n - 1 is a power of two
    # there, the position round trip is exact and tests/test_geo_lookup_positions_cpu.py found no equal-x0 tap pair in the geometry rows
    # and no anomalous pair at all in the correlation rows; D = 10 / W = 18 (n - 1 = 9 / 17) show both kinds in both.
    "radius1_1lv": (1, 2, 10, 2, 18, 8, 1, 1),
}
SETS = ("a", "b", "c", "d", "e", "f")
LATTICE_SETS = ("a", "b", "c", "d")        # the sets whose positions land on (or one ulp beside) integers
COORDS = ("grid", "half")


def inputs(case):
    """fp32 CPU tensors of a case: f1, f2 [B,Cf,H,W], volume [B,C,D,H,W], upstream gradient [B,(C+1)*(2r+1)*levels,H,W]."""
    B, C, D, H, W, Cf, L, r = CASES[case]
    g = torch.Generator().manual_seed(1000 + list(CASES).index(case))
    rn = lambda *s: torch.randn(*s, generator=g)
    # feature amplitude: correlation entries of standard deviation 0.4 at every Cf.  The float32 position round trip of the reference moves a
    # tap of a 70-long row by up to an ulp of 70 (7.6e-6), i.e. the sampled value by that times the difference of two neighbouring entries;
    # at this amplitude the reference's own float32 arithmetic stays within half the forward tolerance (asserted without a GPU in
    # tests/test_geo_lookup_positions_cpu.py), at standard deviation 0.56 it reached 0.54 of it.
    fs = (0.4 / Cf ** 0.5) ** 0.5
    return rn(B, Cf, H, W) * fs, rn(B, Cf, H, W) * fs, rn(B, C, D, H, W), rn(B, (C + 1) * (2 * r + 1) * L, H, W)


def spread(vals, n):
    """n entries of the list `vals`: all of it in order (cycled) when it fits, else an even subsample from its first to its last value"""
    vals = np.asarray(vals, np.float32)
    m = len(vals)
    idx = np.arange(n) % m if n >= m else np.round(np.arange(n) * (m - 1) / (n - 1)).astype(np.int64)
    return vals[idx]


def disparity_sets(case):
    """name -> float32 [B,1,H,W].  No NaN / inf anywhere."""
    B, C, D, H, W, Cf, L, r = CASES[case]
    n = B * H * W
    ints = np.arange(-2, D + 3, dtype=np.float32)
    near = np.empty(2 * len(ints), np.float32)
    near[0::2] = np.nextafter(ints, np.float32(-np.inf))
    near[1::2] = np.nextafter(ints, np.float32(np.inf))
    rng = np.random.default_rng(77 + list(CASES).index(case))
    sets = {
        "a": spread(np.arange(-3, D + 3.5, 0.25), n),                  # quarter-pixel lattice -3, -2.75, ... past D + 3
        "b": spread(ints, n),                                          # integers over [-2, D + 2]
        "c": np.zeros(n, np.float32),
        "d": spread(near, n),                                          # one ulp below / above those integers
        "e": np.abs(rng.normal(0, 1, n)).astype(np.float32) * np.float32(5),
        "f": np.full(n, 1e4, np.float32),                              # every tap out of range
    }
    for v in sets.values():
        assert v.dtype == np.float32 and np.isfinite(v).all()
    return {k: torch.from_numpy(v.copy()).reshape(B, 1, H, W) for k, v in sets.items()}


def coords(case, variant):
    B, C, D, H, W, Cf, L, r = CASES[case]
    c = torch.arange(W).float().reshape(1, 1, W, 1).repeat(B, H, 1, 1)
    return c + 0.5 if variant == "half" else c


# ----------------------------------------------------------------------------- float64 reference
class Reference:
    """The oracle's composition on float64 copies of a case's inputs.  `levels` are the pyramid's level tensors ([B*H*W,C,1,Dl] /
    [B*H*W,1,1,Wl]); out(set, coords) is the lookup and level_grads(set, coords) torch autograd's gradient of sum(out * dout) w.r.t. every
    level on its own (the levels detached from each other, as the kernels see them).  Everything is computed once and kept."""

    def __init__(self, case, dtype=torch.float64):
        from oracle import torch_ref as O
        self.case, self.dtype = case, dtype
        B, C, D, H, W, Cf, L, r = CASES[case]
        self.f1, self.f2, self.gv, self.dout = inputs(case)
        self.disp = disparity_sets(case)
        self.vol = O.GeoEncodingVolume(self.f1.to(dtype), self.f2.to(dtype), self.gv.to(dtype), num_levels=L, radius=r)
        self.levels = [t.detach().clone() for t in self.vol.geo + self.vol.corr]
        self._cache = {}

    def rows(self):
        """the pyramid in the kernels' layout: geo levels [B,H,W,C,Dl], then corr levels [B,H,W,Wl]"""
        B, C, D, H, W, Cf, L, r = CASES[self.case]
        return [t.reshape(B, H, W, C, -1) for t in self.levels[:L]] + [t.reshape(B, H, W, -1) for t in self.levels[L:]]

    def _run(self, s, cv):
        if (s, cv) not in self._cache:
            from oracle import torch_ref as O
            B, C, D, H, W, Cf, L, r = CASES[self.case]
            leaves = [t.clone().requires_grad_() for t in self.levels]
            vol = O.GeoEncodingVolume.__new__(O.GeoEncodingVolume)
            vol.num_levels, vol.radius, vol.geo, vol.corr = L, r, leaves[:L], leaves[L:]
            out = vol(self.disp[s].to(self.dtype), coords(self.case, cv).to(self.dtype))
            grads = torch.autograd.grad((out * self.dout).sum(), leaves)
            grads = [g.reshape(B, H, W, C, -1) for g in grads[:L]] + [g.reshape(B, H, W, -1) for g in grads[L:]]
            self._cache[(s, cv)] = (out.detach(), grads)
        return self._cache[(s, cv)]

    def out(self, s, cv):
        return self._run(s, cv)[0]

    def level_grads(self, s, cv):
        return self._run(s, cv)[1]

    def leaf_grads(self, lookups, douts):
        """gradients of sum_i sum(lookup_i * dout_i) w.r.t. fmap1, fmap2, geo_volume (one pyramid, len(lookups) lookups like GRU iterations)"""
        from oracle import torch_ref as O
        B, C, D, H, W, Cf, L, r = CASES[self.case]
        leaves = [t.to(self.dtype).requires_grad_() for t in (self.f1, self.f2, self.gv)]
        vol = O.GeoEncodingVolume(*leaves, num_levels=L, radius=r)
        loss = sum((vol(self.disp[s].to(self.dtype), coords(self.case, cv).to(self.dtype)) * w).sum() for (s, cv), w in zip(lookups, douts))
        return list(torch.autograd.grad(loss, leaves))


@functools.lru_cache(maxsize=None)
def reference(case, dtype=torch.float64):
    return Reference(case, dtype)


# ----------------------------------------------------------------------------- tap_of() in numpy float32
def tap_x0(x, n):
    """x0 of the kernels' tap_of(x, n) with every operation rounded to float32 and no fma (the library is built -ffp-contract=off)"""
    f = np.float32
    x = np.asarray(x, f)
    nm1 = f(n - 1)
    g = (f(2) * x) / nm1 - f(1)
    ix = ((g + f(1)) / f(2)) * nm1
    assert ix.dtype == np.float32
    return np.floor(ix).astype(np.int64)


def tap_positions(case, s, cv):
    """per level: (float32 tap positions of the geometry rows [pixels, taps], of the correlation rows, Dl, Wl) with the kernels' operand
    order: dx + d * scale and (cx * scale - d * scale) + dx"""
    B, C, D, H, W, Cf, L, r = CASES[case]
    f = np.float32
    d = disparity_sets(case)[s].numpy().reshape(-1, 1).astype(f)
    cx = coords(case, cv).numpy().reshape(-1, 1).astype(f)
    dx = np.arange(-r, r + 1, dtype=f).reshape(1, -1)
    out, Dl, Wl = [], D, W
    for l in range(L):
        scale = f(0.5 ** l)
        out.append((dx + d * scale, (cx * scale - d * scale) + dx, Dl, Wl))
        Dl, Wl = Dl // 2, Wl // 2
    return out


def count_anomalies(x, n):
    """Adjacent taps (k, k + 1) of one row whose x0 differ by 2 ("gap": position x0(k) + 1 is reached by tap k alone) or by 0 ("same": both
    taps reach x0(k) and x0(k) + 1).  Only pairs whose affected position lies inside the row [0, n) count: outside it nothing is stored."""
    x0 = tap_x0(x, n)
    step = x0[:, 1:] - x0[:, :-1]
    lo = x0[:, :-1]
    gap = (step == 2) & (lo + 1 >= 0) & (lo + 1 < n)
    same = (step == 0) & (lo + 1 >= 0) & (lo < n)
    other = (step < 0) | (step > 2)
    return int(gap.sum()), int(same.sum()), int(other.sum())


def unreached(case, s, cv):
    """per level tensor (geo levels then corr levels): boolean [pixels, n], True where no tap comes within 1.001 of the position -- whatever
    the rounding of a tap's position, it has no weight there, so a gradient must be exactly 0"""
    geo, cor = [], []
    for xg, xc, Dl, Wl in tap_positions(case, s, cv):
        for x, n, dst in ((xg, Dl, geo), (xc, Wl, cor)):
            j = np.arange(n, dtype=np.float64).reshape(1, 1, n)
            dst.append(torch.from_numpy((np.abs(x.astype(np.float64)[:, :, None] - j) > 1.001).all(1)))
    return geo + cor
