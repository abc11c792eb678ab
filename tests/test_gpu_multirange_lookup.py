"""GPU: IGEV++'s multi-range lookup (openstereo_amd/csrc/geometry.hip: geo_lookup_mr NCHW / channels-last forward, accumulating backward;
openstereo_amd.geometry.MultiRangeGeoEncodingVolume) against the float64 contract of tests/multirange_cases.py on the CPU, against the
single-pyramid kernels bit for bit, and against the real reference class's outputs (tests/golden/igevpp_geometry.npz).
tests/test_multirange_lookup_cpu.py proves without a GPU that the inputs reach the tap pairs whose x0 differ by 2 or by 0 in volumes 1
and 2 and that the reference's own float32 arithmetic stays inside half the tolerances used here.  No comparison skips or masks an
element; every output buffer is pre-filled (7.0) so that an unwritten element shows."""
import functools

import numpy as np
import pytest
import torch

import multirange_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = [(s, cv) for s in M.SETS for cv in M.COORDS]
case_param = pytest.mark.parametrize("case", list(M.CASES))
FILL = 7.0


def ext():
    from openstereo_amd import _ext
    return _ext.load()


@functools.lru_cache(maxsize=None)
def setup(case):
    """(reference, the float64 sources rounded once to float32 on the GPU, upstream gradients, disparities [B,H,W], coordinates [B,H,W]).
    Shared by every test of a case; nothing in it is written to."""
    ref = M.reference(case)
    B, C, D0, D1, D2, H, W, Cf, L, r = M.CASES[case]
    src = [t.float().contiguous().to(DEV) for t in ref.sources]
    disp = {s: d.reshape(B, H, W).contiguous().to(DEV) for s, d in ref.disp.items()}
    cx = {cv: M.coords(case, cv).reshape(B, H, W).contiguous().to(DEV) for cv in M.COORDS}
    return ref, src, [t.contiguous().to(DEV) for t in ref.douts], disp, cx


@functools.lru_cache(maxsize=None)
def volume(case):
    """the class on the inference path, built once per case"""
    from openstereo_amd.geometry import MultiRangeGeoEncodingVolume
    B, C, D0, D1, D2, H, W, Cf, L, r = M.CASES[case]
    with torch.no_grad():
        fn = MultiRangeGeoEncodingVolume(*[t.to(DEV) for t in M.reference(case).leaves], radius=r, num_levels=L)
    assert not fn.train_path
    return fn


def fwd_close(got, want, what):
    """the project's lookup tolerance (tests/test_gpu_geo_lookup_edges.py)"""
    torch.testing.assert_close(got.detach().cpu().double(), want.double(), rtol=1e-5, atol=2e-5, msg=lambda m: f"{what}: {m}")


def grad_close(got, want, what):
    """the project's gradient tolerance: rtol 1e-4, atol 1e-4 * max |reference|"""
    want = want.to(torch.float64)
    torch.testing.assert_close(got.detach().cpu().to(torch.float64), want, rtol=1e-4, atol=1e-4 * float(want.abs().max()), msg=lambda m: f"{what}: {m}")


def nchw(case, s, cv):
    ref, src, douts, disp, cx = setup(case)
    B, C, D0, D1, D2, H, W, Cf, L, r = M.CASES[case]
    outs = [torch.full((B, n, H, W), FILL, device=DEV) for n in M.channels(case)]
    ext().geo_lookup_mr(src, disp[s], cx[cv], outs, C, r)
    return outs


def acc_bwd(case, lookups, fill=0.0):
    ref, src, douts, disp, cx = setup(case)
    B, C, D0, D1, D2, H, W, Cf, L, r = M.CASES[case]
    acc = [torch.full_like(t, fill) for t in src]
    for s, cv in lookups:
        ext().geo_lookup_mr_bwd_acc(acc, disp[s], cx[cv], douts, C, r)
    return acc


# ----------------------------------------------------------------------------- forward
@case_param
def test_forward_nchw_and_channels_last_vs_float64(case):
    """geo_lookup_mr and geo_lookup_mr_nhwc directly on the rounded float64 sources, and MultiRangeGeoEncodingVolume.__call__ / lookup_cl on
    the pyramid the builders made: atol 2e-5 / rtol 1e-5 of the float64 contract, channels-last == NCHW bit for bit, padding channels
    exactly 0 (at the engine's stride and at an odd one), set (f) exactly 0"""
    ref, src, douts, disp, cx = setup(case)
    B, C, D0, D1, D2, H, W, Cf, L, r = M.CASES[case]
    counts = M.channels(case)
    fn = volume(case)
    names = ("geo_feat0", "geo_feat1", "geo_feat2", "init_corr")
    for s, cv in ALL:
        want = ref.out(s, cv)
        outs = nchw(case, s, cv)
        for o, w, name in zip(outs, want, names):
            fwd_close(o, w, f"{case} set {s} {cv} {name}")
        for strides in ([(n + 3) // 4 * 4 for n in counts], [n + 5 - q for q, n in enumerate(counts)]):
            cl = [torch.full((B, H, W, cs), FILL, device=DEV) for cs in strides]
            ext().geo_lookup_mr_nhwc(src, disp[s], cx[cv], cl, strides, [B, H, W], C, r)
            for t, o, n, name in zip(cl, outs, counts, names):
                assert torch.equal(t[..., :n].permute(0, 3, 1, 2), o), f"{case} set {s} {cv} {name}: channels-last != NCHW (strides {strides})"
                assert not t[..., n:].any(), f"{case} set {s} {cv} {name}: padding channels not zero (strides {strides})"
        d4, c4 = disp[s].reshape(B, 1, H, W), cx[cv].reshape(B, H, W, 1)
        o2 = fn(d4, c4)
        o3 = fn.lookup_cl(d4, c4)
        assert len(o2) == len(o3) == 4
        for a, b_, w, n, name, meta in zip(o2, o3, want, counts, names, fn.metas):
            assert a.dtype == torch.float32 and a.shape == (B, n, H, W)
            fwd_close(a, w, f"{case} set {s} {cv} {name} through the class")
            assert b_.shape == (B, (n + 3) // 4 * 4, 1, H, W) and b_._osa_meta is meta
            assert torch.equal(b_[:, :n, 0], a) and not b_[:, n:].any(), f"{case} set {s} {cv} {name}: lookup_cl"
        if s == "f":
            assert not any(bool(t.any()) for t in (*want, *outs, *o2))


@case_param
def test_forward_is_the_shipped_kernel_bit_for_bit(case):
    """geo_feat0 / init_corr == the de-interleaved output of geo_lookup on (volume 0, corr); geo_feat1 == the level-1 geometry block of
    geo_lookup on a fake 2-level pyramid whose level 1 is volume 1; geo_feat2 == the level-2 block of a fake 3-level pyramid: the new
    kernels do the arithmetic that is already golden-checked"""
    ref, src, douts, disp, cx = setup(case)
    B, C, D0, D1, D2, H, W, Cf, L, r = M.CASES[case]
    T = 2 * r + 1
    per = (C + 1) * T
    geo0, v1, v2, cor = src[:L], src[L], src[L + 1], src[L + 2:]

    def shipped(geo, corr, s, cv):
        n = len(geo)
        out = torch.full((B, per * n, H, W), FILL, device=DEV)
        ext().geo_lookup(list(geo) + list(corr), disp[s], cx[cv], out, C, r)
        return out.reshape(B, n, per, H, W)

    for s, cv in ALL:
        f0, f1, f2, ic = nchw(case, s, cv)
        o = shipped(geo0, cor, s, cv)
        assert torch.equal(f0, o[:, :, :C * T].reshape(B, L * C * T, H, W)), f"{case} set {s} {cv}: geo_feat0"
        assert torch.equal(ic, o[:, :, C * T:].reshape(B, L * T, H, W)), f"{case} set {s} {cv}: init_corr"
        o = shipped([geo0[0], v1], [cor[0], cor[1]], s, cv)
        assert torch.equal(f1, o[:, 1, :C * T]), f"{case} set {s} {cv}: geo_feat1"
        o = shipped([geo0[0], geo0[1], v2], [cor[0], cor[1], cor[1]], s, cv)
        assert torch.equal(f2, o[:, 2, :C * T]), f"{case} set {s} {cv}: geo_feat2"


@pytest.mark.parametrize("case", M.GOLDEN_CASES)
def test_class_vs_the_reference_class_outputs(case):
    """MultiRangeGeoEncodingVolume against what the real models/igevpp/geometry.py class gave on the same inputs, at the forward tolerance"""
    ref, src, douts, disp, cx = setup(case)
    B, C, D0, D1, D2, H, W, Cf, L, r = M.CASES[case]
    z = np.load(M.GOLDEN)
    fn = volume(case)
    for s in M.GOLDEN_SETS:
        outs = fn(disp[s].reshape(B, 1, H, W), cx["grid"].reshape(B, H, W, 1))
        for q, o in enumerate(outs):
            fwd_close(o[:1], torch.from_numpy(z[f"{case}__{s}__{q}"]), f"{case} set {s} output {q} vs the fixture")      # (batch element 0 is stored)


# ----------------------------------------------------------------------------- accumulating backward
@case_param
def test_accumulating_backward_vs_float64_autograd(case):
    """geo_lookup_mr_bwd_acc into zeros: every source's gradient within rtol 1e-4 / atol 1e-4 * max |ref| of float64 autograd.  Into
    accumulators pre-filled with 7.0: bit for bit 7.0 + the gradient into zeros (one float32 addition per entry) -- in particular the entries
    no tap comes within 1.001 of keep 7.0 exactly.  (A NaN pre-fill would show nothing here: NaN + v is NaN whether or not a lane touched
    the entry.)  Twice into zeros is exactly 2 x once.  What no pre-fill can show is a lane that adds an exact 0 to an entry out of reach: the
    value is the same; such a store would only show as a race, which the exact 2 x and the determinism of these comparisons would not catch."""
    ref = M.reference(case)
    for s, cv in ALL:
        once, filled, twice = acc_bwd(case, [(s, cv)]), acc_bwd(case, [(s, cv)], fill=FILL), acc_bwd(case, [(s, cv), (s, cv)])
        for q, (g, g7, g2, want, far) in enumerate(zip(once, filled, twice, ref.source_grads(s, cv), M.unreached(case, s, cv))):
            what = f"{case} set {s} {cv} source {q}"
            grad_close(g, want, what)
            assert torch.equal(g7, g + FILL), what + ": pre-filled accumulator != pre-fill + gradient"
            flat = g7.cpu().reshape(far.shape[0], -1, far.shape[1])               # [pixels, rows, n]
            assert bool((flat[far.unsqueeze(1).expand_as(flat)] == FILL).all()), what + ": an entry no tap reaches was changed"
            assert torch.equal(g2, g * 2), what + ": twice != 2 x once"
            if s == "f":
                assert not g.any() and not want.any()


@case_param
def test_accumulation_of_two_lookups(case):
    """sets (a) then (e) into the same accumulators: the sum of the two float64 gradients, at the gradient tolerance"""
    ref = M.reference(case)
    for cv in M.COORDS:
        got = acc_bwd(case, [("a", cv), ("e", cv)])
        for q, (g, wa, we) in enumerate(zip(got, ref.source_grads("a", cv), ref.source_grads("e", cv))):
            grad_close(g, wa + we, f"{case} {cv} source {q}: a then e")


# ----------------------------------------------------------------------------- the class in training
LOOKUPS = (("a", "grid"), ("e", "half"), ("b", "grid"))        # one pyramid, three lookups like three GRU iterations
LEAVES = ("geo_volume0", "geo_volume1", "geo_volume2", "init_fmap1", "init_fmap2")


def class_douts(case):
    B, C, D0, D1, D2, H, W, Cf, L, r = M.CASES[case]
    g = torch.Generator().manual_seed(4343)
    return [[torch.randn(B, n, H, W, generator=g) for n in M.channels(case)] for _ in LOOKUPS]


def class_run(case, used, autocast=False):
    """gradients of sum over the lookups in `used` of sum_q sum(out_q * w_q) w.r.t. the five inputs, and the outputs of every lookup"""
    from openstereo_amd.geometry import MultiRangeGeoEncodingVolume
    ref, src, douts, disp, cx = setup(case)
    B, C, D0, D1, D2, H, W, Cf, L, r = M.CASES[case]
    leaves = [t.clone().to(DEV).requires_grad_() for t in ref.leaves]
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        fn = MultiRangeGeoEncodingVolume(*leaves, radius=r, num_levels=L)
        assert fn.train_path
        outs = [fn(disp[s].reshape(B, 1, H, W), cx[cv].reshape(B, H, W, 1)) for s, cv in LOOKUPS]
    ws = class_douts(case)
    sum((o.float() * w.to(DEV)).sum() for i in used for o, w in zip(outs[i], ws[i])).backward()
    return [t.grad.clone() for t in leaves], outs


@case_param
def test_training_path_through_the_class(case):
    """three lookups of one pyramid, loss over all four outputs of each: gradients of the three volumes and the two feature maps against
    float64 autograd of the contract; a backward that reaches only the LAST lookup still delivers its gradients (_LevelJoin); under
    autocast(float16) the four outputs are float32 and unchanged"""
    ref = M.reference(case)
    ws = class_douts(case)
    got, outs = class_run(case, (0, 1, 2))
    for g, want, name in zip(got, ref.leaf_grads(LOOKUPS, ws), LEAVES):
        assert float(want.abs().max()) > 0
        grad_close(g, want, f"{case} {name}")
    for (s, cv), o4 in zip(LOOKUPS, outs):
        for o, want in zip(o4, ref.out(s, cv)):
            fwd_close(o, want, f"{case} set {s} {cv} (training path)")
    got, _ = class_run(case, (2,))
    for g, want, name in zip(got, ref.leaf_grads(LOOKUPS[2:], ws[2:]), LEAVES):
        assert float(want.abs().max()) > 0
        grad_close(g, want, f"{case} {name} (last lookup only)")
    got_ac, outs_ac = class_run(case, (0, 1, 2), autocast=True)
    for o4, a4 in zip(outs, outs_ac):
        for o, a in zip(o4, a4):
            assert a.dtype == torch.float32 and torch.equal(a, o), f"{case}: autocast changed an output"
    for g, want, name in zip(got_ac, ref.leaf_grads(LOOKUPS, ws), LEAVES):
        grad_close(g, want, f"{case} {name} (autocast)")


# ----------------------------------------------------------------------------- graph capture
def test_two_channels_last_lookups_in_one_captured_graph():
    """one torch.cuda.graph holds two lookup_cl calls with different disparities (single stream); two replays into overwritten outputs
    equal the eager results bit for bit: the source list travels in the kernel arguments, nothing is allocated or copied by the host call"""
    case = "odd"
    ref, src, douts, disp, cx = setup(case)
    B, C, D0, D1, D2, H, W, Cf, L, r = M.CASES[case]
    fn = volume(case)
    d1, d2, c4 = disp["a"].reshape(B, 1, H, W), disp["e"].reshape(B, 1, H, W), cx["grid"].reshape(B, H, W, 1)
    eager = [[t.clone() for t in fn.lookup_cl(d, c4)] for d in (d1, d2)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        held = [fn.lookup_cl(d1, c4), fn.lookup_cl(d2, c4)]
    for _ in range(2):
        for o4 in held:
            for t in o4:
                t.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        for o4, e4 in zip(held, eager):
            for t, e in zip(o4, e4):
                assert torch.equal(t, e)
