"""GPU: the geometry-encoding lookup family of openstereo_amd/csrc/geometry.hip (forward NCHW / NHWC, dense and accumulating backward,
the inference-path pyramid builders) at lattice, one-ulp-off-lattice and out-of-range sampling positions, at every level count, at radii
1 / 4 / 5 and at the sizes where the host picks another kernel -- against oracle.torch_ref.GeoEncodingVolume on float64 inputs on the CPU
(F.grid_sample(align_corners=True), zero padding; gradients by torch autograd).  Cases, disparity sets and the reference live in
tests/geo_lookup_cases.py; tests/test_geo_lookup_positions_cpu.py proves without a GPU that these inputs reach tap pairs whose x0 differ
by 2 or by 0 (what the accumulating backward once dropped / raced on) and that the reference's own float32 arithmetic stays inside the
tolerances used here.  No comparison skips or masks an element."""
import functools

import pytest
import torch

import geo_lookup_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = [(s, cv) for s in K.SETS for cv in K.COORDS]
LATTICE = [(s, cv) for s in K.LATTICE_SETS for cv in K.COORDS]
case_param = pytest.mark.parametrize("case", list(K.CASES))


def ext():
    from openstereo_amd import _ext
    return _ext.load()


@functools.lru_cache(maxsize=None)
def setup(case):
    """(reference, float32 pyramid on the GPU in the kernels' layout: the float64 pyramid rounded once, upstream gradient, disparities [B,H,W],
    coordinates [B,H,W]).  Shared by every test of a case; nothing in it is written to."""
    ref = K.reference(case)
    B, C, D, H, W, Cf, L, r = K.CASES[case]
    levels = [t.float().contiguous().to(DEV) for t in ref.rows()]
    disp = {s: d.reshape(B, H, W).contiguous().to(DEV) for s, d in ref.disp.items()}
    cx = {cv: K.coords(case, cv).reshape(B, H, W).contiguous().to(DEV) for cv in K.COORDS}
    return ref, levels, ref.dout.contiguous().to(DEV), disp, cx


def grad_close(got, want, what):
    """the project's gradient tolerance (tests/test_gpu_autograd.py): rtol 1e-4, atol 1e-4 * max |reference|"""
    want = want.to(torch.float64)
    torch.testing.assert_close(got.detach().cpu().to(torch.float64), want, rtol=1e-4, atol=1e-4 * float(want.abs().max()), msg=lambda m: f"{what}: {m}")


def dense_bwd(case, s, cv, fill=None):
    ref, levels, dout, disp, cx = setup(case)
    B, C, D, H, W, Cf, L, r = K.CASES[case]
    grads = [torch.empty_like(t) if fill is None else torch.full_like(t, fill) for t in levels]
    ext().geo_lookup_bwd(grads, disp[s], cx[cv], dout, C, r)
    return grads


def acc_bwd(case, lookups, start=None):
    ref, levels, dout, disp, cx = setup(case)
    B, C, D, H, W, Cf, L, r = K.CASES[case]
    acc = [torch.zeros_like(t) for t in levels] if start is None else [t.clone() for t in start]
    for s, cv in lookups:
        ext().geo_lookup_bwd_acc(acc, disp[s], cx[cv], dout, C, r)
    return acc


# ----------------------------------------------------------------------------- pyramid builders (inference path)
@case_param
def test_pyramid_builders_vs_float64(case):
    """allpairs_corr, geo_rows, avgpool_rows, called directly and through CombinedGeoEncodingVolume (no grad), against the float64 pyramid.
    Bounds from the float32 format (u = 2^-24): geo_rows copies, so level 0 of the volume is the input bit for bit; a correlation entry is a
    Cf-term fma chain, |err| <= Cf * u * sum_i |a_i b_i| (entry by entry at level 0, its maximum below); every pooling step (a + b) * 0.5 adds at most
    u * (|a| + |b|) / 2 <= u * max |level 0| to the error it averages."""
    from openstereo_amd import ops
    from openstereo_amd.geometry import CombinedGeoEncodingVolume
    ref = K.reference(case)
    B, C, D, H, W, Cf, L, r = K.CASES[case]
    u = 2.0 ** -24
    f1, f2, gv = ref.f1.to(DEV), ref.f2.to(DEV), ref.gv.to(DEV)
    e = ext()
    corr = torch.full((B, H, W, W), 7.0, device=DEV)
    e.allpairs_corr(f1, f2, corr)
    rows = torch.full((B, H, W, C, D), 7.0, device=DEV)
    e.geo_rows(ops.to_cl(gv, pad_to=1), rows, C)
    geo, cor = [rows], [corr]
    for _ in range(L - 1):
        for pyr in (geo, cor):
            y = torch.full(pyr[-1].shape[:-1] + (pyr[-1].shape[-1] // 2,), 7.0, device=DEV)
            e.avgpool_rows(pyr[-1], y)
            pyr.append(y)
    want = ref.rows()
    assert [tuple(t.shape) for t in geo + cor] == [tuple(t.shape) for t in want]
    assert torch.equal(geo[0].cpu(), want[0].float()), "geo_rows is a permutation"
    e_corr = Cf * u * torch.einsum("aijk,aijh->ajkh", ref.f1.double().abs(), ref.f2.double().abs())
    assert bool(((cor[0].cpu().double() - want[L]).abs() <= e_corr).all()), f"{case}: allpairs_corr"
    for l in range(L):
        bg = l * u * float(want[0].abs().max())
        bc = float(e_corr.max()) + l * u * float(want[L].abs().max())
        eg = float((geo[l].cpu().double() - want[l]).abs().max())
        ec = float((cor[l].cpu().double() - want[L + l]).abs().max())
        print(f"{case} level {l}: geo err {eg:.2e} (bound {bg:.2e}), corr err {ec:.2e} (bound {bc:.2e})")
        assert eg <= bg and ec <= bc, (case, l, eg, bg, ec, bc)
    with torch.no_grad():
        fn = CombinedGeoEncodingVolume(f1, f2, gv, num_levels=L, radius=r)
    assert not fn.train_path
    for a, b_ in zip(fn.geo_volume_pyramid + fn.init_corr_pyramid, geo + cor):
        assert torch.equal(a, b_)


# ----------------------------------------------------------------------------- forward
@case_param
def test_forward_nchw_and_nhwc_vs_float64(case):
    """geo_lookup and geo_lookup_nhwc, directly on the rounded float64 pyramid and through CombinedGeoEncodingVolume.__call__ / lookup_cl
    on the pyramid the builders made: atol 2e-5 / rtol 1e-5 of the reference (the project's lookup tolerance), NHWC == NCHW bit for bit,
    padding channels exactly 0, set (f) exactly 0; the output buffers are pre-filled to show every element is written."""
    from openstereo_amd.geometry import CombinedGeoEncodingVolume
    ref, levels, dout, disp, cx = setup(case)
    B, C, D, H, W, Cf, L, r = K.CASES[case]
    nch = (C + 1) * (2 * r + 1) * L
    with torch.no_grad():
        fn = CombinedGeoEncodingVolume(ref.f1.to(DEV), ref.f2.to(DEV), ref.gv.to(DEV), num_levels=L, radius=r)
    for s, cv in ALL:
        want = ref.out(s, cv)
        out = torch.full((B, nch, H, W), 3.0, device=DEV)
        ext().geo_lookup(levels, disp[s], cx[cv], out, C, r)
        torch.testing.assert_close(out.cpu(), want, rtol=1e-5, atol=2e-5, msg=lambda m: f"{case} set {s} {cv} geo_lookup: {m}")
        for Cs in ((nch + 3) // 4 * 4, nch + 5):
            cl = torch.full((B, H, W, Cs), 3.0, device=DEV)
            ext().geo_lookup_nhwc(levels, disp[s], cx[cv], cl, Cs, [B, H, W], C, r)
            assert torch.equal(cl[..., :nch].permute(0, 3, 1, 2), out), f"{case} set {s} {cv}: NHWC != NCHW (channel stride {Cs})"
            assert not cl[..., nch:].any(), f"{case} set {s} {cv}: padding channels not zero (channel stride {Cs})"
        d4, c4 = disp[s].reshape(B, 1, H, W), cx[cv].reshape(B, H, W, 1)
        o2 = fn(d4, c4)
        torch.testing.assert_close(o2.cpu(), want, rtol=1e-5, atol=2e-5, msg=lambda m: f"{case} set {s} {cv} CombinedGeoEncodingVolume: {m}")
        o3 = fn.lookup_cl(d4, c4)
        assert o3.shape == (B, (nch + 3) // 4 * 4, 1, H, W)
        assert torch.equal(o3[:, :nch, 0], o2) and not o3[:, nch:].any(), f"{case} set {s} {cv}: lookup_cl"
        if s == "f":
            assert not want.any() and not out.any() and not o2.any()


# ----------------------------------------------------------------------------- dense backward
@case_param
def test_dense_backward_vs_float64_autograd(case):
    """geo_lookup_bwd (one wave per (pixel, level), or the gather form for radius > 4 / more than 256 upstream gradients per level) into
    garbage-filled buffers: every level gradient within rtol 1e-4 / atol 1e-4 * max |ref| of float64 autograd, and exactly 0 wherever no
    tap comes within reach of the position."""
    ref, levels, dout, disp, cx = setup(case)
    for s, cv in ALL:
        got = dense_bwd(case, s, cv, fill=1e30)
        again = dense_bwd(case, s, cv, fill=-3.0)
        for i, (g, g2, want, far) in enumerate(zip(got, again, ref.level_grads(s, cv), K.unreached(case, s, cv))):
            what = f"{case} set {s} {cv} level tensor {i}"
            assert torch.equal(g, g2), what + ": depends on what the buffer held"
            grad_close(g, want, what)
            flat = g.cpu().reshape(far.shape[0], -1, far.shape[1])           # [pixels, rows, n]
            assert not flat[far.unsqueeze(1).expand_as(flat)].any(), what + ": non-zero where no tap reaches"
            if s == "f":
                assert not g.any() and not want.any()


@case_param
def test_dense_backward_through_the_class(case):
    """CombinedGeoEncodingVolume in training with the dense backward: one pyramid, one lookup per (set, coordinates) like GRU iterations,
    gradients of fmap1, fmap2, geo_volume vs float64 autograd of the oracle."""
    got = class_grads(case, ALL, acc=False)
    for g, want, name in zip(got, class_reference(case, tuple(ALL)), ("fmap1", "fmap2", "geo_volume")):
        assert float(want.abs().max()) > 0
        grad_close(g, want, f"{case} {name}")


def class_douts(case, n):
    B, C, D, H, W, Cf, L, r = K.CASES[case]
    g = torch.Generator().manual_seed(4242)
    return [torch.randn(B, (C + 1) * (2 * r + 1) * L, H, W, generator=g) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def class_reference(case, lookups):
    return K.reference(case).leaf_grads(lookups, class_douts(case, len(lookups)))


def class_grads(case, lookups, acc):
    from openstereo_amd import geometry as G
    ref, levels, dout, disp, cx = setup(case)
    B, C, D, H, W, Cf, L, r = K.CASES[case]
    old, G.ACC_LOOKUP_BWD = G.ACC_LOOKUP_BWD, acc
    try:
        leaves = [t.clone().to(DEV).requires_grad_() for t in (ref.f1, ref.f2, ref.gv)]
        fn = G.CombinedGeoEncodingVolume(*leaves, num_levels=L, radius=r)
        assert fn.train_path and (fn._acc is not None) == acc
        outs = [fn(disp[s].reshape(B, 1, H, W), cx[cv].reshape(B, H, W, 1)) for s, cv in lookups]
        sum((o * w.to(DEV)).sum() for o, w in zip(outs, class_douts(case, len(lookups)))).backward()
        return [t.grad.clone() for t in leaves]
    finally:
        G.ACC_LOOKUP_BWD = old


# ----------------------------------------------------------------------------- accumulating backward
@case_param
def test_accumulating_backward_into_zeros(case):
    """geo_lookup_bwd_acc into zero-filled accumulators: within 2e-6 * max |dense| of the dense form (the bound of the existing acc-vs-dense
    test) and within the dense test's tolerance of float64 autograd."""
    ref = K.reference(case)
    for s, cv in ALL:
        for i, (a, d, want) in enumerate(zip(acc_bwd(case, [(s, cv)]), dense_bwd(case, s, cv), ref.level_grads(s, cv))):
            what = f"{case} set {s} {cv} level tensor {i}"
            err, m = float((a - d).abs().max()), float(d.abs().max())
            assert err <= 2e-6 * m, f"{what}: acc vs dense {err:.3e}, max |dense| {m:.3e}"
            grad_close(a, want, what)


@case_param
def test_accumulating_backward_into_zeros_is_the_dense_form_bit_for_bit(case):
    """the accumulating kernel adds the taps that land on a position in ascending tap order into 0, as the dense kernels do"""
    for s, cv in ALL:
        for i, (a, d) in enumerate(zip(acc_bwd(case, [(s, cv)]), dense_bwd(case, s, cv))):
            assert torch.equal(a, d), f"{case} set {s} {cv} level tensor {i}: {int((a != d).sum())} of {a.numel()} entries differ"


@case_param
def test_accumulation_adds_to_what_is_there(case):
    """accumulators pre-filled with N(0,1), two calls with two different disparity sets: pre-fill + dense 1 + dense 2, to 2e-6 * max |expected|
    (two float32 additions per entry round by at most 2 * 2^-24 of the running magnitude)"""
    ref, levels, dout, disp, cx = setup(case)
    g = torch.Generator().manual_seed(99)
    start = [torch.randn(t.shape, generator=g).to(DEV) for t in levels]
    for pair in ((("a", "grid"), ("b", "grid")), (("c", "half"), ("d", "grid")), (("e", "grid"), ("f", "half")), (("d", "half"), ("a", "half"))):
        got = acc_bwd(case, pair, start=start)
        dense = [dense_bwd(case, s, cv) for s, cv in pair]
        for i, (a, p, d1, d2) in enumerate(zip(got, start, *dense)):
            want = p.double() + d1.double() + d2.double()
            err, m = float((a.double() - want).abs().max()), float(want.abs().max())
            assert err <= 2e-6 * m, f"{case} {pair} level tensor {i}: {err:.3e}, max |expected| {m:.3e}"


@case_param
def test_backward_forms_are_deterministic_on_lattice_positions(case):
    """three runs of each backward form on sets (a)-(d) are torch.equal; for the accumulating form (into a non-zero pre-fill, two lookups)
    this is the check that no two threads update one address"""
    ref, levels, dout, disp, cx = setup(case)
    g = torch.Generator().manual_seed(98)
    start = [torch.randn(t.shape, generator=g).to(DEV) for t in levels]
    for s, cv in LATTICE:
        first_d, first_a = dense_bwd(case, s, cv), acc_bwd(case, [(s, cv), (s, "half" if cv == "grid" else "grid")], start=start)
        for _ in range(2):
            assert all(torch.equal(x, y) for x, y in zip(dense_bwd(case, s, cv), first_d)), f"{case} set {s} {cv}: dense"
            again = acc_bwd(case, [(s, cv), (s, "half" if cv == "grid" else "grid")], start=start)
            assert all(torch.equal(x, y) for x, y in zip(again, first_a)), f"{case} set {s} {cv}: accumulating"


# ----------------------------------------------------------------------------- model level
@case_param
def test_training_volume_with_both_backward_forms(case):
    """CombinedGeoEncodingVolume in training mode, ACC_LOOKUP_BWD both ways, three lookups (sets a, b, e) of one pyramid: the gradients of
    fmap1, fmap2 and geo_volume against float64 autograd, and the accumulating form within 2e-6 * max |dense| of the dense one."""
    lookups = (("a", "grid"), ("b", "half"), ("e", "grid"))
    want = class_reference(case, lookups)
    dense, acc = class_grads(case, lookups, acc=False), class_grads(case, lookups, acc=True)
    for d, a, w, name in zip(dense, acc, want, ("fmap1", "fmap2", "geo_volume")):
        assert float(w.abs().max()) > 0
        grad_close(d, w, f"{case} {name} (dense)")
        grad_close(a, w, f"{case} {name} (accumulating)")
        err, m = float((a - d).abs().max()), float(d.abs().max())
        assert err <= 2e-6 * m, f"{case} {name}: acc vs dense {err:.3e}, max |dense| {m:.3e}"
