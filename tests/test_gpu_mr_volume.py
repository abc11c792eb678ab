"""GPU: IGEV++'s multi-range cost volumes (csrc/mr_volume.h, volume.hip, backward.hip; osa_native.mr_volume; ops.build_multirange_volumes)
against the restatement of tests/mr_volume_cases.py by the tolerance rule stated there: V0 bit for bit against gwc_volume's planes, V1, V2
and the four gradients within 8 x the float32 restatement's own error against float64, per output."""
import functools

import numpy as np
import pytest
import torch

import mr_volume_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
case_param = pytest.mark.parametrize("case", list(M.CASES))
cl_param = pytest.mark.parametrize("cl", [False, True], ids=["ncdhw", "ndhwc"])


def ext():
    from openstereo_amd import _ext
    return _ext.load()


@functools.lru_cache(maxsize=None)
def gpu_inputs(case):
    return tuple(t.to(DEV) for t in M.inputs(case))


@functools.lru_cache(maxsize=None)
def gpu_out_grads(case):
    return tuple(t.to(DEV) for t in M.out_grads(case))


def run(case, cl=False, leaves=None):
    from openstereo_amd import ops
    B, C, H, W, D, S, Mr, k0, k1 = M.CASES[case]
    return ops.build_multirange_volumes(*(leaves or gpu_inputs(case)), D, S, Mr, channels_last=cl)


def grads(case, cl, use=(0, 1, 2)):
    leaves = [t.clone().requires_grad_() for t in gpu_inputs(case)]
    outs = run(case, cl, leaves)
    dv = gpu_out_grads(case)
    return torch.autograd.grad([outs[i] for i in use], leaves, [dv[i] for i in use])


# ----------------------------------------------------------------------------- forward
@case_param
@cl_param
def test_forward_v0_bitwise_v1_v2_by_the_rule(case, cl):
    B, C, H, W, D, S, Mr, k0, k1 = M.CASES[case]
    L, R, P0, P1 = gpu_inputs(case)
    with torch.no_grad():
        outs = run(case, cl)
        full = ext().gwc_volume(L, R, D, M.G)
    want_cl = torch.channels_last_3d if cl else torch.contiguous_format
    for o, n in zip(outs, (S, Mr // k0, D // k1)):
        assert o.dtype == torch.float32 and tuple(o.shape) == (B, 8, n, H, W)
        assert o.stride() == torch.empty(o.shape).contiguous(memory_format=want_cl).stride()
    assert torch.equal(outs[0], full[:, :, :S]), f"{case}: V0 differs from gwc_volume's first {S} planes"
    r64, r32 = M.reference(case, torch.float64)[0], M.reference(case, torch.float32)[0]
    for i in (1, 2):
        M.check(f"{case} {M.NAMES[i]}", outs[i], r64[i], r32[i])
    if case in M.GOLDEN_CASES:
        # the fixture and the engine each obey the rule against float64, so they are within twice its bound of each other
        z = np.load(M.GOLDEN)
        for i, name in enumerate(M.NAMES):
            g = torch.from_numpy(z[f"{case}__{name}"])
            diff, e32 = float((outs[i].cpu() - g).abs().max()), M.err(r32[i], r64[i])
            print(f"{case} {name} vs golden: {diff:.3e}, fp32 restatement {e32:.3e}")
            assert diff <= 2 * M.FACTOR * e32, f"{case} {name} vs golden: {diff:.3e} > 2 x {M.FACTOR:g} x {e32:.3e}"


# ----------------------------------------------------------------------------- backward
@case_param
@cl_param
def test_backward_by_the_rule(case, cl):
    got = grads(case, cl)
    g64, g32 = M.reference(case, torch.float64)[1], M.reference(case, torch.float32)[1]
    for name, g, a, b_ in zip(M.GRAD_NAMES, got, g64, g32):
        assert g.dtype == torch.float32
        M.check(f"{case} {name}", g, a, b_)


@pytest.mark.parametrize("case", ["small", "tile"])
def test_two_backward_runs_are_bit_equal(case):
    a, b_ = grads(case, False), grads(case, False)
    for name, x, y in zip(M.GRAD_NAMES, a, b_):
        assert torch.equal(x, y), f"{case} {name}"


@pytest.mark.parametrize("only", [0, 1, 2])
def test_gradients_with_one_output_used(only):
    """the other two output gradients are undefined (never materialised); against float64 autograd of the restatement with the same single
    output, by the rule"""
    case = "small"
    B, C, H, W, D, S, Mr, k0, k1 = M.CASES[case]
    got = grads(case, False, use=(only,))
    ref = {}
    for dt in (torch.float64, torch.float32):
        leaves = [t.clone().requires_grad_() for t in M.inputs(case, dt)]
        out = M.restatement(*leaves, D, S, Mr)[only]
        ref[dt] = torch.autograd.grad(out, leaves, M.out_grads(case, dt)[only], allow_unused=True)
    for name, g, a, b_ in zip(M.GRAD_NAMES, got, ref[torch.float64], ref[torch.float32]):
        if a is None:                        # a patch weight the used output does not depend on
            assert g is None or not g.any(), name
        else:
            M.check(f"{case} only {M.NAMES[only]} {name}", g, a, b_)


def test_fp16_inputs_under_autocast_give_fp32_volumes_and_fp16_gradients():
    case = "equal"
    leaves = [t.half().requires_grad_() for t in gpu_inputs(case)]
    with torch.autocast("cuda", dtype=torch.float16):
        outs = run(case, False, leaves)
    assert all(o.dtype == torch.float32 for o in outs)
    with torch.no_grad():
        want = run(case, False, [t.detach().float() for t in leaves])
    for o, w in zip(outs, want):
        assert torch.equal(o, w)                                     # widening is exact
    gs = torch.autograd.grad(outs, leaves, gpu_out_grads(case))
    assert all(g.dtype == torch.float16 and g.shape == t.shape and torch.isfinite(g).all() for g, t in zip(gs, leaves))


# ----------------------------------------------------------------------------- registration
def test_opcheck_on_k44():
    from torch.library import opcheck
    B, C, H, W, D, S, Mr, k0, k1 = M.CASES["k44"]
    for cl in (False, True):
        args = tuple(t.clone().requires_grad_() for t in gpu_inputs("k44")) + (D, S, Mr, cl)
        opcheck(ext().mr_volume.default, args, test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))


def test_make_fx_fake_trace_of_forward_and_backward():
    from torch.fx.experimental.proxy_tensor import make_fx
    B, C, H, W, D, S, Mr, k0, k1 = M.CASES["k44"]
    ns = ext()

    def f(l, r, p0, p1, d0, d1, d2):
        v = ns.mr_volume(l, r, p0, p1, D, S, Mr, False)
        return torch.autograd.grad(v, (l, r, p0, p1), (d0, d1, d2))

    args = [t.clone().requires_grad_() for t in gpu_inputs("k44")] + list(gpu_out_grads("k44"))
    gm = make_fx(f, tracing_mode="fake")(*args)
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert any("osa_native.mr_volume.default" in t for t in targets), targets
    assert any("osa_native.mr_volume_bwd.default" in t for t in targets), targets


# ----------------------------------------------------------------------------- downstream
def test_outputs_feed_the_multirange_lookup():
    """`small`: the engine's volumes and the restatement's, both scaled to unit range as the lookup's own inputs are (tests/
    multirange_cases.py draws them from N(0, 1)), through MultiRangeGeoEncodingVolume at the lookup's forward tolerance"""
    from openstereo_amd.geometry import MultiRangeGeoEncodingVolume
    case = "small"
    B, C, H, W, D, S, Mr, k0, k1 = M.CASES[case]
    L, R, P0, P1 = gpu_inputs(case)
    r64 = M.reference(case, torch.float64)[0]
    scale = [1.0 / float(v.std()) for v in r64]
    fs = (0.4 / C ** 0.5) ** 0.5
    g = torch.Generator().manual_seed(7)
    disp = (torch.rand(B, 1, H, W, generator=g) * (D + 4) - 2).to(DEV)
    cx = torch.arange(W).float().reshape(1, 1, W, 1).repeat(B, H, 1, 1).to(DEV)
    with torch.no_grad():
        mine = [v * s for v, s in zip(run(case), scale)]
        theirs = [(v * s).float().to(DEV) for v, s in zip(r64, scale)]
        a = MultiRangeGeoEncodingVolume(*mine, L * fs, R * fs, radius=4, num_levels=2)(disp, cx)
        b_ = MultiRangeGeoEncodingVolume(*theirs, L * fs, R * fs, radius=4, num_levels=2)(disp, cx)
    assert len(a) == len(b_) == 4
    for q, (x, y) in enumerate(zip(a, b_)):
        assert x.shape == y.shape and y.abs().max() > 0
        torch.testing.assert_close(x, y, rtol=1e-5, atol=2e-5, msg=lambda m: f"lookup output {q}: {m}")


@pytest.mark.parametrize("interval", [1, 2, 4])
def test_disparity_regression_with_interval(interval):
    """igevpp/submodule.py:147-151; the intervals are powers of two, so the scaling is exact: the bound is the soft-argmin ops' own 1e-5"""
    from openstereo_amd import ops
    maxdisp = 48
    g = torch.Generator().manual_seed(11 + interval)
    prob = torch.softmax(torch.randn(2, maxdisp // interval, 5, 23, generator=g), 1).to(DEV)
    got = ops.disparity_regression(prob, maxdisp, True, interval)
    values = torch.arange(0, maxdisp, interval, dtype=prob.dtype, device=DEV).view(1, maxdisp // interval, 1, 1)
    torch.testing.assert_close(got, torch.sum(prob * values, 1, keepdim=True), rtol=0, atol=1e-5)
