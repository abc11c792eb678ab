"""GPU: FoundationStereo's Conv3dNormActReduced as one launch (csrc/conv3d_reduced.hip; osa_native.conv3d_reduced;
models/foundationstereo.py grafted onto the restatement of tests/conv3d_reduced_cases.py) by the tolerance rule stated there: every case in
both memory formats with bit-equal results, the C ABI against the extension op, bit-reproducibility, independence of the batch size, the
goldens of the real reference class, the cases in which the torch composition runs instead, repacking, and a fake trace."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import conv3d_reduced_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def grafted():
    """the mirror's forward on the restatement's class, as attach._graft_plan(True) puts it on the reference's"""
    from openstereo_amd import attach
    from openstereo_amd.models.foundationstereo import Conv3dNormActReduced
    attach._graft(M.Conv3dNormActReduced, Conv3dNormActReduced, ("forward", "reset_engine"), True)
    yield
    attach.unpatch_reference()


def frozen(mod):
    """nothing requires a gradient: the fused launch is eligible with or without no_grad"""
    for q in mod.parameters():
        q.requires_grad_(False)
    return mod


@functools.lru_cache(maxsize=None)
def gpu_module(case):
    return M.make_module(case).to(DEV)


def cl(x):
    return x.contiguous(memory_format=torch.channels_last_3d)


def fused(mod, x):
    """eval, no grad: the fused launch, proven by conv1 not being entered"""
    with M.Entered(mod) as e, torch.no_grad():
        y = mod(x)
    assert e.n == 0, "the torch composition ran instead of the fused kernel"
    return y


@functools.lru_cache(maxsize=None)
def run(case, channels_last=False):
    x = M.make_input(case).to(DEV)
    return fused(gpu_module(case), cl(x) if channels_last else x)


@pytest.mark.parametrize("case", list(M.CASES))
def test_case_in_both_memory_formats(case):
    r64, r32 = M.reference(case, torch.float64), M.reference(case, torch.float32)
    y, ycl = run(case), run(case, True)
    assert y.is_contiguous() and ycl.shape == y.shape
    want = cl(torch.empty(y.shape)).stride()
    assert [s for s, n in zip(ycl.stride(), y.shape) if n > 1] == [s for s, n in zip(want, y.shape) if n > 1]
    M.check(f"{case} NCDHW", y, r64, r32)
    M.check(f"{case} channels-last", ycl, r64, r32)
    assert torch.equal(y, ycl), "the two memory formats differ"


@pytest.mark.parametrize("case", ["fs", "long", "many"])
def test_two_runs_and_the_c_abi_agree_bit_for_bit(case, lib):
    from openstereo_amd import _ext, _lib
    ns, mod = _ext.load(), gpu_module(case)
    B, Ci, Ch, Co, ks, kd, D, H, W = M.CASES[case]
    x = M.make_input(case).to(DEV)
    assert torch.equal(fused(mod, x), run(case))                                       # a second run
    with torch.no_grad():
        pk = ns.conv3d_reduced_pack(*M.pack_args(mod))
    assert tuple(pk.shape) == (lib.osa_conv3d_reduced_packed_floats(Ci, Ch, Co, ks, kd),)
    assert torch.equal(ns.conv3d_reduced(x, pk, Ch, Co, ks, kd), run(case))
    for layout, xin, shape in ((0, x, (B, Co, D, H, W)), (1, x.permute(0, 2, 3, 4, 1).contiguous(), (B, D, H, W, Co))):
        out = torch.full(shape, float("nan"), device=DEV)
        torch.cuda.synchronize()
        _lib.call("osa_conv3d_reduced_f32", xin.data_ptr(), pk.data_ptr(), out.data_ptr(), layout, B, D, H, W, Ci, Ch, Co, ks, kd, None)
        torch.cuda.synchronize()
        assert torch.equal(out if layout == 0 else out.permute(0, 4, 1, 2, 3), run(case)), f"C ABI, layout {layout}"


def test_a_pair_does_not_depend_on_the_batch():
    x = M.make_input("fs").to(DEV)
    assert torch.equal(fused(gpu_module("fs"), x[:1].contiguous()), run("fs")[:1])
    assert torch.equal(fused(gpu_module("fs"), cl(x[:1])), run("fs")[:1])


def test_goldens_of_the_real_reference_class():
    z = np.load(M.GOLDEN)
    for case in M.GOLDEN_CASES:
        M.check(f"{case} with the golden as the fp32 figure", run(case), M.reference(case, torch.float64), torch.from_numpy(z[f"{case}__y"]))


def test_the_torch_composition_runs_where_the_kernel_does_not_apply():
    mod, x = gpu_module("fs"), M.make_input("fs").to(DEV)

    def entered(m, t):
        with M.Entered(m) as e:
            m(t)
        return e.n

    with torch.no_grad():
        tr = M.make_module("fs").to(DEV)
        tr.conv1[1].momentum = tr.conv2[1].momentum = 0.0                               # (the training forward leaves the running statistics as they are)
        assert entered(tr.train(), x) == 1                                              # training mode
        assert torch.equal(fused(tr.eval(), x), run("fs"))                              # ... and the kernel again in eval mode
        with torch.autocast("cuda", dtype=torch.float16):
            assert entered(mod, x) == 1                                                 # autocast
        assert torch.equal(fused(mod, x), run("fs"))
        assert entered(M.make_module("fs").half().to(DEV), x.half()) == 1               # fp16
        for kw, shape in ((dict(hidden=36), (1, 28, 5, 3, 4)), (dict(kernel_disp=19), (1, 28, 5, 3, 4)), (dict(stride=2), (1, 28, 6, 4, 6)),
                          (dict(norm=nn.InstanceNorm3d), (1, 28, 5, 3, 4))):
            other = M.make_module("fs", **kw).to(DEV)
            assert entered(other, torch.randn(shape, device=DEV)) == 1, kw              # Ch = 36; kd = 19; stride 2; another norm
        assert fused(M.make_module("fs", hidden=32, kernel_disp=15).to(DEV), torch.randn(1, 28, 5, 3, 4, device=DEV)).shape == (1, 28, 5, 3, 4)
    assert all(q.requires_grad for q in mod.parameters()) and entered(mod, x) == 1      # parameters require gradients
    try:
        frozen(mod)
        assert entered(mod, x.clone().requires_grad_()) == 1                            # the input requires a gradient
        assert entered(mod, x) == 0                                                     # nothing does: the kernel, with or without no_grad
        assert torch.equal(mod(x), run("fs"))
    finally:
        for q in mod.parameters():
            q.requires_grad_(True)


def test_reset_engine_and_parameter_updates_repack():
    mod, x = M.make_module("plus1").to(DEV), M.make_input("plus1").to(DEV)
    y = fused(mod, x)
    with torch.no_grad():
        mod.conv2[1].running_mean.sub_(1.0)                                             # an in-place BatchNorm update
    y2 = fused(mod, x)
    assert float((y2 - y).abs().max()) > 0.25, "the packed parameters were not rebuilt after an in-place update"
    M.check("plus1 after the update", y2, *_updated_references())
    mod.reset_engine()
    assert torch.equal(fused(mod, x), y2)


def _updated_references():
    out = []
    for dt in (torch.float64, torch.float32):
        ref = M.make_module("plus1", dt)
        with torch.no_grad():
            ref.conv2[1].running_mean.sub_(1.0)
            out.append(ref(M.make_input("plus1", dt)))
    return out


def test_fake_trace_of_the_grafted_module_replays_equal():
    from torch.fx.experimental.proxy_tensor import make_fx
    mod, x = gpu_module("short"), M.make_input("short").to(DEV)
    with torch.no_grad():
        want = run("short")                                                             # eager: also packs (the trace must not)
        gm = make_fx(lambda t: mod(t), tracing_mode="fake", _allow_non_fake_inputs=True)(x)
        ours = [str(n.target) for n in gm.graph.nodes if n.op == "call_function" and str(n.target).startswith("osa_native.")]
        assert ours == ["osa_native.conv3d_reduced.default"], ours
        got = gm(x)
    assert torch.equal(got, want)
    assert torch.equal(fused(mod, x), want)                                             # the trace left the module usable
