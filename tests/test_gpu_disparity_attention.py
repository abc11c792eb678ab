"""GPU: FoundationStereo's disparity transformer as one launch (csrc/disparity_attention.hip; osa_native.disparity_attention;
models/foundationstereo.py grafted onto the restatement of tests/disparity_attention_cases.py) by the tolerance rule stated there: every
case in both memory formats with bit-equal results, the C ABI against the extension op, bit-reproducibility, the goldens of the real
reference class, the cases in which the torch composition runs instead, the reference's own RuntimeError, and a fake trace."""
import functools

import numpy as np
import pytest
import torch

import disparity_attention_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def grafted():
    """the mirror's forward on the restatement's class, as attach._graft_plan() puts it on the reference's"""
    from openstereo_amd import attach
    from openstereo_amd.models.foundationstereo import CostVolumeDisparityAttention
    attach._graft(M.CostVolumeDisparityAttention, CostVolumeDisparityAttention, ("forward", "reset_engine"), True)
    yield
    attach.unpatch_reference()


@functools.lru_cache(maxsize=None)
def gpu_module(case, align_corners=False):
    return M.make_module(case, align_corners=align_corners).to(DEV)


def cl(x):
    return x.contiguous(memory_format=torch.channels_last_3d)


def fused(mod, x):
    """eval, no grad: the fused launch, proven by no sa[i] being entered"""
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


@pytest.mark.parametrize("case", ["fs416", "heads8", "many"])
def test_two_runs_and_the_c_abi_agree_bit_for_bit(case, lib):
    from openstereo_amd import _ext, _lib
    ns, mod = _ext.load(), gpu_module(case)
    B, C, nhead, ff, layers, L, max_len, resize, H, W = M.CASES[case]
    x = M.make_input(case).to(DEV)
    assert torch.equal(fused(mod, x), run(case))                                       # a second run
    pk = ns.disparity_attention_pack(M.layer_params(mod), nhead)
    with torch.no_grad():
        pe = mod.pos_embed0(x.new_zeros(1, L, C), resize_embed=resize).contiguous()
    assert tuple(pk.shape) == (lib.osa_disparity_attention_packed_floats(C, nhead, ff, layers),)
    assert torch.equal(ns.disparity_attention(x, pe, pk, C, nhead, ff, layers), run(case))
    for layout, xin in ((0, x), (1, x.permute(0, 2, 3, 4, 1).contiguous())):
        out = torch.full_like(xin, float("nan"))
        torch.cuda.synchronize()
        _lib.call("osa_disparity_attention_f32", xin.data_ptr(), pe.data_ptr(), pk.data_ptr(), out.data_ptr(), layout, B, C, L, H, W, nhead, ff, layers, None)
        torch.cuda.synchronize()
        assert torch.equal(out if layout == 0 else out.permute(0, 4, 1, 2, 3), run(case)), f"C ABI, layout {layout}"


def test_goldens_of_the_real_reference_class():
    z = np.load(M.GOLDEN)
    for case in M.GOLDEN_CASES:
        M.check(f"{case} with the golden as the fp32 figure", run(case), M.reference(case, torch.float64), torch.from_numpy(z[f"{case}__y"]))
    # the fast copy's resize rule (align_corners=True) comes from the module's own pos_embed0
    y = fused(gpu_module("resize", True), M.make_input("resize").to(DEV))
    M.check("resize, fast copy", y, M.reference("resize", torch.float64, True), M.reference("resize", torch.float32, True))
    assert not torch.equal(y, run("resize"))


def test_the_torch_composition_runs_where_the_kernel_does_not_apply():
    mod, x = gpu_module("fs416"), M.make_input("fs416").to(DEV)
    layers = M.CASES["fs416"][4]

    def entered(m, t, **kw):
        with M.Entered(m) as e:
            y = m(t, **kw)
        assert y.shape == t.shape
        return e.n

    with torch.no_grad():
        assert entered(mod.train(), x) == layers                                        # training mode
        mod.eval()
        with torch.autocast("cuda", dtype=torch.float16):
            assert entered(mod, x) == layers                                            # autocast
        assert entered(M.make_module("fs416").half().to(DEV), x.half()) == layers       # fp16
        long = M.make_module("fs416", max_len=33).to(DEV)
        assert entered(long, torch.randn(1, 28, 33, 1, 2, device=DEV)) == layers        # L = 33
        assert fused(long, torch.randn(1, 28, 32, 1, 2, device=DEV)).shape == (1, 28, 32, 1, 2)
        wide = M.make_module("fs416", d_model=36).to(DEV)
        assert entered(wide, torch.randn(1, 36, 5, 1, 2, device=DEV)) == layers         # C = 36
        with M.Entered(mod) as e, pytest.raises(NotImplementedError):                   # a window: the composition's own error, in its first layer
            mod(x, window_size=(3, 3))
        assert e.n == 1
        assert torch.equal(fused(mod, x), run("fs416"))
    assert all(q.requires_grad for q in mod.parameters()) and entered(mod, x) == layers  # parameters require gradients
    try:
        for q in mod.parameters():
            q.requires_grad_(False)
        assert entered(mod, x.clone().requires_grad_()) == layers                       # the input requires a gradient
        assert entered(mod, x) == 0                                                     # nothing does: the kernel, with or without no_grad
    finally:
        for q in mod.parameters():
            q.requires_grad_(True)


def test_sequence_longer_than_the_table_without_resize_raises():
    mod = gpu_module("fs416")
    with torch.no_grad(), pytest.raises(RuntimeError, match="pe:"):
        mod(torch.randn(1, 28, 27, 1, 2, device=DEV))


def test_reset_engine_and_parameter_updates_repack():
    mod, x = M.make_module("heads8").to(DEV), M.make_input("heads8").to(DEV)
    y = fused(mod, x)
    with torch.no_grad():
        mod.sa[0].norm2.bias.add_(1.0)
    y2 = fused(mod, x)
    assert float((y2 - y).abs().max()) > 0.5, "the packed parameters were not rebuilt after an in-place update"
    mod.reset_engine()
    assert torch.equal(fused(mod, x), y2)


def test_fake_trace_of_the_grafted_module_replays_equal():
    from torch.fx.experimental.proxy_tensor import make_fx
    mod, x = gpu_module("fs192"), M.make_input("fs192").to(DEV)
    with torch.no_grad():
        want = run("fs192")                                                             # eager: also packs (the trace must not)
        gm = make_fx(lambda t: mod(t), tracing_mode="fake", _allow_non_fake_inputs=True)(x)
        ours = [str(n.target) for n in gm.graph.nodes if n.op == "call_function" and str(n.target).startswith("osa_native.")]
        assert ours == ["osa_native.disparity_attention.default"], ours
        got = gm(x)
    assert torch.equal(got, want)
    assert torch.equal(fused(mod, x), want)                                             # the trace left the module usable
