"""CPU: MobileStereoNet's fused 2-D inverted-residual block exists at every layer without a GPU -- C ABI 14 (declared, exported, in the ctypes
table, arguments validated before any launch), the `osa_native.mv2_block2d_pack` / `mv2_block2d` ops (Meta kernels: shape, dtype,
channels_last strides, their own shape errors), the golden fixture of the real reference block against the restatement of
tests/mv2_block2d_cases.py by the tolerance rule stated there, the restatement's epilogues, and the graft onto the reference's class
(training mode and CPU tensors keep the reference's composition)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mv2_block2d_cases as M
from test_abi_cpu import declared_symbols

NEW = ("osa_mv2_block2d_packed_floats", "osa_mv2_block2d_pack_f32", "osa_mv2_block2d_f32")


def test_new_symbols_declared_exported_and_in_the_ctypes_table(lib):
    from openstereo_amd import _lib
    names = declared_symbols()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for n in NEW:
        assert n in names, f"{n} is not declared in include/openstereo_amd.h"
        assert re.search(rf"\bT {n}\b", exported), f"{n} is not exported"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert lib.osa_abi_version() == _lib.abi_version() >= 14


# ----------------------------------------------------------------------------- argument validation
P = 16                                       # any non-NULL, 16-byte aligned "pointer": a failed check returns before it is touched
OK = dict(B=1, H=3, W=4, Ci=32, Ch=64, Co=32, stride=1, residual=0, relu=0)


def _run(lib, ptrs=(P,) * 4, **kw):
    a = {**OK, **kw}
    return lib.osa_mv2_block2d_f32(*ptrs, a["B"], a["H"], a["W"], a["Ci"], a["Ch"], a["Co"], a["stride"], a["residual"], a["relu"], None)


def _pack(lib, ptrs=(P,) * 10, **kw):
    a = {**OK, **kw}
    return lib.osa_mv2_block2d_pack_f32(*ptrs, a["Ci"], a["Ch"], a["Co"], None)


def test_argument_validation_happens_before_any_launch(lib):
    """every condition is reported (non-zero return, a message naming the limit) before anything is launched: nothing here is a device
    pointer.  The pointer order is (x, packed, addend, y); addend may be NULL."""
    err = lambda: lib.osa_last_error()
    for q in (0, 1, 3):
        assert _run(lib, ptrs=tuple(None if i == q else P for i in range(4))) != 0 and b"NULL pointer" in err(), q
    assert _run(lib, ptrs=(P, P, None, P), B=0) != 0 and b"bad dims" in err()                 # a NULL addend alone is no error: the next check speaks
    for q in range(10):
        assert _pack(lib, ptrs=tuple(None if i == q else P for i in range(10))) != 0 and b"NULL pointer" in err(), q
    for dim in ("B", "H", "W", "Ci", "Ch", "Co"):
        for bad in (0, -1):
            assert _run(lib, **{dim: bad}) != 0 and b"bad dims" in err(), (dim, bad)
    for dim in ("Ci", "Ch", "Co"):
        for bad in (0, -1):
            assert _pack(lib, **{dim: bad}) != 0 and b"bad dims" in err(), (dim, bad)
    for s in (0, 3, -1):
        assert _run(lib, stride=s) != 0 and f"stride {s} (supported: 1 and 2)".encode() in err()
    for call in (_run, _pack):
        assert call(lib, Ci=36) != 0 and b"channels 36 -> 64 -> 32 (supported: multiples of 8)" in err()
        assert call(lib, Ch=100) != 0 and b"supported: multiples of 8" in err()
        assert call(lib, Co=12) != 0 and b"supported: multiples of 8" in err()
        assert call(lib, Ci=200) != 0 and b"channels 200 -> 64 -> 32 (supported: input and output <= 192, hidden <= 384)" in err()
        assert call(lib, Co=200) != 0 and b"input and output <= 192, hidden <= 384" in err()
        assert call(lib, Ch=392) != 0 and b"input and output <= 192, hidden <= 384" in err()
    assert _run(lib, residual=1, stride=2) != 0 and b"residual needs stride 1 and equal channels, got stride 2 and 32 -> 32" in err()
    assert _run(lib, residual=1, Co=64) != 0 and b"residual needs stride 1 and equal channels, got stride 1 and 32 -> 64" in err()
    assert _run(lib, B=2, H=8192, W=4096, Ci=32) != 0 and b"2^31 elements or more" in err()            # x: exactly 2^31
    assert _run(lib, B=1, H=8192, W=4096, Ci=32, Co=64) != 0 and b"2^31 elements or more" in err()      # x: 2^30, y: 2^31
    assert _run(lib) != 0 and b"y overlaps x or addend" in err()                                      # x == y, still nothing launched
    assert _run(lib, ptrs=(P, P, 1 << 40, 1 << 40)) != 0 and b"y overlaps x or addend" in err()        # addend == y


def test_packed_floats():
    from openstereo_amd import _lib
    lib = _lib.load()
    assert lib.osa_mv2_block2d_packed_floats(48, 144, 48) == 144 * 48 + 2 * 144 + 9 * 144 + 2 * 144 + 48 * 144 + 2 * 48
    assert lib.osa_mv2_block2d_packed_floats(40, 120, 32) == 120 * (40 + 32 + 13) + 64
    assert lib.osa_mv2_block2d_packed_floats(48, 0, 48) == 0 and lib.osa_mv2_block2d_packed_floats(-8, 96, 48) == 0


# ----------------------------------------------------------------------------- extension ops
def test_meta_kernels_give_shape_dtype_and_channels_last_strides():
    from openstereo_amd import _ext, _lib
    ns = _ext.load()
    for name in ("mv2_block2d_pack", "mv2_block2d"):
        for key in ("Meta", "CUDA"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"osa_native::{name}", key), (name, key)
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"osa_native::{name}", "Autograd")     # an inference op
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)

    def packed(Ci, Ch, Co):
        pk = ns.mv2_block2d_pack(m(Ch, Ci, 1, 1), m(Ch, 1, 3, 3), m(Co, Ch, 1, 1), m(Ch), m(Ch), m(Ch), m(Ch), m(Co), m(Co))
        assert pk.dtype == torch.float32 and tuple(pk.shape) == (_lib.load().osa_mv2_block2d_packed_floats(Ci, Ch, Co),)
        return pk

    for (B, Ci, Ch, Co, stride, H, W), want in (((2, 48, 144, 48, 1, 11, 19), (2, 48, 11, 19)),
                                                ((1, 48, 96, 96, 2, 13, 21), (1, 96, 7, 11)),          # odd sizes
                                                ((1, 96, 192, 192, 2, 12, 20), (1, 192, 6, 10))):      # even sizes
        for x in (m(B, Ci, H, W), cl(m(B, Ci, H, W))):
            for addend in (None, m(*want), cl(m(*want))):
                for relu in (False, True):
                    y = ns.mv2_block2d(x, packed(Ci, Ch, Co), Ch, Co, stride, False, addend, relu)
                    assert y.dtype == torch.float32 and tuple(y.shape) == want
                    assert y.stride() == cl(torch.empty(want, device="meta")).stride()
    x, pk = m(1, 32, 5, 6), packed(32, 64, 32)
    with pytest.raises(RuntimeError, match=r"x must be \[B,Ci,H,W\]"):
        ns.mv2_block2d(m(32, 5, 6), pk, 64, 32, 1, False, None, False)
    with pytest.raises(RuntimeError, match=r"stride 3 \(supported: 1 and 2\)"):
        ns.mv2_block2d(x, pk, 64, 32, 3, False, None, False)
    with pytest.raises(RuntimeError, match="do not belong to channels 32 -> 64 -> 64"):
        ns.mv2_block2d(x, pk, 64, 64, 1, False, None, False)
    with pytest.raises(RuntimeError, match="residual needs stride 1 and equal channels"):
        ns.mv2_block2d(x, pk, 64, 32, 2, True, None, False)
    with pytest.raises(RuntimeError, match=r"addend has shape \[1, 32, 5, 5\], expected \[1, 32, 5, 6\]"):
        ns.mv2_block2d(x, pk, 64, 32, 1, True, m(1, 32, 5, 5), False)
    with pytest.raises(RuntimeError, match=r"\[Ch,Ci,1,1\], \[Ch,1,3,3\] and \[Co,Ch,1,1\]"):
        ns.mv2_block2d_pack(m(64, 32, 1, 1), m(64, 1, 3, 1), m(32, 64, 1, 1), m(64), m(64), m(64), m(64), m(32), m(32))
    with pytest.raises(RuntimeError, match=r"folded BatchNorm vector 4 has shape \[64\], expected \[32\]"):
        ns.mv2_block2d_pack(m(64, 32, 1, 1), m(64, 1, 3, 3), m(32, 64, 1, 1), m(64), m(64), m(64), m(64), m(64), m(32))


# ----------------------------------------------------------------------------- fixture and restatement
@pytest.mark.parametrize("case", M.GOLDEN_CASES)
def test_golden_fixture_satisfies_the_rule_against_the_restatement(case):
    """tests/golden/msnet2d_blocks.npz holds the REAL reference block's outputs (tests/golden/make_golden_msnet2d.py); by the rule, they
    are what the restatement of tests/mv2_block2d_cases.py computes on the regenerated parameters and inputs"""
    z = np.load(M.GOLDEN)
    assert sorted(z.files) == sorted(f"{c}__y" for c in M.GOLDEN_CASES)
    assert os.path.getsize(M.GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(M.GOLDEN), "igevpp_geometry.npz"))
    g = z[f"{case}__y"]
    assert g.dtype == np.float32 and g.any()
    M.check(f"{case} golden", torch.from_numpy(g), M.reference(case, torch.float64), M.reference(case, torch.float32))


def test_restatement_in_float32_is_close_to_but_not_equal_to_float64():
    """the figures the rule rests on are small and not zero: a wrong restatement in one of the two precisions would show here"""
    for case in M.CASES:
        r64, r32 = M.reference(case, torch.float64), M.reference(case, torch.float32)
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32 and tuple(r64.shape) == M.out_shape(case)
        assert 0 < M.err(r32, r64) <= 1e-5 * max(1.0, float(r64.abs().max())), case


def test_epilogues_of_the_restatement_change_the_result():
    """the addend and the ReLU of reference() are not vacuous on `dres`: each changes the result, and the ReLU has something to clip"""
    add = M.make_addend("dres", torch.float64)
    plain, summed = M.reference("dres", torch.float64), M.reference("dres", torch.float64, addend=add)
    assert torch.equal(summed, plain + add) and not torch.equal(summed, plain)
    assert torch.equal(plain, M.reference("dres", torch.float64)), "reference() modified its cached run"
    for pre in (plain, summed):
        assert float((pre < 0).double().mean()) >= 0.05, "fewer than 5 % of the values before the ReLU are negative"
    for kw in ({}, {"addend": add}):
        r = M.reference("dres", torch.float64, relu=True, **kw)
        assert float(r.min()) == 0.0 and not torch.equal(r, M.reference("dres", torch.float64, **kw))
    assert torch.equal(M.reference("dres", torch.float32, x=M.make_input("dres"), addend=add.float(), relu=True),
                       M.reference("dres", torch.float32, addend=add.float(), relu=True))


# ----------------------------------------------------------------------------- graft onto the reference's class
def _reference_class():
    from openstereo_amd import attach
    ref = os.environ.get("OPENSTEREO_REF", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "stereo", "modeling", "models", "msnet")):
        pytest.skip("the reference checkout is not importable here")
    attach.stub_reference_packages(ref)
    import importlib
    return importlib.import_module("stereo.modeling.models.msnet.submodule").MobileV2_Residual


def test_graft_keeps_the_reference_composition_in_training_mode_and_on_cpu_tensors():
    from openstereo_amd import attach
    from openstereo_amd.models.msnet import MobileV2Residual2D
    cls = _reference_class()
    orig = cls.__dict__["forward"]
    B, Ci, Co, stride, ratio, H, W = M.CASES["dres"]
    blk = cls(Ci, Co, stride, ratio)
    blk.load_state_dict(M.make_block("dres").state_dict())
    assert blk.use_res_connect
    x = M.make_input("dres")
    with torch.no_grad():
        want_eval = blk.eval()(x)
    torch.manual_seed(0)
    want_train = blk.train()(x).detach()
    blk.load_state_dict(M.make_block("dres").state_dict())                # the training forward moved the running statistics
    try:
        done = attach.patch_reference_modules()
        assert "stereo.modeling.models.msnet.submodule.MobileV2_Residual" in done
        assert cls.__dict__["forward"] is not orig and cls.reset_engine is MobileV2Residual2D.reset_engine
        with torch.no_grad():
            assert torch.equal(blk.eval()(x), want_eval)                    # CPU tensor: the block's own composition
        assert torch.equal(blk.train()(x).detach(), want_train)            # training mode: the reference's forward
    finally:
        attach.unpatch_reference()
    assert cls.__dict__["forward"] is orig and "reset_engine" not in cls.__dict__ and "_eng" not in cls.__dict__


def test_graft_plan_holds_both_block_classes_and_leaves_the_msnet2d_row_alone():
    from openstereo_amd import attach
    from openstereo_amd.models import msnet as MS
    plan = dict(attach._graft_plan())
    assert plan[attach.M + "msnet.submodule"] == {"MobileV2_Residual_3D": (MS.MobileV2Residual3D, ("forward", "reset_engine"), True),
                                                  "MobileV2_Residual": (MS.MobileV2Residual2D, ("forward", "reset_engine"), True)}
    assert plan[attach.M + "msnet.MSNet2D"] == {"MSNet2D": (MS.MSNet2D, ("forward", "reset_engine"), True)}
    assert sorted(n for n in MS.MSNet2D.__dict__ if not n.startswith("__")) == ["forward", "reset_engine"]


def test_the_function_runs_the_composition_with_the_epilogues_on_cpu_tensors():
    """mv2_block2d on an ungrafted restatement block and CPU tensors: the block's own composition, then + addend, then relu, bit for bit"""
    from openstereo_amd.models.msnet import mv2_block2d, mv2_sequential
    blk, x, add = M.make_block("dres"), M.make_input("dres"), M.make_addend("dres")
    with torch.no_grad():
        assert torch.equal(mv2_block2d(blk, x), M.reference("dres", torch.float32))
        assert torch.equal(mv2_block2d(blk, x, add, True), M.reference("dres", torch.float32, addend=add, relu=True))
        seq = torch.nn.Sequential(blk, torch.nn.ReLU(inplace=True), M.make_block("dres"))
        want = seq[2](torch.relu(blk(x))) + x
        assert torch.equal(mv2_sequential(seq, x, addend=x), want)
        seq = torch.nn.Sequential(blk, torch.nn.ReLU(inplace=True))       # a ReLU behind the last block: the sum is not its epilogue
        assert torch.equal(mv2_sequential(seq, x, addend=x), torch.relu(blk(x)) + x)
