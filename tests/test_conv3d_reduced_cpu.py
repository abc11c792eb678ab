"""CPU: FoundationStereo's fused Conv3dNormActReduced exists at every layer without a GPU -- C ABI 18 (declared, exported, in the ctypes table
with the right arity, the size query, arguments validated before any launch), the `osa_native.conv3d_reduced_pack` / `conv3d_reduced` ops
(Meta kernels: the input's memory format, their own shape errors), the golden fixture of the real reference class against the restatement
of tests/conv3d_reduced_cases.py by the tolerance rule stated there, the non-vacuity of every case, and the rows of the graft plan."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import conv3d_reduced_cases as M
from test_abi_cpu import declared_symbols

NEW = {"osa_conv3d_reduced_packed_floats": 5, "osa_conv3d_reduced_pack_f32": 15, "osa_conv3d_reduced_f32": 14}


def test_new_symbols_declared_exported_and_in_the_ctypes_table(lib):
    from openstereo_amd import _lib
    names = declared_symbols()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for n, arity in NEW.items():
        assert n in names, f"{n} is not declared in include/openstereo_amd.h"
        assert re.search(rf"\bT {n}\b", exported), f"{n} is not exported"
        assert len(_lib.SIGNATURES[n][1]) == arity and hasattr(lib, n)
    assert lib.osa_abi_version() == _lib.abi_version() >= 18


def test_packed_floats_is_the_documented_formula_and_monotone(lib):
    """(ks * ks + kd) * 1024 + 128: every tap a 32 x 32 matrix, four vectors of 32; 0 outside the range"""
    f = lib.osa_conv3d_reduced_packed_floats
    assert f(28, 28, 28, 3, 17) == 26 * 1024 + 128 == 26752
    chans, kss, kds = range(4, 33, 4), (1, 3), range(1, 18, 2)
    for ks in kss:
        for kd in kds:
            vals = [f(c, 28, 28, ks, kd) for c in chans] + [f(28, c, 28, ks, kd) for c in chans] + [f(28, 28, c, ks, kd) for c in chans]
            assert set(vals) == {(ks * ks + kd) * 1024 + 128}, (ks, kd)             # the channels are padded to 32: constant, hence monotone, in each
    assert [f(8, 20, 12, 1, kd) for kd in kds] == sorted(f(8, 20, 12, 1, kd) for kd in kds) and f(8, 20, 12, 1, 1) < f(8, 20, 12, 3, 1)
    for bad in ((36, 28, 28, 3, 17), (28, 36, 28, 3, 17), (28, 28, 36, 3, 17), (30, 28, 28, 3, 17), (28, 28, 26, 3, 17), (0, 28, 28, 3, 17), (28, -4, 28, 3, 17),
                (28, 28, 28, 2, 17), (28, 28, 28, 5, 17), (28, 28, 28, 0, 17), (28, 28, 28, 3, 19), (28, 28, 28, 3, 16), (28, 28, 28, 3, 0), (28, 28, 28, 3, -1)):
        assert f(*bad) == 0, bad


# ----------------------------------------------------------------------------- argument validation
P = 16                                       # any non-NULL, 16-byte aligned "pointer": a failed check returns before it is touched
OK = dict(layout=0, B=1, D=20, H=5, W=9, Ci=28, Ch=28, Co=28, ks=3, kd=17)


def _run(lib, ptrs=(P, P, 1 << 40), **kw):
    a = {**OK, **kw}
    return lib.osa_conv3d_reduced_f32(*ptrs, a["layout"], a["B"], a["D"], a["H"], a["W"], a["Ci"], a["Ch"], a["Co"], a["ks"], a["kd"], None)


def _pack(lib, ptrs=(P,) * 9, **kw):
    a = {**OK, **kw}
    return lib.osa_conv3d_reduced_pack_f32(*ptrs, a["Ci"], a["Ch"], a["Co"], a["ks"], a["kd"], None)


def test_argument_validation_happens_before_any_launch(lib):
    """every condition is reported (non-zero return, a message naming the limit) before anything is launched: nothing here is a device pointer"""
    err = lambda: lib.osa_last_error()
    for q in range(3):
        assert _run(lib, ptrs=tuple(None if i == q else p for i, p in enumerate((P, P, 1 << 40)))) != 0 and b"NULL pointer" in err(), q
    for q in range(9):
        assert _pack(lib, ptrs=tuple(None if i == q else P for i in range(9))) != 0 and b"NULL pointer" in err(), q
    for dim in ("B", "D", "H", "W"):
        for bad in (0, -1):
            assert _run(lib, **{dim: bad}) != 0 and b"bad dims" in err(), (dim, bad)
    assert _run(lib, layout=2) != 0 and b"layout 2" in err()
    for call in (_run, _pack):
        assert call(lib, Ch=36) != 0 and b"channels 28 -> 36 -> 28, kernels (1,3,3) and (17,1,1) (supported: channels multiples of 4 up to 32, ks 1 or 3, kd odd up to 17)" in err()
        for kw in (dict(Ci=36), dict(Co=36), dict(Ci=30), dict(Co=0), dict(ks=2), dict(ks=5), dict(kd=19), dict(kd=4), dict(kd=0)):
            assert call(lib, **kw) != 0 and b"(supported: channels multiples of 4" in err(), kw
    assert _run(lib, ptrs=(P, P, P)) != 0 and b"y overlaps x" in err()
    assert _run(lib, ptrs=(P, P + 4, 1 << 40)) != 0 and b"16-byte aligned" in err()
    assert _run(lib, ptrs=(P + 4, P, 1 << 40), layout=1) != 0 and b"16-byte aligned" in err()
    assert _run(lib, ptrs=(P, P, 1 << 60), B=1 << 15, D=1, H=1 << 15, W=1 << 15) != 0 and b"workgroups" in err()       # 2^38 tiles


# ----------------------------------------------------------------------------- extension ops
def _meta_params(Ci, Ch, Co, ks, kd):
    m = lambda *s: torch.empty(*s, device="meta")
    return [m(Ch, Ci, 1, ks, ks), m(Ch), m(Ch), m(Ch), m(Co, Ch, kd, 1, 1), m(Co), m(Co), m(Co)]


def test_meta_kernels_give_the_inputs_memory_format(lib):
    from openstereo_amd import _ext
    ns = _ext.load()
    for name in ("conv3d_reduced_pack", "conv3d_reduced"):
        for key in ("Meta", "CUDA"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"osa_native::{name}", key), (name, key)
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"osa_native::{name}", "Autograd")     # an inference op
    m = lambda *s: torch.empty(*s, device="meta")
    for case, (B, Ci, Ch, Co, ks, kd, D, H, W) in M.CASES.items():
        pk = ns.conv3d_reduced_pack(*_meta_params(Ci, Ch, Co, ks, kd))
        assert pk.dtype == torch.float32 and tuple(pk.shape) == (lib.osa_conv3d_reduced_packed_floats(Ci, Ch, Co, ks, kd),)
        for x in (m(B, Ci, D, H, W), m(B, Ci, D, H, W).contiguous(memory_format=torch.channels_last_3d), m(B, H, W, D, Ci).permute(0, 4, 3, 1, 2)):
            y = ns.conv3d_reduced(x, pk, Ch, Co, ks, kd)
            assert y.dtype == torch.float32 and tuple(y.shape) == M.out_shape(case)
            if not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last_3d):
                assert y.is_contiguous(memory_format=torch.channels_last_3d)
            else:
                assert y.is_contiguous()
    pk, x = ns.conv3d_reduced_pack(*_meta_params(28, 28, 28, 3, 17)), m(1, 28, 20, 5, 9)
    with pytest.raises(RuntimeError, match=r"x must be \[B,Ci,D,H,W\]"):
        ns.conv3d_reduced(m(28, 20, 5, 9), pk, 28, 28, 3, 17)
    with pytest.raises(RuntimeError, match=r"channels 28 -> 36 -> 28"):
        ns.conv3d_reduced(x, pk, 36, 28, 3, 17)
    with pytest.raises(RuntimeError, match="do not belong to this configuration"):
        ns.conv3d_reduced(x, pk, 28, 28, 3, 5)
    with pytest.raises(RuntimeError, match="x is empty"):
        ns.conv3d_reduced(m(1, 28, 0, 5, 9), pk, 28, 28, 3, 17)
    with pytest.raises(RuntimeError, match=r"kernels \(1,3,3\) and \(19,1,1\)"):
        ns.conv3d_reduced_pack(*_meta_params(28, 28, 28, 3, 19))
    bad = _meta_params(28, 28, 28, 3, 17)
    bad[0] = m(28, 28, 3, 3, 3)
    with pytest.raises(RuntimeError, match=r"weights must be \[Ch,Ci,1,ks,ks\] and \[Co,Ch,kd,1,1\]"):
        ns.conv3d_reduced_pack(*bad)
    bad = _meta_params(28, 28, 28, 3, 17)
    bad[6] = m(24)
    with pytest.raises(RuntimeError, match=r"vector 4 of \(b1, scale1, shift1, b2, scale2, shift2\) has shape \[24\], expected \[28\]"):
        ns.conv3d_reduced_pack(*bad)


# ----------------------------------------------------------------------------- fixture and restatement
def test_golden_fixture_satisfies_the_rule_against_the_restatement():
    """tests/golden/conv3d_reduced.npz holds the REAL reference class's outputs (tests/golden/make_golden_conv3d_reduced.py); by the rule they
    are what the restatement computes on the regenerated parameters and inputs"""
    z = np.load(M.GOLDEN)
    assert sorted(z.files) == sorted(["keys"] + [f"{c}__y" for c in M.GOLDEN_CASES])
    assert os.path.getsize(M.GOLDEN) <= 512 * 1024
    for case in M.GOLDEN_CASES:
        g = z[f"{case}__y"]
        assert g.dtype == np.float32 and g.any() and (g == 0).any()
        M.check(f"{case} golden", torch.from_numpy(g), M.reference(case, torch.float64), M.reference(case, torch.float32))


def test_state_dict_keys_are_the_references():
    assert list(M.make_module("fs").state_dict()) == [str(k) for k in np.load(M.GOLDEN)["keys"]]


def test_every_case_is_not_vacuous_and_float32_is_close_to_but_not_equal_to_float64():
    """reference() asserts the non-vacuity bounds on the float64 run; the figures the rule rests on are small and not zero"""
    for case in M.CASES:
        r64, r32 = M.reference(case, torch.float64), M.reference(case, torch.float32)
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32 and tuple(r64.shape) == M.out_shape(case)
        assert 0 < M.err(r32, r64) <= 1e-5 * max(1.0, float(r64.abs().max())), case


def test_wrong_disparity_padding_would_fail_the_rule():
    """the trap the cases are seeded for: hidden planes outside [0, D) taken as relu(t1) instead of zero are far outside the tolerance"""
    for case in ("fs", "short", "d1"):
        mod, x = M.make_module(case), M.make_input(case)
        pad = mod.conv2[0].padding[0]
        with torch.no_grad():
            h = mod.conv1(torch.nn.functional.pad(x, (0, 0, 0, 0, pad, pad)))           # zero input planes: relu(t1) plus the spatial sum of nothing
            c2 = mod.conv2[0]
            wrong = mod.conv2[2](mod.conv2[1](torch.nn.functional.conv3d(h, c2.weight, c2.bias)))
        r64, r32 = M.reference(case, torch.float64), M.reference(case, torch.float32)
        assert wrong.shape == r32.shape and M.err(wrong, r64) > 1000 * M.FACTOR * M.err(r32, r64), case


# ----------------------------------------------------------------------------- graft
def test_graft_plan_lists_the_class_for_both_copies():
    from openstereo_amd import attach
    from openstereo_amd.models import foundationstereo as FS
    rows = attach._graft_plan(True)
    assert rows[:len(attach._graft_plan())] == attach._graft_plan() and len(rows) == len(attach._graft_plan()) + 2
    for copy in ("foundationstereo", "fast_foundationstereo"):
        mine = [classes for mod, classes in rows if mod == attach.M + copy + ".core.submodule"]
        assert mine == [{"CostVolumeDisparityAttention": (FS.CostVolumeDisparityAttention, ("forward", "reset_engine"), True)},
                        {"Conv3dNormActReduced": (FS.Conv3dNormActReduced, ("forward", "reset_engine"), True)}]
    assert sorted(n for n in FS.Conv3dNormActReduced.__dict__ if not n.startswith("__")) == ["forward"] and callable(FS.Conv3dNormActReduced.reset_engine)


def test_grafted_restatement_keeps_its_composition_on_cpu_tensors_and_in_training_mode():
    from openstereo_amd import attach
    from openstereo_amd.models.foundationstereo import Conv3dNormActReduced as Mirror
    orig = M.Conv3dNormActReduced.__dict__["forward"]
    attach._graft(M.Conv3dNormActReduced, Mirror, ("forward", "reset_engine"), True)
    try:
        mod, x = M.make_module("plus1"), M.make_input("plus1")
        with M.Entered(mod) as e, torch.no_grad():
            assert torch.equal(mod(x), M.reference("plus1", torch.float32))          # a CPU tensor: the composition, bit for bit
        assert e.n == 1
        with M.Entered(mod) as e:
            mod.train()(x)
        assert e.n == 1
    finally:
        attach.unpatch_reference()
    assert M.Conv3dNormActReduced.__dict__["forward"] is orig and "_ref_forward" not in M.Conv3dNormActReduced.__dict__
