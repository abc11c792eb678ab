"""CPU: FoundationStereo's fused disparity transformer exists at every layer without a GPU -- C ABI 15 (declared, exported, in the ctypes
table, the size query, arguments validated before any launch), the `osa_native.disparity_attention_pack` / `disparity_attention` ops (Meta
kernels: the input's shape and strides in both memory formats, their own shape errors), the golden fixture of the real reference class against
the restatement of tests/disparity_attention_cases.py by the tolerance rule stated there, and the two rows of the graft plan."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import disparity_attention_cases as M
from test_abi_cpu import declared_symbols

NEW = ("osa_disparity_attention_packed_floats", "osa_disparity_attention_pack_f32", "osa_disparity_attention_f32")


def test_new_symbols_declared_exported_and_in_the_ctypes_table(lib):
    from openstereo_amd import _lib
    names = declared_symbols()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for n in NEW:
        assert n in names, f"{n} is not declared in include/openstereo_amd.h"
        assert re.search(rf"\bT {n}\b", exported), f"{n} is not exported"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert lib.osa_abi_version() == _lib.abi_version() >= 15


def test_packed_floats(lib):
    """layers * (6 * 1024 + 10 * 32): six matrices and ten vectors per layer, every one zero padded to 32"""
    assert lib.osa_disparity_attention_packed_floats(28, 4, 28, 4) == 4 * (6 * 1024 + 10 * 32)
    assert lib.osa_disparity_attention_packed_floats(24, 8, 16, 1) == 6 * 1024 + 10 * 32
    for bad in ((36, 4, 28, 4), (30, 2, 28, 4), (28, 5, 28, 4), (28, 4, 36, 4), (28, 4, 26, 4), (28, 4, 28, 9), (28, 4, 28, 0), (0, 4, 28, 4), (28, 0, 28, 4)):
        assert lib.osa_disparity_attention_packed_floats(*bad) == 0, bad


# ----------------------------------------------------------------------------- argument validation
P = 16                                       # any non-NULL, 16-byte aligned "pointer": a failed check returns before it is touched
OK = dict(layout=0, B=1, C=28, L=26, H=3, W=4, nhead=4, ff=28, layers=4)


def _run(lib, ptrs=(P, P, P, 1 << 40), **kw):
    a = {**OK, **kw}
    return lib.osa_disparity_attention_f32(*ptrs, a["layout"], a["B"], a["C"], a["L"], a["H"], a["W"], a["nhead"], a["ff"], a["layers"], None)


def _pack(lib, ptrs=(P,) * 8, **kw):
    a = {**OK, **kw}
    return lib.osa_disparity_attention_pack_f32(*ptrs, a["C"], a["nhead"], a["ff"], a["layers"], None)


def test_argument_validation_happens_before_any_launch(lib):
    """every condition is reported (non-zero return, a message naming the limit) before anything is launched: nothing here is a device pointer"""
    err = lambda: lib.osa_last_error()
    for q in range(4):
        assert _run(lib, ptrs=tuple(None if i == q else p for i, p in enumerate((P, P, P, 1 << 40)))) != 0 and b"NULL pointer" in err(), q
    for q in range(8):
        assert _pack(lib, ptrs=tuple(None if i == q else P for i in range(8))) != 0 and b"NULL pointer" in err(), q
    for dim in ("B", "H", "W"):
        for bad in (0, -1):
            assert _run(lib, **{dim: bad}) != 0 and b"bad dims" in err(), (dim, bad)
    assert _run(lib, layout=2) != 0 and b"layout 2" in err()
    for call in (_run, _pack):
        assert call(lib, C=36) != 0 and b"C 36, nhead 4, ff 28, layers 4 (supported: C and ff multiples of 4 up to 32" in err()
        assert call(lib, C=30, nhead=2) != 0 and b"C 30, nhead 2" in err()
        assert call(lib, nhead=5) != 0 and b"nhead a divisor of C" in err()
        assert call(lib, nhead=0) != 0 and b"nhead a divisor of C" in err()
        assert call(lib, ff=36) != 0 and b"ff 36" in err()
        assert call(lib, ff=26) != 0 and b"ff 26" in err()
        assert call(lib, layers=9) != 0 and b"layers 9 (supported" in err() and b"1 .. 8 layers" in err()
        assert call(lib, layers=0) != 0 and b"1 .. 8 layers" in err()
    assert _run(lib, L=33) != 0 and b"33 disparity planes (supported: 1 .. 32)" in err()
    assert _run(lib, L=0) != 0 and b"0 disparity planes (supported: 1 .. 32)" in err()
    assert _run(lib, ptrs=(P, P, P, P)) != 0 and b"out overlaps cv" in err()
    assert _run(lib, ptrs=(P, P + 4, P, 1 << 40)) != 0 and b"16-byte aligned" in err()
    assert _run(lib, ptrs=(P + 4, P, P, 1 << 40), layout=1) != 0 and b"16-byte aligned" in err()


# ----------------------------------------------------------------------------- extension ops
def _meta_params(C, ff, layers):
    m = lambda *s: torch.empty(*s, device="meta")
    return [t for _ in range(layers) for t in (m(C, C), m(C), m(C, C), m(C), m(C, C), m(C), m(C, C), m(C), m(ff, C), m(ff), m(C, ff), m(C), m(C), m(C), m(C), m(C))]


def test_meta_kernels_give_the_inputs_shape_and_strides_in_both_memory_formats(lib):
    from openstereo_amd import _ext
    ns = _ext.load()
    for name in ("disparity_attention_pack", "disparity_attention"):
        for key in ("Meta", "CUDA"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"osa_native::{name}", key), (name, key)
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"osa_native::{name}", "Autograd")     # an inference op
    m = lambda *s: torch.empty(*s, device="meta")
    for B, C, nhead, ff, layers, L, max_len, resize, H, W in M.CASES.values():
        pk = ns.disparity_attention_pack(_meta_params(C, ff, layers), nhead)
        assert pk.dtype == torch.float32 and tuple(pk.shape) == (lib.osa_disparity_attention_packed_floats(C, nhead, ff, layers),)
        for cv in (m(B, C, L, H, W), m(B, C, L, H, W).contiguous(memory_format=torch.channels_last_3d), m(B, H, W, L, C).permute(0, 4, 3, 1, 2)):
            y = ns.disparity_attention(cv, m(1, L, C), pk, C, nhead, ff, layers)
            assert y.dtype == torch.float32 and y.shape == cv.shape
            if cv.is_contiguous() or cv.is_contiguous(memory_format=torch.channels_last_3d):
                assert [s for s, n in zip(y.stride(), y.shape) if n > 1] == [s for s, n in zip(cv.stride(), cv.shape) if n > 1]    # (a plane count of 1 has no stride)
            else:
                assert y.is_contiguous()                    # the reference's own output view [B,H,W,L,C]: made contiguous
    pk, cv, pe = ns.disparity_attention_pack(_meta_params(28, 28, 4), 4), m(1, 28, 26, 2, 3), m(26, 28)
    with pytest.raises(RuntimeError, match=r"cv must be \[B,28,L,H,W\]"):
        ns.disparity_attention(m(1, 24, 26, 2, 3), pe, pk, 28, 4, 28, 4)
    with pytest.raises(RuntimeError, match="do not belong to d_model 28, 4 heads, feed-forward width 28, 2 layers"):
        ns.disparity_attention(cv, pe, pk, 28, 4, 28, 2)
    with pytest.raises(RuntimeError, match=r"pe must be \[26,28\]"):
        ns.disparity_attention(cv, m(25, 28), pk, 28, 4, 28, 4)
    with pytest.raises(RuntimeError, match="16 tensors per layer"):
        ns.disparity_attention_pack(_meta_params(28, 28, 1)[:15], 4)
    with pytest.raises(RuntimeError, match="d_model 36, 4 heads"):
        ns.disparity_attention_pack(_meta_params(36, 28, 1), 4)
    bad = _meta_params(28, 28, 2)
    bad[16 + 9] = m(24)
    with pytest.raises(RuntimeError, match=r"layer 1, module 4 has weight \[28, 28\] and bias \[24\]"):
        ns.disparity_attention_pack(bad, 4)


# ----------------------------------------------------------------------------- fixture and restatement
def test_golden_fixture_satisfies_the_rule_against_the_restatement():
    """tests/golden/disparity_attention.npz holds the REAL reference class's outputs (tests/golden/make_golden_disparity_attention.py); by the
    rule they are what the restatement computes on the regenerated parameters and inputs -- for `resize` with either copy's resize rule"""
    z = np.load(M.GOLDEN)
    assert sorted(z.files) == sorted(["keys", "resize__y_fast"] + [f"{c}__y" for c in M.GOLDEN_CASES])
    assert os.path.getsize(M.GOLDEN) <= 256 * 1024
    for case in M.GOLDEN_CASES:
        g = z[f"{case}__y"]
        assert g.dtype == np.float32 and g.any()
        M.check(f"{case} golden", torch.from_numpy(g), M.reference(case, torch.float64), M.reference(case, torch.float32))
    M.check("resize golden, fast copy", torch.from_numpy(z["resize__y_fast"]), M.reference("resize", torch.float64, True), M.reference("resize", torch.float32, True))
    assert M.err(torch.from_numpy(z["resize__y_fast"]), M.reference("resize", torch.float64)) > 100 * M.err(M.reference("resize", torch.float32), M.reference("resize", torch.float64))


def test_state_dict_keys_are_the_references():
    assert list(M.make_module("fs416").state_dict()) == [str(k) for k in np.load(M.GOLDEN)["keys"]]


def test_restatement_in_float32_is_close_to_but_not_equal_to_float64():
    """the figures the rule rests on are small and not zero; reference() asserts the non-vacuity bounds on the float64 run"""
    for case in M.CASES:
        r64, r32 = M.reference(case, torch.float64), M.reference(case, torch.float32)
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32 and tuple(r64.shape) == M.out_shape(case)
        assert 0 < M.err(r32, r64) <= 1e-5 * max(1.0, float(r64.abs().max())), case


# ----------------------------------------------------------------------------- graft
def test_graft_plan_holds_both_copies_and_leaves_the_other_rows_alone():
    from openstereo_amd import attach
    from openstereo_amd.models import foundationstereo as FS, msnet as MS
    rows = attach._graft_plan()
    plan = dict(rows)
    assert len(plan) == len(rows) == 20
    for copy in ("foundationstereo", "fast_foundationstereo"):
        assert plan[attach.M + copy + ".core.submodule"] == {"CostVolumeDisparityAttention": (FS.CostVolumeDisparityAttention, ("forward", "reset_engine"), True)}
    assert plan[attach.M + "msnet.MSNet2D"] == {"MSNet2D": (MS.MSNet2D, ("forward", "reset_engine"), True)}
    assert plan[attach.M + "igev.update"] == plan[attach.M + "stereobase.gru_blocks"] and sorted(plan[attach.M + "igev.update"]) == ["BasicMotionEncoder", "BasicMultiUpdateBlock", "ConvGRU", "DispHead"]
    assert sorted(n for n in FS.CostVolumeDisparityAttention.__dict__ if not n.startswith("__")) == ["forward"] and callable(FS.CostVolumeDisparityAttention.reset_engine)


def test_grafted_restatement_keeps_its_composition_on_cpu_tensors_and_in_training_mode():
    from openstereo_amd import attach
    from openstereo_amd.models.foundationstereo import CostVolumeDisparityAttention as Mirror
    orig = M.CostVolumeDisparityAttention.__dict__["forward"]
    attach._graft(M.CostVolumeDisparityAttention, Mirror, ("forward", "reset_engine"), True)
    try:
        mod, x = M.make_module("heads8"), M.make_input("heads8")
        with M.Entered(mod) as e, torch.no_grad():
            assert torch.equal(mod(x), M.reference("heads8", torch.float32))         # a CPU tensor: the composition, bit for bit
        assert e.n == 1
        with M.Entered(mod) as e:
            mod.train()(x)
        assert e.n == 1
    finally:
        attach.unpatch_reference()
    assert M.CostVolumeDisparityAttention.__dict__["forward"] is orig and "_ref_forward" not in M.CostVolumeDisparityAttention.__dict__
