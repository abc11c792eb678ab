"""CPU: the fused interlaced cost volume exists at every layer without a GPU -- C ABI 13 (declared, exported, in the ctypes table, arguments
validated before any launch), the `osa_native.interlaced_volume_pack` / `interlaced_volume` ops (Meta kernels: shape, dtype, strides, their
own shape errors), the golden fixture of the real reference (InterlacedVolume and MSNet2D) against the restatements of
tests/interlaced_volume_cases.py by the tolerance rule stated there, and the graft onto the reference's MSNet2D class."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import interlaced_volume_cases as M
from test_abi_cpu import declared_symbols

NEW = ("osa_interlaced_volume_packed_floats", "osa_interlaced_volume_pack_f32", "osa_interlaced_volume_f32")


def test_new_symbols_declared_exported_and_in_the_ctypes_table(lib):
    from openstereo_amd import _lib
    names = declared_symbols()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for n in NEW:
        assert n in names, f"{n} is not declared in include/openstereo_amd.h"
        assert re.search(rf"\bT {n}\b", exported), f"{n} is not exported"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert lib.osa_abi_version() == _lib.abi_version() >= 13
    assert len(_lib.SIGNATURES["osa_interlaced_volume_pack_f32"][1]) == 18 and len(_lib.SIGNATURES["osa_interlaced_volume_f32"][1]) == 13


# ----------------------------------------------------------------------------- argument validation
P = 16                                       # any non-NULL, 16-byte aligned "pointer": a failed check returns before it is touched
OK = dict(B=1, C=32, H=3, W=4, D=5, k2=4, k3=2, F=1)


def _run(lib, ptrs=(P,) * 4, **kw):
    a = {**OK, **kw}
    return lib.osa_interlaced_volume_f32(*ptrs, a["B"], a["C"], a["H"], a["W"], a["D"], a["k2"], a["k3"], a["F"], None)


def _pack(lib, ptrs=(P,) * 13, **kw):
    a = {**OK, **kw}
    return lib.osa_interlaced_volume_pack_f32(*ptrs, a["C"], a["k2"], a["k3"], a["F"], None)


def test_argument_validation_happens_before_any_launch(lib):
    """every condition is reported (non-zero return, a message naming the limit) before anything is launched: nothing here is a device
    pointer"""
    err = lambda: lib.osa_last_error()
    for q in range(4):
        assert _run(lib, ptrs=tuple(None if i == q else P for i in range(4))) != 0 and b"NULL pointer" in err(), q
    for q in range(13):
        assert _pack(lib, ptrs=tuple(None if i == q else P for i in range(13))) != 0 and b"NULL pointer" in err(), q
    for dim in ("B", "C", "H", "W", "D"):
        for bad in (0, -1):
            assert _run(lib, **{dim: bad}) != 0 and b"bad dims" in err(), (dim, bad)
    for call in (_run, _pack):
        assert call(lib, C=64) != 0 and b"C = 64 with depth kernels (8, 4, 2) (supported: C = 32 with (8, 4, 2) and C = 96 with (8, 8, 3))" in err()
        assert call(lib, k2=8) != 0 and b"C = 32 with depth kernels (8, 8, 2)" in err()
        assert call(lib, C=96, k2=8, k3=2) != 0 and b"C = 96 with depth kernels (8, 8, 2)" in err()
        assert call(lib, k3=0) != 0 and b"supported: C = 32 with (8, 4, 2)" in err()
        for f in (0, 17, -1):
            assert call(lib, F=f) != 0 and f"{f} output features (supported: 1 .. 16)".encode() in err()
            assert call(lib, C=96, k2=8, k3=3, F=f) != 0 and b"output features (supported: 1 .. 16)" in err()
    assert _run(lib, B=64, C=32, H=1024, W=1024) != 0 and b"2^31 elements or more" in err()                  # a feature map: exactly 2^31
    assert _run(lib, B=1, C=96, H=1024, W=1024, D=128, k2=8, k3=3, F=16) != 0 and b"2^31 elements or more" in err()   # features 2^26.6, volume 2^31


def test_packed_floats(lib):
    assert lib.osa_interlaced_volume_packed_floats(32, 4, 2, 1) == 9 * 16 * 8 + 9 * 32 * 16 * 4 + 9 * 16 * 32 * 2 + 16 + 2 * (16 + 32 + 16 + 1)
    assert lib.osa_interlaced_volume_packed_floats(96, 8, 3, 8) == 9 * 16 * 8 + 9 * 32 * 16 * 8 + 9 * 16 * 32 * 3 + 16 * 8 + 2 * (16 + 32 + 16 + 8)
    assert lib.osa_interlaced_volume_packed_floats(96, 8, 3, 16) - lib.osa_interlaced_volume_packed_floats(96, 8, 3, 15) == 18
    for bad in ((32, 8, 3, 1), (96, 4, 2, 8), (0, 4, 2, 1), (32, 4, 2, 0), (32, 4, 2, 17), (96, 8, 3, -1)):
        assert lib.osa_interlaced_volume_packed_floats(*bad) == 0, bad


# ----------------------------------------------------------------------------- extension ops
def test_meta_kernels_give_shape_dtype_and_strides(lib):
    from openstereo_amd import _ext
    ns = _ext.load()
    for name in ("interlaced_volume_pack", "interlaced_volume"):
        for key in ("Meta", "CUDA"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"osa_native::{name}", key), (name, key)
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"osa_native::{name}", "Autograd")     # an inference op
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)

    def packed(k2, k3, Fo, k1=8):
        v = [m(n) for n in (16, 16, 32, 32, 16, 16, Fo, Fo)]
        pk = ns.interlaced_volume_pack(m(16, 1, k1, 3, 3), m(32, 16, k2, 3, 3), m(16, 32, k3, 3, 3), m(Fo, 16, 1, 1), *v)
        assert pk.dtype == torch.float32 and tuple(pk.shape) == (lib.osa_interlaced_volume_packed_floats(k1 * k2 * k3 // 2, k2, k3, Fo),)
        return pk

    for (C, k2, k3, Fo, B, H, W, D) in ((32, 4, 2, 1, 2, 7, 19, 6), (96, 8, 3, 8, 2, 7, 19, 6), (96, 8, 3, 3, 1, 5, 11, 4), (32, 4, 2, 1, 1, 3, 5, 8)):
        y = ns.interlaced_volume(m(B, C, H, W), m(B, C, H, W), packed(k2, k3, Fo), D, k2, k3, Fo)
        assert y.dtype == torch.float32 and tuple(y.shape) == (B, Fo, D, H, W) and y.is_contiguous()
        assert y.stride() == torch.empty(B, Fo, D, H, W, device="meta").stride()
    pk = packed(4, 2, 1)
    with pytest.raises(RuntimeError, match=r"features must be \[B,C,H,W\] of equal shape"):
        ns.interlaced_volume(m(1, 32, 4, 5), m(1, 32, 4, 6), pk, 3, 4, 2, 1)
    with pytest.raises(RuntimeError, match=r"64 channels with depth kernels \(8, 4, 2\)"):
        ns.interlaced_volume(m(1, 64, 4, 5), m(1, 64, 4, 5), pk, 3, 4, 2, 1)
    with pytest.raises(RuntimeError, match="17 features"):
        ns.interlaced_volume(m(1, 32, 4, 5), m(1, 32, 4, 5), pk, 3, 4, 2, 17)
    with pytest.raises(RuntimeError, match="do not belong to this configuration"):
        ns.interlaced_volume(m(1, 32, 4, 5), m(1, 32, 4, 5), pk, 3, 4, 2, 2)
    with pytest.raises(RuntimeError, match="maxdisp 0"):
        ns.interlaced_volume(m(1, 32, 4, 5), m(1, 32, 4, 5), pk, 0, 4, 2, 1)
    with pytest.raises(RuntimeError, match=r"depth kernels \(8, 4, 3\)"):
        packed(4, 3, 1)
    with pytest.raises(RuntimeError, match=r"depth kernels \(4, 4, 2\)"):
        packed(4, 2, 1, k1=4)
    with pytest.raises(RuntimeError, match=r"folded BatchNorm vector 6 has shape \[2\], expected \[1\]"):
        ns.interlaced_volume_pack(m(16, 1, 8, 3, 3), m(32, 16, 4, 3, 3), m(16, 32, 2, 3, 3), m(1, 16, 1, 1), m(16), m(16), m(32), m(32), m(16), m(16), m(2), m(1))


# ----------------------------------------------------------------------------- fixture and restatement
def _golden():
    z = np.load(M.GOLDEN)
    assert sorted(z.files) == sorted(M.GOLDEN_KEYS) and os.path.getsize(M.GOLDEN) <= 256 * 1024
    return {k: torch.from_numpy(z[k]) for k in z.files}


def test_golden_fixture_satisfies_the_rule_against_the_restatements():
    """tests/golden/interlaced_volume.npz holds the REAL reference's outputs (tests/golden/make_golden_interlaced_volume.py); by the rule
    they are what the restatements compute: InterlacedVolume on the regenerated inputs, MSNet2D's volume on its own preconv11 outputs"""
    g = _golden()
    assert all(v.dtype == torch.float32 and bool(v.any()) for v in g.values())
    M.check("sb golden", g["sb__vol"], M.reference("sb", torch.float64), M.reference("sb", torch.float32))
    feats, want = (g["ms__featL"], g["ms__featR"]), g["ms__vol"].unsqueeze(1)
    assert M.CASES[M.E2E_VOLUME_CASE][4] == want.shape[2] == 48 < feats[0].shape[3]
    M.check("ms golden", want, M.reference(M.E2E_VOLUME_CASE, torch.float64, feats), M.reference(M.E2E_VOLUME_CASE, torch.float32, feats))


def test_whole_model_restatement_gives_the_reference_disparity():
    """the restated MSNet2D on the CPU against the reference's disp_pred at the project's bar (1e-3 px EPE)"""
    g = _golden()
    L, R = M.e2e_images()
    with torch.no_grad():
        d = M.make_msnet2d()({"left": L, "right": R})["disp_pred"]
    assert g["e2e__disp_pred"].std() > 0.5
    assert float((d - g["e2e__disp_pred"]).abs().mean()) < 1e-3


def test_restatement_in_float32_is_close_to_but_not_equal_to_float64():
    """the figures the rule rests on are small and not zero (and reference() asserts that no case is vacuous)"""
    for case in M.CASES:
        r64, r32 = M.reference(case, torch.float64), M.reference(case, torch.float32)
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32 and tuple(r64.shape) == M.out_shape(case)
        assert 0 < M.err(r32, r64) <= 1e-5 * max(1.0, float(r64.abs().max())), case
        W = M.CASES[case][3]
        assert all(not r64[:, :, i, :, :i].any() for i in range(r64.shape[2])) and not r64[:, :, W:].any()


# ----------------------------------------------------------------------------- graft onto the reference's class
def test_attach_row_grafts_msnet2d_and_unpatch_restores_the_class():
    from openstereo_amd import attach
    from openstereo_amd.models.msnet import MSNet2D
    rows = {mod: classes for mod, classes in attach._graft_plan()}
    assert rows["stereo.modeling.models.msnet.MSNet2D"] == {"MSNet2D": (MSNet2D, ("forward", "reset_engine"), True)}
    assert "__init__" not in MSNet2D.__dict__                                # a mirror: it reads the reference's attribute layout
    ref = os.environ.get("OPENSTEREO_REF", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "stereo", "modeling", "models", "msnet")):
        cls = M.MSNet2D                                                      # no reference checkout here: the restatement's class stands in
        graft = lambda: attach._graft(cls, MSNet2D, ("forward", "reset_engine"), True)
    else:
        attach.stub_reference_packages(ref)
        import importlib
        cls = importlib.import_module("stereo.modeling.models.msnet.MSNet2D").MSNet2D
        graft = lambda: "stereo.modeling.models.msnet.MSNet2D.MSNet2D" in attach.patch_reference_modules() or pytest.fail("MSNet2D was not grafted")
    orig = cls.__dict__["forward"]
    try:
        graft()
        assert cls.__dict__["forward"] is not orig and cls.reset_engine is MSNet2D.reset_engine and cls._ref_forward is orig
    finally:
        attach.unpatch_reference()
    assert cls.__dict__["forward"] is orig and not {"reset_engine", "_eng", "_ref_forward"} & set(cls.__dict__)
