"""CPU: IGEV++'s multi-range lookup exists at every layer without a GPU -- C ABI (declared, exported, in the ctypes table, arguments
validated before any launch), `osa_native` ops (Meta kernels, tracing under FakeTensorMode) -- the golden fixture holds what this file's
own composition of the contract gives, the float64 reference of tests/test_gpu_multirange_lookup.py is validated against the same
composition in float32, and the disparity sets reach the tap pairs the accumulating backward has to get right in volumes 1 and 2."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import multirange_cases as M
from test_abi_cpu import declared_symbols

NEW = ("osa_geo_lookup_mr_f32", "osa_geo_lookup_mr_nhwc_f32", "osa_geo_lookup_mr_bwd_acc_f32")


def test_new_symbols_declared_exported_and_in_the_ctypes_table(lib):
    from openstereo_amd import _lib
    names = declared_symbols()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for n in NEW:
        assert n in names, f"{n} is not declared in include/openstereo_amd.h"
        assert re.search(rf"\bT {n}\b", exported), f"{n} is not exported"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert lib.osa_abi_version() == _lib.abi_version() >= 10


# ----------------------------------------------------------------------------- argument validation
F16 = 16                                     # any non-NULL, 16-byte aligned "pointer": a failed check returns before it is touched


def _arrays(levels, g_len=12, c_len=20, missing=None):
    n = max(levels, 1)
    ptrs = lambda: (ctypes.c_void_p * n)(*[None if missing == l else F16 for l in range(n)])
    lens = lambda v: (ctypes.c_int * n)(*[v >> l for l in range(n)])
    return ptrs(), ptrs(), lens(g_len), lens(c_len)


def _call(lib, form, levels=2, g_len=12, c_len=20, missing=None, g0=True, v1=F16, n1=6, v2=F16, n2=5, disp=F16, coords=F16,
          t=(F16, F16, F16, F16), cs=(144, 72, 72, 20), B=1, H=2, W=20, C=8, radius=4):
    gp, cp, gl, cl = _arrays(levels, g_len, c_len, missing)
    head = (gp if g0 else None, cp, gl, cl, levels, v1, n1, v2, n2, disp, coords, *t)
    tail = (B, H, W, C, radius, None)
    if form == "nchw":
        return lib.osa_geo_lookup_mr_f32(*head, *tail)
    if form == "nhwc":
        return lib.osa_geo_lookup_mr_nhwc_f32(*head, *cs, *tail)
    return lib.osa_geo_lookup_mr_bwd_acc_f32(*head, *tail)


@pytest.mark.parametrize("form", ["nchw", "nhwc", "bwd"])
def test_argument_validation_happens_before_any_launch(lib, form):
    """every condition is reported (non-zero return, message) before anything is launched: nothing here is a device pointer"""
    err = lambda: lib.osa_last_error()
    call = lambda **kw: _call(lib, form, **kw)
    # NULL pointers: the level arrays, a level, volumes 1 / 2, disp / coords, each of the four outputs (gradients)
    assert call(g0=False) != 0 and b"NULL" in err()
    assert call(v1=None) != 0 and b"NULL" in err()
    assert call(v2=None) != 0 and b"NULL" in err()
    assert call(disp=None) != 0 and b"NULL" in err()
    assert call(coords=None) != 0 and b"NULL" in err()
    for q in range(4):
        assert call(t=tuple(None if i == q else F16 for i in range(4))) != 0 and b"NULL" in err()
    assert call(missing=1) != 0 and b"level 1 missing" in err()
    # levels in 1..4
    assert call(levels=0) != 0 and b"levels unsupported" in err()
    assert call(levels=5) != 0 and b"levels unsupported" in err()
    # positive lengths: a level pooled down to nothing, volumes 1 / 2
    assert call(g_len=1) != 0 and b"level 1 missing" in err()
    assert call(c_len=0) != 0 and b"level 0 missing" in err()
    assert call(n1=0) != 0 and b"volume 1 / 2 of length" in err()
    assert call(n2=-3) != 0 and b"volume 1 / 2 of length" in err()
    assert call(B=0) != 0 and b"bad dims" in err()
    assert call(radius=-1) != 0 and b"bad dims" in err()
    # the 2^31 thread limit: 2^29 pixels x 34 rows
    assert call(B=1 << 15, H=1 << 14) != 0 and b"more than 2^31" in err()
    if form == "nhwc":
        for q, count in enumerate((144, 72, 72, 18)):
            cs = [144, 72, 72, 20]
            cs[q] = count - 1
            assert call(cs=tuple(cs)) != 0 and f"channel stride {count - 1} < {count} channels".encode() in err()
    if form == "bwd":
        assert call(radius=31) != 0 and b"has to fit a wave" in err()
        assert call(g_len=(1 << 19) + 1) != 0 and b"longer than 2^19" in err()
        assert call(c_len=(1 << 19) + 1) != 0 and b"longer than 2^19" in err()
        assert call(n1=(1 << 19) + 1) != 0 and b"longer than 2^19" in err()
        assert call(n2=(1 << 19) + 1) != 0 and b"longer than 2^19" in err()


# ----------------------------------------------------------------------------- extension ops
OPS = ("geo_lookup_mr", "geo_lookup_mr_nhwc", "geo_lookup_mr_bwd_acc")


def test_ops_have_meta_kernels_and_trace_under_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from openstereo_amd import _ext
    ns = _ext.load()
    for name in OPS:
        for key in ("Meta", "CUDA"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"osa_native::{name}", key), (name, key)
    B, C, D0, D1, D2, H, W, Cf, L, r = M.CASES["odd"]
    dev = "cuda" if torch.cuda.is_available() else "meta"
    with FakeTensorMode():
        e = lambda *s: torch.empty(*s, device=dev)
        src = [e(B, H, W, C, D0), e(B, H, W, C, D0 // 2), e(B, H, W, C, D1), e(B, H, W, C, D2), e(B, H, W, W), e(B, H, W, W // 2)]
        d, cx = e(B, H, W), e(B, H, W)
        outs = [e(B, n, H, W) for n in M.channels("odd")]
        assert ns.geo_lookup_mr(src, d, cx, outs, C, r) is None
        cl = [e(B, H, W, (n + 3) // 4 * 4) for n in M.channels("odd")]
        assert ns.geo_lookup_mr_nhwc(src, d, cx, cl, [t.shape[-1] for t in cl], [B, H, W], C, r) is None
        assert ns.geo_lookup_mr_bwd_acc([torch.empty_like(t) for t in src], d, cx, outs, C, r) is None
        assert [tuple(o.shape) for o in outs] == [(B, n, H, W) for n in M.channels("odd")]


def test_class_and_alias_are_exported():
    from openstereo_amd import geometry as G
    import inspect
    assert G.Combined_Geo_Encoding_Volume_PP is G.MultiRangeGeoEncodingVolume
    assert list(inspect.signature(G.MultiRangeGeoEncodingVolume.__init__).parameters)[1:] == \
        ["geo_volume0", "geo_volume1", "geo_volume2", "init_fmap1", "init_fmap2", "radius", "num_levels"]      # igevpp/geometry.py:7
    sig = inspect.signature(G.MultiRangeGeoEncodingVolume.__init__).parameters
    assert sig["radius"].default == 4 and sig["num_levels"].default == 2


# ----------------------------------------------------------------------------- fixture and references
def fp32_outputs(case, s, cv):
    """this file's composition of the contract in float32: what the reference project computes"""
    return M.reference(case, torch.float32).out(s, cv)


def test_golden_fixture_is_the_composition_in_float32():
    """tests/golden/igevpp_geometry.npz holds the REAL reference class's outputs (tests/golden/make_golden_igevpp_geometry.py), batch
    element 0 of each; the composition of tests/multirange_cases.py in float32 on the regenerated inputs gives them within 1e-6, with the
    contract's shapes"""
    z = np.load(M.GOLDEN)
    assert sorted(z.files) == sorted(f"{c}__{s}__{q}" for c in M.GOLDEN_CASES for s in M.GOLDEN_SETS for q in range(4))
    for case in M.GOLDEN_CASES:
        B, C, D0, D1, D2, H, W, Cf, L, r = M.CASES[case]
        T = 2 * r + 1
        for s in M.GOLDEN_SETS:
            got = [z[f"{case}__{s}__{q}"] for q in range(4)]
            assert [g.shape for g in got] == [(1, L * C * T, H, W), (1, C * T, H, W), (1, C * T, H, W), (1, L * T, H, W)]
            for q, (g, mine) in enumerate(zip(got, fp32_outputs(case, s, "grid"))):
                assert g.dtype == np.float32 and mine.dtype == torch.float32
                err = float((torch.from_numpy(g) - mine[:1]).abs().max())
                assert err <= 1e-6, f"{case} set {s} output {q}: {err:.3e}"
            assert any(g.any() for g in got)


@pytest.mark.parametrize("case", list(M.CASES))
def test_float64_reference_vs_float32_composition(case):
    """The composition in float32 against float64 on every case, set and coordinate variant: forward within 0.5 of the lookup tolerance
    (atol 2e-5, rtol 1e-5), source gradients within 1e-5 of max |grad| (the GPU tests allow 1e-4).  So the tolerances leave room for a
    correct fp32 kernel and none for a dropped tap.  The float32 side is this module's own composition, not the reference class (tests
    cannot read the reference): the fixture test ties the two together for `odd` and `radius1`, sets a / d / e, `grid` coordinates only;
    for the other cases, sets and the `half` coordinates that it computes what the reference computes rests on it being the same code."""
    r64, r32 = M.reference(case, torch.float64), M.reference(case, torch.float32)
    worst_f, worst_g = 0.0, 0.0
    for s in M.SETS:
        for cv in M.COORDS:
            for o64, o32 in zip(r64.out(s, cv), r32.out(s, cv)):
                assert o64.dtype == torch.float64 and o32.dtype == torch.float32 and o64.shape == o32.shape and torch.isfinite(o64).all()
                worst_f = max(worst_f, float(((o32.double() - o64).abs() / (2e-5 + 1e-5 * o64.abs())).max()))
                if s == "f":
                    assert not o64.any() and not o32.any()
            for g64, g32 in zip(r64.source_grads(s, cv), r32.source_grads(s, cv)):
                m = float(g64.abs().max())
                if m > 0:
                    worst_g = max(worst_g, float((g32.double() - g64).abs().max()) / m)
                else:
                    assert not g32.any()
    print(f"{case}: forward {worst_f:.3f} of the tolerance, gradients {worst_g:.2e} of max |grad|")
    assert worst_f <= 0.5, worst_f
    assert worst_g <= 1e-5, worst_g


def test_lattice_sets_reach_gap_and_same_tap_pairs_in_volumes_1_and_2():
    """as tests/test_geo_lookup_positions_cpu.py, at the scales the single-pyramid lookup never has on a level-0 row: volume 1 (disp / 2)
    and volume 2 (disp / 4) must each show, in at least one case, an adjacent tap pair whose x0 differ by 2 and one whose x0 are equal,
    inside the row -- and no step outside 0..2 in any source of any case (what the window of 2r + 3 positions relies on)"""
    found = {"volume 1": {}, "volume 2": {}}
    for case in M.CASES:
        L = M.CASES[case][8]
        tot = {"volume 1": [0, 0], "volume 2": [0, 0]}
        for s in M.LATTICE_SETS:
            for cv in M.COORDS:
                for q, (x, n) in enumerate(M.tap_positions(case, s, cv)):
                    assert n >= 2, "a row of length 1 divides by zero in the reference too"
                    gap, same, other = M.count_anomalies(x, n)
                    assert other == 0, f"{case} set {s} {cv} source {q}: x0 steps outside 0..2"
                    if q in (L, L + 1):
                        k = "volume 1" if q == L else "volume 2"
                        tot[k][0] += gap; tot[k][1] += same
        for k in tot:
            found[k][case] = tuple(tot[k])
    print(found)
    for k, per_case in found.items():
        assert any(min(v) >= 1 for v in per_case.values()), f"{k}: no case reaches both a gap and a same pair: {per_case}"
