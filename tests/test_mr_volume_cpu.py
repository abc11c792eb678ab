"""CPU: IGEV++'s multi-range cost volumes exist at every layer without a GPU -- C ABI 11 (declared, exported, in the ctypes table, arguments
validated before any launch), the `osa_native.mr_volume` op and its backward (Meta kernels: shapes, strides of both memory formats,
dtypes), ops.build_multirange_volumes refusing CPU tensors, the golden fixture against the restatement of tests/mr_volume_cases.py by the
tolerance rule stated there, and ops.disparity_regression's interval."""
import re
import subprocess

import numpy as np
import pytest
import torch

import mr_volume_cases as M
from test_abi_cpu import declared_symbols

NEW = ("osa_mr_volume_f32", "osa_mr_volume_bwd_workspace_bytes", "osa_mr_volume_bwd_ws_f32")


def test_new_symbols_declared_exported_and_in_the_ctypes_table(lib):
    from openstereo_amd import _lib
    names = declared_symbols()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for n in NEW:
        assert n in names, f"{n} is not declared in include/openstereo_amd.h"
        assert re.search(rf"\bT {n}\b", exported), f"{n} is not exported"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert lib.osa_abi_version() == _lib.abi_version() >= 11


# ----------------------------------------------------------------------------- argument validation
P = 16                                       # any non-NULL, 16-byte aligned "pointer": a failed check returns before it is touched
OK = dict(B=1, C=32, H=2, W=20, G=8, Co=8, D=16, S=4, M=8, k0=2, k1=4, layout=0)


def _fwd(lib, ptrs=(P,) * 7, **kw):
    a = {**OK, **kw}
    return lib.osa_mr_volume_f32(*ptrs, a["layout"], a["B"], a["C"], a["H"], a["W"], a["G"], a["Co"], a["D"], a["S"], a["M"], a["k0"], a["k1"], None)


def _bwd(lib, dv=(P, P, P), ptrs=(P,) * 8, ws=P, ws_bytes=None, **kw):
    a = {**OK, **kw}
    need = lib.osa_mr_volume_bwd_workspace_bytes(a["B"], a["H"], a["W"], a["D"])
    return lib.osa_mr_volume_bwd_ws_f32(*dv, a["layout"], *ptrs, a["B"], a["C"], a["H"], a["W"], a["G"], a["Co"], a["D"], a["S"], a["M"], a["k0"], a["k1"],
                                        ws, need if ws_bytes is None else ws_bytes, None)


@pytest.mark.parametrize("form", ["fwd", "bwd"])
def test_argument_validation_happens_before_any_launch(lib, form):
    """every condition is reported (non-zero return, a message naming the limit) before anything is launched: nothing here is a device
    pointer"""
    err = lambda: lib.osa_last_error()
    call = (lambda **kw: _fwd(lib, **kw)) if form == "fwd" else (lambda **kw: _bwd(lib, **kw))
    n = 7 if form == "fwd" else 8
    for q in range(n):                                               # every required pointer
        assert call(ptrs=tuple(None if i == q else P for i in range(n))) != 0 and b"NULL pointer" in err(), q
    assert call(B=0) != 0 and b"bad dims" in err()
    assert call(C=36) != 0 and b"C=36 not divisible by groups=8" in err()
    assert call(G=4) != 0 and b"supported: 8 groups and 8 output channels" in err()
    assert call(Co=16) != 0 and b"supported: 8 groups and 8 output channels" in err()
    assert call(k0=3, M=9, D=20) != 0 and b"patch sizes k0=3, k1=4 (supported: 2 and 4)" in err()
    assert call(k1=8) != 0 and b"patch sizes k0=2, k1=8 (supported: 2 and 4)" in err()
    for bad in (dict(S=0), dict(S=10), dict(M=18), dict(S=8, M=4)):      # 0 < S <= M <= D
        assert call(**bad) != 0 and b"0 < s_range <= m_range <= maxdisp" in err(), bad
    assert call(M=7) != 0 and b"m_range=7 must be divisible by k0=2" in err()
    assert call(D=18) != 0 and b"maxdisp=18 by k1=4" in err()
    assert call(layout=2) != 0 and b"layout 2" in err()
    if form == "bwd":
        assert _bwd(lib, ws=None) != 0 and b"NULL pointer" in err()
        need = lib.osa_mr_volume_bwd_workspace_bytes(1, 2, 20, 16)
        assert need == 1 * 2 * 1 * 4 * 128 * 4                           # one 64-pixel tile per row, one chunk of planes: 4 waves x 128 partial sums
        assert _bwd(lib, ws_bytes=need - 1) != 0 and f"workspace of {need - 1} bytes, {need} needed".encode() in err()
        assert lib.osa_mr_volume_bwd_workspace_bytes(2, 3, 65, 48) == 2 * 3 * 2 * 2 * 4 * 128 * 4       # two tiles per row, two chunks of 32 planes
        assert lib.osa_mr_volume_bwd_workspace_bytes(1, 136, 240, 192) == 544 * 6 * 4 * 128 * 4      # the evaluation map: six chunks of 32 planes


# ----------------------------------------------------------------------------- extension op
@pytest.mark.parametrize("cl", [False, True])
def test_meta_kernels_give_shapes_strides_and_dtypes(cl):
    from openstereo_amd import _ext
    ns = _ext.load()
    for name in ("mr_volume", "mr_volume_bwd"):
        for key in ("Meta", "CUDA"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"osa_native::{name}", key), (name, key)
    assert torch._C._dispatch_has_kernel_for_dispatch_key("osa_native::mr_volume", "Autograd")
    B, C, H, W, D, S, Mr, k0, k1 = M.CASES["small"]
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)
    l, p0, p1 = m(B, C, H, W), m(8, 8, k0, 1, 1), m(8, 8, k1, 1, 1)
    vs = ns.mr_volume(l, l, p0, p1, D, S, Mr, cl)
    assert [tuple(v.shape) for v in vs] == [(B, 8, S, H, W), (B, 8, Mr // k0, H, W), (B, 8, D // k1, H, W)]
    for v in vs:
        assert v.dtype == torch.float32
        want = torch.empty(v.shape, device="meta").contiguous(memory_format=torch.channels_last_3d if cl else torch.contiguous_format)
        assert v.stride() == want.stride(), (v.stride(), want.stride())
    # other float dtypes are widened by the Autograd kernel; the outputs carry a grad_fn
    h = lambda *s: torch.empty(*s, device="meta", dtype=torch.float16, requires_grad=True)
    vs16 = ns.mr_volume(h(B, C, H, W), h(B, C, H, W), h(8, 8, k0, 1, 1), h(8, 8, k1, 1, 1), D, S, Mr, cl)
    assert all(v.dtype == torch.float32 and v.requires_grad for v in vs16)
    gl, gr, g0, g1 = ns.mr_volume_bwd(vs[0], None, vs[2], l, l, p0, p1, D, S, Mr, cl)
    assert gl.shape == gr.shape == l.shape and g0.shape == p0.shape and g1.shape == p1.shape
    assert all(g.dtype == torch.float32 and g.is_contiguous() for g in (gl, gr, g0, g1))
    with pytest.raises(RuntimeError, match="s_range <= m_range <= maxdisp"):
        ns.mr_volume(l, l, p0, p1, D, Mr + 2, Mr, cl)
    with pytest.raises(RuntimeError, match=r"\[Co, G, k, 1, 1\]"):
        ns.mr_volume(l, l, m(8, 8, k0, 1, 3), p1, D, S, Mr, cl)


def test_cpu_tensors_raise_engine_error():
    from openstereo_amd import ops, _lib
    L, R, P0, P1 = M.inputs("k44")
    B, C, H, W, D, S, Mr, k0, k1 = M.CASES["k44"]
    with pytest.raises(_lib.EngineError, match="match_left is on cpu"):
        ops.build_multirange_volumes(L, R, P0, P1, D, S, Mr)
    with pytest.raises(TypeError):
        ops.build_multirange_volumes(L.numpy(), R, P0, P1, D, S, Mr)


# ----------------------------------------------------------------------------- fixture
@pytest.mark.parametrize("case", M.GOLDEN_CASES)
def test_golden_fixture_satisfies_the_rule_against_the_restatement(case):
    """tests/golden/igevpp_volumes.npz holds the REAL reference's build_gwc_volume + F.conv3d (tests/golden/make_golden_mr_volume.py); by
    the rule, it is what the restatement of tests/mr_volume_cases.py computes on the regenerated inputs"""
    z = np.load(M.GOLDEN)
    assert sorted(z.files) == sorted(f"{c}__{n}" for c in M.GOLDEN_CASES for n in M.NAMES)
    r64, r32 = M.reference(case, torch.float64)[0], M.reference(case, torch.float32)[0]
    for name, o64, o32 in zip(M.NAMES, r64, r32):
        g = z[f"{case}__{name}"]
        assert g.dtype == np.float32 and g.any()
        M.check(f"{case} golden {name}", torch.from_numpy(g), o64, o32)


def test_restatement_gradients_in_float32_are_close_to_float64():
    """the figures the rule rests on are small: a wrong restatement in one of the two precisions would show here"""
    for case in M.CASES:
        (o64, g64), (o32, g32) = M.reference(case, torch.float64), M.reference(case, torch.float32)
        for a, b_ in zip(o64 + g64, o32 + g32):
            assert a.dtype == torch.float64 and b_.dtype == torch.float32
            assert 0 < M.err(b_, a) <= 1e-4 * max(1.0, float(a.abs().max())), case


# ----------------------------------------------------------------------------- disparity_regression(interval)
def test_disparity_regression_rejects_a_wrong_plane_count_for_the_interval(monkeypatch):
    from openstereo_amd import ops
    import inspect
    assert inspect.signature(ops.disparity_regression).parameters["interval"].default == 1
    monkeypatch.setattr(ops, "_chk", lambda t, *a: t)              # the plane check comes before anything touches a device
    x = torch.zeros(1, 48, 2, 5)
    for maxdisp, interval in ((192, 2), (96, 4), (48, 2), (47, 1)):
        with pytest.raises(AssertionError, match="disparity planes"):
            ops.disparity_regression(x, maxdisp, True, interval)
