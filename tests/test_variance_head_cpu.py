"""CPU: the disparity-variance heads exist at every layer -- C ABI (declared, exported, in the ctypes table, arguments validated before any
launch), `osa_native` ops (Meta kernels: shapes and dtypes under FakeTensorMode), `ops.disparity_variance` (no CPU path) -- and the golden
fixture holds what the reference's formula gives on its stored inputs."""
import re
import subprocess

import numpy as np
import pytest
import torch

import variance_cases as VC
from test_abi_cpu import declared_symbols

NEW = ("osa_softargmin_var_f32", "osa_softmax_softargmin_var_f32", "osa_upsample_softargmin_var_f32",
       "osa_softargmin_var_bwd_f32", "osa_softmax_softargmin_var_bwd_f32", "osa_upsample_softargmin_var_bwd_ws_f32")


def test_new_symbols_declared_exported_and_in_the_ctypes_table(lib):
    from openstereo_amd import _lib
    names = declared_symbols()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for n in NEW:
        assert n in names, f"{n} is not declared in include/openstereo_amd.h"
        assert re.search(rf"\bT {n}\b", exported), f"{n} is not exported"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert lib.osa_abi_version() == _lib.abi_version() >= 8


def test_argument_validation_happens_before_any_launch(lib):
    f = 16                                   # any non-NULL, 16-byte aligned "pointer": a failed check returns before it is touched
    err = lambda: lib.osa_last_error()
    # probabilities form
    assert lib.osa_softargmin_var_f32(None, f, f, f, 1, 4, 4, 4, None) != 0 and b"NULL" in err()
    assert lib.osa_softargmin_var_f32(f, None, f, f, 1, 4, 4, 4, None) != 0 and b"NULL" in err()
    assert lib.osa_softargmin_var_f32(f, f, f, None, 1, 4, 4, 4, None) != 0 and b"NULL" in err()
    assert lib.osa_softargmin_var_f32(f, f, f, f, 1, 0, 4, 4, None) != 0 and b"bad dims" in err()
    assert lib.osa_softargmin_var_bwd_f32(f, f, f, None, f, f, 1, 4, 4, 4, None) != 0 and b"NULL" in err()
    assert lib.osa_softargmin_var_bwd_f32(f, f, f, f, f, None, 1, 4, 4, 4, None) != 0 and b"NULL" in err()
    assert lib.osa_softargmin_var_bwd_f32(f, f, None, f, f, f, 1, 4, -1, 4, None) != 0 and b"bad dims" in err()
    # logits form
    assert lib.osa_softmax_softargmin_var_f32(f, None, f, 1, 4, 4, 4, None) != 0 and b"NULL" in err()
    assert lib.osa_softmax_softargmin_var_f32(f, f, None, 1, 4, 4, 4, None) != 0 and b"NULL" in err()
    assert lib.osa_softmax_softargmin_var_f32(f, f, f, 0, 4, 4, 4, None) != 0 and b"bad dims" in err()
    assert lib.osa_softmax_softargmin_var_bwd_f32(f, f, None, f, 1, 4, 4, 4, None) != 0 and b"NULL" in err()
    assert lib.osa_softmax_softargmin_var_bwd_f32(f, f, f, f, 1, 4, 4, 0, None) != 0 and b"bad dims" in err()
    # fused form
    assert lib.osa_upsample_softargmin_var_f32(f, f, None, 1, 4, 4, 4, 16, 16, 16, 0, None) != 0 and b"NULL" in err()
    assert lib.osa_upsample_softargmin_var_f32(None, f, f, 1, 4, 4, 4, 16, 16, 16, 0, None) != 0 and b"NULL" in err()
    assert lib.osa_upsample_softargmin_var_f32(f, f, f, 1, 4, 4, 4, 16, 0, 16, 0, None) != 0 and b"bad dims" in err()
    assert lib.osa_upsample_softargmin_var_f32(f, f, f, 1, 161, 4, 4, 644, 16, 16, 0, None) != 0 and b"too large for LDS" in err()   # 161 * 256 * 4 B > 160 KB
    need = lib.osa_upsample_softargmin_bwd_workspace_bytes(1, 4, 16, 16)
    assert need == 4 * 16 * 16 * 4
    bwd = lambda *a: lib.osa_upsample_softargmin_var_bwd_ws_f32(*a)
    assert bwd(f, f, None, f, 1, 4, 4, 4, 16, 16, 16, 0, f, need, None) != 0 and b"NULL" in err()
    assert bwd(f, f, f, f, 1, 4, 4, 4, 16, 16, 16, 0, None, need, None) != 0 and b"NULL" in err()
    assert bwd(f, f, f, f, 1, 4, 0, 4, 16, 16, 16, 0, f, need, None) != 0 and b"bad dims" in err()
    assert bwd(f, f, f, f, 1, 4, 4, 4, 16, 16, 16, 0, f, need - 1, None) != 0 and b"workspace too small or misaligned" in err()
    assert bwd(f, f, f, f, 1, 4, 4, 4, 16, 16, 16, 0, f + 4, need, None) != 0 and b"workspace too small or misaligned" in err()
    assert bwd(f, f, f, f, 1, 161, 4, 4, 644, 16, 16, 0, f, 161 * 16 * 16 * 4, None) != 0 and b"too large for LDS" in err()             # 2 * 161 * 128 * 4 B


def test_meta_kernels_give_shapes_and_dtypes_under_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from openstereo_amd import _ext
    ns = _ext.load()
    dev = "cuda" if torch.cuda.is_available() else "meta"
    with FakeTensorMode():
        e = lambda *s: torch.empty(*s, device=dev)
        pairs = (ns.softargmin_var(e(2, 12, 5, 7), e(2, 1, 5, 7)), ns.softmax_softargmin_var(e(2, 12, 5, 7)),
                 ns.upsample_softargmin_var(e(2, 3, 2, 4), 12, 5, 7, True))
        for disp, var in pairs:
            assert disp.shape == var.shape == (2, 5, 7) and disp.dtype == var.dtype == torch.float32 and disp.device == var.device == e(1).device
        dp, dd = ns.softargmin_var_bwd(e(2, 12, 5, 7), e(2, 1, 5, 7), e(2, 5, 7), e(2, 5, 7))
        assert dp.shape == (2, 12, 5, 7) and dd.shape == (2, 1, 5, 7) and dp.dtype == dd.dtype == torch.float32
        dc = ns.softmax_softargmin_var_bwd(e(2, 12, 5, 7), e(2, 5, 7), e(2, 5, 7))
        assert dc.shape == (2, 12, 5, 7) and dc.dtype == torch.float32
        dc = ns.upsample_softargmin_var_bwd(e(2, 3, 2, 4), e(2, 5, 7), e(2, 5, 7), 12, 5, 7, True)
        assert dc.shape == (2, 3, 2, 4) and dc.dtype == torch.float32
    for name in ("softargmin_var", "softmax_softargmin_var", "upsample_softargmin_var"):
        for key in ("Meta", "CUDA", "Autograd"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"osa_native::{name}", key), (name, key)
    # the C++ Autograd kernels give both results a grad_fn, on meta tensors too
    c = torch.empty(2, 3, 2, 4, device="meta", requires_grad=True)
    disp, var = ns.upsample_softargmin_var(c, 12, 5, 7, False)
    assert disp.requires_grad and var.requires_grad


def test_product_has_no_cpu_path_for_the_variance():
    from openstereo_amd import ops, _lib
    with pytest.raises(_lib.EngineError):
        ops.disparity_variance(torch.zeros(1, 4, 4, 4), 4, torch.zeros(1, 1, 4, 4))
    with pytest.raises(_lib.EngineError):
        ops.upsample_softargmin(torch.zeros(1, 4, 4, 4), 16, 16, 16, return_variance=True)
    with pytest.raises(_lib.EngineError):
        ops.softmax_disparity_regression(torch.zeros(1, 4, 4, 4), return_variance=True)


def test_models_keep_the_flag_off_by_default():
    from openstereo_amd.models.gwcnet import GwcNet
    from openstereo_amd.models.psmnet import PSMNet
    assert GwcNet.return_variance is False and PSMNet.return_variance is False
    assert "return_variance" not in GwcNet().state_dict() and len(GwcNet().state_dict()) == 533


def test_psmnet_refuses_the_variance_of_a_full_resolution_cost():
    """the stage accepts the reference's full-resolution costs [B,D,H,W] too; those go through FasterSoftArgmin, which has no variance"""
    from openstereo_amd import _lib
    from openstereo_amd.models.psmnet import PSMDispProcessor
    c = torch.zeros(1, 8, 4, 4)
    with pytest.raises(_lib.EngineError, match="low-res cost3"):
        PSMDispProcessor(max_disp=8)({"left": torch.zeros(1, 3, 4, 4), "cost1": c, "cost2": c, "cost3": c}, return_variance=True)


def test_a_grafted_psmnet_class_picks_the_flag_up():
    """attach grafts PSMNet.forward onto the reference's PSMNet class (a stand-in here: same three stage attributes, no `return_variance`
    attribute of its own); the flag set on an instance reaches the head stage, and off it the stage is called as before"""
    from openstereo_amd import attach
    from openstereo_amd.models import psmnet as PSM
    assert any(name.endswith("psmnet.psmnet") and classes.get("PSMNet", (None,))[0] is PSM.PSMNet for name, classes in attach._graft_plan())
    calls = []

    class RefPSMNet(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.Backbone = lambda inputs: {"ref_feature": 1}
            self.CostProcessor = lambda inputs: {"cost3": 2}

        def DispProcessor(self, inputs, return_variance=False):
            calls.append(return_variance)
            return (["d1", "d2", "d3"], "var") if return_variance else ["d1", "d2", "d3"]

        def forward(self, inputs):
            raise AssertionError("the reference forward ran")

    attach._graft(RefPSMNet, PSM.PSMNet, ("forward",), False)
    try:
        net = RefPSMNet().eval()
        assert net({}) == {"disp_pred": "d3", "train_preds": ["d1", "d2", "d3"]}
        net.return_variance = True
        assert net({}) == {"disp_pred": "d3", "train_preds": ["d1", "d2", "d3"], "disp_var": "var"}
        assert net.train()({}) == {"disp_pred": "d3", "train_preds": ["d1", "d2", "d3"]}            # eval mode only
        assert calls == [False, True, False]
    finally:
        attach.unpatch_reference()


def test_golden_equals_the_formula_on_the_stored_inputs():
    """the stored outputs of the reference's two functions are sum_d x (d - disparity)^2 of the stored inputs (fp32: bit for bit, the
    arithmetic of tests/variance_cases.py is the reference's), the stored fp64 values are that formula in fp64, the stored inputs are what
    the seeds give, and every case carries its error figures"""
    g = VC.load_golden()
    T = torch.from_numpy
    for name in VC.PLAIN:
        x, d = T(g[f"{name}__prob_unnorm"]), T(g[f"{name}__given_disp"])
        D = x.shape[1]
        want = VC.variance(x, D, d)
        assert want.shape == d.shape
        for k in ("ref_cfnet", "ref_igevpp"):
            assert torch.equal(T(g[f"{name}__given__prob__{k}"]), want), (name, k)
        dv = torch.arange(D, dtype=torch.float64).view(1, D, 1, 1)
        v64 = (x.double() * (dv - d.double()) ** 2).sum(1, keepdim=True)
        assert torch.equal(T(g[f"{name}__given__prob__var64"]), v64)
        assert VC.var_err(want, v64) == pytest.approx(float(g[f"{name}__given__prob__E_ref"]), rel=1e-6, abs=1e-12)
    for name in list(VC.FUSED) + list(VC.PLAIN):
        for k, v in VC.make_inputs(name).items():
            assert np.array_equal(g[f"{name}__{k}"], v), (name, k)
        for dist in VC.DISTS:
            for form in (("fused",) if name in VC.FUSED else ("logits", "prob")):
                e, eg = g[f"{name}__{dist}__{form}__E_ref"], g[f"{name}__{dist}__{form}__E_ref_grad"]
                assert e.shape == () and 0 <= float(e) < 1e-4 and eg.shape == (1,), (name, dist, form)
    # the sharp fused case is the regime the issue is about: a small variance at a large disparity
    arrs = {k: g[f"x4__{k}"] for k in ("base", "idx_mid", "idx_sharp")}
    disp, var = VC.compose_fused(VC.cost_of(arrs, "sharp").double(), 192, 20, 72, False)
    assert float(var.min()) < 0.5 and float(disp.min()) > 150
