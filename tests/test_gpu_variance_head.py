"""GPU: the disparity-variance heads (csrc/softargmin.hip *_var kernels, csrc/backward.hip *_var_bwd kernels) through `ops`, `autograd`,
`osa_native` and the models.

Cases and inputs: tests/variance_cases.py.  References: the fp64 CPU composition F.interpolate(trilinear) -> softmax -> the reference's
disparity_regression / disparity_variance arithmetic.  Bars: 4 x the reference's OWN fp32 error against fp64 on the same inputs, measured by
tests/golden/make_golden_variance.py with the reference's functions and stored in tests/golden/disparity_variance.npz (for the variance 4e-7 where that
error is below 1e-7; gradient bars have no floor).  The variance metric is max over ALL pixels of |var - var64| / (1 + var64); the gradient metric max |g - g64| /
max |g64| for the loss sum(a disp) + sum(b var) with stored a, b.  A one-pass E[d^2] - E[d]^2 in fp32 misses the sharp fused bar by orders of
magnitude.  Every figure is printed before it is asserted (pytest -s shows them)."""
import functools

import pytest
import torch

import variance_cases as VC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy


@functools.lru_cache(maxsize=None)
def _golden():
    return VC.load_golden()


def _arrs(name):
    g = _golden()
    keys = ("base", "idx_mid", "idx_sharp", "a", "b") + (("given_disp", "prob_unnorm") if name in VC.PLAIN else ())
    return {k: g[f"{name}__{k}"] for k in keys}


@functools.lru_cache(maxsize=None)
def _case(name, dist, form):
    """-> (leaves, constants, fn64 over double leaves, a, b, (disp64, var64), [g64 per leaf], E_ref, E_ref_grad): computed once per case"""
    arrs = _arrs(name)
    a, b = T(arrs["a"]), T(arrs["b"])
    if form == "given":
        leaves = [T(arrs["prob_unnorm"]), T(arrs["given_disp"])]
        fn = lambda x, d: VC.compose_prob(x, d)
        tag = f"{name}__given__prob"
    else:
        cost = VC.cost_of(arrs, dist)
        tag = f"{name}__{dist}__{form}"
        if form == "fused":
            _, (D, h, w), align = VC.FUSED[name]
            leaves, fn = [cost], (lambda c: VC.compose_fused(c, D, h, w, align))
        elif form == "logits":
            leaves, fn = [cost], (lambda c: VC.compose_logits(c))
        else:
            p = VC.prob_of(cost)
            mean = VC.own_mean(p)
            leaves, fn = [p], (lambda x: VC.compose_prob(x, mean.to(x.dtype)))
    with torch.no_grad():
        ref = fn(*[t.double() for t in leaves])
    g64 = VC.loss_grads(fn, [t.double() for t in leaves], a, b)
    g = _golden()
    return leaves, fn, a, b, ref, g64, float(g[tag + "__E_ref"]), [float(e) for e in g[tag + "__E_ref_grad"]]


def _check_var(tag, var, var64, e_ref):
    e, bar = VC.var_err(var.cpu(), var64), VC.bar(e_ref)
    print(f"{tag}: variance error {e:.3g} (reference fp32 {e_ref:.3g}, bar {bar:.3g}); var64 in [{float(var64.min()):.4g}, {float(var64.max()):.4g}]")
    assert torch.isfinite(var).all() and e <= bar, f"{tag}: variance error {e:.3g} > {bar:.3g} = 4 x the reference's fp32 error"


def _check_grad(tag, g, g64, e_ref_grad, zero_bound=None, abs_bound=None):
    if float(g64.abs().max()) == 0.0:
        # Dl = 1: every sample is the same value, the distribution is uniform whatever the cost -- the true gradient is exactly zero and
        # the relative metric has no denominator.  What is left is rounding of sum_d p_d [(d - mu) a + ((d - mu)^2 - var) b] = 0: see the caller
        print(f"{tag}: gradient is identically zero in fp64; max |g| {float(g.abs().max()):.3g} (bound {zero_bound:.3g})")
        assert float(g.abs().max()) <= zero_bound
        return
    e, bar = VC.grad_err(g.cpu(), g64), VC.grad_bar(e_ref_grad)
    print(f"{tag}: gradient error {e:.3g} (reference fp32 {e_ref_grad:.3g}, bar {bar:.3g})")
    assert torch.isfinite(g).all() and e <= bar, f"{tag}: gradient error {e:.3g} > {bar:.3g} = 4 x the reference's fp32 error"
    if abs_bound is not None:
        err = (g.cpu().double() - g64).abs()
        worst = float((err / abs_bound).max())
        print(f"{tag}: largest |g - g64| / per-element bound {worst:.3g}; max |g - g64| {float(err.max()):.3g}, max |g64| {float(g64.abs().max()):.3g}")
        assert worst <= 1.0, f"{tag}: an element's gradient error is {worst:.3g} x its bound"


def _grads_twice(fn, leaves, a, b):
    """gradients of the loss through the engine, twice: the backward kernels are atomic-free, so the two runs agree bit for bit"""
    runs = [VC.loss_grads(fn, [t.to(DEV) for t in leaves], a.to(DEV), b.to(DEV)) for _ in range(2)]
    torch.cuda.synchronize()
    for x, y in zip(*runs):
        assert x is not None and torch.equal(x, y), "two backward runs differ"
    return runs[0]


# ----------------------------------------------------------------------------- fused upsample form (x4 streaming kernel, generic kernel)
@pytest.mark.parametrize("dist", list(VC.DISTS))
@pytest.mark.parametrize("name", list(VC.FUSED))
def test_fused_head(name, dist):
    from openstereo_amd import ops, autograd as AG
    (cost,), _, a, b, (_, var64), (g64,), e_ref, (e_ref_grad,) = _case(name, dist, "fused")
    shape, (D, h, w), align = VC.FUSED[name]
    c = cost.to(DEV)
    want = ops.upsample_softargmin(c, D, h, w, align)
    disp, var = ops.upsample_softargmin(c, D, h, w, align, return_variance=True)
    assert disp.shape == var.shape == (shape[0], h, w) and disp.dtype == var.dtype == torch.float32
    assert torch.equal(disp, want), "the disparity moved when the variance was switched on"
    _check_var(f"{name}/{dist}", var, var64, e_ref)
    (g,) = _grads_twice(lambda x: AG.upsample_softargmin_variance(x, D, h, w, align), [cost], a, b)
    # (Dl = 1: the distribution is uniform, mu = (D - 1) / 2) per output pixel the D terms p_d [(d - mu) a + ((d - mu)^2 - var) b] cancel; each is
    # at most p_d (r |a| + r^2 |b|) with r = (D - 1) / 2 and sum p_d = 1, rounded to fp32 (eps = 2^-24), a factor 8 for the roundings of mu,
    # var, the coefficient and the sums; a low-res cell gathers (h w) / (Hl Wl) output pixels
    r = (D - 1) / 2
    zero_bound = 8 * 2.0 ** -24 * (h * w) / (shape[2] * shape[3]) * (r * float(a.abs().max()) + r * r * float(b.abs().max()))
    _check_grad(f"{name}/{dist}", g, g64, e_ref_grad, zero_bound)


# ----------------------------------------------------------------------------- logits form
@pytest.mark.parametrize("dist", list(VC.DISTS))
@pytest.mark.parametrize("name", list(VC.PLAIN))
def test_logits_head(name, dist):
    from openstereo_amd import ops, autograd as AG
    (cost,), _, a, b, (_, var64), (g64,), e_ref, (e_ref_grad,) = _case(name, dist, "logits")
    c = cost.to(DEV)
    want = ops.softmax_disparity_regression(c, keepdim=False)
    disp, var = ops.softmax_disparity_regression(c, keepdim=False, return_variance=True)
    assert disp.shape == var.shape == want.shape and var.dtype == torch.float32
    assert torch.equal(disp, want), "the disparity moved when the variance was switched on"
    dk, vk = ops.softmax_disparity_regression(c, maxdisp=c.shape[1], return_variance=True)                  # keepdim=True: [B,1,H,W]
    assert torch.equal(dk, disp.unsqueeze(1)) and torch.equal(vk, var.unsqueeze(1))
    _check_var(f"{name}/{dist}/logits", var, var64, e_ref)
    (g,) = _grads_twice(lambda x: AG.softmax_disparity_regression_variance(x, keepdim=False), [cost], a, b)
    # sharp: one plane holds all the mass but e^-40, so every gradient is ~0 (the peak's coefficient (k - mu) g + ((k - mu)^2 - var) g_var is
    # ~1e-13, the other planes' p_k below e^-32): the reference's fp32 autograd returns 0 where fp64 has 1e-12, its stored error is 1.0 and
    # the relative bar of 4.0 says nothing.  So every case also gets a bound per element, from the formula itself:
    #   p_k * S      the coefficient's sensitivity to the fp32 mean: the mean is off by at most 2 ulp of D (2 * 2^-23 * D) and the coefficient
    #                moves by |g| + 2 |k - mu| |g_var| <= max|a| + 2 D max|b| per unit of it.  (At the peak, p_k = 1, this is all fp32 can
    #                promise: k - mu ~ 1e-13 is not representable next to mu ~ 45.  Off the peak it is ~1e-17.)
    #   rel * |g_k|  p_k = exp(c_k - m) / se: the fp32 difference c_k - m is off by 2^-24 |c_k - m|, which is the relative error of p_k; 4 ulp for
    #                exp, the sum, the reciprocal and the two products
    D = cost.shape[1]
    S = 2 * 2.0 ** -23 * D * (float(a.abs().max()) + 2 * D * float(b.abs().max()))
    rel = 2.0 ** -24 * float(cost.max() - cost.min()) + 4 * 2.0 ** -23
    abs_bound = torch.softmax(cost.double(), 1) * S + rel * g64.abs()
    _check_grad(f"{name}/{dist}/logits", g, g64, e_ref_grad, abs_bound=abs_bound)


# ----------------------------------------------------------------------------- probabilities form (the reference function's exact twin)
@pytest.mark.parametrize("dist", list(VC.DISTS))
@pytest.mark.parametrize("name", list(VC.PLAIN))
def test_probabilities_head(name, dist):
    from openstereo_amd import ops, _ext
    (p,), _, a, b, (_, var64), (g64,), e_ref, (e_ref_grad,) = _case(name, dist, "prob")
    D = p.shape[1]
    mean = VC.own_mean(p).to(DEV)
    x = p.to(DEV)
    want = ops.disparity_regression(x, D, keepdim=False)
    disp, var = _ext.load().softargmin_var(x, mean)
    assert torch.equal(disp, want), "the disparity of the variance op is not the disparity_regression kernel's"
    v = ops.disparity_variance(x, D, mean)
    assert v.shape == (p.shape[0], 1, *p.shape[2:]) and v.dtype == torch.float32 and torch.equal(v[:, 0], var)
    _check_var(f"{name}/{dist}/prob", var, var64, e_ref)
    (g,) = _grads_twice(lambda xx: _ext.load().softargmin_var(xx, mean), [p], a, b)
    _check_grad(f"{name}/{dist}/prob", g, g64, e_ref_grad)


@pytest.mark.parametrize("name", list(VC.PLAIN))
def test_disparity_variance_with_a_given_disparity_and_unnormalised_volume(name):
    """ops.disparity_variance(x, maxdisp, disparity) against the stored outputs of BOTH reference functions and against fp64; gradients
    reach the volume and the disparity map"""
    from openstereo_amd import ops, autograd as AG, _ext
    (x, d), _, a, b, (_, var64), g64, e_ref, e_ref_grad = _case(name, "given", "given")
    g = _golden()
    D = x.shape[1]
    var = ops.disparity_variance(x.to(DEV), D, d.to(DEV))
    assert var.shape == d.shape and var.dtype == torch.float32
    assert torch.equal(T(g[f"{name}__given__prob__var64"])[:, 0], var64)
    for k in ("ref_cfnet", "ref_igevpp"):
        ref32 = T(g[f"{name}__given__prob__{k}"])
        e = VC.var_err(var.cpu(), ref32.double())
        print(f"{name}/given: against the stored {k} output {e:.3g} (bar {VC.bar(e_ref):.3g})")
        assert e <= VC.bar(e_ref)
    _check_var(f"{name}/given", var[:, 0], var64, e_ref)
    disp, v2 = _ext.load().softargmin_var(x.to(DEV), d.to(DEV))
    assert torch.equal(disp, ops.disparity_regression(x.to(DEV), D, keepdim=False)) and torch.equal(v2, var[:, 0])
    gx, gd = _grads_twice(lambda xx, dd: _ext.load().softargmin_var(xx, dd), [x, d], a, b)
    assert gd.shape == d.shape
    _check_grad(f"{name}/given dprob", gx, g64[0], e_ref_grad[0])
    _check_grad(f"{name}/given ddisparity", gd, g64[1], e_ref_grad[1])
    # the ops-level entry is differentiable too (variance only: the gradient of b * var)
    xs, ds = x.to(DEV).requires_grad_(), d.to(DEV).requires_grad_()
    (b.to(DEV) * AG.disparity_variance(xs, D, ds)[:, 0]).sum().backward()
    dd = torch.arange(D, dtype=torch.float64).view(1, D, 1, 1) - d.double()
    e_x = VC.grad_err(xs.grad.cpu(), b.double().unsqueeze(1) * dd ** 2)
    e_d = VC.grad_err(ds.grad.cpu(), -2 * b.double().unsqueeze(1) * (x.double() * dd).sum(1, keepdim=True))
    print(f"{name}/given through autograd.disparity_variance: dprob {e_x:.3g} (bar {VC.grad_bar(e_ref_grad[0]):.3g}), ddisparity {e_d:.3g} (bar {VC.grad_bar(e_ref_grad[1]):.3g})")
    assert e_x <= VC.grad_bar(e_ref_grad[0]) and e_d <= VC.grad_bar(e_ref_grad[1])


def test_results_are_fp32_under_autocast_and_for_half_inputs():
    from openstereo_amd import ops
    arrs = _arrs("d5")
    x, d = T(arrs["prob_unnorm"]).to(DEV), T(arrs["given_disp"]).to(DEV)
    want = ops.disparity_variance(x.half().float(), 5, d.half().float())
    with torch.autocast("cuda", dtype=torch.float16):
        v = ops.disparity_variance(x.half(), 5, d.half())
    assert v.dtype == torch.float32 and torch.equal(v, want)                 # inputs cast to fp32, result fp32 (like disparity_regression)
    assert ops.disparity_variance(x.half(), 5, d.half()).dtype == torch.float16
    c = VC.cost_of(_arrs("x4_dl3"), "mid").to(DEV)
    disp, var = ops.upsample_softargmin(c.half()[:, None], 12, 12, 68, return_variance=True)               # [B,1,Dl,Hl,Wl] accepted
    d2, v2 = ops.upsample_softargmin(c.half().float(), 12, 12, 68, return_variance=True)
    assert var.dtype == torch.float32 and torch.equal(disp, d2) and torch.equal(var, v2)


def test_opcheck_of_the_three_ops():
    from torch.library import opcheck
    from openstereo_amd import _ext
    ns = _ext.load()
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    for op, args in ((ns.softargmin_var.default, (r(1, 3, 2, 5).abs().requires_grad_(), r(1, 1, 2, 5).requires_grad_())),
                     (ns.softmax_softargmin_var.default, (r(1, 3, 2, 5).requires_grad_(),)),
                     (ns.upsample_softargmin_var.default, (r(1, 2, 2, 3).requires_grad_(), 8, 8, 12, False)),      # x4 kernel
                     (ns.upsample_softargmin_var.default, (r(1, 2, 2, 3).requires_grad_(), 5, 5, 7, True))):       # generic kernel
        opcheck(op, args, test_utils=utils)


def test_fused_head_replays_bit_identically_from_a_captured_graph():
    from openstereo_amd import ops
    static_c = VC.cost_of(_arrs("x4"), "sharp").to(DEV)
    other = VC.cost_of(_arrs("x4"), "flat").to(DEV)
    eager = [t.clone() for t in ops.upsample_softargmin(static_c, 192, 20, 72, return_variance=True)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.upsample_softargmin(static_c, 192, 20, 72, return_variance=True)
    keep = static_c.clone()
    static_c.copy_(other)
    graph.replay()
    static_c.copy_(keep)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    first = [t.clone() for t in out]
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], first[0]) and torch.equal(out[1], first[1])


# ----------------------------------------------------------------------------- models
def _stashed_final_cost(gw, run):
    """the model's own final low-res cost of one forward: the `classif3.2` stage of the diagnostics stash (GwcDispProcessor.aggregate_cl)"""
    gw.STAGE_STASH = []
    try:
        out = run()
        cost = [t for n, t in gw.STAGE_STASH if n == "classif3.2"]
    finally:
        gw.STAGE_STASH = None
    assert len(cost) == 1
    return out, cost[0]


@pytest.mark.parametrize("vol_split", [True, False], ids=["split_volume_path", "dict_path"])
def test_gwcnet_returns_the_variance_on_request_only(vol_split, monkeypatch):
    from openstereo_amd import ops
    from openstereo_amd.models import gwcnet as gw
    from openstereo_amd.utils.weights import synth_state_dict, synth_images
    from openstereo_amd import engine
    monkeypatch.setattr(engine, "_precision", "f16x3")                  # engine.set_precision("f16x3"), undone after the test: the split volume exists in this mode only
    monkeypatch.setattr(gw, "_SPLIT_ACT", True)
    monkeypatch.setattr(gw, "_VOL_SPLIT", vol_split)                    # what OSA_VOL_SPLIT=0 selects at import
    net = gw.GwcNet()
    net.load_state_dict(synth_state_dict(net, seed=0))
    net = net.to(DEV).eval()
    L, R = (t.to(DEV) for t in synth_images(1, 64, 256, seed=1))      # quarter width 64: the narrowest the split volume builder takes (two 32-pixel tiles at 64 channels)
    with torch.no_grad():
        inputs = {"left": L, "right": R}
        before = net(inputs)                                            # the flag was never set
        assert ("cost_volume" in inputs) == (not vol_split), "the test did not reach the path it names"
        net.return_variance = True
        on, cost = _stashed_final_cost(gw, lambda: net({"left": L, "right": R}))
        net.return_variance = False
        off = net({"left": L, "right": R})
        torch.cuda.synchronize()
        assert sorted(before) == sorted(off) == ["disp_pred"] and torch.equal(off["disp_pred"], before["disp_pred"])
        assert sorted(on) == ["disp_pred", "disp_var"] and torch.equal(on["disp_pred"], before["disp_pred"])
        assert on["disp_var"].shape == (1, 64, 256) and on["disp_var"].dtype == torch.float32
        want = ops.upsample_softargmin(cost, net.maxdisp, 64, 256, align_corners=False, return_variance=True)
        assert torch.equal(on["disp_var"], want[1]) and torch.equal(on["disp_pred"], want[0])
        assert float(on["disp_var"].min()) >= 0 and torch.isfinite(on["disp_var"]).all()


def test_gwcnet_traces_with_fake_tensors_with_the_variance_on():
    from torch.fx.experimental.proxy_tensor import make_fx
    from openstereo_amd import ranges
    from openstereo_amd.models import gwcnet as gw
    from openstereo_amd.utils.weights import synth_state_dict, synth_images
    net = gw.GwcNet()
    net.load_state_dict(synth_state_dict(net, seed=0))
    net = net.to(DEV).eval()
    net.return_variance = True
    L, R = (t.to(DEV) for t in synth_images(1, 64, 128, seed=1))
    try:
        with torch.no_grad():
            def f(a, b):
                o = net({"left": a, "right": b})
                return o["disp_pred"], o["disp_var"]
            want = f(L, R)                                              # eager: also builds every packed weight
            torch.cuda.synchronize()
            ranges.reset_arenas()
            gm = make_fx(f, tracing_mode="fake", _allow_non_fake_inputs=True)(L, R)
            ranges.reset_arenas()
            targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
            assert any("upsample_softargmin_var" in t for t in targets), sorted(set(targets))
            got = gm(L, R)
            torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    finally:
        ranges.reset_arenas()


def test_psmnet_returns_the_variance_of_the_final_cost_on_request_only():
    from openstereo_amd import ops
    from openstereo_amd.models.psmnet import PSMNet, _Cfg
    from openstereo_amd.utils.weights import synth_state_dict, synth_images
    net = PSMNet(_Cfg(MAX_DISP=64))
    net.load_state_dict(synth_state_dict(net, seed=0, head_gain=3.0), strict=False)
    net = net.to(DEV).eval()
    L, R = (t.to(DEV) for t in synth_images(1, 256, 512, seed=1, max_shift=16.0))
    with torch.no_grad():
        before = net({"left": L, "right": R})
        net.return_variance = True
        inputs = {"left": L, "right": R}
        on = net(inputs)
        net.return_variance = False
        off = net({"left": L, "right": R})
        torch.cuda.synchronize()
        assert sorted(before) == sorted(off) == ["disp_pred", "train_preds"] and sorted(on) == ["disp_pred", "disp_var", "train_preds"]
        for x, y, z in zip(before["train_preds"], on["train_preds"], off["train_preds"]):
            assert torch.equal(x, y) and torch.equal(x, z)
        assert torch.equal(on["disp_pred"], before["disp_pred"]) and torch.equal(off["disp_pred"], before["disp_pred"])
        want = ops.upsample_softargmin(inputs["cost3"], 64, 256, 512, align_corners=True, return_variance=True)
        assert on["disp_var"].shape == (1, 256, 512) and torch.equal(on["disp_var"], want[1]) and torch.equal(on["disp_pred"], want[0])
