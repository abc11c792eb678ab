"""Forward, data gradient, weight gradient and bias gradient of the stride-2 convolutions and stride-2 transposed convolutions training
admits (Conv3d k3/s2/p1 on even dims; ConvTranspose3d / ConvTranspose2d as k3/p1/op1 and k4/p1/op0) -- the fused parity kernel, the
stride-2 brick kernel in its "dgrad_of_deconv" form, the class-mode weight-gradient kernels, the bias outside the launch -- against the
float64 reference and under the bounds of tests/strided_conv_cases.py (derived from the number formats in tests/conv_geometry_cases.py);
and the edge of the admitted domain.  Every test prints its error / bound ratios.

Measured on an MI355X (largest error / bound over the table): y 0.028, dx 0.020, db 0.10 in every mode; dw 0.29 on the exact fp32
class-mode kernel (f32 and f16x3 modes alike), 0.39 on the f16x3 class-mode kernel, 0.10 on the fp16 one.  Both dw maxima are the
one-voxel transposed layer t3_k3_one_voxel, where K = 2: a sum of two products has no cancellation of rounding errors to hide behind, so
the worst-case bound 6 u S is nearly met (torch's float32 on the CPU gives the same 0.29 there), and in the split kernel the two operands'
representation errors (2^-22 each, 8 u S together) are most of the (3 K + 16) u S = 22 u S.  Everywhere K is large the ratios sit one to
two orders below 1, as on the stride-1 table."""
import pytest
import torch
import torch.nn as nn

import strided_conv_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = ("y", "dx", "dw", "db")


def _engine_op(case, x, w, b, precision):
    from openstereo_amd import autograd as AG
    if case.kind == "conv3d_s2":
        return AG.conv3d(x, w, b, 2, case.pad, 1, precision=precision)
    f = AG.conv_transpose3d if case.kind == "deconv3d" else AG.conv_transpose2d
    return f(x, w, b, 2, case.pad, case.opad, precision=precision)


def _run(case, x, w, b, dy, precision):
    """y, dx, dw, db of one engine call and its backward"""
    xe, we, be = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    y = _engine_op(case, xe, we, be, precision)
    y.backward(dy.to(y.dtype))
    return {"y": y.detach(), "dx": xe.grad, "dw": we.grad, "db": be.grad}


def _check(tag, got, exact, bnd, whats=ALL):
    ratios = {w: G.ratio(got[w], exact[w], bnd[w]) for w in whats}
    print(f"[strided] {tag}: " + " ".join(f"{w}={r:.4f}" for w, r in ratios.items()))
    for w, r in ratios.items():
        assert r <= 1.0, f"{tag}: {w} error is {r:.3g} x its bound"
    return ratios


def _wgrad_spans(fn):
    """names of the weight-gradient spans that ran inside fn()"""
    from openstereo_amd import timing
    rec = timing.enable()
    try:
        out = fn()
        torch.cuda.synchronize()
        names = [key[0] for key, _, _ in rec if key[0].startswith("wgrad")]
    finally:
        timing.disable()
    return out, names


def _on_device(ref):
    return (t.to(DEV) for t in (ref.x, ref.w, ref.b, ref.dy))


def _split_wgrad_covers(case):
    """the workspace query of the split-precision / fp16 weight-gradient kernel: non-zero where its class mode covers the layer"""
    from openstereo_amd import _lib
    lift = lambda v, unit: ((unit,) * (3 - len(v))) + tuple(v)
    n = G.nd(case)
    return _lib.load().osa_conv3d_wgrad_f16x3_workspace_bytes(G.BATCH, *lift(case.dims, 1), case.ci, *lift(G.out_dims(case), 1), case.co,
                                                              *lift((case.k,) * n, 1), 2, *lift((case.pad,) * n, 0), 1, 1, 1, int(G.transposed(case))) > 0


@pytest.mark.parametrize("cid", G.IDS)
def test_every_case_is_admitted_in_training_mode(cid):
    """the table stays inside the domain engine_convs routes to the kernels"""
    from openstereo_amd import autograd as AG
    case = G.BY_ID[cid]
    m = G.module_of(case).to(DEV).train()
    x = torch.zeros((G.BATCH, case.ci) + case.dims, device=DEV, requires_grad=True)
    assert m.bias is not None and torch.is_grad_enabled() and AG._eligible(m, x)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("cid", G.IDS)
def test_forward_dgrad_wgrad_vs_float64(cid, precision):
    """the shipped defaults: y and dx in the requested arithmetic, dw on the exact fp32 class-mode kernel in both modes"""
    from openstereo_amd import autograd as AG
    case = G.BY_ID[cid]
    ref = G.reference(case)
    x, w, b, dy = _on_device(ref)
    assert not AG.WGRAD_F16X3_CLASS
    got, spans = _wgrad_spans(lambda: _run(case, x, w, b, dy, precision))
    _check(f"{cid} [{precision}]", got, ref.exact, G.bounds(case, ref, precision))
    again = _run(case, x, w, b, dy, precision)
    for what in ALL:
        assert torch.equal(got[what], again[what]), f"{cid} [{precision}]: {what} differs between two runs"
    assert spans == ["wgrad"], spans


@pytest.mark.parametrize("cid", G.IDS)
def test_f16x3_class_mode_weight_gradient(cid):
    """WGRAD_F16X3_CLASS on: the split-precision kernel on the parity sub-lattices where its workspace query says it covers the layer
    (dw under the f16x3 bound), a declined launch falling through to the exact kernel everywhere else (dw under the f32 bound)"""
    from openstereo_amd import autograd as AG
    case = G.BY_ID[cid]
    ref = G.reference(case)
    x, w, b, dy = _on_device(ref)
    covered = _split_wgrad_covers(case)
    old = AG.WGRAD_F16X3_CLASS
    AG.WGRAD_F16X3_CLASS = True
    try:
        got, spans = _wgrad_spans(lambda: _run(case, x, w, b, dy, "f16x3"))
        again = _run(case, x, w, b, dy, "f16x3")
    finally:
        AG.WGRAD_F16X3_CLASS = old
    assert spans == (["wgrad_f16x3"] if covered else ["wgrad_f16x3", "wgrad"]), (covered, spans)
    _check(f"{cid} [f16x3, class-mode dw {'split' if covered else 'declined: exact'}]", got, ref.exact, G.bounds(case, ref, "f16x3", dw_split=covered))
    assert torch.equal(got["dw"], again["dw"])


@pytest.mark.parametrize("cid", G.F16_IDS)
def test_native_f16_with_fp32_tensors(cid):
    """the native f16 mode on fp32 tensors (these layers never take the fp16-tensor path): operands are rounded to fp16 when they are
    staged, so y and dx are those of the rounded operands; so is dw where the fp16 class-mode kernel ran.  Where it declined, the exact
    fp32 kernel reads the tensors as they are and dw is that of the unrounded x and dy; db always sums the fp32 dy as it is."""
    from openstereo_amd import autograd as AG
    case = G.BY_ID[cid]
    ref, r16 = G.reference(case), G.reference(case, rounded=True)
    x, w, b, dy = _on_device(ref)
    assert not AG._native_f16(x, w, 2, "f16", 1) and not AG._native_f16(x.half(), w, 2, "f16", 1)
    got, spans = _wgrad_spans(lambda: _run(case, x, w, b, dy, "f16"))
    assert all(got[k].dtype == torch.float32 for k in ALL)
    assert spans in (["wgrad_f16"], ["wgrad_f16", "wgrad"], ["wgrad"]), spans          # (["wgrad"]: class mode switched off, OSA_WGRAD_F16_CLASS=0)
    fp16_kernel = spans[0] == "wgrad_f16" and "wgrad" not in spans
    print(f"[strided] {cid} [f16, fp32 tensors]: weight-gradient spans {spans}, workspace query covers: {_split_wgrad_covers(case)}")
    _check(f"{cid} [f16, fp32 tensors]", got, r16.exact, G.bounds(case, r16, "f32"), ("y", "dx"))
    if fp16_kernel:
        _check(f"{cid} [f16, fp32 tensors, fp16 weight gradient]", got, r16.exact, G.bounds(case, r16, "f32"), ("dw",))
    else:
        _check(f"{cid} [f16, fp32 tensors, exact weight gradient]", got, ref.exact, G.bounds(case, ref, "f32"), ("dw",))
    _check(f"{cid} [f16, fp32 tensors, bias gradient]", got, ref.exact, G.bounds(case, ref, "f32"), ("db",))


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_hourglass_modules_inside_engine_convs(precision):
    """two stride-2 Conv3d and two ConvTranspose3d modules (k3 and k4) with in-place ReLUs between them, in train mode inside engine_convs:
    every layer is checked where it stands -- its output, its data gradient and its parameter gradients against float64 of the tensors that
    went into THAT layer in this run (captured by hooks), under the layer's own bound.  No bound summed through the network: the per-layer
    check is the one a misplaced tap cannot hide in."""
    from openstereo_amd import autograd as AG, engine
    net = G.make_net().to(DEV).train()
    convs = [m for m in net if not isinstance(m, nn.ReLU)]
    x, g = (t.to(DEV) for t in G.net_inputs())
    x.requires_grad_()
    seen = {}

    def capture(m, args, out):
        rec = seen[m] = {"x": args[0].detach().clone(), "y": out.detach().clone()}
        out.register_hook(lambda gr: rec.__setitem__("dy", gr.detach().clone()))       # (registered before the in-place ReLU: the gradient of the layer's own output)
    hooks = [m.register_forward_hook(capture) for m in convs]
    old = engine.get_precision()
    engine.set_precision(precision)
    try:
        with AG.engine_convs():
            dims = G.NET_IN[2:]
            for i, m in enumerate(convs):
                assert AG._eligible(m, torch.zeros((G.BATCH, m.in_channels) + tuple(dims), device=DEV, requires_grad=True)), i
                dims = G.out_dims(G.case_of_module("", m, dims))
            le = (net(x) * g).mean()
        _, spans = _wgrad_spans(le.backward)
    finally:
        engine.set_precision(old)
        for h in hooks:
            h.remove()
    assert spans == ["wgrad"] * len(convs), spans                                      # the engine's exact class-mode weight-gradient kernel, once per layer
    for i, m in enumerate(convs):
        rec = seen[m]
        case = G.case_of_module(f"net.{i}", m, rec["x"].shape[2:])
        assert tuple(rec["y"].shape[2:]) == G.out_dims(case)
        exact, sums = G.exact_and_sums(case, rec["x"], m.weight, m.bias, rec["dy"])
        # (the range block of a layer's input may cover the values before the in-place ReLU: that maximum enters the f16x3 bound's absolute term)
        xmax = rec["x"].cpu() if i == 0 else torch.maximum(rec["x"], seen[convs[i - 1]]["y"].abs()).cpu()
        bnd = G.bounds(case, G.Ref(xmax, m.weight.detach().cpu(), None, rec["dy"].cpu(), exact, sums), precision)
        dx = x.grad if i == 0 else seen[convs[i - 1]]["dy"]
        if i:                                      # what arrives at the previous layer's output went through the ReLU's mask
            mask = (seen[convs[i - 1]]["y"] > 0).double().cpu()
            exact["dx"], bnd["dx"] = exact["dx"] * mask, bnd["dx"] * mask
        _check(f"net layer {i} {case.kind} k{case.k} [{precision}]", {"y": rec["y"], "dx": dx, "dw": m.weight.grad, "db": m.bias.grad}, exact, bnd)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_one_transposed_weight_three_uses(precision):
    """the spx head's weight applied to three inputs in one graph: with DEFER_WGRAD one weight-gradient launch over the three queued pairs,
    without it three launches added up by autograd; both are the float64 sum of the three within the f32 bound of three times as many
    terms, and so is the bias gradient (three osa_channel_sums passes added up)"""
    from openstereo_amd import autograd as AG
    case = G.BY_ID["t2_k4_64_9"]
    refs = [G.reference(case, salt) for salt in range(3)]
    w, b = refs[0].w.to(DEV), refs[0].b.to(DEV)
    exact = {k: sum(r.exact[k] for r in refs) for k in ("dw", "db")}
    bnd = {k: G.bound_f32(sum(r.sums[k] for r in refs), 3 * G.terms(case, k)) for k in ("dw", "db")}

    def run():
        we, be = w.clone().requires_grad_(), b.clone().requires_grad_()
        xs = [r.x.to(DEV).requires_grad_() for r in refs]
        ys = [_engine_op(case, xe, we, be, precision) for xe in xs]
        torch.autograd.backward(ys, [r.dy.to(DEV) for r in refs])
        return {"dw": we.grad, "db": be.grad, "dx": [xe.grad for xe in xs]}
    old = AG.DEFER_WGRAD
    try:
        AG.DEFER_WGRAD = True
        got, spans = _wgrad_spans(run)
        AG.DEFER_WGRAD = False
        apart, spans_apart = _wgrad_spans(run)
    finally:
        AG.DEFER_WGRAD = old
    assert spans == ["wgrad"] and spans_apart == ["wgrad"] * 3, (spans, spans_apart)
    _check(f"{case.id} x3 deferred [{precision}]", got, exact, bnd, ("dw", "db"))
    _check(f"{case.id} x3 apart [{precision}]", apart, exact, bnd, ("dw", "db"))
    for res, tag in ((got, "deferred"), (apart, "apart")):
        for i, r in enumerate(refs):
            _check(f"{case.id} x3 {tag} dx[{i}] [{precision}]", {"dx": res["dx"][i]}, r.exact, G.bounds(case, r, precision), ("dx",))


@pytest.mark.parametrize("mode", ["grad", "no_grad"])
@pytest.mark.parametrize("name", G.GPU_DECLINED)
def test_layers_outside_the_domain_stay_on_torch(name, mode):
    """inside engine_convs a stride-2 Conv3d on an odd dim, a ConvTranspose3d with k3/p1/op0 and a stride-2 Conv2d are left to torch:
    bit-identical to the plain module, with and without gradients, and backward() works"""
    from openstereo_amd import autograd as AG, engine
    _, args, shape = next(c for c in G.DECLINED if c[0] == name)
    m = G.make_module(*args)
    with torch.no_grad():
        m.weight.mul_(3.0)
    m = m.to(DEV)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    if mode == "grad":
        x.requires_grad_()
    old, old_det = engine.get_precision(), torch.backends.cudnn.deterministic
    engine.set_precision("f32")
    torch.backends.cudnn.deterministic = True          # torch's own convolution: the same solver for every call, so that "left to torch" can be told by the bits
    try:
        with torch.set_grad_enabled(mode == "grad"):
            m(x)                                       # (the first call of a new shape searches for a solver)
            plain = m(x)
            with AG.engine_convs():
                assert not AG._eligible(m, x)
                y = m(x)
        assert torch.equal(y, plain)
        if mode == "grad":
            y.sum().backward()
            assert x.grad is not None and m.weight.grad is not None and m.bias.grad is not None
            assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(m.weight.grad).all())
    finally:
        engine.set_precision(old)
        torch.backends.cudnn.deterministic = old_det


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_direct_stride2_forward_on_odd_dims_without_gradients(precision):
    """a direct AG.conv3d(.., stride=2) under no_grad on odd dims (inference runs this launch at odd sizes; only the data gradient needs
    even ones): y against float64"""
    from openstereo_amd import autograd as AG
    case = G.Case("s2_odd_forward_only", "conv3d_s2", 3, 1, None, 8, 8, (5, 7, 9), ())
    assert G.out_dims(case) == (3, 4, 5)
    x, w, b, _ = G.inputs(case)
    exact = G.op(case, x.double(), w.double(), b.double())
    S = G.op(case, x.double().abs(), w.double().abs(), b.double().abs())
    K = G.terms(case, "y")
    bnd = G.bound_f32(S, K) if precision == "f32" else G.bound_f16x3(S, K, x.abs().max(), w.abs().max())
    with torch.no_grad():
        y = AG.conv3d(x.to(DEV), w.to(DEV), b.to(DEV), 2, 1, 1, precision=precision)
        again = AG.conv3d(x.to(DEV), w.to(DEV), b.to(DEV), 2, 1, 1, precision=precision)
    _check(f"{case.id} [{precision}]", {"y": y}, {"y": exact}, {"y": bnd}, ("y",))
    assert torch.equal(y, again)
