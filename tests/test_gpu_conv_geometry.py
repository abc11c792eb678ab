"""Forward, data gradient and weight gradient of the training convolutions over the geometries `autograd._eligible` admits -- anisotropic
kernels and paddings, dilation, "valid" and over-padded layers, even kernels, 49 taps, depth-only kernels -- against the float64 reference
and under the bounds of tests/conv_geometry_cases.py (derived there from the number formats); and the edge of the admitted domain: layers the
kernels cannot take stay torch modules whatever the gradient mode.  Every test prints its error / bound ratios."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_geometry_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _module(case):
    return (nn.Conv2d if G.flat(case) else nn.Conv3d)(case.ci, case.co, case.k, 1, case.pad, case.dil)


def _engine_conv(case):
    from openstereo_amd import autograd as AG
    return AG.conv2d if G.flat(case) else AG.conv3d


def _run(case, x, w, b, dy, precision):
    """y, dx, dw, db of one engine call and its backward"""
    xe, we, be = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    y = _engine_conv(case)(xe, we, be, 1, case.pad, case.dil, precision=precision)
    y.backward(dy.to(y.dtype))
    return {"y": y.detach(), "dx": xe.grad, "dw": we.grad, "db": be.grad}


def _check(tag, got, exact, bnd, whats=("y", "dx", "dw", "db")):
    ratios = {w: G.ratio(got[w], exact[w], bnd[w]) for w in whats}
    print(f"[geometry] {tag}: " + " ".join(f"{w}={r:.4f}" for w, r in ratios.items()))
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


@pytest.mark.parametrize("cid", G.IDS)
def test_every_case_is_admitted_in_training_mode(cid):
    """the table stays inside the domain engine_convs routes to the kernels"""
    from openstereo_amd import autograd as AG
    case = G.BY_ID[cid]
    m = _module(case).to(DEV).train()
    x = torch.zeros((G.BATCH, case.ci) + case.dims, device=DEV, requires_grad=True)
    assert torch.is_grad_enabled() and AG._eligible(m, x)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("cid", G.IDS)
def test_forward_dgrad_wgrad_vs_float64(cid, precision):
    from openstereo_amd import _lib
    case = G.BY_ID[cid]
    ref = G.reference(case)
    x, w, b, dy = (t.to(DEV) for t in (ref.x, ref.w, ref.b, ref.dy))
    got, spans = _wgrad_spans(lambda: _run(case, x, w, b, dy, precision))
    _check(f"{cid} [{precision}]", got, ref.exact, G.bounds(case, ref, precision))
    again = _run(case, x, w, b, dy, precision)
    for what in ("y", "dx", "dw", "db"):
        assert torch.equal(got[what], again[what]), f"{cid} [{precision}]: {what} differs between two runs"
    # which weight-gradient kernel ran: the workspace query of the split-precision form says what it covers, the spans say what was launched
    k, pad, dil = G.lift(case)
    D, H, W = ((1,) + case.dims) if G.flat(case) else case.dims
    Do, Ho, Wo = ((1,) + G.out_dims(case)) if G.flat(case) else G.out_dims(case)
    covered = _lib.load().osa_conv3d_wgrad_f16x3_workspace_bytes(G.BATCH, D, H, W, case.ci, Do, Ho, Wo, case.co, *k, 1, *pad, *dil, 0) > 0
    assert covered == G.wgrad_is_split(case)
    if precision == "f16x3":
        assert spans == (["wgrad_f16x3"] if covered else ["wgrad_f16x3", "wgrad"]), spans     # (a declined split launch falls through to the exact kernel)
    else:
        assert spans == ["wgrad"], spans


@pytest.mark.parametrize("cid", ["f_3x3_valid", "g_3x3_overpadded", "m_1x3x3", "r_3x3x3_pad_2_0_1"])
def test_native_f16_with_fp16_tensors(cid):
    """the fp16-tensor path (_Conv3dF16IO) against float64 on the fp16-rounded operands; results stored in fp16 carry that format's rounding"""
    from openstereo_amd import autograd as AG
    case = G.BY_ID[cid]
    ref = G.reference(case, rounded=True)
    x, w, b, dy = (t.to(DEV) for t in (ref.x, ref.w, ref.b, ref.dy))
    assert AG._native_f16(x.half(), w, 1, "f16", case.dil)
    got = _run(case, x.half(), w, b, dy, "f16")
    bnd = G.bounds(case, ref, "f32")
    for what in ("y", "dx"):
        if got[what].dtype == torch.float16:
            bnd[what] = G.stored_f16(bnd[what], ref.exact[what])
    assert got["dx"].dtype == torch.float16 and got["dw"].dtype == torch.float32
    exact = dict(ref.exact)
    if got["y"].dtype != torch.float16:
        exact["db"] = G.reference(case).exact["db"]                 # the bias gradient sums the fp32 dy tensor as it is
    _check(f"{cid} [f16, fp16 tensors, y {got['y'].dtype}]", got, exact, bnd)
    again = _run(case, x.half(), w, b, dy, "f16")
    assert torch.equal(got["dx"], again["dx"]) and torch.equal(got["dw"], again["dw"])


@pytest.mark.parametrize("cid", ["a_1x5_gru_row", "d_3x3_dil2"])
def test_native_f16_with_fp32_tensors(cid):
    """layers the fp16-tensor path declines (5 taps on an axis, dilation): operands are rounded to fp16 when they are staged, so y and dx are
    those of the rounded operands; the fp16 weight-gradient kernel declines them too and the exact fp32 kernel reads the tensors as they are,
    so dw is that of the unrounded x and dy (autograd._wgrad)"""
    from openstereo_amd import autograd as AG
    case = G.BY_ID[cid]
    ref, r16 = G.reference(case), G.reference(case, rounded=True)
    x, w, b, dy = (t.to(DEV) for t in (ref.x, ref.w, ref.b, ref.dy))
    assert not AG._native_f16(x, w, 1, "f16", case.dil) and not AG._native_f16(x.half(), w, 1, "f16", case.dil) and not G.wgrad_is_split(case)
    got, spans = _wgrad_spans(lambda: _run(case, x, w, b, dy, "f16"))
    assert spans == ["wgrad_f16", "wgrad"], spans
    _check(f"{cid} [f16, fp32 tensors]", got, r16.exact, G.bounds(case, r16, "f32"), ("y", "dx"))
    _check(f"{cid} [f16, fp32 tensors, exact weight gradient]", got, ref.exact, G.bounds(case, ref, "f32"), ("dw", "db"))
    print(f"[geometry] {cid} [f16, fp32 tensors]: dw against the rounded-operand reference = "
          f"{G.ratio(got['dw'], r16.exact['dw'], G.bounds(case, r16, 'f32')['dw']):.4f} (reported)")


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("cid", ["a_1x5_gru_row", "b_5x1_gru_col", "d_3x3_dil2"])
def test_one_weight_three_uses_one_deferred_weight_gradient(cid, precision):
    """the same weight applied to three inputs in one graph: with DEFER_WGRAD one weight-gradient launch over the three queued pairs
    (osa_conv3d_wgrad_ws_multi) returns the float64 sum of the three.  `_defer_wgrad` promises the same SUM, not the same bits, as three
    launches added up by autograd (another summation order), so the undeferred result is held to the same bound."""
    from openstereo_amd import autograd as AG
    case = G.BY_ID[cid]
    refs = [G.reference(case, salt) for salt in range(3)]
    w, b = refs[0].w.to(DEV), refs[0].b.to(DEV)
    exact = {k: sum(r.exact[k] for r in refs) for k in ("dw", "db")}
    sums = {k: sum(r.sums[k] for r in refs) for k in ("dw", "db")}
    K = 3 * G.terms(case, "dw")
    bnd = {k: G.bound_f32(sums[k], K) for k in ("dw", "db")}          # (these layers take the exact fp32 weight-gradient kernel in both modes)
    assert not G.wgrad_is_split(case)

    def run():
        we, be = w.clone().requires_grad_(), b.clone().requires_grad_()
        xs = [r.x.to(DEV).requires_grad_() for r in refs]
        ys = [_engine_conv(case)(xe, we, be, 1, case.pad, case.dil, precision=precision) for xe in xs]
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
    assert spans.count("wgrad") == 1 and spans_apart.count("wgrad") == 3, (spans, spans_apart)
    _check(f"{cid} x3 deferred [{precision}]", got, exact, bnd, ("dw", "db"))
    _check(f"{cid} x3 apart [{precision}]", apart, exact, bnd, ("dw", "db"))
    for i, r in enumerate(refs):
        _check(f"{cid} x3 dx[{i}] [{precision}]", {"dx": got["dx"][i]}, r.exact, G.bounds(case, r, precision), ("dx",))


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_conv2d_pair_on_the_row_kernel(precision):
    """two 1x5 weights stacked into one layer (conv2d_pair): y, dx and both weights' gradients against float64"""
    from openstereo_amd import autograd as AG
    from openstereo_amd.utils.weights import synth_tensor
    case = G.BY_ID["a_1x5_gru_row"]
    ref = G.reference(case)
    w2 = synth_tensor("pair.second.w", tuple(ref.w.shape), 1) * 3.0
    dy2 = torch.roll(ref.dy, (1, 2), (1, 3)) * 0.75
    both = case._replace(co=2 * case.co)
    exact, sums = G.exact_and_sums(both, ref.x, torch.cat([ref.w, w2], 0), torch.zeros(2 * case.co), torch.cat([ref.dy, dy2], 1))
    pair = G.Ref(ref.x, torch.cat([ref.w, w2], 0), torch.zeros(2 * case.co), torch.cat([ref.dy, dy2], 1), exact, sums)
    xe, wa, wb = ref.x.to(DEV).requires_grad_(), ref.w.to(DEV).requires_grad_(), w2.to(DEV).requires_grad_()
    y = AG.conv2d_pair(xe, wa, wb, case.pad, case.dil, precision=precision)
    y.backward(pair.dy.to(DEV))
    got = {"y": y.detach(), "dx": xe.grad, "dw": torch.cat([wa.grad, wb.grad], 0)}
    _check(f"conv2d_pair 1x5 [{precision}]", got, exact, G.bounds(both, pair, precision), ("y", "dx", "dw"))


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_sequential_of_conv2d_modules_inside_engine_convs(precision):
    """nn.Conv2d modules of geometries a, b, d, e, f with in-place ReLUs between them, in train mode inside engine_convs.
    (1) Loss and every parameter gradient against the float64 run of the same modules, under the layers' bounds summed through the network
    (G.net_reference).  That sum is a worst case over five layers and grows far beyond a gradient's size for the early ones, so
    (2) every layer is also checked where it stands: its output, its data gradient and its parameter gradients against float64 of the tensors
    that went into THAT layer in this run (captured by hooks), under the layer's own bound -- a misplaced tap cannot hide there."""
    from openstereo_amd import autograd as AG, engine
    loss, grads, lb, gb = G.net_reference(precision)
    net = G.make_net().to(DEV).train()
    convs = [m for m in net if isinstance(m, nn.Conv2d)]
    x, g = (t.to(DEV) for t in G.net_inputs())
    x.requires_grad_()
    seen = {}

    def capture(m, args, out):
        rec = seen[m] = {"x": args[0].detach().clone(), "y": out.detach().clone()}
        out.register_hook(lambda gr: rec.__setitem__("dy", gr.detach().clone()))       # (registered before the in-place ReLU: the gradient of the conv's own output)
    hooks = [m.register_forward_hook(capture) for m in convs]
    old = engine.get_precision()
    engine.set_precision(precision)
    try:
        with AG.engine_convs():
            assert all(AG._eligible(m, torch.zeros((G.BATCH, m.in_channels, 13, 37), device=DEV, requires_grad=True)) for m in convs)
            le = (net(x) * g).mean()
        _, spans = _wgrad_spans(le.backward)
    finally:
        engine.set_precision(old)
        for h in hooks:
            h.remove()
    assert len([s for s in spans if s in ("wgrad", "wgrad_f16x3")]) >= len(convs), spans      # the engine's weight-gradient kernels ran
    print(f"[geometry] net [{precision}]: loss error / summed bound = {abs(float(le.detach()) - loss) / lb:.3g}")
    assert abs(float(le.detach()) - loss) <= lb
    ratios = {n: G.ratio(p.grad, grads[n], gb[n]) for n, p in net.named_parameters()}
    print(f"[geometry] net [{precision}] summed bounds: " + " ".join(f"{n}={r:.3g}" for n, r in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    for i, m in enumerate(convs):
        rec = seen[m]
        case = G.Case(f"net.{i}", m.kernel_size, m.padding, m.dilation, m.in_channels, m.out_channels, tuple(rec["x"].shape[2:]), ())
        exact, sums = G.exact_and_sums(case, rec["x"], m.weight, m.bias, rec["dy"])
        # (the range block of a layer's input covers the values before the in-place ReLU: that maximum enters the f16x3 bound's absolute term)
        xmax = rec["x"].cpu() if i == 0 else torch.maximum(rec["x"], seen[convs[i - 1]]["y"].abs()).cpu()
        bnd = G.bounds(case, G.Ref(xmax, m.weight.detach().cpu(), None, rec["dy"].cpu(), exact, sums), precision)
        dx = x.grad if i == 0 else seen[convs[i - 1]]["dy"]
        if i:                                      # what arrives at the previous conv's output went through the ReLU's mask
            mask = (seen[convs[i - 1]]["y"] > 0).double().cpu()
            exact["dx"], bnd["dx"] = exact["dx"] * mask, bnd["dx"] * mask
        _check(f"net layer {i} [{precision}]", {"y": rec["y"], "dx": dx, "dw": m.weight.grad, "db": m.bias.grad}, exact, bnd)


def _declined(name):
    _, (kind, ci, co, k, s, p, d), shape = next(c for c in G.DECLINED if c[0] == name)
    m = getattr(nn, kind)(ci, co, k, s, p, d)
    with torch.no_grad():
        m.weight.mul_(3.0)
    return m.to(DEV), torch.randn(shape, generator=torch.Generator().manual_seed(9)).to(DEV)


@pytest.mark.parametrize("mode", ["grad", "no_grad", "frozen"])
@pytest.mark.parametrize("name", [c[0] for c in G.DECLINED])
def test_layers_the_kernels_cannot_take_stay_on_torch(name, mode):
    """inside engine_convs a layer beyond the kernels' limits (more than 64 taps, a staged brick beyond the LDS) never raises: it returns
    what the plain module returns -- bit-identical when it is left to torch, within the f32 bound when the engine takes it; and a layer
    that is taken without gradients also works with them"""
    from openstereo_amd import autograd as AG, engine
    m, x = _declined(name)
    conv = F.conv2d if isinstance(m, nn.Conv2d) else F.conv3d
    if mode == "frozen":
        m.requires_grad_(False)
    elif mode == "grad":
        x.requires_grad_()
    old, old_det = engine.get_precision(), torch.backends.cudnn.deterministic
    engine.set_precision("f32")
    torch.backends.cudnn.deterministic = True          # torch's own convolution: the same solver for every call, so that "left to torch" can be told by the bits
    try:
        with torch.set_grad_enabled(mode != "no_grad"):
            m(x)                                       # (the first call of a new shape searches for a solver)
            plain = m(x)
            with AG.engine_convs():
                taken = AG._eligible(m, x)
                y = m(x)
        print(f"[geometry] {name} [{mode}]: {'engine' if taken else 'torch'}")
        if not taken:
            assert torch.equal(y, plain)
        else:
            d = lambda t: t.detach().double().cpu()
            exact = conv(d(x), d(m.weight), d(m.bias), 1, m.padding, m.dilation)
            S = conv(d(x).abs(), d(m.weight).abs(), d(m.bias).abs(), 1, m.padding, m.dilation)
            r = G.ratio(y, exact, G.bound_f32(S, m.in_channels * m.weight[0, 0].numel()))
            print(f"[geometry] {name} [{mode}]: y={r:.4f}")
            assert r <= 1.0
            # the same layer with gradients: must work as well, on whichever side eligibility puts it
            xg = x.detach().clone().requires_grad_()
            m.requires_grad_(True)
            with torch.enable_grad(), AG.engine_convs():
                yg = m(xg)
            yg.sum().backward()
            assert xg.grad is not None and m.weight.grad is not None and bool(torch.isfinite(m.weight.grad).all())
        if mode == "grad":
            y.sum().backward()
            assert x.grad is not None and m.weight.grad is not None
    finally:
        engine.set_precision(old)
        torch.backends.cudnn.deterministic = old_det
    # more than 64 taps: no kernel form exists, whatever the mode
    if "taps" in name:
        assert not taken
