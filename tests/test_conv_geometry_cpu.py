"""The table of tests/conv_geometry_cases.py checked without a GPU: torch's own float32 convolution on the CPU stays inside the f32 bound of
the float64 reference on every case (so the reference alone does not use up the bound), and every deliberately wrong result -- an unflipped
axis in dx, swapped paddings, an ignored dilation, a dropped tap, two exchanged taps in dw, a shift by one position -- leaves even the
widest bound (f16x3) on every case it applies to."""
import pytest
import torch

import conv_geometry_cases as G


@pytest.mark.parametrize("cid", G.IDS)
def test_float32_cpu_convolution_is_inside_the_f32_bound(cid):
    case = G.BY_ID[cid]
    ref = G.reference(case)
    got = G._grads(case, ref.x, ref.w, ref.b, ref.dy)
    bnd = G.bounds(case, ref, "f32")
    for what in ("y", "dx", "dw", "db"):
        r = G.ratio(got[what], ref.exact[what], bnd[what])
        print(f"{cid} {what}: float32 error / bound = {r:.3f}")
        assert r <= 1.0, (cid, what, r)


@pytest.mark.parametrize("cid", G.IDS)
def test_every_wrong_result_leaves_the_widest_bound(cid):
    case = G.BY_ID[cid]
    ref = G.reference(case)
    wrong = G.wrong_results(case)
    missing = [n for n in case.must_see if n not in wrong]
    assert not missing, f"{cid} is listed for {missing}, which its geometry cannot show: change the case"
    bnd = G.bounds(case, ref, "f16x3")
    wide = {w: torch.maximum(bnd[w], G.bounds(case, ref, "f32")[w]) for w in bnd}
    for name, (what, value) in wrong.items():
        r = G.ratio(value, ref.exact[what], wide[what])
        print(f"{cid} {name}: wrong {what} error / bound = {r:.3g}")
        assert r > 100.0, f"{cid}: the wrong result '{name}' is within {r:.3g} of the bound of {what}: the case cannot see it"


def test_table_covers_what_the_issue_lists():
    """the geometric properties the cases are there for, stated on the table itself"""
    by = G.BY_ID
    off = lambda c: [(min(o[a] for o in G.tap_offsets(*G.lift(c))), max(o[a] for o in G.tap_offsets(*G.lift(c)))) for a in range(3)]
    assert off(by["a_1x5_gru_row"])[1] != off(by["a_1x5_gru_row"])[2]                      # hmin != wmin
    assert G.taps(by["c_7x7_49taps"]) == 49 and 49 % 9 == 4 and 49 % 3 != 0              # partial last tap group
    assert all(lo >= 0 for lo, _ in off(by["f_3x3_valid"]))                                # offsets all non-negative
    assert all(hi <= 0 for _, hi in off(by["j_2x2_pad1"])[1:])                             # offsets all non-positive
    k, pad, dil = G.lift(by["i_1x1_pad1"])
    assert [d * (kk - 1) - p for kk, p, d in zip(k, pad, dil)][1:] == [-1, -1]             # negative data-gradient padding
    assert G.out_dims(by["o_3x3x3_valid"])[0] == 1                                         # output depth collapses
    assert G.out_dims(by["g_3x3_overpadded"]) > by["g_3x3_overpadded"].dims
    signs = [lo for lo, _ in off(by["r_3x3x3_pad_2_0_1"])]
    assert signs[0] < 0 and signs[1] == 0 and signs[2] < 0 and len(set(signs)) == 3
    assert by["l_3x2_anisotropic"].ci % 4 and by["e_3x3_dil4"].co % 4 == 0 and by["e_3x3_dil4"].co % 8
    assert {c.id for c in G.CASES if G.wgrad_is_split(c)} >= {"f_3x3_valid", "g_3x3_overpadded", "h_3x3_pad_0_1", "j_2x2_pad1", "m_1x3x3", "n_3x1x1",
                                                               "o_3x3x3_valid", "r_3x3x3_pad_2_0_1"}
    assert not any(G.wgrad_is_split(by[i]) for i in ("a_1x5_gru_row", "b_5x1_gru_col", "c_7x7_49taps", "d_3x3_dil2", "e_3x3_dil4", "k_4x4_pad1",
                                                      "l_3x2_anisotropic", "p_3x3x3_dilated_planes"))


def test_network_reference_is_reproduced_by_float32_within_its_bound():
    loss, grads, lb, gb = G.net_reference("f32")
    net = G.make_net()
    x, g = G.net_inputs()
    l32 = (net(x) * g).mean()
    l32.backward()
    assert abs(float(l32.detach()) - loss) <= lb, (float(l32.detach()), loss, lb)
    for n, p in net.named_parameters():
        r = G.ratio(p.grad, grads[n], gb[n])
        print(f"net {n}: float32 error / bound = {r:.3f}")
        assert r <= 1.0, (n, r)


def _fake(shape, requires_grad):
    return type("T", (), {"shape": shape, "requires_grad": requires_grad})()


def _declined(name):
    import torch.nn as nn
    _, (kind, ci, co, k, s, p, d), shape = next(c for c in G.DECLINED if c[0] == name)
    return getattr(nn, kind)(ci, co, k, s, p, d), shape


def test_library_answers_for_the_forward_launch_of_every_case_and_of_its_data_gradient():
    """osa_conv3d_supported (host arithmetic, no GPU): every case of the table and its role-swapped data gradient -- negative padding for
    i_1x1_pad1 -- in the three arithmetic modes; more than 64 taps, tap offsets beyond a signed byte and a brick beyond the LDS are refused"""
    from openstereo_amd import _lib
    ok = _lib.load().osa_conv3d_supported
    for c in G.CASES:
        k, p, d = G.lift(c)
        sp, out = (((1,) + v) if G.flat(c) else v for v in (c.dims, G.out_dims(c)))
        p2 = [d[i] * (k[i] - 1) - p[i] for i in range(3)]
        for prec in (0, 1, 2):
            assert ok(G.BATCH, *sp, c.ci, c.co, *k, 1, *p, *d, prec) == 1, (c.id, prec)
            assert ok(G.BATCH, *out, c.co, c.ci, *k, 1, *p2, *d, prec) == 1, (c.id, prec, "data gradient")
    assert ok(2, 1, 12, 14, 8, 8, 1, 9, 9, 1, 0, 4, 4, 1, 1, 1, 0) == 0                      # 81 taps
    assert ok(1, 6, 7, 9, 8, 8, 5, 5, 5, 1, 2, 2, 2, 1, 1, 1, 0) == 0                       # 125 taps
    assert ok(1, 1, 90, 94, 128, 128, 1, 3, 3, 1, 0, 40, 40, 1, 40, 40, 0) == 0             # 1 x 84 x 88 brick
    assert ok(1, 1, 300, 300, 8, 8, 1, 3, 3, 1, 0, 0, 0, 1, 100, 100, 0) == 0               # tap offset 200
    assert ok(1, 1, 3, 3, 8, 8, 1, 5, 5, 1, 0, 0, 0, 1, 1, 1, 0) == 0                       # empty output


@pytest.mark.parametrize("name", [c[0] for c in G.DECLINED])
def test_eligibility_consults_the_forward_launcher_with_and_without_gradients(name):
    """the preconditions `_eligible` asks for (`_wgrad_ok(..., forward=True)`) under no_grad, for a frozen layer and with gradients: a layer
    with more than 64 taps is never admitted; one whose forward brick fits is admitted without gradients and declined with them when the
    weight-gradient brick does not fit"""
    from openstereo_amd import autograd as AG
    m, shape = _declined(name)
    with torch.no_grad():
        no_grad = AG._wgrad_ok(m, _fake(shape, False), True)
    grad = AG._wgrad_ok(m, _fake(shape, True), True)
    m.requires_grad_(False)
    frozen = AG._wgrad_ok(m, _fake(shape, False), True)
    assert no_grad == frozen and (no_grad or not grad)
    if "taps" in name:
        assert not (no_grad or grad)
    else:
        assert no_grad and not grad


def test_a_forward_brick_beyond_the_lds_is_declined_without_gradients_too():
    """a 3x3 at dilation 40: the forward launcher refuses its 1 x 84 x 88 brick, so the layer stays a torch module under no_grad as well"""
    import torch.nn as nn
    from openstereo_amd import autograd as AG
    m = nn.Conv2d(128, 128, 3, 1, 40, 40)
    with torch.no_grad():
        assert not AG._wgrad_ok(m, _fake((1, 128, 90, 94), False), True)
        assert AG._wgrad_ok(nn.Conv2d(128, 128, 3, 1, 2, 2), _fake((1, 128, 90, 94), False), True)
