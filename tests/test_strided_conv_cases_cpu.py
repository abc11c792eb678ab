"""The table of tests/strided_conv_cases.py checked without a GPU: torch's own float32 stride-2 / transposed convolution on the CPU stays
inside the f32 bound of the float64 reference on every case (so the reference alone does not use up the bound); every deliberately wrong
result -- an unflipped axis, exchanged parity classes, a dropped output_padding, a wrong stride phase, exchanged k = 4 tap pairs, a
replicated edge, a dropped tap, two exchanged taps in dw, a shift by one position -- leaves the wider of the two bounds by more than a
factor 100 on every case it applies to; and the edge of the admitted domain as `autograd._shape_eligible` draws it."""
import numpy as np
import pytest
import torch

import strided_conv_cases as G


@pytest.mark.parametrize("cid", G.IDS)
def test_float32_cpu_result_is_inside_the_f32_bound(cid):
    case = G.BY_ID[cid]
    ref = G.reference(case)
    got = G.grads(case, ref.x, ref.w, ref.b, ref.dy)
    bnd = G.bounds(case, ref, "f32")
    for what in ("y", "dx", "dw", "db"):
        r = G.ratio(got[what], ref.exact[what], bnd[what])
        print(f"{cid} {what}: float32 error / bound = {r:.3f}")
        assert r <= 1.0, (cid, what, r)


@pytest.mark.parametrize("cid", G.IDS)
def test_every_wrong_result_leaves_the_wider_bound(cid):
    case = G.BY_ID[cid]
    ref = G.reference(case)
    wrong = G.wrong_results(case)
    missing = [n for n in case.must_see if n not in wrong]
    assert not missing, f"{cid} is listed for {missing}, which its geometry cannot show: change the case"
    narrow, split = G.bounds(case, ref, "f32"), G.bounds(case, ref, "f16x3", dw_split=True)
    wide = {w: torch.maximum(narrow[w], split[w]) for w in narrow}
    for name, (what, value) in wrong.items():
        r = G.ratio(value, ref.exact[what], wide[what])
        print(f"{cid} {name}: wrong {what} error / bound = {r:.3g}")
        assert r > 100.0, f"{cid}: the wrong result '{name}' is within {r:.3g} of the bound of {what}: the case cannot see it"


def test_table_covers_what_the_issue_lists():
    """the properties the cases are there for, stated on the table itself"""
    by = G.BY_ID
    assert [c.id for c in G.CASES if c.kind == "conv3d_s2"] and all(n % 2 == 0 for c in G.CASES if c.kind == "conv3d_s2" for n in c.dims)
    assert all((c.k, c.pad, c.opad) in ((3, 1, 1), (4, 1, 0)) for c in G.CASES if G.transposed(c))
    assert all((c.k, c.pad, c.opad) == (3, 1, None) for c in G.CASES if not G.transposed(c))
    assert all(G.out_dims(c) == tuple(2 * n for n in c.dims) for c in G.CASES if G.transposed(c))
    # maps of one voxel, one row, one column; one output voxel per item
    assert by["t3_k3_one_voxel"].dims == by["t3_k4_one_voxel"].dims == (1, 1, 1) and by["t2_k3_one_pixel"].dims == (1, 1)
    assert by["t2_k4_one_row"].dims[0] == 1 and by["t2_k4_one_col"].dims[1] == 1 and by["t3_k3_d1"].dims[0] == 1
    assert G.out_dims(by["s2_smallest"]) == (1, 1, 1) and G.out_dims(by["s2_two_ntiles"])[0] == 1
    assert [len(l) for l in G.live_taps(by["s2_smallest"])] == [2, 2, 2]                       # every tap but 8 is padding
    assert G.live_taps(by["t3_k3_one_voxel"]) == [[1, 2]] * 3 and G.live_taps(by["t3_k4_one_voxel"]) == [[1, 2]] * 3
    assert G.live_taps(by["t2_k4_one_row"]) == [[1, 2], [0, 1, 2, 3]]                          # the outer k4 taps never meet a one-row map
    # channel counts off the tiles
    for kind in ("conv3d_s2", "deconv3d", "deconv2d"):
        mine = [c for c in G.CASES if c.kind == kind]
        assert any(c.co % 4 for c in mine) and any(c.co > 32 for c in mine), kind
        assert kind == "deconv2d" or any(c.ci % 4 for c in mine), kind                      # (the flat table has Co = 9 and 5; its Ci are whole 4-channel groups)
    assert by["t3_k3_ragged_ch"].ci % 16 and by["t3_k3_ragged_ch"].ci % 4 == 0 and by["t2_k3_one_pixel"].ci == 4
    assert by["s2_two_ntiles"].co > 64 and by["s2_two_ntiles"].co % 32 and by["t3_k3_two_ntiles"].co % 32 and by["t2_k3_40_out"].co % 32
    # ragged in the bricks: the stride-2 output against 2x4x8, the transposed layers' a-space (= the input map) against 4x4x8
    assert all(n % t for n, t in zip(G.out_dims(by["s2_ragged_ch"]), (2, 4, 8)))
    assert all(n % t for n, t in zip(by["t3_k3_two_ntiles"].dims, (4, 4, 8)))
    assert any(all(n % 2 for n in c.dims) for c in G.CASES if c.kind == "deconv3d" and c.k == 3)
    assert any(any(n % 2 for n in c.dims) for c in G.CASES if c.kind == "deconv3d" and c.k == 4)
    assert any(all(n % 2 for n in c.dims) for c in G.CASES if c.kind == "deconv2d")
    assert set(G.F16_IDS) <= set(G.IDS) and {by[i].kind for i in G.F16_IDS} == {"conv3d_s2", "deconv3d", "deconv2d"}
    # term counts: a transposed layer's taps are accumulated over its INPUT positions
    c = by["t3_k4_48_24"]
    assert G.terms(c, "dw") == G.BATCH * int(np.prod(c.dims)) and G.terms(c, "db") == 8 * G.terms(c, "dw") and G.terms(c, "y") == 48 * 64
    c = by["s2_32_64"]
    assert G.terms(c, "dw") == G.terms(c, "db") == G.BATCH * 4 * 6 * 8 and G.terms(c, "dx") == 64 * 27


def test_network_layers_are_cases_of_the_table_kinds():
    net = G.make_net()
    x, _ = G.net_inputs()
    dims = tuple(x.shape[2:])
    for i, m in enumerate(mm for mm in net if not isinstance(mm, torch.nn.ReLU)):
        case = G.case_of_module(f"net.{i}", m, dims)
        assert m.bias is not None and type(G.module_of(case)) is type(m)
        dims = G.out_dims(case)
    assert dims == tuple(x.shape[2:])
    assert tuple(net(x).shape) == tuple(x.shape)


def _fake(shape, requires_grad=True):
    return type("T", (), {"shape": shape, "requires_grad": requires_grad})()


@pytest.mark.parametrize("cid", G.IDS)
def test_shape_eligible_admits_every_case(cid):
    from openstereo_amd import autograd as AG
    case = G.BY_ID[cid]
    assert AG._shape_eligible(G.module_of(case), _fake((G.BATCH, case.ci) + case.dims))


@pytest.mark.parametrize("name", [c[0] for c in G.DECLINED])
def test_shape_eligible_declines_what_lies_outside(name):
    from openstereo_amd import autograd as AG
    _, args, shape = next(c for c in G.DECLINED if c[0] == name)
    m = G.make_module(*args)
    assert not AG._shape_eligible(m, _fake(shape))
    # the neighbour inside the domain is admitted: the decline is due to the one property the entry is named for
    inside = {"Conv3d": ("Conv3d", 8, 8, 3, 2, 1, None, 1), "ConvTranspose3d": ("ConvTranspose3d", 8, 8, 3, 2, 1, 1, 1),
              "ConvTranspose2d": ("ConvTranspose2d", 4, 8, 4, 2, 1, 0, 1), "Conv2d": ("Conv2d", 8, 8, 3, 1, 1, None, 1)}[args[0]]
    even = shape[:2] + tuple(n + n % 2 for n in shape[2:])
    assert AG._shape_eligible(G.make_module(*inside), _fake((even[0], inside[1]) + even[2:]))
