"""The output-plane-walking form of the fused stride-2 transposed convolutions (csrc/conv_deconv_walk.h): ConvTranspose3d(k = 3, s = 2, p = 1,
op = 1) + BN with the 1x1x1 `redir` branch (Conv3d + BN on the output-resolution tensor) and the activation in one launch, on split tensors --
conv6 + redir1 / conv5 + redir2 of the GwcNet hourglasses (models/gwcnet/hourglass.py:36-56).

Against the layer as the reference computes it (torch fp32 on the CPU), against the brick form of the same launch (osa_deconv_walk(0) selects
it), bit-identical when repeated; the launch counter proves which form ran.  Cases: ragged H / W over several tiles, D = 1 (the only odd
plane sees a zero upper neighbour) and D = 2, D cut into segments, 4 and 8 input chunks, one and two N-tiles, 32 and 64 redir channels, all
three activations, channel slices of wider buffers, and allocations surrounded by NaN."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from openstereo_amd.utils.weights import synth_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(atol=3e-5, rtol=3e-5)

CASES = [
    # name, Ci, Co (= redir channels), (B, D, H, W) of the input, activation
    ("conv6 shape, small", 64, 32, (1, 3, 8, 16), "relu"),
    ("ragged H and W over several tiles", 64, 32, (2, 4, 11, 37), "relu"),
    ("D = 1", 64, 32, (1, 1, 9, 33), "relu"),
    ("D = 2", 64, 32, (1, 2, 8, 34), "leaky"),
    ("many columns: D cut into segments", 64, 32, (3, 12, 20, 40), "relu"),
    ("conv5 shape: 8 chunks, two N-tiles, 64 redir channels", 128, 64, (1, 3, 6, 20), "relu"),
    ("conv5 shape, ragged, several items, no activation", 128, 64, (2, 2, 5, 35), "none"),
    ("no activation", 64, 32, (1, 2, 5, 7), "none"),
    ("32 -> 32 with a 32-channel redir", 32, 32, (1, 3, 7, 30), "leaky"),
]


def _eye(c):
    m = nn.Conv3d(c, c, 1, bias=False)
    m.weight.data = torch.eye(c).reshape(c, c, 1, 1, 1).clone()
    return m


def _bn(c, name):
    bn = nn.BatchNorm3d(c)
    bn.load_state_dict({k: synth_tensor(f"{name}.{k}", v.shape, 2) for k, v in bn.state_dict().items()})
    return bn.eval()


def _layer(name, Ci, Co, act):
    """torch modules, their CPU forward, and the two engine layers"""
    from openstereo_amd.engine import PackedConv3d
    dc = nn.ConvTranspose3d(Ci, Co, 3, stride=2, padding=1, output_padding=1, bias=False)
    dc.weight.data = synth_tensor(name + ".w", dc.weight.shape, 1)
    rc = nn.Conv3d(Co, Co, 1, bias=False)
    rc.weight.data = synth_tensor(name + ".rw", rc.weight.shape, 1)
    bn, rbn = _bn(Co, name + ".bn"), _bn(Co, name + ".rbn")
    actf = {"relu": F.relu, "leaky": lambda t: F.leaky_relu(t, 0.01), "none": lambda t: t}[act]
    ref = lambda x, r: actf(bn(dc(x)) + rbn(rc(r)))
    code = {"none": 0, "relu": 1, "leaky": 2}[act]
    with torch.no_grad():
        gpu = lambda m: copy.deepcopy(m).to(DEV)                    # (the reference stays on the CPU)
        pdc = PackedConv3d(gpu(dc), gpu(bn), code, 0.01, precision="f16x3")
        prl = PackedConv3d(gpu(rc), gpu(rbn), 0, precision="f16x3")
    return ref, pdc, prl


def _inputs(Ci, Co, B, D, H, W, seed=3):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.normal(0, 1, (B, Ci, D, H, W)).astype(np.float32))
    r = torch.from_numpy(rng.normal(0, 1, (B, Co, 2 * D, 2 * H, 2 * W)).astype(np.float32))
    return x, r


def _split(t, out=None, out_off=0):
    """fp32 NCDHW on the CPU -> split NDHWC tensor on the GPU (a 1x1x1 identity layer writes it), optionally into channels of `out`"""
    from openstereo_amd import ops
    from openstereo_amd.engine import PackedConv3d
    return PackedConv3d(_eye(t.shape[1]).to(DEV), None, 0, precision="f16x3")(ops.to_cl(t.to(DEV)), out=out, out_off=out_off, out_split=True)


def _join(y, Co, x_off=0):
    from openstereo_amd.engine import PackedConv3d
    return PackedConv3d(_eye(Co).to(DEV), None, 0, precision="f16x3")(y, x_off=x_off)[:, :Co].cpu()


def _brick(lib, fn):
    prev = lib.osa_deconv_walk(0)
    try:
        n = lib.osa_deconv3d_walk_launches()
        y = fn()
        assert lib.osa_deconv3d_walk_launches() == n, "the switch did not select the brick form"
    finally:
        lib.osa_deconv_walk(prev)
    return y


def _walk(lib, fn, oseg=0):
    """both layer classes, whatever the shipped default is; oseg > 0: that many output planes per segment (osa_deconv_walk_segment_planes) --
    the cost model cuts shapes as small as these into one-plane segments"""
    prev, prev_planes = lib.osa_deconv_walk(3), lib.osa_deconv_walk_segment_planes(oseg)
    try:
        n = lib.osa_deconv3d_walk_launches()
        y = fn()
        assert lib.osa_deconv3d_walk_launches() == n + 1, "the layer did not take the walking form"
    finally:
        lib.osa_deconv_walk(prev)
        lib.osa_deconv_walk_segment_planes(prev_planes)
    return y


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_walking_deconv_vs_torch_and_brick(case, lib):
    from openstereo_amd import ranges
    from openstereo_amd.engine import is_split
    name, Ci, Co, (B, D, H, W), act = case
    ref_fn, pdc, prl = _layer(name, Ci, Co, act)
    x, r = _inputs(Ci, Co, B, D, H, W)
    with torch.no_grad():
        ref = ref_fn(x, r)
        xs, rs = _split(x), _split(r)
        run = lambda: pdc(xs, redir=(prl, rs), out_split=True)
        y = _walk(lib, run)
        assert torch.equal(y, _walk(lib, run)), "not deterministic"
        assert is_split(y) and tuple(y.shape[2:]) == tuple(ref.shape[2:])
        got = _join(y, Co)
        err = float((got - ref).abs().max())
        print(f"[{name}] max |walk - torch| = {err:.3e}, max |ref| = {float(ref.abs().max()):.3e}")
        torch.testing.assert_close(got, ref, **TOL, msg=lambda m: f"walking deconv [{name}] vs torch: {m}")
        yb = _brick(lib, run)
        torch.testing.assert_close(got, _join(yb, Co), **TOL, msg=lambda m: f"walking deconv [{name}] vs brick form: {m}")
        # the range block of the output: max |value| must cover the tensor, and the scale the next layer reads is the brick form's
        import range_block_cases as R
        R.check_recorded_max(float(ranges.amax_of(ranges.meta_of(y))), R.decode_split(y, ranges.meta_of(y).cpu()), "split", name)
        assert float(ranges.amax_of(ranges.meta_of(y))) >= float(ref.abs().max()) * (1 - 1e-5)      # (and it covers the reference's maximum, as before)
        assert float(ranges.meta_of(y)[1]) == float(ranges.meta_of(yb)[1]), "the published output scale differs from the brick form's"


SEGMENT_CASES = [
    # name, Ci, Co, (B, D, H, W), output planes per segment: even and odd segment starts, even -> odd and odd -> even transitions inside a
    # segment, a ragged last segment, the last odd plane (no upper neighbour) as the end of a longer walk, one segment for the whole depth
    ("conv6 class, 2 planes", 64, 32, (1, 3, 9, 33), 2),
    ("conv6 class, 3 planes (odd starts)", 64, 32, (2, 4, 8, 16), 3),
    ("conv6 class, 5 planes, ragged last segment", 64, 32, (1, 4, 11, 37), 5),
    ("conv6 class, one segment", 64, 32, (1, 3, 8, 34), 6),
    ("conv5 class, 2 planes", 128, 64, (1, 3, 6, 20), 2),
    ("conv5 class, 3 planes (odd starts)", 128, 64, (2, 4, 5, 35), 3),
    ("conv5 class, 5 planes, ragged last segment", 128, 64, (1, 3, 4, 33), 5),
    ("conv5 class, one segment", 128, 64, (1, 2, 6, 20), 4),
]


@pytest.mark.parametrize("case", SEGMENT_CASES, ids=[c[0] for c in SEGMENT_CASES])
def test_segments_of_several_output_planes(case, lib):
    """A workgroup that walks more than one plane: accumulators re-zeroed between planes, the transpose tiles aliasing the plane buffer the next
    pass's transfer lands in, the weight look-ahead crossing plane boundaries."""
    name, Ci, Co, (B, D, H, W), oseg = case
    assert 1 < oseg <= 2 * D
    ref_fn, pdc, prl = _layer(name, Ci, Co, "relu")
    x, r = _inputs(Ci, Co, B, D, H, W, seed=13)
    with torch.no_grad():
        ref = ref_fn(x, r)
        xs, rs = _split(x), _split(r)
        run = lambda: pdc(xs, redir=(prl, rs), out_split=True)
        y = _walk(lib, run, oseg)
        assert torch.equal(y, _walk(lib, run, oseg)), "not deterministic"
        got = _join(y, Co)
        print(f"[{name}] max |walk - torch| = {float((got - ref).abs().max()):.3e}, max |ref| = {float(ref.abs().max()):.3e}")
        torch.testing.assert_close(got, ref, **TOL, msg=lambda m: f"walking deconv [{name}] vs torch: {m}")
        torch.testing.assert_close(got, _join(_brick(lib, run), Co), **TOL, msg=lambda m: f"walking deconv [{name}] vs brick form: {m}")
        # the summation order of a plane does not depend on how the depth is cut: one-plane segments give the same bits
        assert torch.equal(y, _walk(lib, run, 1)), "the result depends on the segment length"


def test_layers_outside_the_form_keep_the_brick_kernel(lib):
    """fp32 tensors, a residual instead of redir, k = 4, 2-D, the f32 and f16 modes: the eligibility test falls through, the counter stays"""
    from openstereo_amd import ops
    from openstereo_amd.engine import PackedConv3d
    g = torch.Generator().manual_seed(0)
    x = ops.to_cl(torch.randn(1, 64, 2, 6, 20, generator=g).to(DEV))
    r = ops.to_cl(torch.randn(1, 32, 4, 12, 40, generator=g).to(DEV))
    x2 = ops.to_cl(torch.randn(1, 64, 1, 6, 20, generator=g).to(DEV))
    mk = lambda k, op: nn.ConvTranspose3d(64, 32, k, stride=2, padding=1, output_padding=op, bias=False).to(DEV)
    prev = lib.osa_deconv_walk(3)
    try:
        with torch.no_grad():
            n0 = lib.osa_deconv3d_walk_launches()
            rl = PackedConv3d(nn.Conv3d(32, 32, 1, bias=False).to(DEV), None, 0, precision="f16x3")
            ident = PackedConv3d(_eye(64).to(DEV), None, 0, precision="f16x3")
            ident32 = PackedConv3d(_eye(32).to(DEV), None, 0, precision="f16x3")
            xs, rs = ident(x, out_split=True), ident32(r, out_split=True)
            PackedConv3d(mk(3, 1), None, 1, precision="f16x3")(x, redir=(rl, r))                           # fp32 tensors in and out
            PackedConv3d(mk(3, 1), None, 1, precision="f16x3")(xs, redir=(rl, rs))                         # split in, fp32 out
            PackedConv3d(mk(3, 1), None, 1, precision="f16x3")(xs, residual=rs, out_split=True)            # a residual instead of redir
            PackedConv3d(mk(3, 1), None, 1, precision="f16x3")(xs, out_split=True)                         # no second branch at all
            PackedConv3d(mk(4, 0), None, 1, precision="f16x3")(xs, redir=(rl, rs), out_split=True)         # k = 4
            PackedConv3d(nn.ConvTranspose2d(64, 32, 3, stride=2, padding=1, output_padding=1, bias=False).to(DEV), None, 1,
                         precision="f16x3")(ident(x2, out_split=True))                                     # 2-D (split in, fp32 out: the form it has)
            rl32 = PackedConv3d(nn.Conv3d(32, 32, 1, bias=False).to(DEV), None, 0, precision="f32")
            PackedConv3d(mk(3, 1), None, 1, precision="f32")(x, redir=(rl32, r))                           # exact-f32 mode
            PackedConv3d(mk(3, 1), None, 1, precision="f16")(x)                                            # f16 mode
            assert lib.osa_deconv3d_walk_launches() == n0
    finally:
        lib.osa_deconv_walk(prev)


def test_channel_slices_of_wider_buffers_inside_nan(lib):
    """Input, redir input and output are channel slices / strided views of wider buffers that sit in the middle of allocations filled with NaN:
    halo rows and columns, the plane above the last one, padding slots and masked lanes must not bring any of it in, and nothing outside the
    output slice may be written."""
    from openstereo_amd import ops
    name, Ci, Co, (B, D, H, W) = "views", 64, 32, (2, 2, 9, 35)
    ref_fn, pdc, prl = _layer(name, Ci, Co, "relu")
    x, r = _inputs(Ci, Co, B, D, H, W, seed=5)

    def nan_view(C, d, h, w, guard=4096):
        n = B * d * h * w * C
        flat = torch.full((n + 2 * guard,), float("nan"), device=DEV)
        return flat, flat[guard:guard + n].view(B, d, h, w, C).permute(0, 4, 1, 2, 3)

    with torch.no_grad():
        ref = ref_fn(x, r)
        xflat, xw = nan_view(96, D, H, W)                       # input: channels [16, 80) of 96
        rflat, rw = nan_view(48, 2 * D, 2 * H, 2 * W)           # redir input: channels [0, 32) of 48
        yflat, yw = nan_view(64, 2 * D, 2 * H, 2 * W)           # output: channels [16, 48) of 64
        assert ops.is_cl(xw) and ops.is_cl(rw) and ops.is_cl(yw)
        _split(x, out=xw, out_off=16)
        _split(r, out=rw, out_off=0)
        assert bool(torch.isnan(xw[:, :16]).all()) and bool(torch.isnan(xw[:, 80:]).all()) and bool(torch.isnan(rw[:, 32:]).all())
        run = lambda: pdc(xw, x_off=16, redir=(prl, rw), out=yw, out_off=16, out_split=True)
        _walk(lib, run)
        got = _join(yw, Co, x_off=16)
        assert bool(torch.isfinite(got).all()), "NaN from outside the tensors reached the output"
        torch.testing.assert_close(got, ref, **TOL, msg=lambda m: f"walking deconv on views vs torch: {m}")
        assert bool(torch.isnan(yw[:, :16]).all()) and bool(torch.isnan(yw[:, 48:]).all()), "channels outside the output slice were written"
        assert bool(torch.isnan(yflat[:4096]).all()) and bool(torch.isnan(yflat[-4096:]).all()), "bytes outside the output tensor were written"
        walked = yw[:, 16:48].clone()
        _brick(lib, run)
        torch.testing.assert_close(got, _join(yw, Co, x_off=16), **TOL, msg=lambda m: f"walking deconv on views vs brick form: {m}")
        _walk(lib, run)
        assert torch.equal(yw[:, 16:48], walked), "not deterministic"


def test_graph_replay_equals_eager(lib):
    name, Ci, Co, (B, D, H, W) = "graph", 64, 32, (1, 3, 9, 34)
    _, pdc, prl = _layer(name, Ci, Co, "relu")
    x, r = _inputs(Ci, Co, B, D, H, W, seed=9)
    from openstereo_amd import ops
    prev, prev_planes = lib.osa_deconv_walk(3), lib.osa_deconv_walk_segment_planes(3)
    try:
        with torch.no_grad():
            xs, rs = _split(x), _split(r)
            out = ops.empty_cl(B, Co, 2 * D, 2 * H, 2 * W, torch.device(DEV))
            n0 = lib.osa_deconv3d_walk_launches()
            pdc(xs, redir=(prl, rs), out=out, out_split=True)
            assert lib.osa_deconv3d_walk_launches() == n0 + 1
            eager = out.clone()
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                pdc(xs, redir=(prl, rs), out=out, out_split=True)
            assert lib.osa_deconv3d_walk_launches() == n0 + 2, "the captured launch did not take the walking form"
            for _ in range(3):
                out.zero_()
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, eager), "graph replay differs from the eager launch"
    finally:
        lib.osa_deconv_walk(prev)
        lib.osa_deconv_walk_segment_planes(prev_planes)


def test_co_resident_with_the_marching_conv(lib):
    """the walking kernel on one stream while conv_march_kernel runs on two others: bit-identical to the idle-GPU result"""
    from openstereo_amd import engine, ops
    from openstereo_amd.engine import PackedConv3d
    name, Ci, Co, (B, D, H, W) = "co-resident", 64, 32, (1, 12, 34, 60)
    _, pdc, prl = _layer(name, Ci, Co, "relu")
    x, r = _inputs(Ci, Co, B, D, H, W, seed=11)
    g = torch.Generator().manual_seed(2)
    prev, prev_planes = lib.osa_deconv_walk(3), lib.osa_deconv_walk_segment_planes(4)
    try:
        with torch.no_grad():
            xs, rs = _split(x), _split(r)
            out = ops.empty_cl(B, Co, 2 * D, 2 * H, 2 * W, torch.device(DEV))
            launch = lambda: pdc(xs, redir=(prl, rs), out=out, out_split=True)
            n0 = lib.osa_deconv3d_walk_launches()
            idle = launch().clone()
            assert lib.osa_deconv3d_walk_launches() == n0 + 1
            # the load: two streams looping the 3x3x3 32 -> 32 layer on split tensors
            pc0 = PackedConv3d(nn.Conv3d(32, 32, 3, padding=1, bias=False).to(DEV), None, 1, precision="f16x3")
            loads = []
            for _ in range(2):
                t = ops.to_cl(torch.randn(1, 32, 24, 68, 120, generator=g).to(DEV))
                t._osa_meta = engine.input_meta(t)
                loads.append(pc0(t, out_split=True))
            m0 = lib.osa_conv3d_march_launches()
            pc0(loads[0], out_split=True)
            assert lib.osa_conv3d_march_launches() == m0 + 1, "the load must be the d-marching form"
            torch.cuda.synchronize()
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            bad = torch.zeros(1, dtype=torch.int64, device=DEV)
            for _ in range(20):
                for st, t in zip(streams, loads):
                    with torch.cuda.stream(st):
                        for _ in range(2):
                            pc0(t, out_split=True)
                bad += (launch().view(torch.int32) != idle.view(torch.int32)).sum()
            torch.cuda.synchronize()
            assert int(bad) == 0, f"{int(bad)} differing words next to the marching conv"
    finally:
        lib.osa_deconv_walk(prev)
        lib.osa_deconv_walk_segment_planes(prev_planes)
