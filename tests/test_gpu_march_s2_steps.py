"""The sub-pass structure of the stride-2 d-marching convolution (csrc/conv_march_s2.h): a barrier per (plane, chunk, kd) with all 9
(kh, kw) taps, the 36 KB weight slab of the next sub-pass landing in the second slab buffer.

Method of tests/test_gpu_march_s2.py: a split input made through an identity PackedConv3d; against torch fp32 on the CPU (conv + eval
BatchNorm + activation) and against the brick form of the same launch (bit 29 of osa_conv_b_ring_mask off), both at that file's
atol = rtol = 3e-5; a repeated launch is bit-identical; the launch counter proves the form ran; the range block covers max |y|.

The shapes are the smallest at which the structure can go wrong:
* sub-pass sequencing: one even + one odd plane; an even LAST plane that completes an output plane alone; one output plane per segment
  (osa_conv_march_s2_segment_planes(1): every segment but the first starts on an odd plane that contributes only its kd = 0 half); three
  planes per segment of four output planes (a ragged last segment);
* the slab double buffer: one chunk (the buffers alternate with no chunk change) and four chunks;
* ragged columns: Ho and Wo below the 4 x 32 tile; Wo = 33 (a second column tile with one valid column)."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from openstereo_amd.utils.weights import synth_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = [
    # name, Ci, Co, (B, D, H, W), activation, planes per segment (0: the cost model)
    ("one even and one odd plane", 32, 64, (1, 2, 8, 64), "relu", 0),
    ("even last plane", 32, 64, (1, 3, 8, 64), "relu", 0),
    ("one output plane per segment", 32, 64, (1, 8, 8, 64), "relu", 1),
    ("ragged last segment", 32, 64, (1, 8, 8, 64), "relu", 3),
    ("one chunk", 16, 64, (1, 5, 8, 40), "relu", 0),
    ("four chunks", 64, 64, (1, 6, 10, 66), "relu", 0),
    ("column smaller than the tile", 32, 64, (2, 5, 5, 5), "relu", 0),
    ("second column tile with one column", 32, 64, (1, 4, 9, 66), "relu", 0),
]


def _eye(c):
    m = nn.Conv3d(c, c, 1, bias=False)
    m.weight.data = torch.eye(c).reshape(c, c, 1, 1, 1).clone()
    return m


def _bn(c, name):
    bn = nn.BatchNorm3d(c)
    bn.load_state_dict({k: synth_tensor(f"{name}.{k}", v.shape, 2) for k, v in bn.state_dict().items()})
    return bn.eval()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_sub_pass_form_vs_torch_and_brick(case, lib):
    from openstereo_amd import ops, ranges
    from openstereo_amd.engine import PackedConv3d, is_split
    name, Ci, Co, (B, D, H, W), act, planes = case
    conv = nn.Conv3d(Ci, Co, 3, 2, 1, bias=False)
    conv.weight.data = synth_tensor(name + ".w", conv.weight.shape, 1)
    bn = _bn(Co, name)
    x = torch.from_numpy(np.random.default_rng(5).normal(0, 1, (B, Ci, D, H, W)).astype(np.float32))
    actf = {"relu": F.relu, "leaky": lambda t: F.leaky_relu(t, 0.01), "none": lambda t: t}[act]
    with torch.no_grad():
        ref = actf(bn(conv(x)))
        xs = PackedConv3d(_eye(Ci).to(DEV), None, 0, precision="f16x3")(ops.to_cl(x.to(DEV)), out_split=True)
        assert is_split(xs)
        pc = PackedConv3d(conv.to(DEV), bn.to(DEV), {"none": 0, "relu": 1, "leaky": 2}[act], 0.01, precision="f16x3")
        back = PackedConv3d(_eye(Co).to(DEV), None, 0, precision="f16x3")
        prev_planes = lib.osa_conv_march_s2_segment_planes(planes)
        mask = lib.osa_conv_b_ring_mask(0)
        lib.osa_conv_b_ring_mask(mask)
        try:
            n0 = lib.osa_conv3d_march_s2_launches()
            y = pc(xs, out_split=True)
            assert lib.osa_conv3d_march_s2_launches() == n0 + 1, "the layer did not take the stride-2 marching form"
            assert torch.equal(y, pc(xs, out_split=True)), "not deterministic"
            assert is_split(y) and tuple(y.shape[2:]) == tuple(ref.shape[2:])
            got = back(y)[:, :Co].cpu()
            err = float((got - ref).abs().max())
            print(f"[{name}] max |marching - torch| = {err:.3e}, max |ref| = {float(ref.abs().max()):.3e}")
            torch.testing.assert_close(got, ref, atol=3e-5, rtol=3e-5, msg=lambda m: f"sub-pass form [{name}] vs torch: {m}")
            lib.osa_conv_b_ring_mask(mask & ~(1 << 29))           # the brick form of the same launch
            n1 = lib.osa_conv3d_march_s2_launches()
            yb = pc(xs, out_split=True)
            assert lib.osa_conv3d_march_s2_launches() == n1, "the switch did not select the brick form"
        finally:
            lib.osa_conv_b_ring_mask(mask)
            lib.osa_conv_march_s2_segment_planes(prev_planes)
        torch.testing.assert_close(got, back(yb)[:, :Co].cpu(), atol=3e-5, rtol=3e-5, msg=lambda m: f"sub-pass form [{name}] vs brick form: {m}")
        import range_block_cases as R
        R.check_recorded_max(float(ranges.amax_of(ranges.meta_of(y))), R.decode_split(y, ranges.meta_of(y).cpu()), "split", name)
        assert float(ranges.amax_of(ranges.meta_of(y))) >= float(ref.abs().max()) * (1 - 1e-5)      # (and it covers the reference's maximum, as before)


def test_segment_length_does_not_change_a_bit(lib):
    """Each output plane is summed in the order plane, chunk, kh, kw wherever its segment starts, so every segment length gives the same
    bits -- and the setter returns what it replaced."""
    from openstereo_amd import ops
    from openstereo_amd.engine import PackedConv3d
    conv = nn.Conv3d(32, 64, 3, 2, 1, bias=False)
    conv.weight.data = synth_tensor("seglen.w", conv.weight.shape, 1)
    x = torch.from_numpy(np.random.default_rng(6).normal(0, 1, (1, 32, 8, 8, 64)).astype(np.float32))
    with torch.no_grad():
        xs = PackedConv3d(_eye(32).to(DEV), None, 0, precision="f16x3")(ops.to_cl(x.to(DEV)), out_split=True)
        pc = PackedConv3d(conv.to(DEV), _bn(64, "seglen").to(DEV), 1, precision="f16x3")
        prev = lib.osa_conv_march_s2_segment_planes(0)
        try:
            assert lib.osa_conv_march_s2_segment_planes(4) == 0
            n0 = lib.osa_conv3d_march_s2_launches()
            whole = pc(xs, out_split=True)                          # D = 8 -> 4 output planes: one segment
            for was, planes in ((4, 1), (1, 2), (2, 3)):
                assert lib.osa_conv_march_s2_segment_planes(planes) == was
                assert torch.equal(whole, pc(xs, out_split=True)), f"{planes} output planes per segment changed the result"
            assert lib.osa_conv3d_march_s2_launches() == n0 + 4
        finally:
            lib.osa_conv_march_s2_segment_planes(prev)
