"""GPU: MobileStereoNet's 3-D inverted-residual block as one launch (csrc/mv2_block3d.hip; osa_native.mv2_block3d; models/msnet.py grafted
onto the restatement of tests/mv2_block3d_cases.py) by the tolerance rule stated there: every case in both memory formats, the padding of
the HIDDEN tensor, bit-reproducibility, independence of the batch size, hipGraph capture, an hourglass3D of such blocks, and the cases in
which the block's own torch composition runs instead (the kernel's channel limits among them)."""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mv2_block3d_cases as M
import mv2_cases_common as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def grafted():
    """the mirror's forward on the restatement's class, as attach._graft_plan() puts it on the reference's"""
    from openstereo_amd import attach
    from openstereo_amd.models.msnet import MobileV2Residual3D
    attach._graft(M.Block, MobileV2Residual3D, ("forward", "reset_engine"), True)
    yield
    attach.unpatch_reference()


@functools.lru_cache(maxsize=None)
def gpu_block(case):
    return M.make_block(case).to(DEV)


Entered, fused = functools.partial(C.Entered, cls=M.Block), functools.partial(C.fused, cls=M.Block)


def cl(x):
    return x.contiguous(memory_format=torch.channels_last_3d)


@pytest.mark.parametrize("case", list(M.CASES))
def test_every_case_by_the_rule_in_both_memory_formats(case):
    x = M.make_input(case).to(DEV)
    y_cl, y_nc = fused(gpu_block(case), cl(x)), fused(gpu_block(case), x.contiguous())
    want = M.out_shape(case)
    for y in (y_cl, y_nc):
        assert y.dtype == torch.float32 and tuple(y.shape) == want
        assert y.stride() == torch.empty(want).contiguous(memory_format=torch.channels_last_3d).stride()
    assert torch.equal(y_cl, y_nc), f"{case}: the two memory formats of x give different bits"
    M.check(case, y_cl, M.reference(case, torch.float64), M.reference(case, torch.float32))


@pytest.mark.parametrize("case", ["res", "s2odd"])
def test_the_hidden_tensor_is_padded_with_zeros_not_with_relu6_of_the_shift(case):
    """x = 0: the hidden tensor is relu6(shift1) everywhere inside the volume and ZERO around it, so the output is one value per channel
    in the interior and another on every face; a kernel that pads x instead would return the interior value everywhere"""
    x0 = torch.zeros_like(M.make_input(case))
    r64, r32 = M.reference(case, torch.float64, x0), M.reference(case, torch.float32, x0)
    y = fused(gpu_block(case), cl(x0.to(DEV)))
    M.check(f"{case} x=0", y, r64, r32)
    inner = y[:, :, 1:-1, 1:-1, 1:-1]
    assert inner.numel() and torch.equal(inner, inner[:, :, :1, :1, :1].expand_as(inner)), "the interior is not constant"
    gap = (r64[:, :, 0, 0, 0] - r64[:, :, 1, 1, 1]).abs()                    # corner voxel against the interior, per channel
    assert float(gap.max()) > 1.0, "the case does not tell the two paddings apart"
    assert M.err(y[:, :, 0, 0, 0] - y[:, :, 1, 1, 1], r64[:, :, 0, 0, 0] - r64[:, :, 1, 1, 1]) <= 2 * M.FACTOR * max(M.err(r32, r64), 1e-7)
    for face in (y[:, :, 0], y[:, :, -1], y[:, :, :, 0], y[:, :, :, -1], y[..., 0], y[..., -1]):
        assert not torch.equal(face, inner[:, :, :1, :1, :1].reshape(y.shape[0], y.shape[1], 1, 1).expand_as(face))


def test_bits_do_not_depend_on_the_batch_the_run_or_a_graph_replay():
    blk, x = gpu_block("res"), cl(M.make_input("res").to(DEV))
    y = fused(blk, x)
    assert torch.equal(fused(blk, x), y), "two calls differ"
    assert torch.equal(fused(blk, cl(x[1:2])), y[1:2]), "batch element 1 alone differs from element 1 of the batch of two"
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):                             # one stream, no branches
        yg = blk(x)
    yg.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, y), "the captured launch replays to other bits"


class Hourglass3D(nn.Module):
    """stereo/modeling/models/msnet/MSNet3D.py:10-45 restated from Block"""

    def __init__(self, c):
        super().__init__()
        self.conv1, self.conv2 = M.Block(c, c * 2, 2, 2), M.Block(c * 2, c * 2, 1, 2)
        self.conv3, self.conv4 = M.Block(c * 2, c * 4, 2, 2), M.Block(c * 4, c * 4, 1, 2)
        self.conv5 = nn.Sequential(nn.ConvTranspose3d(c * 4, c * 2, 3, padding=1, output_padding=1, stride=2, bias=False), nn.BatchNorm3d(c * 2))
        self.conv6 = nn.Sequential(nn.ConvTranspose3d(c * 2, c, 3, padding=1, output_padding=1, stride=2, bias=False), nn.BatchNorm3d(c))
        self.redir1, self.redir2 = M.Block(c, c, 1, 2), M.Block(c * 2, c * 2, 1, 2)

    def forward(self, x):
        conv2 = self.conv2(self.conv1(x))
        conv4 = self.conv4(self.conv3(conv2))
        conv5 = F.relu(self.conv5(conv4) + self.redir2(conv2), inplace=True)
        return F.relu(self.conv6(conv5) + self.redir1(x), inplace=True)


def test_hourglass_of_grafted_blocks():
    """the channels_last_3d results flow through torch's transposed convolutions and sums unchanged; training and gradients keep the
    reference's forward"""
    g = torch.Generator().manual_seed(5000)
    net = M.seed_parameters(Hourglass3D(32), g).eval()
    x = 2.0 * torch.randn(1, 32, 8, 12, 20, generator=g)
    with torch.no_grad():
        r64 = copy.deepcopy(net).double()(x.double())
    gnet, gx = copy.deepcopy(net).to(DEV), x.to(DEV)
    with torch.no_grad():                                                    # the float32 figure of the rule: the torch composition (CPU tensors)
        r32 = net(x)
    y = fused(gnet, gx)
    M.check("hourglass3D", y, r64, r32)
    with Entered(gnet) as e:                                                 # eval, but a gradient is required
        gnet(gx.clone().requires_grad_())
    assert e.n == 6
    with Entered(gnet) as e, torch.no_grad():
        gnet.train()(gx)
    assert e.n == 6


def test_fallbacks_run_the_original_composition():
    blk, x = copy.deepcopy(gpu_block("res")), M.make_input("res").to(DEV)
    with Entered(blk) as e, torch.no_grad():
        with torch.autocast("cuda", dtype=torch.float16):
            blk(x)
        assert e.n == 1
        assert blk.half()(x.half()).dtype == torch.float16 and e.n == 2
    r1 = M.Block(32, 32, 1, 1).to(DEV).eval()                                # expanse_ratio == 1: five entries, no expansion
    with Entered(r1) as e, torch.no_grad():
        y = r1(x)
    assert e.n == 1 and tuple(y.shape) == tuple(x.shape)


@pytest.mark.parametrize("channels, dilation", [(20, 1), (136, 1), (32, 2)])
def test_blocks_the_kernel_does_not_take_run_the_original_composition(channels, dilation):
    """channels that are no multiple of 8, channels beyond the kernel's 128 input / output channels, and a dilated depthwise layer (channels
    the kernel takes): `conv` is entered once and the result is the ungrafted composition's, bit for bit"""
    blk = M.Block(channels, channels, 1, 2)
    if dilation != 1:
        blk.conv[3] = nn.Conv3d(2 * channels, 2 * channels, 3, 1, dilation, dilation=dilation, groups=2 * channels, bias=False)
    blk = M.seed_parameters(blk, torch.Generator().manual_seed(6000 + channels)).to(DEV).eval()
    x = torch.randn(1, channels, 2, 3, 3, generator=torch.Generator().manual_seed(6500 + channels)).to(DEV)
    with Entered(blk) as e, torch.no_grad():
        y = blk(x)
        assert e.n == 1
        assert torch.equal(y, blk._ref_forward(x))                              # the restatement's own forward, as attach._graft keeps it
