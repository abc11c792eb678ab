"""Shared by tests/mv2_block2d_cases.py, tests/mv2_block3d_cases.py and the two GPU test files of MobileStereoNet's fused inverted-residual
blocks (a plain module, no fixtures): what does not depend on the rank of the block.

The tolerance rule: err(X) = max |X - float64 restatement| on the same inputs, and every checked tensor X must satisfy
err(X) <= 8 * err(float32 restatement).  The factor 8, as in tests/mr_volume_cases.py: the engine sums K in another order (the halves or
quarters of every 8 or 16 channels interleaved on the matrix unit, the taps row by row, in 2-D the hidden channels in chunks of 48), and a
maximum over thousands of elements is noisy.

A test of such a block passes vacuously when ReLU6 never clamps or when relu6(shift1) is zero (the padding of the hidden tensor could then
be taken for a padding of x), so reference() asserts for the float64 run: outside the degenerate cases at least 5 % of each hidden
pre-activation lies below 0 and at least 5 % above 6; in every case at least 25 % of the expansion's folded shifts are positive.
"""
import torch
import torch.nn as nn

FACTOR = 8.0
CONVS, DECONVS, NORMS = (nn.Conv2d, nn.Conv3d), (nn.ConvTranspose2d, nn.ConvTranspose3d), (nn.BatchNorm2d, nn.BatchNorm3d)


def seed_parameters(module, g):
    """conv weights ~ N(0,1) * 1.5 * sqrt(2 / fan_in), BN weight ~ U(0.5, 2), bias ~ N(0,1), running mean ~ 0.5 N(0,1), running var ~ U(0.5, 2):
    in the order of module.modules(), from the generator g"""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, CONVS + DECONVS):
                fan_in = m.weight[0].numel() if isinstance(m, CONVS) else m.weight[:, 0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 1.5 * (2.0 / fan_in) ** 0.5)
            elif isinstance(m, NORMS):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 1.5 + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.5 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) * 1.5 + 0.5)
    return module


def _assert_not_vacuous(case, blk, x, degenerate):
    pre = []
    hooks = [blk.conv[i].register_forward_hook(lambda m, a, out: pre.append(out.detach().clone())) for i in (1, 4)]   # before the in-place ReLU6
    with torch.no_grad():
        y = blk(x)
    for h in hooks:
        h.remove()
    bn = blk.conv[1]
    shift = bn.bias - bn.running_mean * bn.weight / torch.sqrt(bn.running_var + bn.eps)
    assert float((shift > 0).double().mean()) >= 0.25, f"{case}: too few positive expansion shifts"
    if not degenerate:
        for i, t in enumerate(pre):
            lo, hi = float((t < 0).double().mean()), float((t > 6).double().mean())
            assert lo >= 0.05 and hi >= 0.05, f"{case}: hidden pre-activation {i} has {lo:.1%} below 0 and {hi:.1%} above 6"
    return y


_cache = {}


def reference(cases, case, dtype, x=None):
    """-> the output in `dtype` of the restatement of the case module `cases` (its make_block, make_input, DEGENERATE) on the case's input
    (or on x); the case's own run is computed once and not modified by the tests"""
    if x is not None:
        with torch.no_grad():
            return cases.make_block(case, dtype)(x.to(dtype))
    key = (cases.__name__, case, dtype)
    if key not in _cache:
        blk, xin = cases.make_block(case, dtype), cases.make_input(case, dtype)
        if dtype == torch.float64:
            _cache[key] = _assert_not_vacuous(case, blk, xin, case in cases.DEGENERATE)
        else:
            with torch.no_grad():
                _cache[key] = blk(xin)
    return _cache[key]


def err(x, ref64):
    return float((x.detach().double().cpu() - ref64).abs().max())


def check(what, x, ref64, ref32):
    """the tolerance rule; both numbers in the message"""
    assert tuple(x.shape) == tuple(ref64.shape), f"{what}: shape {tuple(x.shape)}, expected {tuple(ref64.shape)}"
    e, e32 = err(x, ref64), err(ref32, ref64)
    print(f"{what}: err {e:.3e}, fp32 restatement {e32:.3e}")
    assert e <= FACTOR * e32, f"{what}: err {e:.3e} > {FACTOR:g} x {e32:.3e} (the fp32 restatement's error)"


class Entered:
    """counts the calls of the `conv` Sequential of every block of class `cls` under `module`: the torch composition ran"""

    def __init__(self, module, cls):
        self.n = 0
        self.hooks = [m.conv.register_forward_hook(self._hit) for m in module.modules() if isinstance(m, cls)]
        assert self.hooks

    def _hit(self, *a):
        self.n += 1

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for h in self.hooks:
            h.remove()


def fused(blk, x, run=None, *, cls):
    """eval, no grad: the fused launch, proven by `conv` never being entered"""
    with Entered(blk, cls) as e, torch.no_grad():
        y = blk(x) if run is None else run(blk, x)
    assert e.n == 0, "the torch composition ran instead of the fused kernel"
    return y
