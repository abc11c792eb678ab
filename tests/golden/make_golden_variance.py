"""Generate tests/golden/disparity_variance.npz by running the REAL reference's disparity_variance.

Runs only where the reference is mounted (CPU torch).  Its two copies of the function (models/cfnet/submodule.py:128-134,
models/igevpp/submodule.py:153-159) are imported through stub parent packages, as in make_golden.py.

Stored per case of tests/variance_cases.py: the inputs (cost base, raised planes, loss weights), and per cost distribution the reference's
OWN fp32 error against fp64 on those inputs -- `E_ref` for the variance (max over all pixels of |var - var64| / (1 + var64)) and
`E_ref_grad` for the gradients of sum(a disp) + sum(b var) (max |g - g64| / max |g64|): the GPU tests allow the engine 4x these.  For the
probabilities form with a given disparity and an unnormalised volume also the outputs of both reference functions (fp32) and fp64.

    python tests/golden/make_golden_variance.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("OPENSTEREO_REF", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import variance_cases as VC  # noqa: E402


def import_reference():
    if not os.path.isdir(REF):
        raise SystemExit(f"{REF} not found: golden vectors can only be generated where the reference is mounted")
    sys.path.insert(0, REF)
    for name, path in [("stereo", "stereo"), ("stereo.modeling", "stereo/modeling"), ("stereo.modeling.models", "stereo/modeling/models")]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, path)]
        sys.modules[name] = m
    sys.modules.setdefault("timm", types.ModuleType("timm"))
    from stereo.modeling.models.cfnet import submodule as cf
    from stereo.modeling.models.igevpp import submodule as ig
    return cf, ig


def main():
    cf, ig = import_reference()
    torch.manual_seed(0)
    reg = lambda x, maxdisp: cf.disparity_regression(x, maxdisp)
    var = lambda x, maxdisp, disparity: cf.disparity_variance(x, maxdisp, disparity)
    ref = dict(regression=reg, variance=var)
    out = {}
    T = torch.from_numpy
    for name in list(VC.FUSED) + list(VC.PLAIN):
        arrs = VC.make_inputs(name)
        for k, v in arrs.items():
            out[f"{name}__{k}"] = v
        a, b = T(arrs["a"]), T(arrs["b"])
        for dist in VC.DISTS:
            cost = VC.cost_of(arrs, dist)
            forms = {}
            if name in VC.FUSED:
                _, (D, h, w), align = VC.FUSED[name]
                forms["fused"] = (lambda c, **kw: VC.compose_fused(c, D, h, w, align, **kw), [cost])
            else:
                forms["logits"] = (lambda c, **kw: VC.compose_logits(c, **kw), [cost])
                p = VC.prob_of(cost)
                # the distribution's own mean as the given disparity (VC.own_mean): a constant here -- the gradient with respect to it
                # is zero up to rounding and is checked on the `given` inputs below, where it is not
                mean = VC.own_mean(p)
                forms["prob"] = (lambda x, **kw: VC.compose_prob(x, mean, **kw), [p])
            for form, (fn, leaves) in forms.items():
                with torch.no_grad():
                    d32, v32 = fn(*leaves, **ref)
                    d64, v64 = fn(*[t.double() for t in leaves])
                    mine = fn(*leaves)                                 # tests/variance_cases.py's arithmetic == the reference's functions
                    assert torch.equal(mine[0], d32) and torch.equal(mine[1], v32), (name, dist, form)
                g32 = VC.loss_grads(lambda *xs: fn(*xs, **ref), leaves, a, b)
                g64 = VC.loss_grads(fn, [t.double() for t in leaves], a, b)
                tag = f"{name}__{dist}__{form}"
                out[tag + "__E_ref"] = np.float64(VC.var_err(v32, v64))
                out[tag + "__E_ref_grad"] = np.array([VC.grad_err(x, y) for x, y in zip(g32, g64)], dtype=np.float64)
                print(f"{tag:28s} var64 {float(v64.min()):10.4g} .. {float(v64.max()):10.4g}   E_ref {out[tag + '__E_ref']:.3g}   "
                      f"E_ref_grad {' '.join(f'{e:.3g}' for e in out[tag + '__E_ref_grad'])}")
        if name in VC.PLAIN:
            # the exact twin: unnormalised volume, a disparity map that is not its mean -- both copies of the reference function
            x, d = T(arrs["prob_unnorm"]), T(arrs["given_disp"])
            with torch.no_grad():
                r_cf, r_ig = cf.disparity_variance(x, x.shape[1], d), ig.disparity_variance(x, x.shape[1], d)
                v64 = VC.variance(x.double(), x.shape[1], d.double())
            assert torch.equal(r_cf, r_ig) and r_cf.shape == d.shape
            fn = lambda xx, dd, **kw: VC.compose_prob(xx, dd, **kw)
            g32 = VC.loss_grads(lambda *xs: fn(*xs, **ref), [x, d], a, b)
            g64 = VC.loss_grads(fn, [x.double(), d.double()], a, b)
            tag = f"{name}__given__prob"
            out[tag + "__ref_cfnet"], out[tag + "__ref_igevpp"], out[tag + "__var64"] = r_cf.numpy(), r_ig.numpy(), v64.numpy()
            out[tag + "__E_ref"] = np.float64(VC.var_err(r_cf, v64))
            out[tag + "__E_ref_grad"] = np.array([VC.grad_err(p, q) for p, q in zip(g32, g64)], dtype=np.float64)
            print(f"{tag:28s} E_ref {out[tag + '__E_ref']:.3g}   E_ref_grad {' '.join(f'{e:.3g}' for e in out[tag + '__E_ref_grad'])}")
    np.savez_compressed(VC.GOLDEN, **out)
    print(f"wrote {VC.GOLDEN}: {os.path.getsize(VC.GOLDEN) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
