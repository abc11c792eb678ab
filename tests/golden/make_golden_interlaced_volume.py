"""Generate tests/golden/interlaced_volume.npz by running the REAL reference's InterlacedVolume and MSNet2D.

Runs only where the reference is mounted (CPU torch).  stereo/modeling/cost_volume/cost_volume.py and stereo/modeling/models/msnet/MSNet2D.py
are imported through stub parent packages, as in make_golden_msnet3d.py.  Both take the seeded state_dicts of the restatements in
tests/interlaced_volume_cases.py (the keys match) and run in eval mode:

    sb__vol         InterlacedVolume(8) on the seeded inputs of case `sb`
    ms__featL/R     the two preconv11 outputs of MSNet2D (forward hook) on the 32 x 208 synthetic pair: [1, 32, 8, 52]
    ms__vol         the dres0 input of the same run (forward pre-hook): the 48-plane volume, [1, 48, 8, 52]
    e2e__disp_pred  that run's disp_pred

Outputs only: parameters and inputs are regenerated from the seeds by the tests.

    python tests/golden/make_golden_interlaced_volume.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("OPENSTEREO_REF", "/root/reference")
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))

import interlaced_volume_cases as M  # noqa: E402


def import_reference():
    if not os.path.isdir(REF):
        raise SystemExit(f"{REF} not found: golden vectors can only be generated where the reference is mounted")
    sys.path.insert(0, REF)
    for name, path in [("stereo", "stereo"), ("stereo.modeling", "stereo/modeling"), ("stereo.modeling.models", "stereo/modeling/models"),
                       ("stereo.modeling.models.msnet", "stereo/modeling/models/msnet"), ("stereo.modeling.cost_volume", "stereo/modeling/cost_volume")]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, path)]
        sys.modules[name] = m
    from stereo.modeling.cost_volume import cost_volume
    from stereo.modeling.models.msnet import MSNet2D
    return cost_volume.InterlacedVolume, MSNet2D.MSNet2D


def main():
    ref_iv, ref_ms = import_reference()
    out = {}
    with torch.no_grad():
        iv = ref_iv(M.CASES["sb"][5])
        iv.load_state_dict(M.make_volume("sb").state_dict())
        out["sb__vol"] = iv.eval()(*M.make_inputs("sb"), M.CASES["sb"][4])

        net = ref_ms(types.SimpleNamespace(MAX_DISP=M.E2E_MAXDISP))
        net.load_state_dict(M.make_msnet2d().state_dict())
        feats = []
        hooks = [net.preconv11.register_forward_hook(lambda m, a, y: feats.append(y.clone())),
                 net.dres0.register_forward_pre_hook(lambda m, a: out.__setitem__("ms__vol", a[0].clone()))]
        L, R = M.e2e_images()
        out["e2e__disp_pred"] = net.eval()({"left": L, "right": R})["disp_pred"]
        for h in hooks:
            h.remove()
        out["ms__featL"], out["ms__featR"] = feats
    assert sorted(out) == sorted(M.GOLDEN_KEYS)
    h4, w4 = M.E2E_IMAGE[0] // 4, M.E2E_IMAGE[1] // 4
    assert tuple(out["ms__vol"].shape) == (1, 48, h4, w4) and tuple(out["ms__featL"].shape) == (1, 32, h4, w4)
    for k, v in out.items():
        assert v.dtype == torch.float32
        print(k, tuple(v.shape), "max", float(v.abs().max()), "std", float(v.std()))
    np.savez_compressed(M.GOLDEN, **{k: v.contiguous().numpy() for k, v in out.items()})
    print(f"wrote {M.GOLDEN}: {os.path.getsize(M.GOLDEN) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
