"""Generate tests/golden/msnet2d_blocks.npz by running the REAL reference's MobileV2_Residual.

Runs only where the reference is mounted (CPU torch).  models/msnet/submodule.py (lines 94-133) is imported through stub parent packages,
as in make_golden_msnet3d.py; the block is built with the case's arguments, takes the seeded state_dict of the restatement in
tests/mv2_block2d_cases.py (the keys match) and runs in eval mode on the seeded input.

Stored: the fp32 outputs only, for the cases named by mv2_block2d_cases.GOLDEN_CASES, keyed `<case>__y`.  Parameters and inputs are not
stored: tests regenerate them from the seeds.

    python tests/golden/make_golden_msnet2d.py
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

import mv2_block2d_cases as M  # noqa: E402


def import_reference():
    if not os.path.isdir(REF):
        raise SystemExit(f"{REF} not found: golden vectors can only be generated where the reference is mounted")
    sys.path.insert(0, REF)
    for name, path in [("stereo", "stereo"), ("stereo.modeling", "stereo/modeling"), ("stereo.modeling.models", "stereo/modeling/models"),
                       ("stereo.modeling.models.msnet", "stereo/modeling/models/msnet")]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, path)]
        sys.modules[name] = m
    from stereo.modeling.models.msnet import submodule
    return submodule.MobileV2_Residual


def main():
    ref_cls = import_reference()
    out = {}
    for case in M.GOLDEN_CASES:
        B, Ci, Co, stride, ratio, H, W = M.CASES[case]
        blk = ref_cls(Ci, Co, stride, ratio)
        blk.load_state_dict(M.make_block(case).state_dict())
        with torch.no_grad():
            y = blk.eval()(M.make_input(case))
        assert y.dtype == torch.float32 and tuple(y.shape) == M.out_shape(case)
        out[f"{case}__y"] = y.contiguous().numpy()
    np.savez_compressed(M.GOLDEN, **out)
    print(f"wrote {M.GOLDEN}: {os.path.getsize(M.GOLDEN) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
