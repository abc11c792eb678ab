"""Generate tests/golden/igevpp_volumes.npz by running the REAL reference's IGEV++ volume builder.

Runs only where the reference is mounted (CPU torch).  models/igevpp/submodule.py (build_gwc_volume, lines 87-97) is imported through stub
parent packages, as in make_golden_igevpp_geometry.py; the patch convolutions of igevpp_stereo.py:182-186 are F.conv3d with the case's
seeded weights (what nn.Conv3d(8, 8, (k,1,1), (k,1,1), bias=False) computes).

Stored: the three fp32 volumes of the cases named by tests/mr_volume_cases.py (GOLDEN_CASES), keyed `<case>__V0|V1|V2`.  The inputs are
not stored: tests regenerate them from the seeds of mr_volume_cases.inputs.

    python tests/golden/make_golden_mr_volume.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("OPENSTEREO_REF", "/root/reference")
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))

import mr_volume_cases as M  # noqa: E402


def import_reference():
    if not os.path.isdir(REF):
        raise SystemExit(f"{REF} not found: golden vectors can only be generated where the reference is mounted")
    sys.path.insert(0, REF)
    for name, path in [("stereo", "stereo"), ("stereo.modeling", "stereo/modeling"), ("stereo.modeling.models", "stereo/modeling/models"),
                       ("stereo.modeling.models.igevpp", "stereo/modeling/models/igevpp")]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, path)]
        sys.modules[name] = m
    from stereo.modeling.models.igevpp import submodule
    return submodule.build_gwc_volume


def main():
    build_gwc_volume = import_reference()
    out = {}
    for case in M.GOLDEN_CASES:
        B, C, H, W, D, S, Mr, k0, k1 = M.CASES[case]
        L, R, P0, P1 = M.inputs(case)
        with torch.no_grad():
            vol = build_gwc_volume(L, R, D, M.G)
            vs = (vol[:, :, :S], F.conv3d(vol[:, :, :Mr], P0, stride=(k0, 1, 1)), F.conv3d(vol, P1, stride=(k1, 1, 1)))
        for name, v in zip(M.NAMES, vs):
            assert v.dtype == torch.float32
            out[f"{case}__{name}"] = v.contiguous().numpy()
    np.savez_compressed(M.GOLDEN, **out)
    print(f"wrote {M.GOLDEN}: {os.path.getsize(M.GOLDEN) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
