"""Generate tests/golden/igevpp_geometry.npz by running the REAL reference's IGEV++ lookup class.

Runs only where the reference is mounted (CPU torch).  models/igevpp/geometry.py (Combined_Geo_Encoding_Volume, lines 6-87) is imported
through stub parent packages, as in make_golden_variance.py.

Stored: the class's four fp32 outputs (geo_feat0, geo_feat1, geo_feat2, init_corr) for the cases / disparity sets named by
tests/multirange_cases.py (GOLDEN_CASES x GOLDEN_SETS, `grid` coordinates), keyed `<case>__<set>__<output index>`: batch element 0 of each
([:1]; all of `radius1`, half of `odd`), which keeps the file below geo_encoding.npz.  The inputs are not stored: tests regenerate them from
the seeds of multirange_cases.inputs / disparity_sets.

    python tests/golden/make_golden_igevpp_geometry.py
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

import multirange_cases as M  # noqa: E402


def import_reference():
    if not os.path.isdir(REF):
        raise SystemExit(f"{REF} not found: golden vectors can only be generated where the reference is mounted")
    sys.path.insert(0, REF)
    for name, path in [("stereo", "stereo"), ("stereo.modeling", "stereo/modeling"), ("stereo.modeling.models", "stereo/modeling/models"),
                       ("stereo.modeling.models.igevpp", "stereo/modeling/models/igevpp")]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, path)]
        sys.modules[name] = m
    try:
        import scipy  # noqa: F401  (igevpp/utils.py imports scipy.interpolate for a function the lookup does not use)
    except ImportError:
        sp = types.ModuleType("scipy")
        sp.interpolate = types.ModuleType("scipy.interpolate")
        sys.modules["scipy"], sys.modules["scipy.interpolate"] = sp, sp.interpolate
    from stereo.modeling.models.igevpp import geometry
    return geometry.Combined_Geo_Encoding_Volume


def reference_outputs(cls, case, sets=M.SETS, coords=M.COORDS):
    """(set, coords) -> the real class's four fp32 outputs on the case's inputs"""
    B, C, D0, D1, D2, H, W, Cf, L, r = M.CASES[case]
    leaves, _ = M.inputs(case)
    disp = M.disparity_sets(case)
    with torch.no_grad():
        fn = cls(*leaves, radius=r, num_levels=L)
        return {(s, cv): fn(disp[s], M.coords(case, cv)) for s in sets for cv in coords}


def main():
    cls = import_reference()
    out = {}
    for case in M.GOLDEN_CASES:
        for (s, cv), outs in reference_outputs(cls, case, M.GOLDEN_SETS, ("grid",)).items():
            assert [tuple(o.shape[1:2]) for o in outs] == [(n,) for n in M.channels(case)]
            for q, o in enumerate(outs):
                assert o.dtype == torch.float32
                out[f"{case}__{s}__{q}"] = o[:1].numpy()
    np.savez_compressed(M.GOLDEN, **out)
    print(f"wrote {M.GOLDEN}: {os.path.getsize(M.GOLDEN) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
