"""Generate tests/golden/conv3d_reduced.npz by running the REAL reference's Conv3dNormActReduced on the CPU.

Runs only where the reference is mounted (CPU torch).  models/foundationstereo/core/submodule.py (lines 87-112) and
models/fast_foundationstereo/core/submodule.py (lines 90-115) are imported through stub parent packages with the stubs of
make_golden_disparity_attention.py for what the files import and this class does not use.  Each copy's class is built with the
case's arguments, takes the seeded state_dict of the restatement in tests/conv3d_reduced_cases.py (the keys match) and runs in eval mode on
the seeded input; the two copies must agree bit for bit.

Stored: the fp32 outputs only, for the cases named by conv3d_reduced_cases.GOLDEN_CASES, keyed `<case>__y`, and the state_dict keys of the
`fs` reference module as `keys`.  Parameters and inputs are not stored: tests regenerate them from the seeds.

    python tests/golden/make_golden_conv3d_reduced.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))

import conv3d_reduced_cases as M  # noqa: E402
from make_golden_disparity_attention import import_reference  # noqa: E402


def main():
    import_reference()                                     # the stub packages; both submodule files are imported by now
    from stereo.modeling.models.foundationstereo.core import submodule
    from stereo.modeling.models.fast_foundationstereo.core import submodule as fast
    out = {}
    for case in M.GOLDEN_CASES:
        ys = []
        for cls in (submodule.Conv3dNormActReduced, fast.Conv3dNormActReduced):
            mod = cls(**M.ctor_args(case))
            mod.load_state_dict(M.make_module(case).state_dict())
            if case == "fs":
                assert out.setdefault("keys", np.array(list(mod.state_dict()))).tolist() == list(mod.state_dict())
            with torch.no_grad():
                y = mod.eval()(M.make_input(case))
            assert y.dtype == torch.float32 and tuple(y.shape) == M.out_shape(case)
            ys.append(y.contiguous().numpy())
        assert np.array_equal(ys[0], ys[1]), f"{case}: the two reference copies differ"
        out[f"{case}__y"] = ys[0]
    np.savez_compressed(M.GOLDEN, **out)
    print(f"wrote {M.GOLDEN}: {os.path.getsize(M.GOLDEN) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
