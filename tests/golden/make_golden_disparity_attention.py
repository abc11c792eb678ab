"""Generate tests/golden/disparity_attention.npz by running the REAL reference's CostVolumeDisparityAttention on the CPU.

Runs only where the reference is mounted (CPU torch).  models/foundationstereo/core/submodule.py (lines 195-291, 506-562) is imported
through stub parent packages, as in the other generators, with two more stubs for what the file imports and this class does not use: an
empty module stereo.modeling.models.foundationstereo.Utils, and a flash_attn module whose flash_attn_func and flash_attn_qkvpacked_func
are None (fp32 tensors go through F.scaled_dot_product_attention).  The class is built with the case's arguments, takes the seeded
state_dict of the restatement in tests/disparity_attention_cases.py (the keys match) and runs in eval mode on the seeded input.

The case `resize` runs a second time with the fast copy's PositionalEmbedding (fast_foundationstereo/core/submodule.py:547-577, which
resizes with align_corners=True) in the place of pos_embed0; that file imports a top-level `Utils` with an AMP_DTYPE, stubbed likewise.

Stored: the fp32 outputs only, for the cases named by disparity_attention_cases.GOLDEN_CASES, keyed `<case>__y`, `resize__y_fast`, and
the state_dict keys of the `fs416` reference module as `keys`.  Parameters and inputs are not stored: tests regenerate them from the seeds.

    python tests/golden/make_golden_disparity_attention.py
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

import disparity_attention_cases as M  # noqa: E402


def import_reference():
    if not os.path.isdir(REF):
        raise SystemExit(f"{REF} not found: golden vectors can only be generated where the reference is mounted")
    sys.path.insert(0, REF)
    models = "stereo/modeling/models"
    for name, path in [("stereo", "stereo"), ("stereo.modeling", "stereo/modeling"), ("stereo.modeling.models", models),
                       ("stereo.modeling.models.foundationstereo", models + "/foundationstereo"),
                       ("stereo.modeling.models.foundationstereo.core", models + "/foundationstereo/core"),
                       ("stereo.modeling.models.fast_foundationstereo", models + "/fast_foundationstereo"),
                       ("stereo.modeling.models.fast_foundationstereo.core", models + "/fast_foundationstereo/core")]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, path)]
        sys.modules[name] = m
    sys.modules["stereo.modeling.models.foundationstereo.Utils"] = types.ModuleType("stereo.modeling.models.foundationstereo.Utils")
    flash = types.ModuleType("flash_attn")
    flash.flash_attn_func = flash.flash_attn_qkvpacked_func = None
    sys.modules["flash_attn"] = flash
    utils = types.ModuleType("Utils")
    utils.AMP_DTYPE = torch.float16
    sys.modules["Utils"] = utils
    from stereo.modeling.models.foundationstereo.core import submodule
    from stereo.modeling.models.fast_foundationstereo.core import submodule as fast
    return submodule.CostVolumeDisparityAttention, fast.PositionalEmbedding


def main():
    ref_cls, fast_pe = import_reference()
    out = {}
    for case in M.GOLDEN_CASES:
        B, C, nhead, ff, layers, L, max_len, resize, H, W = M.CASES[case]
        mod = ref_cls(C, nhead, ff, num_transformer=layers, max_len=max_len, resize_embed=resize)
        mod.load_state_dict(M.make_module(case).state_dict())
        if case == "fs416":
            out["keys"] = np.array(list(mod.state_dict()))
        with torch.no_grad():
            y = mod.eval()(M.make_input(case))
            assert y.dtype == torch.float32 and tuple(y.shape) == M.out_shape(case)
            out[f"{case}__y"] = y.contiguous().numpy()
            if case == "resize":
                mod.pos_embed0 = fast_pe(C, max_len=max_len)
                out["resize__y_fast"] = mod(M.make_input(case)).contiguous().numpy()
                assert not np.array_equal(out["resize__y_fast"], out["resize__y"])
    np.savez_compressed(M.GOLDEN, **out)
    print(f"wrote {M.GOLDEN}: {os.path.getsize(M.GOLDEN) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
