"""No GPU: (1) the inputs of tests/test_gpu_geo_lookup_edges.py reach the tap sequences the accumulating lookup backward used to get
wrong, (2) the float64 reference those tests use is validated against the same oracle in float32."""
import numpy as np
import pytest
import torch

import geo_lookup_cases as K


@pytest.mark.parametrize("case", list(K.CASES))
def test_lattice_sets_reach_gap_and_same_tap_pairs(case):
    """tap_of() maps a position x through g = 2x/(n-1) - 1 and back, each step rounded to float32, so an integer x returns as k - eps or
    k + eps and consecutive taps do not always have consecutive x0 (and for x one ulp beside an integer the sums dx + x round differently
    from tap to tap).  Every case must show, in the geometry rows and in the correlation rows, at least one adjacent tap pair whose x0
    differ by 2 and one whose x0 are equal, inside the row -- else the GPU tests would prove nothing about such pairs.  (The one-level radius-1 case
    was moved from D = 9 / W = 17 to D = 10 / W = 18 for this, see geo_lookup_cases.CASES.)"""
    B, C, D, H, W, Cf, L, r = K.CASES[case]
    tot = {"geo": [0, 0], "corr": [0, 0]}
    lines = []
    for s in K.LATTICE_SETS:
        for cv in K.COORDS:
            for l, (xg, xc, Dl, Wl) in enumerate(K.tap_positions(case, s, cv)):
                assert Dl >= 2 and Wl >= 2, "a level of length 1 divides by zero in the reference too"
                for kind, x, n in (("geo", xg, Dl), ("corr", xc, Wl)):
                    gap, same, other = K.count_anomalies(x, n)
                    assert other == 0, f"{case} set {s} {cv} level {l} {kind}: x0 steps outside 0..2"
                    tot[kind][0] += gap; tot[kind][1] += same
                    if gap or same:
                        lines.append(f"set {s} coords {cv} level {l} {kind} n={n}: {gap} gaps, {same} sames of {x.shape[0] * (x.shape[1] - 1)} pairs")
    report = f"{case}: geometry rows {tot['geo'][0]} gaps / {tot['geo'][1]} sames, correlation rows {tot['corr'][0]} gaps / {tot['corr'][1]} sames\n  " + "\n  ".join(lines)
    print(report)
    assert min(tot["geo"]) >= 1 and min(tot["corr"]) >= 1, report


def test_random_disparities_almost_never_reach_them():
    """the reason the existing tests (|N(0,1)| * s disparities) never saw the fault: a rate of a few 1e-6 per pair"""
    rng = np.random.default_rng(0)
    x = (np.abs(rng.normal(0, 1, (200000, 1))) * 5).astype(np.float32) + np.arange(-4, 5, dtype=np.float32).reshape(1, -1)
    gap, same, other = K.count_anomalies(x, 24)
    print(f"random disparities, n = 24: {gap} gaps, {same} sames of {x.shape[0] * 8} pairs")
    assert other == 0 and gap + same <= 40          # 1.6M pairs: 25e-6 would still be "almost never"


@pytest.mark.parametrize("case", list(K.CASES))
def test_float64_reference_vs_float32_oracle(case):
    """The oracle in float32 (what the reference project computes) against the same composition in float64 on every case, set and
    coordinate variant: forward within 0.5 of the lookup tolerance (atol 2e-5, rtol 1e-5), level gradients within 1e-5 of max |grad| (the
    GPU tests allow 1e-4).  So the tolerances leave room for a correct fp32 kernel, and none for a dropped tap (an O(|dout|) error)."""
    r64, r32 = K.reference(case, torch.float64), K.reference(case, torch.float32)
    worst_f, worst_g = 0.0, 0.0
    for s in K.SETS:
        for cv in K.COORDS:
            o64, o32 = r64.out(s, cv).double(), r32.out(s, cv).double()
            assert o64.shape == o32.shape and torch.isfinite(o64).all()
            worst_f = max(worst_f, float(((o32 - o64).abs() / (2e-5 + 1e-5 * o64.abs())).max()))
            if s == "f":
                assert not o64.any() and not o32.any()
            for g64, g32 in zip(r64.level_grads(s, cv), r32.level_grads(s, cv)):
                m = float(g64.abs().max())
                if m > 0:
                    worst_g = max(worst_g, float((g32.double() - g64).abs().max()) / m)
                else:
                    assert not g32.any()
    print(f"{case}: forward {worst_f:.3f} of the tolerance, gradients {worst_g:.2e} of max |grad|")
    assert worst_f <= 0.5, worst_f
    assert worst_g <= 1e-5, worst_g
