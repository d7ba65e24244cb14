"""The CPU part of profiles/epipolar_reference.txt: the fp64 oracle's error / sensitivity ratios and the margins, the cubic cases
before (80 halvings) and after, and the search over 1e5 seven-point samples.  python scripts/epipolar_reference_profile.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import ransac_oracle as RO                    # noqa: E402
from tests import epipolar_reference as ER                # noqa: E402
from tests import test_epipolar_reference as T            # noqa: E402


def main():
    m = T.measure_ratios()
    print("== oracle error / sensitivity, first 96 hypotheses of each planted case ==")
    print(f"homography  planted(200, 40, 0): {len(m['homography'])} models, worst {max(m['homography']):.4g}   -> MEASURED_H {ER.MEASURED_H:g}, MARGIN_H = 16 x = {ER.MARGIN_H:.4g}")
    for k, v in m["fundamental"].items():
        print(f"fundamental {k}: {len(v)} models, worst {max(v):.4g}; samples with 0/1/2/3 real solutions {m['solutions'][k]} (oracle and reference agree on every count)")
    print(f"   -> MEASURED_F {ER.MEASURED_F:g}, MARGIN_F = 16 x = {ER.MARGIN_F:.4g}")
    print("\n== cubics: worst |root - reference| / (8 x eps-conditioning) over the well separated roots; roots found / reference ==")
    print(f"{'case':14s} {'80 halvings (parent)':>28s} {'now':>22s}")
    for name, c in T.CUBICS.items():
        if not name.startswith(("c3small", "wide", "atR", "critical", "double")):
            continue
        row = []
        for refine in (False, True):
            RO.REFINE = refine
            rows, n_ref, n_got = T.cubic_errors(c)
            w = max([e for _t, e, sep in rows if sep], default=0.0)
            row.append(f"{w:12.4g} ({n_got}/{n_ref})")
        RO.REFINE = True
        print(f"{name:14s} {row[0]:>28s} {row[1]:>22s}   c = {c}")
    print("\n== search: random seven-point samples, largest R / |t| over the real roots (inf: a root at t = 0) ==")
    for refine in (False, True):
        RO.REFINE = refine
        s = T.search()
        if refine:
            for k, v in s["by_kind"].items():
                print(f"  {k:26s} {v['samples']:6d} samples, largest R/|t| {v['worst'] if v['worst'] < 1e300 else float('inf'):.4g}")
        print(f"{'now' if refine else '80 halvings (parent)'}: {s['samples']} samples; {s['checked']} held to the 50-digit reference (the 40 largest R/|t| and 40 at random): "
              f"worst error / sensitivity {s['worst_model_ratio']:.4g} (margin {ER.MARGIN_F:.4g}), outside the tolerance: {len(s['outside'])}")
    RO.REFINE = True


if __name__ == "__main__":
    main()
