#!/usr/bin/env python3
"""Worst error of the seven convolution add-ons at the upper edge of their range contract, per kernel and corner, beside the
amplitude-1 class worst of the add-on's own profile: whether the constants measured on uniform(-1, 1) data hold at the edge.

    python tools/range_accuracy.py [--seeds 1 2 3] [--out profiles/range_ulps.txt]

Cases, tap kinds and corners: range_ref.upper_edge_params() (what tests/test_gpu_conv_range.py runs) x the seeds. Every data set goes
through the add-on's own check function (tests/test_gpu_<add-on>.py via test_gpu_conv_range.run_checks), so the figure is the one that
test asserts on: binary16 ulps of the unit of the add-on's constant against fp64 with the plan's own spectrum; for a plan with a
gate behind the transform, and for the tap gradients, the ratio of the error to the asserted tolerance. A check that fails is listed
with its message instead of a figure: a finite result above its constant is a finding to be explained from the code."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# the amplitude-1 class worst of each add-on's own profile, and the constant made of it
AMPLITUDE_1 = {
    "conv": "profiles/conv_ulps.txt: fused 2.102 ulp (K 3.5), composed 2.560 ulp (K 4.0)",
    "lconv": "profiles/lconv_ulps.txt: fused 2.113 ulp, composed 2.113 ulp (K 3.5)",
    "gconv": "profiles/lconv_ulps.txt (bit for bit the causal plans between two binary16 products): 2.113 ulp (K 3.5)",
    "sconv": "profiles/sconv_ulps.txt: full pairs 2.100 ulp, zero partner 3.000 ulp in its own unit (K 4.0, the ceiling)",
    "gsconv": "profiles/sconv_ulps.txt (bit for bit the overlap-save plan between two binary16 products); ratio to |g| K ulp + 1/2 ulp",
    "bconv_dx": "profiles/bconv_ulps.txt: full pairs 2.000 ulp, zero partner 3.000 ulp in its own unit (K 4.0)",
    "gbconv_dx": "profiles/gbconv_ulps.txt: dx 0.939, dpre 0.922 of the asserted tolerance",
    "bconv_dh": "profiles/bconv_ulps.txt: at most 0.142 of the derived bound",
    "gbconv_dh": "profiles/gbconv_ulps.txt: at most 0.187 of the derived bound",
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_ulps.txt"))
    args = ap.parse_args()

    import __graft_entry__ as g

    g.build()
    import range_ref as rr
    import tensor_fft_amd as tf
    import test_gpu_conv_range as tr

    tf.device_check(0)
    lines = ["# tools/range_accuracy.py: worst error at the upper edge of the range contract (tests/range_ref.py: every contract quantity within a",
             f"# factor 2 of its limit), through the add-on's own check function; seeds {args.seeds}. Unit: binary16 ulps of the unit of the add-on's",
             "# constant, against fp64 with the plan's own spectrum; gsconv, gbconv_dx and the tap gradients: error / asserted tolerance.",
             "# add-on case kind corner : binding quantity at its share of the limit (seed 1) : worst (seed) | constant"]
    worst_of = {}
    findings = []
    for addon, case, kind, corner in rr.upper_edge_params():
        worst, worst_seed, text = 0.0, 0, ""
        for seed in args.seeds:
            d = rr.upper_edge_data(addon, case, kind, corner, seed)
            if seed == args.seeds[0]:
                name, ratio = rr.binding(d)
                text = f"{name} {ratio:.3f}"
            try:
                w = float(tr.run_checks(tf, d))
            except AssertionError as e:
                findings.append(f"FAILED {addon} {case} {kind} {corner} seed {seed}: {str(e).splitlines()[0][:300]}")
                print(findings[-1], flush=True)
                continue
            if w > worst:
                worst, worst_seed = w, seed
        ratio_unit = addon in ("gsconv", "gbconv_dx") + rr.TAP_GRADS
        bound = "1 (ratio)" if ratio_unit else f"K {tr.constant_of(rr.upper_edge_data(addon, case, kind, corner, args.seeds[0]))}"
        lines.append(f"{addon} {' '.join(map(str, case))} {kind} {corner} : {text} : {worst:.3f} ({worst_seed}) | {bound}")
        print(lines[-1], flush=True)
        key = (addon, corner)
        if worst > worst_of.get(key, (0.0, ""))[0]:
            worst_of[key] = (worst, f"{' '.join(map(str, case))} {kind}")
    lines.append("# worst per add-on and corner, beside the amplitude-1 class worst of the add-on's own profile")
    for addon in rr.FORWARD + rr.TAP_GRADS:
        lines.append(f"# {addon}: amplitude 1: {AMPLITUDE_1[addon]}")
        for corner in rr.corners_of(addon):
            w, where = worst_of.get((addon, corner), (0.0, "-"))
            lines.append(f"worst {addon} {corner}: {w:.3f} ({where})")
            print(lines[-1])
    lines.append(f"checks that failed: {len(findings)}")
    lines += findings
    print(lines[-1] if not findings else "\n".join(findings))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
