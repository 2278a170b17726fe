#!/usr/bin/env python3
"""Worst error of the overlap-save causal convolution plans against fp64, per case: the source of K_SCONV (tests/sconv_ref.py), as
tools/lconv_accuracy.py is the source of the causal plans' constants.

    python tools/sconv_accuracy.py [--seeds 1 2 3] [--out profiles/sconv_ulps.txt]

Cases: sconv_ref.CASES (what tests/test_gpu_sconv.py runs) x the five tap kinds x the seeds. Reference: fp64 with the binary16
spectrum the plan built (tfft_sconv_plan_spectrum), window by window, on the samples a window keeps. Unit: binary16 ulps of the
largest magnitude of each window's 4096-point circular convolution; the rel-L2 of the worst window is listed beside it. The last
lines give the worst value, split into the windows of full pairs and those of a zero partner (the last row of an odd count: a real
signal, whose peak and with it the unit is that of one row), and the constant the project's rule makes of the worst value (the
smallest half-integer >= 1.5 x worst, at most 4)."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sconv_ulps.txt"))
    args = ap.parse_args()

    import torch

    import __graft_entry__ as g

    g.build()
    import elementwise_bound as eb
    import lconv_ref as lr
    import sconv_ref as sr
    import tensor_fft_amd as tf

    dev = "cuda:0"
    lines = ["# tools/sconv_accuracy.py: worst error of the kept samples of every window against fp64 ifft(fft(window) * H), H = the binary16",
             "# spectrum the plan built, in binary16 ulps of the largest magnitude of the window's 4096-point circular convolution; seeds "
             f"{args.seeds}; inputs uniform(-1, 1) binary16",
             "# L K B C launch_iters halo hop segments taps : worst ulp (seed) | worst rel-L2"]
    cls_worst, cls_rel, cls_case = 0.0, 0.0, ""
    split = {"full pairs": [0.0, "", 0.0], "zero partner": [0.0, "", 0.0]}          # worst ulp, case, peak of that window
    for length, taps, rows, channels, iters in sr.CASES:
        halo, hop, segs = sr.geometry(length, taps)
        plan = tf.TfftLongConvPlan(rows, channels, length, taps, 0, launch_iters=iters)
        assert (plan.halo, plan.hop, plan.segments) == (halo, hop, segs) and plan.num_launches == 1
        for kind in lr.TAP_KINDS:
            worst, worst_seed, worst_rel = 0.0, 0, 0.0
            for seed in args.seeds:
                x, h = lr.case_data(length, taps, rows, channels, kind, seed)
                plan.set_taps(torch.from_numpy(h.reshape(-1)).to(dev))
                spec = tuple(t.cpu().numpy() for t in plan.spectrum())
                d_x = torch.from_numpy(x.reshape(-1)).to(dev)
                d_y = torch.empty_like(d_x)
                plan.exec(d_x, d_y)
                torch.cuda.synchronize()
                y = d_y.cpu().numpy().reshape(x.shape).astype(np.float64)
                got_re, got_im = (sr.kept(p, rows, channels, length, taps) for p in sr.windows(y, taps))
                peak = sr.window_peak(sr.reference_taps(x, h))
                ref = sr.reference_spectrum(x, taps, spec[0], spec[1])
                if rows % 2:
                    ref[-segs * channels:].imag = 0.0
                ref = sr.kept(ref, rows, channels, length, taps)
                per_window = eb.errors_in_ulps(got_re, got_im, ref.real, ref.imag, peak=peak).max(axis=1)
                e = float(per_window.max())
                lone = np.zeros(per_window.size, bool)
                if rows % 2:
                    lone[-segs * channels:] = True
                for name, mask in (("full pairs", ~lone), ("zero partner", lone)):
                    if mask.any() and per_window[mask].max() > split[name][0]:
                        i = int(np.flatnonzero(mask)[np.argmax(per_window[mask])])
                        split[name] = [float(per_window[i]), f"L {length}, K {taps}, {rows} x {channels}, {kind}, seed {seed}, item {i}", float(peak[i])]
                rel = float(np.sqrt((((got_re - ref.real) ** 2 + (got_im - ref.imag) ** 2).sum(-1) / (np.abs(ref) ** 2).sum(-1))).max())
                if e > worst:
                    worst, worst_seed = e, seed
                worst_rel = max(worst_rel, rel)
            lines.append(f"{length} {taps} {rows} {channels} {iters} {halo} {hop} {segs} {kind} : {worst:.3f} ({worst_seed}) | {worst_rel:.2e}")
            print(lines[-1], flush=True)
            if worst > cls_worst:
                cls_worst, cls_case = worst, f"L {length}, K {taps}, {rows} x {channels}, {kind}"
            cls_rel = max(cls_rel, worst_rel)
        plan.close()
    for name, (w, case, pk) in split.items():
        lines.append(f"worst over the windows of {name}: {w:.3f} ulp ({case}; that window's peak {pk:.4f}, unit 2^{int(np.log2(eb.ulp16(pk)))})")
        print(lines[-1])
    k = min(4.0, math.ceil(1.5 * cls_worst * 2) / 2)
    lines.append(f"class worst sconv: {cls_worst:.3f} ulp ({cls_case}), rel-L2 {cls_rel:.2e} -> K = {k}" + (" (the ceiling)" if 1.5 * cls_worst > 4 else ""))
    print(lines[-1])
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
