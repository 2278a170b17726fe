#!/usr/bin/env python3
"""Worst error of the causal real convolution plans against fp64, per case and class: the source of K_LCONV_FUSED /
K_LCONV_COMPOSED (tests/lconv_ref.py), as tools/conv_accuracy.py is the source of the complex convolution's constants.

    python tools/lconv_accuracy.py [--seeds 1 2 3] [--out profiles/lconv_ulps.txt]

Cases: lconv_ref.FUSED_CASES and COMPOSED_CASES (what tests/test_gpu_lconv.py runs) x the five tap kinds x the seeds. Reference: fp64
with the binary16 spectrum the plan built (tfft_lconv_plan_spectrum), on the L kept samples of every sequence. Unit: binary16 ulps
of the largest |y| of each pair's full linear convolution; the rel-L2 of the worst pair is listed beside it. The last lines give
the worst value of each class and the constant the project's rule makes of it (the smallest half-integer >= 1.5 x worst, at most 4)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lconv_ulps.txt"))
    args = ap.parse_args()

    import torch

    import __graft_entry__ as g

    g.build()
    import elementwise_bound as eb
    import lconv_ref as lr
    import tensor_fft_amd as tf

    dev = "cuda:0"
    lines = ["# tools/lconv_accuracy.py: worst error of the L kept samples against fp64 ifft(fft(zero-padded pair) * H), H = the binary16",
             "# spectrum the plan built, in binary16 ulps of the largest |y| of each pair's full linear convolution; seeds "
             f"{args.seeds}; inputs uniform(-1, 1) binary16",
             "# n L K B C launch_iters path taps : worst ulp (seed) | worst rel-L2"]
    cls = {"fused": (0.0, 0.0), "composed": (0.0, 0.0)}
    cases = [(4096, c[0], c[1], c[2], c[3], c[4], False) for c in lr.FUSED_CASES] + [(c[0], c[1], c[2], c[3], c[4], 0, c[5]) for c in lr.COMPOSED_CASES]
    for n, length, taps, rows, channels, iters, flag in cases:
        path = "fused" if n == 4096 and not flag else "composed"
        plan = tf.TfftCausalConvPlan(rows, channels, length, taps, 0, launch_iters=iters, composed=flag)
        assert plan.n == n and (plan.num_launches == 1) == (path == "fused")
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
                got_re, got_im = lr.pair_planes(y, length)
                peak = lr.pair_peak(lr.reference_taps(x, h, n))
                ref = lr.reference_spectrum(x, spec[0], spec[1], n)[:, :length]
                if rows % 2:
                    ref[-channels:].imag = 0.0
                e = float(eb.errors_in_ulps(got_re, got_im, ref.real, ref.imag, peak=peak).max())
                rel = float(np.sqrt((((got_re - ref.real) ** 2 + (got_im - ref.imag) ** 2).sum(-1) / (np.abs(ref) ** 2).sum(-1))).max())
                if e > worst:
                    worst, worst_seed = e, seed
                worst_rel = max(worst_rel, rel)
            lines.append(f"{n} {length} {taps} {rows} {channels} {iters} {path} {kind} : {worst:.3f} ({worst_seed}) | {worst_rel:.2e}")
            print(lines[-1], flush=True)
            cls[path] = (max(cls[path][0], worst), max(cls[path][1], worst_rel))
        plan.close()
    for path, (w, rel) in cls.items():
        k = min(4.0, math.ceil(1.5 * w * 2) / 2)
        lines.append(f"class worst {path}: {w:.3f} ulp, rel-L2 {rel:.2e} -> K = {k}" + (" (the ceiling)" if 1.5 * w > 4 else ""))
        print(lines[-1])
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
