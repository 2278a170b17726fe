#!/usr/bin/env python3
"""Worst error of the FFT convolution plans against fp64, per case and class: the source of K_CONV_FUSED / K_CONV_COMPOSED
(tests/conv_ref.py), as tools/accuracy_per_kernel.py is the source of the complex kernels' constants.

    python tools/conv_accuracy.py [--seeds 1 2 3] [--out profiles/conv_ulps.txt]

Cases: conv_ref.CASES (what tests/test_gpu_conv.py runs) x the five filter kinds x the seeds. Unit: binary16 ulps of the largest
|y| of each signal (tests/elementwise_bound.py); the rel-L2 of the worst signal is listed beside it. The last lines give the
worst value of each class and the constant the project's rule makes of it (the smallest half-integer >= 1.5 x worst, at most 4)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_ulps.txt"))
    args = ap.parse_args()

    import torch

    import __graft_entry__ as g

    g.build()
    import conv_ref
    import elementwise_bound as eb
    import tensor_fft_amd as tf

    dev = "cuda:0"
    lines = ["# tools/conv_accuracy.py: worst error against fp64 numpy.fft.ifft(numpy.fft.fft(x) * H), in binary16 ulps of the largest |y| of",
             f"# each signal; seeds {args.seeds}; inputs uniform(-1, 1) binary16; H = the binary16 filter the plan was given",
             "# n batch filters path filter : worst ulp (seed) | worst rel-L2"]
    cls = {"fused": (0.0, 0.0), "composed": (0.0, 0.0)}
    for n, batch, filters, composed in conv_ref.CASES:
        path = "composed" if composed else "fused"
        plan = tf.TfftConvPlan(n, batch, filters, 0, composed=composed)
        for kind in conv_ref.FILTER_KINDS:
            worst, worst_seed, worst_rel = 0.0, 0, 0.0
            for seed in args.seeds:
                rng = np.random.default_rng([seed, n, batch, filters, conv_ref.FILTER_KINDS.index(kind)])
                x_re, x_im = conv_ref.signals(n, batch, rng)
                h_re, h_im = conv_ref.to_half_planes(conv_ref.make_filters(kind, n, filters, rng))
                plan.set_filter(torch.from_numpy(h_re.reshape(-1)).to(dev), torch.from_numpy(h_im.reshape(-1)).to(dev))
                x = torch.from_numpy(np.stack((x_re, x_im), axis=1).reshape(-1)).to(dev)
                y = torch.empty_like(x)
                plan.exec(x, x[n:], y, y[n:])
                torch.cuda.synchronize()
                got = y.cpu().numpy().reshape(batch, 2, n).astype(np.float64)
                r_re, r_im = conv_ref.reference(x_re, x_im, h_re, h_im)
                e = float(eb.errors_in_ulps(got[:, 0], got[:, 1], r_re, r_im).max())
                rel = float(np.sqrt((((got[:, 0] - r_re) ** 2 + (got[:, 1] - r_im) ** 2).sum(-1) / (r_re ** 2 + r_im ** 2).sum(-1))).max())
                if e > worst:
                    worst, worst_seed = e, seed
                worst_rel = max(worst_rel, rel)
            lines.append(f"{n} {batch} {filters} {path} {kind} : {worst:.3f} ({worst_seed}) | {worst_rel:.2e}")
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
