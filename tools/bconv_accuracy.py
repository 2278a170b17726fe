#!/usr/bin/env python3
"""Worst error of the gradient plans of the overlap-save causal convolution against fp64, per case (include/tfft_bconv.h).

    python tools/bconv_accuracy.py [--seeds 1 2 3] [--out profiles/bconv_ulps.txt]

Input gradient: sconv_ref.CASES x the five tap kinds x the seeds, against fp64 with the conjugate of the binary16 spectrum the plan
built, window by window, on the samples a window keeps; in binary16 ulps of the largest magnitude of each window's 4096-point
circular result, the unit of tools/sconv_accuracy.py and K_SCONV, with the rel-L2 of the worst window beside it.
Tap gradient: bconv_ref.DH_CASES x the seeds (the taps do not enter), against direct fp64 sums: the worst ratio of a tap's error to
the derived bound of tests/bconv_ref.py (above 1 anywhere, the derivation is wrong), and the rel-L2 of a channel's taps."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bconv_ulps.txt"))
    args = ap.parse_args()

    import torch

    import __graft_entry__ as g

    g.build()
    import bconv_ref as br
    import elementwise_bound as eb
    import lconv_ref as lr
    import sconv_ref as sr
    import tensor_fft_amd as tf

    dev = "cuda:0"
    lines = ["# tools/bconv_accuracy.py, input gradient: worst error of the kept samples of every window against fp64 ifft(fft(window) * conj(H)),",
             "# H = the binary16 spectrum the plan built, in binary16 ulps of the largest magnitude of the window's 4096-point circular result; seeds "
             f"{args.seeds}; g uniform(-1, 1) binary16",
             "# L K B C launch_iters halo hop segments taps : worst ulp (seed) | worst rel-L2"]
    cls_worst, cls_rel, cls_case = 0.0, 0.0, ""
    split = {"full pairs": [0.0, ""], "zero partner": [0.0, ""]}
    for length, taps, rows, channels, iters in sr.CASES:
        halo, hop, segs = sr.geometry(length, taps)
        plan = tf.TfftLongConvGradPlan(rows, channels, length, taps, 0, launch_iters=iters)
        for kind in lr.TAP_KINDS:
            worst, worst_seed, worst_rel = 0.0, 0, 0.0
            for seed in args.seeds:
                _, h = lr.case_data(length, taps, rows, channels, kind, seed)
                gr = br.grad_signal(rows, channels, length, taps, seed)
                plan.set_taps(torch.from_numpy(h.reshape(-1)).to(dev))
                spec = br.conj_spectrum(*(t.cpu().numpy() for t in plan.spectrum()))
                d_g = torch.from_numpy(gr.reshape(-1)).to(dev)
                d_dx = torch.empty_like(d_g)
                plan.input_grad(d_g, d_dx)
                torch.cuda.synchronize()
                dx = d_dx.cpu().numpy().reshape(gr.shape).astype(np.float64)
                got_re, got_im = (br.dx_kept(p, rows, channels, length, taps) for p in br.dx_windows(dx, taps))
                peak = sr.window_peak(br.dx_reference_taps(gr, h))
                ref = br.dx_reference_spectrum(gr, taps, *spec)
                if rows % 2:
                    ref[-segs * channels:].imag = 0.0
                ref = br.dx_kept(ref, rows, channels, length, taps)
                per_window = eb.errors_in_ulps(got_re, got_im, ref.real, ref.imag, peak=peak).max(axis=1)
                e = float(per_window.max())
                lone = np.zeros(per_window.size, bool)
                if rows % 2:
                    lone[-segs * channels:] = True
                for name, mask in (("full pairs", ~lone), ("zero partner", lone)):
                    if mask.any() and per_window[mask].max() > split[name][0]:
                        split[name] = [float(per_window[mask].max()), f"L {length}, K {taps}, {rows} x {channels}, {kind}, seed {seed}"]
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
    for name, (w, case) in split.items():
        lines.append(f"worst over the windows of {name}: {w:.3f} ulp ({case})")
        print(lines[-1])
    lines.append(f"class worst dgrad: {cls_worst:.3f} ulp ({cls_case}), rel-L2 {cls_rel:.2e}; K_SCONV = {sr.K_SCONV}")
    print(lines[-1])

    lines += ["# tap gradient: every tap against direct fp64 sums; ratio = |error| / bound, bound = sum over the channel's items of",
              f"# ({br.K_CONV_FUSED} + {br.A_SPECTRUM}) * ulp16(peak of the item / 4096) * 4096 (tests/bconv_ref.py); x and g uniform(-1, 1) binary16",
              "# L K B C cap P items/channel : worst ratio (seed) | worst rel-L2 of a channel | bound / rms tap"]
    dh_worst, dh_rel, dh_case = 0.0, 0.0, ""
    for length, taps, rows, channels, cap in br.DH_CASES:
        plan = tf.TfftLongConvGradPlan(rows, channels, length, taps, 0, partials=cap)
        worst, worst_seed, worst_rel, loose = 0.0, 0, 0.0, 0.0
        for seed in args.seeds:
            x, _ = lr.case_data(length, taps, rows, channels, "noise", seed)
            gr = br.grad_signal(rows, channels, length, taps, seed)
            d_dh = torch.empty(channels * taps, dtype=torch.float32, device=dev)
            plan.tap_grad(torch.from_numpy(x.reshape(-1)).to(dev), torch.from_numpy(gr.reshape(-1)).to(dev), d_dh)
            torch.cuda.synchronize()
            dh = d_dh.cpu().numpy().reshape(channels, taps).astype(np.float64)
            want = br.dh_direct(x, gr, taps)
            bound = br.dh_bound(br.dh_items(x, gr, taps), channels)
            ratio = float((np.abs(dh - want) / bound[:, None]).max())
            rel = float(np.sqrt(((dh - want) ** 2).sum(-1) / (want ** 2).sum(-1)).max())
            loose = max(loose, float((bound / np.sqrt((want ** 2).mean(-1))).max()))
            if ratio > worst:
                worst, worst_seed = ratio, seed
            worst_rel = max(worst_rel, rel)
        per_channel = (rows + 1) // 2 * sr.geometry(length, taps)[2]
        lines.append(f"{length} {taps} {rows} {channels} {cap} {plan.partials} {per_channel} : {worst:.3f} ({worst_seed}) | {worst_rel:.2e} | {loose:.2e}")
        print(lines[-1], flush=True)
        if worst > dh_worst:
            dh_worst, dh_case = worst, f"L {length}, K {taps}, {rows} x {channels}, cap {cap}"
        dh_rel = max(dh_rel, worst_rel)
        plan.close()
    lines.append(f"class worst wgrad: {dh_worst:.3f} of the derived bound ({dh_case}), rel-L2 {dh_rel:.2e}")
    print(lines[-1])
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
