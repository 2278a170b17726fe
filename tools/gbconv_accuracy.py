#!/usr/bin/env python3
"""Worst error of the gradient plans of the gated overlap-save causal convolution against fp64, per case (include/tfft_gbconv.h).

    python tools/gbconv_accuracy.py [--seeds 1 2 3] [--out profiles/gbconv_ulps.txt]

Input gradient: gsconv_ref.CASE_MODES x the two tap kinds x the seeds. dx and dpre against gate (.) fp64 of the SAME rounded
gz = post (.) gy with the conjugate of the binary16 spectrum the plan built, sample by sample, as a ratio to the tolerance
tests/test_gpu_gbconv.py asserts (|gate| K_SCONV ulp16(peak of the window) + 1/2 ulp16(|result|); without a pre gate K_SCONV
ulp16(peak)), with the rel-L2 of the worst sequence beside it.
Tap gradient: gbconv_ref.DH_CASE_MODES x the seeds, against direct fp64 sums over the rounded products u = pre (.) x and gz: the worst
ratio of a tap's error to the derived bound of tests/bconv_ref.py, and the rel-L2 of a channel's taps."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gbconv_ulps.txt"))
    args = ap.parse_args()

    import torch

    import __graft_entry__ as g

    g.build()
    import bconv_ref as br
    import elementwise_bound as eb
    import gbconv_ref as gb
    import gsconv_ref as gs
    import sconv_ref as sr
    import tensor_fft_amd as tf

    dev = "cuda:0"

    def to_dev(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev)

    lines = ["# tools/gbconv_accuracy.py, input gradient: worst error of dx and dpre against gate (.) fp64 ifft(fft(window of post (.) gy) * conj(H')),",
             "# H' = the binary16 spectrum the plan built, as a ratio to |gate| K_SCONV ulp16(peak of the window) + 1/2 ulp16(|result|) "
             f"(K_SCONV ulp16(peak) without a pre gate); seeds {args.seeds}",
             "# L K B C launch_iters mode taps : dx worst ratio (seed) | dx worst rel-L2 | dpre worst ratio (seed) | dpre worst rel-L2"]
    cls = {"dx": [0.0, "", 0.0], "dpre": [0.0, "", 0.0]}
    for length, taps, rows, channels, iters, mode in gb.DX_CASE_MODES:
        has_pre, has_post, _ = gb.GATE_MODES[mode]
        plan = tf.TfftGatedLongConvGradPlan(rows, channels, length, taps, 0, pre_gate=has_pre, post_gate=has_post, launch_iters=iters)
        for kind in gb.TAP_KINDS:
            worst = {"dx": [0.0, 0, 0.0], "dpre": [0.0, 0, 0.0]}
            for seed in args.seeds:
                x, h, pre, post, skip, gy = gb.case_data(length, taps, rows, channels, kind, seed, mode)
                plan.set_taps(to_dev(h), to_dev(skip))
                spec = br.conj_spectrum(*(t.cpu().numpy() for t in plan.spectrum()))
                d_dx = torch.empty(gy.size, dtype=torch.float16, device=dev)
                d_dpre = torch.empty_like(d_dx) if has_pre else None
                plan.input_grad(to_dev(gy), d_dx, post=to_dev(post), x=to_dev(x) if has_pre else None, pre=to_dev(pre), dpre=d_dpre)
                torch.cuda.synchronize()
                gz = gb.gated(gy, post)
                peak = gb.du_peak(gz, h, skip)
                ref = br.dx_reference_spectrum(gz, taps, *spec)
                du = br.dx_unwindow(ref.real, ref.imag, rows, channels, length, taps)
                for name, d_out, gate in (("dx", d_dx, pre), ("dpre", d_dpre, x)):
                    if d_out is None:
                        continue
                    got = d_out.cpu().numpy().reshape(gy.shape)
                    if has_pre:
                        want = gate.astype(np.float64) * du
                        tol = gs.post_gate_tolerance(got, gate, gb.K_SCONV, peak, rows, channels, length, taps)
                    else:
                        want, tol = du, gb.K_SCONV * gb.per_sample(eb.ulp16(peak), rows, channels, length, taps)
                    err = np.abs(got.astype(np.float64) - want)
                    ratio = float((err / tol).max())
                    den = (want ** 2).sum(-1)
                    rel = float(np.sqrt((err ** 2).sum(-1)[den > 0] / den[den > 0]).max())
                    if ratio > worst[name][0]:
                        worst[name][:2] = [ratio, seed]
                    worst[name][2] = max(worst[name][2], rel)
            dpre_text = f"{worst['dpre'][0]:.3f} ({worst['dpre'][1]}) | {worst['dpre'][2]:.2e}" if has_pre else "- | -"
            lines.append(f"{length} {taps} {rows} {channels} {iters} {mode} {kind} : {worst['dx'][0]:.3f} ({worst['dx'][1]}) | {worst['dx'][2]:.2e} | {dpre_text}")
            print(lines[-1], flush=True)
            for name in cls:
                if worst[name][0] > cls[name][0]:
                    cls[name][:2] = [worst[name][0], f"L {length}, K {taps}, {rows} x {channels}, {mode}, {kind}"]
                cls[name][2] = max(cls[name][2], worst[name][2])
        plan.close()
    for name in cls:
        lines.append(f"class worst {name}: {cls[name][0]:.3f} of the asserted tolerance ({cls[name][1]}), rel-L2 {cls[name][2]:.2e}; K_SCONV = {sr.K_SCONV}")
        print(lines[-1])

    lines += ["# tap gradient: every tap against direct fp64 sums over u = pre (.) x and gz = post (.) gy as the kernel rounds them; ratio = |error| / bound,",
              f"# bound = sum over the channel's items of ({br.K_CONV_FUSED} + {br.A_SPECTRUM}) * ulp16(peak of the item / 4096) * 4096 (tests/bconv_ref.py)",
              "# L K B C cap mode P items/channel : worst ratio (seed) | worst rel-L2 of a channel"]
    dh_worst, dh_rel, dh_case = 0.0, 0.0, ""
    for length, taps, rows, channels, cap, mode in gb.DH_CASE_MODES:
        has_pre, has_post, _ = gb.GATE_MODES[mode]
        plan = tf.TfftGatedLongConvGradPlan(rows, channels, length, taps, 0, pre_gate=has_pre, post_gate=has_post, partials=cap)
        worst, worst_seed, worst_rel = 0.0, 0, 0.0
        for seed in args.seeds:
            x, _, pre, post, _, gy = gb.case_data(length, taps, rows, channels, "noise", seed, mode)
            d_dh = torch.empty(channels * taps, dtype=torch.float32, device=dev)
            plan.tap_grad(to_dev(x), to_dev(gy), d_dh, pre=to_dev(pre), post=to_dev(post))
            torch.cuda.synchronize()
            dh = d_dh.cpu().numpy().reshape(channels, taps).astype(np.float64)
            u, gz = gb.gated(x, pre), gb.gated(gy, post)
            want = br.dh_direct(u, gz, taps)
            bound = br.dh_bound(br.dh_items(u, gz, taps), channels)
            ratio = float((np.abs(dh - want) / bound[:, None]).max())
            rel = float(np.sqrt(((dh - want) ** 2).sum(-1) / (want ** 2).sum(-1)).max())
            if ratio > worst:
                worst, worst_seed = ratio, seed
            worst_rel = max(worst_rel, rel)
        lines.append(f"{length} {taps} {rows} {channels} {cap} {mode} {plan.partials} {gb.items_per_channel((length, taps, rows))} : {worst:.3f} ({worst_seed}) | {worst_rel:.2e}")
        print(lines[-1], flush=True)
        if worst > dh_worst:
            dh_worst, dh_case = worst, f"L {length}, K {taps}, {rows} x {channels}, cap {cap}, {mode}"
        dh_rel = max(dh_rel, worst_rel)
        plan.close()
    lines.append(f"class worst wgrad: {dh_worst:.3f} of the derived bound ({dh_case}), rel-L2 {dh_rel:.2e}")
    print(lines[-1])
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
