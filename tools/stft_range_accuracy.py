#!/usr/bin/env python3
"""The STFT, short-frame STFT and ISTFT plans at the edges of their range contract: per data set of tests/stft_range_ref.py the binding
quantity's share of its limit and the worst rel-L2 against fp64, for the CPU model of the kernels and for the GPU side by side, and
the round-trip table istft(stft(x 2^e)) against x 2^e.

    python tools/stft_range_accuracy.py [--seeds 1 2 3] [--out profiles/stft_range.txt] [--model-only]

Forward sets: worst frame's rel-L2 against fp64 rfft / n of the binary16 products, and in how many halves the plan differs from
TfftRealPlan.r2c on host-built frames (0: bit for bit). Inverse sets: worst signal's rel-L2 against the fp64 ISTFT of the same
spectra, and in how many halves the workspace frames and y differ from the two yardsticks of tests/test_gpu_istft.py. For the
lower-edge sets rel-L2 says little (tests/test_stft_range_host.py): the bits hold them. --model-only writes the CPU columns and "not
measured" for the GPU (no GPU, no build)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _rel(got, want):
    import stft_range_ref as sr

    with np.errstate(invalid="ignore", divide="ignore"):
        return float(sr.rel_l2(got, want).max())


def forward_row(sr, d, gpu):
    """(model's worst rel-L2, the GPU's or None, halves that differ from the real plan or None)"""
    want = sr.reference(d)
    m = _rel(sr.as_complex(*sr.model(d)), want)
    if gpu is None:
        return m, None, None
    tr, tf = gpu
    re, im = tr.run_forward(tf, d)
    w_re, w_im = tr.via_real_plan(tf, d)
    return m, _rel(sr.as_complex(re.view(np.float16), im.view(np.float16)), want), int((re != w_re).sum() + (im != w_im).sum())


def inverse_row(sr, ir, d, gpu):
    want = sr.reference(d)
    m = _rel(sr.model(d)[1].astype(np.float64), want)
    if gpu is None:
        return m, None, None
    tr, tf = gpu
    geo = (d["rows"], d["length"], d["hop"], d["pad"])
    frames, y = tr.t_istft.run_istft(tf, d["re"].copy(), d["im"].copy(), d["w"].copy(), *geo)
    zr, zi = ir.merge_items(d["re"], d["im"])
    differ = int((frames != tr.t_istft.via_inverse_plan(tf, zr, zi, d["re"].shape[0])).sum())
    differ += int((y != ir.ola(frames.view(np.float16), d["w"], *geo).view(np.int16)).sum())
    return m, _rel(y.view(np.float16).astype(np.float64), want), differ


def gpu_round_trip(sr, ir, tf, torch, e, seed):
    rows, length, hop, pad = sr.ROUND_TRIP_SHAPE
    x, w = sr.st.case_data(rows, length, seed)
    xs = sr.times(x, e)
    d_w = torch.from_numpy(w.copy()).to("cuda:0")
    g_re, g_im = tf.stft(torch.from_numpy(xs.copy()).to("cuda:0"), d_w, hop, center=True)
    back = tf.istft(g_re, g_im, d_w, hop, length, center=True).cpu().numpy()
    return float(ir.rel_l2(back, xs).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stft_range.txt"))
    ap.add_argument("--model-only", action="store_true")
    args = ap.parse_args()

    import istft_ref as ir
    import stft_range_ref as sr

    gpu = torch = tf = None
    if not args.model_only:
        import __graft_entry__ as g

        g.build()
        import tensor_fft_amd as tf
        import test_gpu_stft_range as tr
        import torch

        tf.device_check(0)
        gpu = (tr, tf)

    def fmt(v):
        return "not measured" if v is None else (f"{v:.2e}" if isinstance(v, float) else str(v))

    lines = ["# tools/stft_range_accuracy.py: the STFT family at the edges of its range contract (tests/stft_range_ref.py); seeds " + str(args.seeds),
             "# data set : binding quantity at its share of the limit (first seed) : worst rel-L2 against fp64, model (seed) | GPU (seed) : halves that",
             "# differ from the shipped-plan yardsticks over all seeds (0 = bit for bit). Forward: per frame against rfft / n of the binary16 products,",
             f"# asserted for the upper-edge sets: {sr.K_RFFT:.1e}. Inverse: per signal against the fp64 ISTFT of the same spectra. Lower-edge sets are held",
             "# by the bits; their rel-L2 is listed for the record only."]
    sets = [("forward", c, n) for c, n in sr.forward_params()] + [("forward", "corner-self-outside", n) for n in sr.LENGTHS]
    sets += [("inverse", c, ir.N) for c in sr.UPPER_INVERSE + sr.WINDOW_INVERSE + sr.LOWER_INVERSE]
    for kind, corner, n in sets:
        worst_m, worst_g, differ, text = (0.0, 0), (None, 0), None, ""
        for seed in args.seeds:
            d = sr.forward(corner, n, seed) if kind == "forward" else sr.inverse(corner, seed)
            if seed == args.seeds[0]:
                name, ratio = sr.binding(d)
                text = f"{name} {ratio:.3f}" + (" (outside the contract)" if d["outside"] else "")
            m, g_err, g_diff = forward_row(sr, d, gpu) if kind == "forward" else inverse_row(sr, ir, d, gpu)
            if m >= worst_m[0] or not np.isfinite(m):
                worst_m = (m, seed)
            if g_err is not None and (worst_g[0] is None or g_err >= worst_g[0] or not np.isfinite(g_err)):
                worst_g = (g_err, seed)
            if g_diff is not None:
                differ = (differ or 0) + g_diff
        lines.append(f"{kind} {corner} n={n} : {text} : {fmt(worst_m[0])} ({worst_m[1]}) | {fmt(worst_g[0])}" + (f" ({worst_g[1]})" if worst_g[0] is not None else "")
                     + f" : {fmt(differ)}")
        print(lines[-1], flush=True)
    rows, length, hop, pad = sr.ROUND_TRIP_SHAPE
    lines.append(f"# round trip istft(stft(x 2^e)) against x 2^e, ({rows}, {length}, {hop}, {pad}) Hann, worst signal's rel-L2 over the seeds: model | GPU; whether both")
    lines.append("# contracts hold (model, first seed); max |Z'| of the ISTFT input at its share of 64512")
    for e in sr.ROUND_TRIP_EXPONENTS:
        m = max(sr.round_trip(e, seed)["error"] for seed in args.seeds)
        r = sr.round_trip(e, args.seeds[0])
        g_err = None if gpu is None else max(gpu_round_trip(sr, ir, tf, torch, e, seed) for seed in args.seeds)
        lines.append(f"round trip e={e:+d} : {fmt(m)} | {fmt(g_err)} : holds {r['holds']} : input {sr.binding(r['inverse'], ('input',))[1]:.3f}")
        print(lines[-1], flush=True)
    if gpu is not None:
        tf.stft_cache_clear()
        tf.istft_cache_clear()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
