#!/usr/bin/env python3
"""FFT convolution at N = 4096 against the complex headline, in one process and alternated (include/tfft_conv.h).

    python tools/bench_conv.py [--steps K] [--warmup W] [--rounds R] [--json FILE]

Cases, each on resident data born on the device with the library's hash generator (tfft_synth_uniform, seed 42), 65536 signals:
  complex            the bench.py headline: one tfft_exec (1 GiB in + 1 GiB out)
  conv_composed_F    forward plan -> cmul -> inverse plan (TFFT_CONV_COMPOSED) with F = 1 and 64 filters: three trips through HBM
  conv_fused_F       the one-pass kernel with F = 1 and 64 filters: the bytes of ONE transform
Every output is checked against numpy (float64) on sampled signals before anything is timed. Timing: bench.py's protocol, i.e. RAMP untimed launches, W warm-up steps, then K back-to-back launches between two HIP
events on the launch stream; the cases run in turn, R rounds, and the median round is reported with its range. Bytes are
algorithmic (input + output of the pipeline, not the workspace traffic) against 8 TB/s."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

N = 4096
BATCH = 65536
FILTERS = (1, 64)
SEED = 42
RAMP = 100
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--json", default="")
    args = ap.parse_args()

    import torch

    import __graft_entry__ as g

    g.build()
    import conv_ref
    import tensor_fft_amd as tf

    batch = args.batch
    dev = torch.device("cuda:0")
    x = torch.empty(batch * 2 * N, dtype=torch.float16, device=dev)
    tf.synth_uniform(x, x[N:], N, batch, 2 * N, 0, SEED)
    y = torch.empty_like(x)
    cplan = tf.TfftPlan(N, batch, 0)
    rng = np.random.default_rng(SEED)
    cases = {"complex": lambda: cplan.exec(x, x[N:], y, y[N:])}
    outs, filt, plans = {}, {}, {}
    for nf in FILTERS:
        h_re, h_im = conv_ref.to_half_planes(conv_ref.make_filters("decay", N, nf, rng))
        filt[nf] = (h_re, h_im)
        d_re, d_im = torch.from_numpy(h_re.reshape(-1)).to(dev), torch.from_numpy(h_im.reshape(-1)).to(dev)
        for name, composed in (("conv_composed", True), ("conv_fused", False)):
            plan = tf.TfftConvPlan(N, batch, nf, 0, composed=composed)
            plan.set_filter(d_re, d_im)
            plan.prepare()
            out = torch.empty_like(x)
            key = f"{name}_{nf}"
            plans[key], outs[key] = plan, out
            cases[key] = (lambda p=plan, o=out: p.exec(x, x[N:], o, o[N:]))

    # ---- checks before timing
    for fn in cases.values():
        fn()
    torch.cuda.synchronize()
    rows = np.sort(np.random.default_rng(1).choice(batch, min(64, batch), replace=False))
    xs = x.view(batch, 2 * N)[rows].cpu().numpy()
    check = {}
    for nf in FILTERS:
        h_re, h_im = filt[nf]
        want_re, want_im = conv_ref.reference(xs[:, :N], xs[:, N:], h_re, h_im, index=rows % nf)
        want = want_re + 1j * want_im
        for name in ("conv_composed", "conv_fused"):
            o = outs[f"{name}_{nf}"].view(batch, 2 * N)[rows].cpu().numpy().astype(np.float64)
            got = o[:, :N] + 1j * o[:, N:]
            rel = float(np.sqrt((np.abs(got - want) ** 2).sum(-1) / (np.abs(want) ** 2).sum(-1)).max())
            assert rel < 1.5e-3, f"{name}_{nf} rel-L2 {rel:.3e}"
            check[f"{name}_{nf}_rel_l2"] = rel

    # ---- timing, alternated
    def timed(fn):
        for _ in range(args.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps * 1e3       # us per call

    for _ in range(RAMP):
        cases["complex"]()
    times = {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, fn in cases.items():
            times[k].append(timed(fn))
    io_bytes = batch * N * 4 * 2
    out = {"n": N, "signals": batch, "filters": list(FILTERS), "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "check": check,
           "launches": {k: p.num_launches for k, p in plans.items()}, "cases": {}}
    for k, ts in times.items():
        us = statistics.median(ts)
        out["cases"][k] = {"us_per_call": round(us, 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
                           "gsamples_s": round(batch * N / us / 1e3, 1), "gbytes_s": round(io_bytes / us / 1e3, 1),
                           "hbm_fraction": round(io_bytes / us / 1e3 / HBM_PEAK_GBS, 3)}
    c = out["cases"]
    for nf in FILTERS:
        out[f"fused_over_complex_{nf}"] = round(c[f"conv_fused_{nf}"]["us_per_call"] / c["complex"]["us_per_call"], 3)
        out[f"composed_over_fused_{nf}"] = round(c[f"conv_composed_{nf}"]["us_per_call"] / c[f"conv_fused_{nf}"]["us_per_call"], 3)
        # the gate of the fused default: faster than the composed path with the two ranges (min .. max over the rounds) apart
        out[f"fused_range_below_composed_{nf}"] = bool(c[f"conv_fused_{nf}"]["max_us"] < c[f"conv_composed_{nf}"]["min_us"])
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
