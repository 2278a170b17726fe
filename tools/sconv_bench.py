#!/usr/bin/env python3
"""The overlap-save causal convolution plan against the only path long sequences had before it, in one process and alternated
(include/tfft_sconv.h).

    python tools/sconv_bench.py [--steps K] [--warmup W] [--rounds R] [--rows B] [--json FILE]

B x C = 256 x 64 real sequences of L = 16384 (2^28 samples), resident on the device:
  sconv_k2049   (a) the long plan with K = 2049 taps: halo 2048, hop 2048, every sample read twice and written once
  sconv_k128    (a) the long plan with K = 128 taps: halo 128, hop 3968, every sample read 1.03 times
  lconv_composed (b) the shipped TfftCausalConvPlan on the same shape, K = 2049: pack | n = 32768 sub-plan | crop, workspace prepared
  lconv_fused   (c) the fused causal plan on the same samples seen as 2048 x 64 sequences of 2048, K = 2049: the floor without read
                amplification (another convolution: only its time is of interest)
Before anything is timed, (a) at both K and (b) are checked against the true linear convolution in fp64 on a few sequences.
Timing: the protocol of tools/lconv_bench.py, i.e. RAMP untimed launches, W warm-up steps, then K back-to-back executions between
two HIP events on the launch stream; the cases run in turn, R rounds, and the median round is reported with its range. Bytes are
algorithmic, per pair of sequences: (a) 4 L (hop + halo) / hop in and 4 L out, (b) pack 4 L + 4 n, the sub-plan at least 16 n
(one fused pass; more for what it really launches), crop 4 n + 4 L, (c) 8 L; against 8 TB/s."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

L, K_LONG, K_SHORT = 16384, 2049, 128
ROWS, CHANNELS = 256, 64
L_FUSED = 2048
SEED = 42
RAMP = 20
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--json", default="")
    args = ap.parse_args()

    import torch

    import __graft_entry__ as g

    g.build()
    import lconv_ref as lr
    import sconv_ref as sr
    import tensor_fft_amd as tf

    dev = torch.device("cuda:0")
    rows, channels = args.rows, CHANNELS
    assert rows % 2 == 0
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)
    x = (torch.rand((rows, channels, L), generator=gen, device=dev) * 2 - 1).to(torch.float16)
    rng = np.random.default_rng(SEED)
    h_long = torch.from_numpy(lr.make_taps("decay", channels, K_LONG, rng)).to(dev)
    h_short = torch.from_numpy(lr.make_taps("decay", channels, K_SHORT, rng)).to(dev)

    s_long = tf.TfftLongConvPlan(rows, channels, L, K_LONG, 0)
    s_long.set_taps(h_long.view(-1))
    s_short = tf.TfftLongConvPlan(rows, channels, L, K_SHORT, 0)
    s_short.set_taps(h_short.view(-1))
    assert s_long.kernels == s_short.kernels == ["sconv4096::sconv4096_kernel"]
    composed = tf.TfftCausalConvPlan(rows, channels, L, K_LONG, 0)
    composed.set_taps(h_long.view(-1))
    composed.prepare()
    assert composed.kernels[0] == "lconv_copy::pack_kernel" and composed.kernels[-1] == "lconv_copy::crop_kernel"
    rows_f = rows * (L // L_FUSED)
    fused = tf.TfftCausalConvPlan(rows_f, channels, L_FUSED, K_LONG, 0)
    fused.set_taps(h_long.view(-1))
    assert fused.kernels == ["lconv4096::lconv4096_kernel"]

    y = {k: torch.empty_like(x) for k in ("sconv_k2049", "sconv_k128", "lconv_composed", "lconv_fused")}
    xf = x.view(-1)
    cases = {"sconv_k2049": lambda: s_long.exec(xf, y["sconv_k2049"].view(-1)), "sconv_k128": lambda: s_short.exec(xf, y["sconv_k128"].view(-1)),
             "lconv_composed": lambda: composed.exec(xf, y["lconv_composed"].view(-1)), "lconv_fused": lambda: fused.exec(xf, y["lconv_fused"].view(-1))}

    # ---- checks before timing: against the true linear convolution in fp64 on two whole pairs
    for fn in cases.values():
        fn()
    torch.cuda.synchronize()
    pick = [0, 1, rows - 2, rows - 1]
    rel = {}
    for name, h in (("sconv_k2049", h_long), ("sconv_k128", h_short), ("lconv_composed", h_long)):
        hx, hh = x[pick].cpu().numpy().astype(np.float64), h.cpu().numpy().astype(np.float64)
        n = 1 << 16
        want = np.fft.irfft(np.fft.rfft(hx, n, axis=-1) * np.fft.rfft(hh, n, axis=-1)[None], n, axis=-1)[..., :L]
        got = y[name][pick].cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), name
        rel[name] = float(np.sqrt(((got - want) ** 2).sum(-1) / (want ** 2).sum(-1)).max())
        assert rel[name] < 3e-3, f"{name}: rel-L2 against the true linear convolution {rel[name]:.3e}"

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
        cases["lconv_fused"]()
    times = {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, fn in cases.items():
            times[k].append(timed(fn))
    pairs = rows // 2 * channels
    n = composed.n

    def sconv_bytes(plan):
        return pairs * (4 * L * (plan.hop + plan.halo) // plan.hop + 4 * L)

    io = {"sconv_k2049": sconv_bytes(s_long), "sconv_k128": sconv_bytes(s_short), "lconv_composed": pairs * (8 * L + 8 * n + 16 * n), "lconv_fused": pairs * 8 * L}
    out = {"length": L, "rows": rows, "channels": channels, "samples": rows * channels * L, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "geometry": {"sconv_k2049": [s_long.halo, s_long.hop, s_long.segments], "sconv_k128": [s_short.halo, s_short.hop, s_short.segments]},
           "lconv_composed_n": n, "lconv_composed_kernels": composed.kernels, "check": {"rel_l2_vs_linear_convolution": rel}, "cases": {}}
    for k, ts in times.items():
        us = statistics.median(ts)
        out["cases"][k] = {"us_per_call": round(us, 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
                           "gsamples_s": round(rows * channels * L / us / 1e3, 1), "algorithmic_gbytes_s": round(io[k] / us / 1e3, 1),
                           "hbm_fraction": round(io[k] / us / 1e3 / HBM_PEAK_GBS, 3)}
    c = out["cases"]
    out["sconv_k2049_over_lconv_composed"] = round(c["sconv_k2049"]["us_per_call"] / c["lconv_composed"]["us_per_call"], 3)
    out["sconv_k128_over_lconv_composed"] = round(c["sconv_k128"]["us_per_call"] / c["lconv_composed"]["us_per_call"], 3)
    out["sconv_k2049_over_lconv_fused"] = round(c["sconv_k2049"]["us_per_call"] / c["lconv_fused"]["us_per_call"], 3)
    out["sconv_k128_over_lconv_fused"] = round(c["sconv_k128"]["us_per_call"] / c["lconv_fused"]["us_per_call"], 3)
    # acceptance: (a) faster than (b) with the ranges apart
    out["sconv_faster_than_lconv_composed_ranges_apart"] = bool(max(c["sconv_k2049"]["max_us"], c["sconv_k128"]["max_us"]) < c["lconv_composed"]["min_us"])
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
