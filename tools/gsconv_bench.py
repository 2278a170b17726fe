#!/usr/bin/env python3
"""The gated overlap-save causal convolution plan against what a caller had for gates at long sequence lengths before it, in one
process and alternated (include/tfft_gsconv.h).

    python tools/gsconv_bench.py [--steps K] [--warmup W] [--rounds R] [--rows B] [--json FILE]

B x C = 256 x 64 real sequences of L = 16384 (2^28 samples), both gates and a skip, resident on the device, at K = 2049 taps (halo
2048, hop 2048: x and p are read twice) and at K = 128 taps (halo 128, hop 3968: read 1.03 times):
  gsconv     (a) the new plan, TfftGatedLongConvPlan: one kernel, gsconv4096_kernel<true, true>
  torch_sconv (b) what a caller writes today: u = p * x in torch, TfftLongConvPlan on u, y = g * (z + d u) in torch
  sconv      (c) the ungated TfftLongConvPlan on x, no skip: the floor (another operator: only its time is of interest)
  gconv_composed (d) the shipped TfftGatedConvPlan on the same shape: pack:pre | n = 32768 sub-plan | crop:post, workspace prepared
Before anything is timed, (a), (b) and (d) are checked against g (.) (h * u + d u) in fp64 on a few sequences (u = p (.) x rounded to
binary16, as all three round it).
Timing: the protocol of tools/sconv_bench.py, i.e. RAMP untimed launches, W warm-up steps, then K back-to-back executions between
two HIP events on the launch stream; the cases run in turn, R rounds, and the median round is reported with its range. Bytes are
algorithmic, per pair of sequences with r = (hop + halo) / hop: (a) 8 L r in (x and p), 4 L in (g), 4 L out; (b) 12 L for p * x,
4 L r + 4 L for the plan, at least 20 L for g * (z + d u) as torch evaluates it (d u: 4 L + 4 L, z + .: 8 L + 4 L, g * .: 8 L + 4 L
makes 32 L; 20 L is one fused pass); (c) 4 L r + 4 L; (d) pack 8 L + 4 n, the sub-plan at least 16 n, crop 4 n + 8 L; against 8 TB/s."""
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
    import gconv_ref as gr
    import lconv_ref as lr
    import tensor_fft_amd as tf

    dev = torch.device("cuda:0")
    rows, channels = args.rows, CHANNELS
    assert rows % 2 == 0
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)

    def uniform():
        return (torch.rand((rows, channels, L), generator=gen, device=dev) * 2 - 1).to(torch.float16)

    x, pre, post = uniform(), uniform(), uniform()
    rng = np.random.default_rng(SEED)
    taps = {"k2049": torch.from_numpy(lr.make_taps("decay", channels, K_LONG, rng)).to(dev),
            "k128": torch.from_numpy(lr.make_taps("decay", channels, K_SHORT, rng)).to(dev)}
    skip = torch.from_numpy(gr.skip_values(channels)).to(dev)
    skip_b = skip.view(1, channels, 1)
    xf, pf, gf = x.view(-1), pre.view(-1), post.view(-1)

    plans, cases, outs, geometry = {}, {}, {}, {}
    for tag, h in taps.items():
        k = h.shape[1]
        a = tf.TfftGatedLongConvPlan(rows, channels, L, k, 0, pre_gate=True, post_gate=True)
        a.set_taps(h.view(-1), skip)
        assert a.kernels == ["gsconv4096::gsconv4096_kernel<true, true>"]
        c = tf.TfftLongConvPlan(rows, channels, L, k, 0)
        c.set_taps(h.view(-1))
        d = tf.TfftGatedConvPlan(rows, channels, L, k, 0, pre_gate=True, post_gate=True)
        d.set_taps(h.view(-1), skip)
        d.prepare()
        assert d.kernels[0] == "gate_copy::pack_kernel<true>" and d.kernels[-1] == "gate_copy::crop_kernel<true>"
        plans[tag] = (a, c, d)
        geometry[tag] = [a.halo, a.hop, a.segments]
        for name in ("gsconv", "torch_sconv", "sconv", "gconv_composed"):
            outs[f"{name}_{tag}"] = torch.empty_like(x)
        z = torch.empty_like(x)

        def run_a(a=a, y=outs[f"gsconv_{tag}"]):
            a.exec(xf, y.view(-1), pre=pf, post=gf)

        def run_b(c=c, z=z, tag=tag):
            u = pre * x
            c.exec(u.view(-1), z.view(-1))
            outs[f"torch_sconv_{tag}"] = post * (z + skip_b * u)

        def run_c(c=c, y=outs[f"sconv_{tag}"]):
            c.exec(xf, y.view(-1))

        def run_d(d=d, y=outs[f"gconv_composed_{tag}"]):
            d.exec(xf, y.view(-1), pre=pf, post=gf)

        cases[f"gsconv_{tag}"], cases[f"torch_sconv_{tag}"], cases[f"sconv_{tag}"], cases[f"gconv_composed_{tag}"] = run_a, run_b, run_c, run_d

    # ---- checks before timing: against g (.) (h * u + d u) in fp64 on two whole pairs
    for fn in cases.values():
        fn()
    torch.cuda.synchronize()
    pick = [0, 1, rows - 2, rows - 1]
    rel = {}
    u64 = gr.half_product(pre[pick].cpu().numpy(), x[pick].cpu().numpy()).astype(np.float64)
    g64 = post[pick].cpu().numpy().astype(np.float64)
    d64 = skip.cpu().numpy().astype(np.float64)[None, :, None]
    n_ref = 1 << 16
    for tag, h in taps.items():
        hh = h.cpu().numpy().astype(np.float64)
        want = g64 * (np.fft.irfft(np.fft.rfft(u64, n_ref, axis=-1) * np.fft.rfft(hh, n_ref, axis=-1)[None], n_ref, axis=-1)[..., :L] + d64 * u64)
        for name in ("gsconv", "torch_sconv", "gconv_composed"):
            got = outs[f"{name}_{tag}"][pick].cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all(), (name, tag)
            rel[f"{name}_{tag}"] = float(np.sqrt(((got - want) ** 2).sum(-1) / (want ** 2).sum(-1)).max())
            assert rel[f"{name}_{tag}"] < 3e-3, f"{name}_{tag}: rel-L2 against the fp64 result {rel[f'{name}_{tag}']:.3e}"

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
        cases["sconv_k2049"]()
    times = {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, fn in cases.items():
            times[k].append(timed(fn))
    pairs = rows // 2 * channels
    out = {"length": L, "rows": rows, "channels": channels, "samples": rows * channels * L, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "geometry": geometry, "gconv_composed_n": plans["k2049"][2].n, "gconv_composed_kernels": plans["k2049"][2].kernels,
           "check": {"rel_l2_vs_fp64": rel}, "cases": {}}
    for tag in taps:
        halo, hop, _ = geometry[tag]
        amp = (hop + halo) / hop
        n = plans[tag][2].n
        io = {"gsconv": pairs * (8 * L * amp + 8 * L), "torch_sconv": pairs * (12 * L + 4 * L * amp + 4 * L + 20 * L), "sconv": pairs * (4 * L * amp + 4 * L),
              "gconv_composed": pairs * (16 * L + 8 * n + 16 * n)}
        for name, nbytes in io.items():
            ts = times[f"{name}_{tag}"]
            us = statistics.median(ts)
            out["cases"][f"{name}_{tag}"] = {"us_per_call": round(us, 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
                                             "gsamples_s": round(rows * channels * L / us / 1e3, 1), "algorithmic_gbytes_s": round(nbytes / us / 1e3, 1),
                                             "hbm_fraction": round(nbytes / us / 1e3 / HBM_PEAK_GBS, 3)}
    c = out["cases"]
    for tag in taps:
        a = c[f"gsconv_{tag}"]
        for other in ("torch_sconv", "sconv", "gconv_composed"):
            o = c[f"{other}_{tag}"]
            # the ratio of the medians, and the range the rounds allow it: fastest over slowest, slowest over fastest
            out[f"gsconv_over_{other}_{tag}"] = {"median": round(a["us_per_call"] / o["us_per_call"], 3), "min": round(a["min_us"] / o["max_us"], 3),
                                                 "max": round(a["max_us"] / o["min_us"], 3)}
    # the condition for calling the fusion a win: (a) below (b) with the ranges apart, at both K
    out["gsconv_faster_than_torch_sconv_ranges_apart"] = bool(all(c[f"gsconv_{t}"]["max_us"] < c[f"torch_sconv_{t}"]["min_us"] for t in taps))
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
