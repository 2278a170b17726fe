#!/usr/bin/env python3
"""The fused gated causal convolution against what a caller does today, in one process and alternated (include/tfft_gconv.h).

    python tools/gconv_bench.py [--steps K] [--warmup W] [--rounds R] [--seqs S] [--json FILE]

B x C = 131072 real sequences of L = 2048 with K = 2049 taps (C = 64 channels), both gates and a skip weight, resident on the device:
  gconv_fused      (a) the gated fused plan: y = g * (h * (p x) + d (p x)) in one kernel; x, p, g in and y out, 16 L bytes per pair
  lconv_and_torch  (b) what a caller does today: u = p * x, TfftCausalConvPlan, y = g * (z + d[:, None] * u), the elementwise
                       steps in torch
  lconv_fused      (c) the ungated TfftCausalConvPlan alone, as the floor: 8 L bytes per pair
Before anything is timed, (a) must equal, bit for bit as binary16 values, g * crop(TfftConvPlan(pad(p * x))) with the gated plan's
own skip-carrying spectrum as the filter: the yardstick of tests/test_gpu_gconv.py, the products formed in torch (a binary16 product
in torch is the correctly rounded one). (b) rounds d * u and the sum separately, so it is compared in rel-L2 only. Timing: the
protocol of tools/lconv_bench.py, i.e. RAMP untimed launches, W warm-up steps, then K back-to-back executions between two HIP
events on the launch stream; the cases run in turn, R rounds, and the median round is reported with its range. Bytes are
algorithmic, per pair of sequences, against 8 TB/s. The one condition evaluated: (a) is not slower than (b) beyond (b)'s own spread
over the rounds."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

L, K, N = 2048, 2049, 4096
SEQS, CHANNELS = 131072, 64
SEED = 42
RAMP = 100
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seqs", type=int, default=SEQS)
    ap.add_argument("--json", default="")
    args = ap.parse_args()

    import torch

    import __graft_entry__ as g

    g.build()
    import gconv_ref as gr
    import lconv_ref as lr
    import tensor_fft_amd as tf

    dev = torch.device("cuda:0")
    channels = CHANNELS
    rows = args.seqs // channels
    assert rows % 2 == 0 and rows * channels == args.seqs
    items = rows // 2 * channels
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)

    def uniform():
        return (torch.rand((rows, channels, L), generator=gen, device=dev) * 2 - 1).to(torch.float16)

    x, p, gate = uniform(), uniform(), uniform()
    h = torch.from_numpy(lr.make_taps("decay", channels, K, np.random.default_rng(SEED))).to(dev)
    d = torch.from_numpy(gr.skip_values(channels)).to(dev)

    gplan = tf.TfftGatedConvPlan(rows, channels, L, K, 0, pre_gate=True, post_gate=True)
    gplan.set_taps(h.view(-1), d)
    assert gplan.kernels == ["gconv4096::gconv4096_kernel<true, true>"]
    lplan = tf.TfftCausalConvPlan(rows, channels, L, K, 0)
    lplan.set_taps(h.view(-1))
    assert lplan.kernels == ["lconv4096::lconv4096_kernel"]

    y_a, y_c = torch.empty_like(x), torch.empty_like(x)
    z = torch.empty_like(x)
    d_col = d[None, :, None]

    def fused():
        gplan.exec(x.view(-1), y_a.view(-1), pre=p.view(-1), post=gate.view(-1))

    def today():
        u = p * x
        lplan.exec(u.view(-1), z.view(-1))
        return gate * (z + d_col * u)

    def floor():
        lplan.exec(x.view(-1), y_c.view(-1))

    cases = {"gconv_fused": fused, "lconv_and_torch": today, "lconv_fused": floor}

    # ---- checks before timing
    fused()
    y_b = today()
    torch.cuda.synchronize()
    h_re, h_im = gplan.spectrum()
    cplan = tf.TfftConvPlan(N, items, channels, 0)
    cplan.set_filter(h_re.view(-1), h_im.view(-1))
    padded = torch.zeros((rows // 2, channels, 2, N), dtype=torch.float16, device=dev)     # item p * C + c: [RE n | IM n]
    padded[:, :, :, :L].copy_((p * x).view(rows // 2, 2, channels, L).permute(0, 2, 1, 3))
    out = torch.empty_like(padded)
    cplan.exec(padded.view(-1), padded.view(-1)[N:], out.view(-1), out.view(-1)[N:])
    want = torch.empty_like(x)
    want.view(rows // 2, 2, channels, L).copy_(out[:, :, :, :L].permute(0, 2, 1, 3))
    want = gate * want
    torch.cuda.synchronize()
    assert not torch.isnan(y_a).any() and bool((y_a.float() == want.float()).all()), "the gated plan differs from g * crop(conv(pad(p * x)))"
    cplan.close()
    del padded, out, want
    rel_b = float((y_a.float() - y_b.float()).norm() / y_b.float().norm())
    assert rel_b < 3e-3, f"(a) against (b): rel-L2 {rel_b:.3e}"
    pick = [0, 1, rows - 2, rows - 1]                                     # two whole pairs, against fp64
    u = gr.half_product(p[pick].cpu().numpy(), x[pick].cpu().numpy())
    true = gr.reference_true(u, h.cpu().numpy(), d.cpu().numpy(), N)
    ref = gate[pick].cpu().numpy().astype(np.float64) * lr.unpair(true.real, true.imag, len(pick), channels, L)
    got = y_a[pick].cpu().numpy().astype(np.float64)
    rel = float(np.sqrt(((got - ref) ** 2).sum(-1) / (ref ** 2).sum(-1)).max())
    assert rel < 3e-3, f"rel-L2 against the fp64 result {rel:.3e}"
    del y_b

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
        floor()
    times = {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, fn in cases.items():
            times[k].append(timed(fn))
    # algorithmic HBM bytes per pair: (a) x, p, g in and y out; (c) x in and y out; (b) = (c) plus u = p * x (3 sequences) and
    # y = g * (z + d u) as torch evaluates it (d * u: 2, z + .: 3, g * .: 3), all per sequence of 2 L bytes, two sequences per pair
    per_pair = {"gconv_fused": 16 * L, "lconv_fused": 8 * L, "lconv_and_torch": 8 * L + 4 * L * (3 + 2 + 3 + 3)}
    out = {"length": L, "taps": K, "n": N, "sequences": rows * channels, "channels": channels, "pairs": items, "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds,
           "check": {"gconv_equals_gate_conv_plan_gate": True, "rel_l2_vs_lconv_and_torch": rel_b, "rel_l2_vs_fp64": rel},
           "algorithmic_bytes_per_pair": per_pair, "cases": {}}
    for k, ts in times.items():
        us = statistics.median(ts)
        out["cases"][k] = {"us_per_call": round(us, 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
                           "gsamples_s": round(rows * channels * L / us / 1e3, 1), "gbytes_s": round(items * per_pair[k] / us / 1e3, 1),
                           "hbm_fraction": round(items * per_pair[k] / us / 1e3 / HBM_PEAK_GBS, 3)}
    c = out["cases"]
    out["gconv_over_today"] = round(c["gconv_fused"]["us_per_call"] / c["lconv_and_torch"]["us_per_call"], 3)
    out["gconv_over_lconv"] = round(c["gconv_fused"]["us_per_call"] / c["lconv_fused"]["us_per_call"], 3)
    # (a) against (b) of the same run, with (b)'s own spread over the rounds as the yardstick
    out["today_spread_us"] = round(c["lconv_and_torch"]["max_us"] - c["lconv_and_torch"]["min_us"], 1)
    out["gconv_slower_than_today_beyond_its_spread"] = bool(
        c["gconv_fused"]["us_per_call"] > c["lconv_and_torch"]["us_per_call"] + out["today_spread_us"])
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
