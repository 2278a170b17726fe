#!/usr/bin/env python3
"""The fused causal convolution against what a caller does today, in one process and alternated (include/tfft_lconv.h).

    python tools/lconv_bench.py [--steps K] [--warmup W] [--rounds R] [--seqs S] [--json FILE]

B x C = 131072 real sequences of L = 2048 with K = 2049 taps (C = 64 channels), resident on the device:
  lconv_fused       (a) the fused causal plan: 2 L halves in and 2 L halves out per pair, the padding written into LDS
  conv_fused_padded (b) the shipped fused TfftConvPlan on planes padded beforehand: the same arithmetic on 4 L halves each way
  pad_conv_slice    (c) what a caller does today: a torch pad into those planes, then (b), then a slice into a contiguous result
Every output is checked against (b)'s, which tests/test_gpu_conv.py validates, before anything is timed: (a) and (c) must equal it
bit for bit on the kept samples. Timing: the protocol of tools/bench_conv.py, i.e. RAMP untimed launches, W warm-up steps, then K
back-to-back executions between two HIP events on the launch stream; the cases run in turn, R rounds, and the median round is
reported with its range. Bytes are algorithmic, per pair of sequences: (a) 8 L, (b) 8 n = 16 L, (c) (b) plus 8 L for the pad and
8 L for the slice, against 8 TB/s."""
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
    import lconv_ref as lr
    import tensor_fft_amd as tf

    dev = torch.device("cuda:0")
    channels = CHANNELS
    rows = args.seqs // channels
    assert rows % 2 == 0 and rows * channels == args.seqs
    items = rows // 2 * channels
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)
    x = (torch.rand((rows, channels, L), generator=gen, device=dev) * 2 - 1).to(torch.float16)
    h = torch.from_numpy(lr.make_taps("decay", channels, K, np.random.default_rng(SEED))).to(dev)

    lplan = tf.TfftCausalConvPlan(rows, channels, L, K, 0)
    lplan.set_taps(h.view(-1))
    assert lplan.kernels == ["lconv4096::lconv4096_kernel"]
    h_re, h_im = lplan.spectrum()
    cplan = tf.TfftConvPlan(N, items, channels, 0)
    cplan.set_filter(h_re.view(-1), h_im.view(-1))
    assert cplan.kernels == ["conv4096::conv4096_kernel"]

    y_a = torch.empty_like(x)
    padded = torch.zeros((rows // 2, channels, 2, N), dtype=torch.float16, device=dev)     # item p * C + c: [RE n | IM n]
    out_b = torch.empty_like(padded)
    y_c = torch.empty_like(x)
    xv = x.view(rows // 2, 2, channels, L)

    def pad():
        # rows 2p and 2p + 1 of a channel into the RE and IM plane of item (p, c); the padding halves stay zero
        padded[:, :, :, :L].copy_(xv.permute(0, 2, 1, 3))

    def conv():
        pf, of = padded.view(-1), out_b.view(-1)
        cplan.exec(pf, pf[N:], of, of[N:])

    def crop():
        y_c.view(rows // 2, 2, channels, L).copy_(out_b[:, :, :, :L].permute(0, 2, 1, 3))

    def today():
        pad()
        conv()
        crop()

    cases = {"lconv_fused": lambda: lplan.exec(x.view(-1), y_a.view(-1)), "conv_fused_padded": conv, "pad_conv_slice": today}

    # ---- checks before timing: the three results agree bit for bit (as values) on the kept samples
    today()
    cases["lconv_fused"]()
    torch.cuda.synchronize()
    assert not torch.isnan(y_a).any() and bool((y_a.float() == y_c.float()).all()), "the fused causal plan differs from pad -> conv -> slice"
    pick = [0, 1, rows - 2, rows - 1]                                     # two whole pairs
    true = lr.reference_taps(x[pick].cpu().numpy(), h.cpu().numpy(), N)
    want = lr.unpair(true.real, true.imag, len(pick), channels, L)
    got = y_a[pick].cpu().numpy().astype(np.float64)
    rel = float(np.sqrt(((got - want) ** 2).sum(-1) / (want ** 2).sum(-1)).max())
    assert rel < 3e-3, f"rel-L2 against the true linear convolution {rel:.3e}"

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
        cases["conv_fused_padded"]()
    times = {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, fn in cases.items():
            times[k].append(timed(fn))
    # algorithmic HBM bytes per execution: (a) every sample once in and once out; (b) the padded planes in and out; (c) = (b) plus the
    # pad (read x, write the kept half of the planes) and the slice (read the kept half, write y)
    bytes_a = items * 8 * L
    bytes_b = items * 8 * N
    bytes_c = bytes_b + 2 * items * 8 * L
    io = {"lconv_fused": bytes_a, "conv_fused_padded": bytes_b, "pad_conv_slice": bytes_c}
    out = {"length": L, "taps": K, "n": N, "sequences": rows * channels, "channels": channels, "pairs": items, "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds, "check": {"lconv_equals_pad_conv_slice": True, "rel_l2_vs_linear_convolution": rel},
           "algorithmic_bytes_per_pair": {"lconv_fused": 8 * L, "conv_fused_padded": 8 * N, "pad_conv_slice": 8 * N + 16 * L}, "cases": {}}
    for k, ts in times.items():
        us = statistics.median(ts)
        out["cases"][k] = {"us_per_call": round(us, 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
                           "gsamples_s": round(rows * channels * L / us / 1e3, 1), "gbytes_s": round(io[k] / us / 1e3, 1),
                           "hbm_fraction": round(io[k] / us / 1e3 / HBM_PEAK_GBS, 3)}
    c = out["cases"]
    out["lconv_over_conv_padded"] = round(c["lconv_fused"]["us_per_call"] / c["conv_fused_padded"]["us_per_call"], 3)
    out["today_over_lconv"] = round(c["pad_conv_slice"]["us_per_call"] / c["lconv_fused"]["us_per_call"], 3)
    # (a) against (b) of the same run, with (b)'s own spread over the rounds as the yardstick
    out["conv_padded_spread_us"] = round(c["conv_fused_padded"]["max_us"] - c["conv_fused_padded"]["min_us"], 1)
    out["lconv_slower_than_conv_padded_beyond_its_spread"] = bool(
        c["lconv_fused"]["us_per_call"] > c["conv_fused_padded"]["us_per_call"] + out["conv_padded_spread_us"])
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
