#!/usr/bin/env python3
"""The gradient plans of the overlap-save causal convolution against the forward plan and against what a caller who needs
loss.backward() does without them, in one process and alternated (include/tfft_bconv.h).

    python tools/bconv_bench.py [--steps K] [--warmup W] [--rounds R] [--rows B] [--json FILE]

B x C = 256 x 64 real sequences of L = 16384 (2^28 samples), resident on the device, K = 2049 and K = 128 taps:
  dgrad_k*       (a) TfftLongConvGradPlan.input_grad
  wgrad_k*       (b) TfftLongConvGradPlan.tap_grad, workspace prepared (wgrad_kernel + wreduce_kernel)
  sconv_k*       (c) the forward TfftLongConvPlan, the floor: the same items and transforms as (a)
  torch_fwd_k*, torch_bwd_k*
                 (d) torch.fft.rfft / irfft at 2 L in fp32 with autograd, forward and backward timed separately. It needs about
                 ten times the memory of the plans, so it runs on --torch-rows rows (default 32) and its time is scaled to B rows
                 (the FFTs are batched over rows; the scaling favours torch, whose small-batch efficiency is no worse)
Before anything is timed, (a) and (b) are checked against fp64 on a few sequences / against (d)'s gradient.
Timing: the protocol of tools/sconv_bench.py, i.e. RAMP untimed launches, W warm-up steps, then K back-to-back executions between
two HIP events on the launch stream; the cases run in turn, R rounds, and the median round is reported with its range.
The two kernels of (b) cannot be told apart between two events; the share of wreduce_kernel comes from a kernel trace
(rocprofv3 --kernel-trace --stats on this script with --steps 20 --rounds 1; profiles/README.md). Its traffic, C * P * Kpad * 4
bytes read once, is reported as wreduce_bytes."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--torch-rows", type=int, default=32)
    ap.add_argument("--torch-steps", type=int, default=10)
    ap.add_argument("--json", default="")
    args = ap.parse_args()

    import torch

    import __graft_entry__ as g

    g.build()
    import lconv_ref as lr
    import tensor_fft_amd as tf

    dev = torch.device("cuda:0")
    rows, channels = args.rows, CHANNELS
    assert rows % 2 == 0 and rows % args.torch_rows == 0
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)
    x = (torch.rand((rows, channels, L), generator=gen, device=dev) * 2 - 1).to(torch.float16)
    gr = (torch.rand((rows, channels, L), generator=gen, device=dev) * 2 - 1).to(torch.float16)
    rng = np.random.default_rng(SEED)
    taps = {K_LONG: torch.from_numpy(lr.make_taps("decay", channels, K_LONG, rng)).to(dev),
            K_SHORT: torch.from_numpy(lr.make_taps("decay", channels, K_SHORT, rng)).to(dev)}

    y = torch.empty_like(x)
    xf, gf, yf = x.view(-1), gr.view(-1), y.view(-1)
    cases, plans, dh, geo = {}, [], {}, {}
    tr = args.torch_rows

    def torch_conv(xs, h):
        n = 2 * L
        return torch.fft.irfft(torch.fft.rfft(xs.float(), n) * torch.fft.rfft(h.float(), n)[None], n)[..., :L]

    for k, name in ((K_LONG, "k2049"), (K_SHORT, "k128")):
        b = tf.TfftLongConvGradPlan(rows, channels, L, k, 0)
        b.set_taps(taps[k].view(-1))
        b.prepare()
        f = tf.TfftLongConvPlan(rows, channels, L, k, 0)
        f.set_taps(taps[k].view(-1))
        plans += [b, f]
        geo[name] = {"halo": b.halo, "hop": b.hop, "segments": b.segments, "partials": b.partials, "workspace_bytes": b.workspace_bytes}
        dh[name] = torch.empty((channels, k), dtype=torch.float32, device=dev)
        cases["dgrad_" + name] = (lambda b=b: b.input_grad(gf, yf))
        cases["wgrad_" + name] = (lambda b=b, d=dh[name]: b.tap_grad(xf, gf, d))
        cases["sconv_" + name] = (lambda f=f: f.exec(xf, yf))

    # ---- checks before timing, on the first torch_rows rows: against torch's fp32 autograd (d) and, for dx, fp64 on two pairs
    check = {}
    for k, name in ((K_LONG, "k2049"), (K_SHORT, "k128")):
        xs = x[:tr].detach().clone().requires_grad_()
        hs = taps[k].detach().clone().float().requires_grad_()
        torch_conv(xs, hs).backward(gr[:tr].float())
        small = tf.TfftLongConvGradPlan(tr, channels, L, k, 0)
        small.set_taps(taps[k].view(-1))
        dxs = torch.empty((tr, channels, L), dtype=torch.float16, device=dev)
        dhs = torch.empty((channels, k), dtype=torch.float32, device=dev)
        small.input_grad(gr[:tr].contiguous().view(-1), dxs.view(-1))
        small.tap_grad(x[:tr].contiguous().view(-1), gr[:tr].contiguous().view(-1), dhs)
        torch.cuda.synchronize()
        rel_dx = float(((dxs.float() - xs.grad.float()).norm() / xs.grad.float().norm()).item())
        rel_dh = float(((dhs - hs.grad).norm() / hs.grad.norm()).item())
        small.close()
        check[name] = {"dx_rel_l2_vs_torch_fp32": rel_dx, "dh_rel_l2_vs_torch_fp32": rel_dh}
        assert rel_dx < 3e-3 and rel_dh < 3e-3, (name, rel_dx, rel_dh)
        del xs, hs, dxs, dhs
    torch.cuda.empty_cache()

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3       # us per call

    def torch_times(k):
        """(forward us, backward us) of (d) on torch_rows rows, scaled to `rows`"""
        xs = x[:tr].detach().clone().requires_grad_()
        hs = taps[k].detach().clone().float().requires_grad_()
        gs = gr[:tr].float()
        fw, bw = [], []
        for i in range(2 + args.torch_steps):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            xs.grad = hs.grad = None
            e0.record()
            out = torch_conv(xs, hs)
            e1.record()
            out.backward(gs)
            e2.record()
            torch.cuda.synchronize()
            if i >= 2:
                fw.append(e0.elapsed_time(e1) * 1e3)
                bw.append(e1.elapsed_time(e2) * 1e3)
        scale = rows / tr
        return statistics.median(fw) * scale, statistics.median(bw) * scale

    for _ in range(RAMP):
        cases["sconv_k2049"]()
    times = {k: [] for k in cases}
    for k in ("torch_fwd_k2049", "torch_bwd_k2049", "torch_fwd_k128", "torch_bwd_k128"):
        times[k] = []
    for _ in range(args.rounds):
        for k, fn in cases.items():
            times[k].append(timed(fn, args.steps, args.warmup))
        for k, name in ((K_LONG, "k2049"), (K_SHORT, "k128")):
            fw, bw = torch_times(k)
            times["torch_fwd_" + name].append(fw)
            times["torch_bwd_" + name].append(bw)

    out = {"length": L, "rows": rows, "channels": channels, "samples": rows * channels * L, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "torch_rows": tr, "torch_steps": args.torch_steps, "geometry": geo, "check": check, "cases": {}}
    for k, ts in times.items():
        us = statistics.median(ts)
        out["cases"][k] = {"us_per_call": round(us, 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1)}
    c = out["cases"]
    for name in ("k2049", "k128"):
        a, b, f, d = c["dgrad_" + name], c["wgrad_" + name], c["sconv_" + name], c["torch_bwd_" + name]
        out["dgrad_over_sconv_" + name] = round(a["us_per_call"] / f["us_per_call"], 3)
        out["wgrad_over_sconv_" + name] = round(b["us_per_call"] / f["us_per_call"], 3)
        out["torch_bwd_over_dgrad_plus_wgrad_" + name] = round(d["us_per_call"] / (a["us_per_call"] + b["us_per_call"]), 2)
        out["ranges_apart_" + name] = {"dgrad_vs_sconv": bool(a["min_us"] > f["max_us"] or a["max_us"] < f["min_us"]),
                                       "wgrad_vs_sconv": bool(b["min_us"] > f["max_us"] or b["max_us"] < f["min_us"]),
                                       "torch_bwd_vs_dgrad_plus_wgrad": bool(d["min_us"] > a["max_us"] + b["max_us"])}
        out["wreduce_bytes_" + name] = geo[name]["workspace_bytes"]
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    for p in plans:
        p.close()


if __name__ == "__main__":
    main()
