#!/usr/bin/env python3
"""The gradient plans of the gated overlap-save causal convolution against what a caller had for its backward pass before them, in
one process and alternated (include/tfft_gbconv.h).

    python tools/gbconv_bench.py [--steps K] [--warmup W] [--rounds R] [--rows B] [--json FILE]

B x C = 256 x 64 real sequences of L = 16384 (2^28 samples), both gates and a skip, resident on the device, at K = 2049 taps (halo
2048, hop 2048: gy and post are read twice) and at K = 128 taps (halo 128, hop 3968: read 1.03 times):
  dgrad       (a) the fused input gradient with dpre: one kernel, gbconv4096::dgrad_kernel<true, true>
  torch_dgrad (b) what a caller writes today: gz = post * gy in torch, TfftLongConvGradPlan.input_grad, + skip * gz, pre * du and
                  x * du in torch
  bconv_dgrad (c) the ungated TfftLongConvGradPlan.input_grad on gy: the floor (another operator: only its time is of interest)
  wgrad       (d) the fused tap gradient with dskip (workspace prepared)
  torch_wgrad (e) pre * x and post * gy in torch, then TfftLongConvGradPlan.tap_grad
  bconv_wgrad (f) the ungated TfftLongConvGradPlan.tap_grad
  dpost       (g) the gradient of the post gate: the forward TfftGatedLongConvPlan with gy as its post gate
Before anything is timed every result is checked against fp64 on four rows of every channel (dx, dpre, dpost: those rows of the
timed results; dh, dskip: plans of four rows, since a tap sums over all rows), and the full-size (d) against (e) bit for bit.
Timing: the protocol of tools/gsconv_bench.py, i.e. RAMP untimed launches, W warm-up steps, then K back-to-back executions between
two HIP events on the launch stream; the cases run in turn, R rounds, and the median round is reported with its range. Bytes are
algorithmic, per sequence with r = (hop + halo) / hop: (a) 4 L r in (gy and post), 4 L in (x and pre), 4 L out; (b) 6 L for post * gy,
2 L r + 2 L for the plan, 10 L for + skip * gz as torch evaluates it (two kernels: skip * gz reads 2 L and writes 2 L, du + . reads
4 L and writes 2 L), 6 L each for the two products: 2 L r + 30 L. An estimate of 2 L r + 28 L counts 8 L for the skip step, which
one fused pass could do; the 2 L more are the product skip * gz written out and read back. (c) 2 L r + 2 L."""
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
CASES = ("dgrad", "torch_dgrad", "bconv_dgrad", "wgrad", "torch_wgrad", "bconv_wgrad", "dpost")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "gbconv_bench_line.json"))
    args = ap.parse_args()

    import torch

    import __graft_entry__ as g

    g.build()
    import gconv_ref as gr
    import lconv_ref as lr
    import tensor_fft_amd as tf

    dev = torch.device("cuda:0")
    rows, channels = args.rows, CHANNELS
    assert rows % 2 == 0 and rows >= 4
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)

    def uniform():
        return (torch.rand((rows, channels, L), generator=gen, device=dev) * 2 - 1).to(torch.float16)

    x, pre, gy, post = uniform(), uniform(), uniform(), uniform()
    rng = np.random.default_rng(SEED)
    taps = {"k2049": torch.from_numpy(lr.make_taps("decay", channels, K_LONG, rng)).to(dev),
            "k128": torch.from_numpy(lr.make_taps("decay", channels, K_SHORT, rng)).to(dev)}
    skip = torch.from_numpy(gr.skip_values(channels)).to(dev)
    skip_b = skip.view(1, channels, 1)
    xf, pf, gf, qf = x.view(-1), pre.view(-1), gy.view(-1), post.view(-1)

    plans, cases, outs, geometry = {}, {}, {}, {}
    for tag, h in taps.items():
        k = h.shape[1]
        a = tf.TfftGatedLongConvGradPlan(rows, channels, L, k, 0, pre_gate=True, post_gate=True)
        a.set_taps(h.view(-1), skip)
        a.prepare()
        assert a.kernels == ["gbconv4096::dgrad_kernel<true, true>", "gbconv4096::wgrad_kernel<true, true>", "gbconv4096::wreduce_kernel"]
        b = tf.TfftLongConvGradPlan(rows, channels, L, k, 0)
        b.set_taps(h.view(-1))
        b.prepare()
        f = tf.TfftGatedLongConvPlan(rows, channels, L, k, 0, pre_gate=True, post_gate=True)
        f.set_taps(h.view(-1), skip)
        plans[tag] = (a, b, f)
        geometry[tag] = [a.halo, a.hop, a.segments, a.partials]
        o = outs[tag] = {"dx": torch.empty_like(x), "dpre": torch.empty_like(x), "du": torch.empty_like(x), "floor": torch.empty_like(x),
                         "dpost": torch.empty_like(x)}
        for name in ("dh", "dh_torch", "dh_floor"):
            o[name] = torch.empty((channels, k), dtype=torch.float32, device=dev)
        o["dskip"] = torch.empty((channels,), dtype=torch.float32, device=dev)

        def run_a(a=a, o=o):
            a.input_grad(gf, o["dx"].view(-1), post=qf, x=xf, pre=pf, dpre=o["dpre"].view(-1))

        def run_b(b=b, o=o):
            gz = post * gy
            b.input_grad(gz.view(-1), o["du"].view(-1))
            du = o["du"] + skip_b * gz
            o["dx_torch"], o["dpre_torch"] = pre * du, x * du

        def run_c(b=b, o=o):
            b.input_grad(gf, o["floor"].view(-1))

        def run_d(a=a, o=o):
            a.tap_grad(xf, gf, o["dh"], pre=pf, post=qf, dskip=o["dskip"])

        def run_e(b=b, o=o):
            u, gz = pre * x, post * gy
            b.tap_grad(u.view(-1), gz.view(-1), o["dh_torch"])

        def run_f(b=b, o=o):
            b.tap_grad(xf, gf, o["dh_floor"])

        def run_g(f=f, o=o):
            f.exec(xf, o["dpost"].view(-1), pre=pf, post=gf)

        for name, fn in zip(CASES, (run_a, run_b, run_c, run_d, run_e, run_f, run_g)):
            cases[f"{name}_{tag}"] = fn

    # ---- checks before timing: fp64 on four rows of every channel
    for fn in cases.values():
        fn()
    torch.cuda.synchronize()
    pick = [0, 1, rows - 2, rows - 1]
    rel = {}
    host = {name: t[pick].cpu().numpy() for name, t in (("x", x), ("pre", pre), ("gy", gy), ("post", post))}
    u64 = gr.half_product(host["pre"], host["x"]).astype(np.float64)
    gz64 = gr.half_product(host["post"], host["gy"]).astype(np.float64)
    x64, p64, gy64 = (host[n].astype(np.float64) for n in ("x", "pre", "gy"))
    d64 = skip.cpu().numpy().astype(np.float64)
    n_ref = 1 << 16

    def rel_l2(got, want):
        got = got.astype(np.float64)
        assert np.isfinite(got).all()
        return float(np.sqrt(((got - want) ** 2).sum(-1) / (want ** 2).sum(-1)).max())

    for tag, h in taps.items():
        k = h.shape[1]
        hs = h.cpu().numpy().astype(np.float64)
        hs[:, 0] += d64
        spec = np.fft.rfft(hs, n_ref, axis=-1)[None]
        du = np.fft.irfft(np.fft.rfft(gz64, n_ref, axis=-1) * np.conj(spec), n_ref, axis=-1)[..., :L]
        z = np.fft.irfft(np.fft.rfft(u64, n_ref, axis=-1) * spec, n_ref, axis=-1)[..., :L]
        o = outs[tag]
        for name, got, want in (("dgrad_dx", o["dx"], p64 * du), ("dgrad_dpre", o["dpre"], x64 * du), ("torch_dgrad_dx", o["dx_torch"], p64 * du),
                                ("torch_dgrad_dpre", o["dpre_torch"], x64 * du), ("dpost", o["dpost"], gy64 * z)):
            rel[f"{name}_{tag}"] = rel_l2(got[pick].cpu().numpy(), want)
            assert rel[f"{name}_{tag}"] < 4e-3, f"{name}_{tag}: rel-L2 against the fp64 result {rel[f'{name}_{tag}']:.3e}"
        # the tap gradient sums over all rows: the same kernels on plans of the four picked rows, against fp64
        want_dh = np.fft.irfft(np.fft.rfft(gz64, n_ref, axis=-1) * np.conj(np.fft.rfft(u64, n_ref, axis=-1)), n_ref, axis=-1)[..., :k].sum(axis=0)
        small = tf.TfftGatedLongConvGradPlan(4, channels, L, k, 0, pre_gate=True, post_gate=True)
        small_b = tf.TfftLongConvGradPlan(4, channels, L, k, 0)
        four = {n: t[pick].contiguous() for n, t in (("x", x), ("pre", pre), ("gy", gy), ("post", post))}
        dh4, dh4_torch = torch.empty((channels, k), dtype=torch.float32, device=dev), torch.empty((channels, k), dtype=torch.float32, device=dev)
        ds4 = torch.empty((channels,), dtype=torch.float32, device=dev)
        small.tap_grad(four["x"].view(-1), four["gy"].view(-1), dh4, pre=four["pre"].view(-1), post=four["post"].view(-1), dskip=ds4)
        small_b.tap_grad((four["pre"] * four["x"]).view(-1), (four["post"] * four["gy"]).view(-1), dh4_torch)
        torch.cuda.synchronize()
        rel[f"wgrad_{tag}"] = rel_l2(dh4.cpu().numpy(), want_dh)
        rel[f"torch_wgrad_{tag}"] = rel_l2(dh4_torch.cpu().numpy(), want_dh)
        assert rel[f"wgrad_{tag}"] < 1e-2 and rel[f"torch_wgrad_{tag}"] < 1e-2, (tag, rel)
        assert torch.equal(ds4, dh4[:, 0])
        small.close()
        small_b.close()
        # full size: the fused tap gradient and the composition see the same binary16 products: the same fp32 bits
        assert torch.equal(o["dh"].view(torch.int32), o["dh_torch"].view(torch.int32)), tag
        assert torch.equal(o["dskip"].view(torch.int32), o["dh"][:, 0].contiguous().view(torch.int32)), tag

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
        cases["bconv_dgrad_k2049"]()
    times = {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, fn in cases.items():
            times[k].append(timed(fn))
    seqs = rows * channels
    out = {"length": L, "rows": rows, "channels": channels, "samples": seqs * L, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "geometry_halo_hop_segments_partials": geometry, "check": {"rel_l2_vs_fp64": rel, "wgrad_equals_torch_wgrad_bit_for_bit": True}, "cases": {}}
    for tag in taps:
        halo, hop = geometry[tag][:2]
        amp = (hop + halo) / hop
        io = {"dgrad": seqs * (4 * L * amp + 8 * L), "torch_dgrad": seqs * (2 * L * amp + 30 * L), "bconv_dgrad": seqs * (2 * L * amp + 2 * L)}
        for name in CASES:
            ts = times[f"{name}_{tag}"]
            us = statistics.median(ts)
            entry = {"us_per_call": round(us, 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1), "gsamples_s": round(seqs * L / us / 1e3, 1)}
            if name in io:
                entry["algorithmic_gbytes_s"] = round(io[name] / us / 1e3, 1)
                entry["hbm_fraction"] = round(io[name] / us / 1e3 / HBM_PEAK_GBS, 3)
            out["cases"][f"{name}_{tag}"] = entry
    c = out["cases"]
    for tag in taps:
        for num, den in (("dgrad", "torch_dgrad"), ("dgrad", "bconv_dgrad"), ("wgrad", "bconv_wgrad"), ("wgrad", "torch_wgrad"), ("dpost", "dgrad")):
            a, o = c[f"{num}_{tag}"], c[f"{den}_{tag}"]
            # the ratio of the medians, and the range the rounds allow it: fastest over slowest, slowest over fastest
            out[f"{num}_over_{den}_{tag}"] = {"median": round(a["us_per_call"] / o["us_per_call"], 3), "min": round(a["min_us"] / o["max_us"], 3),
                                             "max": round(a["max_us"] / o["min_us"], 3)}
    # the condition for calling the fusion a win: (a) below (b) with the ranges apart, at both K
    out["dgrad_faster_than_torch_dgrad_ranges_apart"] = bool(all(c[f"dgrad_{t}"]["max_us"] < c[f"torch_dgrad_{t}"]["min_us"] for t in taps))
    out["wgrad_faster_than_torch_wgrad_ranges_apart"] = bool(all(c[f"wgrad_{t}"]["max_us"] < c[f"torch_wgrad_{t}"]["min_us"] for t in taps))
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
