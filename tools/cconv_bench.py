#!/usr/bin/env python3
"""The carried convolution plans (include/tfft_cconv.h) against the shipped long plans they restate and against what a caller
writes without them, in one process and alternated.

    python tools/cconv_bench.py [--steps K] [--warmup W] [--rounds R] [--rows B] [--json FILE]

B x C = 256 x 64 real sequences of L = 16384 (2^28 samples), resident on the device, K = 2049 and K = 128 taps. x lies in a buffer
[B][C][halo + L] with its history in front of it, g in a buffer [B][C][L + halo] with its future behind it, so every plan below
reads the same memory with the same sequence stride (L + halo) and the context costs no copy:
  long_{fwd,dgrad,wgrad}_k*      (a) the shipped TfftLongConvPlan / TfftLongConvGradPlan on x (g) alone
  null_{fwd,dgrad,wgrad}_k*      (b) the carried plans with NULL contexts: the same windows as (a)
  ctx_{fwd,dgrad,wgrad}_k*       (c) the carried plans with history = future = halo: hist = in - halo, future = g + L
  cat_fwd_k*, cat_fwd_view_k*    (d) what a caller writes today for (c)'s forward pass: torch.cat([hist, x], -1) into a fresh buffer,
                                 the long plan at L + halo, then the slice [halo:] (copied out / left as a view)
Before anything is timed, (c) is checked against fp64 on four rows (FFTs of 65536 points in numpy).
Timing: the protocol of tools/sconv_bench.py and tools/bconv_bench.py: RAMP untimed launches, W warm-up steps, then K back-to-back
executions between two HIP events on the launch stream; the cases run in turn, R rounds, and the median round is reported with its
range. The expectation for (b) / (a) and (c) / (a) is 1; the margin is twice the relative range of (a) in the same run, and
`within_margin` says whether the ratio's distance from 1 stays inside it. (c) / (d) is the number the add-on exists for.
Not measured: other L, C and row counts, and chunk lengths below one hop, where a single segment per sequence re-reads the whole
halo."""
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
CHECK_ROWS = 4


def fp64_references(xe, ge, h, hn, fn):
    """y, dx [rows][C][L] and dh [C][K] of include/tfft_cconv.h in fp64 by FFTs of 65536 points: xe = [hist | x], ge = [g | fut]"""
    n = 65536
    taps = h.shape[1]
    hf = np.fft.rfft(h.astype(np.float64), n)[None]
    xf = np.fft.rfft(xe.astype(np.float64), n)
    y = np.fft.irfft(xf * hf, n)[..., hn:hn + L]
    dx = np.fft.irfft(np.fft.rfft(ge.astype(np.float64), n) * np.conj(hf), n)[..., :L]
    gz = np.zeros(xe.shape)                                  # g at the place of x in xe: dh[j] = sum_t gz[t] xe[t - j]
    gz[..., hn:] = ge[..., :L]
    dh = np.fft.irfft(np.conj(xf) * np.fft.rfft(gz, n), n).sum(axis=0)[:, :taps]
    return y, dx, dh


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
    import tensor_fft_amd as tf

    dev = torch.device("cuda:0")
    rows, channels = args.rows, CHANNELS
    assert rows % 2 == 0 and rows >= CHECK_ROWS
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)
    rng = np.random.default_rng(SEED)
    cases, plans, geo, check, keep = {}, [], {}, {}, []

    for k, name in ((K_LONG, "k2049"), (K_SHORT, "k128")):
        halo, hop, segments, partials, carry_min = tf.cconv_geometry(L, k, rows, channels)
        stride = L + halo
        geo[name] = {"halo": halo, "hop": hop, "segments": segments, "partials": partials, "carry_min": carry_min, "seq_stride": stride}
        taps = torch.from_numpy(lr.make_taps("decay", channels, k, rng)).to(dev)
        xb = (torch.rand((rows, channels, stride), generator=gen, device=dev) * 2 - 1).to(torch.float16)      # [hist | x]
        gb = (torch.rand((rows, channels, stride), generator=gen, device=dev) * 2 - 1).to(torch.float16)      # [g | fut]
        y = torch.empty((rows, channels, L), dtype=torch.float16, device=dev)
        dh = torch.empty((channels, k), dtype=torch.float32, device=dev)
        x_f, hist_f, g_f, fut_f, y_f = xb.view(-1)[halo:], xb.view(-1), gb.view(-1), gb.view(-1)[L:], y.view(-1)
        keep += [xb, gb, y, dh, taps]

        lf = tf.TfftLongConvPlan(rows, channels, L, k, 0, in_seq_stride=stride)
        lg = tf.TfftLongConvGradPlan(rows, channels, L, k, 0, x_seq_stride=stride, g_seq_stride=stride)
        cf = tf.TfftChunkedConvPlan(rows, channels, L, k, 0, in_seq_stride=stride, history=halo, hist_seq_stride=stride)
        cg = tf.TfftChunkedConvGradPlan(rows, channels, L, k, 0, x_seq_stride=stride, g_seq_stride=stride, history=halo, hist_seq_stride=stride,
                                        future=halo, fut_seq_stride=stride)
        cat = tf.TfftLongConvPlan(rows, channels, stride, k, 0)
        for p in (lf, lg, cf, cg, cat):
            p.set_taps(taps.view(-1))
        lg.prepare()
        cg.prepare()
        plans += [lf, lg, cf, cg, cat]
        assert lg.partials == cg.partials == partials

        cases["long_fwd_" + name] = (lambda lf=lf, a=x_f, o=y_f: lf.exec(a, o))
        cases["long_dgrad_" + name] = (lambda lg=lg, a=g_f, o=y_f: lg.input_grad(a, o))
        cases["long_wgrad_" + name] = (lambda lg=lg, a=x_f, b=g_f, d=dh: lg.tap_grad(a, b, d))
        cases["null_fwd_" + name] = (lambda cf=cf, a=x_f, o=y_f: cf.exec(a, o))
        cases["null_dgrad_" + name] = (lambda cg=cg, a=g_f, o=y_f: cg.input_grad(a, o))
        cases["null_wgrad_" + name] = (lambda cg=cg, a=x_f, b=g_f, d=dh: cg.tap_grad(a, b, d))
        cases["ctx_fwd_" + name] = (lambda cf=cf, a=x_f, c=hist_f, o=y_f: cf.exec(a, o, c))
        cases["ctx_dgrad_" + name] = (lambda cg=cg, a=g_f, c=fut_f, o=y_f: cg.input_grad(a, o, c))
        cases["ctx_wgrad_" + name] = (lambda cg=cg, a=x_f, b=g_f, c=hist_f, d=dh: cg.tap_grad(a, b, d, c))

        def cat_run(copy, cat=cat, xb=xb, halo=halo):
            # [hist | x] joined into a fresh buffer (here the two views happen to be adjacent; torch.cat copies them all the same)
            joined = torch.cat([xb[..., :halo], xb[..., halo:]], -1)
            out = torch.empty_like(joined)
            cat.exec(joined.view(-1), out.view(-1))
            return out[..., halo:].contiguous() if copy else out[..., halo:]

        cases["cat_fwd_" + name] = (lambda f=cat_run: f(True))
        cases["cat_fwd_view_" + name] = (lambda f=cat_run: f(False))

        # ---- (c) against fp64 on the first four rows, with plans of their own on contiguous copies
        r = CHECK_ROWS
        xe, ge = xb[:r].cpu().numpy(), gb[:r].cpu().numpy()
        want_y, want_dx, want_dh = fp64_references(xe, ge, taps.cpu().numpy(), halo, halo)
        t_x, t_hist = xb[:r, :, halo:], xb[:r, :, :halo]
        t_g, t_fut = gb[:r, :, :L], gb[:r, :, L:]
        got_y = tf.chunked_causal_conv(t_x, taps, t_hist).cpu().numpy().astype(np.float64)
        got_dx = tf.chunked_causal_conv_input_grad(t_g, taps, t_fut).cpu().numpy().astype(np.float64)
        got_dh = tf.chunked_causal_conv_tap_grad(t_x, t_g, k, t_hist).cpu().numpy().astype(np.float64)
        tf.cconv_cache_clear()
        rel = lambda a, b: float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))
        check[name] = {"y_rel_l2_vs_fp64": rel(got_y, want_y), "dx_rel_l2_vs_fp64": rel(got_dx, want_dx), "dh_rel_l2_vs_fp64": rel(got_dh, want_dh)}
        assert max(check[name].values()) < 3e-3, (name, check[name])
        # and (d) computes what (c) computes
        cf.exec(x_f, y_f, hist_f)
        torch.cuda.synchronize()
        rel_cat = float(((cat_run(True)[:r].float() - y[:r].float()).norm() / y[:r].float().norm()).item())
        check[name]["cat_vs_ctx_rel_l2"] = rel_cat
        assert rel_cat < 3e-3, (name, rel_cat)
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

    for _ in range(RAMP):
        cases["long_fwd_k2049"]()
    times = {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, fn in cases.items():
            times[k].append(timed(fn, args.steps, args.warmup))

    out = {"length": L, "rows": rows, "channels": channels, "samples": rows * channels * L, "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds, "geometry": geo, "check": check, "cases": {}}
    for k, ts in times.items():
        us = statistics.median(ts)
        out["cases"][k] = {"us_per_call": round(us, 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1)}
    c = out["cases"]
    for name in ("k2049", "k128"):
        for op in ("fwd", "dgrad", "wgrad"):
            a = c[f"long_{op}_{name}"]
            margin = 2 * (a["max_us"] - a["min_us"]) / a["us_per_call"]
            for which in ("null", "ctx"):
                ratio = c[f"{which}_{op}_{name}"]["us_per_call"] / a["us_per_call"]
                out[f"{which}_over_long_{op}_{name}"] = {"ratio": round(ratio, 4), "margin": round(margin, 4), "within_margin": bool(abs(ratio - 1) <= margin)}
        cc, d, dv = c["ctx_fwd_" + name], c["cat_fwd_" + name], c["cat_fwd_view_" + name]
        out["ctx_over_cat_fwd_" + name] = {"ratio": round(cc["us_per_call"] / d["us_per_call"], 3), "ctx_range_us": [cc["min_us"], cc["max_us"]],
                                           "cat_range_us": [d["min_us"], d["max_us"]], "ranges_apart": bool(cc["max_us"] < d["min_us"])}
        out["ctx_over_cat_fwd_view_" + name] = {"ratio": round(cc["us_per_call"] / dv["us_per_call"], 3), "ctx_range_us": [cc["min_us"], cc["max_us"]],
                                                "cat_range_us": [dv["min_us"], dv["max_us"]], "ranges_apart": bool(cc["max_us"] < dv["min_us"])}
    out["not_measured"] = "other L, C and row counts; chunk lengths below one hop, where a single segment per sequence re-reads the whole halo"
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    for p in plans:
        p.close()


if __name__ == "__main__":
    main()
