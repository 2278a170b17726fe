#!/usr/bin/env python3
"""The gated carried convolution plans (include/tfft_gcconv.h) against the shipped gated plans they restate and against the two
things a caller writes without them, in one process and alternated.

    python tools/gcconv_bench.py [--steps K] [--warmup W] [--rounds R] [--rows B] [--json FILE]

B x C = 256 x 64 real sequences of L = 16384 (2^28 samples), resident on the device, K = 2049 and K = 128 taps, both gates and a skip.
x and the pre gate lie in buffers [B][C][halo + L] with their histories in front of them, gy and the post gate in buffers
[B][C][L + halo] with their futures behind them, so every plan below reads the same memory with the same sequence stride (L + halo)
and the contexts cost no copy:
  long_{fwd,dgrad,wgrad}_k*   (a) the shipped TfftGatedLongConvPlan / TfftGatedLongConvGradPlan on x (gy) alone
  null_{fwd,dgrad,wgrad}_k*   (b) the carried plans with NULL contexts: the same windows as (a)
  ctx_{fwd,dgrad,wgrad}_k*    (c) the carried plans with history = future = halo: hist = x - halo, pre_hist = pre - halo,
                              future = gy + L, post_future = post + L
  cat_{fwd,dgrad}_k*          (d) what a caller writes today for (c): torch.cat of x and of pre with their histories into fresh buffers,
                              the shipped gated plan at L + halo (post gate padded with ones), the slice [halo:] copied out; backward:
                              torch.cat of gy and of post with their futures, x and pre padded, the gated gradient plan at L + halo,
                              dx and dpre sliced and copied out
  hand_{fwd,dgrad}_k*         (e) the ungate-by-hand route: pre * x over [history | chunk] in torch, the UNGATED carried plan
                              (chunked_causal_conv's), then post * (z + skip * u) in torch; backward: post * gy over [chunk | future],
                              the ungated carried input gradient, then pre * du and x * du (du + skip * gz first)
Before anything is timed, (c) is checked against fp64 on four rows (FFTs of 65536 points in numpy), and (d) and (e) against (c).
Timing: the protocol of tools/cconv_bench.py: RAMP untimed launches, W warm-up steps, then K back-to-back executions between two HIP
events on the launch stream; the cases run in turn, R rounds, and the median round is reported with its range. (c) / (a) is called
within noise only if its distance from 1 lies inside twice the relative range of (a) in the same run (`within_margin`); otherwise it
is a finding. (c) / (d) and (c) / (e) are the numbers the add-on exists for.
Not measured: other L, C and row counts, single-gate plans, chunk lengths below one hop (where a single segment per sequence re-reads
the whole halo), and the tap gradient's (d) and (e) routes."""
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


def fp64_references(xe, pe, ge, qe, h, skip, hn):
    """y, dx, dpre [rows][C][L] and dh [C][K] of include/tfft_gcconv.h in fp64 by FFTs of 65536 points: xe = [hist | x],
    pe = [pre_hist | pre], ge = [gy | fut], qe = [post | post_fut]"""
    n = 65536
    taps = h.shape[1]
    hs = h.astype(np.float64).copy()
    hs[:, 0] += skip.astype(np.float64)
    hf = np.fft.rfft(hs, n)[None]
    xe, pe, ge, qe = (a.astype(np.float64) for a in (xe, pe, ge, qe))
    uf = np.fft.rfft(pe * xe, n)
    y = qe[..., :L] * np.fft.irfft(uf * hf, n)[..., hn:hn + L]
    du = np.fft.irfft(np.fft.rfft(qe * ge, n) * np.conj(hf), n)[..., :L]
    gz = np.zeros(xe.shape)                                  # gz at the place of x in xe: dh[j] = sum_t gz[t] ue[t - j]
    gz[..., hn:] = (qe * ge)[..., :L]
    dh = np.fft.irfft(np.conj(uf) * np.fft.rfft(gz, n), n).sum(axis=0)[:, :taps]
    return y, pe[..., hn:] * du, xe[..., hn:] * du, dh


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
    gates = dict(pre_gate=True, post_gate=True)

    def add_cases(k, name):
        """everything of one K; a function, so that the cases' closures hold this K's plans and buffers"""
        halo, hop, segments, partials, carry_min = tf.gcconv_geometry(L, k, rows, channels)
        stride = L + halo
        geo[name] = {"halo": halo, "hop": hop, "segments": segments, "partials": partials, "carry_min": carry_min, "seq_stride": stride}
        taps = torch.from_numpy(lr.make_taps("decay", channels, k, rng)).to(dev)
        skip = torch.from_numpy(((0.5 - 0.125 * (np.arange(channels) % 4)) * (-1.0) ** np.arange(channels)).astype(np.float16)).to(dev)
        rand = lambda: (torch.rand((rows, channels, stride), generator=gen, device=dev) * 2 - 1).to(torch.float16)    # noqa: E731
        xb, pb, gb, qb = rand(), rand(), rand(), rand()                # [hist | x], [pre_hist | pre], [gy | fut], [post | post_fut]
        y = torch.empty((rows, channels, L), dtype=torch.float16, device=dev)
        y2 = torch.empty_like(y)
        dh = torch.empty((channels, k), dtype=torch.float32, device=dev)
        dskip = torch.empty((channels,), dtype=torch.float32, device=dev)
        x_f, hist_f, p_f, phist_f = xb.view(-1)[halo:], xb.view(-1), pb.view(-1)[halo:], pb.view(-1)
        g_f, fut_f, q_f, qfut_f = gb.view(-1), gb.view(-1)[L:], qb.view(-1), qb.view(-1)[L:]
        y_f, y2_f = y.view(-1), y2.view(-1)
        keep.extend([xb, pb, gb, qb, y, y2, dh, dskip, taps, skip])

        st = dict(pre_seq_stride=stride, post_seq_stride=stride)
        lf = tf.TfftGatedLongConvPlan(rows, channels, L, k, 0, in_seq_stride=stride, **st, **gates)
        lg = tf.TfftGatedLongConvGradPlan(rows, channels, L, k, 0, x_seq_stride=stride, gy_seq_stride=stride, **st, **gates)
        cf = tf.TfftGatedChunkedConvPlan(rows, channels, L, k, 0, in_seq_stride=stride, history=halo, hist_seq_stride=stride,
                                         pre_hist_seq_stride=stride, **st, **gates)
        cg = tf.TfftGatedChunkedConvGradPlan(rows, channels, L, k, 0, x_seq_stride=stride, gy_seq_stride=stride, history=halo,
                                             hist_seq_stride=stride, pre_hist_seq_stride=stride, future=halo, fut_seq_stride=stride,
                                             post_fut_seq_stride=stride, **st, **gates)
        cat_f = tf.TfftGatedLongConvPlan(rows, channels, stride, k, 0, **gates)
        cat_g = tf.TfftGatedLongConvGradPlan(rows, channels, stride, k, 0, **gates)
        # (e): the ungated carried plans on a buffer of products with the same layout
        hf = tf.TfftChunkedConvPlan(rows, channels, L, k, 0, in_seq_stride=stride, history=halo, hist_seq_stride=stride)
        hg = tf.TfftChunkedConvGradPlan(rows, channels, L, k, 0, g_seq_stride=stride, future=halo, fut_seq_stride=stride)
        for p in (lf, lg, cf, cg, cat_f, cat_g):
            p.set_taps(taps.view(-1), skip)
        for p in (hf, hg):
            p.set_taps(taps.view(-1))
        lg.prepare()
        cg.prepare()
        plans.extend([lf, lg, cf, cg, cat_f, cat_g, hf, hg])
        assert lg.partials == cg.partials == partials

        cases["long_fwd_" + name] = (lambda: lf.exec(x_f, y_f, pre=p_f, post=q_f))
        cases["long_dgrad_" + name] = (lambda: lg.input_grad(g_f, y_f, post=q_f, x=x_f, pre=p_f, dpre=y2_f))
        cases["long_wgrad_" + name] = (lambda: lg.tap_grad(x_f, g_f, dh, pre=p_f, post=q_f, dskip=dskip))
        cases["null_fwd_" + name] = (lambda: cf.exec(x_f, y_f, pre=p_f, post=q_f))
        cases["null_dgrad_" + name] = (lambda: cg.input_grad(g_f, y_f, post=q_f, x=x_f, pre=p_f, dpre=y2_f))
        cases["null_wgrad_" + name] = (lambda: cg.tap_grad(x_f, g_f, dh, pre=p_f, post=q_f, dskip=dskip))
        cases["ctx_fwd_" + name] = (lambda: cf.exec(x_f, y_f, pre=p_f, post=q_f, hist=hist_f, pre_hist=phist_f))
        cases["ctx_dgrad_" + name] = (lambda: cg.input_grad(g_f, y_f, post=q_f, x=x_f, pre=p_f, dpre=y2_f, future=fut_f, post_future=qfut_f))
        cases["ctx_wgrad_" + name] = (lambda: cg.tap_grad(x_f, g_f, dh, pre=p_f, post=q_f, dskip=dskip, history=hist_f, pre_history=phist_f))

        ones = torch.ones((rows, channels, halo), dtype=torch.float16, device=dev)
        keep.append(ones)

        def cat_fwd():
            # [hist | x] and [pre_hist | pre] joined into fresh buffers (here the views happen to be adjacent; torch.cat copies them all
            # the same), the post gate padded in front
            jx = torch.cat([xb[..., :halo], xb[..., halo:]], -1)
            jp = torch.cat([pb[..., :halo], pb[..., halo:]], -1)
            jq = torch.cat([ones, qb[..., :L]], -1)
            out = torch.empty_like(jx)
            cat_f.exec(jx.view(-1), out.view(-1), pre=jp.view(-1), post=jq.view(-1))
            return out[..., halo:].contiguous()

        def cat_dgrad():
            jg = torch.cat([gb[..., :L], gb[..., L:]], -1)
            jq = torch.cat([qb[..., :L], qb[..., L:]], -1)
            jx = torch.cat([xb[..., halo:], ones], -1)
            jp = torch.cat([pb[..., halo:], ones], -1)
            dx, dpre = torch.empty_like(jg), torch.empty_like(jg)
            cat_g.input_grad(jg.view(-1), dx.view(-1), post=jq.view(-1), x=jx.view(-1), pre=jp.view(-1), dpre=dpre.view(-1))
            return dx[..., :L].contiguous(), dpre[..., :L].contiguous()

        def hand_fwd():
            u = pb * xb                                                           # [pre_hist * hist | pre * x]
            uf = u.view(-1)
            z = torch.empty((rows, channels, L), dtype=torch.float16, device=dev)
            hf.exec(uf[halo:], z.view(-1), uf)
            return qb[..., :L] * (z + skip[None, :, None] * u[..., halo:])

        def hand_dgrad():
            gz = qb * gb                                                          # [post * gy | post_fut * fut]
            gf = gz.view(-1)
            du = torch.empty((rows, channels, L), dtype=torch.float16, device=dev)
            hg.input_grad(gf, du.view(-1), gf[L:])
            du = du + skip[None, :, None] * gz[..., :L]
            return pb[..., halo:] * du, xb[..., halo:] * du

        cases["cat_fwd_" + name], cases["cat_dgrad_" + name] = cat_fwd, cat_dgrad
        cases["hand_fwd_" + name], cases["hand_dgrad_" + name] = hand_fwd, hand_dgrad

        # ---- (c) against fp64 on the first four rows, through the convenience functions on views of the buffers
        r = CHECK_ROWS
        host = lambda t: t[:r].cpu().numpy()                                      # noqa: E731
        want_y, want_dx, want_dpre, want_dh = fp64_references(host(xb), host(pb), host(gb), host(qb), taps.cpu().numpy(), skip.cpu().numpy(), halo)
        v = dict(x=xb[:r, :, halo:], hist=xb[:r, :, :halo], pre=pb[:r, :, halo:], pre_hist=pb[:r, :, :halo], gy=gb[:r, :, :L], fut=gb[:r, :, L:],
                 post=qb[:r, :, :L], post_fut=qb[:r, :, L:])
        got_y = tf.gated_chunked_causal_conv(v["x"], taps, pre=v["pre"], post=v["post"], skip=skip, history=v["hist"], pre_history=v["pre_hist"])
        got_dx, got_dpre = tf.gated_chunked_causal_conv_input_grad(v["gy"], taps, x=v["x"], pre=v["pre"], post=v["post"], skip=skip, future=v["fut"],
                                                                   post_future=v["post_fut"])
        got_dh, _ = tf.gated_chunked_causal_conv_tap_grad(v["x"], v["gy"], k, pre=v["pre"], post=v["post"], history=v["hist"], pre_history=v["pre_hist"])
        tf.gcconv_cache_clear()
        n64 = lambda t: t.cpu().numpy().astype(np.float64)                        # noqa: E731
        rel = lambda a, b: float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))  # noqa: E731
        check[name] = {"y_rel_l2_vs_fp64": rel(n64(got_y), want_y), "dx_rel_l2_vs_fp64": rel(n64(got_dx), want_dx),
                       "dpre_rel_l2_vs_fp64": rel(n64(got_dpre), want_dpre), "dh_rel_l2_vs_fp64": rel(n64(got_dh), want_dh)}
        assert max(check[name].values()) < 3e-3, (name, check[name])
        # and (d) and (e) compute what (c) computes
        cases["ctx_fwd_" + name]()
        torch.cuda.synchronize()
        relt = lambda a, b: float(((a[:r].float() - b[:r].float()).norm() / b[:r].float().norm()).item())    # noqa: E731
        check[name]["cat_fwd_vs_ctx_rel_l2"] = relt(cat_fwd(), y)
        check[name]["hand_fwd_vs_ctx_rel_l2"] = relt(hand_fwd(), y)
        cases["ctx_dgrad_" + name]()
        torch.cuda.synchronize()
        for route, fn in (("cat", cat_dgrad), ("hand", hand_dgrad)):
            dx, dpre = fn()
            check[name][route + "_dgrad_vs_ctx_rel_l2"] = max(relt(dx, y), relt(dpre, y2))
        assert max(v for key, v in check[name].items() if key.endswith("_vs_ctx_rel_l2")) < 3e-3, (name, check[name])

    for k, name in ((K_LONG, "k2049"), (K_SHORT, "k128")):
        add_cases(k, name)
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
           "rounds": args.rounds, "mode": "pre+post+skip", "geometry": geo, "check": check, "cases": {}}
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
        for op in ("fwd", "dgrad"):
            cc = c[f"ctx_{op}_{name}"]
            for route in ("cat", "hand"):
                d = c[f"{route}_{op}_{name}"]
                out[f"ctx_over_{route}_{op}_{name}"] = {"ratio": round(cc["us_per_call"] / d["us_per_call"], 3), "ctx_range_us": [cc["min_us"], cc["max_us"]],
                                                        route + "_range_us": [d["min_us"], d["max_us"]], "ranges_apart": bool(cc["max_us"] < d["min_us"])}
    out["not_measured"] = ("other L, C and row counts; single-gate plans; chunk lengths below one hop, where a single segment per sequence re-reads the "
                           "whole halo; the tap gradient's cat and by-hand routes")
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    for p in plans:
        p.close()


if __name__ == "__main__":
    main()
