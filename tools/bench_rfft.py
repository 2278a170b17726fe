#!/usr/bin/env python3
"""Real-input transforms at N = 4096 against the complex headline, in one process and alternated (include/tfft.h, tfft_rplan_*).

    python tools/bench_rfft.py [--steps K] [--warmup W] [--rounds R] [--json FILE]

Cases, each on resident data born on the device with the library's hash generator (tfft_synth_uniform, seed 42):
  complex     the bench.py headline: 65536 complex transforms (1 GiB in + 1 GiB out)
  r2c_fused   131072 real signals through the fused N = 4096 kernel (the same 1 GiB in, 1.0005 GiB of half spectra out)
  r2c_2pass   the same data through TFFT_RPLAN_TWO_PASS (complex plan into the workspace + split pass)
  c2r         the half spectra back to 131072 real signals (merge pass + inverse complex plan)
Every output is checked against numpy (float64) on sampled signals before anything is timed. Timing: bench.py's protocol, i.e.
RAMP untimed launches, W warm-up steps, then K back-to-back launches between two HIP events on the launch stream; the cases run
in turn, R rounds, and the median round is reported. Real Gsamples/s counts real samples (complex: 2 per complex sample, the
zero-IM workaround's rate is half of it); bytes are algorithmic (input + output, not the workspace) against 8 TB/s."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

N = 4096
BATCH = 65536
REAL = 2 * BATCH
SEED = 42
RAMP = 100
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default="")
    args = ap.parse_args()

    import torch

    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd as tf

    dev = torch.device("cuda:0")
    x = torch.empty(REAL * N, dtype=torch.float16, device=dev)           # = 65536 [RE | IM] complex blocks
    tf.synth_uniform(x, x[N:], N, BATCH, 2 * N, 0, SEED)
    y = torch.empty_like(x)
    cplan = tf.TfftPlan(N, BATCH, 0)
    fused = tf.TfftRealPlan(N, REAL, 0)
    two = tf.TfftRealPlan(N, REAL, 0, two_pass=True)
    two.prepare()
    fused.prepare()
    h = fused.pitch
    spec = torch.empty(REAL * 2 * h, dtype=torch.float16, device=dev)
    spec2 = torch.empty_like(spec)
    back = torch.empty_like(x)

    cases = {
        "complex": lambda: cplan.exec(x, x[N:], y, y[N:]),
        "r2c_fused": lambda: fused.r2c(x, spec, spec[h:]),
        "r2c_2pass": lambda: two.r2c(x, spec2, spec2[h:]),
        "c2r": lambda: fused.c2r(spec, spec[h:], back),
    }
    # ---- checks before timing
    for fn in cases.values():
        fn()
    torch.cuda.synchronize()
    rng = np.random.default_rng(1)
    rows = np.sort(rng.choice(REAL, 64, replace=False))
    xs = x.view(REAL, N)[rows].float().cpu().numpy().astype(np.float64)
    want = np.fft.rfft(xs, axis=-1) / N
    sp = spec.view(REAL, 2 * h)[rows].float().cpu().numpy()
    got = sp[:, :N // 2 + 1] + 1j * sp[:, h:h + N // 2 + 1]
    rel = np.sqrt((np.abs(got - want) ** 2).sum(-1) / (np.abs(want) ** 2).sum(-1)).max()
    assert rel < 1.5e-3, f"r2c rel-L2 {rel:.3e}"
    assert torch.equal(spec.view(torch.int16).view(REAL, 2 * h)[:, :N // 2 + 1], spec2.view(torch.int16).view(REAL, 2 * h)[:, :N // 2 + 1])
    assert torch.equal(spec.view(torch.int16).view(REAL, 2 * h)[:, h:h + N // 2 + 1], spec2.view(torch.int16).view(REAL, 2 * h)[:, h:h + N // 2 + 1])
    bk = back.view(REAL, N)[rows].float().cpu().numpy()
    rt = np.sqrt(((bk - xs / N) ** 2).sum(-1) / ((xs / N) ** 2).sum(-1)).max()
    assert rt < 3e-3, f"c2r(r2c(x)) rel-L2 {rt:.3e}"
    cb = y.view(BATCH, 2 * N)[rows // 2].double().cpu().numpy()
    cx = x.view(BATCH, 2 * N)[rows // 2].double().cpu().numpy()
    cw = np.fft.fft(cx[:, :N] + 1j * cx[:, N:], axis=-1) / N
    crel = np.sqrt((np.abs(cb[:, :N] + 1j * cb[:, N:] - cw) ** 2).sum(-1) / (np.abs(cw) ** 2).sum(-1)).max()
    assert crel < 1.5e-3, f"complex rel-L2 {crel:.3e}"

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
    spec_bytes = REAL * (N // 2 + 1) * 4
    io = {"complex": (BATCH * N * 4, BATCH * N * 4), "r2c_fused": (REAL * N * 2, spec_bytes), "r2c_2pass": (REAL * N * 2, spec_bytes),
          "c2r": (spec_bytes, REAL * N * 2)}
    out = {"n": N, "real_signals": REAL, "complex_transforms": BATCH, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "check": {"r2c_rel_l2": float(rel), "roundtrip_rel_l2": float(rt), "complex_rel_l2": float(crel), "fused_equals_two_pass": True},
           "launches": {"r2c_fused": fused.num_launches(), "r2c_2pass": two.num_launches(), "c2r": fused.num_launches(True)},
           "cases": {}}
    for k, ts in times.items():
        us = statistics.median(ts)
        rb, wb = io[k]
        out["cases"][k] = {"us_per_call": round(us, 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
                           "real_gsamples_s": round(REAL * N / us / 1e3, 1),
                           "gbytes_s": round((rb + wb) / us / 1e3, 1), "hbm_fraction": round((rb + wb) / us / 1e3 / HBM_PEAK_GBS, 3)}
    out["fused_over_complex"] = round(out["cases"]["r2c_fused"]["us_per_call"] / out["cases"]["complex"]["us_per_call"], 3)
    out["two_pass_over_fused"] = round(out["cases"]["r2c_2pass"]["us_per_call"] / out["cases"]["r2c_fused"]["us_per_call"], 3)
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
