#!/usr/bin/env python3
"""The STFT plan against what a caller had to write before it, in one process and alternated (include/tfft_stft.h).

    python tools/stft_bench.py [--steps K] [--warmup W] [--rounds R] [--rows B] [--frames F] [--json FILE]

B = 128 real signals, F = 1024 frames of 4096 samples each under a binary16 Hann window: 131 072 frames, the frame count of
profiles/rfft_bench_line.json. Two shapes, hop = 1024 (L = 4096 + 1023 * 1024, 75 % overlap) and hop = 2048 (L = 4096 + 1023 * 2048,
50 %), each with
  stft          (a) the STFT plan: one kernel, every sample read 4096 / hop times (from cache after the first), every bin written once
  unfold_rfft   (b) what a caller does today: (x.unfold(-1, 4096, hop) * window), contiguous, then TfftRealPlan(4096, B F)
  rfft_only     (c) TfftRealPlan alone on frames built beforehand: the floor
  torch_stft    (d) for context, torch.stft in float32 (another precision, another layout), if the installed torch runs it; its
                refusal is recorded otherwise
Before anything is timed, four frames per signal of (a) are checked against fp64 rfft / 4096 of the same binary16 products, and
(a) against (b) in every bit. Timing: the protocol of tools/sconv_bench.py, i.e. RAMP untimed launches, W warm-up steps, then K
back-to-back executions between two device events on the launch stream; the cases run in turn, R rounds, and the median round is
reported with its range. Bytes are algorithmic, per frame: (a) 2 hop in and 4 * 2049 out, (b) 2 hop in, 8192 out and 8192 in for
the frames, 4 * 2049 out, (c) 8192 in and 4 * 2049 out; against 8 TB/s."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

N, BINS, PITCH = 4096, 2049, 2056
ROWS, FRAMES = 128, 1024
HOPS = (1024, 2048)
SEED = 42
RAMP = 20
HBM_PEAK_GBS = 8000.0
K_RFFT = 1.5e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--json", default="")
    args = ap.parse_args()

    import torch

    import __graft_entry__ as g

    g.build()
    import stft_ref as st
    import tensor_fft_amd as tf

    assert torch.cuda.is_available(), "stft_bench needs a GPU: a time taken anywhere else says nothing"
    dev = torch.device("cuda:0")
    rows, frames = args.rows, args.frames
    total = rows * frames
    w_host = st.hann()
    window = torch.from_numpy(w_host).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)

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

    out = {"n": N, "rows": rows, "frames_per_signal": frames, "frames": total, "window": "hann (binary16)", "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds, "shapes": {}}
    for hop in HOPS:
        length = N + (frames - 1) * hop
        x = (torch.rand((rows, length), generator=gen, device=dev) * 2 - 1).to(torch.float16)
        plan = tf.TfftStftPlan(rows, length, hop, 0, 0)
        assert plan.frames == frames and plan.kernels == ["stft4096::stft4096_kernel"] and plan.num_launches == 1
        plan.set_window(window)
        rplan = tf.TfftRealPlan(N, total, 0)
        assert rplan.num_launches() == 1
        spec = {k: torch.empty(total * 2 * PITCH, dtype=torch.float16, device=dev) for k in ("stft", "unfold_rfft", "rfft_only")}
        built = (x.unfold(-1, N, hop) * window).contiguous()          # (c)'s input, built beforehand
        xf = x.view(-1)

        def run_unfold():
            u = (x.unfold(-1, N, hop) * window).contiguous()
            rplan.r2c(u.view(-1), spec["unfold_rfft"], spec["unfold_rfft"][PITCH:])

        cases = {"stft": lambda: plan.exec(xf, spec["stft"], spec["stft"][PITCH:]), "unfold_rfft": run_unfold,
                 "rfft_only": lambda: rplan.r2c(built.view(-1), spec["rfft_only"], spec["rfft_only"][PITCH:])}
        # (d) torch.stft in float32, for context
        x32, w32 = x.float(), window.float()
        torch_note = None
        try:
            ref = torch.stft(x32, N, hop_length=hop, window=w32, center=False, return_complex=True)
            torch.cuda.synchronize()
            assert ref.shape == (rows, BINS, frames)
            del ref
            cases["torch_stft"] = lambda: torch.stft(x32, N, hop_length=hop, window=w32, center=False, return_complex=True)
        except Exception as e:       # recorded, not hidden: the case is context, not part of the comparison
            torch_note = f"{type(e).__name__}: {e}"[:300]

        # ---- checks before timing: four frames per signal against fp64, and (a) against (b) bit for bit
        for fn in cases.values():
            fn()
        torch.cuda.synchronize()
        pick = sorted({0, 1, frames // 2, frames - 1})
        got = spec["stft"].view(rows, frames, 2, PITCH)[:, pick].cpu().numpy().astype(np.float64)
        got = (got[:, :, 0, :BINS] + 1j * got[:, :, 1, :BINS]).reshape(-1, BINS)
        idx = (np.asarray(pick) * hop)[:, None] + np.arange(N)[None, :]
        u = (x.cpu().numpy()[:, idx].astype(np.float32) * w_host.astype(np.float32)).astype(np.float16).reshape(-1, N)
        rel = float(st.rel_l2(got, np.fft.rfft(u.astype(np.float64), axis=-1) / N).max())
        assert np.isfinite(got.view(np.float64)).all() and rel <= K_RFFT, f"hop {hop}: rel-L2 against fp64 {rel:.3e}"
        a = spec["stft"].view(total, 2, PITCH)[:, :, :BINS].view(torch.int16)
        same = bool(torch.equal(a, spec["unfold_rfft"].view(total, 2, PITCH)[:, :, :BINS].view(torch.int16)))
        assert same, f"hop {hop}: the STFT plan and unfold -> TfftRealPlan differ"

        for _ in range(RAMP):
            cases["rfft_only"]()
        times = {k: [] for k in cases}
        for _ in range(args.rounds):
            for k, fn in cases.items():
                times[k].append(timed(fn))
        io = {"stft": total * (2 * hop + 4 * BINS), "unfold_rfft": total * (2 * hop + 16384 + 4 * BINS), "rfft_only": total * (8192 + 4 * BINS)}
        shape = {"hop": hop, "length": length, "check": {"rel_l2_vs_fp64_worst_of_checked_frames": rel, "checked_frames_per_signal": len(pick),
                                                         "stft_equals_unfold_rfft_bit_for_bit": same}, "cases": {}}
        for k, ts in times.items():
            us = statistics.median(ts)
            shape["cases"][k] = {"us_per_call": round(us, 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
                                 "frames_per_us": round(total / us, 1)}
            if k in io:
                shape["cases"][k].update({"algorithmic_kib_per_frame": round(io[k] / total / 1024, 2), "algorithmic_gbytes_s": round(io[k] / us / 1e3, 1),
                                          "hbm_fraction": round(io[k] / us / 1e3 / HBM_PEAK_GBS, 3)})
        if torch_note:
            shape["torch_stft_refused"] = torch_note
        c = shape["cases"]
        shape["stft_over_unfold_rfft"] = round(c["stft"]["us_per_call"] / c["unfold_rfft"]["us_per_call"], 3)
        shape["stft_over_rfft_only"] = round(c["stft"]["us_per_call"] / c["rfft_only"]["us_per_call"], 3)
        # the ratios at the ends of the two ranges
        shape["stft_over_unfold_rfft_range"] = [round(c["stft"]["min_us"] / c["unfold_rfft"]["max_us"], 3), round(c["stft"]["max_us"] / c["unfold_rfft"]["min_us"], 3)]
        shape["stft_over_rfft_only_range"] = [round(c["stft"]["min_us"] / c["rfft_only"]["max_us"], 3), round(c["stft"]["max_us"] / c["rfft_only"]["min_us"], 3)]
        # acceptance: (a) faster than (b) with the ranges apart
        shape["stft_faster_than_unfold_rfft_ranges_apart"] = bool(c["stft"]["max_us"] < c["unfold_rfft"]["min_us"])
        out["shapes"]["hop_%d" % hop] = shape
        plan.close()
        rplan.close()
        del x, x32, built, spec, cases
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
