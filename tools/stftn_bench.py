#!/usr/bin/env python3
"""The short-frame STFT plans against what a caller had to write before them, in one process and alternated (include/tfft_stftn.h).

    python tools/stftn_bench.py [--steps K] [--warmup W] [--rounds R] [--rows B] [--samples S] [--json FILE]

B = 128 real signals under a binary16 Hann window, pad 0, S = 2^29 output-side samples (frames x n, the count of tools/stft_bench.py):
n = 512 with hop 128 (8192 frames per signal), n = 1024 with hop 256 (4096), n = 2048 with hop 512 (2048); 75 % overlap. Each with
  stftn         (a) the plan: one kernel, every sample read n / hop times (from cache after the first), every bin written once
  unfold_rfft   (b) what a caller does today: (x.unfold(-1, n, hop) * window), contiguous, then TfftRealPlan(n, B F), which at
                these n is a complex plan into a workspace and a split pass
  rfft_only     (c) TfftRealPlan alone on frames built beforehand
  torch_stft    (d) for context, torch.stft in float32 (another precision, another layout), if the installed torch runs it; its
                refusal is recorded otherwise
Before anything is timed, four frames per signal of (a) are checked against fp64 rfft / n of the same binary16 products, and (a)
against (b) in every bit. Timing: the protocol of tools/stft_bench.py, i.e. RAMP untimed launches, W warm-up steps, then K
back-to-back executions between two device events on the launch stream; the cases run in turn, R rounds, and the median round is
reported with its range. Bytes are algorithmic, per frame: (a) 2 hop in and 4 (n / 2 + 1) out; (b) 2 hop in, 2 n out and 2 n in for
the frames, 2 n out and 2 n in for the spectrum in the workspace, 4 (n / 2 + 1) out; (c) 2 n in, 2 n out and 2 n in for the
workspace, 4 (n / 2 + 1) out; against 8 TB/s."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

ROWS, SAMPLES = 128, 1 << 29
SHAPES = ((512, 128), (1024, 256), (2048, 512))          # (n, hop)
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
    ap.add_argument("--samples", type=int, default=SAMPLES)
    ap.add_argument("--json", default="")
    args = ap.parse_args()

    import torch

    import __graft_entry__ as g

    g.build()
    import stftn_ref as sn
    import tensor_fft_amd as tf

    assert torch.cuda.is_available(), "stftn_bench needs a GPU: a time taken anywhere else says nothing"
    dev = torch.device("cuda:0")
    rows = args.rows
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

    out = {"rows": rows, "output_side_samples": args.samples, "window": "hann (binary16)", "pad": 0, "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds, "shapes": {}}
    for n, hop in SHAPES:
        bins, pitch = sn.bins(n), sn.pitch(n)
        frames = args.samples // n // rows
        total = rows * frames
        length = n + (frames - 1) * hop
        w_host = sn.hann(n)
        window = torch.from_numpy(w_host).to(dev)
        x = (torch.rand((rows, length), generator=gen, device=dev) * 2 - 1).to(torch.float16)
        plan = tf.TfftShortStftPlan(n, rows, length, hop, 0, 0)
        assert plan.frames == frames and plan.kernels == [f"stft256r::stft256r_kernel<{n // 256}>"] and plan.num_launches == 1
        plan.set_window(window)
        rplan = tf.TfftRealPlan(n, total, 0)
        spec = {k: torch.empty(total * 2 * pitch, dtype=torch.float16, device=dev) for k in ("stftn", "unfold_rfft", "rfft_only")}
        built = (x.unfold(-1, n, hop) * window).contiguous()          # (c)'s input, built beforehand
        xf = x.view(-1)

        def run_unfold():
            u = (x.unfold(-1, n, hop) * window).contiguous()
            rplan.r2c(u.view(-1), spec["unfold_rfft"], spec["unfold_rfft"][pitch:])

        cases = {"stftn": lambda: plan.exec(xf, spec["stftn"], spec["stftn"][pitch:]), "unfold_rfft": run_unfold,
                 "rfft_only": lambda: rplan.r2c(built.view(-1), spec["rfft_only"], spec["rfft_only"][pitch:])}
        # (d) torch.stft in float32, for context
        x32, w32 = x.float(), window.float()
        torch_note = None
        try:
            ref = torch.stft(x32, n, hop_length=hop, window=w32, center=False, return_complex=True)
            torch.cuda.synchronize()
            assert ref.shape == (rows, bins, frames)
            del ref
            cases["torch_stft"] = lambda: torch.stft(x32, n, hop_length=hop, window=w32, center=False, return_complex=True)
        except Exception as e:       # recorded, not hidden: the case is context, not part of the comparison
            torch_note = f"{type(e).__name__}: {e}"[:300]

        # ---- checks before timing: four frames per signal against fp64, and (a) against (b) bit for bit
        for fn in cases.values():
            fn()
        torch.cuda.synchronize()
        pick = sorted({0, 1, frames // 2, frames - 1})
        got = spec["stftn"].view(rows, frames, 2, pitch)[:, pick].cpu().numpy().astype(np.float64)
        got = (got[:, :, 0, :bins] + 1j * got[:, :, 1, :bins]).reshape(-1, bins)
        idx = (np.asarray(pick) * hop)[:, None] + np.arange(n)[None, :]
        u = (x.cpu().numpy()[:, idx].astype(np.float32) * w_host.astype(np.float32)).astype(np.float16).reshape(-1, n)
        rel = float(sn.rel_l2(got, np.fft.rfft(u.astype(np.float64), axis=-1) / n).max())
        assert np.isfinite(got.view(np.float64)).all() and rel <= K_RFFT, f"n {n}: rel-L2 against fp64 {rel:.3e}"
        a = spec["stftn"].view(total, 2, pitch)[:, :, :bins].view(torch.int16)
        same = bool(torch.equal(a, spec["unfold_rfft"].view(total, 2, pitch)[:, :, :bins].view(torch.int16)))
        assert same, f"n {n}: the plan and unfold -> TfftRealPlan differ"

        for _ in range(RAMP):
            cases["rfft_only"]()
        times = {k: [] for k in cases}
        for _ in range(args.rounds):
            for k, fn in cases.items():
                times[k].append(timed(fn))
        io = {"stftn": total * (2 * hop + 4 * bins), "unfold_rfft": total * (2 * hop + 8 * n + 4 * bins), "rfft_only": total * (6 * n + 4 * bins)}
        shape = {"n": n, "hop": hop, "length": length, "frames_per_signal": frames, "frames": total,
                 "real_plan_launches": rplan.num_launches(),
                 "check": {"rel_l2_vs_fp64_worst_of_checked_frames": rel, "checked_frames_per_signal": len(pick),
                           "stftn_equals_unfold_rfft_bit_for_bit": same}, "cases": {}}
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
        shape["stftn_over_unfold_rfft"] = round(c["stftn"]["us_per_call"] / c["unfold_rfft"]["us_per_call"], 3)
        shape["stftn_over_rfft_only"] = round(c["stftn"]["us_per_call"] / c["rfft_only"]["us_per_call"], 3)
        # the ratios at the ends of the two ranges
        shape["stftn_over_unfold_rfft_range"] = [round(c["stftn"]["min_us"] / c["unfold_rfft"]["max_us"], 3), round(c["stftn"]["max_us"] / c["unfold_rfft"]["min_us"], 3)]
        shape["stftn_over_rfft_only_range"] = [round(c["stftn"]["min_us"] / c["rfft_only"]["max_us"], 3), round(c["stftn"]["max_us"] / c["rfft_only"]["min_us"], 3)]
        # whether the ranges of the two cases are apart, and which way
        shape["stftn_faster_than_unfold_rfft_ranges_apart"] = bool(c["stftn"]["max_us"] < c["unfold_rfft"]["min_us"])
        shape["stftn_faster_than_rfft_only_ranges_apart"] = bool(c["stftn"]["max_us"] < c["rfft_only"]["min_us"])
        shape["stftn_slower_than_rfft_only_ranges_apart"] = bool(c["stftn"]["min_us"] > c["rfft_only"]["max_us"])
        out["shapes"]["n_%d" % n] = shape
        plan.close()
        rplan.close()
        del x, x32, built, spec, cases
        torch.cuda.empty_cache()
    out["not_measured"] = ["other hops", "padded plans (pad > 0)", "other row counts", "no PMC (hardware counter) run was made"]
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
