#!/usr/bin/env python3
"""The spectrogram plans against what a caller had to write before them, in one process and alternated (include/tfft_spec.h).

    python tools/spec_bench.py [--steps K] [--warmup W] [--rounds R] [--rows B] [--samples S] [--json FILE]

B = 128 real signals under a binary16 Hann window, pad 0, S = 2^29 frame-side samples (frames x n, the count of tools/stftn_bench.py):
n = 512, 1024 and 2048 at hop n / 4, and n = 512 at hop 160 (the speech front end). Each with
  power         (a) the power plan: one kernel, every sample read n / hop times, n / 2 + 1 floats written per frame
  stft_square   (b) what a caller does today: short_stft, then re.float() ** 2 + im.float() ** 2 in torch
  bands         (c) the band plan with mel_bands(n, 16000, 80): one kernel, 80 floats written per frame
  stft_matmul   (d) (b), then a matmul with the dense [n / 2 + 1, 80] bank
all at gain 1. Before anything is timed, (a) is held to (b) in every bit over the whole output (torch's float32 square and sum
are the restatement's), and (c) to the sequential float32 restatement of tests/spec_ref.py on the first, a middle and the last frame
of every signal. Timing: the protocol of tools/stftn_bench.py, i.e. RAMP untimed launches, W warm-up steps, then K back-to-back
executions between two device events on the launch stream; the cases run in turn, R rounds, and the median round is reported with
its range, every ratio with the ratios at the ends of the two ranges. The byte counts say (a) < (b) and (c) < (d); whether the
time follows is what this driver records, either way. Bytes are algorithmic, per frame: (a) 2 hop in, 4 (n / 2 + 1) out; (c) 2 hop
in, 4 B out; the short_stft inside (b) and (d) 2 hop in, 4 (n / 2 + 1) out; against 8 TB/s."""
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
SHAPES = ((512, 128), (1024, 256), (2048, 512), (512, 160))          # (n, hop)
MELS, RATE = 80, 16000
SEED = 42
RAMP = 20
HBM_PEAK_GBS = 8000.0


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
    import spec_ref as sr
    import stftn_ref as sn
    import tensor_fft_amd as tf

    assert torch.cuda.is_available(), "spec_bench needs a GPU: a time taken anywhere else says nothing"
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

    out = {"rows": rows, "frame_side_samples": args.samples, "window": "hann (binary16)", "pad": 0, "gain": 1.0, "bands": f"mel_bands(n, {RATE}, {MELS})",
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "shapes": {}, "findings": []}
    for n, hop in SHAPES:
        bins, pitch = sn.bins(n), sn.pitch(n)
        frames = args.samples // n // rows
        total = rows * frames
        length = n + (frames - 1) * hop
        window = torch.from_numpy(sn.hann(n)).to(dev)
        x = (torch.rand((rows, length), generator=gen, device=dev) * 2 - 1).to(torch.float16)
        mel = tf.mel_bands(n, RATE, MELS)
        dense = torch.from_numpy(np.ascontiguousarray(mel.dense(bins).T)).to(dev)          # [bins, 80]
        p_plan = tf.TfftSpectrogramPlan(n, rows, length, hop)
        b_plan = tf.TfftSpectrogramPlan(n, rows, length, hop, bands=MELS)
        assert p_plan.frames == frames and p_plan.kernels == [f"spec256r::spec_kernel<{n // 256}, false>"] and p_plan.num_launches == 1
        assert b_plan.kernels == [f"spec256r::spec_kernel<{n // 256}, true>"] and b_plan.num_launches == 1
        for plan in (p_plan, b_plan):
            plan.set_window(window)
        b_plan.set_bands(mel)
        p_out = torch.empty(total * pitch, dtype=torch.float32, device=dev)
        b_out = torch.empty(total * MELS, dtype=torch.float32, device=dev)
        xf = x.view(-1)

        def stft_square():
            re, im = tf.short_stft(x, window, hop, n)
            return re.float() ** 2 + im.float() ** 2

        cases = {"power": lambda: p_plan.exec(xf, p_out), "stft_square": stft_square, "bands": lambda: b_plan.exec(xf, b_out),
                 "stft_matmul": lambda: torch.matmul(stft_square(), dense)}

        # ---- checks before timing
        for name in ("power", "bands"):
            cases[name]()
        want = stft_square()
        torch.cuda.synchronize()
        got = p_out.view(rows, frames, pitch)[:, :, :bins]
        power_same = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
        assert power_same, f"n {n} hop {hop}: the power plan and short_stft -> re^2 + im^2 differ"
        pick = sorted({0, frames // 2, frames - 1})
        ref = sr.band_energies(want[:, pick].reshape(-1, bins).cpu().numpy(), sr.bands_of(mel.dense(bins)))
        bands_same = bool(np.array_equal(b_out.view(rows, frames, MELS)[:, pick].reshape(-1, MELS).cpu().numpy().view(np.uint32), ref.view(np.uint32)))
        assert bands_same, f"n {n} hop {hop}: the band plan and the sequential float32 restatement differ"
        del want, got

        for _ in range(RAMP):
            cases["power"]()
        times = {k: [] for k in cases}
        for _ in range(args.rounds):
            for k, fn in cases.items():
                times[k].append(timed(fn))
        io = {"power": total * (2 * hop + 4 * bins), "bands": total * (2 * hop + 4 * MELS)}
        shape = {"n": n, "hop": hop, "length": length, "frames_per_signal": frames, "frames": total,
                 "check": {"power_equals_stft_square_bit_for_bit": power_same, "bands_equal_restatement_bit_for_bit": bands_same,
                           "band_frames_checked_per_signal": len(pick)}, "cases": {}}
        for k, ts in times.items():
            us = statistics.median(ts)
            shape["cases"][k] = {"us_per_call": round(us, 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1), "frames_per_us": round(total / us, 1)}
            if k in io:
                shape["cases"][k].update({"algorithmic_bytes_per_frame": io[k] // total, "algorithmic_gbytes_s": round(io[k] / us / 1e3, 1),
                                          "hbm_fraction": round(io[k] / us / 1e3 / HBM_PEAK_GBS, 3)})
        c = shape["cases"]
        for a, b in (("power", "stft_square"), ("bands", "stft_matmul"), ("bands", "power")):
            shape[f"{a}_over_{b}"] = round(c[a]["us_per_call"] / c[b]["us_per_call"], 3)
            shape[f"{a}_over_{b}_range"] = [round(c[a]["min_us"] / c[b]["max_us"], 3), round(c[a]["max_us"] / c[b]["min_us"], 3)]
            shape[f"{a}_faster_than_{b}_ranges_apart"] = bool(c[a]["max_us"] < c[b]["min_us"])
            shape[f"{a}_slower_than_{b}_ranges_apart"] = bool(c[a]["min_us"] > c[b]["max_us"])
        for a, b in (("power", "stft_square"), ("bands", "stft_matmul")):
            if not shape[f"{a}_faster_than_{b}_ranges_apart"]:
                out["findings"].append(f"n {n} hop {hop}: the byte counts say {a} < {b} with the ranges apart; measured {c[a]['us_per_call']} us "
                                       f"({c[a]['min_us']}-{c[a]['max_us']}) against {c[b]['us_per_call']} us ({c[b]['min_us']}-{c[b]['max_us']})")
        if shape["bands_slower_than_power_ranges_apart"]:
            out["findings"].append(f"n {n} hop {hop}: the band plan writes {4 * MELS} bytes per frame where the power plan writes {4 * bins}, and is slower: "
                                   f"{c['bands']['us_per_call']} us against {c['power']['us_per_call']} us; the band tasks cost more than the stores they save")
        out["shapes"][f"n_{n}_hop_{hop}"] = shape
        p_plan.close()
        b_plan.close()
        tf.stftn_cache_clear()
        del x, p_out, b_out, cases, dense
        torch.cuda.empty_cache()
    out["not_measured"] = ["other hops", "padded plans (pad > 0)", "other row counts", "other band counts and banks", "other gains",
                           "no PMC (hardware counter) run was made"]
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
