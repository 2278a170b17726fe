#!/usr/bin/env python3
"""The ISTFT plan against what a caller had to write before it, in one process and alternated (include/tfft_istft.h).

    python tools/istft_bench.py [--steps K] [--warmup W] [--rounds R] [--rows B] [--frames F] [--json FILE]

B = 128 real signals, F = 1024 frames of 4096 samples each under a binary16 Hann window: 131 072 frames, the frame count of
profiles/stft_bench_line.json. Two shapes, hop = 1024 (L = 4096 + 1023 * 1024) and hop = 2048 (L = 4096 + 1023 * 2048), pad 0. The
spectra are what TfftStftPlan writes for random signals. Each shape with
  istft         (a) the ISTFT plan: frames_kernel (one-pass C2R with the gain, into the workspace) and ola_kernel
  frames_only   (a') frames_kernel alone, as nearly as the interface gives it: a second ISTFT plan on the SAME spectra, frames and
                pairing, cut as B F / 2 signals of L = 8 with pad 2048 and hop 8 (two frames each), so that its ola_kernel writes 8
                samples per signal (B F / 2 chunks, 32 bytes read each) and the rest of the execution is frames_kernel on all B F frames.
                (a) - (a') is recorded as what ola_kernel adds
  c2r_fold      (b) what a caller does today: TfftRealPlan.c2r (merge pass + inverse plan), * (4096 * window), overlap-add with
                torch.nn.functional.fold (index_add_ where fold refuses binary16), / a precomputed envelope
  c2r_only      (c) TfftRealPlan.c2r alone: the floor of (b), and the comparison for frames_kernel
  torch_istft   (d) for context, torch.istft in float32 (another precision, another layout, center=True framing of the same frame
                count: torch refuses a Hann window with center=False, whose envelope is 0 at sample 0), if the installed torch runs it
Before anything is timed, four frames per signal of (a)'s workspace are checked against fp64 irfft * 4096 of the same binary16
spectra, and the output of signal 0 against tests/istft_ref.ola of its frames in every bit. Timing: the protocol of
tools/stft_bench.py, i.e. RAMP untimed launches, W warm-up steps, then K back-to-back executions between two device events on the
launch stream; the cases run in turn, R rounds, and the median round is reported with its range. Bytes are algorithmic, per frame:
(a) 4 * 2049 in, 8192 out and 8192 in for the frames, 2 hop out; (a') 4 * 2049 in, 8192 out; (b) 4 * 2049 in, 8192 out and in for Z
(one complex spectrum of 4096 per PAIR of frames), 8192 out, 8192 in and out for the product, 8192 in for the overlap-add, 2 hop out,
and 2 hop in and out for the division; (c) 4 * 2049 in, 8192 out and in for Z, 8192 out; against 8 TB/s."""
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
K_C2R = 1.5e-3            # per pair (tests/test_gpu_rfft.py); sqrt(2) covers one frame of a pair of like magnitude


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
    import istft_ref as ir
    import stft_ref as st
    import tensor_fft_amd as tf

    assert torch.cuda.is_available(), "istft_bench needs a GPU: a time taken anywhere else says nothing"
    dev = torch.device("cuda:0")
    rows, frames = args.rows, args.frames
    total = rows * frames
    w_host = st.hann()
    window = torch.from_numpy(w_host.copy()).to(dev)
    gain_window = (window.float() * 4096).to(torch.float16)
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

    out = {"n": N, "rows": rows, "frames_per_signal": frames, "frames": total, "window": "hann (binary16)", "pad": 0, "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds, "shapes": {}}
    for hop in HOPS:
        length = N + (frames - 1) * hop
        x = (torch.rand((rows, length), generator=gen, device=dev) * 2 - 1).to(torch.float16)
        fwd = tf.TfftStftPlan(rows, length, hop, 0, 0)
        fwd.set_window(window)
        spec = torch.empty(total * 2 * PITCH, dtype=torch.float16, device=dev)
        fwd.exec(x.view(-1), spec, spec[PITCH:])
        torch.cuda.synchronize()
        fwd.close()
        del x

        plan = tf.TfftIstftPlan(rows, length, hop, 0, 0)
        assert plan.frames == frames and plan.kernels == ["istft4096::frames_kernel", "istft4096::ola_kernel"] and plan.num_launches == 2
        plan.set_window(window)
        ws = torch.empty(total * N, dtype=torch.float16, device=dev)
        plan.set_workspace(ws)
        assert total % 2 == 0, "frames_only cuts the frames into signals of two"
        fplan = tf.TfftIstftPlan(total // 2, 8, 8, N // 2, 0)
        assert fplan.frames == 2 and fplan.workspace_bytes() == plan.workspace_bytes()
        fplan.set_window(window)
        ws_f = torch.empty(total * N, dtype=torch.float16, device=dev)
        fplan.set_workspace(ws_f)
        y_f = torch.empty(total // 2 * 8, dtype=torch.float16, device=dev)
        rplan = tf.TfftRealPlan(N, total, 0)
        rplan.prepare()
        y = {k: torch.empty(rows * length, dtype=torch.float16, device=dev) for k in ("istft", "c2r_fold")}
        v = torch.empty(total * N, dtype=torch.float16, device=dev)
        env = torch.nn.functional.fold((window.float() ** 2).expand(1, frames, N).transpose(1, 2), (1, length), (1, N), stride=(1, hop)).view(length)
        env16 = torch.where(env > 0, env, torch.ones_like(env)).to(torch.float16)

        def ola_fold(u):
            return torch.nn.functional.fold(u.transpose(1, 2), (1, length), (1, N), stride=(1, hop)).view(rows, length)

        idx = ((torch.arange(frames, device=dev) * hop)[:, None] + torch.arange(N, device=dev)[None, :]).view(-1)

        def ola_index_add(u):
            return torch.zeros((rows, length), dtype=u.dtype, device=dev).index_add_(1, idx, u.reshape(rows, frames * N))

        ola, ola_name = ola_fold, "fold"
        try:
            ola(torch.zeros((rows, frames, N), dtype=torch.float16, device=dev))
            torch.cuda.synchronize()
        except Exception:
            ola, ola_name = ola_index_add, "index_add_"

        def run_fold():
            rplan.c2r(spec, spec[PITCH:], v)
            u = v.view(rows, frames, N) * gain_window
            torch.div(ola(u), env16, out=y["c2r_fold"].view(rows, length))

        cases = {"istft": lambda: plan.exec(spec, spec[PITCH:], y["istft"]), "frames_only": lambda: fplan.exec(spec, spec[PITCH:], y_f), "c2r_fold": run_fold,
                 "c2r_only": lambda: rplan.c2r(spec, spec[PITCH:], v)}
        torch_note = None
        try:
            s4 = spec.view(rows, frames, 2, PITCH)
            spec_c = torch.complex(s4[:, :, 0, :BINS].float(), s4[:, :, 1, :BINS].float()).transpose(1, 2).contiguous() * N
            w32 = window.float()
            ref = torch.istft(spec_c, N, hop_length=hop, window=w32, center=True)
            torch.cuda.synchronize()
            del ref
            cases["torch_istft"] = lambda: torch.istft(spec_c, N, hop_length=hop, window=w32, center=True)
        except Exception as e:       # recorded, not hidden: the case is context, not part of the comparison
            torch_note = f"{type(e).__name__}: {e}"[:300]

        # ---- checks before timing: four frames per signal of the workspace against fp64, signal 0's output against the numpy overlap-add
        for fn in cases.values():
            fn()
        torch.cuda.synchronize()
        pick = sorted({0, 1, frames // 2, frames - 1})
        s_host = spec.view(rows, frames, 2, PITCH)[:, pick].cpu().numpy().astype(np.float64)
        want = np.fft.irfft(s_host[:, :, 0, :BINS] + 1j * s_host[:, :, 1, :BINS], n=N, axis=-1) * N
        got = ws.view(rows, frames, N)[:, pick].cpu().numpy().astype(np.float64)
        rel = float(ir.rel_l2(got.reshape(-1, N), want.reshape(-1, N)).max())
        assert np.isfinite(got).all() and rel <= K_C2R * np.sqrt(2), f"hop {hop}: rel-L2 of a frame against fp64 {rel:.3e}"
        assert bool(torch.equal(ws.view(torch.int16), ws_f.view(torch.int16))), f"hop {hop}: frames_only does not compute the plan's frames"
        frames0 = ws.view(rows, frames, N)[0].cpu().numpy()
        same = bool(np.array_equal(ir.ola(frames0, w_host, 1, length, hop, 0).view(np.int16)[0], y["istft"][:length].cpu().numpy().view(np.int16)))
        assert same, f"hop {hop}: the output of signal 0 is not the overlap-add of its workspace frames"
        assert bool(torch.isfinite(y["istft"]).all())
        # (b) computes the same thing in another arithmetic (binary16 sums): the two agree to a few binary16 steps where the envelope is not small
        inner = slice(N, length - N)
        a_in = y["istft"].view(rows, length)[:, inner].float()
        dev_ab = float(((a_in - y["c2r_fold"].view(rows, length)[:, inner].float()).norm() / a_in.norm()).item())

        for _ in range(RAMP):
            cases["c2r_only"]()
        times = {k: [] for k in cases}
        for _ in range(args.rounds):
            for k, fn in cases.items():
                times[k].append(timed(fn))
        spec_b = 4 * BINS
        io = {"istft": total * (spec_b + 16384 + 2 * hop), "frames_only": total * (spec_b + 8192),
              "c2r_fold": total * (spec_b + 16384 + 8192 + 16384 + 8192 + 2 * hop + 4 * hop), "c2r_only": total * (spec_b + 16384 + 8192)}
        shape = {"hop": hop, "length": length, "overlap_add_of_b": ola_name,
                 "check": {"rel_l2_vs_fp64_worst_of_checked_frames": rel, "checked_frames_per_signal": len(pick),
                           "signal_0_equals_numpy_ola_bit_for_bit": same, "rel_l2_between_a_and_b_inner_samples": dev_ab}, "cases": {}}
        for k, ts in times.items():
            us = statistics.median(ts)
            shape["cases"][k] = {"us_per_call": round(us, 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
                                 "frames_per_us": round(total / us, 1)}
            if k in io:
                shape["cases"][k].update({"algorithmic_kib_per_frame": round(io[k] / total / 1024, 2), "algorithmic_gbytes_s": round(io[k] / us / 1e3, 1),
                                          "hbm_fraction": round(io[k] / us / 1e3 / HBM_PEAK_GBS, 3)})
        if torch_note:
            shape["torch_istft_refused"] = torch_note
        c = shape["cases"]
        # what ola_kernel adds, round by round (the cases alternate, so a round's two figures were taken next to each other)
        added = [a - f for a, f in zip(times["istft"], times["frames_only"])]
        shape["ola_added_us"] = {"median": round(statistics.median(added), 1), "min": round(min(added), 1), "max": round(max(added), 1)}
        shape["frames_only_over_c2r_only"] = round(c["frames_only"]["us_per_call"] / c["c2r_only"]["us_per_call"], 3)
        shape["frames_only_over_c2r_only_range"] = [round(c["frames_only"]["min_us"] / c["c2r_only"]["max_us"], 3),
                                                    round(c["frames_only"]["max_us"] / c["c2r_only"]["min_us"], 3)]
        for other in ("c2r_fold", "c2r_only"):
            shape["istft_over_" + other] = round(c["istft"]["us_per_call"] / c[other]["us_per_call"], 3)
            # the ratios at the ends of the two ranges
            shape["istft_over_" + other + "_range"] = [round(c["istft"]["min_us"] / c[other]["max_us"], 3), round(c["istft"]["max_us"] / c[other]["min_us"], 3)]
            shape["istft_faster_than_" + other + "_ranges_apart"] = bool(c["istft"]["max_us"] < c[other]["min_us"])
        out["shapes"]["hop_%d" % hop] = shape
        plan.close()
        fplan.close()
        rplan.close()
        spec_c = w32 = None
        del spec, ws, ws_f, y_f, v, y, cases, env, env16, idx
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
