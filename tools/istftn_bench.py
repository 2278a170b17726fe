#!/usr/bin/env python3
"""The short-frame ISTFT plans against what a caller had to write before them, in one process and alternated (include/tfft_istftn.h).

    python tools/istftn_bench.py [--steps K] [--warmup W] [--rounds R] [--rows B] [--samples S] [--lengths 512,1024,2048] [--json FILE]

Per frame length n = 512, 1024, 2048: B = 128 real signals under a binary16 Hann window, pad 0, hop n / 4, and S = 2^29 frame-side
samples in all (B F n = S: F = 8192, 4096, 2048 frames per signal, L = n + (F - 1) n / 4). The spectra are what TfftShortStftPlan
writes for random signals. Each n with
  istft         (a) the ISTFT plan: frames_kernel<R> (one-pass C2R with the gain, into the workspace) and ola_kernel
  frames_only   (a') frames_kernel<R> alone, as nearly as the interface gives it: a second plan on the SAME spectra, frames and
                pairing, cut as B F / 2 signals of L = 8 with pad n / 2 and hop 8 (two frames each), so that its ola_kernel writes 8
                samples per signal and the rest of the execution is frames_kernel on all B F frames. (a) - (a') is recorded as what
                ola_kernel adds
  c2r_fold      (b) what a caller does today: TfftRealPlan(n, B F).c2r (merge pass + inverse plan: two launches), * (n * window),
                overlap-add with torch.nn.functional.fold (index_add_ where fold refuses binary16), / a precomputed envelope
  c2r_only      (c) TfftRealPlan.c2r alone: the floor of (b), and the comparison for frames_kernel
  torch_istft   (d) for context, torch.istft in float32 (another precision, another layout, center=True framing of the same frame
                count: torch refuses a Hann window with center=False, whose envelope is 0 at sample 0), if the installed torch runs it
Before anything is timed the plan's result on the benchmark shape is held to the path tests/test_gpu_istftn.py tests, in every bit:
the workspace frames of signal 0 against TfftPlan(n, F / 2).exec_inverse on tests/istftn_ref.merge_items of its spectra, the output of
signal 0 against tests/istftn_ref.ola of its frames, and the workspace of (a') against that of (a); four frames per signal are also
checked against fp64 irfft * n of the same binary16 spectra. Timing: the protocol of tools/istft_bench.py, i.e. RAMP untimed launches,
W warm-up steps, then K back-to-back executions between two device events on the launch stream; the cases run in turn, R rounds,
and the median round is reported with its range, every ratio with the ratios at the ends of the two ranges. Bytes are algorithmic,
per frame: (a) 4 (n / 2 + 1) in, 2 n out and 2 n in for the frames, 2 hop out; (a') 4 (n / 2 + 1) in, 2 n out; (b) 4 (n / 2 + 1) in, 2 n out
and in for Z (one complex spectrum of n per PAIR of frames), 2 n out, 2 n in and out for the product, 2 n in for the overlap-add, 2 hop
out, and 2 hop in and out for the division; (c) 4 (n / 2 + 1) in, 2 n out and in for Z, 2 n out; against 8 TB/s."""
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
    ap.add_argument("--samples", type=int, default=SAMPLES)
    ap.add_argument("--lengths", default="512,1024,2048")
    ap.add_argument("--json", default="")
    args = ap.parse_args()

    import torch

    import __graft_entry__ as g

    g.build()
    import istftn_ref as inr
    import stftn_ref as sn
    import tensor_fft_amd as tf

    assert torch.cuda.is_available(), "istftn_bench needs a GPU: a time taken anywhere else says nothing"
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

    out = {"rows": rows, "frame_side_samples": args.samples, "window": "hann (binary16)", "pad": 0, "hop": "n / 4", "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds, "shapes": {}}
    for n in [int(v) for v in args.lengths.split(",")]:
        bins, pitch, hop = sn.bins(n), sn.pitch(n), n // 4
        frames = args.samples // (rows * n)
        total = rows * frames
        assert frames >= 2 and frames % 2 == 0 and total * n == args.samples, "rows * frames * n must be the sample count, frames even"
        length = n + (frames - 1) * hop
        w_host = sn.hann(n)
        window = torch.from_numpy(w_host.copy()).to(dev)
        gain_window = (window.float() * n).to(torch.float16)
        x = (torch.rand((rows, length), generator=gen, device=dev) * 2 - 1).to(torch.float16)
        fwd = tf.TfftShortStftPlan(n, rows, length, hop, 0, 0)
        fwd.set_window(window)
        spec = torch.empty(total * 2 * pitch, dtype=torch.float16, device=dev)
        fwd.exec(x.view(-1), spec, spec[pitch:])
        torch.cuda.synchronize()
        fwd.close()
        del x

        plan = tf.TfftShortIstftPlan(n, rows, length, hop, 0, 0)
        assert plan.frames == frames and plan.kernels == [f"istft256r::frames_kernel<{n // 256}>", "olan::ola_kernel"] and plan.num_launches == 2
        plan.set_window(window)
        ws = torch.empty(total * n, dtype=torch.float16, device=dev)
        plan.set_workspace(ws)
        fplan = tf.TfftShortIstftPlan(n, total // 2, 8, 8, n // 2, 0)
        assert fplan.frames == 2 and fplan.workspace_bytes() == plan.workspace_bytes()
        fplan.set_window(window)
        ws_f = torch.empty(total * n, dtype=torch.float16, device=dev)
        fplan.set_workspace(ws_f)
        y_f = torch.empty(total // 2 * 8, dtype=torch.float16, device=dev)
        rplan = tf.TfftRealPlan(n, total, 0)
        rplan.prepare()
        y = {k: torch.empty(rows * length, dtype=torch.float16, device=dev) for k in ("istft", "c2r_fold")}
        v = torch.empty(total * n, dtype=torch.float16, device=dev)
        env = torch.nn.functional.fold((window.float() ** 2).expand(1, frames, n).transpose(1, 2), (1, length), (1, n), stride=(1, hop)).view(length)
        env16 = torch.where(env > 0, env, torch.ones_like(env)).to(torch.float16)

        def ola_fold(u):
            return torch.nn.functional.fold(u.transpose(1, 2), (1, length), (1, n), stride=(1, hop)).view(rows, length)

        idx = ((torch.arange(frames, device=dev) * hop)[:, None] + torch.arange(n, device=dev)[None, :]).view(-1)

        def ola_index_add(u):
            return torch.zeros((rows, length), dtype=u.dtype, device=dev).index_add_(1, idx, u.reshape(rows, frames * n))

        ola, ola_name = ola_fold, "fold"
        try:
            ola(torch.zeros((rows, frames, n), dtype=torch.float16, device=dev))
            torch.cuda.synchronize()
        except Exception:
            ola, ola_name = ola_index_add, "index_add_"

        def run_fold():
            rplan.c2r(spec, spec[pitch:], v)
            u = v.view(rows, frames, n) * gain_window
            torch.div(ola(u), env16, out=y["c2r_fold"].view(rows, length))

        cases = {"istft": lambda: plan.exec(spec, spec[pitch:], y["istft"]), "frames_only": lambda: fplan.exec(spec, spec[pitch:], y_f),
                 "c2r_fold": run_fold, "c2r_only": lambda: rplan.c2r(spec, spec[pitch:], v)}
        torch_note = None
        try:
            s4 = spec.view(rows, frames, 2, pitch)
            spec_c = torch.complex(s4[:, :, 0, :bins].float(), s4[:, :, 1, :bins].float()).transpose(1, 2).contiguous() * n
            w32 = window.float()
            ref = torch.istft(spec_c, n, hop_length=hop, window=w32, center=True)
            torch.cuda.synchronize()
            del ref
            cases["torch_istft"] = lambda: torch.istft(spec_c, n, hop_length=hop, window=w32, center=True)
        except Exception as e:       # recorded, not hidden: the case is context, not part of the comparison
            torch_note = f"{type(e).__name__}: {e}"[:300]

        # ---- checks before timing
        for fn in cases.values():
            fn()
        torch.cuda.synchronize()
        pick = sorted({0, 1, frames // 2, frames - 1})
        s_host = spec.view(rows, frames, 2, pitch)[:, pick].cpu().numpy().astype(np.float64)
        want = np.fft.irfft(s_host[:, :, 0, :bins] + 1j * s_host[:, :, 1, :bins], n=n, axis=-1) * n
        got = ws.view(rows, frames, n)[:, pick].cpu().numpy().astype(np.float64)
        rel = float(inr.rel_l2(got.reshape(-1, n), want.reshape(-1, n)).max())
        assert np.isfinite(got).all() and rel <= K_C2R * np.sqrt(2), f"n {n}: rel-L2 of a frame against fp64 {rel:.3e}"
        assert bool(torch.equal(ws.view(torch.int16), ws_f.view(torch.int16))), f"n {n}: frames_only does not compute the plan's frames"
        # the tested path on signal 0: merge on the host, the shipped inverse plan, the numpy overlap-add
        s0 = spec.view(rows, frames, 2, pitch)[0].cpu().numpy()
        zr, zi = inr.merge_items(np.ascontiguousarray(s0[:, 0, :bins]), np.ascontiguousarray(s0[:, 1, :bins]), n)
        iplan = tf.TfftPlan(n, frames // 2, 0)
        assert iplan.num_launches == 1 and "fft256r_kernel" in iplan.kernels[0]
        d_z = torch.from_numpy(np.ascontiguousarray(np.stack([zr, zi], axis=1)).reshape(-1)).to(dev)
        d_v = torch.zeros(frames * n, dtype=torch.float16, device=dev)
        iplan.exec_inverse(d_z, d_z[n:], d_v, d_v[n:])
        torch.cuda.synchronize()
        iplan.close()
        frames_same = bool(torch.equal(d_v.view(torch.int16), ws[:frames * n].view(torch.int16)))
        assert frames_same, f"n {n}: the workspace frames of signal 0 are not TfftPlan.exec_inverse of the merged spectra"
        frames0 = ws.view(rows, frames, n)[0].cpu().numpy()
        same = bool(np.array_equal(inr.ola(frames0, w_host, n, 1, length, hop, 0).view(np.int16)[0], y["istft"][:length].cpu().numpy().view(np.int16)))
        assert same, f"n {n}: the output of signal 0 is not the overlap-add of its workspace frames"
        assert bool(torch.isfinite(y["istft"]).all())
        del d_z, d_v
        # (b) computes the same thing in another arithmetic (binary16 sums, frames kept at x / n through the inverse stages)
        inner = slice(n, length - n)
        a_in = y["istft"].view(rows, length)[:, inner].float()
        dev_ab = float(((a_in - y["c2r_fold"].view(rows, length)[:, inner].float()).norm() / a_in.norm()).item())

        for _ in range(RAMP):
            cases["c2r_only"]()
        times = {k: [] for k in cases}
        for _ in range(args.rounds):
            for k, fn in cases.items():
                times[k].append(timed(fn))
        spec_b = 4 * bins
        io = {"istft": total * (spec_b + 4 * n + 2 * hop), "frames_only": total * (spec_b + 2 * n),
              "c2r_fold": total * (spec_b + 4 * n + 2 * n + 4 * n + 2 * n + 2 * hop + 4 * hop), "c2r_only": total * (spec_b + 4 * n + 2 * n)}
        shape = {"n": n, "hop": hop, "frames_per_signal": frames, "frames": total, "length": length, "overlap_add_of_b": ola_name,
                 "check": {"rel_l2_vs_fp64_worst_of_checked_frames": rel, "checked_frames_per_signal": len(pick),
                           "signal_0_frames_equal_exec_inverse_bit_for_bit": frames_same, "signal_0_equals_numpy_ola_bit_for_bit": same,
                           "rel_l2_between_a_and_b_inner_samples": dev_ab}, "cases": {}}
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
        shape["frames_only_faster_than_c2r_only_ranges_apart"] = bool(c["frames_only"]["max_us"] < c["c2r_only"]["min_us"])
        for other in ("c2r_fold", "c2r_only"):
            shape["istft_over_" + other] = round(c["istft"]["us_per_call"] / c[other]["us_per_call"], 3)
            # the ratios at the ends of the two ranges
            shape["istft_over_" + other + "_range"] = [round(c["istft"]["min_us"] / c[other]["max_us"], 3), round(c["istft"]["max_us"] / c[other]["min_us"], 3)]
            shape["istft_faster_than_" + other + "_ranges_apart"] = bool(c["istft"]["max_us"] < c[other]["min_us"])
        out["shapes"]["n_%d" % n] = shape
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
