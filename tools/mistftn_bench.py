#!/usr/bin/env python3
"""The masked short-frame ISTFT plan against what a caller had to write before it, and the power spectrogram's gradient, in one
process and alternated (include/tfft_mistftn.h, tensor-fft_amd/stft_autograd.py).

    python tools/mistftn_bench.py [--steps K] [--warmup W] [--rounds R] [--rows B] [--samples S] [--json FILE]

B = 128 real signals under a binary16 Hann window, pad 0, hop n / 4, S = 2^29 frame-side samples (frames x n, the count of
tools/spec_bench.py), n = 512, 1024 and 2048, spectra of short_stft of uniform(-1, 1) signals, a per-frame mask uniform in [0, 1].
  masked         (a) the masked plan: the frames kernel reads 4 bytes of spectra and 2 of mask per bin
  mul_then_istft (b) what a caller does today: re * M and im * M in torch (two passes, into planes at the plan's own strides, nothing
                     allocated), then TfftShortIstftPlan
  istft          (c) TfftShortIstftPlan alone on the unmasked spectra
  grad_power     (d) the backward pass of differentiable_power_spectrogram (short_stft recomputed, the mask formed, one masked plan)
  grad_torch         for context: the backward pass of gain * |torch.stft(x.float())|^2 / n^2 through torch's float32 autograd
Before anything is timed, (a) is held to (b): they do not agree bit for bit, because (b) rounds the products to binary16, but each
lies within K sqrt(2 env_max / env_min) + 2^-11 = 2.81e-03 of the fp64 result (tests/test_gpu_mistftn.py), so per signal their
rel-L2 distance over the samples under full frames (n .. L - n, where the Hann envelope lies in [1.25, 1.5]) is held to twice that.
Timing: the protocol of tools/spec_bench.py, i.e. RAMP untimed launches, W warm-up steps, then K back-to-back executions between two
device events on the launch stream; the cases run in turn, R rounds, and the median round is reported with its range, every ratio
with the ratios at the ends of the two ranges. No ratio is fixed in advance. The byte counts say (a) < (b) with the ranges apart, and
(a) / (c) near (4 + 2) / 4 on the frames kernel's read side; whether the time follows is what this driver records, either way.
Bytes are algorithmic, per frame: the frames kernel of (c) 4 (n / 2 + 1) in, 2 n out, the overlap-add 2 n in, 2 hop out; (a) adds
2 (n / 2 + 1) in; (b) adds 8 (n / 2 + 1) + 4 (n / 2 + 1) in and 4 (n / 2 + 1) out; against 8 TB/s."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROWS, SAMPLES = 128, 1 << 29
LENGTHS = (512, 1024, 2048)
SEED = 42
RAMP = 20
HBM_PEAK_GBS = 8000.0
AGREE = 2 * (1.5e-3 * (2 * 1.5 / 1.25) ** 0.5 + 2.0 ** -11)


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

    assert torch.cuda.is_available(), "mistftn_bench needs a GPU: a time taken anywhere else says nothing"
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

    out = {"rows": rows, "frame_side_samples": args.samples, "window": "hann (binary16)", "pad": 0, "hop": "n / 4", "mask": "per frame, uniform [0, 1]",
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "agreement_bound": round(AGREE, 5), "shapes": {}, "findings": []}
    for n in LENGTHS:
        hop, bins, pitch = n // 4, sn.bins(n), sn.pitch(n)
        frames = args.samples // n // rows
        total = rows * frames
        length = n + (frames - 1) * hop
        window = torch.from_numpy(sn.hann(n)).to(dev)
        x = (torch.rand((rows, length), generator=gen, device=dev) * 2 - 1).to(torch.float16)
        re, im = tf.short_stft(x, window, hop, n)                                     # views of one [R, F, 2, h] buffer
        spectra = re.as_strided((total * 2 * pitch,), (1,), re.storage_offset())
        mask = tf.mask_buffer(rows, frames, n, dev)
        mask.copy_(torch.rand((rows, frames, bins), generator=gen, device=dev))
        mask_flat = mask.as_strided((total * pitch,), (1,), mask.storage_offset())
        held = torch.empty((rows, frames, 2, pitch), dtype=torch.float16, device=dev)   # the masked planes of (b)
        held_re, held_im, held_flat = held[:, :, 0, :bins], held[:, :, 1, :bins], held.view(-1)
        m_plan = tf.TfftMaskedIstftPlan(n, rows, length, hop)
        i_plan = tf.TfftShortIstftPlan(n, rows, length, hop)
        assert m_plan.frames == frames and m_plan.kernels == [f"mistft256r::frames_kernel<{n // 256}>", "olan::ola_kernel"]
        for plan in (m_plan, i_plan):
            plan.set_window(window)
            plan.prepare()
        y_a = torch.empty(rows * length, dtype=torch.float16, device=dev)
        y_b = torch.empty_like(y_a)

        def mul_then_istft():
            torch.mul(re, mask, out=held_re)
            torch.mul(im, mask, out=held_im)
            i_plan.exec(held_flat, held_flat[pitch:], y_b)

        # (d): one forward each, then the backward passes alone
        xg = x.clone().requires_grad_(True)
        p = tf.differentiable_power_spectrogram(xg, window, hop, n)
        g_p = torch.rand(p.shape, generator=gen, device=dev) * 2 - 1
        x32 = x.float().requires_grad_(True)
        w32 = window.float()
        try:
            p32 = (torch.stft(x32, n, hop_length=hop, window=w32, center=False, return_complex=True).abs() ** 2 / (n * n)).transpose(1, 2)
        except RuntimeError as e:         # the context figure needs torch's own FFT back end; its absence is recorded, not hidden
            p32 = None
            out["findings"].append(f"n {n}: torch.stft is not available here ({str(e).splitlines()[0]}): grad_torch was not measured")
        cases = {"masked": lambda: m_plan.exec(spectra, spectra[pitch:], mask_flat, y_a), "mul_then_istft": mul_then_istft,
                 "istft": lambda: i_plan.exec(spectra, spectra[pitch:], y_b),
                 "grad_power": lambda: torch.autograd.grad(p, xg, g_p, retain_graph=True),
                 "grad_torch": lambda: torch.autograd.grad(p32, x32, g_p, retain_graph=True)}
        if p32 is None:
            del cases["grad_torch"]

        # ---- checks before timing: (a) against (b) under full frames, and the two gradients against each other
        cases["masked"]()
        mul_then_istft()
        torch.cuda.synchronize()
        a, b = (y.view(rows, length)[:, n:length - n].double() for y in (y_a, y_b))
        agree = float(((a - b).pow(2).sum(-1) / b.pow(2).sum(-1)).sqrt().max())
        assert agree <= AGREE, f"n {n}: the masked plan and re * M, im * M -> TfftShortIstftPlan differ by rel-L2 {agree:.2e} (bound {AGREE:.2e})"
        same_bits = bool(torch.equal(y_a.view(torch.int16), y_b.view(torch.int16)))
        grad_agree = float("nan")
        if p32 is not None:
            ga, gb = cases["grad_power"]()[0].double(), cases["grad_torch"]()[0].double()
            grad_agree = float(((ga - gb).pow(2).sum(-1) / gb.pow(2).sum(-1)).sqrt().max())
            del ga, gb
        del a, b

        for _ in range(RAMP):
            cases["masked"]()
        times = {k: [] for k in cases}
        for _ in range(args.rounds):
            for k, fn in cases.items():
                times[k].append(timed(fn))
        base = total * (4 * bins + 2 * n + 2 * n + 2 * hop)
        io = {"istft": base, "masked": base + total * 2 * bins, "mul_then_istft": base + total * 16 * bins}
        shape = {"n": n, "hop": hop, "length": length, "frames_per_signal": frames, "frames": total,
                 "check": {"masked_against_mul_then_istft_worst_signal_rel_l2": float(f"{agree:.3e}"), "bit_for_bit": same_bits,
                           "grad_power_against_grad_torch_worst_signal_rel_l2": float(f"{grad_agree:.3e}")}, "cases": {}}
        for k, ts in times.items():
            us = statistics.median(ts)
            shape["cases"][k] = {"us_per_call": round(us, 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1), "frames_per_us": round(total / us, 1)}
            if k in io:
                shape["cases"][k].update({"algorithmic_bytes_per_frame": io[k] // total, "algorithmic_gbytes_s": round(io[k] / us / 1e3, 1),
                                          "hbm_fraction": round(io[k] / us / 1e3 / HBM_PEAK_GBS, 3)})
        c = shape["cases"]
        for a, b in (("masked", "mul_then_istft"), ("masked", "istft")) + ((("grad_power", "grad_torch"),) if p32 is not None else ()):
            shape[f"{a}_over_{b}"] = round(c[a]["us_per_call"] / c[b]["us_per_call"], 3)
            shape[f"{a}_over_{b}_range"] = [round(c[a]["min_us"] / c[b]["max_us"], 3), round(c[a]["max_us"] / c[b]["min_us"], 3)]
            shape[f"{a}_faster_than_{b}_ranges_apart"] = bool(c[a]["max_us"] < c[b]["min_us"])
        shape["read_side_byte_ratio_masked_over_istft"] = 1.5
        if not shape["masked_faster_than_mul_then_istft_ranges_apart"]:
            out["findings"].append(f"n {n}: the byte counts say masked < mul_then_istft with the ranges apart; measured {c['masked']['us_per_call']} us "
                                   f"({c['masked']['min_us']}-{c['masked']['max_us']}) against {c['mul_then_istft']['us_per_call']} us "
                                   f"({c['mul_then_istft']['min_us']}-{c['mul_then_istft']['max_us']})")
        out["shapes"][f"n_{n}"] = shape
        m_plan.close()
        i_plan.close()
        del x, re, im, spectra, mask, mask_flat, held, held_re, held_im, held_flat, y_a, y_b, xg, p, g_p, x32, p32, cases
        tf.stftn_cache_clear()
        tf.spec_cache_clear()
        tf.mistftn_cache_clear()
        torch.cuda.empty_cache()
    out["not_measured"] = ["other hops", "padded plans (pad > 0)", "other row counts", "per-bin masks", "raw-sum plans on their own",
                           "masks outside [0, 1]", "the backward pass of differentiable_short_stft", "no PMC (hardware counter) run was made"]
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
