#!/usr/bin/env python3
"""The single-pass kernels N = 256 .. 4096 on every basis vector against the stage models of tests/stage_model.py: the source of
the constants of tests/test_gpu_basis_sweep.py, as tools/accuracy_per_kernel.py is the source of K_TABLE.

    python tools/basis_accuracy.py [--out profiles/basis_ulps.txt]

Impulses: x = 1024 delta_p in the RE and in the IM plane, every p, forward and exec_inverse, sequential scaling. Per N, direction
and plane: the share of the 2 N^2 output components that differ from the model at all, the worst |kernel - model| in
u = ulp16(1024 / N), and the worst error of the kernel and of the model against the exact (1024 / N) w_N^(+-p k) in u.
Scale modes: how many components of TFFT_SCALE_ONCE and of TFFT_SCALE_NONE / N differ from the sequential output (RE plane, forward).
Tones: x_t = h16(exp(+2 pi i f t / N)), every f, forward: the worst error against fp64 of the rounded input in binary16 ulps of
the largest bin (tests/elementwise_bound.py), and the largest bin other than f in the same unit. The last line is the constant
the project's rule makes of the tones' worst value (the smallest half-integer >= 1.5 x worst)."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "basis_ulps.txt"))
    ap.add_argument("--sizes", type=int, nargs="+", default=None)
    args = ap.parse_args()

    import torch

    import __graft_entry__ as g

    g.build()
    import basis_sweep as bs
    import elementwise_bound as eb
    import stage_model as sm
    import tensor_fft_amd as tf

    sizes = args.sizes or list(sm.SIZES)
    lines = ["# tools/basis_accuracy.py: the single-pass kernels on every basis vector against tests/stage_model.py",
             "# impulses x = 1024 delta_p, sequential scaling, u = ulp16(1024 / N); share = components that differ from the model / 2 N^2",
             "# N direction plane : share differing (components) | worst |kernel - model| (u) at (p, k, plane) | kernel against exact (u) | model against exact (u)"]
    share_worst = {}
    for n in sizes:
        for inverse in (False, True):
            for plane in bs.PLANES:
                got = bs.run(tf, torch, n, *bs.impulse_planes(n, plane), inverse=inverse)
                model = bs.impulse_model(n, plane, inverse)
                c = bs.compare(got, model, n)
                exact = sm.impulse_exact(n, bs.A if plane == "re" else 1j * bs.A, inverse)
                lines.append(f"{n} {'inverse' if inverse else 'forward'} {plane} : {c['share']:.3e} ({c['count']}) | {c['worst']:.3f} at {c['at']} | "
                             f"{bs.error_in_u(got, exact, n):.3f} | {bs.error_in_u(model, exact, n):.3f}")
                print(lines[-1], flush=True)
                share_worst[n] = max(share_worst.get(n, 0.0), c["share"])
                for row in bs.differing(got, model, n, 4):
                    print("    " + row, flush=True)
    lines.append("# N : the largest share over directions and planes")
    for n in sizes:
        lines.append(f"share {n} : {share_worst[n]:.3e}")
        print(lines[-1])
    lines.append("# scale modes, RE plane, forward: components that differ from the sequential output (of 2 N^2)")
    for n in sizes:
        re, im = bs.impulse_planes(n, "re")
        seq = bs.run(tf, torch, n, re, im)
        once = bs.run(tf, torch, n, re, im, scale="once")
        none = bs.run(tf, torch, n, re, im, scale="none")
        d_once = sum(int((a.view(np.uint16) != b.view(np.uint16)).sum()) for a, b in zip(once, seq))
        d_none = sum(int(((a.astype(np.float32) / n).astype(np.float16).view(np.uint16) != b.view(np.uint16)).sum()) for a, b in zip(none, seq))
        lines.append(f"modes {n} : once {d_once} | none / N {d_none}")
        print(lines[-1], flush=True)
    lines.append("# tones x_t = h16(exp(+2 pi i f t / N)), every f, forward, sequential: worst error against fp64 of the rounded input in ulps of the "
                 "largest bin (f of the worst) | largest bin other than f, same unit | the model's worst error")
    tone_worst = 0.0
    for n in sizes:
        re, im = bs.tone_planes(n)
        got = bs.run(tf, torch, n, re, im)
        ref = np.fft.fft(re.astype(np.float64) + 1j * im.astype(np.float64), axis=1) / n
        d = eb.errors_in_ulps(got[0], got[1], ref.real, ref.imag)
        f = int(np.argmax(d.max(axis=1)))
        mag = np.hypot(got[0].astype(np.float64), got[1].astype(np.float64))
        mag[np.arange(n), np.arange(n)] = 0.0
        other = float((mag.max(axis=1) / eb.ulp16(np.abs(ref).max(axis=1))).max())
        m = sm.forward(n, re, im)
        dm = float(eb.errors_in_ulps(m.real, m.imag, ref.real, ref.imag).max())
        lines.append(f"tone {n} : {float(d.max()):.3f} (f = {f}) | {other:.3f} | {dm:.3f}")
        print(lines[-1], flush=True)
        tone_worst = max(tone_worst, float(d.max()))
    k = math.ceil(1.5 * tone_worst * 2) / 2
    lines.append(f"class worst tones: {tone_worst:.3f} ulp -> K_TONE = {k}")
    print(lines[-1])
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
