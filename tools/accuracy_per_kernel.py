"""Worst error of every kernel instantiation, in binary16 ulps of the largest output bin, over the CASES of
tests/test_gpu_kernel_matrix.py and three seeds: the evidence behind the K values of tests/elementwise_bound.py.

A case's error (forward, in place and inverse runs) is charged to every kernel its plan launches; an instantiation's value is
the worst over the cases that launch it. Each case runs with K = 4 (the ceiling the K values may not exceed), so that a case
above the committed K is measured rather than stopped. Writes profiles/per_kernel_ulps.txt (or the path given).

    python tools/accuracy_per_kernel.py [out.txt]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SEEDS = (1, 2, 3)


def c2r_merge_isolation(tf, torch, eb, n=4096, batch=36, seed=1):
    """The N = 4096 C2R against the best a binary16 merged spectrum allows: (library C2R, merge done in fp64 and rounded to
    binary16 once, then the library's complex inverse), both in ulps of the signal pair's largest sample."""
    rng = np.random.default_rng([seed, n, batch, 2])                  # the input of test_gpu_kernel_matrix.run_real
    x = rng.uniform(-1, 1, (batch, n)).astype(np.float16)
    h = n // 2 + 1
    spec = np.fft.rfft(x.astype(np.float64), axis=1) / np.sqrt(n)
    x16 = spec.real.astype(np.float16).astype(np.float64) + 1j * spec.imag.astype(np.float16).astype(np.float64)
    want = np.fft.irfft(x16, n, axis=1)
    plan = tf.TfftRealPlan(n, batch, 0)
    pitch = plan.pitch
    s_host = np.zeros(batch * 2 * pitch, dtype=np.float16)
    for b in range(batch):
        s_host[b * 2 * pitch:b * 2 * pitch + h] = x16[b].real
        s_host[b * 2 * pitch + pitch:b * 2 * pitch + pitch + h] = x16[b].imag
    d_in = torch.from_numpy(s_host).cuda()
    y = torch.empty(batch * n, dtype=torch.float16, device="cuda")
    plan.c2r(d_in, d_in[pitch:], y)
    torch.cuda.synchronize()
    got = y.cpu().numpy().astype(np.float64).reshape(batch, n)
    z0 = np.zeros_like(got)
    e_lib = eb.errors_in_ulps(got, z0, want, z0, pairs=True).max()
    # the merged spectrum Z = A + iB of each pair, in fp64, rounded once
    full = np.concatenate([x16, np.conj(x16[:, -2:0:-1])], axis=1)
    z = full[0::2] + 1j * full[1::2]
    host = np.stack([z.real, z.imag], axis=1).astype(np.float16).reshape(-1)
    d_z = torch.from_numpy(host).cuda()
    out = torch.empty_like(d_z)
    cp = tf.TfftPlan(n, batch // 2, 0)
    cp.exec_inverse(d_z, d_z[n:], out, out[n:])
    torch.cuda.synchronize()
    o = out.cpu().numpy().astype(np.float64).reshape(batch // 2, 2, n)
    ideal = np.empty_like(got)
    ideal[0::2], ideal[1::2] = o[:, 0], o[:, 1]
    e_ideal = eb.errors_in_ulps(ideal, z0, want, z0, pairs=True).max()
    return float(e_lib), float(e_ideal)


def main():
    import torch

    import __graft_entry__ as g

    g.build()
    import elementwise_bound as eb
    import test_gpu_kernel_matrix as km
    import tensor_fft_amd as tf
    from oracle import orc

    orc.build()
    tf.device_check(0)
    eb.K_TABLE = eb.K_SINCOS = eb.K_REAL = 4.0
    per_kernel, per_class = {}, {}
    for c in km.CASES:
        for seed in SEEDS:
            res = km.run_case(tf, orc, torch, c, seed)
            cls = km.arithmetic_class(list(res), c)
            for k, w in res.items():
                if w >= per_kernel.get(k, (-1.0, ""))[0]:
                    per_kernel[k] = (w, c["id"])
                per_class[cls] = max(per_class.get(cls, 0.0), w)
        print(c["id"], "done", flush=True)
    iso = [c2r_merge_isolation(tf, torch, eb, seed=s) for s in SEEDS]
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "per_kernel_ulps.txt")
    with open(out, "w") as f:
        f.write("# tools/accuracy_per_kernel.py: worst max(|dRe|, |dIm|) per instantiation over tests/test_gpu_kernel_matrix.py CASES,\n")
        f.write(f"# seeds {SEEDS}, in binary16 ulps of the transform's largest bin (real-input plans: of the signal pair's). Columns:\n")
        f.write("# worst ulps, the case it came from, kernel. One MI355X.\n")
        for k in sorted(per_kernel):
            w, cid = per_kernel[k]
            f.write(f"{w:6.3f}  {cid:32s} {k}\n")
        for cls in ("table", "sincos", "real"):
            w = per_class.get(cls, 0.0)
            kk = min(4.0, max(0.5, -(-1.5 * w // 0.5) * 0.5))
            f.write(f"# class worst {cls:7s} {w:6.3f} ulp -> K = {kk:.1f} (smallest half-integer >= 1.5 x worst, at most 4)\n")
        f.write("# C2R of N = 4096 x 36, library against fp64 merge rounded once to binary16 + the library's complex inverse, worst "
                f"ulps per seed: {', '.join(f'{a:.3f} / {b:.3f}' for a, b in iso)}\n")
    print(open(out).read())


if __name__ == "__main__":
    main()
