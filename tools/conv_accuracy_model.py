#!/usr/bin/env python3
"""CPU model of the accuracy of the two FFT convolution paths at N = 4096 (no GPU): what the constants of tests/conv_ref.py were
expected to be before anything had run. Built from the binary16 restatement of the reference kernels in oracle/ (orc.ref_fft =
DFT(x) / N with binary16 intermediates): three seeds, six filters, 32 signals each, errors in binary16 ulps of the largest |y|.

  composed   spectrum X / N rounded to binary16, multiplied by H N, rounded again, inverse restatement on exchanged planes
  fused      exact forward transform, the filtered spectrum rounded ONCE, the same inverse

Expectation it gave: composed 1.6 - 3.05 ulp, rel-L2 <= 1.0e-3; one rounding 1.0 - 2.13 ulp, rel-L2 <= 7.0e-4; max |X H| < 200."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import orc  # noqa: E402

N = 4096


def ulp16(v):
    return 2.0 ** (np.floor(np.log2(np.maximum(v, 2.0 ** -14))) - 10)


def r16(a):
    return a.astype(np.float16)


def filters(rng):
    k = np.arange(N)
    f = np.minimum(k, N - k)
    out = {"ones": np.ones(N, complex), "delay5": np.exp(-2j * np.pi * k * 5 / N), "gauss_lp": np.exp(-(f / 300.0) ** 2).astype(complex),
           "randphase": np.exp(2j * np.pi * rng.uniform(size=N))}
    h = np.exp(-np.arange(N) / 64.0) * rng.standard_normal(N)
    spec = np.fft.fft(h)
    out["decay_real"] = spec / np.abs(spec).max()
    h = (rng.standard_normal(N) + 1j * rng.standard_normal(N)) * np.exp(-np.arange(N) / 200.0)
    spec = np.fft.fft(h)
    out["decay_cplx"] = spec / np.abs(spec).max()
    return out


def main():
    orc.build()
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        batch = 32
        xr, xi = r16(rng.uniform(-1, 1, (batch, N))), r16(rng.uniform(-1, 1, (batch, N)))
        x = xr.astype(float) + 1j * xi.astype(float)
        for name, spec in filters(rng).items():
            hh = r16(spec.real).astype(float) + 1j * r16(spec.imag).astype(float)      # the caller's binary16 filter
            want = np.fft.ifft(np.fft.fft(x, axis=-1) * hh, axis=-1)
            u = ulp16(np.abs(want).max(axis=1))[:, None]

            def through_inverse(img):
                yi, yr = orc.ref_fft(r16(img.imag), r16(img.real))                     # inverse = forward on exchanged planes
                y = yr.astype(float) + 1j * yi.astype(float)
                e = (np.maximum(np.abs(y.real - want.real), np.abs(y.imag - want.imag)) / u).max()
                return e, np.sqrt((np.abs(y - want) ** 2).sum() / (np.abs(want) ** 2).sum())

            ar, ai = orc.ref_fft(xr, xi)
            e_c, rel_c = through_inverse((ar.astype(float) + 1j * ai.astype(float)) * hh * N)
            exact = np.fft.fft(x, axis=-1) * hh
            e_f, rel_f = through_inverse(exact)
            print(f"{seed} {name}: composed {e_c:.2f} ulp rel {rel_c:.2e} | one rounding {e_f:.2f} ulp rel {rel_f:.2e} | max|X H| {np.abs(exact).max():.0f}")


if __name__ == "__main__":
    main()
