"""Test infrastructure of the FFT convolution plans (include/tfft_conv.h): the numpy restatement of the pointwise kernel, the fp64
reference, the filters and cases that the GPU tests and tools/conv_accuracy.py share, and the accuracy constants of the two paths.

Accuracy constants, in binary16 ulps of the largest |y| of each signal. The rule is that of tests/elementwise_bound.py:
tools/conv_accuracy.py writes the worst error of each class over CASES, the five filter kinds and three seeds to
profiles/conv_ulps.txt, and K = the smallest half-integer >= 1.5 x the worst value of the class, at most 4 (the ceiling K_REAL sits at
for the same reason: an inverse transform spreads the spectrum's rounding over samples whose peak is only 2 to 3 x their rms).

    K_CONV_FUSED     the one-pass N = 4096 kernel (the filtered spectrum is rounded once): class worst 2.102 ulp (batch 1029, one
                     filter, gauss), rel-L2 6.4e-4; 1.5 x 2.102 = 3.15 -> 3.5
    K_CONV_COMPOSED  forward plan, cmul, inverse plan (spectrum rounded, multiplied, rounded again): class worst 2.560 ulp (2^20), rel-L2
                     8.2e-4; 1.5 x 2.560 = 3.84 -> 4.0

Both hold unchanged at the upper edge of the range contract (profiles/range_ulps.txt, tests/test_gpu_conv_range.py: signals, filters
or both scaled until max |X H| lies within a factor 2 of 32752). They are constants for signals whose peak is 2 to 3 x their rms, as
the profile's are. One input outside that class is known: a REAL full-scale square wave of one period, +-65504 at every sample, times
H = 2^-14 comes back 4.000 ulp from the exact answer through conv4096's arithmetic (measured through sconv4096_kernel, which restates
it bit for bit and is held to K_SCONV = 4.0 there; tests/test_conv_range_host.py reproduces the 4.0 from the six roundings in numpy):
every sample is at the peak, the peak at the top of a binade, and the roundings of the one dominant tone add up.
"""
import numpy as np

K_CONV_FUSED = 3.5
K_CONV_COMPOSED = 4.0

FILTER_KINDS = ("ones", "delays", "gauss", "allpass", "decay")

# (n, batch, filters, composed): what tests/test_gpu_conv.py runs and tools/conv_accuracy.py measures
FUSED_CASES = [(4096, 1, 1, False), (4096, 37, 1, False), (4096, 37, 3, False), (4096, 37, 8, False),
               (4096, 1029, 1, False), (4096, 1029, 3, False), (4096, 1029, 8, False)]
COMPOSED_CASES = [(4096, 37, 3, True), (256, 21, 4, True), (2048, 9, 2, True), (8192, 5, 3, True), (1 << 16, 5, 2, True),
                  (1 << 20, 3, 2, True)]
CASES = FUSED_CASES + COMPOSED_CASES


def cmul(x_re, x_im, h_re, h_im, scale):
    """cmul_kernel (tensor-fft_amd/conv/cmul.hpp) in numpy: binary16 -> fp32, H times the power of two `scale`, one fma per component
    on an exactly representable inner product, then one conversion to binary16. The products of two binary16 values are exact in
    fp32 (11 x 11 bits, 22 bits each), so float64 holds x_re h_re - x_im h_im exactly, and astype(float32) is the fma's single
    rounding, as long as the two products lie within 53 - 22 = 31 binades of each other: true of the spectra and filters the tests
    use (normal binary16 values of similar size). For a subnormal next to a large value the float64 sum itself rounds, and the
    restatement may then differ from the kernel in the last bit: the bit-for-bit tests hold under that condition only."""
    xr, xi = np.asarray(x_re, np.float16).astype(np.float64), np.asarray(x_im, np.float16).astype(np.float64)
    hr = np.asarray(h_re, np.float16).astype(np.float64) * float(scale)
    hi = np.asarray(h_im, np.float16).astype(np.float64) * float(scale)
    with np.errstate(over="ignore"):
        z_re = (xr * hr - xi * hi).astype(np.float32).astype(np.float16)
        z_im = (xr * hi + xi * hr).astype(np.float32).astype(np.float16)
    return z_re, z_im


def make_filters(kind, n, filters, rng):
    """[filters][n] complex128 spectra, natural bin order, max |H| <= 1. delays: filter f is a circular delay by delay_shift(f, n)."""
    k = np.arange(n)
    f = np.minimum(k, n - k)
    out = np.empty((filters, n), dtype=np.complex128)
    for c in range(filters):
        if kind == "ones":
            out[c] = 1.0
        elif kind == "delays":
            out[c] = np.exp(-2j * np.pi * ((k * delay_shift(c, n)) % n) / n)
        elif kind == "gauss":
            out[c] = np.exp(-(f / (n * (0.05 + 0.03 * c))) ** 2)
        elif kind == "allpass":
            out[c] = np.exp(2j * np.pi * rng.uniform(size=n))
        elif kind == "decay":
            h = np.exp(-np.arange(n) / (n / 64.0)) * rng.standard_normal(n)
            spec = np.fft.fft(h)
            out[c] = spec / np.abs(spec).max()
        else:
            raise ValueError(kind)
    return out


def delay_shift(c, n):
    """a different shift for every channel"""
    return (5 + 37 * c) % n


def to_half_planes(spec):
    """the binary16 planes the plan is given"""
    return spec.real.astype(np.float16), spec.imag.astype(np.float16)


def reference(x_re, x_im, h_re, h_im, index=None):
    """fp64 ifft(fft(x_b) * H_(b mod filters)); x: [batch][n] binary16, h: [filters][n] binary16 (what the plan was given). index:
    the filter of each row, for rows sampled out of a batch."""
    x = np.asarray(x_re, np.float16).astype(np.float64) + 1j * np.asarray(x_im, np.float16).astype(np.float64)
    h = np.asarray(h_re, np.float16).astype(np.float64) + 1j * np.asarray(h_im, np.float16).astype(np.float64)
    idx = np.arange(x.shape[0]) % h.shape[0] if index is None else np.asarray(index)
    y = np.fft.ifft(np.fft.fft(x, axis=-1) * h[idx], axis=-1)
    return y.real, y.imag


def signals(n, batch, rng):
    """uniform(-1, 1) binary16, different for every signal"""
    return rng.uniform(-1, 1, (batch, n)).astype(np.float16), rng.uniform(-1, 1, (batch, n)).astype(np.float16)


def case_data(n, batch, filters, kind, seed):
    """(x_re, x_im, h_re, h_im) of a case: the signals above and the binary16 planes of make_filters"""
    rng = np.random.default_rng([seed, n, batch, filters, FILTER_KINDS.index(kind)])
    x_re, x_im = signals(n, batch, rng)
    h_re, h_im = to_half_planes(make_filters(kind, n, filters, rng))
    return x_re, x_im, h_re, h_im
