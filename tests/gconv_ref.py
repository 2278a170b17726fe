"""Test infrastructure of the gated causal convolution plans (include/tfft_gconv.h): the gates, skip weights and cases that
tests/test_gconv_host.py, tests/test_gpu_gconv.py and tools/gconv_bench.py share, and the CPU restatement of the contract

    u = p (.) x  (one binary16 multiply)      z = h * u + d u  (the shipped arithmetic on u)      y = g (.) z  (one binary16 multiply)

Signals and taps are those of tests/lconv_ref.py (imported read-only), so are the accuracy constants K_LCONV_FUSED and
K_LCONV_COMPOSED: the gated kernels restate the shipped arithmetic between two exact-to-one-rounding multiplies, and the GPU tests
hold them to the shipped plans bit for bit, so no constant of their own is measured.

The skip weight is folded into tap 0 before the spectrum is rounded to binary16. With the gates and skips below max |U_k| |H'_k| = 222
over the cases x tap kinds x gate modes x seeds 1, 2, 3 (the skip-only mode, where |H'| reaches 1.5 and no gate shrinks the input;
the range contract of tfft_gconv.h holds with room to spare), and the binary16 rounding of H' alone moves the kept samples by at most
0.54 ulp of the pair's peak and rel-L2 2.2e-4. These three-seed figures come from a one-off sweep on the CPU that no test reproduces
(they differ from figures obtained with other gates: the gates are this file's own generator's);
tests/test_gconv_host.py::test_range_contract_and_spectrum_rounding recomputes the same quantities for seed 1 only and asserts the
allowances, not the figures: max |U H'| <= 32752 / 64, 1 ulp, rel-L2 2^-11. The method: fp64 with
gconv_spectrum_host's spectrum against fp64 with the taps and the skip (reference_spectrum against reference_true below), in ulps
of the largest magnitude of the pair's full fp64 convolution. That is inside the "+ 1 ulp, + 2^-11" tests/test_gpu_lconv.py already
grants for the rounding of the spectrum, which is what the comparison with the true result is allowed on top of K.
"""
import numpy as np

import lconv_ref as lr

K_LCONV_FUSED = lr.K_LCONV_FUSED
K_LCONV_COMPOSED = lr.K_LCONV_COMPOSED

TAP_KINDS = ("delay", "noise")

# mode -> (pre gate, post gate, skip)
GATE_MODES = {"pre": (True, False, False), "post": (False, True, False), "pre+post": (True, True, False), "skip": (False, False, True),
              "pre+post+skip": (True, True, True)}

# (L, K, B, C, launch_iters): the fused kernel at transform length 4096
FUSED_CASES = [
    (8, 1, 1, 1, 0),            # one chunk, zero partner
    (520, 7, 3, 3, 0),          # 65 chunks: one chunk into a swizzled partial block; odd B
    (2040, 2057, 3, 2, 0),      # L + K - 1 = 4096 exactly; last chunk of block 3 absent
    (2048, 2049, 3, 3, 2),      # grid 3: wave g takes item g (full pair), then g + 3 (zero partner): stale gate registers, or a plane
                                # that is not re-zeroed, show here
    (520, 7, 9, 3, 4),          # waves loop
]
# (n, L, K, B, C, composed flag): the generic path; the flag where the fused kernel would take the shape
COMPOSED_CASES = [
    (256, 96, 33, 5, 4, True),
    (4096, 2048, 2049, 3, 3, True),
    (8192, 4096, 4097, 3, 2, False),
]

fft_length = lr.fft_length
plan_length = lr.plan_length


def gates(rows, channels, length, seed):
    """(p, g): uniform(-1, 1) binary16, different for every sample, row and channel: [B][C][L] each"""
    rng = np.random.default_rng([seed, rows, channels, length, 0x6A7E])
    return (rng.uniform(-1, 1, (rows, channels, length)).astype(np.float16), rng.uniform(-1, 1, (rows, channels, length)).astype(np.float16))


def skip_values(channels):
    """skip[c] = (0.5 - 0.125 (c mod 4)) (-1)^c: exact in binary16"""
    c = np.arange(channels)
    d = ((0.5 - 0.125 * (c % 4)) * (-1.0) ** c).astype(np.float16)
    assert np.array_equal(d.astype(np.float64), (0.5 - 0.125 * (c % 4)) * (-1.0) ** c)
    return d


def half_product(a, b):
    """one IEEE binary16 multiply per sample: the fp32 product of two binary16 values is exact (22 bits), so its conversion is the
    one rounding (to nearest even, subnormals kept)"""
    return (np.asarray(a, np.float16).astype(np.float32) * np.asarray(b, np.float16).astype(np.float32)).astype(np.float16)


def case_data(length, taps, rows, channels, kind, seed, mode):
    """(x, h, p or None, g or None, skip or None) of a case: x and h are lconv_ref.case_data's"""
    x, h = lr.case_data(length, taps, rows, channels, kind, seed)
    pre, post, skip = GATE_MODES[mode]
    p, g = gates(rows, channels, length, seed)
    return x, h, (p if pre else None), (g if post else None), (skip_values(channels) if skip else None)


def gated_input(x, p):
    return x if p is None else half_product(p, x)


def gated_output(z, g):
    return z if g is None else half_product(g, z)


def taps_with_skip(h, skip):
    """[C][K] fp64: the taps with the skip weight added to tap 0"""
    h = np.asarray(h, np.float16).astype(np.float64).copy()
    if skip is not None:
        h[:, 0] += np.asarray(skip, np.float16).astype(np.float64)
    return h


def reference_true(u, h, skip, n):
    """h * u + d u in fp64 with the binary16 taps and skip: the complex signals [items][n] of the pairs"""
    return lr._convolve(u, np.fft.fft(taps_with_skip(h, skip), n, axis=-1), n)


def delay_expected(u, h_channels_taps, skip, g, tap=None):
    """the exact answer of the delay kind: g (.) (shift(u) + d u) in fp64, [B][C][L]; tap: the value of the one tap of every channel
    [C], 1 where it is not given"""
    rows, channels, length = u.shape
    taps = h_channels_taps
    out = np.zeros(u.shape)
    for c in range(channels):
        d = lr.delay_shift(c, taps)
        if d < length:
            out[:, c, d:] = (1.0 if tap is None else float(tap[c])) * u[:, c, :length - d].astype(np.float64)
        if skip is not None:
            out[:, c] += float(skip[c]) * u[:, c].astype(np.float64)
    return out if g is None else g.astype(np.float64) * out
