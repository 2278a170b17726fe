"""Test infrastructure of the causal real convolution plans (include/tfft_lconv.h): the cases, signals and taps that
tests/test_gpu_lconv.py and tools/lconv_accuracy.py share, the fp64 references, the pairing of rows into complex signals, and the
accuracy constants of the two paths.

Accuracy constants, in binary16 ulps of the largest |y| of the PAIR's full linear convolution (rows 2p and 2p + 1 of a channel
travel as one complex signal y_2p + i y_2p+1 of n samples, of which L are kept; the unit is that signal's largest magnitude, the
unit of tests/conv_ref.py). The rule is that of tests/elementwise_bound.py: tools/lconv_accuracy.py writes the worst error of each
class over the cases below, the five tap kinds and three seeds to profiles/lconv_ulps.txt, against fp64 with the plan's own
binary16 spectrum, and K = the smallest half-integer >= 1.5 x the worst value of the class, at most 4.

    K_LCONV_FUSED     lconv4096_kernel (conv4096_kernel's arithmetic bit for bit, tested): class worst 2.113 ulp (L 2048, K 2049, 3 x 3,
                      launch_iters 2, delay), rel-L2 1.17e-3 (box, K 2049: the kept half of a running mean that is still filling
                      holds less energy than the discarded half, the error is spread evenly); 1.5 x 2.113 = 3.17 -> 3.5. The 2.102
                      of profiles/conv_ulps.txt within seed noise.
    K_LCONV_COMPOSED  pack, tfft_conv_plan, crop (bit for bit that plan on padded data, tested): class worst 2.113 ulp (the same case
                      under the flag, where the sub-plan is the fused kernel; 2.048 at 2^16, box), rel-L2 1.08e-3; -> 3.5. Below the
                      2.560 of profiles/conv_ulps.txt: no case here reaches that profile's 2^20.

With the taps below max |X H| <= 137 (on the CPU, over the cases x kinds x three seeds: the range contract of tfft_conv.h holds with
room to spare), and the binary16 rounding of H alone moves the kept samples by at most 0.66 ulp and rel-L2 3.4e-4 (the same sweep,
fp64 with tfft_lconv_spectrum_host's spectrum against fp64 with the taps): inside the "+ 1 ulp, + 2^-11" that tests/test_gpu_conv.py
derives for its delay filters, which is what the comparison with the true linear convolution is allowed on top of K.
"""
import numpy as np

K_LCONV_FUSED = 3.5
K_LCONV_COMPOSED = 3.5

TAP_KINDS = ("delta", "delay", "box", "decay", "noise")

# (L, K, B, C, launch_iters): L <= 2048 with L + K - 1 <= 4096, the fused kernel at transform length 4096
FUSED_CASES = [
    (8, 1, 1, 1, 0),            # one chunk, zero partner
    (520, 7, 3, 3, 0),          # 65 chunks: one chunk into a swizzled partial block; odd B
    (1024, 1025, 2, 3, 0),
    (2040, 2057, 3, 2, 0),      # L + K - 1 = 4096 exactly; last chunk of block 3 absent
    (2048, 2049, 5, 3, 0),
    (2048, 64, 37, 3, 3),       # waves loop three times
    (520, 7, 9, 3, 4),
    (2048, 2049, 3, 3, 2),      # grid 3: wave g takes item g (full pair), then g + 3 (zero partner): the IM plane must be re-zeroed
]
# (n, L, K, B, C, composed flag): the generic path; the flag where the fused kernel would take the shape
COMPOSED_CASES = [
    (256, 96, 33, 5, 4, True),
    (2048, 1000, 500, 3, 2, True),
    (4096, 2048, 2049, 3, 3, True),
    (8192, 4096, 4097, 3, 2, False),
    (1 << 16, 40000, 20000, 3, 2, False),    # transposed order inside the sub-plan
]


def fft_length(length, taps):
    """tfft_lconv_fft_length"""
    n = 256
    while n < length + taps - 1:
        n *= 2
    return n


def plan_length(length, taps, composed=False):
    """the transform length of a plan: 4096 where the fused kernel takes the shape"""
    return 4096 if length <= 2048 and length + taps - 1 <= 4096 and not composed else fft_length(length, taps)


def delay_shift(c, taps):
    """a different delay for every channel"""
    return (5 + 37 * c) % taps


def signals(rows, channels, length, rng):
    """uniform(-1, 1) binary16, different for every sequence: [B][C][L]"""
    return rng.uniform(-1, 1, (rows, channels, length)).astype(np.float16)


def make_taps(kind, channels, taps, rng):
    """[C][K] binary16. decay and noise are normalised to sum |h| = 1 (before the rounding to binary16)."""
    h = np.zeros((channels, taps))
    j = np.arange(taps)
    for c in range(channels):
        if kind == "delta":
            h[c, 0] = 1.0
        elif kind == "delay":
            h[c, delay_shift(c, taps)] = 1.0
        elif kind == "box":
            h[c] = 1.0 / taps
        elif kind == "decay":
            h[c] = np.exp(-j / (taps / (8.0 + 4.0 * c) + 1.0)) * rng.standard_normal(taps)
            h[c] /= np.abs(h[c]).sum()
        elif kind == "noise":
            h[c] = rng.standard_normal(taps)
            h[c] /= np.abs(h[c]).sum()
        else:
            raise ValueError(kind)
    return h.astype(np.float16)


def case_data(length, taps, rows, channels, kind, seed):
    rng = np.random.default_rng([seed, length, taps, rows, channels, TAP_KINDS.index(kind)])
    return signals(rows, channels, length, rng), make_taps(kind, channels, taps, rng)


def pair_planes(x, n):
    """[B][C][L] real -> the zero-padded complex signals the plan transforms: (re, im), each [items][n], item p * C + c holding
    row 2p in re and row 2p + 1 (zeros where B is odd) in im."""
    rows, channels, length = x.shape
    pairs = (rows + 1) // 2
    re = np.zeros((pairs, channels, n), x.dtype)
    im = np.zeros((pairs, channels, n), x.dtype)
    re[:, :, :length] = x[0::2]
    im[:rows // 2, :, :length] = x[1::2]
    return re.reshape(pairs * channels, n), im.reshape(pairs * channels, n)


def unpair(re, im, rows, channels, length):
    """the inverse of pair_planes on the kept samples: [items][>= L] planes -> [B][C][L]"""
    pairs = (rows + 1) // 2
    out = np.empty((rows, channels, length), re.dtype)
    out[0::2] = re.reshape(pairs, channels, -1)[:, :, :length]
    out[1::2] = im.reshape(pairs, channels, -1)[:rows // 2, :, :length]
    return out


def _convolve(x, spec, n):
    """ifft(fft(pair) * spec[c]) in fp64: the complex signals [items][n]"""
    re, im = pair_planes(np.asarray(x, np.float16).astype(np.float64), n)
    channels = x.shape[1]
    idx = np.arange(re.shape[0]) % channels
    return np.fft.ifft(np.fft.fft(re + 1j * im, axis=-1) * spec[idx], axis=-1)


def reference_spectrum(x, h_re, h_im, n):
    """fp64 with the binary16 spectrum the plan built ([C][n] planes): the complex signals [items][n]"""
    return _convolve(x, np.asarray(h_re, np.float16).astype(np.float64) + 1j * np.asarray(h_im, np.float16).astype(np.float64), n)


def reference_taps(x, h, n):
    """the true linear convolution with the binary16 taps, in fp64: the complex signals [items][n] (n >= L + K - 1: nothing wraps)"""
    return _convolve(x, np.fft.fft(np.asarray(h, np.float16).astype(np.float64), n, axis=-1), n)


def pair_peak(y):
    """the unit of the constants: the largest magnitude of each pair's full linear convolution"""
    return np.abs(y).max(axis=1)
