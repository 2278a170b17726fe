"""Test infrastructure of the overlap-save causal convolution plans (include/tfft_sconv.h): the cases that tests/test_gpu_sconv.py
and tools/sconv_accuracy.py share, the geometry restated, the window builder and its inverse, the fp64 references (on the helpers of
tests/lconv_ref.py: the same signals, taps and pairing) and the accuracy constant.

A plan cuts every sequence into S = ceil(L / hop) segments; segment s transforms the 4096-sample window that starts at sample
s * hop - halo (zeros outside [0, L)) and keeps window samples [halo, halo + min(hop, L - s * hop)). Rows 2p and 2p + 1 of a
channel are the RE and IM plane of one complex window; item (p * S + s) * C + c.

K_SCONV, in binary16 ulps of the largest magnitude of a WINDOW's 4096-point circular convolution (the pair's complex signal, the
discarded halo included: the unit of tests/lconv_ref.py applied per window). The rule is that of tests/elementwise_bound.py:
tools/sconv_accuracy.py writes the worst error over the cases below, the five tap kinds and three seeds to profiles/sconv_ulps.txt,
against fp64 with the plan's own binary16 spectrum, and K = the smallest half-integer >= 1.5 x the worst value, at most 4.

    K_SCONV   sconv4096_kernel (conv4096_kernel's arithmetic bit for bit on full windows, tested). Measured on the MI355X
              (profiles/sconv_ulps.txt): over the windows of full pairs worst 2.100 ulp, the class of profiles/conv_ulps.txt (2.102)
              and profiles/lconv_ulps.txt (2.113), which would give 3.5. Over the windows of a ZERO PARTNER (the last row of an odd
              count: a real signal) worst 3.000 ulp (L 12288, K 65, 9 x 3, delta). That is the unit, not the arithmetic: a full window
              of one row of uniform(-1, 1) samples peaks at 1.0 or a step below it (the worst window: 1.0 less the rounding error of the
              fp64 reference's own FFT, which lands in the lower binade as well), so its ulp is 2^-11, where a full pair peaks in [1, 1.41) and
              has 2^-10; 3.000 x 2^-11 is 1.5 ulp of a pair. The causal plans' zero partners have half-empty windows and the
              convolution plans' profile has no real signal, so neither profile met it. 1.5 x 3.000 = 4.5 exceeds the ceiling, so
              K_SCONV is the ceiling, 4.0, as K_REAL is (tests/elementwise_bound.py); DESIGN.md 3.11.
              At the upper edge of the range contract the classes do not move (profiles/range_ulps.txt). One zero-partner input
              reaches the constant exactly: the lone row +-65504 of one period with the tap 2^-14, 4.000 ulp
              (tests/test_gpu_conv_range.py::test_corner_signal_overlap_save, explained there and modelled on the CPU).
              rel-L2 of the kept samples of a window: at most 6.5e-4 everywhere but box taps at K = 2049, 1.08e-3 to 1.69e-3 (seed 2;
              the running mean of 2049 samples, an output of about 1/45 of the input's size; profiles/lconv_ulps.txt shows the same
              taps at 1.08e-3 to 1.17e-3 on half-empty windows). The test's seed stays under elementwise_bound.REL_L2.

The comparison with the true linear convolution gets the allowance tests/test_gpu_lconv.py grants for the binary16 rounding of the
spectrum, + 1 ulp and + 2^-11 of rel-L2. tests/test_sconv_host.py measures on the CPU, for these cases' data, what that rounding
alone does (the spectrum is the n = 4096 spectrum of tfft_lconv_spectrum_host): at most 0.843 ulp of the window's peak and rel-L2
2.64e-4, with max |X H| = 185 of the range contract's 32752.
"""
import numpy as np

import lconv_ref as lr

K_SCONV = 4.0
N = 4096

# (L, K, B, C, launch_iters): the smallest shapes at which each thing can go wrong
CASES = [
    (8, 1, 1, 1, 0),             # one chunk, halo 0, zero partner
    (2056, 1, 2, 2, 0),          # first length the causal plans cannot fuse; one segment, no halo
    (2048, 2049, 3, 3, 2),       # one segment behind a full zero halo; launch_iters 2: a wave takes a full pair, then a zero partner
    (4104, 7, 3, 3, 0),          # halo 64, second segment of 9 chunks, odd B
    (4096, 2049, 3, 2, 0),       # two segments, halo = hop
    (8064, 65, 2, 3, 0),         # L = 2 hop exactly, no tail
    (6152, 130, 3, 3, 0),        # halo 192, hop 3904: blocks straddle both boundaries
    (8192, 2049, 5, 3, 3),       # four segments, waves loop
    (12288, 65, 9, 3, 4),        # four segments, waves loop
]
# (L, K) at which the indexing was checked against numpy.convolve when the contract was written
INDEX_CASES = [(8, 1), (2056, 1), (2048, 2049), (4096, 2049), (4104, 7), (4040, 65), (6152, 130), (8192, 2049), (12288, 65), (16384, 1)]


def geometry(length, taps):
    """tfft_sconv_geometry: (halo, hop, segments)"""
    halo = -(-(taps - 1) // 64) * 64
    hop = N - halo
    return halo, hop, -(-length // hop)


def items_of(rows, channels, length, taps):
    return (rows + 1) // 2 * geometry(length, taps)[2] * channels


def windows(x, taps):
    """[B][C][L] real -> the complex windows the plan transforms: (re, im), each [items][4096], item (p * S + s) * C + c holding
    samples s * hop - halo ... of row 2p in re and of row 2p + 1 (zeros where B is odd) in im; zeros outside [0, L)."""
    rows, channels, length = x.shape
    halo, hop, segs = geometry(length, taps)
    pairs = (rows + 1) // 2
    planes = []
    for plane in lr.pair_planes(x, length):                       # [pairs * C][L], item p * C + c
        padded = np.zeros((pairs, channels, halo + (segs - 1) * hop + N), x.dtype)
        padded[:, :, halo:halo + length] = plane.reshape(pairs, channels, length)
        w = np.stack([padded[:, :, s * hop:s * hop + N] for s in range(segs)], axis=1)       # [pairs][S][C][4096]
        planes.append(np.ascontiguousarray(w).reshape(pairs * segs * channels, N))
    return planes[0], planes[1]


def kept(plane, rows, channels, length, taps):
    """[items][4096] (a plane of windows, real or complex) -> [items][hop]: the samples behind the halo, zero where a segment
    reaches beyond sample L (nothing is stored there)"""
    halo, hop, segs = geometry(length, taps)
    pairs = (rows + 1) // 2
    out = np.array(plane[:, halo:halo + hop]).reshape(pairs, segs, channels, hop)
    for s in range(segs):
        out[:, s, :, max(0, min(hop, length - s * hop)):] = 0
    return out.reshape(pairs * segs * channels, hop)


def unwindow(re, im, rows, channels, length, taps):
    """the inverse of windows() on the kept samples: [items][4096] planes -> [B][C][L]"""
    halo, hop, segs = geometry(length, taps)
    pairs = (rows + 1) // 2

    def join(plane):
        w = np.asarray(plane)[:, halo:halo + hop].reshape(pairs, segs, channels, hop)
        return w.transpose(0, 2, 1, 3).reshape(pairs * channels, segs * hop)

    return lr.unpair(join(re), join(im), rows, channels, length)


def _convolve(x, taps, spec):
    """ifft(fft(window) * spec[c]) in fp64: the complex windows [items][4096], circular"""
    re, im = windows(np.asarray(x, np.float16).astype(np.float64), taps)
    idx = np.arange(re.shape[0]) % x.shape[1]
    return np.fft.ifft(np.fft.fft(re + 1j * im, axis=-1) * spec[idx], axis=-1)


def reference_spectrum(x, taps, h_re, h_im):
    """fp64 with the binary16 spectrum the plan built ([C][4096] planes): the complex windows [items][4096]"""
    return _convolve(x, taps, np.asarray(h_re, np.float16).astype(np.float64) + 1j * np.asarray(h_im, np.float16).astype(np.float64))


def reference_taps(x, h):
    """the circular convolution of every window with the binary16 taps, in fp64: [items][4096]; behind the halo it is the true linear
    convolution (K - 1 <= halo: nothing wraps into the kept samples)"""
    return _convolve(x, h.shape[1], np.fft.fft(np.asarray(h, np.float16).astype(np.float64), N, axis=-1))


def window_peak(y):
    """the unit of K_SCONV: the largest magnitude of each window's circular convolution"""
    return np.abs(y).max(axis=1)
