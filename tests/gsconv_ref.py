"""Test infrastructure of the gated overlap-save causal convolution plans (include/tfft_gsconv.h): the cases and modes that
tests/test_gsconv_host.py, tests/test_gpu_gsconv.py and tools/gsconv_bench.py share, and the CPU restatement of the contract

    u = p (.) x  (one binary16 multiply)      z = h * u + d u  (overlap-save, the shipped arithmetic on the windows of u)
    y = g (.) z  (one binary16 multiply)

Nothing here is new data or a new constant: signals and taps are tests/lconv_ref.py's, gates, skips and modes tests/gconv_ref.py's,
shapes, windows and the accuracy constant K_SCONV tests/sconv_ref.py's (all imported read-only). The gated kernel restates the
shipped arithmetic between two exact-to-one-rounding multiplies, and the GPU test holds it to the shipped TfftConvPlan on host-built
windows of u bit for bit, which ties it to the class profiles/sconv_ulps.txt measured.

The pre gate is applied BEFORE the windows are cut, so a window's halo carries gated samples (the kernel indexes the gate by the
source sample); the post gate is applied AFTER the kept samples are joined (the kernel indexes it by the output sample). A kernel
that indexes either gate by the window sample is wrong wherever halo != 0, from segment 0 on for the post gate and from segment 1
on for the pre gate.

Bound with a post gate. The kernel's z lies within K ulp(peak) of the reference z' (peak: the largest magnitude of the window's
circular convolution, the unit of K_SCONV), and y = round16(g z). So |y - g z'| <= |g| K ulp(peak) + 1/2 ulp16(|y|): the first term
is the gate times the error in front of it, the second the gate's one rounding (round to nearest: at most half the spacing at the
exact product, which is at most the spacing at the rounded result y).
"""
import numpy as np

import elementwise_bound as eb
import gconv_ref as gr
import lconv_ref as lr
import sconv_ref as sr

K_SCONV = sr.K_SCONV
N = sr.N
CASES = sr.CASES
TAP_KINDS = gr.TAP_KINDS
GATE_MODES = gr.GATE_MODES
EVERY_CASE_MODE = "pre+post+skip"
# the cases that run all five modes: one chunk; one segment behind a full zero halo with looping waves; blocks that straddle both
# boundaries at halo 192; four segments with looping waves
ALL_MODE_CASES = [(8, 1, 1, 1, 0), (2048, 2049, 3, 3, 2), (6152, 130, 3, 3, 0), (8192, 2049, 5, 3, 3)]
assert all(c in CASES for c in ALL_MODE_CASES)


def modes_of(case):
    return list(GATE_MODES) if tuple(case) in ALL_MODE_CASES else [EVERY_CASE_MODE]


# (L, K, B, C, launch_iters, mode)
CASE_MODES = [tuple(c) + (m,) for c in CASES for m in modes_of(c)]

geometry = sr.geometry
case_data = gr.case_data
half_product = gr.half_product
gated_input = gr.gated_input
gated_output = gr.gated_output


def reference_true(u, h, skip):
    """the circular convolution of every window of u with the binary16 taps and skip, in fp64: the complex windows [items][4096];
    behind the halo it is the true h * u + d u (K - 1 <= halo: nothing wraps into the kept samples)"""
    return sr._convolve(u, h.shape[1], np.fft.fft(gr.taps_with_skip(h, skip), N, axis=-1))


def reference_spectrum(u, taps, h_re, h_im):
    """fp64 with the binary16 spectrum the plan built ([C][4096] planes): the complex windows [items][4096]"""
    return sr.reference_spectrum(u, taps, h_re, h_im)


def per_sample(per_window, rows, channels, length, taps):
    """one value per window [items] -> the value of the window that holds each sample: [B][C][L]"""
    full = np.repeat(np.asarray(per_window, np.float64)[:, None], N, axis=1)
    return sr.unwindow(full, full, rows, channels, length, taps)


def joined(windows, rows, channels, length, taps):
    """complex windows [items][4096] -> the kept samples joined: [B][C][L] fp64"""
    return sr.unwindow(windows.real, windows.imag, rows, channels, length, taps)


def post_gate_tolerance(y, g, k, peak, rows, channels, length, taps):
    """|g| k ulp(peak) + 1/2 ulp16(|y|) per sample (see the module's docstring): [B][C][L]"""
    return (np.abs(g.astype(np.float64)) * k * per_sample(eb.ulp16(peak), rows, channels, length, taps)
            + 0.5 * eb.ulp16(np.abs(y.astype(np.float64))))


def delay_expected(u, taps, skip, g, tap=None):
    """the exact answer of the delay kind: g (.) (shift(u) + d u) in fp64, [B][C][L]"""
    return gr.delay_expected(u, taps, skip, g, tap)


def model(x, h, p, g, skip):
    """the contract in numpy fp64, by the kernel's route: gate -> windows -> circular convolution -> un-window -> gate; x, p, g any
    real arrays [B][C][L] (p, g, skip may be None), h [C][K]"""
    rows, channels, length = x.shape
    taps = h.shape[1]
    u = x if p is None else p * x
    re, im = sr.windows(u, taps)
    hs = np.array(h, np.float64)
    if skip is not None:
        hs[:, 0] += skip
    y = np.fft.ifft(np.fft.fft(re + 1j * im, axis=-1) * np.fft.fft(hs, N, axis=-1)[np.arange(re.shape[0]) % channels], axis=-1)
    z = sr.unwindow(y.real, y.imag, rows, channels, length, taps)
    return z if g is None else g * z
