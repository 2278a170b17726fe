"""Test infrastructure of the carried convolution plans (include/tfft_cconv.h): the cases that tests/test_cconv_host.py and
tests/test_gpu_cconv.py share, the window builders of tests/sconv_ref.py and tests/bconv_ref.py with a history in front of x and a
future behind g, the concatenations that turn a carried execution into a whole-sequence execution of the shipped plans, and the
fp64 direct sums of the extended sequences.

No constant of its own: every numeric bound is K_SCONV, K_CONV_FUSED, A_SPECTRUM, the + 1 ulp / + 2^-11 allowance and dh_bound of
tests/sconv_ref.py and tests/bconv_ref.py. The kernels are the shipped ones with the load ends re-indexed, and the windows they
transform are windows the shipped plans transform on a longer sequence:

    forward        window s of the carried plan = segment s + 1 of the long plan at length hop + L on [zeros(hop - Hn) | hist | x]
                   (that sequence's sample hop is x[0], and hop - halo >= 0 puts segment 1 exactly halo in front of it)
    input gradient window s of the carried plan = segment s of the gradient plan at length L + Fn on [g | fut]
    tap gradient   item (p, s) = item (p, s + 1) of the gradient plan at length hop + L on [zeros(hop - Hn) | hist | x] and
                   [zeros(hop) | g]; the items (p, 0) there hold only zeros of g and add exact zeros
"""
import numpy as np

import bconv_ref as br
import lconv_ref as lr
import sconv_ref as sr

N = sr.N

# (L, K, B, C, context, launch_iters): the smallest shapes at which each thing can go wrong; the context is Hn and Fn alike
CASES = [
    (8, 1, 1, 1, 0, 0),           # halo 0: a context is refused, NULL runs
    (8, 9, 1, 1, 8, 0),           # chunk shorter than the halo; zeros in front of a short context
    (2048, 2049, 3, 3, 2048, 2),  # context = halo = hop; zero partner; waves loop
    (4104, 7, 3, 3, 8, 0),        # one block holds zeros, context and sequence
    (6152, 130, 3, 3, 136, 0),    # carry_min < halo = 192
    (4096, 2049, 3, 2, 1024, 0),  # context shorter than K - 1
    (8064, 65, 2, 3, 64, 0),      # L = 2 hop
    (12288, 65, 9, 3, 64, 4),     # four segments; waves loop
]


def carry_min(taps):
    """K - 1 rounded up to a multiple of 8: the smallest context that loses nothing"""
    return -(-(taps - 1) // 8) * 8


def context_signal(rows, channels, n, seed, which):
    """a history (which = 0) or a future (1) of n samples per sequence: uniform(-1, 1) binary16, independent of the case's x and g"""
    rng = np.random.default_rng([seed, n, rows, channels, 991 + which])
    return lr.signals(rows, channels, n, rng)


def extend(x, hist=None, fut=None):
    """[hist | x | fut] along the last axis"""
    parts = ([] if hist is None else [hist]) + [x] + ([] if fut is None else [fut])
    return np.concatenate(parts, axis=-1)


def front_padded(x, hist, taps):
    """[zeros(hop - Hn) | hist | x]: the sequence of hop + L samples whose segment s + 1 in the shipped plans is window s here"""
    hop = sr.geometry(x.shape[2], taps)[1]
    hn = 0 if hist is None else hist.shape[2]
    return extend(x, extend(np.zeros(x.shape[:2] + (hop - hn,), x.dtype), fut=hist))


def windows(x, taps, hist=None):
    """sr.windows with the history: the complex windows the carried forward plan (and pass (a) of its tap gradient) transforms,
    (re, im) each [items][4096]; samples [-Hn, 0) come from hist, zeros in front of that and at or behind L"""
    rows, channels, length = x.shape
    halo, hop, segs = sr.geometry(length, taps)
    pairs = (rows + 1) // 2
    hn = 0 if hist is None else hist.shape[2]
    assert hn <= halo and hn % 8 == 0
    planes = []
    for plane, hplane in zip(lr.pair_planes(x, length), lr.pair_planes(hist, hn) if hn else (None, None)):
        padded = np.zeros((pairs, channels, halo + (segs - 1) * hop + N), x.dtype)
        padded[:, :, halo:halo + length] = plane.reshape(pairs, channels, length)
        if hn:
            padded[:, :, halo - hn:halo] = hplane.reshape(pairs, channels, hn)
        w = np.stack([padded[:, :, s * hop:s * hop + N] for s in range(segs)], axis=1)       # [pairs][S][C][4096]
        planes.append(np.ascontiguousarray(w).reshape(pairs * segs * channels, N))
    return planes[0], planes[1]


def dx_windows(g, taps, fut=None):
    """br.dx_windows with the future: window s starts at sample s * hop of [g | fut | zeros]"""
    rows, channels, length = g.shape
    halo, hop, segs = sr.geometry(length, taps)
    pairs = (rows + 1) // 2
    fn = 0 if fut is None else fut.shape[2]
    assert fn <= halo and fn % 8 == 0
    planes = []
    for plane, fplane in zip(lr.pair_planes(g, length), lr.pair_planes(fut, fn) if fn else (None, None)):
        padded = np.zeros((pairs, channels, (segs - 1) * hop + N + fn), g.dtype)
        padded[:, :, :length] = plane.reshape(pairs, channels, length)
        if fn:
            padded[:, :, length:length + fn] = fplane.reshape(pairs, channels, fn)
        w = np.stack([padded[:, :, s * hop:s * hop + N] for s in range(segs)], axis=1)
        planes.append(np.ascontiguousarray(w).reshape(pairs * segs * channels, N))
    return planes[0], planes[1]


def dh_windows(x, g, taps, hist=None):
    """br.dh_windows with the history: (Zx, Zg), Zx the windows of [hist | x], Zg those of g with their first halo samples zero"""
    halo = sr.geometry(x.shape[2], taps)[0]
    x_re, x_im = windows(np.asarray(x).astype(np.float64), taps, None if hist is None else np.asarray(hist).astype(np.float64))
    g_re, g_im = sr.windows(np.asarray(g).astype(np.float64), taps)
    g_re[:, :halo] = 0
    g_im[:, :halo] = 0
    return x_re + 1j * x_im, g_re + 1j * g_im


def dh_items(x, g, taps, hist=None, rounded=False):
    """br.dh_items with the history: every item's full complex circular correlation, [items][4096] in fp64"""
    zx, zg = dh_windows(x, g, taps, hist)
    sx = br.half_spectrum(zx) * N if rounded else np.fft.fft(zx, axis=-1)
    return np.fft.ifft(np.conj(sx) * np.fft.fft(zg, axis=-1), axis=-1)


def _spec_of_taps(h):
    return np.fft.fft(np.asarray(h, np.float16).astype(np.float64), N, axis=-1)


def reference_taps(x, h, hist=None):
    """sr.reference_taps with the history: the circular convolution of every window with the binary16 taps in fp64, [items][4096];
    behind the halo it is the true linear convolution of [zeros | hist | x]"""
    f = lambda a: None if a is None else np.asarray(a, np.float16).astype(np.float64)
    re, im = windows(f(x), h.shape[1], f(hist))
    idx = np.arange(re.shape[0]) % x.shape[1]
    return np.fft.ifft(np.fft.fft(re + 1j * im, axis=-1) * _spec_of_taps(h)[idx], axis=-1)


def dx_reference_taps(g, h, fut=None):
    """br.dx_reference_taps with the future: the circular correlation of every window with the taps, [items][4096]; below hop it is
    the true anticausal correlation of [g | fut | zeros]"""
    f = lambda a: None if a is None else np.asarray(a, np.float16).astype(np.float64)
    re, im = dx_windows(f(g), h.shape[1], f(fut))
    idx = np.arange(re.shape[0]) % g.shape[1]
    return np.fft.ifft(np.fft.fft(re + 1j * im, axis=-1) * np.conj(_spec_of_taps(h))[idx], axis=-1)


# ---- the definitions of include/tfft_cconv.h by direct fp64 sums

def y_direct(x, h, hist=None):
    """y[t] = sum_j h[j] xe[t - j], t in [0, L): numpy.convolve on [hist | x], the first Hn outputs dropped"""
    xe = np.asarray(extend(x, hist), np.float64)
    h = np.asarray(h, np.float64)
    hn = 0 if hist is None else hist.shape[2]
    rows, channels, length = x.shape
    out = np.empty((rows, channels, length))
    for b in range(rows):
        for c in range(channels):
            out[b, c] = np.convolve(xe[b, c], h[c])[hn:hn + length]
    return out


def dx_direct(g, h, fut=None):
    """dx[t] = sum_j h[j] ge[t + j], t in [0, L): br.dx_direct on [g | fut], the last Fn outputs dropped"""
    return br.dx_direct(extend(g, fut=fut), h)[:, :, :g.shape[2]]


def dh_direct(x, g, taps, hist=None):
    """dh[c][j] = sum_b sum_{0 <= t < L} g[t] xe[t - j]: br.dh_direct on [hist | x] and [zeros(Hn) | g]"""
    hn = 0 if hist is None else hist.shape[2]
    return br.dh_direct(extend(x, hist), extend(g, np.zeros(g.shape[:2] + (hn,), g.dtype)), taps)


def dhist_direct(g, h, hn):
    """d loss / d hist[u] = sum_j h[j] g[u + j - Hn], u in [0, Hn): the first Hn samples of br.dx_direct on [zeros(Hn) | g]"""
    return br.dx_direct(extend(g, np.zeros(g.shape[:2] + (hn,), g.dtype)), h)[:, :, :hn]
