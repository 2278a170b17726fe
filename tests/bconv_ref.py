"""Test infrastructure of the gradient plans of the overlap-save causal convolution (include/tfft_bconv.h): the cases that
tests/test_bconv_host.py, tests/test_gpu_bconv.py and tools/bconv_accuracy.py share, the window builders of both gradients and their
inverses, the fp64 references (direct sums and window arithmetic), the numpy emulation of the tap gradient, and its derived bound.
Built on tests/sconv_ref.py and tests/lconv_ref.py: the same geometry, signals, taps and pairing.

Input gradient, dx[b][c][t] = sum_{j < K, t + j < L} h[c][j] g[b][c][t + j]. Segment s is the 4096-sample window of g that starts at
sample s * hop (zeros at or beyond L), multiplied by conj(H); window samples [0, min(hop, L - s * hop)) are kept. The arithmetic is
sconv4096_kernel's, so the constant is K_SCONV of tests/sconv_ref.py in its unit (binary16 ulps of the largest magnitude of the
window's 4096-point circular result), and the comparison with the true correlation gets the same + 1 ulp for the spectrum's
rounding (|conj(H)| = |H|: what tests/test_sconv_host.py measures for H holds for its conjugate).

Tap gradient, dh[c][j] = sum_b sum_{t >= j} g[b][c][t] x[b][c][t - j]. Item (p, s) of channel c is
ifft(conj(fft(Zx)) fft(Zg)), Zx the forward plan's window of the x pair, Zg that of the g pair with its first halo samples zeroed;
its RE plane at lags 0 .. K - 1 is the item's share of dh[c]. The kernel computes the item DIVIDED BY 4096 with fp16(fft(Zx) / 4096)
as the filter of conv4096_kernel's arithmetic, so the bound of one item is that arithmetic's constant plus what the rounding of the
filter does, in binary16 ulps of the item's peak / 4096, scaled back by 4096:

    |dh[c][j] - fp64| <= sum over the items i of channel c of (K_CONV_FUSED + A_SPECTRUM) * ulp16(peak_i / 4096) * 4096

peak_i = the largest magnitude of item i's full complex 4096-point circular correlation (the unit of K_CONV_FUSED and K_SCONV).
K_CONV_FUSED = 3.5 (tests/conv_ref.py) is the constant of conv4096_kernel against fp64 WITH ITS OWN binary16 filter. A_SPECTRUM
is what the rounding of Zx / 4096 to binary16 alone moves an item's kept lags by, measured on the CPU by
tests/test_bconv_host.py over DH_CASES (fp64 with the rounded spectrum against fp64 with the exact one): at most 0.41 ulp of the
item's peak with the test's seed (0.43 over three seeds), rounded up to the next half-integer: 0.5. On the same data
max |G| |Zx / 4096| = 5.2 of the range contract's 32752. The fp32 additions of the items and partials contribute less than
n_items * 2^-24 relative to the sum of magnitudes, four orders below one binary16 ulp of one item, and are ignored.
Measured on the MI355X (tools/bconv_accuracy.py, profiles/bconv_ulps.txt, three seeds): dx in the 2.0 / 3.0 classes of
profiles/sconv_ulps.txt (full pairs / zero partner); dh at most 0.142 of this bound (L 2048, K 2049, 3 x 3), the emulation 0.039: the
bound adds the items' errors in magnitude at their peak, the errors add at random and most lags lie far below an item's peak.
The host test also checks that the numpy emulation (fp64 arithmetic, binary16 Zx spectrum) meets this bound on these inputs, so that
the GPU test cannot be passing on slack alone.
"""
import numpy as np

import lconv_ref as lr
import sconv_ref as sr

N = sr.N
K_CONV_FUSED = 3.5         # tests/conv_ref.py
A_SPECTRUM = 0.5           # see above; tests/test_bconv_host.py measures it

# (L, K, B, C, partials cap): the tap gradient's cases; 0 = the default P
DH_CASES = [
    (8, 1, 1, 1, 0),             # tap 0 only, zero partner
    (2056, 1, 2, 2, 0),          # first length past the fused plans
    (2048, 2049, 3, 3, 0),       # chunk 256, full zero halo
    (4104, 7, 3, 3, 0),          # second segment of 9 chunks
    (4096, 2049, 3, 2, 0),       # halo = hop
    (6152, 130, 3, 3, 0),        # blocks straddle both boundaries
    (8192, 2049, 5, 3, 1),       # a wave accumulates 12 items
    (8192, 2049, 5, 3, 2),       # ... and 6
    (12288, 65, 9, 3, 2),        # 20 items per channel in two partials
    (12288, 65, 9, 3, 0),        # ... and in 20
]


def partials_of(rows, channels, length, taps, cap=0):
    """P of tfft_bconv_geometry"""
    per_channel = (rows + 1) // 2 * sr.geometry(length, taps)[2]
    p = min(per_channel, -(-2048 // channels))
    return min(p, cap) if cap else p


def grad_signal(rows, channels, length, taps, seed):
    """g = d loss / d y for a case: uniform(-1, 1) binary16, independent of the case's x"""
    rng = np.random.default_rng([seed, length, taps, rows, channels, 77])
    return lr.signals(rows, channels, length, rng)


# ---- input gradient

def dx_windows(g, taps):
    """[B][C][L] real -> the complex windows dgrad_kernel transforms: (re, im), each [items][4096], item (p * S + s) * C + c holding
    samples s * hop ... of row 2p in re and of row 2p + 1 (zeros where B is odd) in im; zeros at or beyond L."""
    rows, channels, length = g.shape
    halo, hop, segs = sr.geometry(length, taps)
    pairs = (rows + 1) // 2
    planes = []
    for plane in lr.pair_planes(g, length):
        padded = np.zeros((pairs, channels, (segs - 1) * hop + N), g.dtype)
        padded[:, :, :length] = plane.reshape(pairs, channels, length)
        w = np.stack([padded[:, :, s * hop:s * hop + N] for s in range(segs)], axis=1)
        planes.append(np.ascontiguousarray(w).reshape(pairs * segs * channels, N))
    return planes[0], planes[1]


def dx_unwindow(re, im, rows, channels, length, taps):
    """the inverse of dx_windows() on the kept samples [0, hop): [items][4096] planes -> [B][C][L]"""
    halo, hop, segs = sr.geometry(length, taps)
    pairs = (rows + 1) // 2

    def join(plane):
        w = np.asarray(plane)[:, :hop].reshape(pairs, segs, channels, hop)
        return w.transpose(0, 2, 1, 3).reshape(pairs * channels, segs * hop)

    return lr.unpair(join(re), join(im), rows, channels, length)


def dx_kept(plane, rows, channels, length, taps):
    """[items][4096] -> [items][hop]: the kept samples, zero where a segment reaches beyond sample L"""
    halo, hop, segs = sr.geometry(length, taps)
    pairs = (rows + 1) // 2
    out = np.array(plane[:, :hop]).reshape(pairs, segs, channels, hop)
    for s in range(segs):
        out[:, s, :, max(0, min(hop, length - s * hop)):] = 0
    return out.reshape(pairs * segs * channels, hop)


def conj_spectrum(h_re, h_im):
    """conj(H) as the plan builds it: the sign of every non-zero imaginary part flipped, a zero stays +0"""
    h_im = np.asarray(h_im, np.float16)
    return np.asarray(h_re, np.float16), np.where(h_im == 0, np.float16(0), -h_im).astype(np.float16)


def _correlate_windows(g, taps, spec):
    re, im = dx_windows(np.asarray(g, np.float16).astype(np.float64), taps)
    idx = np.arange(re.shape[0]) % g.shape[1]
    return np.fft.ifft(np.fft.fft(re + 1j * im, axis=-1) * spec[idx], axis=-1)


def dx_reference_spectrum(g, taps, c_re, c_im):
    """fp64 with the binary16 conjugated spectrum ([C][4096] planes): the complex windows [items][4096]"""
    return _correlate_windows(g, taps, np.asarray(c_re, np.float16).astype(np.float64) + 1j * np.asarray(c_im, np.float16).astype(np.float64))


def dx_reference_taps(g, h):
    """the circular correlation of every window with the binary16 taps, in fp64: [items][4096]; below hop it is the true anticausal
    correlation"""
    return _correlate_windows(g, h.shape[1], np.conj(np.fft.fft(np.asarray(h, np.float16).astype(np.float64), N, axis=-1)))


def dx_direct(g, h):
    """dx by direct fp64 sums (numpy.convolve of the reversed sequence): [B][C][L]"""
    g, h = np.asarray(g, np.float64), np.asarray(h, np.float64)
    rows, channels, length = g.shape
    out = np.empty_like(g)
    for b in range(rows):
        for c in range(channels):
            out[b, c] = np.convolve(g[b, c, ::-1], h[c])[:length][::-1]
    return out


# ---- tap gradient

def dh_direct(x, g, taps):
    """dh by direct fp64 sums: [C][K]"""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    rows, channels, length = x.shape
    out = np.zeros((channels, taps))
    for c in range(channels):
        for j in range(min(taps, length)):
            out[c, j] = sum(np.dot(g[b, c, j:], x[b, c, :length - j]) for b in range(rows))
    return out


def dh_windows(x, g, taps):
    """(Zx, Zg): the complex windows of both pairs, [items][4096] each, item (p * S + s) * C + c; Zg with its first halo samples zero"""
    halo = sr.geometry(x.shape[2], taps)[0]
    x_re, x_im = sr.windows(np.asarray(x).astype(np.float64), taps)
    g_re, g_im = sr.windows(np.asarray(g).astype(np.float64), taps)
    g_re[:, :halo] = 0
    g_im[:, :halo] = 0
    return x_re + 1j * x_im, g_re + 1j * g_im


def half_spectrum(zx):
    """fp16(fft(Zx) / 4096), component by component, as complex128: what pass (a) of wgrad_kernel keeps (up to its own arithmetic)"""
    s = np.fft.fft(zx, axis=-1) / N
    return s.real.astype(np.float16).astype(np.float64) + 1j * s.imag.astype(np.float16).astype(np.float64)


def dh_items(x, g, taps, rounded=False):
    """every item's full complex circular correlation, [items][4096] in fp64 (NOT divided by 4096); rounded: with the binary16
    spectrum of Zx, the numpy emulation of the kernel"""
    zx, zg = dh_windows(x, g, taps)
    sx = half_spectrum(zx) * N if rounded else np.fft.fft(zx, axis=-1)
    return np.fft.ifft(np.conj(sx) * np.fft.fft(zg, axis=-1), axis=-1)


def item_unit(items):
    """the unit of one item's error: ulp16(peak / 4096) * 4096, peak the largest magnitude of its complex circular correlation"""
    import elementwise_bound as eb

    return eb.ulp16(np.abs(items).max(axis=1) / N) * N


def by_channel(per_item, channels):
    """[items, ...] with item (p * S + s) * C + c -> [C][items per channel, ...], in increasing i = p * S + s"""
    per_item = np.asarray(per_item)
    return np.moveaxis(per_item.reshape((-1, channels) + per_item.shape[1:]), 1, 0)


def dh_from_items(items, channels, taps):
    """[C][K]: the RE planes' lags 0 .. K - 1 summed over the items of every channel, fp64"""
    return by_channel(items.real[:, :taps], channels).sum(axis=1)


def dh_bound(items, channels):
    """[C]: the derived bound of every tap of a channel (see the module's text); items: the TRUE correlations of dh_items()"""
    return (K_CONV_FUSED + A_SPECTRUM) * by_channel(item_unit(items), channels).sum(axis=1)


def sum_in_plan_order(per_item, channels, partials):
    """[items][K] float32 values of the items (already divided by 4096) -> [C][K] float32: partial q adds the items i = q, q + P, ...
    of a channel in increasing i, the partials are added in increasing q, the sum is multiplied by 4096: wgrad_kernel and
    wreduce_kernel, addition by addition"""
    v = by_channel(np.asarray(per_item, np.float32), channels)            # [C][per_channel][K]
    out = np.zeros((channels, v.shape[2]), np.float32)
    for c in range(channels):
        total = None
        for q in range(partials):
            part = np.zeros(v.shape[2], np.float32)
            for i in range(q, v.shape[1], partials):
                part = (part + v[c, i]).astype(np.float32)
            total = part if total is None else (total + part).astype(np.float32)
        out[c] = total * np.float32(4096)
    return out
