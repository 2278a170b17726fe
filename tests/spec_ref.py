"""numpy restatement of the spectrogram plans (include/tfft_spec.h): both modes in float32 on given binary16 half spectra (re, im),
the dense triangular mel filterbank in float64 from the published formulas (HTK and Slaney), the band sets and the shapes of
tests/test_gpu_spec.py, and the bound both modes are held to against fp64. No library, no GPU."""
import numpy as np

import stftn_ref as sn

LENGTHS = sn.LENGTHS
K_RFFT = 1.5e-3                    # the project's bound on a half spectrum of this arithmetic, rel-L2 against fp64 (tests/test_gpu_rfft.py)
# |P - P64| summed over a frame, relative to the frame's power: with a the fp64 spectrum and b the binary16 one,
# | |a|^2 - |b|^2 | <= |a - b| (|a| + |b|), Cauchy-Schwarz over the bins and |b|_2 <= (1 + eps) |a|_2 give eps (2 + eps); the two
# float32 roundings of a power (sum, gain) add 2 * 2^-24 relative to first order, 2^-22 with room for the second
POWER_BOUND = K_RFFT * (2 + K_RFFT) + 2.0 ** -22


# ---- the two modes, float32
def power(re, im, gain=1.0):
    """(re, im) binary16 [G, bins] -> P float32 [G, bins]: fp32(gain * fp32(re^2 + im^2)); the squares are exact in float32"""
    re, im = np.asarray(re), np.asarray(im)
    assert re.dtype == np.float16 and im.dtype == np.float16
    a, b = re.astype(np.float32), im.astype(np.float32)
    s = a * a + b * b
    out = np.float32(gain) * s
    assert s.dtype == np.float32 and out.dtype == np.float32
    return out


def band_energies(p, bands):
    """P float32 [G, bins], bands a list of (start, weights float32) -> [G, B] float32: acc = w[0] * P[start], then
    acc = acc + w[i] * P[start + i] in ascending i, every product and every sum rounded to float32 on its own"""
    p = np.asarray(p)
    assert p.dtype == np.float32
    out = np.empty((p.shape[0], len(bands)), np.float32)
    for j, (start, w) in enumerate(bands):
        w = np.asarray(w)
        assert w.dtype == np.float32 and w.size >= 1 and start + w.size <= p.shape[1]
        acc = w[0] * p[:, start]
        for i in range(1, w.size):
            acc = acc + w[i] * p[:, start + i]
        assert acc.dtype == np.float32
        out[:, j] = acc
    return out


def dense_of(bands, nbins):
    """the [B, bins] float32 matrix of a band list"""
    out = np.zeros((len(bands), nbins), np.float32)
    for j, (start, w) in enumerate(bands):
        out[j, start:start + len(w)] = w
    return out


def bands_of(dense):
    """a dense [B, bins] float32 matrix -> the band list: every row from its first to its last nonzero"""
    dense = np.asarray(dense, np.float32)
    out = []
    for row in dense:
        nz = np.flatnonzero(row)
        assert nz.size, "an empty band"
        out.append((int(nz[0]), row[nz[0]:nz[-1] + 1].copy()))
    return out


def arrays_of(bands):
    """(starts, counts, weights) as tfft_spec_plan_set_bands takes them"""
    return (np.array([s for s, _ in bands], np.uint32), np.array([len(w) for _, w in bands], np.uint32),
            np.concatenate([w for _, w in bands]).astype(np.float32))


# ---- the mel filterbank, float64
def hz_to_mel(f, scale):
    f = np.asarray(f, np.float64)
    if scale == "htk":                             # O'Shaughnessy: 2595 log10(1 + f / 700)
        return 2595.0 * np.log10(1.0 + f / 700.0)
    # Slaney's Auditory Toolbox: 200 / 3 Hz per mel below 1 kHz, 27 steps per factor 6.4 above
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), f / (200.0 / 3.0))


def mel_to_hz(m, scale):
    m = np.asarray(m, np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_dense(n_fft, sample_rate, n_mels, f_min=0.0, f_max=None, scale="htk", norm=None):
    """[n_mels, n_fft / 2 + 1] float64, filter by filter: n_mels + 2 edges equally spaced in mel; filter j is
    max(0, min((f - e[j]) / (e[j + 1] - e[j]), (e[j + 2] - f) / (e[j + 2] - e[j + 1]))) at f = k * sample_rate / n_fft, times
    2 / (e[j + 2] - e[j]) with norm = "slaney\""""
    f_max = sample_rate / 2.0 if f_max is None else float(f_max)
    edges = mel_to_hz(np.linspace(hz_to_mel(float(f_min), scale), hz_to_mel(f_max, scale), n_mels + 2), scale)
    freqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(sample_rate) / n_fft)
    out = np.zeros((n_mels, freqs.size))
    for j in range(n_mels):
        up = (freqs - edges[j]) / (edges[j + 1] - edges[j])
        down = (edges[j + 2] - freqs) / (edges[j + 2] - edges[j + 1])
        out[j] = np.maximum(0.0, np.minimum(up, down))
        if norm == "slaney":
            out[j] = out[j] * (2.0 / (edges[j + 2] - edges[j]))
    return out


MEL_CASES = [(512, 16000, 80, "htk", None), (1024, 22050, 128, "htk", None), (2048, 44100, 64, "slaney", "slaney")]


# ---- the cases of tests/test_gpu_spec.py
def shapes(n):
    """(rows, length, hop, pad, launch_iters)"""
    return [
        (3, 3 * n // 2, n // 4, 0, 0),           # three frames per signal, nine in all: the last self-paired, pairs straddle signals
        (4, 11 * n // 4, n // 4, 0, 0),          # 32 frames: an even total in full groups (the nine frames above end in a ragged group at every n)
        (2, n, 160, n // 2, 0),                  # centre padding, a hop that does not divide n, zeros at both ends
        (1, n, n, 0, 0),                         # one frame
        (5, 2 * n, n // 4, 0, 8),                # 25 frames, 13 transforms in 2, 4, 7 groups, all taken by ONE wave (conv_shape: grid 1, live 1)
    ]


ACCURACY_SHAPES = (0, 1)                         # pad 0: every frame is full and a pair's two frames have like magnitude
LOOP_SHAPE = 4


def band_sets(n):
    """name -> band list. Every weight is non-negative, so the fp64 bound of a band holds for all four."""
    nbins = sn.bins(n)
    rng = np.random.default_rng([n, 21])
    sets = {"mel80": bands_of(mel_dense(n, 16000, 80).astype(np.float32))}
    sets["all"] = [(0, rng.uniform(0, 1, nbins).astype(np.float32))]
    # bin n / 2 alone, bin 0 alone, and twelve bins across the boundary between the 256-bin segments 0 and 1 of the staged spectrum
    # (n = 512: bins 250 .. 256, out of the image and into bin n / 2, which lies apart)
    sets["edges"] = [(n // 2, np.array([0.75], np.float32)), (0, np.array([1.5], np.float32)),
                     (250, rng.uniform(0, 1, min(12, nbins - 250)).astype(np.float32))]
    # 37 bands of n / 16 + 3 bins, the first bins descending from high to low: neighbours overlap by more than half, the first one ends on bin n / 2
    count = n // 16 + 3
    starts = [(nbins - count) * (36 - j) // 36 for j in range(37)]
    sets["desc37"] = [(s, rng.uniform(0, 1, count).astype(np.float32)) for s in starts]
    return sets


def column_sum_max(bands, nbins):
    return float(dense_of(bands, nbins).astype(np.float64).sum(0).max())


def p64(n, x, w, hop, pad, gain=1.0):
    """gain * |rfft(u) / n|^2 in float64 on the binary16 products u = fp16(w * x): [G, bins]"""
    z = np.fft.rfft(sn.frames(x, w, hop, pad).astype(np.float64), axis=-1) / n
    return float(gain) * (z.real ** 2 + z.imag ** 2)


def band_bound(p_ref64, bands, nbins):
    """per frame, the bound on sum_j |E[j] - E64[j]| for non-negative weights: the power bound times the largest column sum of the
    bank (bin k's error enters band j with weight w[j][k]), plus count * 2^-24 of every band's energy for the count roundings a term
    of the sequential float32 sum can go through"""
    dense = dense_of(bands, nbins).astype(np.float64)
    assert (dense >= 0).all()
    e64 = p_ref64 @ dense.T
    counts = np.array([len(w) for _, w in bands], np.float64)
    return POWER_BOUND * p_ref64.sum(-1) * dense.sum(0).max() + (e64 * counts[None, :]).sum(-1) * 2.0 ** -24, e64
