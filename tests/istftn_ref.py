"""numpy restatement of the arithmetic of the short-frame ISTFT plans (include/tfft_istftn.h, frame lengths 512, 1024 and 2048): the
merge with the gain n in front of the inverse transform, the windowed overlap-add in its fixed order, and the cases of
tests/test_gpu_istftn.py. Built on stftn_ref.py (geometry, framing, data) and rfft_ref.py (merge, pairing). No library, no GPU."""
import numpy as np

import rfft_ref
import stftn_ref as sn

LENGTHS = sn.LENGTHS


def cases(n):
    """(rows, length, hop, pad, launch_iters, window): the smallest shapes at which each index of the two kernels can go wrong"""
    return [
        (1, n, 8, 0, 0, "random"),                       # one frame, self-paired in a ragged group
        (1, n + 8, 8, 0, 0, "random"),                   # two frames one chunk apart
        (3, 3 * n // 2, n // 4, 0, 0, "random"),         # 9 frames: pairs straddle signals, the last one self-paired
        (2, 2 * n, n // 2, n // 2, 0, "hann"),           # F = 5, both ends trimmed
        (2, n, n // 8, n - 8, 0, "random"),              # F = 16, frame 0 gives 8 samples
        (1, 8, 8, n // 2, 0, "random"),                  # L = 8, two frames
        (1, 3 * n, 2 * n, 0, 0, "random"),               # hop beyond a frame: n uncovered samples, +0
        (1, 3 * n // 2 + 8, n // 4, 0, 0, "random"),     # 8 tail samples that no frame reaches, +0
        (4, n + 320, 8, 0, 3, "random"),                 # 164 frames, waves loop; 41 frames under one sample
        sn.looping_case(n) + (sn.LOOP_ITERS, "random"),  # 93 / 45 / 21 frames: every live wave takes three groups, odd total, ragged last group
    ]


FRAMES_PER_SIGNAL = (1, 2, 3, 5, 16, 2, 2, 3, 41, None)      # of cases(n), whatever n (None: 31, 15, 7)


def huge_hop_cases(n):
    """one frame per signal and a hop that signed 64-bit arithmetic does not hold: 2^63, the largest below it whose sum with a sample
    position passes it, and the largest of all. The samples behind the frame are +0"""
    return [
        (3, 2 * n, 1 << 63, 0, 0, "random"),
        (1, 2 * n, (1 << 63) - 8, 0, 0, "random"),
        (2, 3 * n // 2, (1 << 64) - 8, n // 2, 0, "random"),
    ]


def accuracy_shapes(n):
    """(rows, length, hop, pad): Hann at hop n / 4 and pad n / 2, the envelope in [1.25, 1.5]"""
    return [(3, 2 * n, n // 4, n // 2), (4, 3 * n, n // 4, n // 2)]


def geometry(n, length, hop, pad=0):
    """F, the frames per signal; any hop beyond the padded signal is one frame (Python's integers carry 2^64 - 8)"""
    return sn.geometry(n, length, hop, pad)


def merge_gain(ar, ai, br, bi, n):
    """rfft_ref.merge with the factor float(n) in float32 in front of the one rounding: Z'[k] = fp16(n * (fp32 add)), on the edge
    bins fp16(n * fp32(A.re)), fp16(n * fp32(B.re)). Returns (zr, zi) float16, length n."""
    zr, zi = rfft_ref.merge(ar, ai, br, bi, n, dtype=np.float32, to16=False)
    gain = np.float32(n)
    with np.errstate(over="ignore"):
        return (gain * zr.astype(np.float32)).astype(np.float16), (gain * zi.astype(np.float32)).astype(np.float16)


def merge_items(re, im, n):
    """re, im [G][>= n / 2 + 1] float16 half spectra in the flat order g -> Z' (zr, zi), [ceil(G / 2)][n] float16: transform b from
    frames 2b and 2b + 1, the last frame of an odd total paired with itself"""
    a, b = rfft_ref.pair_rows(re.shape[0])
    k = sn.bins(n)
    return merge_gain(re[a, :k], im[a, :k], re[b, :k], im[b, :k], n)


def _spans(n, length, hop, pad):
    """(f, lo, j0, j1) of every frame that covers a sample of [0, L), f ascending"""
    for f in range(geometry(n, length, hop, pad)):
        lo = f * hop - pad
        j0, j1 = max(0, -lo), min(n, length - lo)
        if j1 > j0:
            yield f, lo, j0, j1


def ola(v, w, n, rows, length, hop, pad, raw=False):
    """v [R * F][n] frames in the order g, w [n] -> y [R][L]. float16 in: every product is exact in float32, the adds run in float32
    with f ascending from +0, y = fp16(num / den) where den > 0 and +0 where den = 0 (raw: fp16(num) everywhere), returned as
    float16. Any other dtype: the same sums in that dtype, not rounded."""
    v, w = np.asarray(v), np.asarray(w)
    half = v.dtype == np.float16
    acc = np.float32 if half else v.dtype.type
    frames = geometry(n, length, hop, pad)
    assert v.shape == (rows * frames, n) and w.shape == (n,)
    wf = w.astype(acc)
    vf = v.astype(acc).reshape(rows, frames, n)
    num = np.zeros((rows, length), acc)
    den = np.zeros((rows, length), acc)
    for f, lo, j0, j1 in _spans(n, length, hop, pad):    # ascending f: for every sample the adds run in the order of the frames that cover it
        sl = slice(lo + j0, lo + j1)
        num[:, sl] = num[:, sl] + wf[None, j0:j1] * vf[:, f, j0:j1]
        den[:, sl] = den[:, sl] + (wf[j0:j1] * wf[j0:j1])[None, :]
    if raw:
        y = num
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            y = np.where(den > 0, num / np.where(den > 0, den, acc(1)), acc(0))
    if not half:
        return y
    with np.errstate(over="ignore"):
        return y.astype(np.float16)


def envelope(w, n, length, hop, pad):
    """sum of w^2 over the frames that cover each sample, float64, [L]"""
    w2 = np.asarray(w, np.float64) ** 2
    den = np.zeros(length)
    for _, lo, j0, j1 in _spans(n, length, hop, pad):
        den[lo + j0:lo + j1] += w2[j0:j1]
    return den


def spectra16(x, w, hop, pad):
    """the inputs of the GPU cases: binary16 roundings of rfft / n of stftn_ref.frames(x, w), (re, im) [R * F][n / 2 + 1] float16"""
    n = w.shape[0]
    s = np.fft.rfft(sn.frames(x, w, hop, pad).astype(np.float64), axis=-1) / n
    return s.real.astype(np.float16), s.imag.astype(np.float16)


def istft64(re, im, w, rows, length, hop, pad):
    """fp64 ISTFT of binary16 spectra: irfft * n of every frame (numpy ignores the IM of bins 0 and n / 2), then ola in float64"""
    n = np.asarray(w).shape[0]
    k = sn.bins(n)
    s = re[:, :k].astype(np.float64) + 1j * im[:, :k].astype(np.float64)
    return ola(np.fft.irfft(s, n=n, axis=-1) * n, np.asarray(w, np.float64), n, rows, length, hop, pad)


def rel_l2(got, want):
    """per row: |got - want|_2 / |want|_2"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.sqrt(((got - want) ** 2).sum(-1) / (want ** 2).sum(-1))
