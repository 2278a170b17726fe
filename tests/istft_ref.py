"""numpy restatement of the arithmetic of the ISTFT plans (include/tfft_istft.h): the merge with gain in front of the inverse
transform, the windowed overlap-add in its fixed order, and the cases of tests/test_gpu_istft.py. No library, no GPU."""
import numpy as np

import rfft_ref
import stft_ref as st

N = st.N
BINS = st.BINS
PITCH = st.PITCH
GAIN = np.float32(4096.0)

# (rows, length, hop, pad, launch_iters, window): the smallest shapes at which each index of the two kernels can go wrong
CASES = [
    (1, 4096, 8, 0, 0, "random"),          # one frame, paired with itself
    (1, 4104, 8, 0, 0, "random"),          # two frames one chunk apart
    (3, 6144, 1024, 0, 0, "random"),       # 9 frames: pairs straddle signals, the last one is paired with itself
    (2, 8192, 2048, 2048, 0, "hann"),      # both ends trimmed, F = 5; the envelope stays in [0.5, 1]
    (2, 4096, 512, 4088, 0, "random"),     # frame 0 gives 8 samples
    (1, 8, 8, 2048, 0, "random"),          # L = 8, two frames
    (1, 12288, 8192, 0, 0, "random"),      # hop beyond a frame: 4096 uncovered samples, +0
    (1, 6152, 1024, 0, 0, "random"),       # 8 tail samples the last frame does not reach, +0
    (4, 4416, 8, 0, 3, "random"),          # 164 frames, every wave loops; up to 41 frames under one sample
    (5, 8192, 2048, 2048, 3, "random"),    # padding and looping together
]

# one frame per signal and a hop that signed 64-bit arithmetic does not hold: 2^63, the largest below it whose sum with a sample
# position passes it, and the largest of all. The samples behind the frame are +0
HUGE_HOP_CASES = [
    (3, 8192, 1 << 63, 0, 0, "random"),
    (1, 8192, (1 << 63) - 8, 0, 0, "random"),
    (2, 6144, (1 << 64) - 8, 2048, 0, "random"),
]


def merge_gain(ar, ai, br, bi, n=N):
    """rfft_ref.merge with the factor 4096 in float32 in front of the one rounding: Z'[k] = fp16(4096 * (fp32 add)), on the edge
    bins fp16(4096 * fp32(A.re)), fp16(4096 * fp32(B.re)). Returns (zr, zi) float16, length n."""
    zr, zi = rfft_ref.merge(ar, ai, br, bi, n, dtype=np.float32, to16=False)
    with np.errstate(over="ignore"):
        return (GAIN * zr.astype(np.float32)).astype(np.float16), (GAIN * zi.astype(np.float32)).astype(np.float16)


def merge_items(re, im):
    """re, im [G][>= 2049] float16 half spectra in the flat order g -> Z' (zr, zi), [ceil(G / 2)][4096] float16: item i from frames 2i
    and 2i + 1, the last frame of an odd total paired with itself"""
    a, b = rfft_ref.pair_rows(re.shape[0])
    return merge_gain(re[a, :BINS], im[a, :BINS], re[b, :BINS], im[b, :BINS])


def ola(v, w, rows, length, hop, pad, raw=False):
    """v [R * F][4096] frames in the order g, w [4096] -> y [R][L]. float16 in: every product is exact in float32, the adds run in
    float32 with f ascending from +0, y = fp16(num / den) where den > 0 and +0 where den = 0 (raw: fp16(num) everywhere), returned as
    float16. Any other dtype: the same sums in that dtype, not rounded."""
    v, w = np.asarray(v), np.asarray(w)
    half = v.dtype == np.float16
    acc = np.float32 if half else v.dtype.type
    frames = st.geometry(length, hop, pad)
    assert v.shape == (rows * frames, N) and w.shape == (N,)
    wf = w.astype(acc)
    vf = v.astype(acc).reshape(rows, frames, N)
    num = np.zeros((rows, length), acc)
    den = np.zeros((rows, length), acc)
    for f in range(frames):                      # ascending f: for every sample the adds run in the order of the frames that cover it
        lo = f * hop - pad
        j0, j1 = max(0, -lo), min(N, length - lo)
        if j1 <= j0:
            continue
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


def envelope(w, length, hop, pad):
    """sum of w^2 over the frames that cover each sample, float64, [L]"""
    frames = st.geometry(length, hop, pad)
    w2 = np.asarray(w, np.float64) ** 2
    den = np.zeros(length)
    for f in range(frames):
        lo = f * hop - pad
        j0, j1 = max(0, -lo), min(N, length - lo)
        if j1 > j0:
            den[lo + j0:lo + j1] += w2[j0:j1]
    return den


def spectra16(x, w, hop, pad):
    """the inputs of the GPU cases: binary16 roundings of rfft / 4096 of stft_ref.frames(x, w), (re, im) [R * F][2049] float16"""
    s = np.fft.rfft(st.frames(x, w, hop, pad).astype(np.float64), axis=-1) / N
    return s.real.astype(np.float16), s.imag.astype(np.float16)


def istft64(re, im, w, rows, length, hop, pad):
    """fp64 ISTFT of binary16 spectra: irfft * 4096 of every frame (numpy ignores the IM of bins 0 and 2048), then ola in float64"""
    s = re[:, :BINS].astype(np.float64) + 1j * im[:, :BINS].astype(np.float64)
    return ola(np.fft.irfft(s, n=N, axis=-1) * N, np.asarray(w, np.float64), rows, length, hop, pad)


def rel_l2(got, want):
    """per row: |got - want|_2 / |want|_2"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.sqrt(((got - want) ** 2).sum(-1) / (want ** 2).sum(-1))
