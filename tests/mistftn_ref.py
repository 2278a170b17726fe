"""numpy restatement of the arithmetic of the masked short-frame ISTFT plans (include/tfft_mistftn.h, frame lengths 512, 1024 and
2048): the merge with a real binary16 mask inside its float32 sum and the gain n in front of the one rounding, per frame and per
bin; the exact adjoint of the short-frame STFT in float64; and the masks of tests/test_gpu_mistftn.py. Built on istftn_ref.py
(pairing, overlap-add, cases) and rfft_ref.py (pairing). No library, no GPU."""
import numpy as np

import istftn_ref as inr
import rfft_ref
import stftn_ref as sn

LENGTHS = inr.LENGTHS


def _sums(ma, mb, ar, ai, br, bi, n, dtype):
    """the sums of the masked merge in `dtype`, before the gain: (zr, zi), length n. Every operand [..., n / 2 + 1]. In float32 on
    binary16 operands each product is exact, so each sum is rounded once."""
    k = np.arange(n)
    low = k <= n // 2
    src = np.where(low, k, n - k)
    Ma, Mb = ma[..., src].astype(dtype), mb[..., src].astype(dtype)
    Ar, Ai = ar[..., src].astype(dtype), ai[..., src].astype(dtype)
    Br, Bi = br[..., src].astype(dtype), bi[..., src].astype(dtype)
    zr = np.where(low, Ma * Ar - Mb * Bi, Ma * Ar + Mb * Bi)
    zi = np.where(low, Ma * Ai + Mb * Br, Mb * Br - Ma * Ai)
    edge = (k == 0) | (k == n // 2)
    zr = np.where(edge, Ma * Ar, zr)
    zi = np.where(edge, Mb * Br, zi)
    return zr, zi


def merge_gain_masked(ma, mb, ar, ai, br, bi, n):
    """Z'[k] = fp16(n * fp32(mA A.re - mB B.im)) + i fp16(n * fp32(mA A.im + mB B.re)) on the low bins, the high bins from bin n - k
    with merge_high_gain's signs, the edges fp16(n * mA A.re) and fp16(n * mB B.re), in float32 exactly as include/tfft_mistftn.h
    states it. Every argument float16 [..., n / 2 + 1] (the masks broadcast). Returns (zr, zi) float16, length n."""
    for a in (ma, mb, ar, ai, br, bi):
        assert a.dtype == np.float16
    with np.errstate(over="ignore", invalid="ignore"):
        zr, zi = _sums(ma, mb, ar, ai, br, bi, n, np.float32)
        gain = np.float32(n)
        return (gain * zr).astype(np.float16), (gain * zi).astype(np.float16)


def merge_items_masked(re, im, mask, n):
    """re, im [G][>= n / 2 + 1] float16 half spectra in the flat order g; mask [G][>= n / 2 + 1] (per frame) or [>= n / 2 + 1] (per
    bin: one mask for every frame) -> Z' (zr, zi), [ceil(G / 2)][n] float16: transform b from frames 2b and 2b + 1 and their masks,
    the last frame of an odd total paired with itself, with its own mask for both"""
    a, b = rfft_ref.pair_rows(re.shape[0])
    k = sn.bins(n)
    if mask.ndim == 1:
        ma = mb = np.broadcast_to(mask[None, :k], (a.size, k))
    else:
        ma, mb = mask[a, :k], mask[b, :k]
    return merge_gain_masked(ma, mb, re[a, :k], im[a, :k], re[b, :k], im[b, :k], n)


def masked64(re, im, mask, n):
    """the masked spectra in float64, (re, im) [G][n / 2 + 1]: the reference of the accuracy tests"""
    k = sn.bins(n)
    m = mask[..., :k].astype(np.float64)
    return m * re[:, :k].astype(np.float64), m * im[:, :k].astype(np.float64)


def istft64_masked(re, im, mask, w, rows, length, hop, pad, raw=False):
    """fp64 ISTFT of the fp64-masked binary16 spectra: irfft * n of every frame, then the overlap-add in float64"""
    n = np.asarray(w).shape[0]
    mr, mi = masked64(re, im, mask, n)
    return inr.ola(np.fft.irfft(mr + 1j * mi, n=n, axis=-1) * n, np.asarray(w, np.float64), n, rows, length, hop, pad, raw=raw)


# ---- the adjoint of the short-frame STFT, float64
def stft64(x, w, hop, pad):
    """S [R * F][n / 2 + 1] complex128: rfft / n of the UNROUNDED products w * x of every frame"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n = w.shape[0]
    return np.fft.rfft(sn.windows(n, x, hop, pad) * w[None, :], axis=-1) / n


def adjoint_frames64(g_re, g_im, n):
    """du [G][n]: (1 / n) (G_0 + sum_{0 < k < n / 2} Re(G_k e^{+2 pi i k j / n}) + G_{n / 2} (-1)^j), the gradient of
    <S, G> = sum_k Re(S_k) g_re[k] + Im(S_k) g_im[k] with respect to the frame. The IM of bins 0 and n / 2 carries nothing. Written as
    the inverse transform of c_k G_k, c = 1 / n on the edge bins and 1 / (2 n) between (irfft * n is X_0 + X_{n / 2} (-1)^j + 2 sum Re)."""
    k = sn.bins(n)
    c = np.full(k, 1.0 / (2 * n))
    c[0] = c[n // 2] = 1.0 / n
    return np.fft.irfft(c[None, :] * (np.asarray(g_re, np.float64)[:, :k] + 1j * np.asarray(g_im, np.float64)[:, :k]), n=n, axis=-1) * n


def adjoint64(g_re, g_im, w, rows, length, hop, pad):
    """dx [R][L] float64: dx[t] = sum_f w[j] du_f[j], j = t + pad - f hop: the raw-sum overlap-add of adjoint_frames64"""
    w = np.asarray(w, np.float64)
    n = w.shape[0]
    return inr.ola(adjoint_frames64(g_re, g_im, n), w, n, rows, length, hop, pad, raw=True)


def inner_spectra(s, g_re, g_im):
    """<S, G> over real and imaginary parts"""
    return float((s.real * np.asarray(g_re, np.float64)).sum() + (s.imag * np.asarray(g_im, np.float64)).sum())


# ---- the masks of the tests
PLANTED = (0.0, 1.0, -0.5, 2.0 ** -20, 2.0)      # exact 0 and 1, a negative value, a binary16 subnormal, and a value beyond 1


def random_mask(shape, seed, planted=True):
    """uniform [0, 1] rounded to binary16; with `planted`, the PLANTED values stand at bins 5 .. 9 of every mask frame and, shifted by
    one so that a pair's two masks differ there, at the bins that end a chunk of 8 (bins 8 v + 7) of the odd frames. The edge bins 0
    and n / 2 stay random: a zero there would hide which frame's mask was read."""
    rng = np.random.default_rng([17, seed])
    m = rng.uniform(0, 1, shape).astype(np.float16)
    if planted:
        for i, v in enumerate(PLANTED):
            m[..., 5 + i] = np.float16(v)
        if m.ndim > 1:
            for i, v in enumerate(PLANTED):
                m[1::2, 8 * (i + 2) + 7] = np.float16(v)
    assert np.float16(2.0 ** -20) != 0 and np.float16(2.0 ** -20) < np.finfo(np.float16).tiny
    return m


def sign_mask(shape, seed):
    """a mask drawn from {0, +-1, +-2}: multiplying binary16 by it is exact (where the doubling does not overflow)"""
    rng = np.random.default_rng([19, seed])
    return rng.choice(np.array([0.0, 1.0, -1.0, 2.0, -2.0], np.float16), shape)
