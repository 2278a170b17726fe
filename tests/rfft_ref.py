"""numpy restatement of the real-input split / merge arithmetic (tensor-fft_amd/csrc/rsplit.hpp), bit for bit in float32:
fp16 operands widened to float32, one IEEE add, an exact * 0.5 (split only), one round to nearest even to fp16. With a float64
spectrum (dtype=np.float64, to16=False) the same formulas are the exact algebra that tests compare with numpy.fft.rfft."""
import numpy as np


def split(zr, zi, dtype=np.float32, to16=True):
    """Z = DFT(a + i b) (last axis, length N) -> the half spectra (ar, ai, br, bi) of a and b, bins 0 .. N/2."""
    n = zr.shape[-1]
    k = np.arange(n // 2 + 1)
    m = (-k) % n
    xr, xi = zr[..., k].astype(dtype), zi[..., k].astype(dtype)
    yr, yi = zr[..., m].astype(dtype), zi[..., m].astype(dtype)
    half = dtype(0.5)
    out = (half * (xr + yr), half * (xi - yi), half * (xi + yi), half * (yr - xr))
    return tuple(o.astype(np.float16) for o in out) if to16 else out


def merge(ar, ai, br, bi, n, dtype=np.float32, to16=True):
    """Half spectra of a and b (bins 0 .. N/2) -> Z = DFT(a + i b), length N; the IM of bins 0 and N/2 is ignored."""
    k = np.arange(n)
    low = k <= n // 2
    src = np.where(low, k, n - k)
    Ar, Ai = ar[..., src].astype(dtype), ai[..., src].astype(dtype)
    Br, Bi = br[..., src].astype(dtype), bi[..., src].astype(dtype)
    zr = np.where(low, Ar - Bi, Ar + Bi)
    zi = np.where(low, Ai + Br, Br - Ai)
    edge = (k == 0) | (k == n // 2)
    zr = np.where(edge, Ar, zr)
    zi = np.where(edge, Br, zi)
    return (zr.astype(np.float16), zi.astype(np.float16)) if to16 else (zr, zi)


def pair_rows(batch):
    """(first, second) signal index of each complex transform: 2p, 2p + 1, the last one of an odd batch paired with itself."""
    pairs = (batch + 1) // 2
    a = 2 * np.arange(pairs)
    b = np.minimum(a + 1, batch - 1)
    return a, b
