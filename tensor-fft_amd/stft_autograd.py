"""Gradients of the short-frame STFT family (frame lengths 512, 1024 and 2048): torch.autograd hooks whose backward passes are
raw-sum masked ISTFT plans (mistftn.py, include/tfft_mistftn.h). No fallback of any kind: torch supplies memory, streams and the
autograd graph, nothing else.

The adjoint. short_stft maps the frames u = w * x to S_k = (1 / n) sum_j u[j] e^{-2 pi i k j / n}, k = 0 .. n / 2. For an incoming
gradient G = g_re + i g_im, d<S, G> / du[j] = (1 / n) (G_0 + sum_{0 < k < n / 2} Re(G_k e^{+2 pi i k j / n}) + G_{n / 2} (-1)^j); the IM
of bins 0 and n / 2 carries no gradient (their sines vanish). The inverse transform of a half spectrum X is X_0 + X_{n / 2} (-1)^j +
2 sum Re(X_k e^{+2 pi i k j / n}), so the adjoint is the inverse transform of c_k G_k with c_0 = c_{n / 2} = 1 / n and c_k = 1 / (2 n)
between, all exact in binary16, and dx[t] = sum_f w[j] du_f[j] is the overlap-add without the division: a raw-sum, per-bin masked
plan. The power spectrogram P = gain (re^2 + im^2) has dP / dS = 2 gain S, so its gradient is the same plan, per frame, on the
recomputed S with the real mask M = gain gP c' (c' = 2 c: 2 / n on bins 0 and n / 2, 1 / n between).

Out of scope: the gradients of band-mode spectrograms (band_spectrogram), the gradient of the ISTFT with respect to its spectra,
and the gradient with respect to the window (it comes back as None)."""
from . import _stft_common as common
from . import mistftn, spec, stftn
from .capi import TfftError

_adjoint_masks = {}        # (n, device index) -> the per-bin mask c of the adjoint, n / 2 + 1 halves
_functions = None


def _adjoint_mask(n, device):
    import torch

    key = (int(n), device.index)
    if key not in _adjoint_masks:
        c = torch.full((common._bins(n),), 1.0 / (2 * n), dtype=torch.float16, device=device)     # 2^-10 .. 2^-12: exact
        c[0] = c[n // 2] = 1.0 / n
        _adjoint_masks[key] = c
    return _adjoint_masks[key]


def _check(name, n_fft):
    n = int(n_fft)
    if n not in mistftn.MISTFTN_LENGTHS:
        raise TfftError(5, f"{name} takes n_fft = 512, 1024 or 2048")
    return n


def _build():
    """the torch.autograd.Functions, built on first use so that importing the package does not import torch"""
    global _functions
    if _functions is not None:
        return _functions
    import torch

    class ShortStft(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, window, hop, n, center):
            ctx.save_for_backward(window)
            ctx.shape = (hop, n, center, x.shape[1], x.dtype)
            return stftn.short_stft(x, window, hop, n, center=center)

        @staticmethod
        def backward(ctx, g_re, g_im):
            (window,) = ctx.saved_tensors
            hop, n, center, length, dtype = ctx.shape
            if not ctx.needs_input_grad[0]:
                return None, None, None, None, None
            rows, frames = (g_re if g_re is not None else g_im).shape[:2]
            bins, pitch = common._bins(n), common._pitch(n)
            # (g_re, g_im) in the layout short_stft writes; halves beyond bin n / 2 are never read
            buf = torch.empty((rows, frames, 2, pitch), dtype=torch.float16, device=window.device)
            for plane, g in enumerate((g_re, g_im)):
                if g is None:
                    buf[:, :, plane, :bins] = 0
                else:
                    buf[:, :, plane, :bins] = g
            entry = mistftn._plan_for(n, rows, length, hop, n // 2 if center else 0, True, True, window.device.index)
            dx = mistftn._run(entry, buf[:, :, 0, :bins], buf[:, :, 1, :bins], _adjoint_mask(n, window.device), window, length)
            return dx.to(dtype), None, None, None, None

    class PowerSpectrogram(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, window, hop, n, center, gain):
            ctx.save_for_backward(x, window)
            ctx.shape = (hop, n, center, gain)
            return spec.power_spectrogram(x, window, hop, n, center=center, gain=gain)

        @staticmethod
        def backward(ctx, g_p):
            x, window = ctx.saved_tensors
            hop, n, center, gain = ctx.shape
            if not ctx.needs_input_grad[0]:
                return None, None, None, None, None, None
            re, im = stftn.short_stft(x, window, hop, n, center=center)              # S, recomputed
            rows, frames, bins = re.shape
            weight = torch.full((bins,), gain / n, dtype=torch.float32, device=x.device)
            weight[0] = weight[n // 2] = 2.0 * gain / n
            m = g_p.to(torch.float32) * weight                                         # M, fp32
            # a power-of-two scale s >= max |M| without a host sync: max |M| = mant * 2^exp with mant in [0.5, 1), s = 2^exp; a maximum of
            # 0 has exp = 0, s = 1
            _, exp = torch.frexp(m.abs().amax())
            s = torch.ldexp(torch.ones((), dtype=torch.float32, device=x.device), exp)
            mask = mistftn.mask_buffer(rows, frames, n, x.device)
            mask.copy_(m / s)                                                          # fp16(M / s): entries below 2^-24 s are dropped
            entry = mistftn._plan_for(n, rows, x.shape[1], hop, n // 2 if center else 0, True, False, x.device.index)
            y = mistftn._run(entry, re, im, mask, window, x.shape[1])
            return (y.to(torch.float32) * s).to(x.dtype), None, None, None, None, None

    _functions = (ShortStft, PowerSpectrogram)
    return _functions


def differentiable_short_stft(x, window, hop, n_fft, center=False):
    """short_stft(x, window, hop, n_fft, center) with a grad_fn: returns the same (re, im) views with the same bits. The backward
    pass lays the incoming (g_re, g_im) out as short_stft lays its spectra out and runs ONE cached raw-sum, per-bin masked ISTFT plan
    on them with the mask c[0] = c[n / 2] = 1 / n, c[k] = 1 / (2 n) between (exact in binary16), which is the exact adjoint (the module's
    docstring has the derivation):
        dx[t] = sum_f w[j] (1 / n) (G_0 + sum_{0 < k < n / 2} Re(G_k e^{+2 pi i k j / n}) + G_{n / 2} (-1)^j),   j = t + pad - f hop,
    in the arithmetic of include/tfft_mistftn.h (binary16 frames, an fp32 overlap-add, one rounding to binary16), cast to x.dtype.
    The IM of bins 0 and n / 2 carries no gradient. The window's gradient is None: the window is treated as a constant. The plan's
    input condition, n |c_k (G_A[k] + i G_B[k])| <= 64512 for the two frames A, B of a pair, holds for every finite binary16 gradient
    between the edge bins (|G_A + i G_B| / 2 <= 65504 / sqrt(2)) and on the edge bins for |G| <= 64512."""
    n = _check("differentiable_short_stft", n_fft)
    return _build()[0].apply(x, window, int(hop), n, bool(center))


def differentiable_power_spectrogram(x, window, hop, n_fft, center=False, gain=1.0):
    """power_spectrogram(x, window, hop, n_fft, center, gain) with a grad_fn: the same float32 view with the same bits. The backward
    pass recomputes S with short_stft, forms M = gain * gP * (2 / n on bins 0 and n / 2, 1 / n between) in fp32, takes a power-of-two
    scale s >= max |M| on the device (no host sync; s = 1 when the maximum is 0), runs ONE cached raw-sum, per-frame masked ISTFT plan on
    (S, fp16(M / s)) and returns s * y in x.dtype. Mask entries below 2^-24 * s are dropped (they round to zero in binary16), and those
    below 2^-14 * s keep fewer bits. The window's gradient is None."""
    n = _check("differentiable_power_spectrogram", n_fft)
    return _build()[1].apply(x, window, int(hop), n, bool(center), float(gain))


def stft_autograd_cache_clear():
    """Drops the adjoint masks this module keeps per (n_fft, device); the plans are mistftn's (mistftn_cache_clear)."""
    _adjoint_masks.clear()
