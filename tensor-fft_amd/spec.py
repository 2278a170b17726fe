"""ctypes binding of include/tfft_spec.h (libtfft_spec.so, the spectrogram add-on: power and band energies of the short-frame STFT
at frame lengths 512, 1024 and 2048), the host-side band containers and the mel filterbank. No fallback of any kind. What the STFT
bindings share lives in _stft_common.py."""
import ctypes
import math
import os

from . import _stft_common as common
from ._binding import _is_cuda
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_spec.so"
_PREFIX = "tfft_spec_"

# every symbol include/tfft_spec.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_spec_geometry", "tfft_spec_plan_create", "tfft_spec_plan_destroy", "tfft_spec_plan_set_window", "tfft_spec_plan_set_bands",
    "tfft_spec_exec", "tfft_spec_plan_num_launches", "tfft_spec_plan_kernels", "tfft_spec_describe", "tfft_spec_last_error",
]
SPEC_LENGTHS = (512, 1024, 2048)                              # the frame lengths of a plan
SPEC_MAX_BANDS = 1024                                         # TFFT_SPEC_MAX_BANDS


class SpecOpts(ctypes.Structure):
    """tfft_spec_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_sig_stride", ctypes.c_uint64),
                ("out_frame_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int),
                ("bands", ctypes.c_uint32), ("gain", ctypes.c_float)]


def spec_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


_lib = None


def load_spec_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_spec.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is None:
        vp, u32p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)
        own = {"exec": (ctypes.c_int, [vp, vp, vp, vp]),
               "plan_set_bands": (ctypes.c_int, [vp, ctypes.c_uint32, u32p, u32p, ctypes.POINTER(ctypes.c_float), vp])}
        _lib = common._load(spec_lib_path(), "spectrogram", _PREFIX, SpecOpts, takes_n=True, inverse=False, own=own)
    return _lib


def spec_geometry(n, length, hop, pad=0):
    """tfft_spec_geometry: F = 1 + (length + 2 pad - n) // hop, the frames per signal. Host only."""
    return common._geometry(load_spec_library(), _PREFIX, n, length, hop, pad)


def spec_describe(n, length, hop, pad=0, rows=1):
    """tfft_spec_describe: "spec256r<R>:n x F", R = n / 256 and F the frames per signal. Host only, no GPU needed."""
    return common._describe(load_spec_library(), _PREFIX, n, length, hop, pad, rows, 0)


# ---- bands, on the host
class Bands:
    """B bands over the bins 0 .. n / 2 of a power spectrum: band j covers bins starts[j] .. starts[j] + counts[j] - 1 with the
    float32 weights weights[offsets[j] : offsets[j] + counts[j]]. Host arrays (numpy); TfftSpectrogramPlan.set_bands copies them."""

    def __init__(self, starts, counts, weights):
        import numpy as np

        self.starts = np.ascontiguousarray(starts, dtype=np.uint32).reshape(-1)
        self.counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        self.weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        if self.starts.size == 0 or self.starts.size != self.counts.size:
            raise TfftError(5, "Bands takes as many counts as starts, and at least one band")
        if int(self.counts.astype(np.int64).sum()) != self.weights.size:
            raise TfftError(5, "Bands takes sum(counts) weights")
        self.offsets = np.concatenate([[0], np.cumsum(self.counts.astype(np.int64))[:-1]])

    def __len__(self):
        return int(self.starts.size)

    def dense(self, bins):
        """the [B, bins] float32 matrix with the weights at their bins and zeros elsewhere"""
        import numpy as np

        out = np.zeros((len(self), int(bins)), np.float32)
        for j, (s, c, o) in enumerate(zip(self.starts, self.counts, self.offsets)):
            out[j, int(s):int(s) + int(c)] = self.weights[int(o):int(o) + int(c)]
        return out


def bands_from_dense(W, gain=1.0):
    """Bands of a dense [B, n / 2 + 1] filterbank (numpy or a CPU tensor): every row from its first to its last nonzero, the zeros
    inside that span kept; a row of zeros is refused. The weights are fp32(W * gain), formed in float64 and rounded once."""
    import numpy as np

    W = np.asarray(W, dtype=np.float64)
    if W.ndim != 2 or W.shape[0] == 0:
        raise TfftError(5, "bands_from_dense takes a [B, bins] matrix")
    W = (W * float(gain)).astype(np.float32)
    starts, counts, weights = [], [], []
    for j, row in enumerate(W):
        nz = np.flatnonzero(row)
        if nz.size == 0:
            raise TfftError(5, f"row {j} of the filterbank is all zero: a band holds at least one bin")
        starts.append(nz[0])
        counts.append(nz[-1] - nz[0] + 1)
        weights.append(row[nz[0]:nz[-1] + 1])
    return Bands(starts, counts, np.concatenate(weights))


def _hz_to_mel(f, scale):
    import numpy as np

    f = np.asarray(f, dtype=np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    # Slaney's Auditory Toolbox: linear below 1 kHz (200 / 3 Hz per mel), logarithmic above (27 steps per factor 6.4)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (math.log(6.4) / 27.0), f / (200.0 / 3.0))


def _mel_to_hz(m, scale):
    import numpy as np

    m = np.asarray(m, dtype=np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m >= 15.0, 1000.0 * np.exp((math.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_filterbank(n_fft, sample_rate, n_mels, f_min=0.0, f_max=None, scale="htk", norm=None):
    """The dense [n_mels, n_fft / 2 + 1] triangular mel filterbank in float64: n_mels + 2 edges equally spaced in mel between f_min
    and f_max (default: sample_rate / 2), triangle j rising from edge j to edge j + 1 and falling to edge j + 2 over the bin
    frequencies k * sample_rate / n_fft; norm="slaney" divides triangle j by half its width in Hz (unit area)."""
    import numpy as np

    if scale not in ("htk", "slaney") or norm not in (None, "slaney"):
        raise TfftError(5, 'mel bands take scale "htk" or "slaney" and norm None or "slaney"')
    f_max = float(sample_rate) / 2.0 if f_max is None else float(f_max)
    if not (0.0 <= float(f_min) < f_max <= float(sample_rate) / 2.0) or int(n_mels) < 1:
        raise TfftError(5, "mel bands take 0 <= f_min < f_max <= sample_rate / 2 and n_mels >= 1")
    edges = _mel_to_hz(np.linspace(_hz_to_mel(float(f_min), scale), _hz_to_mel(f_max, scale), int(n_mels) + 2), scale)
    freqs = np.arange(int(n_fft) // 2 + 1, dtype=np.float64) * (float(sample_rate) / int(n_fft))
    up = (freqs[None, :] - edges[:-2, None]) / (edges[1:-1] - edges[:-2])[:, None]
    down = (edges[2:, None] - freqs[None, :]) / (edges[2:] - edges[1:-1])[:, None]
    W = np.maximum(0.0, np.minimum(up, down))
    if norm == "slaney":
        W = W * (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return W


def mel_bands(n_fft, sample_rate, n_mels, f_min=0.0, f_max=None, scale="htk", norm=None):
    """Bands of the triangular mel filterbank (mel_filterbank: computed in float64, rounded once to float32). A triangle so narrow
    that no bin falls inside it is refused."""
    return bands_from_dense(mel_filterbank(n_fft, sample_rate, n_mels, f_min, f_max, scale, norm))


# ---- the plan
class TfftSpectrogramPlan(common._Plan):
    """Owning wrapper of tfft_spec_plan: `rows` real fp16 signals of `length` samples -> per frame of n samples (512, 1024 or 2048;
    framing, window and pairing as TfftShortStftPlan) either the power of bins 0 .. n / 2, fp32(gain * (re^2 + im^2)) on the
    binary16 (re, im) that plan writes (bands = 0), or the energies of `bands` bands of it, each the sequential float32 sum of
    weight * power over its bins (include/tfft_spec.h), in one kernel. Frame g = r * frames + f lies at g * out_frame_stride floats
    (0 = pitch in power mode, = bands in band mode). set_window(w) and, for a band plan, set_bands(Bands) come before the first
    exec. Input and output must not overlap."""
    _prefix, _takes_n = _PREFIX, True

    def __init__(self, n, rows, length, hop, pad=0, bands=0, gain=1.0, device=0, in_sig_stride=0, out_frame_stride=0, launch_iters=0):
        bands = int(bands)
        if not 0 <= bands < 1 << 32:
            raise TfftError(5, "bands must be 0 (power mode) or 1 .. 1024")
        opts = SpecOpts(ctypes.sizeof(SpecOpts), 0, int(in_sig_stride), int(out_frame_stride), int(launch_iters), 0, bands, float(gain))
        self._create(load_spec_library(), opts, n, rows, length, hop, pad, device)
        self.bands, self.gain = bands, float(gain)
        self.per_frame = bands or self.bins                  # floats written per frame
        self.in_sig_stride = int(in_sig_stride) or self.length
        self.out_frame_stride = int(out_frame_stride) or (bands or self.pitch)

    def set_bands(self, bands, stream=None):
        """Hands a Bands object over (tfft_spec_plan_set_bands): copied to the device; not referenced by the plan afterwards."""
        import torch

        if not isinstance(bands, Bands):
            raise TfftError(5, "set_bands takes a Bands object (bands_from_dense, mel_bands)")
        u32p, f32p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float)
        with torch.cuda.device(self.device):
            self._call("plan_set_bands", self._h, len(bands), bands.starts.ctypes.data_as(u32p), bands.counts.ctypes.data_as(u32p),
                       bands.weights.ctypes.data_as(f32p), self._stream(stream))

    def exec_ptr(self, src, out, stream=0):
        self._call("exec", self._h, src, out, stream)

    def exec(self, x, out, stream=None):
        """x: flat CUDA float16 tensor, signal r at r * in_sig_stride; out: flat CUDA float32 tensor, frame g at g * out_frame_stride."""
        import torch

        self._check_kind(x, "signals")
        if not (_is_cuda(out, torch.float32) and out.is_contiguous()):
            raise TfftError(5, "the output must be a contiguous CUDA float32 tensor")
        if out.device.index != self.device:
            raise TfftError(5, "tensor on another device than the plan")
        if x.numel() < (self.rows - 1) * self.in_sig_stride + self.length:
            raise TfftError(5, "the signal buffer is shorter than (rows - 1) * in_sig_stride + length")
        if out.numel() < (self.rows * self.frames - 1) * self.out_frame_stride + self.per_frame:
            raise TfftError(5, f"the output is shorter than (rows * frames - 1) * out_frame_stride + {self.per_frame}")
        with torch.cuda.device(self.device):
            self.exec_ptr(x.data_ptr(), out.data_ptr(), self._stream(stream))


# power_spectrogram and band_spectrogram keep the plans of the last SPEC_CACHE_SIZE (n, rows, length, hop, pad, device, bands, gain)
# keys, least recently used first out, each with the identity of the window and the Bands object it holds, as short_stft does. A plan
# holds device memory outside torch's allocator: a caller with many shapes should hold TfftSpectrogramPlan objects itself;
# spec_cache_clear() releases them.
SPEC_CACHE_SIZE = 8
_plans = {}


def _plan_for(n, rows, length, hop, pad, device, bands, gain):
    key = (int(n), int(rows), int(length), int(hop), int(pad), int(device), int(bands), float(gain))
    return common._cached(_plans, SPEC_CACHE_SIZE, key, lambda: TfftSpectrogramPlan(n, rows, length, hop, pad, bands, gain, device))


def spec_cache_clear():
    """Destroys the plans power_spectrogram and band_spectrogram cached."""
    common._cache_clear(_plans)


def _entry(name, x, window, hop, n_fft, center, bands, gain):
    n = int(n_fft)
    if n not in SPEC_LENGTHS:
        raise TfftError(5, f"{name} takes n_fft = 512, 1024 or 2048")
    common._check_forward(name, x, window, n)
    rows, length = x.shape
    entry = _plan_for(n, rows, length, hop, n // 2 if center else 0, x.device.index, bands, gain)
    common._hand_window(entry, window)
    return entry


def power_spectrogram(x, window, hop, n_fft, center=False, gain=1.0):
    """Power spectrogram at frame length n_fft = 512, 1024 or 2048: x, window, hop and center as short_stft. Returns a float32
    [R, F, n_fft / 2 + 1] view of a new [R, F, pitch] buffer: gain * |rfft(window * frame) / n_fft|^2 on the binary16 spectrum of
    short_stft (gain = n_fft ** 2 undoes the 1 / n_fft). FRAME-major. The window is handed to the cached plan again only when its
    identity changed."""
    import torch

    plan = _entry("power_spectrogram", x, window, hop, n_fft, center, 0, gain)[0]
    buf = torch.empty((plan.rows, plan.frames, plan.pitch), dtype=torch.float32, device=x.device)
    plan.exec(x.contiguous().view(-1), buf.view(-1))
    return buf[:, :, :plan.bins]


def band_spectrogram(x, window, hop, n_fft, bands, center=False, gain=1.0):
    """Band energies of the power spectrogram (mel_bands, bands_from_dense): a new float32 [R, F, B] tensor, band j of a frame the
    sequential float32 sum of weight * power over the band's bins. The power spectrum is never written. The window and the Bands
    object are handed to the cached plan again only when their identity changed (a Bands object changed in place is not noticed)."""
    import torch

    if not isinstance(bands, Bands):
        raise TfftError(5, "band_spectrogram takes a Bands object (bands_from_dense, mel_bands)")
    plan = _entry("band_spectrogram", x, window, hop, n_fft, center, len(bands), gain)[0]
    if getattr(plan, "_held_bands", None) is not bands:
        plan.set_bands(bands)
        plan._held_bands = bands
    out = torch.empty((plan.rows, plan.frames, len(bands)), dtype=torch.float32, device=x.device)
    plan.exec(x.contiguous().view(-1), out.view(-1))
    return out
