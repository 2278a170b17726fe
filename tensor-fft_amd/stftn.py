"""ctypes binding of include/tfft_stftn.h (libtfft_stftn.so, the short-frame STFT add-on: frame lengths 512, 1024 and 2048). No
fallback of any kind. What the four STFT bindings share lives in _stft_common.py."""
import ctypes
import os

from . import _stft_common as common
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_stftn.so"
_PREFIX = "tfft_stftn_"

# every symbol include/tfft_stftn.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_stftn_geometry", "tfft_stftn_plan_create", "tfft_stftn_plan_destroy", "tfft_stftn_plan_set_window", "tfft_stftn_exec",
    "tfft_stftn_plan_num_launches", "tfft_stftn_plan_kernels", "tfft_stftn_describe", "tfft_stftn_last_error",
]
STFTN_LENGTHS = (512, 1024, 2048)                             # the frame lengths of a plan


def stftn_bins(n):
    """bins 0 .. n / 2 of a frame"""
    return common._bins(n)


def stftn_pitch(n):
    """tfft_rplan_spectrum_pitch(n): 264, 520, 1032"""
    return common._pitch(n)


class StftNOpts(ctypes.Structure):
    """tfft_stftn_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_sig_stride", ctypes.c_uint64),
                ("out_frame_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int)]


def stftn_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


_lib = None


def load_stftn_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_stftn.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is None:
        _lib = common._load(stftn_lib_path(), "short-frame STFT", _PREFIX, StftNOpts, takes_n=True, inverse=False)
    return _lib


def stftn_geometry(n, length, hop, pad=0):
    """tfft_stftn_geometry: F = 1 + (length + 2 pad - n) // hop, the frames per signal. Host only."""
    return common._geometry(load_stftn_library(), _PREFIX, n, length, hop, pad)


def stftn_describe(n, length, hop, pad=0, rows=1):
    """tfft_stftn_describe: "stft256r<R>:n x F", R = n / 256 and F the frames per signal. Host only, no GPU needed."""
    return common._describe(load_stftn_library(), _PREFIX, n, length, hop, pad, rows, 0)


class TfftShortStftPlan(common._ForwardPlan):
    """Owning wrapper of tfft_stftn_plan: `rows` real fp16 signals of `length` samples (a multiple of 8) -> frames of n samples
    (512, 1024 or 2048) that start at f * hop - pad (zeros outside the signal), each multiplied by the window in binary16 and
    transformed to bins 0 .. n / 2 of rfft / n, in one kernel (include/tfft_stftn.h). Frame g = r * frames + f of a plane lies at
    g * out_frame_stride (0 = 2 * pitch). set_window(w) takes a CUDA float16 tensor of n halves before the first exec. Input and
    output must not overlap."""
    _prefix, _takes_n = _PREFIX, True

    def __init__(self, n, rows, length, hop, pad=0, device=0, in_sig_stride=0, out_frame_stride=0, launch_iters=0):
        opts = StftNOpts(ctypes.sizeof(StftNOpts), 0, int(in_sig_stride), int(out_frame_stride), int(launch_iters), 0)
        self._create(load_stftn_library(), opts, n, rows, length, hop, pad, device)


# short_stft keeps the plans of the last STFTN_CACHE_SIZE (n, rows, length, hop, pad, device) shapes, least recently used first out,
# each with the identity of the window it holds, as stft does. A plan holds device memory outside torch's allocator (tables, window):
# a caller with many shapes should hold TfftShortStftPlan objects itself; stftn_cache_clear() releases them.
STFTN_CACHE_SIZE = 8
_plans = {}


def _plan_for(n, rows, length, hop, pad, device):
    key = (int(n), int(rows), int(length), int(hop), int(pad), int(device))
    return common._cached(_plans, STFTN_CACHE_SIZE, key, lambda: TfftShortStftPlan(n, rows, length, hop, pad, device))


def stftn_cache_clear():
    """Destroys the plans short_stft cached."""
    common._cache_clear(_plans)


def short_stft(x, window, hop, n_fft, center=False):
    """Short-time Fourier transform at frame length n_fft = 512, 1024 or 2048: x a CUDA float16 tensor [R, L] (L a multiple of 8),
    window a CUDA float16 tensor [win_length <= n_fft] (a shorter window is zero-padded to n_fft with the window centred, as
    torch.stft does), hop a multiple of 8. center=False frames from sample 0 (torch.stft(center=False)); center=True pads n_fft / 2
    zeros on both sides (torch.stft(center=True, pad_mode="constant")). Returns (re, im), each an [R, F, n_fft / 2 + 1] view of one
    new [R, F, 2, h] buffer, h = rplan_spectrum_pitch(n_fft): bins 0 .. n_fft / 2 of rfft(window * frame) / n_fft. The layout is
    FRAME-major; torch.stft returns [R, bins, F], bin-major, and does not divide by n_fft. The window is handed to the cached plan
    again only when (data_ptr, _version) of it changed since the last call."""
    n = int(n_fft)
    if n not in STFTN_LENGTHS:
        raise TfftError(5, "short_stft takes n_fft = 512, 1024 or 2048 (4096: stft)")
    common._check_forward("short_stft", x, window, n)
    rows, length = x.shape
    return common._forward(_plan_for(n, rows, length, hop, n // 2 if center else 0, x.device.index), x, window)
