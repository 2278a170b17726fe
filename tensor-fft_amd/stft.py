"""ctypes binding of include/tfft_stft.h (libtfft_stft.so, the short-time Fourier transform add-on). No fallback of any kind. What
the four STFT bindings share lives in _stft_common.py."""
import ctypes
import os

from . import _stft_common as common
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_stft.so"
_PREFIX = "tfft_stft_"

# every symbol include/tfft_stft.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_stft_geometry", "tfft_stft_plan_create", "tfft_stft_plan_destroy", "tfft_stft_plan_set_window", "tfft_stft_exec",
    "tfft_stft_plan_num_launches", "tfft_stft_plan_kernels", "tfft_stft_describe", "tfft_stft_last_error",
]
STFT_N = 4096                                                 # TFFT_STFT_N: the frame length of every plan
STFT_BINS = 2049                                              # TFFT_STFT_BINS: bins 0 .. n / 2
STFT_PITCH = 2056                                             # TFFT_STFT_PITCH: rplan_spectrum_pitch(4096)


class StftOpts(ctypes.Structure):
    """tfft_stft_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_sig_stride", ctypes.c_uint64),
                ("out_frame_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int)]


def stft_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


_lib = None


def load_stft_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_stft.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is None:
        _lib = common._load(stft_lib_path(), "STFT", _PREFIX, StftOpts, takes_n=False, inverse=False)
    return _lib


def stft_geometry(length, hop, pad=0):
    """tfft_stft_geometry: F = 1 + (length + 2 pad - 4096) // hop, the frames per signal. Host only."""
    return common._geometry(load_stft_library(), _PREFIX, None, length, hop, pad)


def stft_describe(length, hop, pad=0, rows=1):
    """tfft_stft_describe: "stft4096:4096 x F", F the frames per signal. Host only, no GPU needed."""
    return common._describe(load_stft_library(), _PREFIX, None, length, hop, pad, rows, 0)


class TfftStftPlan(common._ForwardPlan):
    """Owning wrapper of tfft_stft_plan: `rows` real fp16 signals of `length` samples (a multiple of 8) -> frames of 4096 samples
    that start at f * hop - pad (zeros outside the signal), each multiplied by the window in binary16 and transformed to bins
    0 .. 2048 of rfft / 4096, in one kernel (include/tfft_stft.h). Frame g = r * frames + f of a plane lies at g * out_frame_stride
    (0 = 2 * pitch). set_window(w) takes a CUDA float16 tensor of 4096 halves before the first exec. Input and output must not
    overlap."""
    _prefix, _takes_n = _PREFIX, False

    def __init__(self, rows, length, hop, pad=0, device=0, in_sig_stride=0, out_frame_stride=0, launch_iters=0):
        opts = StftOpts(ctypes.sizeof(StftOpts), 0, int(in_sig_stride), int(out_frame_stride), int(launch_iters), 0)
        self._create(load_stft_library(), opts, STFT_N, rows, length, hop, pad, device)


# stft keeps the plans of the last STFT_CACHE_SIZE (rows, length, hop, pad, device) shapes, least recently used first out, each with
# the identity of the window it holds, as long_causal_conv does for its taps. A plan holds device memory outside torch's allocator
# (tables, window): a caller with many shapes should hold TfftStftPlan objects itself; stft_cache_clear() releases them.
STFT_CACHE_SIZE = 8
_plans = {}


def _plan_for(rows, length, hop, pad, device):
    key = (int(rows), int(length), int(hop), int(pad), int(device))
    return common._cached(_plans, STFT_CACHE_SIZE, key, lambda: TfftStftPlan(rows, length, hop, pad, device))


def stft_cache_clear():
    """Destroys the plans stft cached."""
    common._cache_clear(_plans)


def stft(x, window, hop, center=False, n_fft=STFT_N):
    """n_fft = 512, 1024 or 2048: short_stft(x, window, hop, n_fft, center) of tensor_fft_amd.stftn (include/tfft_stftn.h), with
    n_fft in the place of 4096 below; nothing of this module is touched. Any other n_fft but 4096 is refused.

    Short-time Fourier transform at frame length 4096: x a CUDA float16 tensor [R, L] (L a multiple of 8), window a CUDA float16
    tensor [win_length <= 4096] (a shorter window is zero-padded to 4096 with the window centred, as torch.stft does), hop a
    multiple of 8. center=False frames from sample 0 (torch.stft(center=False)); center=True pads 2048 zeros on both sides
    (torch.stft(center=True, pad_mode="constant")). Returns (re, im), each an [R, F, 2049] view of one new [R, F, 2, 2056] buffer:
    bins 0 .. 2048 of rfft(window * frame) / 4096. The layout is FRAME-major; torch.stft returns [R, 2049, F], bin-major, and does
    not divide by 4096. The window is handed to the cached plan again only when (data_ptr, _version) of it changed since the last
    call."""
    if n_fft != STFT_N:
        from . import stftn

        if n_fft not in stftn.STFTN_LENGTHS:
            raise TfftError(5, "stft takes n_fft = 512, 1024, 2048 or 4096")
        return stftn.short_stft(x, window, hop, n_fft, center)
    common._check_forward("stft", x, window, STFT_N)
    rows, length = x.shape
    return common._forward(_plan_for(rows, length, hop, STFT_N // 2 if center else 0, x.device.index), x, window)
