"""ctypes binding of include/tfft_istftn.h (libtfft_istftn.so, the short-frame inverse STFT add-on: frame lengths 512, 1024 and
2048). No fallback of any kind. What the four STFT bindings share lives in _stft_common.py."""
import ctypes
import os

from . import _stft_common as common
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_istftn.so"
_PREFIX = "tfft_istftn_"

# every symbol include/tfft_istftn.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_istftn_geometry", "tfft_istftn_plan_create", "tfft_istftn_plan_destroy", "tfft_istftn_plan_set_window",
    "tfft_istftn_plan_workspace_bytes", "tfft_istftn_plan_set_workspace", "tfft_istftn_plan_prepare", "tfft_istftn_exec",
    "tfft_istftn_plan_num_launches", "tfft_istftn_plan_kernels", "tfft_istftn_describe", "tfft_istftn_last_error",
]
ISTFTN_LENGTHS = (512, 1024, 2048)                            # the frame lengths of a plan
ISTFTN_RAW_SUM = 1                                            # TFFT_ISTFTN_RAW_SUM: no division by the window envelope


def istftn_bins(n):
    """bins 0 .. n / 2 of a frame"""
    return common._bins(n)


def istftn_pitch(n):
    """tfft_rplan_spectrum_pitch(n): 264, 520, 1032"""
    return common._pitch(n)


class IstftNOpts(ctypes.Structure):
    """tfft_istftn_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_frame_stride", ctypes.c_uint64),
                ("out_sig_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int)]


def istftn_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


_lib = None


def load_istftn_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_istftn.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is None:
        _lib = common._load(istftn_lib_path(), "short-frame ISTFT", _PREFIX, IstftNOpts, takes_n=True, inverse=True)
    return _lib


def istftn_geometry(n, length, hop, pad=0):
    """tfft_istftn_geometry: F = 1 + (length + 2 pad - n) // hop, the frames per signal. Host only."""
    return common._geometry(load_istftn_library(), _PREFIX, n, length, hop, pad)


def istftn_describe(n, length, hop, pad=0, rows=1, raw_sum=False):
    """tfft_istftn_describe: "istft256r<R>:n x F + ola", R = n / 256 and F the frames per signal. Host only, no GPU needed."""
    return common._describe(load_istftn_library(), _PREFIX, n, length, hop, pad, rows, ISTFTN_RAW_SUM if raw_sum else 0)


class TfftShortIstftPlan(common._InversePlan):
    """Owning wrapper of tfft_istftn_plan: half spectra (bins 0 .. n / 2 of rfft / n, what TfftShortStftPlan writes) of `rows` * frames
    frames of n samples (512, 1024 or 2048) that start at f * hop - pad -> `rows` real fp16 signals of `length` samples
    (include/tfft_istftn.h): a one-pass C2R of every frame into the workspace, then y = sum w v / sum w w over the frames that cover a
    sample, +0 where that sum of squares is 0 (raw_sum: y = sum w v). Frame g = r * frames + f of an input plane lies at
    g * in_frame_stride (0 = 2 * pitch), signal r of the output at r * out_sig_stride (0 = length). set_window(w) takes a CUDA
    float16 tensor of n halves before the first exec. Output, inputs and workspace must not overlap."""
    _prefix, _takes_n = _PREFIX, True

    def __init__(self, n, rows, length, hop, pad=0, device=0, in_frame_stride=0, out_sig_stride=0, launch_iters=0, raw_sum=False):
        opts = IstftNOpts(ctypes.sizeof(IstftNOpts), 0, int(in_frame_stride), int(out_sig_stride), int(launch_iters),
                          ISTFTN_RAW_SUM if raw_sum else 0)
        self._create(load_istftn_library(), opts, n, rows, length, hop, pad, device)
        self.raw_sum = bool(raw_sum)


# short_istft keeps the plans of the last ISTFTN_CACHE_SIZE (n, rows, length, hop, pad, raw_sum, device) shapes, least recently used
# first out, each with the identity of the window it holds, as istft does. A plan holds device memory outside torch's allocator
# (tables, window, workspace): a caller with many shapes should hold TfftShortIstftPlan objects itself; istftn_cache_clear()
# releases them.
ISTFTN_CACHE_SIZE = 8
_plans = {}


def _plan_for(n, rows, length, hop, pad, raw_sum, device):
    key = (int(n), int(rows), int(length), int(hop), int(pad), bool(raw_sum), int(device))
    return common._cached(_plans, ISTFTN_CACHE_SIZE, key, lambda: TfftShortIstftPlan(n, rows, length, hop, pad, device, raw_sum=raw_sum))


def istftn_cache_clear():
    """Destroys the plans short_istft cached."""
    common._cache_clear(_plans)


def short_istft(re, im, window, hop, length, n_fft, center=False, raw_sum=False):
    """Inverse short-time Fourier transform at frame length n_fft = 512, 1024 or 2048: re, im the CUDA float16 [R, F, n_fft / 2 + 1]
    views short_stft() returns (bins 0 .. n_fft / 2 of rfft(window * frame) / n_fft, frame-major), taken as they are; any other
    [R, F, n_fft / 2 + 1] pair is copied into that layout first. window a CUDA float16 tensor [win_length <= n_fft] (a shorter one
    is zero-padded to n_fft with the window centred, as in short_stft), hop a multiple of 8, length the samples per signal (F must
    be the frame count of that length). center as in short_stft: True means pad = n_fft / 2. Returns a new [R, length] tensor:
    sum w v / sum w w over the frames that cover a sample, +0 where no frame or only zeros of the window cover it; raw_sum=True
    leaves the division out. The window is handed to the cached plan again only when (data_ptr, _version) of it changed since the
    last call."""
    n = int(n_fft)
    if n not in ISTFTN_LENGTHS:
        raise TfftError(5, "short_istft takes n_fft = 512, 1024 or 2048 (4096: istft)")
    common._check_inverse("short_istft", re, im, window, n)
    entry = _plan_for(n, int(re.shape[0]), length, hop, n // 2 if center else 0, raw_sum, re.device.index)
    return common._inverse(entry, re, im, window, length)
