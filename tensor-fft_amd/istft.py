"""ctypes binding of include/tfft_istft.h (libtfft_istft.so, the inverse short-time Fourier transform add-on). No fallback of any
kind. What the four STFT bindings share lives in _stft_common.py."""
import ctypes
import os

from . import _stft_common as common
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_istft.so"
_PREFIX = "tfft_istft_"

# every symbol include/tfft_istft.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_istft_geometry", "tfft_istft_plan_create", "tfft_istft_plan_destroy", "tfft_istft_plan_set_window",
    "tfft_istft_plan_workspace_bytes", "tfft_istft_plan_set_workspace", "tfft_istft_plan_prepare", "tfft_istft_exec",
    "tfft_istft_plan_num_launches", "tfft_istft_plan_kernels", "tfft_istft_describe", "tfft_istft_last_error",
]
ISTFT_N = 4096                                                # TFFT_ISTFT_N: the frame length of every plan
ISTFT_BINS = 2049                                             # TFFT_ISTFT_BINS: bins 0 .. n / 2
ISTFT_PITCH = 2056                                            # TFFT_ISTFT_PITCH: rplan_spectrum_pitch(4096)
ISTFT_RAW_SUM = 1                                             # TFFT_ISTFT_RAW_SUM: no division by the window envelope


class IstftOpts(ctypes.Structure):
    """tfft_istft_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_frame_stride", ctypes.c_uint64),
                ("out_sig_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int)]


def istft_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


_lib = None


def load_istft_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_istft.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is None:
        _lib = common._load(istft_lib_path(), "ISTFT", _PREFIX, IstftOpts, takes_n=False, inverse=True)
    return _lib


def istft_geometry(length, hop, pad=0):
    """tfft_istft_geometry: F = 1 + (length + 2 pad - 4096) // hop, the frames per signal. Host only."""
    return common._geometry(load_istft_library(), _PREFIX, None, length, hop, pad)


def istft_describe(length, hop, pad=0, rows=1, raw_sum=False):
    """tfft_istft_describe: "istft4096:4096 x F + ola", F the frames per signal. Host only, no GPU needed."""
    return common._describe(load_istft_library(), _PREFIX, None, length, hop, pad, rows, ISTFT_RAW_SUM if raw_sum else 0)


class TfftIstftPlan(common._InversePlan):
    """Owning wrapper of tfft_istft_plan: half spectra (bins 0 .. 2048 of rfft / 4096, what TfftStftPlan writes) of `rows` * frames
    frames of 4096 samples that start at f * hop - pad -> `rows` real fp16 signals of `length` samples (include/tfft_istft.h): a
    one-pass C2R of every frame into the workspace, then y = sum w v / sum w w over the frames that cover a sample, +0 where that
    sum of squares is 0 (raw_sum: y = sum w v). Frame g = r * frames + f of an input plane lies at g * in_frame_stride (0 = 2 *
    pitch), signal r of the output at r * out_sig_stride (0 = length). set_window(w) takes a CUDA float16 tensor of 4096 halves
    before the first exec. Output, inputs and workspace must not overlap."""
    _prefix, _takes_n = _PREFIX, False

    def __init__(self, rows, length, hop, pad=0, device=0, in_frame_stride=0, out_sig_stride=0, launch_iters=0, raw_sum=False):
        opts = IstftOpts(ctypes.sizeof(IstftOpts), 0, int(in_frame_stride), int(out_sig_stride), int(launch_iters), ISTFT_RAW_SUM if raw_sum else 0)
        self._create(load_istft_library(), opts, ISTFT_N, rows, length, hop, pad, device)
        self.raw_sum = bool(raw_sum)


# istft keeps the plans of the last ISTFT_CACHE_SIZE (rows, length, hop, pad, raw_sum, device) shapes, least recently used first out,
# each with the identity of the window it holds, as stft does. A plan holds device memory outside torch's allocator (tables, window,
# workspace): a caller with many shapes should hold TfftIstftPlan objects itself; istft_cache_clear() releases them.
ISTFT_CACHE_SIZE = 8
_plans = {}


def _plan_for(rows, length, hop, pad, raw_sum, device):
    key = (int(rows), int(length), int(hop), int(pad), bool(raw_sum), int(device))
    return common._cached(_plans, ISTFT_CACHE_SIZE, key, lambda: TfftIstftPlan(rows, length, hop, pad, device, raw_sum=raw_sum))


def istft_cache_clear():
    """Destroys the plans istft cached."""
    common._cache_clear(_plans)


def istft(re, im, window, hop, length, center=False, raw_sum=False, n_fft=ISTFT_N):
    """Inverse short-time Fourier transform at frame length 4096 (n_fft = 512, 1024 or 2048: istftn.short_istft, which takes the
    same arguments at that frame length): re, im the CUDA float16 [R, F, 2049] views stft() returns (bins
    0 .. 2048 of rfft(window * frame) / 4096, frame-major), taken as they are; any other [R, F, 2049] pair is copied into that
    layout first. window a CUDA float16 tensor [win_length <= 4096] (a shorter one is zero-padded to 4096 with the window centred, as
    in stft), hop a multiple of 8, length the samples per signal (F must be the frame count of that length). center as in stft.
    Returns a new [R, length] tensor: sum w v / sum w w over the frames that cover a sample, +0 where no frame or only zeros of the
    window cover it; raw_sum=True leaves the division out. The window is handed to the cached plan again only when (data_ptr,
    _version) of it changed since the last call."""
    if n_fft != ISTFT_N:
        from . import istftn

        if n_fft not in istftn.ISTFTN_LENGTHS:
            raise TfftError(5, "istft takes n_fft = 512, 1024, 2048 or 4096")
        return istftn.short_istft(re, im, window, hop, length, n_fft, center, raw_sum)
    common._check_inverse("istft", re, im, window, ISTFT_N)
    entry = _plan_for(int(re.shape[0]), length, hop, ISTFT_N // 2 if center else 0, raw_sum, re.device.index)
    return common._inverse(entry, re, im, window, length)
