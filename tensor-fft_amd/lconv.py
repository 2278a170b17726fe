"""ctypes binding of include/tfft_lconv.h (libtfft_lconv.so, the causal real convolution add-on). No fallback of any kind. What the
convolution bindings share lives in _conv_common.py. exec refuses a tensor of the wrong kind, x or y, before a short one: its own
order, kept here."""
import ctypes
import os

from . import _binding
from . import _conv_common as common
from . import conv

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_lconv.so"
_PREFIX = "tfft_lconv_"

# every symbol include/tfft_lconv.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_lconv_fft_length", "tfft_lconv_plan_create", "tfft_lconv_plan_destroy", "tfft_lconv_plan_set_taps", "tfft_lconv_plan_spectrum",
    "tfft_lconv_spectrum_host", "tfft_lconv_plan_fft_length", "tfft_lconv_plan_workspace_bytes", "tfft_lconv_plan_set_workspace", "tfft_lconv_plan_prepare",
    "tfft_lconv_exec", "tfft_lconv_plan_num_launches", "tfft_lconv_plan_kernels", "tfft_lconv_describe", "tfft_lconv_last_error",
]
LCONV_COMPOSED = 1                                            # tfft_lconv_opts.flags


class LconvOpts(ctypes.Structure):
    """tfft_lconv_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_seq_stride", ctypes.c_uint64),
                ("out_seq_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int)]


def lconv_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


def _prototypes():
    vp, u64, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
    return {
        "tfft_lconv_fft_length": (u64, [u64, u64]),
        "tfft_lconv_plan_create": (ci, [u64, u64, u64, u64, ci, ctypes.POINTER(LconvOpts), ctypes.POINTER(vp)]),
        "tfft_lconv_plan_destroy": (None, [vp]),
        "tfft_lconv_plan_set_taps": (ci, [vp, vp, vp]),
        "tfft_lconv_plan_spectrum": (ci, [vp, vp, vp]),
        "tfft_lconv_spectrum_host": (ci, [vp, u64, u64, vp, vp]),
        "tfft_lconv_plan_fft_length": (u64, [vp]),
        "tfft_lconv_plan_workspace_bytes": (sz, [vp]),
        "tfft_lconv_plan_set_workspace": (ci, [vp, vp, sz]),
        "tfft_lconv_plan_prepare": (ci, [vp]),
        "tfft_lconv_exec": (ci, [vp, vp, vp, vp]),
        "tfft_lconv_plan_num_launches": (ci, [vp]),
        "tfft_lconv_plan_kernels": (ci, [vp, ctypes.c_char_p, sz]),
        "tfft_lconv_describe": (ci, [u64, u64, u64, u64, ci, ctypes.c_char_p, sz]),
        "tfft_lconv_last_error": (ctypes.c_char_p, []),
    }


_lib = None


def load_lconv_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_lconv.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is None:
        _lib = _binding._load(conv.load_conv_library, lconv_lib_path(), "causal convolution", _prototypes())
    return _lib


def lconv_fft_length(length, taps):
    """tfft_lconv_fft_length: the smallest power of two >= max(length + taps - 1, 256), the composed path's transform length; 0 for
    shapes no plan accepts. Host only."""
    return int(load_lconv_library().tfft_lconv_fft_length(int(length), int(taps)))


def lconv_describe(length, taps, rows=1, channels=1, composed=False):
    """tfft_lconv_describe: "lconv4096:4096" or "pack | <the sub-plan's description> | crop". Host only, no GPU needed."""
    L = load_lconv_library()
    buf = ctypes.create_string_buffer(512)
    _binding._check(L, _PREFIX, L.tfft_lconv_describe(int(length), int(taps), int(rows), int(channels), LCONV_COMPOSED if composed else 0,
                                                    buf, len(buf)))
    return buf.value.decode()


def lconv_spectrum_host(taps, n):
    """tfft_lconv_spectrum_host: (re, im) float16 arrays of n bins, the binary16 spectrum a plan builds from one filter's taps."""
    import numpy as np

    L = load_lconv_library()
    taps = np.ascontiguousarray(taps, dtype=np.float16)
    re, im = np.empty(int(n), np.float16), np.empty(int(n), np.float16)
    _binding._check(L, _PREFIX, L.tfft_lconv_spectrum_host(taps.ctypes.data, taps.size, int(n), re.ctypes.data, im.ctypes.data))
    return re, im


class TfftCausalConvPlan(common._Taps, _binding._Workspace, common._SeqPlan):
    """Owning wrapper of tfft_lconv_plan: y[b][c][t] = sum_j h[c][j] x[b][c][t - j] for rows x channels real fp16 sequences of
    `length` samples and `taps` real taps per channel (include/tfft_lconv.h). set_taps(h) takes a CUDA float16 tensor of
    channels * taps halves before the first exec. length <= 2048 with length + taps - 1 <= 4096 runs as one fused kernel unless composed=True."""
    _prefix = _PREFIX

    def __init__(self, rows, channels, length, taps, device=0, in_seq_stride=0, out_seq_stride=0, launch_iters=0, composed=False):
        L = load_lconv_library()
        opts = LconvOpts(ctypes.sizeof(LconvOpts), 0, int(in_seq_stride), int(out_seq_stride), int(launch_iters), LCONV_COMPOSED if composed else 0)
        self._create(L, L.tfft_lconv_plan_create, rows, channels, length, taps, device, opts)
        self.composed = bool(composed)
        self.n = int(L.tfft_lconv_plan_fft_length(self._h))       # 4096 for the fused kernel, else lconv_fft_length(length, taps)
        self.in_seq_stride = int(in_seq_stride) or self.length
        self.out_seq_stride = int(out_seq_stride) or self.length

    def exec_ptr(self, src, dst, stream=0):
        self._check(self._lib.tfft_lconv_exec(self._h, src, dst, stream))

    def exec(self, x, y, stream=None):
        """x, y: flat CUDA float16 tensors, sequence (b, c) at (b * channels + c) * seq stride."""
        import torch

        for t in (x, y):
            self._check_kind(t, "sequences")
        self._check_room(x, self.in_seq_stride, self.length, "sequences")
        self._check_room(y, self.out_seq_stride, self.length, "sequences")
        with torch.cuda.device(self.device):
            self.exec_ptr(x.data_ptr(), y.data_ptr(), self._stream(stream))


# causal_conv keeps the plans of the last LCONV_CACHE_SIZE (rows, channels, length, taps, device) shapes, least recently used first
# out, each with the identity of the taps it holds. A plan holds device memory outside torch's allocator (tables, spectra, a workspace
# on the composed path): a caller with many shapes should hold TfftCausalConvPlan objects itself; lconv_cache_clear() releases them.
LCONV_CACHE_SIZE = 8
_plans = {}


def _plan_for(rows, channels, length, taps, device):
    key = (int(rows), int(channels), int(length), int(taps), int(device))
    return _binding._cached(_plans, LCONV_CACHE_SIZE, key, lambda: TfftCausalConvPlan(rows, channels, length, taps, device))


def lconv_cache_clear():
    """Destroys the plans causal_conv cached."""
    _binding._cache_clear(_plans)


def causal_conv(x, h):
    """y[b, c, t] = sum_{j <= t} h[c, j] x[b, c, t - j]: x a CUDA float16 tensor [B, C, L] (L a multiple of 8), h [C, K]. Returns
    y [B, C, L]. The taps are handed to the cached plan again only when (data_ptr, _version) of h changed since the last call."""
    import torch

    common._check_tap_args("causal_conv takes CUDA float16 tensors x (B, C, L) and h (C, K) on one device", (x,), (), h)
    rows, channels, length = x.shape
    entry = _plan_for(rows, channels, length, h.shape[1], x.device.index)
    common._hand_taps(entry, h)
    x = x.contiguous()
    y = torch.empty_like(x)
    entry[0].exec(x.view(-1), y.view(-1))
    return y
