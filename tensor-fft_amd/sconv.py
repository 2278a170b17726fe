"""ctypes binding of include/tfft_sconv.h (libtfft_sconv.so, the overlap-save causal convolution add-on). No fallback of any kind.
What the convolution bindings share lives in _conv_common.py. exec refuses a tensor of the wrong kind, x or y, before a short one,
as lconv's does: its own order, kept here."""
import ctypes
import os

from . import _binding
from . import _conv_common as common
from . import conv

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_sconv.so"
_PREFIX = "tfft_sconv_"

# every symbol include/tfft_sconv.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_sconv_geometry", "tfft_sconv_plan_create", "tfft_sconv_plan_destroy", "tfft_sconv_plan_set_taps", "tfft_sconv_plan_spectrum",
    "tfft_sconv_exec", "tfft_sconv_plan_num_launches", "tfft_sconv_plan_kernels", "tfft_sconv_describe", "tfft_sconv_last_error",
]
SCONV_MAX_TAPS = 2049                                         # TFFT_SCONV_MAX_TAPS
SCONV_N = 4096                                                # the transform length of every plan


class SconvOpts(ctypes.Structure):
    """tfft_sconv_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_seq_stride", ctypes.c_uint64),
                ("out_seq_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int)]


def sconv_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


def _prototypes():
    vp, u64, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
    pu64 = ctypes.POINTER(u64)
    return {
        "tfft_sconv_geometry": (ci, [u64, u64, pu64, pu64, pu64]),
        "tfft_sconv_plan_create": (ci, [u64, u64, u64, u64, ci, ctypes.POINTER(SconvOpts), ctypes.POINTER(vp)]),
        "tfft_sconv_plan_destroy": (None, [vp]),
        "tfft_sconv_plan_set_taps": (ci, [vp, vp, vp]),
        "tfft_sconv_plan_spectrum": (ci, [vp, vp, vp]),
        "tfft_sconv_exec": (ci, [vp, vp, vp, vp]),
        "tfft_sconv_plan_num_launches": (ci, [vp]),
        "tfft_sconv_plan_kernels": (ci, [vp, ctypes.c_char_p, sz]),
        "tfft_sconv_describe": (ci, [u64, u64, u64, u64, ci, ctypes.c_char_p, sz]),
        "tfft_sconv_last_error": (ctypes.c_char_p, []),
    }


_lib = None


def load_sconv_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_sconv.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is None:
        _lib = _binding._load(conv.load_conv_library, sconv_lib_path(), "overlap-save convolution", _prototypes())
    return _lib


def sconv_geometry(length, taps):
    """tfft_sconv_geometry: (halo, hop, segments) of a plan for sequences of `length` samples and `taps` taps. Host only."""
    L = load_sconv_library()
    halo, hop, segments = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    _binding._check(L, _PREFIX, L.tfft_sconv_geometry(int(length), int(taps), ctypes.byref(halo), ctypes.byref(hop), ctypes.byref(segments)))
    return int(halo.value), int(hop.value), int(segments.value)


def sconv_describe(length, taps, rows=1, channels=1):
    """tfft_sconv_describe: "sconv4096:4096 x S", S the segments per sequence. Host only, no GPU needed."""
    L = load_sconv_library()
    buf = ctypes.create_string_buffer(128)
    _binding._check(L, _PREFIX, L.tfft_sconv_describe(int(length), int(taps), int(rows), int(channels), 0, buf, len(buf)))
    return buf.value.decode()


class TfftLongConvPlan(common._Taps, common._SeqPlan):
    """Owning wrapper of tfft_sconv_plan: y[b][c][t] = sum_j h[c][j] x[b][c][t - j] for rows x channels real fp16 sequences of any
    `length` (a multiple of 8) and `taps` <= 2049 real taps per channel, by overlap-save at transform length 4096 in one kernel
    (include/tfft_sconv.h). set_taps(h) takes a CUDA float16 tensor of channels * taps halves before the first exec. Input and
    output must not overlap."""
    _prefix = _PREFIX

    def __init__(self, rows, channels, length, taps, device=0, in_seq_stride=0, out_seq_stride=0, launch_iters=0):
        L = load_sconv_library()
        opts = SconvOpts(ctypes.sizeof(SconvOpts), 0, int(in_seq_stride), int(out_seq_stride), int(launch_iters), 0)
        self._create(L, L.tfft_sconv_plan_create, rows, channels, length, taps, device, opts)
        self.n = SCONV_N
        self.halo, self.hop, self.segments = sconv_geometry(length, taps)
        self.in_seq_stride = int(in_seq_stride) or self.length
        self.out_seq_stride = int(out_seq_stride) or self.length

    def exec_ptr(self, src, dst, stream=0):
        self._check(self._lib.tfft_sconv_exec(self._h, src, dst, stream))

    def exec(self, x, y, stream=None):
        """x, y: flat CUDA float16 tensors that share no element, sequence (b, c) at (b * channels + c) * seq stride."""
        import torch

        for t in (x, y):
            self._check_kind(t, "sequences")
        self._check_room(x, self.in_seq_stride, self.length, "sequences")
        self._check_room(y, self.out_seq_stride, self.length, "sequences")
        with torch.cuda.device(self.device):
            self.exec_ptr(x.data_ptr(), y.data_ptr(), self._stream(stream))


# long_causal_conv keeps the plans of the last SCONV_CACHE_SIZE (rows, channels, length, taps, device) shapes, least recently used
# first out, each with the identity of the taps it holds, as causal_conv does. A plan holds device memory outside torch's allocator
# (tables, spectra): a caller with many shapes should hold TfftLongConvPlan objects itself; sconv_cache_clear() releases them.
SCONV_CACHE_SIZE = 8
_plans = {}


def _plan_for(rows, channels, length, taps, device):
    key = (int(rows), int(channels), int(length), int(taps), int(device))
    return _binding._cached(_plans, SCONV_CACHE_SIZE, key, lambda: TfftLongConvPlan(rows, channels, length, taps, device))


def sconv_cache_clear():
    """Destroys the plans long_causal_conv cached."""
    _binding._cache_clear(_plans)


def long_causal_conv(x, h):
    """y[b, c, t] = sum_{j <= t} h[c, j] x[b, c, t - j]: x a CUDA float16 tensor [B, C, L] (L a multiple of 8, any length), h [C, K]
    with K <= 2049. Returns y [B, C, L], a new tensor. The taps are handed to the cached plan again only when (data_ptr, _version)
    of h changed since the last call."""
    import torch

    common._check_tap_args("long_causal_conv takes CUDA float16 tensors x (B, C, L) and h (C, K) on one device", (x,), (), h)
    rows, channels, length = x.shape
    entry = _plan_for(rows, channels, length, h.shape[1], x.device.index)
    common._hand_taps(entry, h)
    x = x.contiguous()
    y = torch.empty_like(x)
    entry[0].exec(x.view(-1), y.view(-1))
    return y
