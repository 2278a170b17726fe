"""ctypes binding of include/tfft_gconv.h (libtfft_gconv.so, the gated causal convolution add-on). No fallback of any kind. What
the convolution bindings share lives in _conv_common.py."""
import ctypes
import os

from . import _binding
from . import _conv_common as common
from . import conv
from ._conv_common import _flags, _flat, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_gconv.so"
_PREFIX = "tfft_gconv_"

# every symbol include/tfft_gconv.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_gconv_fft_length", "tfft_gconv_plan_create", "tfft_gconv_plan_destroy", "tfft_gconv_plan_set_taps", "tfft_gconv_plan_spectrum",
    "tfft_gconv_spectrum_host", "tfft_gconv_plan_fft_length", "tfft_gconv_plan_workspace_bytes", "tfft_gconv_plan_set_workspace", "tfft_gconv_plan_prepare",
    "tfft_gconv_exec", "tfft_gconv_plan_num_launches", "tfft_gconv_plan_kernels", "tfft_gconv_describe", "tfft_gconv_last_error",
]
GCONV_PRE_GATE, GCONV_POST_GATE, GCONV_COMPOSED = 1, 2, 4     # tfft_gconv_opts.flags


class GconvOpts(ctypes.Structure):
    """tfft_gconv_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_seq_stride", ctypes.c_uint64),
                ("out_seq_stride", ctypes.c_uint64), ("pre_seq_stride", ctypes.c_uint64), ("post_seq_stride", ctypes.c_uint64),
                ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int)]


def gconv_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


def _prototypes():
    vp, u64, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
    return {
        "tfft_gconv_fft_length": (u64, [u64, u64]),
        "tfft_gconv_plan_create": (ci, [u64, u64, u64, u64, ci, ctypes.POINTER(GconvOpts), ctypes.POINTER(vp)]),
        "tfft_gconv_plan_destroy": (None, [vp]),
        "tfft_gconv_plan_set_taps": (ci, [vp, vp, vp, vp]),
        "tfft_gconv_plan_spectrum": (ci, [vp, vp, vp]),
        "tfft_gconv_spectrum_host": (ci, [vp, u64, vp, u64, vp, vp]),
        "tfft_gconv_plan_fft_length": (u64, [vp]),
        "tfft_gconv_plan_workspace_bytes": (sz, [vp]),
        "tfft_gconv_plan_set_workspace": (ci, [vp, vp, sz]),
        "tfft_gconv_plan_prepare": (ci, [vp]),
        "tfft_gconv_exec": (ci, [vp, vp, vp, vp, vp, vp]),
        "tfft_gconv_plan_num_launches": (ci, [vp]),
        "tfft_gconv_plan_kernels": (ci, [vp, ctypes.c_char_p, sz]),
        "tfft_gconv_describe": (ci, [u64, u64, u64, u64, ci, ctypes.c_char_p, sz]),
        "tfft_gconv_last_error": (ctypes.c_char_p, []),
    }


_lib = None


def load_gconv_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_gconv.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is None:
        _lib = _binding._load(conv.load_conv_library, gconv_lib_path(), "gated causal convolution", _prototypes())
    return _lib


def gconv_fft_length(length, taps):
    """tfft_gconv_fft_length: the smallest power of two >= max(length + taps - 1, 256), the composed path's transform length; 0 for
    shapes no plan accepts. Host only."""
    return int(load_gconv_library().tfft_gconv_fft_length(int(length), int(taps)))


def gconv_describe(length, taps, rows=1, channels=1, pre_gate=False, post_gate=False, composed=False):
    """tfft_gconv_describe: "gconv4096:4096[:pre][+post]" or "pack[:pre] | <the sub-plan's description> | crop[:post]". Host only, no
    GPU needed."""
    L = load_gconv_library()
    buf = ctypes.create_string_buffer(512)
    _binding._check(L, _PREFIX, L.tfft_gconv_describe(int(length), int(taps), int(rows), int(channels), _flags(pre_gate, post_gate, composed),
                                                    buf, len(buf)))
    return buf.value.decode()


def gconv_spectrum_host(taps, n, skip=None):
    """tfft_gconv_spectrum_host: (re, im) float16 arrays of n bins, the binary16 spectrum a plan builds from one filter's taps with
    the skip weight (a number exact in binary16, or None) added to tap 0 in fp64."""
    import numpy as np

    L = load_gconv_library()
    taps = np.ascontiguousarray(taps, dtype=np.float16)
    re, im = np.empty(int(n), np.float16), np.empty(int(n), np.float16)
    d = None if skip is None else np.array([skip], dtype=np.float16)
    _binding._check(L, _PREFIX, L.tfft_gconv_spectrum_host(taps.ctypes.data, taps.size, None if d is None else d.ctypes.data, int(n),
                                                         re.ctypes.data, im.ctypes.data))
    return re, im


class TfftGatedConvPlan(common._GatedTaps, _binding._Workspace, common._SeqPlan):
    """Owning wrapper of tfft_gconv_plan: y = post * (h * (pre * x) + skip (pre * x)) for rows x channels real fp16 sequences of
    `length` samples, `taps` real taps and one skip weight per channel (include/tfft_gconv.h). Which gates the plan has is fixed at
    creation. set_taps(h, skip) takes CUDA float16 tensors before the first exec. length <= 2048 with length + taps - 1 <= 4096 runs
    as one fused kernel unless composed=True."""
    _prefix = _PREFIX

    def __init__(self, rows, channels, length, taps, device=0, pre_gate=False, post_gate=False, composed=False, in_seq_stride=0,
                 out_seq_stride=0, pre_seq_stride=0, post_seq_stride=0, launch_iters=0):
        L = load_gconv_library()
        opts = GconvOpts(ctypes.sizeof(GconvOpts), 0, int(in_seq_stride), int(out_seq_stride), int(pre_seq_stride), int(post_seq_stride),
                         int(launch_iters), _flags(pre_gate, post_gate, composed))
        self._create(L, L.tfft_gconv_plan_create, rows, channels, length, taps, device, opts)
        self.composed = bool(composed)
        self.pre_gate, self.post_gate = bool(pre_gate), bool(post_gate)
        self.n = int(L.tfft_gconv_plan_fft_length(self._h))       # 4096 for the fused kernel, else gconv_fft_length(length, taps)
        self.in_seq_stride = int(in_seq_stride) or self.length
        self.out_seq_stride = int(out_seq_stride) or self.length
        self.pre_seq_stride = int(pre_seq_stride) or self.length
        self.post_seq_stride = int(post_seq_stride) or self.length

    def exec_ptr(self, src, dst, pre=None, post=None, stream=0):
        self._check(self._lib.tfft_gconv_exec(self._h, src, pre, post, dst, stream))

    def exec(self, x, y, pre=None, post=None, stream=None):
        """x, y, pre, post: flat CUDA float16 tensors, sequence (b, c) at (b * channels + c) * the tensor's seq stride. The library
        refuses a gate the plan does not have and misses one it has."""
        import torch

        for t, stride in ((x, self.in_seq_stride), (y, self.out_seq_stride), (pre, self.pre_seq_stride), (post, self.post_seq_stride)):
            self._check_seqs(t, stride)
        with torch.cuda.device(self.device):
            self.exec_ptr(x.data_ptr(), y.data_ptr(), _ptr(pre), _ptr(post), self._stream(stream))


# gated_causal_conv keeps the plans of the last GCONV_CACHE_SIZE (rows, channels, length, taps, device, pre gate, post gate) keys,
# least recently used first out, each with the identity of the taps and skip it holds. A plan holds device memory outside torch's
# allocator: a caller with many shapes should hold TfftGatedConvPlan objects itself; gconv_cache_clear() releases them.
GCONV_CACHE_SIZE = 8
_plans = {}


def _plan_for(rows, channels, length, taps, device, pre_gate, post_gate):
    key = (int(rows), int(channels), int(length), int(taps), int(device), bool(pre_gate), bool(post_gate))
    return _binding._cached(_plans, GCONV_CACHE_SIZE, key,
                          lambda: TfftGatedConvPlan(rows, channels, length, taps, device, pre_gate=pre_gate, post_gate=post_gate))


def gconv_cache_clear():
    """Destroys the plans gated_causal_conv cached."""
    _binding._cache_clear(_plans)


def gated_causal_conv(x, h, pre=None, post=None, skip=None):
    """y = post * (h * u + skip[:, None] * u) with u = pre * x and * the causal convolution along t: x, pre, post CUDA float16
    tensors [B, C, L] (L a multiple of 8; a gate may be None), h [C, K], skip [C] or None. Returns y [B, C, L]. Taps and skip are
    handed to the cached plan again only when (data_ptr, _version) of h or skip changed since the last call."""
    import torch

    common._check_tap_args("gated_causal_conv takes CUDA float16 tensors x, pre, post (B, C, L), h (C, K) and skip (C,) on one device",
                           (x,), (pre, post), h, skip)
    rows, channels, length = x.shape
    entry = _plan_for(rows, channels, length, h.shape[1], x.device.index, pre is not None, post is not None)
    common._hand_taps(entry, h, skip)
    x = x.contiguous()
    y = torch.empty_like(x)
    entry[0].exec(x.view(-1), y.view(-1), _flat(pre), _flat(post))
    return y
