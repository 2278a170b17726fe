"""ctypes binding of include/tfft_gsconv.h (libtfft_gsconv.so, the gated overlap-save causal convolution add-on). No fallback of
any kind. What the convolution bindings share lives in _conv_common.py."""
import ctypes
import os

from . import _binding
from . import _conv_common as common
from . import conv
from ._conv_common import _flags, _flat, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_gsconv.so"
_PREFIX = "tfft_gsconv_"

# every symbol include/tfft_gsconv.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_gsconv_geometry", "tfft_gsconv_plan_create", "tfft_gsconv_plan_destroy", "tfft_gsconv_plan_set_taps", "tfft_gsconv_plan_spectrum",
    "tfft_gsconv_exec", "tfft_gsconv_plan_num_launches", "tfft_gsconv_plan_kernels", "tfft_gsconv_describe", "tfft_gsconv_last_error",
]
GSCONV_PRE_GATE, GSCONV_POST_GATE = 1, 2                      # tfft_gsconv_opts.flags
GSCONV_MAX_TAPS = 2049                                        # TFFT_GSCONV_MAX_TAPS
GSCONV_N = 4096                                               # the transform length of every plan


class GsconvOpts(ctypes.Structure):
    """tfft_gsconv_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_seq_stride", ctypes.c_uint64),
                ("out_seq_stride", ctypes.c_uint64), ("pre_seq_stride", ctypes.c_uint64), ("post_seq_stride", ctypes.c_uint64),
                ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int)]


def gsconv_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


def _prototypes():
    vp, u64, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
    pu64 = ctypes.POINTER(u64)
    return {
        "tfft_gsconv_geometry": (ci, [u64, u64, pu64, pu64, pu64]),
        "tfft_gsconv_plan_create": (ci, [u64, u64, u64, u64, ci, ctypes.POINTER(GsconvOpts), ctypes.POINTER(vp)]),
        "tfft_gsconv_plan_destroy": (None, [vp]),
        "tfft_gsconv_plan_set_taps": (ci, [vp, vp, vp, vp]),
        "tfft_gsconv_plan_spectrum": (ci, [vp, vp, vp]),
        "tfft_gsconv_exec": (ci, [vp, vp, vp, vp, vp, vp]),
        "tfft_gsconv_plan_num_launches": (ci, [vp]),
        "tfft_gsconv_plan_kernels": (ci, [vp, ctypes.c_char_p, sz]),
        "tfft_gsconv_describe": (ci, [u64, u64, u64, u64, ci, ctypes.c_char_p, sz]),
        "tfft_gsconv_last_error": (ctypes.c_char_p, []),
    }


_lib = None


def load_gsconv_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_gsconv.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is None:
        _lib = _binding._load(conv.load_conv_library, gsconv_lib_path(), "gated overlap-save convolution", _prototypes())
    return _lib


def gsconv_geometry(length, taps):
    """tfft_gsconv_geometry: (halo, hop, segments) of a plan for sequences of `length` samples and `taps` taps. Host only."""
    L = load_gsconv_library()
    halo, hop, segments = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    _binding._check(L, _PREFIX, L.tfft_gsconv_geometry(int(length), int(taps), ctypes.byref(halo), ctypes.byref(hop), ctypes.byref(segments)))
    return int(halo.value), int(hop.value), int(segments.value)


def gsconv_describe(length, taps, rows=1, channels=1, pre_gate=False, post_gate=False):
    """tfft_gsconv_describe: "gsconv4096:4096[:pre][+post] x S", S the segments per sequence. Host only, no GPU needed."""
    L = load_gsconv_library()
    buf = ctypes.create_string_buffer(128)
    _binding._check(L, _PREFIX, L.tfft_gsconv_describe(int(length), int(taps), int(rows), int(channels), _flags(pre_gate, post_gate), buf, len(buf)))
    return buf.value.decode()


class TfftGatedLongConvPlan(common._GatedTaps, common._SeqPlan):
    """Owning wrapper of tfft_gsconv_plan: y = post * (h * (pre * x) + skip (pre * x)) for rows x channels real fp16 sequences of any
    `length` (a multiple of 8), `taps` <= 2049 real taps and one skip weight per channel, by overlap-save at transform length 4096 in
    one kernel (include/tfft_gsconv.h). Which gates the plan has is fixed at creation. set_taps(h, skip) takes CUDA float16 tensors
    before the first exec. The output must not overlap the input or a gate."""
    _prefix = _PREFIX

    def __init__(self, rows, channels, length, taps, device=0, pre_gate=False, post_gate=False, in_seq_stride=0, out_seq_stride=0,
                 pre_seq_stride=0, post_seq_stride=0, launch_iters=0):
        L = load_gsconv_library()
        opts = GsconvOpts(ctypes.sizeof(GsconvOpts), 0, int(in_seq_stride), int(out_seq_stride), int(pre_seq_stride), int(post_seq_stride),
                          int(launch_iters), _flags(pre_gate, post_gate))
        self._create(L, L.tfft_gsconv_plan_create, rows, channels, length, taps, device, opts)
        self.pre_gate, self.post_gate = bool(pre_gate), bool(post_gate)
        self.n = GSCONV_N
        self.halo, self.hop, self.segments = gsconv_geometry(length, taps)
        self.in_seq_stride = int(in_seq_stride) or self.length
        self.out_seq_stride = int(out_seq_stride) or self.length
        self.pre_seq_stride = int(pre_seq_stride) or self.length
        self.post_seq_stride = int(post_seq_stride) or self.length

    def exec_ptr(self, src, dst, pre=None, post=None, stream=0):
        self._check(self._lib.tfft_gsconv_exec(self._h, src, pre, post, dst, stream))

    def exec(self, x, y, pre=None, post=None, stream=None):
        """x, y, pre, post: flat CUDA float16 tensors, sequence (b, c) at (b * channels + c) * the tensor's seq stride; y shares no
        element with the others. The library refuses a gate the plan does not have and misses one it has."""
        import torch

        for t, stride in ((x, self.in_seq_stride), (y, self.out_seq_stride), (pre, self.pre_seq_stride), (post, self.post_seq_stride)):
            self._check_seqs(t, stride)
        with torch.cuda.device(self.device):
            self.exec_ptr(x.data_ptr(), y.data_ptr(), _ptr(pre), _ptr(post), self._stream(stream))


# gated_long_causal_conv keeps the plans of the last GSCONV_CACHE_SIZE (rows, channels, length, taps, device, pre gate, post gate)
# keys, least recently used first out, each with the identity of the taps and skip it holds, as gated_causal_conv does. A plan holds
# device memory outside torch's allocator: a caller with many shapes should hold TfftGatedLongConvPlan objects itself;
# gsconv_cache_clear() releases them.
GSCONV_CACHE_SIZE = 8
_plans = {}


def _plan_for(rows, channels, length, taps, device, pre_gate, post_gate):
    key = (int(rows), int(channels), int(length), int(taps), int(device), bool(pre_gate), bool(post_gate))
    return _binding._cached(_plans, GSCONV_CACHE_SIZE, key,
                          lambda: TfftGatedLongConvPlan(rows, channels, length, taps, device, pre_gate=pre_gate, post_gate=post_gate))


def gsconv_cache_clear():
    """Destroys the plans gated_long_causal_conv cached."""
    _binding._cache_clear(_plans)


def gated_long_causal_conv(x, h, pre=None, post=None, skip=None):
    """y = post * (h * u + skip[:, None] * u) with u = pre * x and * the causal convolution along t, by overlap-save: x, pre, post
    CUDA float16 tensors [B, C, L] (L a multiple of 8, any length; a gate may be None), h [C, K] with K <= 2049, skip [C] or None.
    Returns y [B, C, L], a new tensor. Taps and skip are handed to the cached plan again only when (data_ptr, _version) of h or skip
    changed since the last call."""
    import torch

    common._check_tap_args("gated_long_causal_conv takes CUDA float16 tensors x, pre, post (B, C, L), h (C, K) and skip (C,) on one device",
                           (x,), (pre, post), h, skip)
    rows, channels, length = x.shape
    entry = _plan_for(rows, channels, length, h.shape[1], x.device.index, pre is not None, post is not None)
    common._hand_taps(entry, h, skip)
    x = x.contiguous()
    y = torch.empty_like(x)
    entry[0].exec(x.view(-1), y.view(-1), _flat(pre), _flat(post))
    return y
