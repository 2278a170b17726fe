"""ctypes binding of include/tfft_gsconv.h (libtfft_gsconv.so, the gated overlap-save causal convolution add-on). No fallback of
any kind."""
import ctypes
import os

from . import capi, conv
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_gsconv.so"

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


_lib = None


def load_gsconv_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_gsconv.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    conv.load_conv_library()     # first: the add-on binds to the two libraries (and the HIP runtime) this process already holds
    path = gsconv_lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the gated overlap-save convolution add-on has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` from the repository root.")
    L = ctypes.CDLL(path)
    vp, u64, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
    pu64 = ctypes.POINTER(u64)
    L.tfft_gsconv_geometry.restype = ci
    L.tfft_gsconv_geometry.argtypes = [u64, u64, pu64, pu64, pu64]
    L.tfft_gsconv_plan_create.restype = ci
    L.tfft_gsconv_plan_create.argtypes = [u64, u64, u64, u64, ci, ctypes.POINTER(GsconvOpts), ctypes.POINTER(vp)]
    L.tfft_gsconv_plan_destroy.restype = None
    L.tfft_gsconv_plan_destroy.argtypes = [vp]
    L.tfft_gsconv_plan_set_taps.restype = ci
    L.tfft_gsconv_plan_set_taps.argtypes = [vp, vp, vp, vp]
    L.tfft_gsconv_plan_spectrum.restype = ci
    L.tfft_gsconv_plan_spectrum.argtypes = [vp, vp, vp]
    L.tfft_gsconv_exec.restype = ci
    L.tfft_gsconv_exec.argtypes = [vp, vp, vp, vp, vp, vp]
    L.tfft_gsconv_plan_num_launches.restype = ci
    L.tfft_gsconv_plan_num_launches.argtypes = [vp]
    L.tfft_gsconv_plan_kernels.restype = ci
    L.tfft_gsconv_plan_kernels.argtypes = [vp, ctypes.c_char_p, sz]
    L.tfft_gsconv_describe.restype = ci
    L.tfft_gsconv_describe.argtypes = [u64, u64, u64, u64, ci, ctypes.c_char_p, sz]
    L.tfft_gsconv_last_error.restype = ctypes.c_char_p
    L.tfft_gsconv_last_error.argtypes = []
    _lib = L
    return L


def _check(rc):
    if rc != capi.TFFT_OK:
        raise TfftError(rc, load_gsconv_library().tfft_gsconv_last_error().decode())


def _flags(pre_gate, post_gate):
    return (GSCONV_PRE_GATE if pre_gate else 0) | (GSCONV_POST_GATE if post_gate else 0)


def gsconv_geometry(length, taps):
    """tfft_gsconv_geometry: (halo, hop, segments) of a plan for sequences of `length` samples and `taps` taps. Host only."""
    halo, hop, segments = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    _check(load_gsconv_library().tfft_gsconv_geometry(int(length), int(taps), ctypes.byref(halo), ctypes.byref(hop), ctypes.byref(segments)))
    return int(halo.value), int(hop.value), int(segments.value)


def gsconv_describe(length, taps, rows=1, channels=1, pre_gate=False, post_gate=False):
    """tfft_gsconv_describe: "gsconv4096:4096[:pre][+post] x S", S the segments per sequence. Host only, no GPU needed."""
    buf = ctypes.create_string_buffer(128)
    _check(load_gsconv_library().tfft_gsconv_describe(int(length), int(taps), int(rows), int(channels), _flags(pre_gate, post_gate), buf, len(buf)))
    return buf.value.decode()


def _is_cuda_half(t):
    import torch

    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16


class TfftGatedLongConvPlan:
    """Owning wrapper of tfft_gsconv_plan: y = post * (h * (pre * x) + skip (pre * x)) for rows x channels real fp16 sequences of any
    `length` (a multiple of 8), `taps` <= 2049 real taps and one skip weight per channel, by overlap-save at transform length 4096 in
    one kernel (include/tfft_gsconv.h). Which gates the plan has is fixed at creation. set_taps(h, skip) takes CUDA float16 tensors
    before the first exec. The output must not overlap the input or a gate."""

    def __init__(self, rows, channels, length, taps, device=0, pre_gate=False, post_gate=False, in_seq_stride=0, out_seq_stride=0,
                 pre_seq_stride=0, post_seq_stride=0, launch_iters=0):
        L = load_gsconv_library()
        self._lib = L
        self._h = ctypes.c_void_p()
        opts = GsconvOpts(ctypes.sizeof(GsconvOpts), 0, int(in_seq_stride), int(out_seq_stride), int(pre_seq_stride), int(post_seq_stride),
                          int(launch_iters), _flags(pre_gate, post_gate))
        _check(L.tfft_gsconv_plan_create(int(rows), int(channels), int(length), int(taps), int(device), ctypes.byref(opts), ctypes.byref(self._h)))
        self.rows, self.channels, self.length, self.taps = int(rows), int(channels), int(length), int(taps)
        self.device = int(device)
        self.pre_gate, self.post_gate = bool(pre_gate), bool(post_gate)
        self.n = GSCONV_N
        self.halo, self.hop, self.segments = gsconv_geometry(length, taps)
        self.in_seq_stride = int(in_seq_stride) or self.length
        self.out_seq_stride = int(out_seq_stride) or self.length
        self.pre_seq_stride = int(pre_seq_stride) or self.length
        self.post_seq_stride = int(post_seq_stride) or self.length

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            self._lib.tfft_gsconv_plan_destroy(h)

    __del__ = close

    @property
    def num_launches(self):
        return int(self._lib.tfft_gsconv_plan_num_launches(self._h))

    @property
    def kernels(self):
        """tfft_gsconv_plan_kernels: the kernels one execution launches, in launch order."""
        return capi._kernel_lines(self._lib.tfft_gsconv_plan_kernels, self._h)

    def _stream(self, stream):
        import torch

        return torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream

    def set_taps(self, h, skip=None, stream=None):
        """Hands the taps [channels][taps] and the skip weights [channels] (or None) over (tfft_gsconv_plan_set_taps); the tensors
        are not referenced afterwards."""
        import torch

        for t, count, what in ((h, self.channels * self.taps, "taps"), (skip, self.channels, "skip")):
            if t is None and what == "skip":
                continue
            if not (_is_cuda_half(t) and t.is_contiguous() and t.device.index == self.device):
                raise TfftError(5, f"{what} must be a contiguous CUDA float16 tensor on the plan's device")
            if t.numel() < count:
                raise TfftError(5, f"the {what} tensor is shorter than channels{' * taps' if what == 'taps' else ''}")
        with torch.cuda.device(self.device):
            _check(self._lib.tfft_gsconv_plan_set_taps(self._h, h.data_ptr(), None if skip is None else skip.data_ptr(), self._stream(stream)))

    def spectrum(self):
        """tfft_gsconv_plan_spectrum: (h_re, h_im), two CUDA float16 tensors [channels, 4096], what a TfftConvPlan takes as its filter."""
        import torch

        h_re = torch.empty((self.channels, self.n), dtype=torch.float16, device=f"cuda:{self.device}")
        h_im = torch.empty_like(h_re)
        with torch.cuda.device(self.device):
            _check(self._lib.tfft_gsconv_plan_spectrum(self._h, h_re.data_ptr(), h_im.data_ptr()))
        return h_re, h_im

    def exec_ptr(self, src, dst, pre=None, post=None, stream=0):
        _check(self._lib.tfft_gsconv_exec(self._h, src, pre, post, dst, stream))

    def exec(self, x, y, pre=None, post=None, stream=None):
        """x, y, pre, post: flat CUDA float16 tensors, sequence (b, c) at (b * channels + c) * the tensor's seq stride; y shares no
        element with the others. The library refuses a gate the plan does not have and misses one it has."""
        import torch

        seqs = self.rows * self.channels
        for t, stride in ((x, self.in_seq_stride), (y, self.out_seq_stride), (pre, self.pre_seq_stride), (post, self.post_seq_stride)):
            if t is None:
                continue
            if not (_is_cuda_half(t) and t.is_contiguous()):
                raise TfftError(5, "sequences and gates must be contiguous CUDA float16 tensors")
            if t.device.index != self.device:
                raise TfftError(5, "tensor on another device than the plan")
            if t.numel() < (seqs - 1) * stride + self.length:
                raise TfftError(5, "a tensor is shorter than (rows * channels - 1) * stride + length")
        with torch.cuda.device(self.device):
            self.exec_ptr(x.data_ptr(), y.data_ptr(), None if pre is None else pre.data_ptr(), None if post is None else post.data_ptr(),
                          self._stream(stream))


# gated_long_causal_conv keeps the plans of the last GSCONV_CACHE_SIZE (rows, channels, length, taps, device, pre gate, post gate)
# keys, least recently used first out, each with the identity of the taps and skip it holds, as gated_causal_conv does. A plan holds
# device memory outside torch's allocator: a caller with many shapes should hold TfftGatedLongConvPlan objects itself;
# gsconv_cache_clear() releases them.
GSCONV_CACHE_SIZE = 8
_plans = {}


def _plan_for(rows, channels, length, taps, device, pre_gate, post_gate):
    key = (int(rows), int(channels), int(length), int(taps), int(device), bool(pre_gate), bool(post_gate))
    entry = _plans.pop(key, None)
    if entry is None:
        entry = [TfftGatedLongConvPlan(rows, channels, length, taps, device, pre_gate=pre_gate, post_gate=post_gate), None]
    _plans[key] = entry
    while len(_plans) > GSCONV_CACHE_SIZE:
        _plans.pop(next(iter(_plans)))[0].close()
    return entry


def gsconv_cache_clear():
    """Destroys the plans gated_long_causal_conv cached."""
    while _plans:
        _plans.popitem()[1][0].close()


def gated_long_causal_conv(x, h, pre=None, post=None, skip=None):
    """y = post * (h * u + skip[:, None] * u) with u = pre * x and * the causal convolution along t, by overlap-save: x, pre, post
    CUDA float16 tensors [B, C, L] (L a multiple of 8, any length; a gate may be None), h [C, K] with K <= 2049, skip [C] or None.
    Returns y [B, C, L], a new tensor. Taps and skip are handed to the cached plan again only when (data_ptr, _version) of h or skip
    changed since the last call."""
    import torch

    ok = _is_cuda_half(x) and _is_cuda_half(h) and x.dim() == 3 and h.dim() == 2 and h.shape[0] == x.shape[1] and h.device == x.device
    for gate in (pre, post):
        ok = ok and (gate is None or (_is_cuda_half(gate) and gate.shape == x.shape and gate.device == x.device))
    ok = ok and (skip is None or (_is_cuda_half(skip) and skip.shape == (x.shape[1],) and skip.device == x.device))
    if not ok:
        raise TfftError(5, "gated_long_causal_conv takes CUDA float16 tensors x, pre, post (B, C, L), h (C, K) and skip (C,) on one device")
    rows, channels, length = x.shape
    entry = _plan_for(rows, channels, length, h.shape[1], x.device.index, pre is not None, post is not None)
    plan = entry[0]
    # (a non-contiguous tensor is copied per call, and a copy's address and version say nothing about its content)
    ident = (h.data_ptr(), h._version, None if skip is None else (skip.data_ptr(), skip._version))
    if not h.is_contiguous() or not (skip is None or skip.is_contiguous()):
        ident = None
    if ident is None or entry[1] != ident:
        plan.set_taps(h.contiguous().view(-1), None if skip is None else skip.contiguous())
        entry[1] = ident
    x = x.contiguous()
    y = torch.empty_like(x)
    plan.exec(x.view(-1), y.view(-1), None if pre is None else pre.contiguous().view(-1), None if post is None else post.contiguous().view(-1))
    return y
