"""ctypes binding of include/tfft_sconv.h (libtfft_sconv.so, the overlap-save causal convolution add-on). No fallback of any kind."""
import ctypes
import os

from . import capi, conv
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_sconv.so"

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


_lib = None


def load_sconv_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_sconv.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    conv.load_conv_library()     # first: the add-on binds to the two libraries (and the HIP runtime) this process already holds
    path = sconv_lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the overlap-save convolution add-on has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` from the repository root.")
    L = ctypes.CDLL(path)
    vp, u64, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
    pu64 = ctypes.POINTER(u64)
    L.tfft_sconv_geometry.restype = ci
    L.tfft_sconv_geometry.argtypes = [u64, u64, pu64, pu64, pu64]
    L.tfft_sconv_plan_create.restype = ci
    L.tfft_sconv_plan_create.argtypes = [u64, u64, u64, u64, ci, ctypes.POINTER(SconvOpts), ctypes.POINTER(vp)]
    L.tfft_sconv_plan_destroy.restype = None
    L.tfft_sconv_plan_destroy.argtypes = [vp]
    L.tfft_sconv_plan_set_taps.restype = ci
    L.tfft_sconv_plan_set_taps.argtypes = [vp, vp, vp]
    L.tfft_sconv_plan_spectrum.restype = ci
    L.tfft_sconv_plan_spectrum.argtypes = [vp, vp, vp]
    L.tfft_sconv_exec.restype = ci
    L.tfft_sconv_exec.argtypes = [vp, vp, vp, vp]
    L.tfft_sconv_plan_num_launches.restype = ci
    L.tfft_sconv_plan_num_launches.argtypes = [vp]
    L.tfft_sconv_plan_kernels.restype = ci
    L.tfft_sconv_plan_kernels.argtypes = [vp, ctypes.c_char_p, sz]
    L.tfft_sconv_describe.restype = ci
    L.tfft_sconv_describe.argtypes = [u64, u64, u64, u64, ci, ctypes.c_char_p, sz]
    L.tfft_sconv_last_error.restype = ctypes.c_char_p
    L.tfft_sconv_last_error.argtypes = []
    _lib = L
    return L


def _check(rc):
    if rc != capi.TFFT_OK:
        raise TfftError(rc, load_sconv_library().tfft_sconv_last_error().decode())


def sconv_geometry(length, taps):
    """tfft_sconv_geometry: (halo, hop, segments) of a plan for sequences of `length` samples and `taps` taps. Host only."""
    halo, hop, segments = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    _check(load_sconv_library().tfft_sconv_geometry(int(length), int(taps), ctypes.byref(halo), ctypes.byref(hop), ctypes.byref(segments)))
    return int(halo.value), int(hop.value), int(segments.value)


def sconv_describe(length, taps, rows=1, channels=1):
    """tfft_sconv_describe: "sconv4096:4096 x S", S the segments per sequence. Host only, no GPU needed."""
    buf = ctypes.create_string_buffer(128)
    _check(load_sconv_library().tfft_sconv_describe(int(length), int(taps), int(rows), int(channels), 0, buf, len(buf)))
    return buf.value.decode()


def _is_cuda_half(t):
    import torch

    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16


class TfftLongConvPlan:
    """Owning wrapper of tfft_sconv_plan: y[b][c][t] = sum_j h[c][j] x[b][c][t - j] for rows x channels real fp16 sequences of any
    `length` (a multiple of 8) and `taps` <= 2049 real taps per channel, by overlap-save at transform length 4096 in one kernel
    (include/tfft_sconv.h). set_taps(h) takes a CUDA float16 tensor of channels * taps halves before the first exec. Input and
    output must not overlap."""

    def __init__(self, rows, channels, length, taps, device=0, in_seq_stride=0, out_seq_stride=0, launch_iters=0):
        L = load_sconv_library()
        self._lib = L
        self._h = ctypes.c_void_p()
        opts = SconvOpts(ctypes.sizeof(SconvOpts), 0, int(in_seq_stride), int(out_seq_stride), int(launch_iters), 0)
        _check(L.tfft_sconv_plan_create(int(rows), int(channels), int(length), int(taps), int(device), ctypes.byref(opts), ctypes.byref(self._h)))
        self.rows, self.channels, self.length, self.taps = int(rows), int(channels), int(length), int(taps)
        self.device = int(device)
        self.n = SCONV_N
        self.halo, self.hop, self.segments = sconv_geometry(length, taps)
        self.in_seq_stride = int(in_seq_stride) or self.length
        self.out_seq_stride = int(out_seq_stride) or self.length

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            self._lib.tfft_sconv_plan_destroy(h)

    __del__ = close

    @property
    def num_launches(self):
        return int(self._lib.tfft_sconv_plan_num_launches(self._h))

    @property
    def kernels(self):
        """tfft_sconv_plan_kernels: the kernels one execution launches, in launch order."""
        return capi._kernel_lines(self._lib.tfft_sconv_plan_kernels, self._h)

    def _stream(self, stream):
        import torch

        return torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream

    def set_taps(self, h, stream=None):
        """Hands the taps over (tfft_sconv_plan_set_taps): [channels][taps]; the tensor is not referenced afterwards."""
        import torch

        if not (_is_cuda_half(h) and h.is_contiguous() and h.device.index == self.device):
            raise TfftError(5, "taps must be a contiguous CUDA float16 tensor on the plan's device")
        if h.numel() < self.channels * self.taps:
            raise TfftError(5, "the taps tensor is shorter than channels * taps")
        with torch.cuda.device(self.device):
            _check(self._lib.tfft_sconv_plan_set_taps(self._h, h.data_ptr(), self._stream(stream)))

    def spectrum(self):
        """tfft_sconv_plan_spectrum: (h_re, h_im), two CUDA float16 tensors [channels, 4096], what a TfftConvPlan takes as its filter."""
        import torch

        h_re = torch.empty((self.channels, self.n), dtype=torch.float16, device=f"cuda:{self.device}")
        h_im = torch.empty_like(h_re)
        with torch.cuda.device(self.device):
            _check(self._lib.tfft_sconv_plan_spectrum(self._h, h_re.data_ptr(), h_im.data_ptr()))
        return h_re, h_im

    def exec_ptr(self, src, dst, stream=0):
        _check(self._lib.tfft_sconv_exec(self._h, src, dst, stream))

    def exec(self, x, y, stream=None):
        """x, y: flat CUDA float16 tensors that share no element, sequence (b, c) at (b * channels + c) * seq stride."""
        import torch

        for t in (x, y):
            if not (_is_cuda_half(t) and t.is_contiguous()):
                raise TfftError(5, "sequences must be contiguous CUDA float16 tensors")
            if t.device.index != self.device:
                raise TfftError(5, "tensor on another device than the plan")
        seqs = self.rows * self.channels
        if x.numel() < (seqs - 1) * self.in_seq_stride + self.length or y.numel() < (seqs - 1) * self.out_seq_stride + self.length:
            raise TfftError(5, "a tensor is shorter than (rows * channels - 1) * stride + length")
        with torch.cuda.device(self.device):
            self.exec_ptr(x.data_ptr(), y.data_ptr(), self._stream(stream))


# long_causal_conv keeps the plans of the last SCONV_CACHE_SIZE (rows, channels, length, taps, device) shapes, least recently used
# first out, each with the identity of the taps it holds, as causal_conv does. A plan holds device memory outside torch's allocator
# (tables, spectra): a caller with many shapes should hold TfftLongConvPlan objects itself; sconv_cache_clear() releases them.
SCONV_CACHE_SIZE = 8
_plans = {}


def _plan_for(rows, channels, length, taps, device):
    key = (int(rows), int(channels), int(length), int(taps), int(device))
    entry = _plans.pop(key, None)
    if entry is None:
        entry = [TfftLongConvPlan(rows, channels, length, taps, device), None]
    _plans[key] = entry
    while len(_plans) > SCONV_CACHE_SIZE:
        _plans.pop(next(iter(_plans)))[0].close()
    return entry


def sconv_cache_clear():
    """Destroys the plans long_causal_conv cached."""
    while _plans:
        _plans.popitem()[1][0].close()


def long_causal_conv(x, h):
    """y[b, c, t] = sum_{j <= t} h[c, j] x[b, c, t - j]: x a CUDA float16 tensor [B, C, L] (L a multiple of 8, any length), h [C, K]
    with K <= 2049. Returns y [B, C, L], a new tensor. The taps are handed to the cached plan again only when (data_ptr, _version)
    of h changed since the last call."""
    import torch

    if not (_is_cuda_half(x) and _is_cuda_half(h) and x.dim() == 3 and h.dim() == 2 and h.shape[0] == x.shape[1] and h.device == x.device):
        raise TfftError(5, "long_causal_conv takes CUDA float16 tensors x (B, C, L) and h (C, K) on one device")
    rows, channels, length = x.shape
    entry = _plan_for(rows, channels, length, h.shape[1], x.device.index)
    plan = entry[0]
    # (a non-contiguous h is copied per call, and a copy's address and version say nothing about its content)
    ident = (h.data_ptr(), h._version) if h.is_contiguous() else None
    h = h.contiguous()
    if ident is None or entry[1] != ident:
        plan.set_taps(h.view(-1))
        entry[1] = ident
    x = x.contiguous()
    y = torch.empty_like(x)
    plan.exec(x.view(-1), y.view(-1))
    return y
