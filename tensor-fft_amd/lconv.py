"""ctypes binding of include/tfft_lconv.h (libtfft_lconv.so, the causal real convolution add-on). No fallback of any kind."""
import ctypes
import os

from . import capi, conv
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_lconv.so"

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


_lib = None


def load_lconv_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_lconv.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    conv.load_conv_library()     # first: the add-on binds to the two libraries (and the HIP runtime) this process already holds
    path = lconv_lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the causal convolution add-on has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` from the repository root.")
    L = ctypes.CDLL(path)
    vp, u64, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
    L.tfft_lconv_fft_length.restype = u64
    L.tfft_lconv_fft_length.argtypes = [u64, u64]
    L.tfft_lconv_plan_create.restype = ci
    L.tfft_lconv_plan_create.argtypes = [u64, u64, u64, u64, ci, ctypes.POINTER(LconvOpts), ctypes.POINTER(vp)]
    L.tfft_lconv_plan_destroy.restype = None
    L.tfft_lconv_plan_destroy.argtypes = [vp]
    L.tfft_lconv_plan_set_taps.restype = ci
    L.tfft_lconv_plan_set_taps.argtypes = [vp, vp, vp]
    L.tfft_lconv_plan_spectrum.restype = ci
    L.tfft_lconv_plan_spectrum.argtypes = [vp, vp, vp]
    L.tfft_lconv_spectrum_host.restype = ci
    L.tfft_lconv_spectrum_host.argtypes = [vp, u64, u64, vp, vp]
    L.tfft_lconv_plan_fft_length.restype = u64
    L.tfft_lconv_plan_fft_length.argtypes = [vp]
    L.tfft_lconv_plan_workspace_bytes.restype = sz
    L.tfft_lconv_plan_workspace_bytes.argtypes = [vp]
    L.tfft_lconv_plan_set_workspace.restype = ci
    L.tfft_lconv_plan_set_workspace.argtypes = [vp, vp, sz]
    L.tfft_lconv_plan_prepare.restype = ci
    L.tfft_lconv_plan_prepare.argtypes = [vp]
    L.tfft_lconv_exec.restype = ci
    L.tfft_lconv_exec.argtypes = [vp, vp, vp, vp]
    L.tfft_lconv_plan_num_launches.restype = ci
    L.tfft_lconv_plan_num_launches.argtypes = [vp]
    L.tfft_lconv_plan_kernels.restype = ci
    L.tfft_lconv_plan_kernels.argtypes = [vp, ctypes.c_char_p, sz]
    L.tfft_lconv_describe.restype = ci
    L.tfft_lconv_describe.argtypes = [u64, u64, u64, u64, ci, ctypes.c_char_p, sz]
    L.tfft_lconv_last_error.restype = ctypes.c_char_p
    L.tfft_lconv_last_error.argtypes = []
    _lib = L
    return L


def _check(rc):
    if rc != capi.TFFT_OK:
        raise TfftError(rc, load_lconv_library().tfft_lconv_last_error().decode())


def lconv_fft_length(length, taps):
    """tfft_lconv_fft_length: the smallest power of two >= max(length + taps - 1, 256), the composed path's transform length; 0 for
    shapes no plan accepts. Host only."""
    return int(load_lconv_library().tfft_lconv_fft_length(int(length), int(taps)))


def lconv_describe(length, taps, rows=1, channels=1, composed=False):
    """tfft_lconv_describe: "lconv4096:4096" or "pack | <the sub-plan's description> | crop". Host only, no GPU needed."""
    buf = ctypes.create_string_buffer(512)
    _check(load_lconv_library().tfft_lconv_describe(int(length), int(taps), int(rows), int(channels), LCONV_COMPOSED if composed else 0,
                                                    buf, len(buf)))
    return buf.value.decode()


def lconv_spectrum_host(taps, n):
    """tfft_lconv_spectrum_host: (re, im) float16 arrays of n bins, the binary16 spectrum a plan builds from one filter's taps."""
    import numpy as np

    taps = np.ascontiguousarray(taps, dtype=np.float16)
    re, im = np.empty(int(n), np.float16), np.empty(int(n), np.float16)
    _check(load_lconv_library().tfft_lconv_spectrum_host(taps.ctypes.data, taps.size, int(n), re.ctypes.data, im.ctypes.data))
    return re, im


def _is_cuda_half(t):
    import torch

    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16


class TfftCausalConvPlan:
    """Owning wrapper of tfft_lconv_plan: y[b][c][t] = sum_j h[c][j] x[b][c][t - j] for rows x channels real fp16 sequences of
    `length` samples and `taps` real taps per channel (include/tfft_lconv.h). set_taps(h) takes a CUDA float16 tensor of
    channels * taps halves before the first exec. length <= 2048 with length + taps - 1 <= 4096 runs as one fused kernel unless composed=True."""

    def __init__(self, rows, channels, length, taps, device=0, in_seq_stride=0, out_seq_stride=0, launch_iters=0, composed=False):
        L = load_lconv_library()
        self._lib = L
        self._h = ctypes.c_void_p()
        opts = LconvOpts(ctypes.sizeof(LconvOpts), 0, int(in_seq_stride), int(out_seq_stride), int(launch_iters), LCONV_COMPOSED if composed else 0)
        _check(L.tfft_lconv_plan_create(int(rows), int(channels), int(length), int(taps), int(device), ctypes.byref(opts), ctypes.byref(self._h)))
        self.rows, self.channels, self.length, self.taps = int(rows), int(channels), int(length), int(taps)
        self.device, self.composed = int(device), bool(composed)
        self.n = int(L.tfft_lconv_plan_fft_length(self._h))       # 4096 for the fused kernel, else lconv_fft_length(length, taps)
        self.in_seq_stride = int(in_seq_stride) or self.length
        self.out_seq_stride = int(out_seq_stride) or self.length
        self._ws = None

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            self._lib.tfft_lconv_plan_destroy(h)

    __del__ = close

    @property
    def num_launches(self):
        return int(self._lib.tfft_lconv_plan_num_launches(self._h))

    @property
    def workspace_bytes(self):
        return int(self._lib.tfft_lconv_plan_workspace_bytes(self._h))

    @property
    def kernels(self):
        """tfft_lconv_plan_kernels: the kernels one execution launches, in launch order."""
        return capi._kernel_lines(self._lib.tfft_lconv_plan_kernels, self._h)

    def _stream(self, stream):
        import torch

        return torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream

    def set_taps(self, h, stream=None):
        """Hands the taps over (tfft_lconv_plan_set_taps): [channels][taps]; the tensor is not referenced afterwards."""
        import torch

        if not (_is_cuda_half(h) and h.is_contiguous() and h.device.index == self.device):
            raise TfftError(5, "taps must be a contiguous CUDA float16 tensor on the plan's device")
        if h.numel() < self.channels * self.taps:
            raise TfftError(5, "the taps tensor is shorter than channels * taps")
        with torch.cuda.device(self.device):
            _check(self._lib.tfft_lconv_plan_set_taps(self._h, h.data_ptr(), self._stream(stream)))

    def spectrum(self):
        """tfft_lconv_plan_spectrum: (h_re, h_im), two CUDA float16 tensors [channels, n], what a TfftConvPlan takes as its filter."""
        import torch

        h_re = torch.empty((self.channels, self.n), dtype=torch.float16, device=f"cuda:{self.device}")
        h_im = torch.empty_like(h_re)
        with torch.cuda.device(self.device):
            _check(self._lib.tfft_lconv_plan_spectrum(self._h, h_re.data_ptr(), h_im.data_ptr()))
        return h_re, h_im

    def set_workspace(self, tensor):
        """Hands a torch CUDA tensor in as the plan's workspace (kept alive by the plan)."""
        _check(self._lib.tfft_lconv_plan_set_workspace(self._h, tensor.data_ptr(), tensor.numel() * tensor.element_size()))
        self._ws = tensor

    def prepare(self):
        """Allocates the plan's own workspace now (tfft_lconv_plan_prepare): later executions only launch kernels."""
        _check(self._lib.tfft_lconv_plan_prepare(self._h))

    def exec_ptr(self, src, dst, stream=0):
        _check(self._lib.tfft_lconv_exec(self._h, src, dst, stream))

    def exec(self, x, y, stream=None):
        """x, y: flat CUDA float16 tensors, sequence (b, c) at (b * channels + c) * seq stride."""
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


# causal_conv keeps the plans of the last LCONV_CACHE_SIZE (rows, channels, length, taps, device) shapes, least recently used first
# out, each with the identity of the taps it holds. A plan holds device memory outside torch's allocator (tables, spectra, a workspace
# on the composed path): a caller with many shapes should hold TfftCausalConvPlan objects itself; lconv_cache_clear() releases them.
LCONV_CACHE_SIZE = 8
_plans = {}


def _plan_for(rows, channels, length, taps, device):
    key = (int(rows), int(channels), int(length), int(taps), int(device))
    entry = _plans.pop(key, None)
    if entry is None:
        entry = [TfftCausalConvPlan(rows, channels, length, taps, device), None]
    _plans[key] = entry
    while len(_plans) > LCONV_CACHE_SIZE:
        _plans.pop(next(iter(_plans)))[0].close()
    return entry


def lconv_cache_clear():
    """Destroys the plans causal_conv cached."""
    while _plans:
        _plans.popitem()[1][0].close()


def causal_conv(x, h):
    """y[b, c, t] = sum_{j <= t} h[c, j] x[b, c, t - j]: x a CUDA float16 tensor [B, C, L] (L a multiple of 8), h [C, K]. Returns
    y [B, C, L]. The taps are handed to the cached plan again only when (data_ptr, _version) of h changed since the last call."""
    import torch

    if not (_is_cuda_half(x) and _is_cuda_half(h) and x.dim() == 3 and h.dim() == 2 and h.shape[0] == x.shape[1] and h.device == x.device):
        raise TfftError(5, "causal_conv takes CUDA float16 tensors x (B, C, L) and h (C, K) on one device")
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
