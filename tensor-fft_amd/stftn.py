"""ctypes binding of include/tfft_stftn.h (libtfft_stftn.so, the short-frame STFT add-on: frame lengths 512, 1024 and 2048). No
fallback of any kind."""
import ctypes
import os

from . import capi, conv
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_stftn.so"

# every symbol include/tfft_stftn.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_stftn_geometry", "tfft_stftn_plan_create", "tfft_stftn_plan_destroy", "tfft_stftn_plan_set_window", "tfft_stftn_exec",
    "tfft_stftn_plan_num_launches", "tfft_stftn_plan_kernels", "tfft_stftn_describe", "tfft_stftn_last_error",
]
STFTN_LENGTHS = (512, 1024, 2048)                             # the frame lengths of a plan


def stftn_bins(n):
    """bins 0 .. n / 2 of a frame"""
    return int(n) // 2 + 1


def stftn_pitch(n):
    """tfft_rplan_spectrum_pitch(n): 264, 520, 1032"""
    return (stftn_bins(n) + 7) // 8 * 8


class StftNOpts(ctypes.Structure):
    """tfft_stftn_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_sig_stride", ctypes.c_uint64),
                ("out_frame_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int)]


def stftn_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


_lib = None


def load_stftn_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_stftn.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    conv.load_conv_library()     # first: the add-on binds to the two libraries (and the HIP runtime) this process already holds
    path = stftn_lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the short-frame STFT add-on has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` from the repository root.")
    L = ctypes.CDLL(path)
    vp, u32, u64, ci, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
    L.tfft_stftn_geometry.restype = ci
    L.tfft_stftn_geometry.argtypes = [u32, u64, u64, u64, ctypes.POINTER(u64)]
    L.tfft_stftn_plan_create.restype = ci
    L.tfft_stftn_plan_create.argtypes = [u32, u64, u64, u64, u64, ci, ctypes.POINTER(StftNOpts), ctypes.POINTER(vp)]
    L.tfft_stftn_plan_destroy.restype = None
    L.tfft_stftn_plan_destroy.argtypes = [vp]
    L.tfft_stftn_plan_set_window.restype = ci
    L.tfft_stftn_plan_set_window.argtypes = [vp, vp, vp]
    L.tfft_stftn_exec.restype = ci
    L.tfft_stftn_exec.argtypes = [vp, vp, vp, vp, vp]
    L.tfft_stftn_plan_num_launches.restype = ci
    L.tfft_stftn_plan_num_launches.argtypes = [vp]
    L.tfft_stftn_plan_kernels.restype = ci
    L.tfft_stftn_plan_kernels.argtypes = [vp, ctypes.c_char_p, sz]
    L.tfft_stftn_describe.restype = ci
    L.tfft_stftn_describe.argtypes = [u32, u64, u64, u64, u64, ci, ctypes.c_char_p, sz]
    L.tfft_stftn_last_error.restype = ctypes.c_char_p
    L.tfft_stftn_last_error.argtypes = []
    _lib = L
    return L


def _check(rc):
    if rc != capi.TFFT_OK:
        raise TfftError(rc, load_stftn_library().tfft_stftn_last_error().decode())


def _u32(n):
    """the frame length as the C ABI takes it; a value that does not fit 32 bits is as unsupported as any other"""
    n = int(n)
    return n if 0 <= n < 1 << 32 else 0


def stftn_geometry(n, length, hop, pad=0):
    """tfft_stftn_geometry: F = 1 + (length + 2 pad - n) // hop, the frames per signal. Host only."""
    frames = ctypes.c_uint64()
    _check(load_stftn_library().tfft_stftn_geometry(_u32(n), int(length), int(hop), int(pad), ctypes.byref(frames)))
    return int(frames.value)


def stftn_describe(n, length, hop, pad=0, rows=1):
    """tfft_stftn_describe: "stft256r<R>:n x F", R = n / 256 and F the frames per signal. Host only, no GPU needed."""
    buf = ctypes.create_string_buffer(128)
    _check(load_stftn_library().tfft_stftn_describe(_u32(n), int(length), int(hop), int(pad), int(rows), 0, buf, len(buf)))
    return buf.value.decode()


def _is_cuda_half(t):
    import torch

    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16


class TfftShortStftPlan:
    """Owning wrapper of tfft_stftn_plan: `rows` real fp16 signals of `length` samples (a multiple of 8) -> frames of n samples
    (512, 1024 or 2048) that start at f * hop - pad (zeros outside the signal), each multiplied by the window in binary16 and
    transformed to bins 0 .. n / 2 of rfft / n, in one kernel (include/tfft_stftn.h). Frame g = r * frames + f of a plane lies at
    g * out_frame_stride (0 = 2 * pitch). set_window(w) takes a CUDA float16 tensor of n halves before the first exec. Input and
    output must not overlap."""

    def __init__(self, n, rows, length, hop, pad=0, device=0, in_sig_stride=0, out_frame_stride=0, launch_iters=0):
        L = load_stftn_library()
        self._lib = L
        self._h = ctypes.c_void_p()
        opts = StftNOpts(ctypes.sizeof(StftNOpts), 0, int(in_sig_stride), int(out_frame_stride), int(launch_iters), 0)
        _check(L.tfft_stftn_plan_create(_u32(n), int(rows), int(length), int(hop), int(pad), int(device), ctypes.byref(opts),
                                        ctypes.byref(self._h)))
        self.n, self.rows, self.length, self.hop, self.pad = int(n), int(rows), int(length), int(hop), int(pad)
        self.device = int(device)
        self.bins, self.pitch = stftn_bins(n), stftn_pitch(n)
        self.frames = stftn_geometry(n, length, hop, pad)
        self.in_sig_stride = int(in_sig_stride) or self.length
        self.out_frame_stride = int(out_frame_stride) or 2 * self.pitch

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            self._lib.tfft_stftn_plan_destroy(h)

    __del__ = close

    @property
    def num_launches(self):
        return int(self._lib.tfft_stftn_plan_num_launches(self._h))

    @property
    def kernels(self):
        """tfft_stftn_plan_kernels: the kernels one execution launches, in launch order."""
        return capi._kernel_lines(self._lib.tfft_stftn_plan_kernels, self._h)

    def _stream(self, stream):
        import torch

        return torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream

    def set_window(self, w, stream=None):
        """Hands the window over (tfft_stftn_plan_set_window): n halves, copied on the stream; the tensor is not referenced by the
        plan afterwards."""
        import torch

        if not (_is_cuda_half(w) and w.is_contiguous() and w.device.index == self.device):
            raise TfftError(5, "the window must be a contiguous CUDA float16 tensor on the plan's device")
        if w.numel() != self.n:
            raise TfftError(5, f"the window must hold {self.n} halves")
        with torch.cuda.device(self.device):
            _check(self._lib.tfft_stftn_plan_set_window(self._h, w.data_ptr(), self._stream(stream)))

    def exec_ptr(self, src, out_re, out_im, stream=0):
        _check(self._lib.tfft_stftn_exec(self._h, src, out_re, out_im, stream))

    def exec(self, x, out_re, out_im, stream=None):
        """x: flat CUDA float16 tensor, signal r at r * in_sig_stride; out_re / out_im: flat planes, frame g at g * out_frame_stride,
        n / 2 + 1 bins each (out_im may be a view of out_re's buffer, `pitch` halves on: the [RE | IM] blocks of TfftRealPlan)."""
        import torch

        for t in (x, out_re, out_im):
            if not (_is_cuda_half(t) and t.is_contiguous()):
                raise TfftError(5, "buffers must be contiguous CUDA float16 tensors")
            if t.device.index != self.device:
                raise TfftError(5, "tensor on another device than the plan")
        if x.numel() < (self.rows - 1) * self.in_sig_stride + self.length:
            raise TfftError(5, "the signal buffer is shorter than (rows - 1) * in_sig_stride + length")
        need = (self.rows * self.frames - 1) * self.out_frame_stride + self.bins
        if out_re.numel() < need or out_im.numel() < need:
            raise TfftError(5, f"an output plane is shorter than (rows * frames - 1) * out_frame_stride + {self.bins}")
        with torch.cuda.device(self.device):
            self.exec_ptr(x.data_ptr(), out_re.data_ptr(), out_im.data_ptr(), self._stream(stream))


# short_stft keeps the plans of the last STFTN_CACHE_SIZE (n, rows, length, hop, pad, device) shapes, least recently used first out,
# each with the identity of the window it holds, as stft does. A plan holds device memory outside torch's allocator (tables, window):
# a caller with many shapes should hold TfftShortStftPlan objects itself; stftn_cache_clear() releases them.
STFTN_CACHE_SIZE = 8
_plans = {}


def _plan_for(n, rows, length, hop, pad, device):
    key = (int(n), int(rows), int(length), int(hop), int(pad), int(device))
    entry = _plans.pop(key, None)
    if entry is None:
        entry = [TfftShortStftPlan(n, rows, length, hop, pad, device), None]
    _plans[key] = entry
    while len(_plans) > STFTN_CACHE_SIZE:
        _plans.pop(next(iter(_plans)))[0].close()
    return entry


def stftn_cache_clear():
    """Destroys the plans short_stft cached."""
    while _plans:
        _plans.popitem()[1][0].close()


def short_stft(x, window, hop, n_fft, center=False):
    """Short-time Fourier transform at frame length n_fft = 512, 1024 or 2048: x a CUDA float16 tensor [R, L] (L a multiple of 8),
    window a CUDA float16 tensor [win_length <= n_fft] (a shorter window is zero-padded to n_fft with the window centred, as
    torch.stft does), hop a multiple of 8. center=False frames from sample 0 (torch.stft(center=False)); center=True pads n_fft / 2
    zeros on both sides (torch.stft(center=True, pad_mode="constant")). Returns (re, im), each an [R, F, n_fft / 2 + 1] view of one
    new [R, F, 2, h] buffer, h = rplan_spectrum_pitch(n_fft): bins 0 .. n_fft / 2 of rfft(window * frame) / n_fft. The layout is
    FRAME-major; torch.stft returns [R, bins, F], bin-major, and does not divide by n_fft. The window is handed to the cached plan
    again only when (data_ptr, _version) of it changed since the last call."""
    import torch

    n = int(n_fft)
    if n not in STFTN_LENGTHS:
        raise TfftError(5, "short_stft takes n_fft = 512, 1024 or 2048 (4096: stft)")
    if not (_is_cuda_half(x) and _is_cuda_half(window) and x.dim() == 2 and window.dim() == 1 and window.device == x.device):
        raise TfftError(5, "short_stft takes CUDA float16 tensors x (R, L) and window (win_length) on one device")
    if window.numel() == 0 or window.numel() > n:
        raise TfftError(5, f"the window must hold 1 .. {n} values")
    rows, length = x.shape
    entry = _plan_for(n, rows, length, hop, n // 2 if center else 0, x.device.index)
    plan = entry[0]
    # (a non-contiguous window is copied per call, and a copy's address and version say nothing about its content)
    ident = (window.data_ptr(), window._version, window.numel()) if window.is_contiguous() else None
    if ident is None or entry[1] != ident:
        w = window.contiguous()
        if w.numel() < n:
            left = (n - w.numel()) // 2
            w = torch.nn.functional.pad(w, (left, n - w.numel() - left))
        plan.set_window(w)
        entry[1] = ident
    x = x.contiguous()
    buf = torch.empty((rows, plan.frames, 2, plan.pitch), dtype=torch.float16, device=x.device)
    flat = buf.view(-1)
    plan.exec(x.view(-1), flat, flat[plan.pitch:])
    return buf[:, :, 0, :plan.bins], buf[:, :, 1, :plan.bins]
