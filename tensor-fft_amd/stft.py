"""ctypes binding of include/tfft_stft.h (libtfft_stft.so, the short-time Fourier transform add-on). No fallback of any kind."""
import ctypes
import os

from . import capi, conv
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_stft.so"

# every symbol include/tfft_stft.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_stft_geometry", "tfft_stft_plan_create", "tfft_stft_plan_destroy", "tfft_stft_plan_set_window", "tfft_stft_exec",
    "tfft_stft_plan_num_launches", "tfft_stft_plan_kernels", "tfft_stft_describe", "tfft_stft_last_error",
]
STFT_N = 4096                                                 # TFFT_STFT_N: the frame length of every plan
STFT_BINS = 2049                                              # TFFT_STFT_BINS: bins 0 .. n / 2
STFT_PITCH = 2056                                             # TFFT_STFT_PITCH: rplan_spectrum_pitch(4096)


class StftOpts(ctypes.Structure):
    """tfft_stft_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_sig_stride", ctypes.c_uint64),
                ("out_frame_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int)]


def stft_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


_lib = None


def load_stft_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_stft.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    conv.load_conv_library()     # first: the add-on binds to the two libraries (and the HIP runtime) this process already holds
    path = stft_lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the STFT add-on has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` from the repository root.")
    L = ctypes.CDLL(path)
    vp, u64, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
    L.tfft_stft_geometry.restype = ci
    L.tfft_stft_geometry.argtypes = [u64, u64, u64, ctypes.POINTER(u64)]
    L.tfft_stft_plan_create.restype = ci
    L.tfft_stft_plan_create.argtypes = [u64, u64, u64, u64, ci, ctypes.POINTER(StftOpts), ctypes.POINTER(vp)]
    L.tfft_stft_plan_destroy.restype = None
    L.tfft_stft_plan_destroy.argtypes = [vp]
    L.tfft_stft_plan_set_window.restype = ci
    L.tfft_stft_plan_set_window.argtypes = [vp, vp, vp]
    L.tfft_stft_exec.restype = ci
    L.tfft_stft_exec.argtypes = [vp, vp, vp, vp, vp]
    L.tfft_stft_plan_num_launches.restype = ci
    L.tfft_stft_plan_num_launches.argtypes = [vp]
    L.tfft_stft_plan_kernels.restype = ci
    L.tfft_stft_plan_kernels.argtypes = [vp, ctypes.c_char_p, sz]
    L.tfft_stft_describe.restype = ci
    L.tfft_stft_describe.argtypes = [u64, u64, u64, u64, ci, ctypes.c_char_p, sz]
    L.tfft_stft_last_error.restype = ctypes.c_char_p
    L.tfft_stft_last_error.argtypes = []
    _lib = L
    return L


def _check(rc):
    if rc != capi.TFFT_OK:
        raise TfftError(rc, load_stft_library().tfft_stft_last_error().decode())


def stft_geometry(length, hop, pad=0):
    """tfft_stft_geometry: F = 1 + (length + 2 pad - 4096) // hop, the frames per signal. Host only."""
    frames = ctypes.c_uint64()
    _check(load_stft_library().tfft_stft_geometry(int(length), int(hop), int(pad), ctypes.byref(frames)))
    return int(frames.value)


def stft_describe(length, hop, pad=0, rows=1):
    """tfft_stft_describe: "stft4096:4096 x F", F the frames per signal. Host only, no GPU needed."""
    buf = ctypes.create_string_buffer(128)
    _check(load_stft_library().tfft_stft_describe(int(length), int(hop), int(pad), int(rows), 0, buf, len(buf)))
    return buf.value.decode()


def _is_cuda_half(t):
    import torch

    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16


class TfftStftPlan:
    """Owning wrapper of tfft_stft_plan: `rows` real fp16 signals of `length` samples (a multiple of 8) -> frames of 4096 samples
    that start at f * hop - pad (zeros outside the signal), each multiplied by the window in binary16 and transformed to bins
    0 .. 2048 of rfft / 4096, in one kernel (include/tfft_stft.h). Frame g = r * frames + f of a plane lies at g * out_frame_stride
    (0 = 2 * pitch). set_window(w) takes a CUDA float16 tensor of 4096 halves before the first exec. Input and output must not
    overlap."""

    def __init__(self, rows, length, hop, pad=0, device=0, in_sig_stride=0, out_frame_stride=0, launch_iters=0):
        L = load_stft_library()
        self._lib = L
        self._h = ctypes.c_void_p()
        opts = StftOpts(ctypes.sizeof(StftOpts), 0, int(in_sig_stride), int(out_frame_stride), int(launch_iters), 0)
        _check(L.tfft_stft_plan_create(int(rows), int(length), int(hop), int(pad), int(device), ctypes.byref(opts), ctypes.byref(self._h)))
        self.rows, self.length, self.hop, self.pad = int(rows), int(length), int(hop), int(pad)
        self.device = int(device)
        self.n, self.bins, self.pitch = STFT_N, STFT_BINS, STFT_PITCH
        self.frames = stft_geometry(length, hop, pad)
        self.in_sig_stride = int(in_sig_stride) or self.length
        self.out_frame_stride = int(out_frame_stride) or 2 * self.pitch

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            self._lib.tfft_stft_plan_destroy(h)

    __del__ = close

    @property
    def num_launches(self):
        return int(self._lib.tfft_stft_plan_num_launches(self._h))

    @property
    def kernels(self):
        """tfft_stft_plan_kernels: the kernels one execution launches, in launch order."""
        return capi._kernel_lines(self._lib.tfft_stft_plan_kernels, self._h)

    def _stream(self, stream):
        import torch

        return torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream

    def set_window(self, w, stream=None):
        """Hands the window over (tfft_stft_plan_set_window): 4096 halves, copied on the stream; the tensor is not referenced by the
        plan afterwards."""
        import torch

        if not (_is_cuda_half(w) and w.is_contiguous() and w.device.index == self.device):
            raise TfftError(5, "the window must be a contiguous CUDA float16 tensor on the plan's device")
        if w.numel() != self.n:
            raise TfftError(5, "the window must hold 4096 halves")
        with torch.cuda.device(self.device):
            _check(self._lib.tfft_stft_plan_set_window(self._h, w.data_ptr(), self._stream(stream)))

    def exec_ptr(self, src, out_re, out_im, stream=0):
        _check(self._lib.tfft_stft_exec(self._h, src, out_re, out_im, stream))

    def exec(self, x, out_re, out_im, stream=None):
        """x: flat CUDA float16 tensor, signal r at r * in_sig_stride; out_re / out_im: flat planes, frame g at g * out_frame_stride,
        2049 bins each (out_im may be a view of out_re's buffer, 2056 halves on: the [RE | IM] blocks of TfftRealPlan)."""
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
            raise TfftError(5, "an output plane is shorter than (rows * frames - 1) * out_frame_stride + 2049")
        with torch.cuda.device(self.device):
            self.exec_ptr(x.data_ptr(), out_re.data_ptr(), out_im.data_ptr(), self._stream(stream))


# stft keeps the plans of the last STFT_CACHE_SIZE (rows, length, hop, pad, device) shapes, least recently used first out, each with
# the identity of the window it holds, as long_causal_conv does for its taps. A plan holds device memory outside torch's allocator
# (tables, window): a caller with many shapes should hold TfftStftPlan objects itself; stft_cache_clear() releases them.
STFT_CACHE_SIZE = 8
_plans = {}


def _plan_for(rows, length, hop, pad, device):
    key = (int(rows), int(length), int(hop), int(pad), int(device))
    entry = _plans.pop(key, None)
    if entry is None:
        entry = [TfftStftPlan(rows, length, hop, pad, device), None]
    _plans[key] = entry
    while len(_plans) > STFT_CACHE_SIZE:
        _plans.pop(next(iter(_plans)))[0].close()
    return entry


def stft_cache_clear():
    """Destroys the plans stft cached."""
    while _plans:
        _plans.popitem()[1][0].close()


def stft(x, window, hop, center=False, n_fft=STFT_N):
    """n_fft = 512, 1024 or 2048: short_stft(x, window, hop, n_fft, center) of tensor_fft_amd.stftn (include/tfft_stftn.h), with
    n_fft in the place of 4096 below; nothing of this module is touched. Any other n_fft but 4096 is refused.

    Short-time Fourier transform at frame length 4096: x a CUDA float16 tensor [R, L] (L a multiple of 8), window a CUDA float16
    tensor [win_length <= 4096] (a shorter window is zero-padded to 4096 with the window centred, as torch.stft does), hop a
    multiple of 8. center=False frames from sample 0 (torch.stft(center=False)); center=True pads 2048 zeros on both sides
    (torch.stft(center=True, pad_mode="constant")). Returns (re, im), each an [R, F, 2049] view of one new [R, F, 2, 2056] buffer:
    bins 0 .. 2048 of rfft(window * frame) / 4096. The layout is FRAME-major; torch.stft returns [R, 2049, F], bin-major, and does
    not divide by 4096. The window is handed to the cached plan again only when (data_ptr, _version) of it changed since the last
    call."""
    import torch

    if n_fft != STFT_N:
        from . import stftn

        if n_fft not in stftn.STFTN_LENGTHS:
            raise TfftError(5, "stft takes n_fft = 512, 1024, 2048 or 4096")
        return stftn.short_stft(x, window, hop, n_fft, center)
    if not (_is_cuda_half(x) and _is_cuda_half(window) and x.dim() == 2 and window.dim() == 1 and window.device == x.device):
        raise TfftError(5, "stft takes CUDA float16 tensors x (R, L) and window (win_length) on one device")
    if window.numel() == 0 or window.numel() > STFT_N:
        raise TfftError(5, "the window must hold 1 .. 4096 values")
    rows, length = x.shape
    entry = _plan_for(rows, length, hop, STFT_N // 2 if center else 0, x.device.index)
    plan = entry[0]
    # (a non-contiguous window is copied per call, and a copy's address and version say nothing about its content)
    ident = (window.data_ptr(), window._version, window.numel()) if window.is_contiguous() else None
    if ident is None or entry[1] != ident:
        w = window.contiguous()
        if w.numel() < STFT_N:
            left = (STFT_N - w.numel()) // 2
            w = torch.nn.functional.pad(w, (left, STFT_N - w.numel() - left))
        plan.set_window(w)
        entry[1] = ident
    x = x.contiguous()
    buf = torch.empty((rows, plan.frames, 2, STFT_PITCH), dtype=torch.float16, device=x.device)
    flat = buf.view(-1)
    plan.exec(x.view(-1), flat, flat[STFT_PITCH:])
    return buf[:, :, 0, :STFT_BINS], buf[:, :, 1, :STFT_BINS]
