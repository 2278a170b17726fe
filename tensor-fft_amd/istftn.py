"""ctypes binding of include/tfft_istftn.h (libtfft_istftn.so, the short-frame inverse STFT add-on: frame lengths 512, 1024 and
2048). No fallback of any kind."""
import ctypes
import os

from . import capi, conv
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_istftn.so"

# every symbol include/tfft_istftn.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_istftn_geometry", "tfft_istftn_plan_create", "tfft_istftn_plan_destroy", "tfft_istftn_plan_set_window",
    "tfft_istftn_plan_workspace_bytes", "tfft_istftn_plan_set_workspace", "tfft_istftn_plan_prepare", "tfft_istftn_exec",
    "tfft_istftn_plan_num_launches", "tfft_istftn_plan_kernels", "tfft_istftn_describe", "tfft_istftn_last_error",
]
ISTFTN_LENGTHS = (512, 1024, 2048)                            # the frame lengths of a plan
ISTFTN_RAW_SUM = 1                                            # TFFT_ISTFTN_RAW_SUM: no division by the window envelope


def istftn_bins(n):
    """bins 0 .. n / 2 of a frame"""
    return int(n) // 2 + 1


def istftn_pitch(n):
    """tfft_rplan_spectrum_pitch(n): 264, 520, 1032"""
    return (istftn_bins(n) + 7) // 8 * 8


class IstftNOpts(ctypes.Structure):
    """tfft_istftn_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_frame_stride", ctypes.c_uint64),
                ("out_sig_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int)]


def istftn_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


_lib = None


def load_istftn_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_istftn.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    conv.load_conv_library()     # first: the add-on binds to the two libraries (and the HIP runtime) this process already holds
    path = istftn_lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the short-frame ISTFT add-on has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` from the repository root.")
    L = ctypes.CDLL(path)
    vp, u32, u64, ci, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
    L.tfft_istftn_geometry.restype = ci
    L.tfft_istftn_geometry.argtypes = [u32, u64, u64, u64, ctypes.POINTER(u64)]
    L.tfft_istftn_plan_create.restype = ci
    L.tfft_istftn_plan_create.argtypes = [u32, u64, u64, u64, u64, ci, ctypes.POINTER(IstftNOpts), ctypes.POINTER(vp)]
    L.tfft_istftn_plan_destroy.restype = None
    L.tfft_istftn_plan_destroy.argtypes = [vp]
    L.tfft_istftn_plan_set_window.restype = ci
    L.tfft_istftn_plan_set_window.argtypes = [vp, vp, vp]
    L.tfft_istftn_plan_workspace_bytes.restype = sz
    L.tfft_istftn_plan_workspace_bytes.argtypes = [vp]
    L.tfft_istftn_plan_set_workspace.restype = ci
    L.tfft_istftn_plan_set_workspace.argtypes = [vp, vp, sz]
    L.tfft_istftn_plan_prepare.restype = ci
    L.tfft_istftn_plan_prepare.argtypes = [vp]
    L.tfft_istftn_exec.restype = ci
    L.tfft_istftn_exec.argtypes = [vp, vp, vp, vp, vp]
    L.tfft_istftn_plan_num_launches.restype = ci
    L.tfft_istftn_plan_num_launches.argtypes = [vp]
    L.tfft_istftn_plan_kernels.restype = ci
    L.tfft_istftn_plan_kernels.argtypes = [vp, ctypes.c_char_p, sz]
    L.tfft_istftn_describe.restype = ci
    L.tfft_istftn_describe.argtypes = [u32, u64, u64, u64, u64, ci, ctypes.c_char_p, sz]
    L.tfft_istftn_last_error.restype = ctypes.c_char_p
    L.tfft_istftn_last_error.argtypes = []
    _lib = L
    return L


def _check(rc):
    if rc != capi.TFFT_OK:
        raise TfftError(rc, load_istftn_library().tfft_istftn_last_error().decode())


def _u32(n):
    """the frame length as the C ABI takes it; a value that does not fit 32 bits is as unsupported as any other"""
    n = int(n)
    return n if 0 <= n < 1 << 32 else 0


def istftn_geometry(n, length, hop, pad=0):
    """tfft_istftn_geometry: F = 1 + (length + 2 pad - n) // hop, the frames per signal. Host only."""
    frames = ctypes.c_uint64()
    _check(load_istftn_library().tfft_istftn_geometry(_u32(n), int(length), int(hop), int(pad), ctypes.byref(frames)))
    return int(frames.value)


def istftn_describe(n, length, hop, pad=0, rows=1, raw_sum=False):
    """tfft_istftn_describe: "istft256r<R>:n x F + ola", R = n / 256 and F the frames per signal. Host only, no GPU needed."""
    buf = ctypes.create_string_buffer(128)
    _check(load_istftn_library().tfft_istftn_describe(_u32(n), int(length), int(hop), int(pad), int(rows), ISTFTN_RAW_SUM if raw_sum else 0,
                                                      buf, len(buf)))
    return buf.value.decode()


def _is_cuda_half(t):
    import torch

    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16


class TfftShortIstftPlan:
    """Owning wrapper of tfft_istftn_plan: half spectra (bins 0 .. n / 2 of rfft / n, what TfftShortStftPlan writes) of `rows` * frames
    frames of n samples (512, 1024 or 2048) that start at f * hop - pad -> `rows` real fp16 signals of `length` samples
    (include/tfft_istftn.h): a one-pass C2R of every frame into the workspace, then y = sum w v / sum w w over the frames that cover a
    sample, +0 where that sum of squares is 0 (raw_sum: y = sum w v). Frame g = r * frames + f of an input plane lies at
    g * in_frame_stride (0 = 2 * pitch), signal r of the output at r * out_sig_stride (0 = length). set_window(w) takes a CUDA
    float16 tensor of n halves before the first exec. Output, inputs and workspace must not overlap."""

    def __init__(self, n, rows, length, hop, pad=0, device=0, in_frame_stride=0, out_sig_stride=0, launch_iters=0, raw_sum=False):
        L = load_istftn_library()
        self._lib = L
        self._h = ctypes.c_void_p()
        self._ws = None
        opts = IstftNOpts(ctypes.sizeof(IstftNOpts), 0, int(in_frame_stride), int(out_sig_stride), int(launch_iters),
                          ISTFTN_RAW_SUM if raw_sum else 0)
        _check(L.tfft_istftn_plan_create(_u32(n), int(rows), int(length), int(hop), int(pad), int(device), ctypes.byref(opts),
                                         ctypes.byref(self._h)))
        self.n, self.rows, self.length, self.hop, self.pad = int(n), int(rows), int(length), int(hop), int(pad)
        self.device = int(device)
        self.raw_sum = bool(raw_sum)
        self.bins, self.pitch = istftn_bins(n), istftn_pitch(n)
        self.frames = istftn_geometry(n, length, hop, pad)
        self.in_frame_stride = int(in_frame_stride) or 2 * self.pitch
        self.out_sig_stride = int(out_sig_stride) or self.length

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            self._lib.tfft_istftn_plan_destroy(h)
            self._ws = None

    __del__ = close

    @property
    def num_launches(self):
        return int(self._lib.tfft_istftn_plan_num_launches(self._h))

    @property
    def kernels(self):
        """tfft_istftn_plan_kernels: the kernels one execution launches, in launch order."""
        return capi._kernel_lines(self._lib.tfft_istftn_plan_kernels, self._h)

    def workspace_bytes(self):
        return int(self._lib.tfft_istftn_plan_workspace_bytes(self._h))

    def set_workspace(self, tensor):
        """Hands a torch CUDA tensor in as the workspace of the time-domain frames (kept alive by the plan); None returns to a
        workspace of the plan's own."""
        if tensor is None:
            _check(self._lib.tfft_istftn_plan_set_workspace(self._h, None, 0))
        else:
            _check(self._lib.tfft_istftn_plan_set_workspace(self._h, tensor.data_ptr(), tensor.numel() * tensor.element_size()))
        self._ws = tensor

    def prepare(self):
        """Allocates the plan's own workspace now (tfft_istftn_plan_prepare): later executions only launch kernels."""
        _check(self._lib.tfft_istftn_plan_prepare(self._h))

    def _stream(self, stream):
        import torch

        return torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream

    def set_window(self, w, stream=None):
        """Hands the window over (tfft_istftn_plan_set_window): n halves, copied on the stream; the tensor is not referenced by the
        plan afterwards."""
        import torch

        if not (_is_cuda_half(w) and w.is_contiguous() and w.device.index == self.device):
            raise TfftError(5, "the window must be a contiguous CUDA float16 tensor on the plan's device")
        if w.numel() != self.n:
            raise TfftError(5, f"the window must hold {self.n} halves")
        with torch.cuda.device(self.device):
            _check(self._lib.tfft_istftn_plan_set_window(self._h, w.data_ptr(), self._stream(stream)))

    def exec_ptr(self, in_re, in_im, out, stream=0):
        _check(self._lib.tfft_istftn_exec(self._h, in_re, in_im, out, stream))

    def exec(self, in_re, in_im, out, stream=None):
        """in_re / in_im: flat CUDA float16 planes, frame g at g * in_frame_stride, n / 2 + 1 bins each (in_im may be a view of in_re's
        buffer, `pitch` halves on: the [RE | IM] blocks TfftShortStftPlan writes); out: flat, signal r at r * out_sig_stride."""
        import torch

        for t in (in_re, in_im, out):
            if not (_is_cuda_half(t) and t.is_contiguous()):
                raise TfftError(5, "buffers must be contiguous CUDA float16 tensors")
            if t.device.index != self.device:
                raise TfftError(5, "tensor on another device than the plan")
        need = (self.rows * self.frames - 1) * self.in_frame_stride + self.bins
        if in_re.numel() < need or in_im.numel() < need:
            raise TfftError(5, f"an input plane is shorter than (rows * frames - 1) * in_frame_stride + {self.bins}")
        if out.numel() < (self.rows - 1) * self.out_sig_stride + self.length:
            raise TfftError(5, "the output buffer is shorter than (rows - 1) * out_sig_stride + length")
        with torch.cuda.device(self.device):
            self.exec_ptr(in_re.data_ptr(), in_im.data_ptr(), out.data_ptr(), self._stream(stream))


# short_istft keeps the plans of the last ISTFTN_CACHE_SIZE (n, rows, length, hop, pad, raw_sum, device) shapes, least recently used
# first out, each with the identity of the window it holds, as istft does. A plan holds device memory outside torch's allocator
# (tables, window, workspace): a caller with many shapes should hold TfftShortIstftPlan objects itself; istftn_cache_clear()
# releases them.
ISTFTN_CACHE_SIZE = 8
_plans = {}


def _plan_for(n, rows, length, hop, pad, raw_sum, device):
    key = (int(n), int(rows), int(length), int(hop), int(pad), bool(raw_sum), int(device))
    entry = _plans.pop(key, None)
    if entry is None:
        entry = [TfftShortIstftPlan(n, rows, length, hop, pad, device, raw_sum=raw_sum), None]
    _plans[key] = entry
    while len(_plans) > ISTFTN_CACHE_SIZE:
        _plans.pop(next(iter(_plans)))[0].close()
    return entry


def istftn_cache_clear():
    """Destroys the plans short_istft cached."""
    while _plans:
        _plans.popitem()[1][0].close()


def short_istft(re, im, window, hop, length, n_fft, center=False, raw_sum=False):
    """Inverse short-time Fourier transform at frame length n_fft = 512, 1024 or 2048: re, im the CUDA float16 [R, F, n_fft / 2 + 1]
    views short_stft() returns (bins 0 .. n_fft / 2 of rfft(window * frame) / n_fft, frame-major), taken as they are; any other
    [R, F, n_fft / 2 + 1] pair is copied into that layout first. window a CUDA float16 tensor [win_length <= n_fft] (a shorter one
    is zero-padded to n_fft with the window centred, as in short_stft), hop a multiple of 8, length the samples per signal (F must
    be the frame count of that length). center as in short_stft: True means pad = n_fft / 2. Returns a new [R, length] tensor:
    sum w v / sum w w over the frames that cover a sample, +0 where no frame or only zeros of the window cover it; raw_sum=True
    leaves the division out. The window is handed to the cached plan again only when (data_ptr, _version) of it changed since the
    last call."""
    import torch

    n = int(n_fft)
    if n not in ISTFTN_LENGTHS:
        raise TfftError(5, "short_istft takes n_fft = 512, 1024 or 2048 (4096: istft)")
    bins, pitch = istftn_bins(n), istftn_pitch(n)
    if not (_is_cuda_half(re) and _is_cuda_half(im) and _is_cuda_half(window) and re.dim() == 3 and re.shape == im.shape
            and re.shape[2] == bins and window.dim() == 1 and window.device == re.device == im.device):
        raise TfftError(5, f"short_istft takes CUDA float16 tensors re, im (R, F, {bins}) and window (win_length) on one device")
    if window.numel() == 0 or window.numel() > n:
        raise TfftError(5, f"the window must hold 1 .. {n} values")
    rows, frames = int(re.shape[0]), int(re.shape[1])
    entry = _plan_for(n, rows, length, hop, n // 2 if center else 0, raw_sum, re.device.index)
    plan = entry[0]
    if plan.frames != frames:
        raise TfftError(5, f"{frames} frames per signal, but length {int(length)} with this hop and padding has {plan.frames}")
    # (a non-contiguous window is copied per call, and a copy's address and version say nothing about its content)
    ident = (window.data_ptr(), window._version, window.numel()) if window.is_contiguous() else None
    if ident is None or entry[1] != ident:
        w = window.contiguous()
        if w.numel() < n:
            left = (n - w.numel()) // 2
            w = torch.nn.functional.pad(w, (left, n - w.numel() - left))
        plan.set_window(w)
        entry[1] = ident
    stride = 2 * pitch
    want = (frames * stride, stride, 1)
    if not (re.stride() == want and im.stride() == want and re.data_ptr() % 16 == 0 and im.data_ptr() % 16 == 0):
        buf = torch.empty((rows, frames, 2, pitch), dtype=torch.float16, device=re.device)
        buf[:, :, 0, :bins] = re
        buf[:, :, 1, :bins] = im
        re, im = buf[:, :, 0, :bins], buf[:, :, 1, :bins]
    out = torch.empty((rows, plan.length), dtype=torch.float16, device=re.device)
    with torch.cuda.device(plan.device):
        plan.exec_ptr(re.data_ptr(), im.data_ptr(), out.data_ptr(), plan._stream(None))
    return out
