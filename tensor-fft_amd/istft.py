"""ctypes binding of include/tfft_istft.h (libtfft_istft.so, the inverse short-time Fourier transform add-on). No fallback of any kind."""
import ctypes
import os

from . import capi, conv
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_istft.so"

# every symbol include/tfft_istft.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_istft_geometry", "tfft_istft_plan_create", "tfft_istft_plan_destroy", "tfft_istft_plan_set_window",
    "tfft_istft_plan_workspace_bytes", "tfft_istft_plan_set_workspace", "tfft_istft_plan_prepare", "tfft_istft_exec",
    "tfft_istft_plan_num_launches", "tfft_istft_plan_kernels", "tfft_istft_describe", "tfft_istft_last_error",
]
ISTFT_N = 4096                                                # TFFT_ISTFT_N: the frame length of every plan
ISTFT_BINS = 2049                                             # TFFT_ISTFT_BINS: bins 0 .. n / 2
ISTFT_PITCH = 2056                                            # TFFT_ISTFT_PITCH: rplan_spectrum_pitch(4096)
ISTFT_RAW_SUM = 1                                             # TFFT_ISTFT_RAW_SUM: no division by the window envelope


class IstftOpts(ctypes.Structure):
    """tfft_istft_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_frame_stride", ctypes.c_uint64),
                ("out_sig_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int)]


def istft_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


_lib = None


def load_istft_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_istft.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    conv.load_conv_library()     # first: the add-on binds to the two libraries (and the HIP runtime) this process already holds
    path = istft_lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the ISTFT add-on has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` from the repository root.")
    L = ctypes.CDLL(path)
    vp, u64, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
    L.tfft_istft_geometry.restype = ci
    L.tfft_istft_geometry.argtypes = [u64, u64, u64, ctypes.POINTER(u64)]
    L.tfft_istft_plan_create.restype = ci
    L.tfft_istft_plan_create.argtypes = [u64, u64, u64, u64, ci, ctypes.POINTER(IstftOpts), ctypes.POINTER(vp)]
    L.tfft_istft_plan_destroy.restype = None
    L.tfft_istft_plan_destroy.argtypes = [vp]
    L.tfft_istft_plan_set_window.restype = ci
    L.tfft_istft_plan_set_window.argtypes = [vp, vp, vp]
    L.tfft_istft_plan_workspace_bytes.restype = sz
    L.tfft_istft_plan_workspace_bytes.argtypes = [vp]
    L.tfft_istft_plan_set_workspace.restype = ci
    L.tfft_istft_plan_set_workspace.argtypes = [vp, vp, sz]
    L.tfft_istft_plan_prepare.restype = ci
    L.tfft_istft_plan_prepare.argtypes = [vp]
    L.tfft_istft_exec.restype = ci
    L.tfft_istft_exec.argtypes = [vp, vp, vp, vp, vp]
    L.tfft_istft_plan_num_launches.restype = ci
    L.tfft_istft_plan_num_launches.argtypes = [vp]
    L.tfft_istft_plan_kernels.restype = ci
    L.tfft_istft_plan_kernels.argtypes = [vp, ctypes.c_char_p, sz]
    L.tfft_istft_describe.restype = ci
    L.tfft_istft_describe.argtypes = [u64, u64, u64, u64, ci, ctypes.c_char_p, sz]
    L.tfft_istft_last_error.restype = ctypes.c_char_p
    L.tfft_istft_last_error.argtypes = []
    _lib = L
    return L


def _check(rc):
    if rc != capi.TFFT_OK:
        raise TfftError(rc, load_istft_library().tfft_istft_last_error().decode())


def istft_geometry(length, hop, pad=0):
    """tfft_istft_geometry: F = 1 + (length + 2 pad - 4096) // hop, the frames per signal. Host only."""
    frames = ctypes.c_uint64()
    _check(load_istft_library().tfft_istft_geometry(int(length), int(hop), int(pad), ctypes.byref(frames)))
    return int(frames.value)


def istft_describe(length, hop, pad=0, rows=1, raw_sum=False):
    """tfft_istft_describe: "istft4096:4096 x F + ola", F the frames per signal. Host only, no GPU needed."""
    buf = ctypes.create_string_buffer(128)
    _check(load_istft_library().tfft_istft_describe(int(length), int(hop), int(pad), int(rows), ISTFT_RAW_SUM if raw_sum else 0, buf, len(buf)))
    return buf.value.decode()


def _is_cuda_half(t):
    import torch

    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16


class TfftIstftPlan:
    """Owning wrapper of tfft_istft_plan: half spectra (bins 0 .. 2048 of rfft / 4096, what TfftStftPlan writes) of `rows` * frames
    frames of 4096 samples that start at f * hop - pad -> `rows` real fp16 signals of `length` samples (include/tfft_istft.h): a
    one-pass C2R of every frame into the workspace, then y = sum w v / sum w w over the frames that cover a sample, +0 where that
    sum of squares is 0 (raw_sum: y = sum w v). Frame g = r * frames + f of an input plane lies at g * in_frame_stride (0 = 2 *
    pitch), signal r of the output at r * out_sig_stride (0 = length). set_window(w) takes a CUDA float16 tensor of 4096 halves
    before the first exec. Output, inputs and workspace must not overlap."""

    def __init__(self, rows, length, hop, pad=0, device=0, in_frame_stride=0, out_sig_stride=0, launch_iters=0, raw_sum=False):
        L = load_istft_library()
        self._lib = L
        self._h = ctypes.c_void_p()
        self._ws = None
        opts = IstftOpts(ctypes.sizeof(IstftOpts), 0, int(in_frame_stride), int(out_sig_stride), int(launch_iters), ISTFT_RAW_SUM if raw_sum else 0)
        _check(L.tfft_istft_plan_create(int(rows), int(length), int(hop), int(pad), int(device), ctypes.byref(opts), ctypes.byref(self._h)))
        self.rows, self.length, self.hop, self.pad = int(rows), int(length), int(hop), int(pad)
        self.device = int(device)
        self.raw_sum = bool(raw_sum)
        self.n, self.bins, self.pitch = ISTFT_N, ISTFT_BINS, ISTFT_PITCH
        self.frames = istft_geometry(length, hop, pad)
        self.in_frame_stride = int(in_frame_stride) or 2 * self.pitch
        self.out_sig_stride = int(out_sig_stride) or self.length

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            self._lib.tfft_istft_plan_destroy(h)
            self._ws = None

    __del__ = close

    @property
    def num_launches(self):
        return int(self._lib.tfft_istft_plan_num_launches(self._h))

    @property
    def kernels(self):
        """tfft_istft_plan_kernels: the kernels one execution launches, in launch order."""
        return capi._kernel_lines(self._lib.tfft_istft_plan_kernels, self._h)

    def workspace_bytes(self):
        return int(self._lib.tfft_istft_plan_workspace_bytes(self._h))

    def set_workspace(self, tensor):
        """Hands a torch CUDA tensor in as the workspace of the time-domain frames (kept alive by the plan); None returns to a
        workspace of the plan's own."""
        if tensor is None:
            _check(self._lib.tfft_istft_plan_set_workspace(self._h, None, 0))
        else:
            _check(self._lib.tfft_istft_plan_set_workspace(self._h, tensor.data_ptr(), tensor.numel() * tensor.element_size()))
        self._ws = tensor

    def prepare(self):
        """Allocates the plan's own workspace now (tfft_istft_plan_prepare): later executions only launch kernels."""
        _check(self._lib.tfft_istft_plan_prepare(self._h))

    def _stream(self, stream):
        import torch

        return torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream

    def set_window(self, w, stream=None):
        """Hands the window over (tfft_istft_plan_set_window): 4096 halves, copied on the stream; the tensor is not referenced by the
        plan afterwards."""
        import torch

        if not (_is_cuda_half(w) and w.is_contiguous() and w.device.index == self.device):
            raise TfftError(5, "the window must be a contiguous CUDA float16 tensor on the plan's device")
        if w.numel() != self.n:
            raise TfftError(5, "the window must hold 4096 halves")
        with torch.cuda.device(self.device):
            _check(self._lib.tfft_istft_plan_set_window(self._h, w.data_ptr(), self._stream(stream)))

    def exec_ptr(self, in_re, in_im, out, stream=0):
        _check(self._lib.tfft_istft_exec(self._h, in_re, in_im, out, stream))

    def exec(self, in_re, in_im, out, stream=None):
        """in_re / in_im: flat CUDA float16 planes, frame g at g * in_frame_stride, 2049 bins each (in_im may be a view of in_re's
        buffer, 2056 halves on: the [RE | IM] blocks TfftStftPlan writes); out: flat, signal r at r * out_sig_stride."""
        import torch

        for t in (in_re, in_im, out):
            if not (_is_cuda_half(t) and t.is_contiguous()):
                raise TfftError(5, "buffers must be contiguous CUDA float16 tensors")
            if t.device.index != self.device:
                raise TfftError(5, "tensor on another device than the plan")
        need = (self.rows * self.frames - 1) * self.in_frame_stride + self.bins
        if in_re.numel() < need or in_im.numel() < need:
            raise TfftError(5, "an input plane is shorter than (rows * frames - 1) * in_frame_stride + 2049")
        if out.numel() < (self.rows - 1) * self.out_sig_stride + self.length:
            raise TfftError(5, "the output buffer is shorter than (rows - 1) * out_sig_stride + length")
        with torch.cuda.device(self.device):
            self.exec_ptr(in_re.data_ptr(), in_im.data_ptr(), out.data_ptr(), self._stream(stream))


# istft keeps the plans of the last ISTFT_CACHE_SIZE (rows, length, hop, pad, raw_sum, device) shapes, least recently used first out,
# each with the identity of the window it holds, as stft does. A plan holds device memory outside torch's allocator (tables, window,
# workspace): a caller with many shapes should hold TfftIstftPlan objects itself; istft_cache_clear() releases them.
ISTFT_CACHE_SIZE = 8
_plans = {}


def _plan_for(rows, length, hop, pad, raw_sum, device):
    key = (int(rows), int(length), int(hop), int(pad), bool(raw_sum), int(device))
    entry = _plans.pop(key, None)
    if entry is None:
        entry = [TfftIstftPlan(rows, length, hop, pad, device, raw_sum=raw_sum), None]
    _plans[key] = entry
    while len(_plans) > ISTFT_CACHE_SIZE:
        _plans.pop(next(iter(_plans)))[0].close()
    return entry


def istft_cache_clear():
    """Destroys the plans istft cached."""
    while _plans:
        _plans.popitem()[1][0].close()


def istft(re, im, window, hop, length, center=False, raw_sum=False, n_fft=ISTFT_N):
    """Inverse short-time Fourier transform at frame length 4096 (n_fft = 512, 1024 or 2048: istftn.short_istft, which takes the
    same arguments at that frame length): re, im the CUDA float16 [R, F, 2049] views stft() returns (bins
    0 .. 2048 of rfft(window * frame) / 4096, frame-major), taken as they are; any other [R, F, 2049] pair is copied into that
    layout first. window a CUDA float16 tensor [win_length <= 4096] (a shorter one is zero-padded to 4096 with the window centred, as
    in stft), hop a multiple of 8, length the samples per signal (F must be the frame count of that length). center as in stft.
    Returns a new [R, length] tensor: sum w v / sum w w over the frames that cover a sample, +0 where no frame or only zeros of the
    window cover it; raw_sum=True leaves the division out. The window is handed to the cached plan again only when (data_ptr,
    _version) of it changed since the last call."""
    import torch

    if n_fft != ISTFT_N:
        from . import istftn

        if n_fft not in istftn.ISTFTN_LENGTHS:
            raise TfftError(5, "istft takes n_fft = 512, 1024, 2048 or 4096")
        return istftn.short_istft(re, im, window, hop, length, n_fft, center, raw_sum)
    if not (_is_cuda_half(re) and _is_cuda_half(im) and _is_cuda_half(window) and re.dim() == 3 and re.shape == im.shape
            and re.shape[2] == ISTFT_BINS and window.dim() == 1 and window.device == re.device == im.device):
        raise TfftError(5, "istft takes CUDA float16 tensors re, im (R, F, 2049) and window (win_length) on one device")
    if window.numel() == 0 or window.numel() > ISTFT_N:
        raise TfftError(5, "the window must hold 1 .. 4096 values")
    rows, frames = int(re.shape[0]), int(re.shape[1])
    entry = _plan_for(rows, length, hop, ISTFT_N // 2 if center else 0, raw_sum, re.device.index)
    plan = entry[0]
    if plan.frames != frames:
        raise TfftError(5, f"{frames} frames per signal, but length {int(length)} with this hop and padding has {plan.frames}")
    ident = (window.data_ptr(), window._version, window.numel()) if window.is_contiguous() else None
    if ident is None or entry[1] != ident:
        w = window.contiguous()
        if w.numel() < ISTFT_N:
            left = (ISTFT_N - w.numel()) // 2
            w = torch.nn.functional.pad(w, (left, ISTFT_N - w.numel() - left))
        plan.set_window(w)
        entry[1] = ident
    stride = 2 * ISTFT_PITCH
    want = (frames * stride, stride, 1)
    if not (re.stride() == want and im.stride() == want and re.data_ptr() % 16 == 0 and im.data_ptr() % 16 == 0):
        buf = torch.empty((rows, frames, 2, ISTFT_PITCH), dtype=torch.float16, device=re.device)
        buf[:, :, 0, :ISTFT_BINS] = re
        buf[:, :, 1, :ISTFT_BINS] = im
        re, im = buf[:, :, 0, :ISTFT_BINS], buf[:, :, 1, :ISTFT_BINS]
    out = torch.empty((rows, plan.length), dtype=torch.float16, device=re.device)
    with torch.cuda.device(plan.device):
        plan.exec_ptr(re.data_ptr(), im.data_ptr(), out.data_ptr(), plan._stream(None))
    return out
