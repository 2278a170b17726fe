"""ctypes binding of include/tfft_conv.h (libtfft_conv.so, the FFT convolution add-on). No fallback of any kind. Loading, the
handle's life cycle and the workspace calls are _binding.py's; the plan cache is this module's own (see below)."""
import ctypes
import os

from . import _binding
from . import capi
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_conv.so"
_PREFIX = "tfft_conv_"

# every symbol include/tfft_conv.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_conv_plan_create", "tfft_conv_plan_destroy", "tfft_conv_plan_set_filter", "tfft_conv_plan_workspace_bytes",
    "tfft_conv_plan_set_workspace", "tfft_conv_plan_prepare", "tfft_conv_exec", "tfft_conv_plan_num_launches",
    "tfft_conv_plan_kernels", "tfft_conv_describe", "tfft_conv_filter_slot", "tfft_conv_last_error",
]
CONV_COMPOSED = 1                                             # tfft_conv_plan_create flags


def conv_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


def _prototypes():
    vp, u64, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
    return {
        "tfft_conv_plan_create": (ci, [u64, u64, u64, ci, u64, u64, ci, ctypes.POINTER(vp)]),
        "tfft_conv_plan_destroy": (None, [vp]),
        "tfft_conv_plan_set_filter": (ci, [vp, vp, vp, vp]),
        "tfft_conv_plan_workspace_bytes": (sz, [vp]),
        "tfft_conv_plan_set_workspace": (ci, [vp, vp, sz]),
        "tfft_conv_plan_prepare": (ci, [vp]),
        "tfft_conv_exec": (ci, [vp, vp, vp, vp, vp, vp]),
        "tfft_conv_plan_num_launches": (ci, [vp]),
        "tfft_conv_plan_kernels": (ci, [vp, ctypes.c_char_p, sz]),
        "tfft_conv_describe": (ci, [u64, u64, u64, ci, ctypes.c_char_p, sz]),
        "tfft_conv_filter_slot": (u64, [u64, ci, u64]),
        "tfft_conv_last_error": (ctypes.c_char_p, []),
    }


_lib = None


def load_conv_library():
    """Loads libtfft.so, then libtfft_conv.so; raises (never falls back) when either has not been built."""
    global _lib
    if _lib is None:
        _lib = _binding._load(capi.load_library, conv_lib_path(), "convolution", _prototypes())
    return _lib


def conv_describe(n, batch=1, filters=1, composed=False):
    """tfft_conv_describe: "conv4096:4096" or "<forward chain> | cmul | <inverse chain>". Host only, no GPU needed."""
    L = load_conv_library()
    buf = ctypes.create_string_buffer(512)
    _binding._check(L, _PREFIX, L.tfft_conv_describe(int(n), int(batch), int(filters), CONV_COMPOSED if composed else 0, buf, len(buf)))
    return buf.value.decode()


def conv_filter_slot(n, k, composed=False):
    """tfft_conv_filter_slot: where bin k sits inside a plane of the filter image of a plan (n, composed). Host only."""
    slot = int(load_conv_library().tfft_conv_filter_slot(int(n), CONV_COMPOSED if composed else 0, int(k)))
    if slot == 2 ** 64 - 1:
        raise TfftError(5, f"no convolution plan has bin {k} of length {n}")
    return slot


class TfftConvPlan(_binding._Handle, _binding._Workspace):
    """Owning wrapper of tfft_conv_plan: y_b = ifft(fft(x_b) * H_(b mod filters)) for `batch` complex fp16 signals of length n
    (numpy conventions; include/tfft_conv.h). Planar data as TfftPlan takes it; set_filter(h_re, h_im) takes two CUDA float16 tensors
    of filters * n halves, natural bin order, before the first exec. n = 4096 runs as one fused kernel unless composed=True."""
    _prefix = _PREFIX

    def __init__(self, n, batch=1, filters=1, device=0, in_batch_stride=0, out_batch_stride=0, composed=False):
        L = load_conv_library()
        self._open(L, L.tfft_conv_plan_create, int(n), int(batch), int(filters), int(device), int(in_batch_stride), int(out_batch_stride),
                   CONV_COMPOSED if composed else 0)
        self.n, self.batch, self.filters, self.device, self.composed = int(n), int(batch), int(filters), int(device), bool(composed)
        self.in_batch_stride = int(in_batch_stride) or 2 * self.n
        self.out_batch_stride = int(out_batch_stride) or 2 * self.n

    def set_filter(self, h_re, h_im, stream=None):
        """Hands the filter spectra over (tfft_conv_plan_set_filter); the tensors are not referenced afterwards."""
        import torch

        for t in (h_re, h_im):
            if not (_binding._is_cuda_half(t) and t.is_contiguous() and t.device.index == self.device):
                raise TfftError(5, "filter planes must be contiguous CUDA float16 tensors on the plan's device")
            if t.numel() < self.filters * self.n:
                raise TfftError(5, "a filter plane is shorter than filters * n")
        with torch.cuda.device(self.device):
            self._check(self._lib.tfft_conv_plan_set_filter(self._h, h_re.data_ptr(), h_im.data_ptr(), self._stream(stream)))

    def exec_ptr(self, in_re, in_im, out_re, out_im, stream=0):
        self._check(self._lib.tfft_conv_exec(self._h, in_re, in_im, out_re, out_im, stream))

    def exec(self, in_re, in_im, out_re, out_im, stream=None):
        import torch

        for t in (in_re, in_im, out_re, out_im):
            self._check_kind(t, "planes")
        need_in = (self.batch - 1) * self.in_batch_stride + self.n
        need_out = (self.batch - 1) * self.out_batch_stride + self.n
        if in_re.numel() < need_in or in_im.numel() < need_in or out_re.numel() < need_out or out_im.numel() < need_out:
            raise TfftError(5, "a plane is shorter than (batch-1)*stride + n")
        with torch.cuda.device(self.device):
            self.exec_ptr(in_re.data_ptr(), in_im.data_ptr(), out_re.data_ptr(), out_im.data_ptr(), self._stream(stream))


# fftconv keeps the plans of the last CONV_CACHE_SIZE (n, batch, filters, device) shapes, least recently used first out. A plan holds
# device memory outside torch's allocator (tables, the filter image, a workspace on the composed path): a caller with many shapes
# should hold TfftConvPlan objects itself; conv_cache_clear() releases the cached ones. An entry is the bare plan, not the
# [plan, identity] of the other families (_binding._cached): fftconv sets the filter on every call, so there is no identity to keep.
CONV_CACHE_SIZE = 8
_plans = {}


def _plan_for(n, batch, filters, device):
    key = (int(n), int(batch), int(filters), int(device))
    plan = _plans.pop(key, None)
    if plan is None:
        plan = TfftConvPlan(n, batch, filters, device)
    _plans[key] = plan
    while len(_plans) > CONV_CACHE_SIZE:
        _plans.pop(next(iter(_plans))).close()
    return plan


def conv_cache_clear():
    """Destroys the plans fftconv cached."""
    while _plans:
        _plans.popitem()[1].close()


def fftconv(x_re, x_im, h_re, h_im):
    """ifft(fft(x) * H) row by row: x_re / x_im CUDA float16 (batch, n), h_re / h_im (filters, n) filter spectra in natural bin order
    (numpy.fft.fft of the kernels), row b taking filter b % filters. Returns (y_re, y_im), each (batch, n). A real filter convolves
    the two planes independently."""
    import torch

    if not all(_binding._is_cuda_half(t) and t.dim() == 2 for t in (x_re, x_im, h_re, h_im)) or x_re.shape != x_im.shape or h_re.shape != h_im.shape \
            or h_re.shape[1] != x_re.shape[1]:
        raise TfftError(5, "fftconv takes CUDA float16 tensors x (batch, n) and h (filters, n), RE and IM of equal shape")
    batch, n = x_re.shape
    plan = _plan_for(n, batch, h_re.shape[0], x_re.device.index)
    plan.set_filter(h_re.contiguous().view(-1), h_im.contiguous().view(-1))
    x = torch.stack((x_re, x_im), dim=1).contiguous().view(-1)            # the [RE | IM] block per signal
    y = torch.empty_like(x)
    plan.exec(x, x[n:], y, y[n:])
    y = y.view(batch, 2, n)
    return y[:, 0], y[:, 1]
