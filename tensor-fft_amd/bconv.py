"""ctypes binding of include/tfft_bconv.h (libtfft_bconv.so, the gradients of the overlap-save causal convolution), and the
torch.autograd hook over it. No fallback of any kind: torch supplies memory, streams and the autograd graph, nothing else."""
import ctypes
import os

from . import capi, conv, sconv
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_bconv.so"

# every symbol include/tfft_bconv.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_bconv_geometry", "tfft_bconv_plan_create", "tfft_bconv_plan_destroy", "tfft_bconv_plan_set_taps", "tfft_bconv_plan_spectrum",
    "tfft_bconv_plan_workspace_bytes", "tfft_bconv_plan_set_workspace", "tfft_bconv_plan_prepare", "tfft_bconv_exec_input_grad",
    "tfft_bconv_exec_tap_grad", "tfft_bconv_plan_num_launches", "tfft_bconv_plan_kernels", "tfft_bconv_describe", "tfft_bconv_last_error",
]
BCONV_MAX_TAPS = 2049                                         # TFFT_BCONV_MAX_TAPS
BCONV_N = 4096                                                # the transform length of every plan


class BconvOpts(ctypes.Structure):
    """tfft_bconv_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("x_seq_stride", ctypes.c_uint64),
                ("g_seq_stride", ctypes.c_uint64), ("dx_seq_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32),
                ("partials", ctypes.c_uint32), ("flags", ctypes.c_int)]


def bconv_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


_lib = None


def load_bconv_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_bconv.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    conv.load_conv_library()     # first: the add-on binds to the two libraries (and the HIP runtime) this process already holds
    path = bconv_lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the convolution gradient add-on has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` from the repository root.")
    L = ctypes.CDLL(path)
    vp, u64, u32, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t
    pu64 = ctypes.POINTER(u64)
    L.tfft_bconv_geometry.restype = ci
    L.tfft_bconv_geometry.argtypes = [u64, u64, u64, u64, u32, pu64, pu64, pu64, pu64]
    L.tfft_bconv_plan_create.restype = ci
    L.tfft_bconv_plan_create.argtypes = [u64, u64, u64, u64, ci, ctypes.POINTER(BconvOpts), ctypes.POINTER(vp)]
    L.tfft_bconv_plan_destroy.restype = None
    L.tfft_bconv_plan_destroy.argtypes = [vp]
    L.tfft_bconv_plan_set_taps.restype = ci
    L.tfft_bconv_plan_set_taps.argtypes = [vp, vp, vp]
    L.tfft_bconv_plan_spectrum.restype = ci
    L.tfft_bconv_plan_spectrum.argtypes = [vp, vp, vp]
    L.tfft_bconv_plan_workspace_bytes.restype = sz
    L.tfft_bconv_plan_workspace_bytes.argtypes = [vp]
    L.tfft_bconv_plan_set_workspace.restype = ci
    L.tfft_bconv_plan_set_workspace.argtypes = [vp, vp, sz]
    L.tfft_bconv_plan_prepare.restype = ci
    L.tfft_bconv_plan_prepare.argtypes = [vp]
    L.tfft_bconv_exec_input_grad.restype = ci
    L.tfft_bconv_exec_input_grad.argtypes = [vp, vp, vp, vp]
    L.tfft_bconv_exec_tap_grad.restype = ci
    L.tfft_bconv_exec_tap_grad.argtypes = [vp, vp, vp, vp, vp]
    L.tfft_bconv_plan_num_launches.restype = ci
    L.tfft_bconv_plan_num_launches.argtypes = [vp]
    L.tfft_bconv_plan_kernels.restype = ci
    L.tfft_bconv_plan_kernels.argtypes = [vp, ctypes.c_char_p, sz]
    L.tfft_bconv_describe.restype = ci
    L.tfft_bconv_describe.argtypes = [u64, u64, u64, u64, u32, ci, ctypes.c_char_p, sz]
    L.tfft_bconv_last_error.restype = ctypes.c_char_p
    L.tfft_bconv_last_error.argtypes = []
    _lib = L
    return L


def _check(rc):
    if rc != capi.TFFT_OK:
        raise TfftError(rc, load_bconv_library().tfft_bconv_last_error().decode())


def bconv_geometry(length, taps, rows=1, channels=1, partials=0):
    """tfft_bconv_geometry: (halo, hop, segments, P): the geometry of sconv_geometry and the partial sums per channel of the tap
    gradient under the cap `partials` (0 = none). Host only."""
    out = [ctypes.c_uint64() for _ in range(4)]
    _check(load_bconv_library().tfft_bconv_geometry(int(length), int(taps), int(rows), int(channels), int(partials), *[ctypes.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def bconv_describe(length, taps, rows=1, channels=1, partials=0):
    """tfft_bconv_describe: "bconv4096:4096 x S | partials P". Host only, no GPU needed."""
    buf = ctypes.create_string_buffer(128)
    _check(load_bconv_library().tfft_bconv_describe(int(length), int(taps), int(rows), int(channels), int(partials), 0, buf, len(buf)))
    return buf.value.decode()


def _is_cuda(t, dtype):
    import torch

    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype


class TfftLongConvGradPlan:
    """Owning wrapper of tfft_bconv_plan: the two gradients of TfftLongConvPlan for rows x channels real fp16 sequences of `length`
    samples and `taps` <= 2049 taps per channel (include/tfft_bconv.h). input_grad(g, dx) needs set_taps(h) first; tap_grad(x, g, dh)
    writes [channels][taps] float32 and needs no taps. `partials` caps the partial sums per channel (0 = the library's default); the
    tap gradient depends on it through the order of fp32 additions only."""

    def __init__(self, rows, channels, length, taps, device=0, x_seq_stride=0, g_seq_stride=0, dx_seq_stride=0, launch_iters=0, partials=0):
        L = load_bconv_library()
        self._lib = L
        self._h = ctypes.c_void_p()
        opts = BconvOpts(ctypes.sizeof(BconvOpts), 0, int(x_seq_stride), int(g_seq_stride), int(dx_seq_stride), int(launch_iters), int(partials), 0)
        _check(L.tfft_bconv_plan_create(int(rows), int(channels), int(length), int(taps), int(device), ctypes.byref(opts), ctypes.byref(self._h)))
        self.rows, self.channels, self.length, self.taps = int(rows), int(channels), int(length), int(taps)
        self.device = int(device)
        self.n = BCONV_N
        self.halo, self.hop, self.segments, self.partials = bconv_geometry(length, taps, rows, channels, partials)
        self.x_seq_stride = int(x_seq_stride) or self.length
        self.g_seq_stride = int(g_seq_stride) or self.length
        self.dx_seq_stride = int(dx_seq_stride) or self.length
        self._ws = None

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            self._lib.tfft_bconv_plan_destroy(h)
            self._ws = None

    __del__ = close

    @property
    def num_launches(self):
        return int(self._lib.tfft_bconv_plan_num_launches(self._h))

    @property
    def workspace_bytes(self):
        return int(self._lib.tfft_bconv_plan_workspace_bytes(self._h))

    @property
    def kernels(self):
        """tfft_bconv_plan_kernels: the input gradient's kernel, then the tap gradient's two."""
        return capi._kernel_lines(self._lib.tfft_bconv_plan_kernels, self._h)

    def _stream(self, stream):
        import torch

        return torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream

    def set_taps(self, h, stream=None):
        """Hands the taps over (tfft_bconv_plan_set_taps): [channels][taps] float16; the tensor is not referenced afterwards."""
        import torch

        if not (_is_cuda(h, torch.float16) and h.is_contiguous() and h.device.index == self.device):
            raise TfftError(5, "taps must be a contiguous CUDA float16 tensor on the plan's device")
        if h.numel() < self.channels * self.taps:
            raise TfftError(5, "the taps tensor is shorter than channels * taps")
        with torch.cuda.device(self.device):
            _check(self._lib.tfft_bconv_plan_set_taps(self._h, h.data_ptr(), self._stream(stream)))

    def spectrum(self):
        """tfft_bconv_plan_spectrum: (h_re, h_im), H as two CUDA float16 tensors [channels, 4096] (not conjugated)."""
        import torch

        h_re = torch.empty((self.channels, self.n), dtype=torch.float16, device=f"cuda:{self.device}")
        h_im = torch.empty_like(h_re)
        with torch.cuda.device(self.device):
            _check(self._lib.tfft_bconv_plan_spectrum(self._h, h_re.data_ptr(), h_im.data_ptr()))
        return h_re, h_im

    def set_workspace(self, tensor):
        """Hands a torch CUDA tensor in as the workspace of the tap gradient (kept alive by the plan)."""
        _check(self._lib.tfft_bconv_plan_set_workspace(self._h, tensor.data_ptr(), tensor.numel() * tensor.element_size()))
        self._ws = tensor

    def prepare(self):
        """Allocates the plan's own workspace now (tfft_bconv_plan_prepare): later tap gradients only launch kernels."""
        _check(self._lib.tfft_bconv_plan_prepare(self._h))

    def input_grad_ptr(self, g, dx, stream=0):
        _check(self._lib.tfft_bconv_exec_input_grad(self._h, g, dx, stream))

    def tap_grad_ptr(self, x, g, dh, stream=0):
        _check(self._lib.tfft_bconv_exec_tap_grad(self._h, x, g, dh, stream))

    def _check_seqs(self, t, stride):
        import torch

        if not (_is_cuda(t, torch.float16) and t.is_contiguous()):
            raise TfftError(5, "sequences must be contiguous CUDA float16 tensors")
        if t.device.index != self.device:
            raise TfftError(5, "tensor on another device than the plan")
        if t.numel() < (self.rows * self.channels - 1) * stride + self.length:
            raise TfftError(5, "a tensor is shorter than (rows * channels - 1) * stride + length")

    def input_grad(self, g, dx, stream=None):
        """g, dx: flat CUDA float16 tensors that share no element, sequence (b, c) at (b * channels + c) * seq stride."""
        import torch

        self._check_seqs(g, self.g_seq_stride)
        self._check_seqs(dx, self.dx_seq_stride)
        with torch.cuda.device(self.device):
            self.input_grad_ptr(g.data_ptr(), dx.data_ptr(), self._stream(stream))

    def tap_grad(self, x, g, dh, stream=None):
        """x, g: flat CUDA float16 tensors (they may be the same); dh: a contiguous CUDA float32 tensor of channels * taps elements."""
        import torch

        self._check_seqs(x, self.x_seq_stride)
        self._check_seqs(g, self.g_seq_stride)
        if not (_is_cuda(dh, torch.float32) and dh.is_contiguous() and dh.device.index == self.device and dh.numel() >= self.channels * self.taps):
            raise TfftError(5, "the tap gradient must be a contiguous CUDA float32 tensor of channels * taps elements on the plan's device")
        with torch.cuda.device(self.device):
            self.tap_grad_ptr(x.data_ptr(), g.data_ptr(), dh.data_ptr(), self._stream(stream))


# The convenience functions keep the plans of the last BCONV_CACHE_SIZE (rows, channels, length, taps, device) shapes, least recently
# used first out, as sconv._plan_for does: one cache per gradient (a caller who needs only one gradient creates no plan for the
# other, and the tap gradient's plans hold a workspace), the input gradient's with the identity of the taps each plan holds.
# bconv_cache_clear() releases both.
BCONV_CACHE_SIZE = 8
_dx_plans = {}
_dh_plans = {}


def _plan_for(cache, rows, channels, length, taps, device):
    key = (int(rows), int(channels), int(length), int(taps), int(device))
    entry = cache.pop(key, None)
    if entry is None:
        entry = [TfftLongConvGradPlan(rows, channels, length, taps, device), None]
    cache[key] = entry
    while len(cache) > BCONV_CACHE_SIZE:
        cache.pop(next(iter(cache)))[0].close()
    return entry


def bconv_cache_clear():
    """Destroys the plans long_causal_conv_input_grad and long_causal_conv_tap_grad cached."""
    for cache in (_dx_plans, _dh_plans):
        while cache:
            cache.popitem()[1][0].close()


def long_causal_conv_input_grad(g, h):
    """dx[b, c, t] = sum_j h[c, j] g[b, c, t + j]: g a CUDA float16 tensor [B, C, L], h [C, K] with K <= 2049. Returns dx [B, C, L], a
    new tensor. The taps are handed to the cached plan again only when (data_ptr, _version) of h changed since the last call."""
    import torch

    if not (_is_cuda(g, torch.float16) and _is_cuda(h, torch.float16) and g.dim() == 3 and h.dim() == 2 and h.shape[0] == g.shape[1]
            and h.device == g.device):
        raise TfftError(5, "long_causal_conv_input_grad takes CUDA float16 tensors g (B, C, L) and h (C, K) on one device")
    rows, channels, length = g.shape
    entry = _plan_for(_dx_plans, rows, channels, length, h.shape[1], g.device.index)
    plan = entry[0]
    ident = (h.data_ptr(), h._version) if h.is_contiguous() else None
    h = h.contiguous()
    if ident is None or entry[1] != ident:
        plan.set_taps(h.view(-1))
        entry[1] = ident
    g = g.contiguous()
    dx = torch.empty_like(g)
    plan.input_grad(g.view(-1), dx.view(-1))
    return dx


def long_causal_conv_tap_grad(x, g, taps):
    """dh[c, j] = sum_{b, t} g[b, c, t] x[b, c, t - j], j < taps: x, g CUDA float16 tensors [B, C, L]. Returns dh [C, taps] float32."""
    import torch

    if not (_is_cuda(x, torch.float16) and _is_cuda(g, torch.float16) and x.dim() == 3 and g.shape == x.shape and g.device == x.device):
        raise TfftError(5, "long_causal_conv_tap_grad takes CUDA float16 tensors x and g of one shape (B, C, L) on one device")
    rows, channels, length = x.shape
    plan = _plan_for(_dh_plans, rows, channels, length, taps, x.device.index)[0]
    dh = torch.empty((channels, int(taps)), dtype=torch.float32, device=x.device)
    plan.tap_grad(x.contiguous().view(-1), g.contiguous().view(-1), dh)
    return dh


_function = None


def _autograd_function():
    """the torch.autograd.Function, built on first use so that importing the package does not import torch"""
    global _function
    if _function is not None:
        return _function
    import torch

    class LongCausalConv(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, h):
            ctx.save_for_backward(x, h)
            return sconv.long_causal_conv(x, h)

        @staticmethod
        def backward(ctx, g):
            x, h = ctx.saved_tensors
            dx = dh = None
            if ctx.needs_input_grad[0]:
                dx = long_causal_conv_input_grad(g, h)
            if ctx.needs_input_grad[1]:
                dh = long_causal_conv_tap_grad(x, g, h.shape[1]).to(h.dtype)
            return dx, dh

    _function = LongCausalConv
    return _function


def differentiable_long_causal_conv(x, h):
    """long_causal_conv(x, h) with a grad_fn: the forward pass is TfftLongConvPlan, the backward pass the two gradient plans, each
    run only when its input needs a gradient; the tap gradient comes back cast to h.dtype."""
    return _autograd_function().apply(x, h)
