"""ctypes binding of include/tfft_cconv.h (libtfft_cconv.so, the carried convolution add-on: the overlap-save causal convolution
and its gradients on a chunk of a longer sequence, with the history in front of x and the future behind g read in place), and the
torch.autograd hook over it. No fallback of any kind: torch supplies memory, streams and the autograd graph, nothing else."""
import ctypes
import os

from . import capi, conv
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_cconv.so"

# every symbol include/tfft_cconv.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_cconv_geometry", "tfft_cconv_plan_create", "tfft_cconv_plan_destroy", "tfft_cconv_plan_set_taps", "tfft_cconv_plan_spectrum",
    "tfft_cconv_exec", "tfft_cconv_plan_num_launches", "tfft_cconv_plan_kernels", "tfft_cconv_describe",
    "tfft_cconv_grad_geometry", "tfft_cconv_grad_create", "tfft_cconv_grad_destroy", "tfft_cconv_grad_set_taps", "tfft_cconv_grad_spectrum",
    "tfft_cconv_grad_workspace_bytes", "tfft_cconv_grad_set_workspace", "tfft_cconv_grad_prepare", "tfft_cconv_grad_exec_input_grad",
    "tfft_cconv_grad_exec_tap_grad", "tfft_cconv_grad_num_launches", "tfft_cconv_grad_kernels", "tfft_cconv_grad_describe",
    "tfft_cconv_last_error",
]
CCONV_MAX_TAPS = 2049                                         # TFFT_CCONV_MAX_TAPS
CCONV_N = 4096                                                # the transform length of every plan


class CconvOpts(ctypes.Structure):
    """tfft_cconv_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_seq_stride", ctypes.c_uint64),
                ("out_seq_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int),
                ("history", ctypes.c_uint64), ("hist_seq_stride", ctypes.c_uint64)]


class CconvGradOpts(ctypes.Structure):
    """tfft_cconv_grad_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("x_seq_stride", ctypes.c_uint64),
                ("g_seq_stride", ctypes.c_uint64), ("dx_seq_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32),
                ("partials", ctypes.c_uint32), ("flags", ctypes.c_int), ("history", ctypes.c_uint64), ("hist_seq_stride", ctypes.c_uint64),
                ("future", ctypes.c_uint64), ("fut_seq_stride", ctypes.c_uint64)]


def cconv_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


_lib = None


def load_cconv_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_cconv.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    conv.load_conv_library()     # first: the add-on binds to the two libraries (and the HIP runtime) this process already holds
    path = cconv_lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the carried convolution add-on has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` from the repository root.")
    L = ctypes.CDLL(path)
    vp, u64, u32, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t
    pu64 = ctypes.POINTER(u64)
    L.tfft_cconv_geometry.restype = ci
    L.tfft_cconv_geometry.argtypes = [u64, u64, pu64, pu64, pu64, pu64]
    L.tfft_cconv_plan_create.restype = ci
    L.tfft_cconv_plan_create.argtypes = [u64, u64, u64, u64, ci, ctypes.POINTER(CconvOpts), ctypes.POINTER(vp)]
    L.tfft_cconv_plan_destroy.restype = None
    L.tfft_cconv_plan_destroy.argtypes = [vp]
    L.tfft_cconv_plan_set_taps.restype = ci
    L.tfft_cconv_plan_set_taps.argtypes = [vp, vp, vp]
    L.tfft_cconv_plan_spectrum.restype = ci
    L.tfft_cconv_plan_spectrum.argtypes = [vp, vp, vp]
    L.tfft_cconv_exec.restype = ci
    L.tfft_cconv_exec.argtypes = [vp, vp, vp, vp, vp]
    L.tfft_cconv_plan_num_launches.restype = ci
    L.tfft_cconv_plan_num_launches.argtypes = [vp]
    L.tfft_cconv_plan_kernels.restype = ci
    L.tfft_cconv_plan_kernels.argtypes = [vp, ctypes.c_char_p, sz]
    L.tfft_cconv_describe.restype = ci
    L.tfft_cconv_describe.argtypes = [u64, u64, u64, u64, ci, ctypes.c_char_p, sz]
    L.tfft_cconv_grad_geometry.restype = ci
    L.tfft_cconv_grad_geometry.argtypes = [u64, u64, u64, u64, u32, pu64, pu64, pu64, pu64, pu64]
    L.tfft_cconv_grad_create.restype = ci
    L.tfft_cconv_grad_create.argtypes = [u64, u64, u64, u64, ci, ctypes.POINTER(CconvGradOpts), ctypes.POINTER(vp)]
    L.tfft_cconv_grad_destroy.restype = None
    L.tfft_cconv_grad_destroy.argtypes = [vp]
    L.tfft_cconv_grad_set_taps.restype = ci
    L.tfft_cconv_grad_set_taps.argtypes = [vp, vp, vp]
    L.tfft_cconv_grad_spectrum.restype = ci
    L.tfft_cconv_grad_spectrum.argtypes = [vp, vp, vp]
    L.tfft_cconv_grad_workspace_bytes.restype = sz
    L.tfft_cconv_grad_workspace_bytes.argtypes = [vp]
    L.tfft_cconv_grad_set_workspace.restype = ci
    L.tfft_cconv_grad_set_workspace.argtypes = [vp, vp, sz]
    L.tfft_cconv_grad_prepare.restype = ci
    L.tfft_cconv_grad_prepare.argtypes = [vp]
    L.tfft_cconv_grad_exec_input_grad.restype = ci
    L.tfft_cconv_grad_exec_input_grad.argtypes = [vp, vp, vp, vp, vp]
    L.tfft_cconv_grad_exec_tap_grad.restype = ci
    L.tfft_cconv_grad_exec_tap_grad.argtypes = [vp, vp, vp, vp, vp, vp]
    L.tfft_cconv_grad_num_launches.restype = ci
    L.tfft_cconv_grad_num_launches.argtypes = [vp]
    L.tfft_cconv_grad_kernels.restype = ci
    L.tfft_cconv_grad_kernels.argtypes = [vp, ctypes.c_char_p, sz]
    L.tfft_cconv_grad_describe.restype = ci
    L.tfft_cconv_grad_describe.argtypes = [u64, u64, u64, u64, u32, ci, ctypes.c_char_p, sz]
    L.tfft_cconv_last_error.restype = ctypes.c_char_p
    L.tfft_cconv_last_error.argtypes = []
    _lib = L
    return L


def _check(rc):
    if rc != capi.TFFT_OK:
        raise TfftError(rc, load_cconv_library().tfft_cconv_last_error().decode())


def cconv_geometry(length, taps, rows=1, channels=1, partials=0):
    """tfft_cconv_grad_geometry: (halo, hop, segments, P, carry_min): the geometry of sconv_geometry, the partial sums per channel of
    the tap gradient under the cap `partials` (0 = none), and K - 1 rounded up to a multiple of 8, the smallest context that loses
    nothing. Host only."""
    out = [ctypes.c_uint64() for _ in range(5)]
    _check(load_cconv_library().tfft_cconv_grad_geometry(int(length), int(taps), int(rows), int(channels), int(partials),
                                                         *[ctypes.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def cconv_describe(length, taps, rows=1, channels=1, partials=0):
    """(tfft_cconv_describe, tfft_cconv_grad_describe): ("cconv4096:4096 x S", "cconv4096:4096 x S | partials P"). Host only."""
    L = load_cconv_library()
    fwd, grad = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
    _check(L.tfft_cconv_describe(int(length), int(taps), int(rows), int(channels), 0, fwd, len(fwd)))
    _check(L.tfft_cconv_grad_describe(int(length), int(taps), int(rows), int(channels), int(partials), 0, grad, len(grad)))
    return fwd.value.decode(), grad.value.decode()


def _is_cuda(t, dtype):
    import torch

    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype


class _PlanBase:
    def _stream(self, stream):
        import torch

        return torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream

    def _check_taps(self, h):
        import torch

        if not (_is_cuda(h, torch.float16) and h.is_contiguous() and h.device.index == self.device):
            raise TfftError(5, "taps must be a contiguous CUDA float16 tensor on the plan's device")
        if h.numel() < self.channels * self.taps:
            raise TfftError(5, "the taps tensor is shorter than channels * taps")

    def _check_seqs(self, t, stride, length, what="sequences"):
        import torch

        if not (_is_cuda(t, torch.float16) and t.is_contiguous()):
            raise TfftError(5, f"{what} must be contiguous CUDA float16 tensors")
        if t.device.index != self.device:
            raise TfftError(5, "tensor on another device than the plan")
        if t.numel() < (self.rows * self.channels - 1) * stride + length:
            raise TfftError(5, f"{what}: a tensor is shorter than (rows * channels - 1) * stride + length")

    def _spectrum(self, fn):
        import torch

        h_re = torch.empty((self.channels, self.n), dtype=torch.float16, device=f"cuda:{self.device}")
        h_im = torch.empty_like(h_re)
        with torch.cuda.device(self.device):
            _check(fn(self._h, h_re.data_ptr(), h_im.data_ptr()))
        return h_re, h_im


class TfftChunkedConvPlan(_PlanBase):
    """Owning wrapper of tfft_cconv_plan: TfftLongConvPlan on a chunk of a longer sequence. y[b][c][t] = sum_j h[c][j] xe[b][c][t - j],
    xe the input with `history` (a multiple of 8, at most halo) samples of context in front of it, read from a second pointer
    (include/tfft_cconv.h). exec(x, y, hist) with hist = None reads zeros there. The output must not overlap the input or the history;
    the input and the history may be views of one buffer."""

    def __init__(self, rows, channels, length, taps, device=0, in_seq_stride=0, out_seq_stride=0, launch_iters=0, history=0, hist_seq_stride=0):
        L = load_cconv_library()
        self._lib = L
        self._h = ctypes.c_void_p()
        opts = CconvOpts(ctypes.sizeof(CconvOpts), 0, int(in_seq_stride), int(out_seq_stride), int(launch_iters), 0, int(history), int(hist_seq_stride))
        _check(L.tfft_cconv_plan_create(int(rows), int(channels), int(length), int(taps), int(device), ctypes.byref(opts), ctypes.byref(self._h)))
        self.rows, self.channels, self.length, self.taps = int(rows), int(channels), int(length), int(taps)
        self.device = int(device)
        self.n = CCONV_N
        self.halo, self.hop, self.segments, _, self.carry_min = cconv_geometry(length, taps, rows, channels)
        self.in_seq_stride = int(in_seq_stride) or self.length
        self.out_seq_stride = int(out_seq_stride) or self.length
        self.history = int(history)
        self.hist_seq_stride = int(hist_seq_stride) or self.history

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            self._lib.tfft_cconv_plan_destroy(h)

    __del__ = close

    @property
    def num_launches(self):
        return int(self._lib.tfft_cconv_plan_num_launches(self._h))

    @property
    def kernels(self):
        """tfft_cconv_plan_kernels: the kernels one execution launches, in launch order."""
        return capi._kernel_lines(self._lib.tfft_cconv_plan_kernels, self._h)

    def set_taps(self, h, stream=None):
        """Hands the taps over (tfft_cconv_plan_set_taps): [channels][taps]; the tensor is not referenced afterwards."""
        import torch

        self._check_taps(h)
        with torch.cuda.device(self.device):
            _check(self._lib.tfft_cconv_plan_set_taps(self._h, h.data_ptr(), self._stream(stream)))

    def spectrum(self):
        """tfft_cconv_plan_spectrum: (h_re, h_im), two CUDA float16 tensors [channels, 4096]."""
        return self._spectrum(self._lib.tfft_cconv_plan_spectrum)

    def exec_ptr(self, src, hist, dst, stream=0):
        _check(self._lib.tfft_cconv_exec(self._h, src, hist, dst, stream))

    def exec(self, x, y, hist=None, stream=None):
        """x, y, hist: flat CUDA float16 tensors, sequence (b, c) at (b * channels + c) * its seq stride; hist = None: zeros."""
        import torch

        self._check_seqs(x, self.in_seq_stride, self.length)
        self._check_seqs(y, self.out_seq_stride, self.length)
        if hist is not None:
            self._check_seqs(hist, self.hist_seq_stride, self.history, "histories")
        with torch.cuda.device(self.device):
            self.exec_ptr(x.data_ptr(), None if hist is None else hist.data_ptr(), y.data_ptr(), self._stream(stream))


class TfftChunkedConvGradPlan(_PlanBase):
    """Owning wrapper of tfft_cconv_grad: TfftLongConvGradPlan on a chunk of a longer sequence. input_grad(g, dx, future) reads
    `future` samples of g behind sample L from a second pointer; tap_grad(x, g, dh, history) reads `history` samples of x in front
    of sample 0 from one (include/tfft_cconv.h). None reads zeros."""

    def __init__(self, rows, channels, length, taps, device=0, x_seq_stride=0, g_seq_stride=0, dx_seq_stride=0, launch_iters=0, partials=0,
                 history=0, hist_seq_stride=0, future=0, fut_seq_stride=0):
        L = load_cconv_library()
        self._lib = L
        self._h = ctypes.c_void_p()
        opts = CconvGradOpts(ctypes.sizeof(CconvGradOpts), 0, int(x_seq_stride), int(g_seq_stride), int(dx_seq_stride), int(launch_iters),
                             int(partials), 0, int(history), int(hist_seq_stride), int(future), int(fut_seq_stride))
        _check(L.tfft_cconv_grad_create(int(rows), int(channels), int(length), int(taps), int(device), ctypes.byref(opts), ctypes.byref(self._h)))
        self.rows, self.channels, self.length, self.taps = int(rows), int(channels), int(length), int(taps)
        self.device = int(device)
        self.n = CCONV_N
        self.halo, self.hop, self.segments, self.partials, self.carry_min = cconv_geometry(length, taps, rows, channels, partials)
        self.x_seq_stride = int(x_seq_stride) or self.length
        self.g_seq_stride = int(g_seq_stride) or self.length
        self.dx_seq_stride = int(dx_seq_stride) or self.length
        self.history, self.future = int(history), int(future)
        self.hist_seq_stride = int(hist_seq_stride) or self.history
        self.fut_seq_stride = int(fut_seq_stride) or self.future
        self._ws = None

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            self._lib.tfft_cconv_grad_destroy(h)
            self._ws = None

    __del__ = close

    @property
    def num_launches(self):
        return int(self._lib.tfft_cconv_grad_num_launches(self._h))

    @property
    def workspace_bytes(self):
        return int(self._lib.tfft_cconv_grad_workspace_bytes(self._h))

    @property
    def kernels(self):
        """tfft_cconv_grad_kernels: the input gradient's kernel, then the tap gradient's two."""
        return capi._kernel_lines(self._lib.tfft_cconv_grad_kernels, self._h)

    def set_taps(self, h, stream=None):
        """Hands the taps over (tfft_cconv_grad_set_taps): [channels][taps] float16; only the input gradient needs them."""
        import torch

        self._check_taps(h)
        with torch.cuda.device(self.device):
            _check(self._lib.tfft_cconv_grad_set_taps(self._h, h.data_ptr(), self._stream(stream)))

    def spectrum(self):
        """tfft_cconv_grad_spectrum: (h_re, h_im), H as two CUDA float16 tensors [channels, 4096] (not conjugated)."""
        return self._spectrum(self._lib.tfft_cconv_grad_spectrum)

    def set_workspace(self, tensor):
        """Hands a torch CUDA tensor in as the workspace of the tap gradient (kept alive by the plan)."""
        _check(self._lib.tfft_cconv_grad_set_workspace(self._h, tensor.data_ptr(), tensor.numel() * tensor.element_size()))
        self._ws = tensor

    def prepare(self):
        """Allocates the plan's own workspace now (tfft_cconv_grad_prepare): later tap gradients only launch kernels."""
        _check(self._lib.tfft_cconv_grad_prepare(self._h))

    def input_grad_ptr(self, g, future, dx, stream=0):
        _check(self._lib.tfft_cconv_grad_exec_input_grad(self._h, g, future, dx, stream))

    def tap_grad_ptr(self, x, history, g, dh, stream=0):
        _check(self._lib.tfft_cconv_grad_exec_tap_grad(self._h, x, history, g, dh, stream))

    def input_grad(self, g, dx, future=None, stream=None):
        """g, dx, future: flat CUDA float16 tensors, sequence (b, c) at (b * channels + c) * its seq stride; future = None: zeros."""
        import torch

        self._check_seqs(g, self.g_seq_stride, self.length)
        self._check_seqs(dx, self.dx_seq_stride, self.length)
        if future is not None:
            self._check_seqs(future, self.fut_seq_stride, self.future, "futures")
        with torch.cuda.device(self.device):
            self.input_grad_ptr(g.data_ptr(), None if future is None else future.data_ptr(), dx.data_ptr(), self._stream(stream))

    def tap_grad(self, x, g, dh, history=None, stream=None):
        """x, g, history: flat CUDA float16 tensors; dh: a contiguous CUDA float32 tensor of channels * taps elements."""
        import torch

        self._check_seqs(x, self.x_seq_stride, self.length)
        self._check_seqs(g, self.g_seq_stride, self.length)
        if history is not None:
            self._check_seqs(history, self.hist_seq_stride, self.history, "histories")
        if not (_is_cuda(dh, torch.float32) and dh.is_contiguous() and dh.device.index == self.device and dh.numel() >= self.channels * self.taps):
            raise TfftError(5, "the tap gradient must be a contiguous CUDA float32 tensor of channels * taps elements on the plan's device")
        with torch.cuda.device(self.device):
            self.tap_grad_ptr(x.data_ptr(), None if history is None else history.data_ptr(), g.data_ptr(), dh.data_ptr(), self._stream(stream))


# ---- the convenience functions. They take [B, C, L] VIEWS without copying, which is the point of the add-on: a chunk of a longer
# buffer (x = buf[..., t0:t0 + L]) and its history (buf[..., t0 - Hn:t0]) go to the plan as two pointers and one sequence stride.
# A view qualifies when its last dimension is contiguous, its sequences are a multiple of 8 halves >= L apart (batch stride =
# C x that) and it starts on a 16-byte boundary; anything else is made contiguous first, as long_causal_conv does with every input.
# The plans of the last CCONV_CACHE_SIZE (shape, strides, context, device) keys are kept, least recently used first out, one cache
# per operation (a caller who needs only one gradient creates no plan for the other); cconv_cache_clear() releases all three.
CCONV_CACHE_SIZE = 8
_fwd_plans = {}
_dx_plans = {}
_dh_plans = {}


def _strided(t):
    """(tensor, sequence stride): `t` itself where the plan can read it in place, a contiguous copy otherwise"""
    rows, channels, length = t.shape
    ok = (t.stride(2) == 1 or length == 1) and t.data_ptr() % 16 == 0
    stride = length
    if ok and rows * channels > 1:
        stride = t.stride(1) if channels > 1 else t.stride(0)
        ok = stride >= length and stride % 8 == 0 and (rows == 1 or channels == 1 or t.stride(0) == channels * stride)
    if not ok:
        t = t.contiguous()
        stride = length
    return t, stride


def _context(ctx, like, halo, what):
    """the context as the plan takes it: (tensor or None, samples, stride). Longer than halo: its inner `halo` samples (no window
    reaches further), the end of a history, the start of a future."""
    import torch

    if ctx is None or halo == 0 or ctx.shape[-1] == 0:
        return None, 0, 0
    if not (_is_cuda(ctx, torch.float16) and ctx.dim() == 3 and ctx.shape[:2] == like.shape[:2] and ctx.device == like.device):
        raise TfftError(5, f"{what} must be a CUDA float16 tensor (B, C, n) on the device of the sequences")
    if ctx.shape[2] % 8:
        raise TfftError(5, f"{what} must hold a multiple of 8 samples per sequence")
    if ctx.shape[2] > halo:
        ctx = ctx[..., -halo:] if what == "history" else ctx[..., :halo]
    ctx, stride = _strided(ctx)
    return ctx, ctx.shape[2], stride


def _cached(cache, key, make):
    entry = cache.pop(key, None)
    if entry is None:
        entry = [make(), None]
    cache[key] = entry
    while len(cache) > CCONV_CACHE_SIZE:
        cache.pop(next(iter(cache)))[0].close()
    return entry


def _hand_taps(entry, h):
    """set_taps only when (data_ptr, _version) of h changed since the plan's last call, as long_causal_conv does"""
    ident = (h.data_ptr(), h._version) if h.is_contiguous() else None
    if ident is None or entry[1] != ident:
        entry[0].set_taps(h.contiguous().view(-1))
        entry[1] = ident


def cconv_cache_clear():
    """Destroys the plans the chunked_causal_conv* functions cached."""
    for cache in (_fwd_plans, _dx_plans, _dh_plans):
        while cache:
            cache.popitem()[1][0].close()


def _flat(t):
    """the flat tensor from the first element of a qualifying view to the end of its storage: what the plans' exec methods check"""
    return t.as_strided((t.untyped_storage().nbytes() // 2 - t.storage_offset(),), (1,))


def chunked_causal_conv(x, h, history=None):
    """y[b, c, t] = sum_j h[c, j] xe[b, c, t - j], xe = [history | x] with zeros in front: x a CUDA float16 tensor or view [B, C, L],
    h [C, K] with K <= 2049, history None (zeros) or [B, C, Hn], Hn a multiple of 8 (more than halo samples: the last halo are used).
    Neither x nor history is copied when it is a view the plan can read (see above). Returns y [B, C, L], a new tensor."""
    import torch

    if not (_is_cuda(x, torch.float16) and _is_cuda(h, torch.float16) and x.dim() == 3 and h.dim() == 2 and h.shape[0] == x.shape[1]
            and h.device == x.device):
        raise TfftError(5, "chunked_causal_conv takes CUDA float16 tensors x (B, C, L) and h (C, K) on one device")
    rows, channels, length = x.shape
    taps = h.shape[1]
    halo = cconv_geometry(length, taps, rows, channels)[0]
    x, x_stride = _strided(x)
    hist, hn, hist_stride = _context(history, x, halo, "history")
    dev = x.device.index
    entry = _cached(_fwd_plans, (rows, channels, length, taps, dev, x_stride, hn, hist_stride),
                    lambda: TfftChunkedConvPlan(rows, channels, length, taps, dev, in_seq_stride=x_stride, history=hn, hist_seq_stride=hist_stride))
    _hand_taps(entry, h)
    y = torch.empty((rows, channels, length), dtype=torch.float16, device=x.device)
    entry[0].exec(_flat(x), y.view(-1), None if hist is None else _flat(hist))
    return y


def chunked_causal_conv_input_grad(g, h, future=None):
    """dx[b, c, t] = sum_j h[c, j] ge[b, c, t + j], ge = [g | future] with zeros behind: g [B, C, L], h [C, K], future None or
    [B, C, Fn], Fn a multiple of 8 (more than halo samples: the first halo are used). Returns dx [B, C, L], a new tensor."""
    import torch

    if not (_is_cuda(g, torch.float16) and _is_cuda(h, torch.float16) and g.dim() == 3 and h.dim() == 2 and h.shape[0] == g.shape[1]
            and h.device == g.device):
        raise TfftError(5, "chunked_causal_conv_input_grad takes CUDA float16 tensors g (B, C, L) and h (C, K) on one device")
    rows, channels, length = g.shape
    taps = h.shape[1]
    halo = cconv_geometry(length, taps, rows, channels)[0]
    g, g_stride = _strided(g)
    fut, fn, fut_stride = _context(future, g, halo, "future")
    dev = g.device.index
    entry = _cached(_dx_plans, (rows, channels, length, taps, dev, g_stride, fn, fut_stride),
                    lambda: TfftChunkedConvGradPlan(rows, channels, length, taps, dev, g_seq_stride=g_stride, future=fn, fut_seq_stride=fut_stride))
    _hand_taps(entry, h)
    dx = torch.empty((rows, channels, length), dtype=torch.float16, device=g.device)
    entry[0].input_grad(_flat(g), dx.view(-1), None if fut is None else _flat(fut))
    return dx


def chunked_causal_conv_tap_grad(x, g, taps, history=None):
    """dh[c, j] = sum_{b, 0 <= t < L} g[b, c, t] xe[b, c, t - j], j < taps, xe = [history | x]: x, g [B, C, L]. Returns dh [C, taps]
    float32."""
    import torch

    if not (_is_cuda(x, torch.float16) and _is_cuda(g, torch.float16) and x.dim() == 3 and g.shape == x.shape and g.device == x.device):
        raise TfftError(5, "chunked_causal_conv_tap_grad takes CUDA float16 tensors x and g of one shape (B, C, L) on one device")
    rows, channels, length = x.shape
    taps = int(taps)
    halo = cconv_geometry(length, taps, rows, channels)[0]
    x, x_stride = _strided(x)
    g, g_stride = _strided(g)
    hist, hn, hist_stride = _context(history, x, halo, "history")
    dev = x.device.index
    entry = _cached(_dh_plans, (rows, channels, length, taps, dev, x_stride, g_stride, hn, hist_stride),
                    lambda: TfftChunkedConvGradPlan(rows, channels, length, taps, dev, x_seq_stride=x_stride, g_seq_stride=g_stride, history=hn,
                                                    hist_seq_stride=hist_stride))
    dh = torch.empty((channels, taps), dtype=torch.float32, device=x.device)
    entry[0].tap_grad(_flat(x), _flat(g), dh, None if hist is None else _flat(hist))
    return dh


def next_history(x, history, n):
    """The last n samples of [history | x], what the next chunk takes as its history: a VIEW of x whenever L >= n (no copy); otherwise
    the end of `history` (None: zeros) joined to x in a new tensor. n = 0: None."""
    import torch

    n = int(n)
    if n == 0:
        return None
    length = x.shape[-1]
    if length >= n:
        return x[..., length - n:]
    need = n - length
    have = 0 if history is None else history.shape[-1]
    parts = []
    if need > have:
        parts.append(torch.zeros(x.shape[:-1] + (need - have,), dtype=x.dtype, device=x.device))
    if have:
        parts.append(history[..., have - min(have, need):])
    return torch.cat(parts + [x], dim=-1)


_function = None


def _autograd_function():
    """the torch.autograd.Function, built on first use so that importing the package does not import torch"""
    global _function
    if _function is not None:
        return _function
    import torch

    class ChunkedCausalConv(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, h, history):
            ctx.save_for_backward(x, h, history)
            return chunked_causal_conv(x, h, history)

        @staticmethod
        def backward(ctx, g):
            x, h, history = ctx.saved_tensors
            dx = dh = dhist = None
            if ctx.needs_input_grad[0]:
                dx = chunked_causal_conv_input_grad(g, h)            # no future: what later chunks add arrives through their history
            if ctx.needs_input_grad[1]:
                dh = chunked_causal_conv_tap_grad(x, g, h.shape[1], history).to(h.dtype)
            if history is not None and ctx.needs_input_grad[2]:
                # d loss / d history[u] = sum_j h[j] g[u + j - Hn]: the input gradient of a sequence of Hn samples whose own gradient is
                # zero and whose future is the start of g (K - 1 samples reach back into the history, carry_min rounds that up to 8)
                carry_min = cconv_geometry(x.shape[2], h.shape[1])[4]
                if carry_min == 0:
                    dhist = torch.zeros_like(history)
                else:
                    dhist = chunked_causal_conv_input_grad(torch.zeros_like(history), h, g[..., :min(g.shape[2], carry_min)])
            return dx, dh, dhist

    _function = ChunkedCausalConv
    return _function


def differentiable_chunked_causal_conv(x, h, history=None):
    """chunked_causal_conv(x, h, history) with a grad_fn: the backward pass runs the gradient plans, each only when its input needs a
    gradient: dx (no future), dh cast to h.dtype, and the gradient of `history`, which autograd adds to the previous chunk's dx
    when the history is a view of it (next_history). A history longer than halo is cut to its last halo samples first."""
    if history is not None:
        halo = cconv_geometry(x.shape[2], h.shape[1])[0]
        if halo == 0:
            history = None
        elif history.shape[-1] > halo:
            history = history[..., history.shape[-1] - halo:]
    return _autograd_function().apply(x, h, history)
