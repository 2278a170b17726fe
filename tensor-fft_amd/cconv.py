"""ctypes binding of include/tfft_cconv.h (libtfft_cconv.so, the carried convolution add-on: the overlap-save causal convolution
and its gradients on a chunk of a longer sequence, with the history in front of x and the future behind g read in place), and the
torch.autograd hook over it. No fallback of any kind: torch supplies memory, streams and the autograd graph, nothing else. What the
convolution bindings share lives in _conv_common.py, the rules for views and contexts among it."""
import ctypes
import os

from . import _binding
from . import _conv_common as common
from . import conv
from ._conv_common import _context, _flat_view, _ptr, _strided

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_cconv.so"
_PREFIX = "tfft_cconv_"

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


def _prototypes():
    vp, u64, u32, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t
    pu64 = ctypes.POINTER(u64)
    return {
        "tfft_cconv_geometry": (ci, [u64, u64, pu64, pu64, pu64, pu64]),
        "tfft_cconv_plan_create": (ci, [u64, u64, u64, u64, ci, ctypes.POINTER(CconvOpts), ctypes.POINTER(vp)]),
        "tfft_cconv_plan_destroy": (None, [vp]),
        "tfft_cconv_plan_set_taps": (ci, [vp, vp, vp]),
        "tfft_cconv_plan_spectrum": (ci, [vp, vp, vp]),
        "tfft_cconv_exec": (ci, [vp, vp, vp, vp, vp]),
        "tfft_cconv_plan_num_launches": (ci, [vp]),
        "tfft_cconv_plan_kernels": (ci, [vp, ctypes.c_char_p, sz]),
        "tfft_cconv_describe": (ci, [u64, u64, u64, u64, ci, ctypes.c_char_p, sz]),
        "tfft_cconv_grad_geometry": (ci, [u64, u64, u64, u64, u32, pu64, pu64, pu64, pu64, pu64]),
        "tfft_cconv_grad_create": (ci, [u64, u64, u64, u64, ci, ctypes.POINTER(CconvGradOpts), ctypes.POINTER(vp)]),
        "tfft_cconv_grad_destroy": (None, [vp]),
        "tfft_cconv_grad_set_taps": (ci, [vp, vp, vp]),
        "tfft_cconv_grad_spectrum": (ci, [vp, vp, vp]),
        "tfft_cconv_grad_workspace_bytes": (sz, [vp]),
        "tfft_cconv_grad_set_workspace": (ci, [vp, vp, sz]),
        "tfft_cconv_grad_prepare": (ci, [vp]),
        "tfft_cconv_grad_exec_input_grad": (ci, [vp, vp, vp, vp, vp]),
        "tfft_cconv_grad_exec_tap_grad": (ci, [vp, vp, vp, vp, vp, vp]),
        "tfft_cconv_grad_num_launches": (ci, [vp]),
        "tfft_cconv_grad_kernels": (ci, [vp, ctypes.c_char_p, sz]),
        "tfft_cconv_grad_describe": (ci, [u64, u64, u64, u64, u32, ci, ctypes.c_char_p, sz]),
        "tfft_cconv_last_error": (ctypes.c_char_p, []),
    }


_lib = None


def load_cconv_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_cconv.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is None:
        _lib = _binding._load(conv.load_conv_library, cconv_lib_path(), "carried convolution", _prototypes())
    return _lib


def cconv_geometry(length, taps, rows=1, channels=1, partials=0):
    """tfft_cconv_grad_geometry: (halo, hop, segments, P, carry_min): the geometry of sconv_geometry, the partial sums per channel of
    the tap gradient under the cap `partials` (0 = none), and K - 1 rounded up to a multiple of 8, the smallest context that loses
    nothing. Host only."""
    L = load_cconv_library()
    out = [ctypes.c_uint64() for _ in range(5)]
    _binding._check(L, _PREFIX, L.tfft_cconv_grad_geometry(int(length), int(taps), int(rows), int(channels), int(partials),
                                                         *[ctypes.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def cconv_describe(length, taps, rows=1, channels=1, partials=0):
    """(tfft_cconv_describe, tfft_cconv_grad_describe): ("cconv4096:4096 x S", "cconv4096:4096 x S | partials P"). Host only."""
    L = load_cconv_library()
    fwd, grad = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
    _binding._check(L, _PREFIX, L.tfft_cconv_describe(int(length), int(taps), int(rows), int(channels), 0, fwd, len(fwd)))
    _binding._check(L, _PREFIX, L.tfft_cconv_grad_describe(int(length), int(taps), int(rows), int(channels), int(partials), 0, grad, len(grad)))
    return fwd.value.decode(), grad.value.decode()


class TfftChunkedConvPlan(common._Taps, common._SeqPlan):
    """Owning wrapper of tfft_cconv_plan: TfftLongConvPlan on a chunk of a longer sequence. y[b][c][t] = sum_j h[c][j] xe[b][c][t - j],
    xe the input with `history` (a multiple of 8, at most halo) samples of context in front of it, read from a second pointer
    (include/tfft_cconv.h). exec(x, y, hist) with hist = None reads zeros there. The output must not overlap the input or the history;
    the input and the history may be views of one buffer."""
    _prefix, _names_short = _PREFIX, True

    def __init__(self, rows, channels, length, taps, device=0, in_seq_stride=0, out_seq_stride=0, launch_iters=0, history=0, hist_seq_stride=0):
        L = load_cconv_library()
        opts = CconvOpts(ctypes.sizeof(CconvOpts), 0, int(in_seq_stride), int(out_seq_stride), int(launch_iters), 0, int(history), int(hist_seq_stride))
        self._create(L, L.tfft_cconv_plan_create, rows, channels, length, taps, device, opts)
        self.n = CCONV_N
        self.halo, self.hop, self.segments, _, self.carry_min = cconv_geometry(length, taps, rows, channels)
        self.in_seq_stride = int(in_seq_stride) or self.length
        self.out_seq_stride = int(out_seq_stride) or self.length
        self.history = int(history)
        self.hist_seq_stride = int(hist_seq_stride) or self.history

    def exec_ptr(self, src, hist, dst, stream=0):
        self._check(self._lib.tfft_cconv_exec(self._h, src, hist, dst, stream))

    def exec(self, x, y, hist=None, stream=None):
        """x, y, hist: flat CUDA float16 tensors, sequence (b, c) at (b * channels + c) * its seq stride; hist = None: zeros."""
        import torch

        self._check_seqs(x, self.in_seq_stride)
        self._check_seqs(y, self.out_seq_stride)
        if hist is not None:
            self._check_seqs(hist, self.hist_seq_stride, self.history, "histories")
        with torch.cuda.device(self.device):
            self.exec_ptr(x.data_ptr(), _ptr(hist), y.data_ptr(), self._stream(stream))


class TfftChunkedConvGradPlan(common._Taps, _binding._Workspace, common._SeqPlan):
    """Owning wrapper of tfft_cconv_grad: TfftLongConvGradPlan on a chunk of a longer sequence. input_grad(g, dx, future) reads
    `future` samples of g behind sample L from a second pointer; tap_grad(x, g, dh, history) reads `history` samples of x in front
    of sample 0 from one (include/tfft_cconv.h). None reads zeros. Only the input gradient needs the taps; the workspace is the tap
    gradient's; `kernels` lists the input gradient's kernel, then the tap gradient's two."""
    _prefix, _plan, _names_short = _PREFIX, "grad_", True

    def __init__(self, rows, channels, length, taps, device=0, x_seq_stride=0, g_seq_stride=0, dx_seq_stride=0, launch_iters=0, partials=0,
                 history=0, hist_seq_stride=0, future=0, fut_seq_stride=0):
        L = load_cconv_library()
        opts = CconvGradOpts(ctypes.sizeof(CconvGradOpts), 0, int(x_seq_stride), int(g_seq_stride), int(dx_seq_stride), int(launch_iters),
                             int(partials), 0, int(history), int(hist_seq_stride), int(future), int(fut_seq_stride))
        self._create(L, L.tfft_cconv_grad_create, rows, channels, length, taps, device, opts)
        self.n = CCONV_N
        self.halo, self.hop, self.segments, self.partials, self.carry_min = cconv_geometry(length, taps, rows, channels, partials)
        self.x_seq_stride = int(x_seq_stride) or self.length
        self.g_seq_stride = int(g_seq_stride) or self.length
        self.dx_seq_stride = int(dx_seq_stride) or self.length
        self.history, self.future = int(history), int(future)
        self.hist_seq_stride = int(hist_seq_stride) or self.history
        self.fut_seq_stride = int(fut_seq_stride) or self.future

    def input_grad_ptr(self, g, future, dx, stream=0):
        self._check(self._lib.tfft_cconv_grad_exec_input_grad(self._h, g, future, dx, stream))

    def tap_grad_ptr(self, x, history, g, dh, stream=0):
        self._check(self._lib.tfft_cconv_grad_exec_tap_grad(self._h, x, history, g, dh, stream))

    def input_grad(self, g, dx, future=None, stream=None):
        """g, dx, future: flat CUDA float16 tensors, sequence (b, c) at (b * channels + c) * its seq stride; future = None: zeros."""
        import torch

        self._check_seqs(g, self.g_seq_stride)
        self._check_seqs(dx, self.dx_seq_stride)
        if future is not None:
            self._check_seqs(future, self.fut_seq_stride, self.future, "futures")
        with torch.cuda.device(self.device):
            self.input_grad_ptr(g.data_ptr(), _ptr(future), dx.data_ptr(), self._stream(stream))

    def tap_grad(self, x, g, dh, history=None, stream=None):
        """x, g, history: flat CUDA float16 tensors; dh: a contiguous CUDA float32 tensor of channels * taps elements."""
        import torch

        self._check_seqs(x, self.x_seq_stride)
        self._check_seqs(g, self.g_seq_stride)
        if history is not None:
            self._check_seqs(history, self.hist_seq_stride, self.history, "histories")
        self._check_grad(dh, self.channels * self.taps, "tap")
        with torch.cuda.device(self.device):
            self.tap_grad_ptr(x.data_ptr(), _ptr(history), g.data_ptr(), dh.data_ptr(), self._stream(stream))


# ---- the convenience functions. They take [B, C, L] VIEWS without copying, which is the point of the add-on: a chunk of a longer
# buffer (x = buf[..., t0:t0 + L]) and its history (buf[..., t0 - Hn:t0]) go to the plan as two pointers and one sequence stride.
# A view qualifies when its last dimension is contiguous, its sequences are a multiple of 8 halves >= L apart (batch stride =
# C x that) and it starts on a 16-byte boundary; anything else is made contiguous first, as long_causal_conv does with every input
# (_conv_common._strided). The plans of the last CCONV_CACHE_SIZE (shape, strides, context, device) keys are kept, least recently
# used first out, one cache per operation (a caller who needs only one gradient creates no plan for the other); cconv_cache_clear()
# releases all three.
CCONV_CACHE_SIZE = 8
_fwd_plans = {}
_dx_plans = {}
_dh_plans = {}


def cconv_cache_clear():
    """Destroys the plans the chunked_causal_conv* functions cached."""
    _binding._cache_clear(_fwd_plans, _dx_plans, _dh_plans)


def chunked_causal_conv(x, h, history=None):
    """y[b, c, t] = sum_j h[c, j] xe[b, c, t - j], xe = [history | x] with zeros in front: x a CUDA float16 tensor or view [B, C, L],
    h [C, K] with K <= 2049, history None (zeros) or [B, C, Hn], Hn a multiple of 8 (more than halo samples: the last halo are used).
    Neither x nor history is copied when it is a view the plan can read (see above). Returns y [B, C, L], a new tensor."""
    import torch

    common._check_tap_args("chunked_causal_conv takes CUDA float16 tensors x (B, C, L) and h (C, K) on one device", (x,), (), h)
    rows, channels, length = x.shape
    taps = h.shape[1]
    halo = cconv_geometry(length, taps, rows, channels)[0]
    x, x_stride = _strided(x)
    hist, hn, hist_stride = _context(history, x, halo, "history")
    dev = x.device.index
    entry = _binding._cached(_fwd_plans, CCONV_CACHE_SIZE, (rows, channels, length, taps, dev, x_stride, hn, hist_stride),
                           lambda: TfftChunkedConvPlan(rows, channels, length, taps, dev, in_seq_stride=x_stride, history=hn, hist_seq_stride=hist_stride))
    common._hand_taps(entry, h)
    y = torch.empty((rows, channels, length), dtype=torch.float16, device=x.device)
    entry[0].exec(_flat_view(x), y.view(-1), _flat_view(hist))
    return y


def chunked_causal_conv_input_grad(g, h, future=None):
    """dx[b, c, t] = sum_j h[c, j] ge[b, c, t + j], ge = [g | future] with zeros behind: g [B, C, L], h [C, K], future None or
    [B, C, Fn], Fn a multiple of 8 (more than halo samples: the first halo are used). Returns dx [B, C, L], a new tensor."""
    import torch

    common._check_tap_args("chunked_causal_conv_input_grad takes CUDA float16 tensors g (B, C, L) and h (C, K) on one device", (g,), (), h)
    rows, channels, length = g.shape
    taps = h.shape[1]
    halo = cconv_geometry(length, taps, rows, channels)[0]
    g, g_stride = _strided(g)
    fut, fn, fut_stride = _context(future, g, halo, "future")
    dev = g.device.index
    entry = _binding._cached(_dx_plans, CCONV_CACHE_SIZE, (rows, channels, length, taps, dev, g_stride, fn, fut_stride),
                           lambda: TfftChunkedConvGradPlan(rows, channels, length, taps, dev, g_seq_stride=g_stride, future=fn, fut_seq_stride=fut_stride))
    common._hand_taps(entry, h)
    dx = torch.empty((rows, channels, length), dtype=torch.float16, device=g.device)
    entry[0].input_grad(_flat_view(g), dx.view(-1), _flat_view(fut))
    return dx


def chunked_causal_conv_tap_grad(x, g, taps, history=None):
    """dh[c, j] = sum_{b, 0 <= t < L} g[b, c, t] xe[b, c, t - j], j < taps, xe = [history | x]: x, g [B, C, L]. Returns dh [C, taps]
    float32."""
    import torch

    common._check_seq_args("chunked_causal_conv_tap_grad takes CUDA float16 tensors x and g of one shape (B, C, L) on one device", (x, g))
    rows, channels, length = x.shape
    taps = int(taps)
    halo = cconv_geometry(length, taps, rows, channels)[0]
    x, x_stride = _strided(x)
    g, g_stride = _strided(g)
    hist, hn, hist_stride = _context(history, x, halo, "history")
    dev = x.device.index
    entry = _binding._cached(_dh_plans, CCONV_CACHE_SIZE, (rows, channels, length, taps, dev, x_stride, g_stride, hn, hist_stride),
                           lambda: TfftChunkedConvGradPlan(rows, channels, length, taps, dev, x_seq_stride=x_stride, g_seq_stride=g_stride, history=hn,
                                                           hist_seq_stride=hist_stride))
    dh = torch.empty((channels, taps), dtype=torch.float32, device=x.device)
    entry[0].tap_grad(_flat_view(x), _flat_view(g), dh, _flat_view(hist))
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
