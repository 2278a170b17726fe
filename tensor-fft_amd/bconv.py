"""ctypes binding of include/tfft_bconv.h (libtfft_bconv.so, the gradients of the overlap-save causal convolution), and the
torch.autograd hook over it. No fallback of any kind: torch supplies memory, streams and the autograd graph, nothing else. What the
convolution bindings share lives in _conv_common.py."""
import ctypes
import os

from . import _binding
from . import _conv_common as common
from . import conv, sconv

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_bconv.so"
_PREFIX = "tfft_bconv_"

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


def _prototypes():
    vp, u64, u32, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t
    pu64 = ctypes.POINTER(u64)
    return {
        "tfft_bconv_geometry": (ci, [u64, u64, u64, u64, u32, pu64, pu64, pu64, pu64]),
        "tfft_bconv_plan_create": (ci, [u64, u64, u64, u64, ci, ctypes.POINTER(BconvOpts), ctypes.POINTER(vp)]),
        "tfft_bconv_plan_destroy": (None, [vp]),
        "tfft_bconv_plan_set_taps": (ci, [vp, vp, vp]),
        "tfft_bconv_plan_spectrum": (ci, [vp, vp, vp]),
        "tfft_bconv_plan_workspace_bytes": (sz, [vp]),
        "tfft_bconv_plan_set_workspace": (ci, [vp, vp, sz]),
        "tfft_bconv_plan_prepare": (ci, [vp]),
        "tfft_bconv_exec_input_grad": (ci, [vp, vp, vp, vp]),
        "tfft_bconv_exec_tap_grad": (ci, [vp, vp, vp, vp, vp]),
        "tfft_bconv_plan_num_launches": (ci, [vp]),
        "tfft_bconv_plan_kernels": (ci, [vp, ctypes.c_char_p, sz]),
        "tfft_bconv_describe": (ci, [u64, u64, u64, u64, u32, ci, ctypes.c_char_p, sz]),
        "tfft_bconv_last_error": (ctypes.c_char_p, []),
    }


_lib = None


def load_bconv_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_bconv.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is None:
        _lib = _binding._load(conv.load_conv_library, bconv_lib_path(), "convolution gradient", _prototypes())
    return _lib


def bconv_geometry(length, taps, rows=1, channels=1, partials=0):
    """tfft_bconv_geometry: (halo, hop, segments, P): the geometry of sconv_geometry and the partial sums per channel of the tap
    gradient under the cap `partials` (0 = none). Host only."""
    L = load_bconv_library()
    out = [ctypes.c_uint64() for _ in range(4)]
    _binding._check(L, _PREFIX, L.tfft_bconv_geometry(int(length), int(taps), int(rows), int(channels), int(partials), *[ctypes.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def bconv_describe(length, taps, rows=1, channels=1, partials=0):
    """tfft_bconv_describe: "bconv4096:4096 x S | partials P". Host only, no GPU needed."""
    L = load_bconv_library()
    buf = ctypes.create_string_buffer(128)
    _binding._check(L, _PREFIX, L.tfft_bconv_describe(int(length), int(taps), int(rows), int(channels), int(partials), 0, buf, len(buf)))
    return buf.value.decode()


class TfftLongConvGradPlan(common._Taps, _binding._Workspace, common._SeqPlan):
    """Owning wrapper of tfft_bconv_plan: the two gradients of TfftLongConvPlan for rows x channels real fp16 sequences of `length`
    samples and `taps` <= 2049 taps per channel (include/tfft_bconv.h). input_grad(g, dx) needs set_taps(h) first; tap_grad(x, g, dh)
    writes [channels][taps] float32 and needs no taps. `partials` caps the partial sums per channel (0 = the library's default); the
    tap gradient depends on it through the order of fp32 additions only. The workspace is the tap gradient's; `kernels` lists the
    input gradient's kernel, then the tap gradient's two."""
    _prefix = _PREFIX

    def __init__(self, rows, channels, length, taps, device=0, x_seq_stride=0, g_seq_stride=0, dx_seq_stride=0, launch_iters=0, partials=0):
        L = load_bconv_library()
        opts = BconvOpts(ctypes.sizeof(BconvOpts), 0, int(x_seq_stride), int(g_seq_stride), int(dx_seq_stride), int(launch_iters), int(partials), 0)
        self._create(L, L.tfft_bconv_plan_create, rows, channels, length, taps, device, opts)
        self.n = BCONV_N
        self.halo, self.hop, self.segments, self.partials = bconv_geometry(length, taps, rows, channels, partials)
        self.x_seq_stride = int(x_seq_stride) or self.length
        self.g_seq_stride = int(g_seq_stride) or self.length
        self.dx_seq_stride = int(dx_seq_stride) or self.length

    def input_grad_ptr(self, g, dx, stream=0):
        self._check(self._lib.tfft_bconv_exec_input_grad(self._h, g, dx, stream))

    def tap_grad_ptr(self, x, g, dh, stream=0):
        self._check(self._lib.tfft_bconv_exec_tap_grad(self._h, x, g, dh, stream))

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
        self._check_grad(dh, self.channels * self.taps, "tap")
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
    return _binding._cached(cache, BCONV_CACHE_SIZE, key, lambda: TfftLongConvGradPlan(rows, channels, length, taps, device))


def bconv_cache_clear():
    """Destroys the plans long_causal_conv_input_grad and long_causal_conv_tap_grad cached."""
    _binding._cache_clear(_dx_plans, _dh_plans)


def long_causal_conv_input_grad(g, h):
    """dx[b, c, t] = sum_j h[c, j] g[b, c, t + j]: g a CUDA float16 tensor [B, C, L], h [C, K] with K <= 2049. Returns dx [B, C, L], a
    new tensor. The taps are handed to the cached plan again only when (data_ptr, _version) of h changed since the last call."""
    import torch

    common._check_tap_args("long_causal_conv_input_grad takes CUDA float16 tensors g (B, C, L) and h (C, K) on one device", (g,), (), h)
    rows, channels, length = g.shape
    entry = _plan_for(_dx_plans, rows, channels, length, h.shape[1], g.device.index)
    common._hand_taps(entry, h)
    g = g.contiguous()
    dx = torch.empty_like(g)
    entry[0].input_grad(g.view(-1), dx.view(-1))
    return dx


def long_causal_conv_tap_grad(x, g, taps):
    """dh[c, j] = sum_{b, t} g[b, c, t] x[b, c, t - j], j < taps: x, g CUDA float16 tensors [B, C, L]. Returns dh [C, taps] float32."""
    import torch

    common._check_seq_args("long_causal_conv_tap_grad takes CUDA float16 tensors x and g of one shape (B, C, L) on one device", (x, g))
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
