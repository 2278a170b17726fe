"""ctypes binding of include/tfft_gcconv.h (libtfft_gcconv.so, the gated carried convolution add-on: the gated overlap-save causal
convolution and its gradients on a chunk of a longer sequence, with the history in front of x and the pre gate and the future behind
gy and the post gate read in place), and the torch.autograd hook over it. No fallback of any kind: torch supplies memory, streams
and the autograd graph, nothing else. What the convolution bindings share lives in _conv_common.py. The tap gradient's function
refuses a missing gy with a message of its own, after the shared argument check: kept here."""
import ctypes
import os

from . import _binding
from . import _conv_common as common
from . import conv
from ._binding import TfftError
from ._conv_common import _context, _flags, _flat_view, _ptr, _strided
from .cconv import next_history  # noqa: F401  (next_history serves x and the pre gate alike)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_gcconv.so"
_PREFIX = "tfft_gcconv_"

# every symbol include/tfft_gcconv.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_gcconv_geometry", "tfft_gcconv_plan_create", "tfft_gcconv_plan_destroy", "tfft_gcconv_plan_set_taps", "tfft_gcconv_plan_spectrum",
    "tfft_gcconv_exec", "tfft_gcconv_plan_num_launches", "tfft_gcconv_plan_kernels", "tfft_gcconv_describe",
    "tfft_gcconv_grad_geometry", "tfft_gcconv_grad_create", "tfft_gcconv_grad_destroy", "tfft_gcconv_grad_set_taps", "tfft_gcconv_grad_spectrum",
    "tfft_gcconv_grad_workspace_bytes", "tfft_gcconv_grad_set_workspace", "tfft_gcconv_grad_prepare", "tfft_gcconv_grad_exec_input_grad",
    "tfft_gcconv_grad_exec_tap_grad", "tfft_gcconv_grad_num_launches", "tfft_gcconv_grad_kernels", "tfft_gcconv_grad_describe",
    "tfft_gcconv_last_error",
]
GCCONV_PRE_GATE, GCCONV_POST_GATE = 1, 2                      # the flags of both option structs
GCCONV_MAX_TAPS = 2049                                        # TFFT_GCCONV_MAX_TAPS
GCCONV_N = 4096                                               # the transform length of every plan


class GcconvOpts(ctypes.Structure):
    """tfft_gcconv_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_seq_stride", ctypes.c_uint64),
                ("out_seq_stride", ctypes.c_uint64), ("pre_seq_stride", ctypes.c_uint64), ("post_seq_stride", ctypes.c_uint64),
                ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int), ("history", ctypes.c_uint64),
                ("hist_seq_stride", ctypes.c_uint64), ("pre_hist_seq_stride", ctypes.c_uint64)]


class GcconvGradOpts(ctypes.Structure):
    """tfft_gcconv_grad_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("x_seq_stride", ctypes.c_uint64),
                ("pre_seq_stride", ctypes.c_uint64), ("gy_seq_stride", ctypes.c_uint64), ("post_seq_stride", ctypes.c_uint64),
                ("dx_seq_stride", ctypes.c_uint64), ("dpre_seq_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32),
                ("partials", ctypes.c_uint32), ("flags", ctypes.c_int), ("history", ctypes.c_uint64), ("hist_seq_stride", ctypes.c_uint64),
                ("pre_hist_seq_stride", ctypes.c_uint64), ("future", ctypes.c_uint64), ("fut_seq_stride", ctypes.c_uint64),
                ("post_fut_seq_stride", ctypes.c_uint64)]


def gcconv_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


def _prototypes():
    vp, u64, u32, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t
    pu64 = ctypes.POINTER(u64)
    return {
        "tfft_gcconv_geometry": (ci, [u64, u64, pu64, pu64, pu64, pu64]),
        "tfft_gcconv_plan_create": (ci, [u64, u64, u64, u64, ci, ctypes.POINTER(GcconvOpts), ctypes.POINTER(vp)]),
        "tfft_gcconv_plan_destroy": (None, [vp]),
        "tfft_gcconv_plan_set_taps": (ci, [vp, vp, vp, vp]),
        "tfft_gcconv_plan_spectrum": (ci, [vp, vp, vp]),
        "tfft_gcconv_exec": (ci, [vp] * 8),
        "tfft_gcconv_plan_num_launches": (ci, [vp]),
        "tfft_gcconv_plan_kernels": (ci, [vp, ctypes.c_char_p, sz]),
        "tfft_gcconv_describe": (ci, [u64, u64, u64, u64, ci, ctypes.c_char_p, sz]),
        "tfft_gcconv_grad_geometry": (ci, [u64, u64, u64, u64, u32, pu64, pu64, pu64, pu64, pu64]),
        "tfft_gcconv_grad_create": (ci, [u64, u64, u64, u64, ci, ctypes.POINTER(GcconvGradOpts), ctypes.POINTER(vp)]),
        "tfft_gcconv_grad_destroy": (None, [vp]),
        "tfft_gcconv_grad_set_taps": (ci, [vp, vp, vp, vp]),
        "tfft_gcconv_grad_spectrum": (ci, [vp, vp, vp]),
        "tfft_gcconv_grad_workspace_bytes": (sz, [vp]),
        "tfft_gcconv_grad_set_workspace": (ci, [vp, vp, sz]),
        "tfft_gcconv_grad_prepare": (ci, [vp]),
        "tfft_gcconv_grad_exec_input_grad": (ci, [vp] * 10),
        "tfft_gcconv_grad_exec_tap_grad": (ci, [vp] * 10),
        "tfft_gcconv_grad_num_launches": (ci, [vp]),
        "tfft_gcconv_grad_kernels": (ci, [vp, ctypes.c_char_p, sz]),
        "tfft_gcconv_grad_describe": (ci, [u64, u64, u64, u64, u32, ci, ctypes.c_char_p, sz]),
        "tfft_gcconv_last_error": (ctypes.c_char_p, []),
    }


_lib = None


def load_gcconv_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_gcconv.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is None:
        _lib = _binding._load(conv.load_conv_library, gcconv_lib_path(), "gated carried convolution", _prototypes())
    return _lib


def gcconv_geometry(length, taps, rows=1, channels=1, partials=0):
    """tfft_gcconv_grad_geometry: (halo, hop, segments, P, carry_min), as cconv_geometry. Host only."""
    L = load_gcconv_library()
    out = [ctypes.c_uint64() for _ in range(5)]
    _binding._check(L, _PREFIX, L.tfft_gcconv_grad_geometry(int(length), int(taps), int(rows), int(channels), int(partials),
                                                          *[ctypes.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def gcconv_describe(length, taps, rows=1, channels=1, partials=0, pre_gate=False, post_gate=False):
    """(tfft_gcconv_describe, tfft_gcconv_grad_describe): ("gcconv4096:4096[:gates] x S", "gcconv4096:4096[:gates] x S | partials P").
    Host only."""
    L = load_gcconv_library()
    fwd, grad = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
    _binding._check(L, _PREFIX, L.tfft_gcconv_describe(int(length), int(taps), int(rows), int(channels), _flags(pre_gate, post_gate), fwd, len(fwd)))
    _binding._check(L, _PREFIX, L.tfft_gcconv_grad_describe(int(length), int(taps), int(rows), int(channels), int(partials), _flags(pre_gate, post_gate),
                                                          grad, len(grad)))
    return fwd.value.decode(), grad.value.decode()


class TfftGatedChunkedConvPlan(common._GatedTaps, common._SeqPlan):
    """Owning wrapper of tfft_gcconv_plan: TfftGatedLongConvPlan on a chunk of a longer sequence. y = post * (h' * (pe * xe)), xe and pe
    the input and the pre gate with `history` (a multiple of 8, at most halo) samples of context in front of them, each read from a
    second pointer (include/tfft_gcconv.h). exec(x, y, pre, post, hist, pre_hist) with hist = None reads zeros there."""
    _prefix, _names_short = _PREFIX, True

    def __init__(self, rows, channels, length, taps, device=0, pre_gate=False, post_gate=False, in_seq_stride=0, out_seq_stride=0,
                 pre_seq_stride=0, post_seq_stride=0, launch_iters=0, history=0, hist_seq_stride=0, pre_hist_seq_stride=0):
        L = load_gcconv_library()
        opts = GcconvOpts(ctypes.sizeof(GcconvOpts), 0, int(in_seq_stride), int(out_seq_stride), int(pre_seq_stride), int(post_seq_stride),
                          int(launch_iters), _flags(pre_gate, post_gate), int(history), int(hist_seq_stride), int(pre_hist_seq_stride))
        self._create(L, L.tfft_gcconv_plan_create, rows, channels, length, taps, device, opts)
        self.pre_gate, self.post_gate = bool(pre_gate), bool(post_gate)
        self.n = GCCONV_N
        self.halo, self.hop, self.segments, _, self.carry_min = gcconv_geometry(length, taps, rows, channels)
        self.in_seq_stride = int(in_seq_stride) or self.length
        self.out_seq_stride = int(out_seq_stride) or self.length
        self.pre_seq_stride = int(pre_seq_stride) or self.length
        self.post_seq_stride = int(post_seq_stride) or self.length
        self.history = int(history)
        self.hist_seq_stride = int(hist_seq_stride) or self.history
        self.pre_hist_seq_stride = int(pre_hist_seq_stride) or self.history

    def exec_ptr(self, src, dst, pre=None, post=None, hist=None, pre_hist=None, stream=0):
        self._check(self._lib.tfft_gcconv_exec(self._h, src, pre, post, hist, pre_hist, dst, stream))

    def exec(self, x, y, pre=None, post=None, hist=None, pre_hist=None, stream=None):
        """x, y, pre, post, hist, pre_hist: flat CUDA float16 tensors, sequence (b, c) at (b * channels + c) * its seq stride; hist = None:
        zeros. The library refuses a gate the plan does not have, misses one it has, and wants pre_hist exactly with hist and a pre gate."""
        import torch

        for t, stride in ((x, self.in_seq_stride), (y, self.out_seq_stride), (pre, self.pre_seq_stride), (post, self.post_seq_stride)):
            self._check_seqs(t, stride)
        self._check_seqs(hist, self.hist_seq_stride, self.history, "histories")
        self._check_seqs(pre_hist, self.pre_hist_seq_stride, self.history, "histories")
        with torch.cuda.device(self.device):
            self.exec_ptr(x.data_ptr(), y.data_ptr(), _ptr(pre), _ptr(post), _ptr(hist), _ptr(pre_hist), self._stream(stream))


class TfftGatedChunkedConvGradPlan(common._GatedTaps, _binding._Workspace, common._SeqPlan):
    """Owning wrapper of tfft_gcconv_grad: TfftGatedLongConvGradPlan on a chunk of a longer sequence. input_grad reads `future` samples
    of gy and of the post gate behind sample L, tap_grad reads `history` samples of x and of the pre gate in front of sample 0, each
    from a pointer of its own (include/tfft_gcconv.h). None reads zeros. Only the input gradient needs the taps; the workspace is
    the tap gradient's; `kernels` lists the input gradient's kernel, then the tap gradient's two."""
    _prefix, _plan, _names_short = _PREFIX, "grad_", True

    def __init__(self, rows, channels, length, taps, device=0, pre_gate=False, post_gate=False, x_seq_stride=0, pre_seq_stride=0,
                 gy_seq_stride=0, post_seq_stride=0, dx_seq_stride=0, dpre_seq_stride=0, launch_iters=0, partials=0, history=0,
                 hist_seq_stride=0, pre_hist_seq_stride=0, future=0, fut_seq_stride=0, post_fut_seq_stride=0):
        L = load_gcconv_library()
        opts = GcconvGradOpts(ctypes.sizeof(GcconvGradOpts), 0, int(x_seq_stride), int(pre_seq_stride), int(gy_seq_stride), int(post_seq_stride),
                              int(dx_seq_stride), int(dpre_seq_stride), int(launch_iters), int(partials), _flags(pre_gate, post_gate),
                              int(history), int(hist_seq_stride), int(pre_hist_seq_stride), int(future), int(fut_seq_stride),
                              int(post_fut_seq_stride))
        self._create(L, L.tfft_gcconv_grad_create, rows, channels, length, taps, device, opts)
        self.pre_gate, self.post_gate = bool(pre_gate), bool(post_gate)
        self.n = GCCONV_N
        self.halo, self.hop, self.segments, self.partials, self.carry_min = gcconv_geometry(length, taps, rows, channels, partials)
        self.x_seq_stride = int(x_seq_stride) or self.length
        self.pre_seq_stride = int(pre_seq_stride) or self.length
        self.gy_seq_stride = int(gy_seq_stride) or self.length
        self.post_seq_stride = int(post_seq_stride) or self.length
        self.dx_seq_stride = int(dx_seq_stride) or self.length
        self.dpre_seq_stride = int(dpre_seq_stride) or self.length
        self.history, self.future = int(history), int(future)
        self.hist_seq_stride = int(hist_seq_stride) or self.history
        self.pre_hist_seq_stride = int(pre_hist_seq_stride) or self.history
        self.fut_seq_stride = int(fut_seq_stride) or self.future
        self.post_fut_seq_stride = int(post_fut_seq_stride) or self.future

    def input_grad_ptr(self, gy, dx, post=None, x=None, pre=None, dpre=None, future=None, post_future=None, stream=0):
        self._check(self._lib.tfft_gcconv_grad_exec_input_grad(self._h, gy, post, future, post_future, x, pre, dx, dpre, stream))

    def tap_grad_ptr(self, x, gy, dh, pre=None, post=None, dskip=None, history=None, pre_history=None, stream=0):
        self._check(self._lib.tfft_gcconv_grad_exec_tap_grad(self._h, x, pre, history, pre_history, gy, post, dh, dskip, stream))

    def input_grad(self, gy, dx, post=None, x=None, pre=None, dpre=None, future=None, post_future=None, stream=None):
        """gy, dx, post, x, pre, dpre, future, post_future: flat CUDA float16 tensors, sequence (b, c) at (b * channels + c) * the
        tensor's seq stride; future = None: zeros. dpre = None on a plan with a pre gate writes dx only."""
        import torch

        for t, stride in ((gy, self.gy_seq_stride), (dx, self.dx_seq_stride), (post, self.post_seq_stride), (x, self.x_seq_stride),
                          (pre, self.pre_seq_stride), (dpre, self.dpre_seq_stride)):
            self._check_seqs(t, stride)
        self._check_seqs(future, self.fut_seq_stride, self.future, "futures")
        self._check_seqs(post_future, self.post_fut_seq_stride, self.future, "futures")
        with torch.cuda.device(self.device):
            self.input_grad_ptr(gy.data_ptr(), dx.data_ptr(), _ptr(post), _ptr(x), _ptr(pre), _ptr(dpre), _ptr(future), _ptr(post_future),
                                self._stream(stream))

    def tap_grad(self, x, gy, dh, pre=None, post=None, dskip=None, history=None, pre_history=None, stream=None):
        """x, gy, pre, post, history, pre_history: flat CUDA float16 tensors; dh: a contiguous CUDA float32 tensor of channels * taps
        elements; dskip: one of channels elements, or None."""
        import torch

        for t, stride in ((x, self.x_seq_stride), (gy, self.gy_seq_stride), (pre, self.pre_seq_stride), (post, self.post_seq_stride)):
            self._check_seqs(t, stride)
        self._check_seqs(history, self.hist_seq_stride, self.history, "histories")
        self._check_seqs(pre_history, self.pre_hist_seq_stride, self.history, "histories")
        self._check_grad(dh, self.channels * self.taps, "tap")
        if dskip is not None:
            self._check_grad(dskip, self.channels, "skip")
        with torch.cuda.device(self.device):
            self.tap_grad_ptr(x.data_ptr(), gy.data_ptr(), dh.data_ptr(), _ptr(pre), _ptr(post), _ptr(dskip), _ptr(history), _ptr(pre_history),
                              self._stream(stream))


# ---- the convenience functions. They take [B, C, L] VIEWS without copying, under the rules of cconv.py (_conv_common._strided): a
# chunk of a longer buffer and its history go to the plan as two pointers and one sequence stride, and so do a gate and its history.
# The plans of the last GCCONV_CACHE_SIZE (shape, gates, strides, context, device) keys are kept, least recently used first out, one
# cache per operation; gcconv_cache_clear() releases all three.
GCCONV_CACHE_SIZE = 8
_fwd_plans = {}
_dx_plans = {}
_dh_plans = {}


def gcconv_cache_clear():
    """Destroys the plans the gated_chunked_causal_conv* functions cached."""
    _binding._cache_clear(_fwd_plans, _dx_plans, _dh_plans)


def _takes(name):
    return f"{name} takes CUDA float16 tensors (B, C, L) for the sequences and gates, h (C, K) and skip (C,) on one device"


def _gate_context(ctx, gate_ctx, gate, like, halo, what, gate_what):
    """a sequence's context and its gate's, as the plan takes them: (ctx, gate_ctx, samples, ctx stride, gate_ctx stride). One length
    serves both; the gate's context is wanted exactly when the sequence has one and the gate exists."""
    ctx, n, stride = _context(ctx, like, halo, what)
    if gate is None or ctx is None:
        if gate_ctx is not None and gate_ctx.shape[-1] and halo:
            raise TfftError(5, f"{gate_what} is given without {'its gate' if gate is None else what}")
        return ctx, None, n, stride, 0
    if gate_ctx is None:
        raise TfftError(5, f"{gate_what} is missing: {what} is given and the plan has that gate (one length serves both)")
    gate_ctx, gn, gate_stride = _context(gate_ctx, like, halo, what)
    if gn != n:
        raise TfftError(5, f"{what} and {gate_what} must hold the same number of samples")
    return ctx, gate_ctx, n, stride, gate_stride


def gated_chunked_causal_conv(x, h, pre=None, post=None, skip=None, history=None, pre_history=None):
    """y = post * (h' * (pe * xe)) on a chunk: xe = [history | x], pe = [pre_history | pre], zeros in front; h' = h with skip added to
    tap 0. x, pre, post CUDA float16 tensors or views [B, C, L]; h [C, K], K <= 2049; skip [C] or None; history / pre_history None
    (zeros) or [B, C, Hn], Hn a multiple of 8 (more than halo samples: the last halo are used), pre_history exactly when history and
    pre are given. Nothing is copied that the plan can read in place (cconv.py). Returns y [B, C, L], a new tensor."""
    import torch

    common._check_tap_args(_takes("gated_chunked_causal_conv"), (x,), (pre, post), h, skip)
    rows, channels, length = x.shape
    taps = h.shape[1]
    halo = gcconv_geometry(length, taps, rows, channels)[0]
    x, x_stride = _strided(x)
    pre, pre_stride = _strided(pre)
    post, post_stride = _strided(post)
    hist, phist, hn, hist_stride, phist_stride = _gate_context(history, pre_history, pre, x, halo, "history", "pre_history")
    dev = x.device.index
    key = (rows, channels, length, taps, dev, pre is not None, post is not None, x_stride, pre_stride, post_stride, hn, hist_stride, phist_stride)
    entry = _binding._cached(_fwd_plans, GCCONV_CACHE_SIZE, key, lambda: TfftGatedChunkedConvPlan(
        rows, channels, length, taps, dev, pre_gate=pre is not None, post_gate=post is not None, in_seq_stride=x_stride, pre_seq_stride=pre_stride,
        post_seq_stride=post_stride, history=hn, hist_seq_stride=hist_stride, pre_hist_seq_stride=phist_stride))
    common._hand_taps(entry, h, skip)
    y = torch.empty((rows, channels, length), dtype=torch.float16, device=x.device)
    f = _flat_view
    entry[0].exec(f(x), y.view(-1), pre=f(pre), post=f(post), hist=f(hist), pre_hist=f(phist))
    return y


def gated_chunked_causal_conv_input_grad(gy, h, x=None, pre=None, post=None, skip=None, future=None, post_future=None, want_dpre=True):
    """(dx, dpre) on a chunk: dx = pre * du, dpre = x * du, du[t] = sum_j h'[j] gze[t + j], gze = [post * gy | post_future * future]
    with zeros behind. gy, x, pre, post [B, C, L]; future / post_future None or [B, C, Fn] (more than halo samples: the first halo
    are used), post_future exactly when future and post are given. x is needed exactly when pre is given. dpre is None without a pre
    gate or when want_dpre is false."""
    import torch

    common._check_tap_args(_takes("gated_chunked_causal_conv_input_grad"), (gy,), (x, pre, post), h, skip)
    if (pre is None) != (x is None):
        raise TfftError(5, "gated_chunked_causal_conv_input_grad takes x exactly when it takes pre")
    rows, channels, length = gy.shape
    taps = h.shape[1]
    halo = gcconv_geometry(length, taps, rows, channels)[0]
    gy, gy_stride = _strided(gy)
    post, post_stride = _strided(post)
    x, x_stride = _strided(x)
    pre, pre_stride = _strided(pre)
    fut, pfut, fn, fut_stride, pfut_stride = _gate_context(future, post_future, post, gy, halo, "future", "post_future")
    dev = gy.device.index
    key = (rows, channels, length, taps, dev, pre is not None, post is not None, gy_stride, post_stride, x_stride, pre_stride, fn, fut_stride, pfut_stride)
    entry = _binding._cached(_dx_plans, GCCONV_CACHE_SIZE, key, lambda: TfftGatedChunkedConvGradPlan(
        rows, channels, length, taps, dev, pre_gate=pre is not None, post_gate=post is not None, gy_seq_stride=gy_stride, post_seq_stride=post_stride,
        x_seq_stride=x_stride, pre_seq_stride=pre_stride, future=fn, fut_seq_stride=fut_stride, post_fut_seq_stride=pfut_stride))
    common._hand_taps(entry, h, skip)
    dx = torch.empty((rows, channels, length), dtype=torch.float16, device=gy.device)
    dpre = torch.empty_like(dx) if pre is not None and want_dpre else None
    f = _flat_view
    entry[0].input_grad(f(gy), dx.view(-1), post=f(post), x=f(x), pre=f(pre), dpre=None if dpre is None else dpre.view(-1), future=f(fut),
                        post_future=f(pfut))
    return dx, dpre


def gated_chunked_causal_conv_tap_grad(x, gy, taps, pre=None, post=None, history=None, pre_history=None):
    """(dh, dskip) on a chunk: dh[c, j] = sum_{b, 0 <= t < L} (post * gy)[b, c, t] ue[b, c, t - j], j < taps, ue = [pre_history * history |
    pre * x]; float32 [C, taps], and dskip = dh[:, 0] as a tensor of its own [C]."""
    import torch

    common._check_seq_args(_takes("gated_chunked_causal_conv_tap_grad"), (x,), (gy, pre, post))
    if gy is None:
        raise TfftError(5, "gated_chunked_causal_conv_tap_grad takes gy, a CUDA float16 tensor of the shape of x")
    rows, channels, length = x.shape
    taps = int(taps)
    halo = gcconv_geometry(length, taps, rows, channels)[0]
    x, x_stride = _strided(x)
    gy, gy_stride = _strided(gy)
    pre, pre_stride = _strided(pre)
    post, post_stride = _strided(post)
    hist, phist, hn, hist_stride, phist_stride = _gate_context(history, pre_history, pre, x, halo, "history", "pre_history")
    dev = x.device.index
    key = (rows, channels, length, taps, dev, pre is not None, post is not None, x_stride, gy_stride, pre_stride, post_stride, hn, hist_stride, phist_stride)
    entry = _binding._cached(_dh_plans, GCCONV_CACHE_SIZE, key, lambda: TfftGatedChunkedConvGradPlan(
        rows, channels, length, taps, dev, pre_gate=pre is not None, post_gate=post is not None, x_seq_stride=x_stride, gy_seq_stride=gy_stride,
        pre_seq_stride=pre_stride, post_seq_stride=post_stride, history=hn, hist_seq_stride=hist_stride, pre_hist_seq_stride=phist_stride))
    dh = torch.empty((channels, taps), dtype=torch.float32, device=x.device)
    dskip = torch.empty((channels,), dtype=torch.float32, device=x.device)
    f = _flat_view
    entry[0].tap_grad(f(x), f(gy), dh, pre=f(pre), post=f(post), dskip=dskip, history=f(hist), pre_history=f(phist))
    return dh, dskip


_function = None


def _autograd_function():
    """the torch.autograd.Function, built on first use so that importing the package does not import torch"""
    global _function
    if _function is not None:
        return _function
    import torch

    class GatedChunkedCausalConv(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, h, pre, post, skip, history, pre_history):
            ctx.save_for_backward(x, h, pre, post, skip, history, pre_history)
            return gated_chunked_causal_conv(x, h, pre=pre, post=post, skip=skip, history=history, pre_history=pre_history)

        @staticmethod
        def backward(ctx, gy):
            x, h, pre, post, skip, history, pre_history = ctx.saved_tensors
            need_x, need_h, need_pre, need_post, need_skip, need_hist, need_phist = ctx.needs_input_grad
            dx = dh = dpre = dpost = dskip = dhist = dphist = None
            if need_x or need_pre:
                # no future: what later chunks add arrives through their histories
                dx, dpre = gated_chunked_causal_conv_input_grad(gy, h, x=None if pre is None else x, pre=pre, post=post, skip=skip,
                                                                want_dpre=need_pre)
            if need_h or need_skip:
                dh, dskip = gated_chunked_causal_conv_tap_grad(x, gy, h.shape[1], pre=pre, post=post, history=history, pre_history=pre_history)
                dh = dh.to(h.dtype) if need_h else None
                dskip = dskip.to(skip.dtype) if need_skip else None
            if need_post:
                # d loss / d post = gy * z: the forward plan with gy handed in as its post gate
                dpost = gated_chunked_causal_conv(x, h, pre=pre, post=gy, skip=skip, history=history, pre_history=pre_history)
            if history is not None and (need_hist or (need_phist and pre_history is not None)):
                # With du_h[u] = sum_j h'[j] gz[u + j - Hn], d loss / d history = pre_history * du_h and d loss / d pre_history =
                # history * du_h: the input gradient of a sequence of Hn samples (x = history, pre = pre_history) whose own gradient is
                # zero and whose future is the start of gy and of post (K - 1 samples reach back, carry_min rounds that up to 8)
                carry_min = gcconv_geometry(x.shape[2], h.shape[1])[4]
                if carry_min == 0:
                    dhist = torch.zeros_like(history) if need_hist else None
                    dphist = torch.zeros_like(pre_history) if need_phist and pre_history is not None else None
                else:
                    n = min(gy.shape[2], carry_min)
                    dhist, dphist = gated_chunked_causal_conv_input_grad(
                        torch.zeros_like(history), h, x=None if pre_history is None else history, pre=pre_history,
                        post=None if post is None else torch.ones_like(history), skip=skip, future=gy[..., :n],
                        post_future=None if post is None else post[..., :n], want_dpre=need_phist)
            return ((dx if need_x else None), dh, dpre, dpost, dskip, (dhist if need_hist else None),
                    (dphist if need_phist and pre_history is not None else None))

    _function = GatedChunkedCausalConv
    return _function


def differentiable_gated_chunked_causal_conv(x, h, pre=None, post=None, skip=None, history=None, pre_history=None):
    """gated_chunked_causal_conv(...) with a grad_fn: the backward pass runs each piece only when an input needs it: dx and dpre in one
    launch (no future), dh and dskip in one tap gradient (cast to h.dtype and skip.dtype), dpost through the forward plan with gy as
    its post gate, and the gradients of `history` and `pre_history` in one input gradient at length Hn, which autograd adds to the
    previous chunk's dx and dpre when the histories are views of its x and pre (next_history). Histories longer than halo are cut to
    their last halo samples first."""
    if history is not None:
        halo = gcconv_geometry(x.shape[2], h.shape[1])[0]
        if halo == 0:
            history = pre_history = None
        elif history.shape[-1] > halo:
            history = history[..., history.shape[-1] - halo:]
            if pre_history is not None:
                pre_history = pre_history[..., pre_history.shape[-1] - halo:]
    if pre is None or history is None:
        pre_history = None
    return _autograd_function().apply(x, h, pre, post, skip, history, pre_history)
