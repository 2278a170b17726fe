"""ctypes binding of include/tfft_gbconv.h (libtfft_gbconv.so, the gradients of the gated overlap-save causal convolution), and the
torch.autograd hook over it and the forward plan of gsconv. No fallback of any kind: torch supplies memory, streams and the autograd
graph, nothing else. What the convolution bindings share lives in _conv_common.py."""
import ctypes
import os

from . import _binding
from . import _conv_common as common
from . import conv, gsconv
from ._conv_common import _flags, _flat, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_gbconv.so"
_PREFIX = "tfft_gbconv_"

# every symbol include/tfft_gbconv.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_gbconv_geometry", "tfft_gbconv_plan_create", "tfft_gbconv_plan_destroy", "tfft_gbconv_plan_set_taps", "tfft_gbconv_plan_spectrum",
    "tfft_gbconv_plan_workspace_bytes", "tfft_gbconv_plan_set_workspace", "tfft_gbconv_plan_prepare", "tfft_gbconv_exec_input_grad",
    "tfft_gbconv_exec_tap_grad", "tfft_gbconv_plan_num_launches", "tfft_gbconv_plan_kernels", "tfft_gbconv_describe", "tfft_gbconv_last_error",
]
GBCONV_PRE_GATE, GBCONV_POST_GATE = 1, 2                      # tfft_gbconv_opts.flags
GBCONV_MAX_TAPS = 2049                                        # TFFT_GBCONV_MAX_TAPS
GBCONV_N = 4096                                               # the transform length of every plan


class GbconvOpts(ctypes.Structure):
    """tfft_gbconv_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("x_seq_stride", ctypes.c_uint64),
                ("pre_seq_stride", ctypes.c_uint64), ("gy_seq_stride", ctypes.c_uint64), ("post_seq_stride", ctypes.c_uint64),
                ("dx_seq_stride", ctypes.c_uint64), ("dpre_seq_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32),
                ("partials", ctypes.c_uint32), ("flags", ctypes.c_int)]


def gbconv_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


def _prototypes():
    vp, u64, u32, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t
    pu64 = ctypes.POINTER(u64)
    return {
        "tfft_gbconv_geometry": (ci, [u64, u64, u64, u64, u32, pu64, pu64, pu64, pu64]),
        "tfft_gbconv_plan_create": (ci, [u64, u64, u64, u64, ci, ctypes.POINTER(GbconvOpts), ctypes.POINTER(vp)]),
        "tfft_gbconv_plan_destroy": (None, [vp]),
        "tfft_gbconv_plan_set_taps": (ci, [vp, vp, vp, vp]),
        "tfft_gbconv_plan_spectrum": (ci, [vp, vp, vp]),
        "tfft_gbconv_plan_workspace_bytes": (sz, [vp]),
        "tfft_gbconv_plan_set_workspace": (ci, [vp, vp, sz]),
        "tfft_gbconv_plan_prepare": (ci, [vp]),
        "tfft_gbconv_exec_input_grad": (ci, [vp, vp, vp, vp, vp, vp, vp, vp]),
        "tfft_gbconv_exec_tap_grad": (ci, [vp, vp, vp, vp, vp, vp, vp, vp]),
        "tfft_gbconv_plan_num_launches": (ci, [vp]),
        "tfft_gbconv_plan_kernels": (ci, [vp, ctypes.c_char_p, sz]),
        "tfft_gbconv_describe": (ci, [u64, u64, u64, u64, u32, ci, ctypes.c_char_p, sz]),
        "tfft_gbconv_last_error": (ctypes.c_char_p, []),
    }


_lib = None


def load_gbconv_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_gbconv.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is None:
        _lib = _binding._load(conv.load_conv_library, gbconv_lib_path(), "gated convolution gradient", _prototypes())
    return _lib


def gbconv_geometry(length, taps, rows=1, channels=1, partials=0):
    """tfft_gbconv_geometry: (halo, hop, segments, P): the geometry of sconv_geometry and the partial sums per channel of the tap
    gradient under the cap `partials` (0 = none). Host only."""
    L = load_gbconv_library()
    out = [ctypes.c_uint64() for _ in range(4)]
    _binding._check(L, _PREFIX, L.tfft_gbconv_geometry(int(length), int(taps), int(rows), int(channels), int(partials), *[ctypes.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def gbconv_describe(length, taps, rows=1, channels=1, partials=0, pre_gate=False, post_gate=False):
    """tfft_gbconv_describe: "gbconv4096:4096[:pre][+post] x S | partials P". Host only, no GPU needed."""
    L = load_gbconv_library()
    buf = ctypes.create_string_buffer(128)
    _binding._check(L, _PREFIX, L.tfft_gbconv_describe(int(length), int(taps), int(rows), int(channels), int(partials), _flags(pre_gate, post_gate),
                                                     buf, len(buf)))
    return buf.value.decode()


class TfftGatedLongConvGradPlan(common._GatedTaps, _binding._Workspace, common._SeqPlan):
    """Owning wrapper of tfft_gbconv_plan: the gradients of TfftGatedLongConvPlan for rows x channels real fp16 sequences of `length`
    samples, `taps` <= 2049 taps and one skip weight per channel (include/tfft_gbconv.h). Which gates the forward operator has is
    fixed at creation. input_grad(gy, dx, ...) needs set_taps(h, skip) first and writes dx and, where asked, dpre; tap_grad(x, gy,
    dh, ...) writes [channels][taps] float32 and, where asked, dskip [channels] float32, and needs no taps. `partials` caps the
    partial sums per channel (0 = the library's default); the tap gradient depends on it through the order of fp32 additions only.
    The gradient of the post gate is TfftGatedLongConvPlan.exec with gy as its post gate. The workspace is the tap gradient's;
    `kernels` lists the input gradient's kernel, then the tap gradient's two."""
    _prefix = _PREFIX

    def __init__(self, rows, channels, length, taps, device=0, pre_gate=False, post_gate=False, x_seq_stride=0, pre_seq_stride=0,
                 gy_seq_stride=0, post_seq_stride=0, dx_seq_stride=0, dpre_seq_stride=0, launch_iters=0, partials=0):
        L = load_gbconv_library()
        opts = GbconvOpts(ctypes.sizeof(GbconvOpts), 0, int(x_seq_stride), int(pre_seq_stride), int(gy_seq_stride), int(post_seq_stride),
                          int(dx_seq_stride), int(dpre_seq_stride), int(launch_iters), int(partials), _flags(pre_gate, post_gate))
        self._create(L, L.tfft_gbconv_plan_create, rows, channels, length, taps, device, opts)
        self.pre_gate, self.post_gate = bool(pre_gate), bool(post_gate)
        self.n = GBCONV_N
        self.halo, self.hop, self.segments, self.partials = gbconv_geometry(length, taps, rows, channels, partials)
        self.x_seq_stride = int(x_seq_stride) or self.length
        self.pre_seq_stride = int(pre_seq_stride) or self.length
        self.gy_seq_stride = int(gy_seq_stride) or self.length
        self.post_seq_stride = int(post_seq_stride) or self.length
        self.dx_seq_stride = int(dx_seq_stride) or self.length
        self.dpre_seq_stride = int(dpre_seq_stride) or self.length

    def input_grad_ptr(self, gy, dx, post=None, x=None, pre=None, dpre=None, stream=0):
        self._check(self._lib.tfft_gbconv_exec_input_grad(self._h, gy, post, x, pre, dx, dpre, stream))

    def tap_grad_ptr(self, x, gy, dh, pre=None, post=None, dskip=None, stream=0):
        self._check(self._lib.tfft_gbconv_exec_tap_grad(self._h, x, pre, gy, post, dh, dskip, stream))

    def input_grad(self, gy, dx, post=None, x=None, pre=None, dpre=None, stream=None):
        """gy, dx, post, x, pre, dpre: flat CUDA float16 tensors, sequence (b, c) at (b * channels + c) * the tensor's seq stride; dx
        and dpre share no element with the others or each other. The library refuses a gate the plan does not have and misses one
        it has; dpre=None on a plan with a pre gate writes dx only."""
        import torch

        for t, stride in ((gy, self.gy_seq_stride), (dx, self.dx_seq_stride), (post, self.post_seq_stride), (x, self.x_seq_stride),
                          (pre, self.pre_seq_stride), (dpre, self.dpre_seq_stride)):
            self._check_seqs(t, stride)
        with torch.cuda.device(self.device):
            self.input_grad_ptr(gy.data_ptr(), dx.data_ptr(), _ptr(post), _ptr(x), _ptr(pre), _ptr(dpre), self._stream(stream))

    def tap_grad(self, x, gy, dh, pre=None, post=None, dskip=None, stream=None):
        """x, gy, pre, post: flat CUDA float16 tensors (they may be the same); dh: a contiguous CUDA float32 tensor of channels * taps
        elements; dskip: one of channels elements, or None."""
        import torch

        for t, stride in ((x, self.x_seq_stride), (gy, self.gy_seq_stride), (pre, self.pre_seq_stride), (post, self.post_seq_stride)):
            self._check_seqs(t, stride)
        self._check_grad(dh, self.channels * self.taps, "tap")
        if dskip is not None:
            self._check_grad(dskip, self.channels, "skip")
        with torch.cuda.device(self.device):
            self.tap_grad_ptr(x.data_ptr(), gy.data_ptr(), dh.data_ptr(), _ptr(pre), _ptr(post), _ptr(dskip), self._stream(stream))


# The convenience functions keep the plans of the last GBCONV_CACHE_SIZE (rows, channels, length, taps, device, pre gate, post gate)
# keys, least recently used first out, as bconv._plan_for does: one cache per gradient (a caller who needs only one gradient creates
# no plan for the other, and the tap gradient's plans hold a workspace), the input gradient's with the identity of the taps and skip
# each plan holds. gbconv_cache_clear() releases both.
GBCONV_CACHE_SIZE = 8
_dx_plans = {}
_dh_plans = {}


def _plan_for(cache, rows, channels, length, taps, device, pre_gate, post_gate):
    key = (int(rows), int(channels), int(length), int(taps), int(device), bool(pre_gate), bool(post_gate))
    return _binding._cached(cache, GBCONV_CACHE_SIZE, key,
                          lambda: TfftGatedLongConvGradPlan(rows, channels, length, taps, device, pre_gate=pre_gate, post_gate=post_gate))


def gbconv_cache_clear():
    """Destroys the plans gated_long_causal_conv_input_grad and gated_long_causal_conv_tap_grad cached."""
    _binding._cache_clear(_dx_plans, _dh_plans)


def gated_long_causal_conv_input_grad(gy, h, x=None, pre=None, post=None, skip=None, want_dpre=True):
    """(dx, dpre) of gated_long_causal_conv(x, h, pre, post, skip) for gy = d loss / d y: dx = pre * du and dpre = x * du with
    du[b, c, t] = sum_j h'[c, j] (post * gy)[b, c, t + j], in one launch. gy, x, pre, post: CUDA float16 tensors [B, C, L]; h [C, K]
    with K <= 2049; skip [C] or None. x is needed exactly when pre is given. dpre is None without a pre gate or when want_dpre is
    false. Taps and skip are handed to the cached plan again only when (data_ptr, _version) of h or skip changed since the last call."""
    import torch

    common._check_tap_args("gated_long_causal_conv_input_grad takes CUDA float16 tensors gy, x, pre, post (B, C, L), h (C, K) and skip (C,) on one device",
                           (gy,), (x, pre, post), h, skip)
    if (pre is None) != (x is None):
        raise _binding.TfftError(5, "gated_long_causal_conv_input_grad takes x exactly when it takes pre")
    rows, channels, length = gy.shape
    entry = _plan_for(_dx_plans, rows, channels, length, h.shape[1], gy.device.index, pre is not None, post is not None)
    common._hand_taps(entry, h, skip)
    gy = gy.contiguous()
    dx = torch.empty_like(gy)
    dpre = torch.empty_like(gy) if pre is not None and want_dpre else None
    entry[0].input_grad(gy.view(-1), dx.view(-1), post=_flat(post), x=_flat(x), pre=_flat(pre), dpre=None if dpre is None else dpre.view(-1))
    return dx, dpre


def gated_long_causal_conv_tap_grad(x, gy, taps, pre=None, post=None):
    """(dh, dskip) of gated_long_causal_conv: dh[c, j] = sum_{b, t} (post * gy)[b, c, t] (pre * x)[b, c, t - j], j < taps, float32
    [C, taps], and dskip = dh[:, 0] as a tensor of its own [C]. x, gy, pre, post: CUDA float16 tensors [B, C, L]."""
    import torch

    common._check_seq_args("gated_long_causal_conv_tap_grad takes CUDA float16 tensors x, gy, pre and post of one shape (B, C, L) on one device",
                           (x, gy), (pre, post))
    rows, channels, length = x.shape
    plan = _plan_for(_dh_plans, rows, channels, length, taps, x.device.index, pre is not None, post is not None)[0]
    dh = torch.empty((channels, int(taps)), dtype=torch.float32, device=x.device)
    dskip = torch.empty((channels,), dtype=torch.float32, device=x.device)
    plan.tap_grad(_flat(x), _flat(gy), dh, pre=_flat(pre), post=_flat(post), dskip=dskip)
    return dh, dskip


_function = None


def _autograd_function():
    """the torch.autograd.Function, built on first use so that importing the package does not import torch"""
    global _function
    if _function is not None:
        return _function
    import torch

    class GatedLongCausalConv(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, h, pre, post, skip):
            ctx.save_for_backward(x, h, pre, post, skip)
            return gsconv.gated_long_causal_conv(x, h, pre=pre, post=post, skip=skip)

        @staticmethod
        def backward(ctx, gy):
            x, h, pre, post, skip = ctx.saved_tensors
            need_x, need_h, need_pre, need_post, need_skip = ctx.needs_input_grad
            dx = dh = dpre = dpost = dskip = None
            if need_x or need_pre:
                dx, dpre = gated_long_causal_conv_input_grad(gy, h, x=None if pre is None else x, pre=pre, post=post, skip=skip, want_dpre=need_pre)
            if need_h or need_skip:
                dh, dskip = gated_long_causal_conv_tap_grad(x, gy, h.shape[1], pre=pre, post=post)
                dh = dh.to(h.dtype) if need_h else None
                dskip = dskip.to(skip.dtype) if need_skip else None
            if need_post:
                # d loss / d post = gy * z: the forward plan with gy handed in as its post gate
                dpost = gsconv.gated_long_causal_conv(x, h, pre=pre, post=gy, skip=skip)
            return (dx if need_x else None), dh, dpre, dpost, dskip

    _function = GatedLongCausalConv
    return _function


def differentiable_gated_long_causal_conv(x, h, pre=None, post=None, skip=None):
    """gated_long_causal_conv(x, h, pre, post, skip) with a grad_fn: the forward pass is TfftGatedLongConvPlan, bit for bit; the
    backward pass runs each piece only when an input needs it: dx and dpre in one launch of the gated gradient plan, dh and dskip in
    one tap gradient (cast to h.dtype and skip.dtype), dpost through the forward plan with gy as its post gate."""
    return _autograd_function().apply(x, h, pre, post, skip)
