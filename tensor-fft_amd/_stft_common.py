"""What the STFT bindings (stft, istft, stftn, istftn, and spec on top of them) do the same way: the ctypes prototypes of a library,
the owning plan wrapper with its tensor checks, the hand-over of a window to a cached plan by identity, and the tensor functions on top. What is
not about windows and frames (loading, the return-code check, the handle's life cycle, the workspace calls, the cache) is
_binding.py's. Private: the public names stay in the modules. No fallback of any kind."""
import ctypes

from . import conv
from ._binding import TfftError, _cache_clear, _cached, _check, _Handle, _is_cuda_half, _Workspace  # noqa: F401
from ._binding import _load as _load_addon


def _u32(n):
    """the frame length as the C ABI takes it; a value that does not fit 32 bits is as unsupported as any other"""
    n = int(n)
    return n if 0 <= n < 1 << 32 else 0


def _bins(n):
    return int(n) // 2 + 1


def _pitch(n):
    return (_bins(n) + 7) // 8 * 8


def _load(path, what, prefix, opts, takes_n, inverse, own=None):
    """Loads libtfft.so and libtfft_conv.so, then the add-on at `path` ("the `what` add-on"), and sets the prototypes of its calls
    <prefix>*: with the frame length in front where the library `takes_n`, with the workspace calls where it is an `inverse`, and
    with `own`, {name: (restype, argtypes)}, for the calls a library has beyond these or with other arguments."""
    vp, u64, ci, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
    n = [ctypes.c_uint32] if takes_n else []
    protos = {
        "geometry": (ci, n + [u64, u64, u64, ctypes.POINTER(u64)]),
        "plan_create": (ci, n + [u64, u64, u64, u64, ci, ctypes.POINTER(opts), ctypes.POINTER(vp)]),
        "plan_destroy": (None, [vp]),
        "plan_set_window": (ci, [vp, vp, vp]),
        "exec": (ci, [vp, vp, vp, vp, vp]),
        "plan_num_launches": (ci, [vp]),
        "plan_kernels": (ci, [vp, ctypes.c_char_p, sz]),
        "describe": (ci, n + [u64, u64, u64, u64, ci, ctypes.c_char_p, sz]),
        "last_error": (ctypes.c_char_p, []),
    }
    if inverse:
        protos.update({"plan_workspace_bytes": (sz, [vp]), "plan_set_workspace": (ci, [vp, vp, sz]), "plan_prepare": (ci, [vp])})
    protos.update(own or {})
    return _load_addon(conv.load_conv_library, path, what, {prefix + name: proto for name, proto in protos.items()})


def _geometry(L, prefix, n, length, hop, pad):
    """<prefix>geometry; n None for a library of one frame length"""
    frames = ctypes.c_uint64()
    front = [] if n is None else [_u32(n)]
    _check(L, prefix, getattr(L, prefix + "geometry")(*front, int(length), int(hop), int(pad), ctypes.byref(frames)))
    return int(frames.value)


def _describe(L, prefix, n, length, hop, pad, rows, flags):
    buf = ctypes.create_string_buffer(128)
    front = [] if n is None else [_u32(n)]
    _check(L, prefix, getattr(L, prefix + "describe")(*front, int(length), int(hop), int(pad), int(rows), flags, buf, len(buf)))
    return buf.value.decode()


class _Plan(_Handle):
    """What the four plan wrappers share. A subclass sets _prefix ("tfft_stftn_") and _takes_n, and its __init__ calls _create."""

    def _create(self, L, opts, n, rows, length, hop, pad, device):
        front = [_u32(n)] if self._takes_n else []
        self._open(L, getattr(L, self._prefix + "plan_create"), *front, int(rows), int(length), int(hop), int(pad), int(device), ctypes.byref(opts))
        self.n, self.rows, self.length, self.hop, self.pad = int(n), int(rows), int(length), int(hop), int(pad)
        self.device = int(device)
        self.bins, self.pitch = _bins(n), _pitch(n)
        self.frames = _geometry(L, self._prefix, n if self._takes_n else None, length, hop, pad)

    def _call(self, name, *args):
        self._check(getattr(self._lib, self._prefix + name)(*args))

    def set_window(self, w, stream=None):
        """Hands the window over (<prefix>plan_set_window): n halves, copied on the stream; the tensor is not referenced by the plan
        afterwards."""
        import torch

        if not (_is_cuda_half(w) and w.is_contiguous() and w.device.index == self.device):
            raise TfftError(5, "the window must be a contiguous CUDA float16 tensor on the plan's device")
        if w.numel() != self.n:
            raise TfftError(5, f"the window must hold {self.n} halves")
        with torch.cuda.device(self.device):
            self._call("plan_set_window", self._h, w.data_ptr(), self._stream(stream))

    def _exec(self, tensors, needs, stream):
        """`tensors`: the three buffers in the order of the call; `needs`: (tensor, halves, message when it holds fewer), in the order
        in which they are refused"""
        import torch

        for t in tensors:
            self._check_kind(t, "buffers")
        for t, need, message in needs:
            if t.numel() < need:
                raise TfftError(5, message)
        with torch.cuda.device(self.device):
            self.exec_ptr(*(t.data_ptr() for t in tensors), self._stream(stream))


class _ForwardPlan(_Plan):
    def _create(self, L, opts, n, rows, length, hop, pad, device):
        super()._create(L, opts, n, rows, length, hop, pad, device)
        self.in_sig_stride = int(opts.in_sig_stride) or self.length
        self.out_frame_stride = int(opts.out_frame_stride) or 2 * self.pitch

    def exec_ptr(self, src, out_re, out_im, stream=0):
        self._call("exec", self._h, src, out_re, out_im, stream)

    def exec(self, x, out_re, out_im, stream=None):
        """x: flat CUDA float16 tensor, signal r at r * in_sig_stride; out_re / out_im: flat planes, frame g at g * out_frame_stride,
        n / 2 + 1 bins each (out_im may be a view of out_re's buffer, `pitch` halves on: the [RE | IM] blocks of TfftRealPlan)."""
        plane = (self.rows * self.frames - 1) * self.out_frame_stride + self.bins
        short = f"an output plane is shorter than (rows * frames - 1) * out_frame_stride + {self.bins}"
        self._exec((x, out_re, out_im), [
            (x, (self.rows - 1) * self.in_sig_stride + self.length, "the signal buffer is shorter than (rows - 1) * in_sig_stride + length"),
            (out_re, plane, short), (out_im, plane, short)], stream)


class _InversePlan(_Workspace, _Plan):
    def _create(self, L, opts, n, rows, length, hop, pad, device):
        super()._create(L, opts, n, rows, length, hop, pad, device)
        self.in_frame_stride = int(opts.in_frame_stride) or 2 * self.pitch
        self.out_sig_stride = int(opts.out_sig_stride) or self.length

    def workspace_bytes(self):
        """the bytes of the time-domain frames (a method here, a property on the convolution plans: both are public)"""
        return self._workspace_bytes()

    def set_workspace(self, tensor):
        """Hands a torch CUDA tensor in as the workspace of the time-domain frames (kept alive by the plan); None returns to a
        workspace of the plan's own."""
        if tensor is None:
            self._call("plan_set_workspace", self._h, None, 0)
            self._ws = None
        else:
            super().set_workspace(tensor)

    def exec_ptr(self, in_re, in_im, out, stream=0):
        self._call("exec", self._h, in_re, in_im, out, stream)

    def exec(self, in_re, in_im, out, stream=None):
        """in_re / in_im: flat CUDA float16 planes, frame g at g * in_frame_stride, n / 2 + 1 bins each (in_im may be a view of in_re's
        buffer, `pitch` halves on: the [RE | IM] blocks a forward plan writes); out: flat, signal r at r * out_sig_stride."""
        plane = (self.rows * self.frames - 1) * self.in_frame_stride + self.bins
        short = f"an input plane is shorter than (rows * frames - 1) * in_frame_stride + {self.bins}"
        self._exec((in_re, in_im, out), [
            (in_re, plane, short), (in_im, plane, short),
            (out, (self.rows - 1) * self.out_sig_stride + self.length, "the output buffer is shorter than (rows - 1) * out_sig_stride + length")], stream)


# ---- the tensor functions, over _binding._cached: each entry [plan, identity of the window it holds]
def _hand_window(entry, window):
    """Hands `window` (1 .. n values, checked by the caller) to the plan of a cache entry unless the entry holds it already by
    (data_ptr, _version, numel). A shorter window is zero-padded to n with the window centred, as torch.stft does."""
    import torch

    plan = entry[0]
    # (a non-contiguous window is copied per call, and a copy's address and version say nothing about its content)
    ident = (window.data_ptr(), window._version, window.numel()) if window.is_contiguous() else None
    if ident is None or entry[1] != ident:
        w = window.contiguous()
        if w.numel() < plan.n:
            left = (plan.n - w.numel()) // 2
            w = torch.nn.functional.pad(w, (left, plan.n - w.numel() - left))
        plan.set_window(w)
        entry[1] = ident


def _check_forward(name, x, window, n):
    if not (_is_cuda_half(x) and _is_cuda_half(window) and x.dim() == 2 and window.dim() == 1 and window.device == x.device):
        raise TfftError(5, f"{name} takes CUDA float16 tensors x (R, L) and window (win_length) on one device")
    if window.numel() == 0 or window.numel() > n:
        raise TfftError(5, f"the window must hold 1 .. {n} values")


def _forward(entry, x, window):
    """(re, im), each an [R, F, bins] view of one new [R, F, 2, pitch] buffer"""
    import torch

    plan = entry[0]
    _hand_window(entry, window)
    x = x.contiguous()
    buf = torch.empty((plan.rows, plan.frames, 2, plan.pitch), dtype=torch.float16, device=x.device)
    flat = buf.view(-1)
    plan.exec(x.view(-1), flat, flat[plan.pitch:])
    return buf[:, :, 0, :plan.bins], buf[:, :, 1, :plan.bins]


def _check_inverse(name, re, im, window, n):
    if not (_is_cuda_half(re) and _is_cuda_half(im) and _is_cuda_half(window) and re.dim() == 3 and re.shape == im.shape
            and re.shape[2] == _bins(n) and window.dim() == 1 and window.device == re.device == im.device):
        raise TfftError(5, f"{name} takes CUDA float16 tensors re, im (R, F, {_bins(n)}) and window (win_length) on one device")
    if window.numel() == 0 or window.numel() > n:
        raise TfftError(5, f"the window must hold 1 .. {n} values")


def _inverse(entry, re, im, window, length):
    """a new [R, length] tensor; re, im are taken as they are in the layout _forward returns, and copied into it otherwise"""
    import torch

    plan = entry[0]
    rows, frames = int(re.shape[0]), int(re.shape[1])
    if plan.frames != frames:
        raise TfftError(5, f"{frames} frames per signal, but length {int(length)} with this hop and padding has {plan.frames}")
    _hand_window(entry, window)
    stride = 2 * plan.pitch
    want = (frames * stride, stride, 1)
    if not (re.stride() == want and im.stride() == want and re.data_ptr() % 16 == 0 and im.data_ptr() % 16 == 0):
        buf = torch.empty((rows, frames, 2, plan.pitch), dtype=torch.float16, device=re.device)
        buf[:, :, 0, :plan.bins] = re
        buf[:, :, 1, :plan.bins] = im
        re, im = buf[:, :, 0, :plan.bins], buf[:, :, 1, :plan.bins]
    out = torch.empty((rows, plan.length), dtype=torch.float16, device=re.device)
    with torch.cuda.device(plan.device):
        plan.exec_ptr(re.data_ptr(), im.data_ptr(), out.data_ptr(), plan._stream(None))
    return out
