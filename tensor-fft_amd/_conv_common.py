"""What the convolution bindings do the same way on top of _binding.py: the plan of rows x channels real sequences with its taps,
spectrum and sequence checks, the hand-over of taps to a cached plan by identity, the two argument checks of the tensor functions, and
the views a carried plan reads in place. Private: the public names stay in the nine modules. No fallback of any kind."""
import ctypes

from ._binding import TfftError, _Handle, _is_cuda, _is_cuda_half

PRE_GATE, POST_GATE, COMPOSED = 1, 2, 4       # the flags of every gated add-on's option struct (COMPOSED: tfft_gconv_opts alone)


def _flags(pre_gate, post_gate, composed=False):
    return (PRE_GATE if pre_gate else 0) | (POST_GATE if post_gate else 0) | (COMPOSED if composed else 0)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _flat(t):
    """a contiguous tensor (None stays None), flat"""
    return None if t is None else t.contiguous().view(-1)


class _SeqPlan(_Handle):
    """A plan over rows x channels real fp16 sequences of `length` samples with `taps` taps per channel and a spectrum of n bins.
    A subclass sets _prefix (and _plan) as _Handle wants them; _gated where set_taps takes skip weights as well, in which case a
    tensor an execution can do without may be None in every check; _names_short where the refusal of a short tensor names its kind
    (the carried plans, which take contexts of another length beside the sequences)."""
    _gated = False
    _names_short = False

    def _create(self, L, create, rows, channels, length, taps, device, opts):
        """create(rows, channels, length, taps, device, &opts, &handle)"""
        self._open(L, create, int(rows), int(channels), int(length), int(taps), int(device), ctypes.byref(opts))
        self.rows, self.channels, self.length, self.taps = int(rows), int(channels), int(length), int(taps)
        self.device = int(device)

    def _check_taps(self, h, skip=None):
        for t, count, what in ((h, self.channels * self.taps, "taps"), (skip, self.channels, "skip")):
            if t is None and what == "skip":
                continue
            if not (_is_cuda_half(t) and t.is_contiguous() and t.device.index == self.device):
                raise TfftError(5, f"{what} must be a contiguous CUDA float16 tensor on the plan's device")
            if t.numel() < count:
                raise TfftError(5, f"the {what} tensor is shorter than channels{' * taps' if what == 'taps' else ''}")

    def _set_taps(self, h, skip, stream):
        import torch

        self._check_taps(h, skip)
        with torch.cuda.device(self.device):
            if self._gated:
                self._check(self._fn("set_taps")(self._h, h.data_ptr(), _ptr(skip), self._stream(stream)))
            else:
                self._check(self._fn("set_taps")(self._h, h.data_ptr(), self._stream(stream)))

    def spectrum(self):
        """<prefix><plan>spectrum: (h_re, h_im), the spectrum the plan built from its taps (and skip weights) as two CUDA float16
        tensors [channels, n], not conjugated: what a TfftConvPlan takes as its filter."""
        import torch

        h_re = torch.empty((self.channels, self.n), dtype=torch.float16, device=f"cuda:{self.device}")
        h_im = torch.empty_like(h_re)
        with torch.cuda.device(self.device):
            self._check(self._fn("spectrum")(self._h, h_re.data_ptr(), h_im.data_ptr()))
        return h_re, h_im

    def _check_room(self, t, stride, length, what):
        if t.numel() < (self.rows * self.channels - 1) * stride + length:
            short = "a tensor is shorter than (rows * channels - 1) * stride + length"
            raise TfftError(5, f"{what}: {short}" if self._names_short else short)

    def _check_seqs(self, t, stride, length=None, what=None):
        """`t` holds rows * channels sequences of `length` samples (the plan's own unless given) `stride` apart; `what`: the kind
        of tensor the refusal names, where it is not the plan's sequences"""
        if t is None and self._gated:
            return
        what = what or ("sequences and gates" if self._gated else "sequences")
        self._check_kind(t, what)
        self._check_room(t, stride, self.length if length is None else length, what)

    def _check_grad(self, t, count, what):
        """`t` is the float32 gradient of the taps ("tap") or of the skip weights ("skip"): `count` elements"""
        import torch

        if not (_is_cuda(t, torch.float32) and t.is_contiguous() and t.device.index == self.device and t.numel() >= count):
            raise TfftError(5, f"the {what} gradient must be a contiguous CUDA float32 tensor of channels"
                               f"{' * taps' if what == 'tap' else ''} elements on the plan's device")


class _Taps:
    def set_taps(self, h, stream=None):
        """Hands the taps over (<prefix><plan>set_taps): [channels][taps] float16; the tensor is not referenced afterwards."""
        self._set_taps(h, None, stream)


class _GatedTaps:
    _gated = True

    def set_taps(self, h, skip=None, stream=None):
        """Hands the taps [channels][taps] and the skip weights [channels] (or None) over (<prefix><plan>set_taps): float16; the
        tensors are not referenced afterwards."""
        self._set_taps(h, skip, stream)


def _hand_taps(entry, h, skip=None):
    """set_taps on the plan of a cache entry unless it holds these tensors already by (data_ptr, _version) of h and, on a gated
    plan, of skip. A non-contiguous tensor is copied per call, and a copy's address and version say nothing about its content."""
    plan = entry[0]
    ident = None
    if h.is_contiguous() and (skip is None or skip.is_contiguous()):
        ident = (h.data_ptr(), h._version)
        if plan._gated:
            ident += (None if skip is None else (skip.data_ptr(), skip._version),)
    if ident is None or entry[1] != ident:
        if plan._gated:
            plan.set_taps(h.contiguous().view(-1), None if skip is None else skip.contiguous())
        else:
            plan.set_taps(h.contiguous().view(-1))
        entry[1] = ident


def _seqs_ok(seqs, optional):
    """`seqs`: CUDA float16 tensors of one shape (B, C, L) on one device; `optional`: more of them, or None"""
    seq = seqs[0]

    def same(t):
        return _is_cuda_half(t) and t.shape == seq.shape and t.device == seq.device

    return _is_cuda_half(seq) and seq.dim() == 3 and all(same(t) for t in seqs[1:]) and all(t is None or same(t) for t in optional)


def _check_seq_args(message, seqs, optional=()):
    """The arguments of a tensor function that takes no taps (a tap gradient), refused with `message` as one."""
    if not _seqs_ok(seqs, optional):
        raise TfftError(5, message)


def _check_tap_args(message, seqs, optional, h, skip=None):
    """The arguments of a tensor function that takes taps, refused with `message` as one: the sequences as above, h (C, K), and
    skip (C,) or None, on the device of the sequences."""
    seq = seqs[0]
    ok = _seqs_ok(seqs, optional) and _is_cuda_half(h) and h.dim() == 2 and h.shape[0] == seq.shape[1] and h.device == seq.device
    ok = ok and (skip is None or (_is_cuda_half(skip) and skip.shape == (seq.shape[1],) and skip.device == seq.device))
    if not ok:
        raise TfftError(5, message)


# ---- the views a carried plan reads in place (cconv.py says when a view qualifies)
def _strided(t):
    """(tensor, sequence stride): `t` itself where the plan can read it in place, a contiguous copy otherwise; (None, 0) for None"""
    if t is None:
        return None, 0
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
    if ctx is None or halo == 0 or ctx.shape[-1] == 0:
        return None, 0, 0
    if not (_is_cuda_half(ctx) and ctx.dim() == 3 and ctx.shape[:2] == like.shape[:2] and ctx.device == like.device):
        raise TfftError(5, f"{what} must be a CUDA float16 tensor (B, C, n) on the device of the sequences")
    if ctx.shape[2] % 8:
        raise TfftError(5, f"{what} must hold a multiple of 8 samples per sequence")
    if ctx.shape[2] > halo:
        ctx = ctx[..., -halo:] if what == "history" else ctx[..., :halo]
    ctx, stride = _strided(ctx)
    return ctx, ctx.shape[2], stride


def _flat_view(t):
    """the flat tensor from the first element of a qualifying view to the end of its storage: what the plans' exec methods check;
    None stays None"""
    return None if t is None else t.as_strided((t.untyped_storage().nbytes() // 2 - t.storage_offset(),), (1,))
