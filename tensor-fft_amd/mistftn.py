"""ctypes binding of include/tfft_mistftn.h (libtfft_mistftn.so, the masked short-frame inverse STFT add-on: the plans of istftn.py
with a real binary16 mask inside the merge; frame lengths 512, 1024 and 2048). No fallback of any kind. What the STFT bindings share
lives in _stft_common.py."""
import ctypes
import os

from . import _stft_common as common
from ._binding import _is_cuda_half
from .capi import TfftError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtfft_mistftn.so"
_PREFIX = "tfft_mistftn_"

# every symbol include/tfft_mistftn.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "tfft_mistftn_geometry", "tfft_mistftn_plan_create", "tfft_mistftn_plan_destroy", "tfft_mistftn_plan_set_window",
    "tfft_mistftn_plan_workspace_bytes", "tfft_mistftn_plan_set_workspace", "tfft_mistftn_plan_prepare", "tfft_mistftn_exec",
    "tfft_mistftn_plan_num_launches", "tfft_mistftn_plan_kernels", "tfft_mistftn_describe", "tfft_mistftn_last_error",
]
MISTFTN_LENGTHS = (512, 1024, 2048)                           # the frame lengths of a plan
MISTFTN_RAW_SUM = 1                                           # TFFT_MISTFTN_RAW_SUM: no division by the window envelope
MISTFTN_MASK_PER_BIN = 2                                      # TFFT_MISTFTN_MASK_PER_BIN: one mask of n / 2 + 1 halves for every frame


class MaskedIstftNOpts(ctypes.Structure):
    """tfft_mistftn_opts"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("in_frame_stride", ctypes.c_uint64),
                ("out_sig_stride", ctypes.c_uint64), ("launch_iters", ctypes.c_uint32), ("flags", ctypes.c_int),
                ("mask_frame_stride", ctypes.c_uint64)]


def mistftn_lib_path():
    return os.path.join(_HERE, _LIB_NAME)


_lib = None


def load_mistftn_library():
    """Loads libtfft.so and libtfft_conv.so, then libtfft_mistftn.so; raises (never falls back) when one has not been built."""
    global _lib
    if _lib is None:
        vp = ctypes.c_void_p
        own = {"exec": (ctypes.c_int, [vp, vp, vp, vp, vp, vp])}         # plan, in_re, in_im, mask, out, stream
        _lib = common._load(mistftn_lib_path(), "masked short-frame ISTFT", _PREFIX, MaskedIstftNOpts, takes_n=True, inverse=True, own=own)
    return _lib


def _flags(raw_sum, per_bin):
    return (MISTFTN_RAW_SUM if raw_sum else 0) | (MISTFTN_MASK_PER_BIN if per_bin else 0)


def mistftn_geometry(n, length, hop, pad=0):
    """tfft_mistftn_geometry: F = 1 + (length + 2 pad - n) // hop, the frames per signal. Host only."""
    return common._geometry(load_mistftn_library(), _PREFIX, n, length, hop, pad)


def mistftn_describe(n, length, hop, pad=0, rows=1, raw_sum=False, per_bin=False):
    """tfft_mistftn_describe: "mistft256r<R>:n x F + ola", R = n / 256 and F the frames per signal. Host only, no GPU needed."""
    return common._describe(load_mistftn_library(), _PREFIX, n, length, hop, pad, rows, _flags(raw_sum, per_bin))


class TfftMaskedIstftPlan(common._InversePlan):
    """Owning wrapper of tfft_mistftn_plan: TfftShortIstftPlan with a real float16 mask on the half spectra, multiplied in inside the
    merge's fp32 sum in front of its single rounding (include/tfft_mistftn.h): Z' = fp16(n * fp32(mA A + i mB B)) for the frames A, B of
    a pair and their masks, then the C2R of every frame into the workspace and y = sum w v / sum w w (raw_sum: y = sum w v). The mask of
    frame g = r * frames + f lies at g * mask_frame_stride (0 = pitch; bins 0 .. n / 2 of it are read); with per_bin one mask of
    n / 2 + 1 halves serves every frame and mask_frame_stride must be 0. A mask of ones gives TfftShortIstftPlan's bits. Output and
    workspace must not overlap the inputs, the mask or each other; the mask may alias the spectra."""
    _prefix, _takes_n = _PREFIX, True

    def __init__(self, n, rows, length, hop, pad=0, device=0, in_frame_stride=0, mask_frame_stride=0, out_sig_stride=0, launch_iters=0,
                 raw_sum=False, per_bin=False):
        opts = MaskedIstftNOpts(ctypes.sizeof(MaskedIstftNOpts), 0, int(in_frame_stride), int(out_sig_stride), int(launch_iters),
                                _flags(raw_sum, per_bin), int(mask_frame_stride))
        self._create(load_mistftn_library(), opts, n, rows, length, hop, pad, device)
        self.raw_sum, self.per_bin = bool(raw_sum), bool(per_bin)
        self.mask_frame_stride = 0 if per_bin else int(mask_frame_stride) or self.pitch
        self.mask_halves = (self.rows * self.frames - 1) * self.mask_frame_stride + self.bins      # what an execution asks of the mask

    def exec_ptr(self, in_re, in_im, mask, out, stream=0):
        self._call("exec", self._h, in_re, in_im, mask, out, stream)

    def exec(self, in_re, in_im, mask, out, stream=None):
        """in_re / in_im / out as TfftShortIstftPlan.exec; mask: flat CUDA float16, the mask of frame g at g * mask_frame_stride,
        n / 2 + 1 bins (per_bin: n / 2 + 1 halves in all)."""
        import torch

        plane = (self.rows * self.frames - 1) * self.in_frame_stride + self.bins
        short = f"an input plane is shorter than (rows * frames - 1) * in_frame_stride + {self.bins}"
        for t in (in_re, in_im, mask, out):
            self._check_kind(t, "buffers")
        for t, need, message in [
                (in_re, plane, short), (in_im, plane, short),
                (mask, self.mask_halves, f"the mask is shorter than {'' if self.per_bin else '(rows * frames - 1) * mask_frame_stride + '}{self.bins}"),
                (out, (self.rows - 1) * self.out_sig_stride + self.length, "the output buffer is shorter than (rows - 1) * out_sig_stride + length")]:
            if t.numel() < need:
                raise TfftError(5, message)
        with torch.cuda.device(self.device):
            self.exec_ptr(in_re.data_ptr(), in_im.data_ptr(), mask.data_ptr(), out.data_ptr(), self._stream(stream))


# masked_istft (and the gradients of stft_autograd.py) keep the plans of the last MISTFTN_CACHE_SIZE (n, rows, length, hop, pad, raw_sum,
# per_bin, device, mask stride) shapes, least recently used first out, each with the identity of the window it holds, as istftn does.
# A plan holds device memory outside torch's allocator (tables, window, workspace): a caller with many shapes should hold
# TfftMaskedIstftPlan objects itself; mistftn_cache_clear() releases them.
MISTFTN_CACHE_SIZE = 8
_plans = {}


def _plan_for(n, rows, length, hop, pad, raw_sum, per_bin, device, mask_frame_stride=0):
    key = (int(n), int(rows), int(length), int(hop), int(pad), bool(raw_sum), bool(per_bin), int(device), int(mask_frame_stride))
    return common._cached(_plans, MISTFTN_CACHE_SIZE, key,
                          lambda: TfftMaskedIstftPlan(n, rows, length, hop, pad, device, mask_frame_stride=mask_frame_stride, raw_sum=raw_sum,
                                                      per_bin=per_bin))


def _in_place_stride(mask, n):
    """the frame stride at which a plan reads the [R, F, n / 2 + 1] mask where it lies, or None when it has to be copied"""
    s0, s1, s2 = mask.stride()
    if s2 == 1 and s1 % 8 == 0 and s1 >= common._bins(n) and s0 == mask.shape[1] * s1 and mask.data_ptr() % 16 == 0:
        return s1
    return None


def mistftn_cache_clear():
    """Destroys the plans masked_istft and the gradient functions cached."""
    common._cache_clear(_plans)


def mask_buffer(rows, frames, n_fft, device):
    """A float16 [rows, frames, n_fft / 2 + 1] view of a new, uninitialised [rows, frames, pitch] buffer (pitch = 264, 520, 1032): the
    layout a masked plan reads by default. A network that writes its mask into this view spares masked_istft its copy."""
    import torch

    n = int(n_fft)
    if n not in MISTFTN_LENGTHS:
        raise TfftError(5, "mask_buffer takes n_fft = 512, 1024 or 2048")
    buf = torch.empty((int(rows), int(frames), common._pitch(n)), dtype=torch.float16, device=device)
    return buf[:, :, :common._bins(n)]


def _run(entry, re, im, mask, window, length):
    """_stft_common._inverse with the mask: a new [R, length] tensor. The mask is a 1-D tensor of n / 2 + 1 halves for a per-bin
    plan, else [R, F, n / 2 + 1], read in place when its frame stride is a multiple of 8 (a plan of that stride) and copied once into
    an [R, F, pitch] buffer otherwise"""
    import torch

    plan = entry[0]
    rows, frames = int(re.shape[0]), int(re.shape[1])
    if plan.frames != frames:
        raise TfftError(5, f"{frames} frames per signal, but length {int(length)} with this hop and padding has {plan.frames}")
    common._hand_window(entry, window)
    stride = 2 * plan.pitch
    want = (frames * stride, stride, 1)
    if not (re.stride() == want and im.stride() == want and re.data_ptr() % 16 == 0 and im.data_ptr() % 16 == 0):
        buf = torch.empty((rows, frames, 2, plan.pitch), dtype=torch.float16, device=re.device)
        buf[:, :, 0, :plan.bins] = re
        buf[:, :, 1, :plan.bins] = im
        re, im = buf[:, :, 0, :plan.bins], buf[:, :, 1, :plan.bins]
    if plan.per_bin:
        if not (mask.is_contiguous() and mask.data_ptr() % 16 == 0):
            mask = mask.contiguous().clone()
    elif not (mask.stride() == (frames * plan.mask_frame_stride, plan.mask_frame_stride, 1) and mask.data_ptr() % 16 == 0):
        held = mask_buffer(rows, frames, plan.n, mask.device)
        held.copy_(mask)
        mask = held
    out = torch.empty((rows, plan.length), dtype=torch.float16, device=re.device)
    with torch.cuda.device(plan.device):
        plan.exec_ptr(re.data_ptr(), im.data_ptr(), mask.data_ptr(), out.data_ptr(), plan._stream(None))
    return out


def masked_istft(re, im, mask, window, hop, length, n_fft, center=False, raw_sum=False):
    """short_istft with a real mask on the spectra, applied in the frames kernel: re, im, window, hop, length, n_fft, center and
    raw_sum as short_istft; mask a CUDA float16 tensor, either 1-D with n_fft / 2 + 1 values (one mask for every frame) or
    [R, F, n_fft / 2 + 1]. A per-frame mask whose frame stride is a multiple of 8 (a view mask_buffer returns has the pitch, 264, 520
    or 1032) is read in place; any other is copied once into such a buffer. Returns a new [R, length] tensor, the ISTFT of
    (mask * re, mask * im) with the products formed in fp32 in front of the merge's single rounding: no masked spectra are ever
    written."""
    n = int(n_fft)
    if n not in MISTFTN_LENGTHS:
        raise TfftError(5, "masked_istft takes n_fft = 512, 1024 or 2048")
    common._check_inverse("masked_istft", re, im, window, n)
    per_bin = _is_cuda_half(mask) and mask.dim() == 1
    if not (_is_cuda_half(mask) and mask.device == re.device
            and (tuple(mask.shape) == (common._bins(n),) if per_bin else tuple(mask.shape) == tuple(re.shape))):
        raise TfftError(5, f"masked_istft takes a CUDA float16 mask ({common._bins(n)},) or (R, F, {common._bins(n)}) on the device of the spectra")
    stride = 0 if per_bin else _in_place_stride(mask, n) or 0
    entry = _plan_for(n, int(re.shape[0]), length, hop, n // 2 if center else 0, raw_sum, per_bin, re.device.index,
                      0 if stride == common._pitch(n) else stride)
    return _run(entry, re, im, mask, window, length)
