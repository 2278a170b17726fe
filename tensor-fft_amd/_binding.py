"""What every add-on binding does the same way, beneath both families (_conv_common.py: the nine convolution bindings;
_stft_common.py: the four STFT ones): loading a library and setting its prototypes from a table, the return-code check, the life
cycle of a plan handle, the three workspace calls, the CUDA-tensor predicates and the cache of plans. Private: the public names
stay in the thirteen modules. It imports neither family, and torch only inside a call that needs it. No fallback of any kind."""
import ctypes
import os

from . import capi
from .capi import TfftError


def _load(below, path, what, prototypes):
    """Calls `below` (the loader of what the add-on is layered on: the add-on binds to the libraries, and the HIP runtime, this
    process already holds), then loads the add-on at `path` ("the `what` add-on") and sets `prototypes`,
    {symbol: (restype, argtypes)}. Raises (never falls back) when the file has not been built."""
    below()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the {what} add-on has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` from the repository root.")
    L = ctypes.CDLL(path)
    for name, (restype, argtypes) in prototypes.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    return L


def _check(L, prefix, rc):
    if rc != capi.TFFT_OK:
        raise TfftError(rc, getattr(L, prefix + "last_error")().decode())


def _is_cuda(t, dtype):
    import torch

    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype


def _is_cuda_half(t):
    import torch

    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16


class _Handle:
    """The owner of one C plan handle. A subclass sets _prefix, its library's ("tfft_bconv_"), and, where the calls on its handle
    are not <prefix>plan_*, _plan ("grad_": tfft_cconv_grad_destroy); its __init__ goes through _open and sets `device`."""
    _plan = "plan_"
    _ws = None       # the workspace tensor a plan keeps alive

    def _open(self, L, create, *args):
        """create(*args, &handle)"""
        self._lib = L
        self._h = ctypes.c_void_p()
        self._check(create(*args, ctypes.byref(self._h)))

    def _check(self, rc):
        if rc != capi.TFFT_OK:
            _check(self._lib, self._prefix, rc)

    def _fn(self, name):
        return getattr(self._lib, self._prefix + self._plan + name)

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            self._fn("destroy")(h)
            self._ws = None

    __del__ = close

    @property
    def num_launches(self):
        return int(self._fn("num_launches")(self._h))

    @property
    def kernels(self):
        """<prefix><plan>kernels: the kernels of the plan, in launch order."""
        return capi._kernel_lines(self._fn("kernels"), self._h)

    def _stream(self, stream):
        import torch

        return torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream

    def _check_kind(self, t, what):
        """`t` is one of the `what` ("sequences") an execution takes: a contiguous CUDA float16 tensor on the plan's device"""
        if not (_is_cuda_half(t) and t.is_contiguous()):
            raise TfftError(5, f"{what} must be contiguous CUDA float16 tensors")
        if t.device.index != self.device:
            raise TfftError(5, "tensor on another device than the plan")


class _Workspace:
    """The workspace calls of a _Handle whose library has them: <prefix><plan>workspace_bytes, set_workspace and prepare."""

    def _workspace_bytes(self):
        return int(self._fn("workspace_bytes")(self._h))

    workspace_bytes = property(_workspace_bytes)     # (the inverse STFT plans, whose workspace_bytes() is a method, define their own)

    def set_workspace(self, tensor):
        """Hands a torch CUDA tensor in as the plan's workspace (kept alive by the plan)."""
        self._check(self._fn("set_workspace")(self._h, tensor.data_ptr(), tensor.numel() * tensor.element_size()))
        self._ws = tensor

    def prepare(self):
        """Allocates the plan's own workspace now (<prefix><plan>prepare): later executions only launch kernels."""
        self._check(self._fn("prepare")(self._h))


# ---- the tensor functions. A module keeps the plans of its last `size` keys in a dict of its own, least recently used first out,
# each entry [plan, identity of the taps or the window it holds]
def _cached(plans, size, key, make):
    entry = plans.pop(key, None)
    if entry is None:
        entry = [make(), None]
    plans[key] = entry
    while len(plans) > size:
        plans.pop(next(iter(plans)))[0].close()
    return entry


def _cache_clear(*caches):
    for plans in caches:
        while plans:
            plans.popitem()[1][0].close()
