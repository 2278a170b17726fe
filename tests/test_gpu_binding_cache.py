"""The plan caches of the tensor functions whose own GPU tests do not look into them: causal_conv (lconv), long_causal_conv
(sconv), gated_causal_conv (gconv), gated_long_causal_conv (gsconv) and fftconv (conv), at the smallest shapes: B = 1, C = 1, K = 2,
L = 8, 16, ... (one length per key); fftconv at n = 4096 with batch 1, 2, ... Per function:

  - CACHE_SIZE + 1 distinct keys leave CACHE_SIZE entries, and the evicted plan is closed;
  - a repeated key returns the same plan object and moves it to the young end;
  - set_taps runs once for two calls with the same h, again after h.add_(0) bumped its version, and on every call for a
    non-contiguous h (fftconv: set_filter on every call, which is why its entries are bare plans);
  - the *_cache_clear function empties the dict.

Every output of the first pass is held to the family's fp64 reference (tests/*_ref.py) under the bound the family's own GPU test
uses against the true result, so a plan that computes nothing cannot pass. tests/test_gpu_gsconv.py already asserts that a repeated
key returns the same object and that gsconv_cache_clear empties the dict: those two points are left to it. The caches of bconv,
gbconv, cconv and gcconv are looked into by their own tests."""
import numpy as np
import pytest

import conv_ref
import elementwise_bound as eb
import gconv_ref as gr
import gsconv_ref as gs
import lconv_ref as lr
import sconv_ref as sr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
TAPS = 2
SKIP = np.array([0.375], np.float16)
TRUE_REL_L2 = eb.REL_L2 + 2.0 ** -11       # the allowance of the families' tests for the binary16 rounding of the spectrum


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    return tensor_fft_amd


def _check_pairs(y, true, k, what):
    """y [1][1][L] against the pair's true complex signal [1][n] (tests/test_gpu_lconv.py, comparison 3): one row, a zero partner"""
    length = y.shape[2]
    peak = lr.pair_peak(true)
    true.imag = 0.0
    got_re, got_im = lr.pair_planes(y.astype(np.float64), length)
    eb.check(got_re, got_im, true.real[:, :length], true.imag[:, :length], k + 1.0, rel_l2=TRUE_REL_L2, peak=peak, what=what)


def _check_windows(y, true, k, what):
    """y [1][1][L] against the windows' true circular convolutions [S][4096] (tests/test_gpu_sconv.py, comparison 3)"""
    rows, channels, length = y.shape
    peak = sr.window_peak(true)
    true.imag = 0.0
    got_re, got_im = (sr.kept(p, rows, channels, length, TAPS) for p in sr.windows(y.astype(np.float64), TAPS))
    true_k = sr.kept(true, rows, channels, length, TAPS)
    eb.check(got_re, got_im, true_k.real, true_k.imag, k + 1.0, rel_l2=TRUE_REL_L2, peak=peak, what=what)


# module, tensor function, plan class, cache size, clear function, skip weights, the check against the family's reference
FAMILIES = {
    "lconv": ("causal_conv", "TfftCausalConvPlan", "LCONV_CACHE_SIZE", "lconv_cache_clear", False,
              lambda x, h, y: _check_pairs(y, lr.reference_taps(x, h, 4096), lr.K_LCONV_FUSED, "causal_conv")),
    "sconv": ("long_causal_conv", "TfftLongConvPlan", "SCONV_CACHE_SIZE", "sconv_cache_clear", False,
              lambda x, h, y: _check_windows(y, sr.reference_taps(x, h), sr.K_SCONV, "long_causal_conv")),
    "gconv": ("gated_causal_conv", "TfftGatedConvPlan", "GCONV_CACHE_SIZE", "gconv_cache_clear", True,
              lambda x, h, y: _check_pairs(y, gr.reference_true(x, h, SKIP, 4096), gr.K_LCONV_FUSED, "gated_causal_conv")),
    "gsconv": ("gated_long_causal_conv", "TfftGatedLongConvPlan", "GSCONV_CACHE_SIZE", "gsconv_cache_clear", True,
               lambda x, h, y: _check_windows(y, gs.reference_true(x, h, SKIP), gs.K_SCONV, "gated_long_causal_conv")),
}


def _counted(monkeypatch, cls, name):
    """wraps cls.<name> to count its calls: the list holds one plan per call"""
    calls = []
    inner = getattr(cls, name)

    def wrapper(self, *args, **kwargs):
        calls.append(self)
        return inner(self, *args, **kwargs)

    monkeypatch.setattr(cls, name, wrapper)
    return calls


@pytest.mark.parametrize("family", list(FAMILIES))
def test_cache_and_taps_identity(tf, monkeypatch, family):
    import importlib

    fn_name, plan_name, size_name, clear_name, gated, check = FAMILIES[family]
    mod = importlib.import_module("tensor_fft_amd." + family)
    fn, clear, size = getattr(tf, fn_name), getattr(tf, clear_name), getattr(mod, size_name)
    calls = _counted(monkeypatch, getattr(tf, plan_name), "set_taps")
    d_skip = torch.from_numpy(SKIP).to(DEV)
    extra = {"skip": d_skip} if gated else {}

    def key(length):
        return (1, 1, length, TAPS, 0) + ((False, False) if gated else ())

    clear()
    assert mod._plans == {}
    lengths = [8 * (i + 1) for i in range(size + 1)]
    first = None
    alive = []              # (a freed h would lend its address, at version 0, to the next one: the same identity)
    for length in lengths:
        x, h = lr.case_data(length, TAPS, 1, 1, "noise", 11)
        alive.append(torch.from_numpy(h).to(DEV))
        y = fn(torch.from_numpy(x).to(DEV), alive[-1], **extra)
        torch.cuda.synchronize()
        assert y.shape == x.shape
        print(f"{fn_name} L={length}")
        check(x, h, y.cpu().numpy())
        entry = mod._plans[key(length)]
        assert isinstance(entry, list) and len(entry) == 2 and isinstance(entry[0], getattr(tf, plan_name))
        first = first or entry[0]
    # size + 1 keys: the oldest went, closed
    assert list(mod._plans) == [key(length) for length in lengths[1:]]
    assert first._h is None
    assert len(calls) == size + 1 and len(set(map(id, calls))) == size + 1
    # a repeated key: the same plan, now the youngest
    length = lengths[1]
    held = mod._plans[key(length)][0]
    x, h = lr.case_data(length, TAPS, 1, 1, "noise", 11)
    t_x, t_h = torch.from_numpy(x).to(DEV), torch.from_numpy(h).to(DEV)
    del calls[:]
    y1 = fn(t_x, t_h, **extra)             # a new tensor at this key: the taps are handed over
    assert list(mod._plans)[-1] == key(length) and len(mod._plans) == size
    if family != "gsconv":
        assert mod._plans[key(length)][0] is held
    assert calls == [held]
    y2 = fn(t_x, t_h, **extra)             # the same tensor, unchanged: not again
    assert calls == [held]
    t_h.add_(0)                            # the same values under a new version: again
    y3 = fn(t_x, t_h, **extra)
    assert calls == [held, held]
    wide = torch.zeros((1, 2 * TAPS), dtype=torch.float16, device=DEV)
    wide[:, ::2] = t_h
    strided = wide[:, ::2]
    assert not strided.is_contiguous()
    y4 = fn(t_x, strided, **extra)         # a non-contiguous h is copied per call: on every call
    y5 = fn(t_x, strided, **extra)
    assert calls == [held] * 4
    assert mod._plans[key(length)][1] is None
    y6 = fn(t_x, t_h, **extra)             # and the contiguous one after it is handed over anew
    assert calls == [held] * 5
    torch.cuda.synchronize()
    for y in (y2, y3, y4, y5, y6):
        assert torch.equal(y, y1)
    check(x, h, y6.cpu().numpy())
    if gated:
        d_skip.add_(0)                     # the skip weights have an identity of their own
        fn(t_x, t_h, **extra)
        assert calls == [held] * 6
        fn(t_x, t_h)                       # and None is another one
        assert calls == [held] * 7
    clear()
    if family != "gsconv":
        assert mod._plans == {}
    assert held._h is None


def test_fftconv_cache(tf, monkeypatch):
    from tensor_fft_amd import conv

    n, size = 4096, conv.CONV_CACHE_SIZE
    calls = _counted(monkeypatch, tf.TfftConvPlan, "set_filter")
    tf.conv_cache_clear()
    assert conv._plans == {}
    first = None
    for batch in range(1, size + 2):
        x_re, x_im, h_re, h_im = conv_ref.case_data(n, batch, 1, "gauss", 11)
        y_re, y_im = tf.fftconv(*(torch.from_numpy(a).to(DEV) for a in (x_re, x_im, h_re, h_im)))
        torch.cuda.synchronize()
        print(f"fftconv batch={batch}")
        eb.check(y_re.cpu().numpy(), y_im.cpu().numpy(), *conv_ref.reference(x_re, x_im, h_re, h_im), conv_ref.K_CONV_FUSED, what=f"fftconv batch {batch}")
        plan = conv._plans[(n, batch, 1, 0)]
        assert isinstance(plan, tf.TfftConvPlan)           # a bare plan: no identity is kept, the filter is set on every call
        first = first or plan
    assert list(conv._plans) == [(n, batch, 1, 0) for batch in range(2, size + 2)]
    assert first._h is None
    assert len(calls) == size + 1
    held = conv._plans[(n, 2, 1, 0)]
    tensors = [torch.from_numpy(a).to(DEV) for a in conv_ref.case_data(n, 2, 1, "gauss", 11)]
    del calls[:]
    a = tf.fftconv(*tensors)
    b = tf.fftconv(*tensors)
    torch.cuda.synchronize()
    assert list(conv._plans)[-1] == (n, 2, 1, 0) and conv._plans[(n, 2, 1, 0)] is held and len(conv._plans) == size
    assert calls == [held, held]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    tf.conv_cache_clear()
    assert conv._plans == {} and held._h is None
