"""Carried convolution plans on the GPU (tfft_cconv_*, include/tfft_cconv.h): the overlap-save causal convolution and its two
gradients on a chunk of a longer sequence, the history in front of x and the future behind g read from a second pointer.

The kernels are the shipped ones with their load ends re-indexed, and every window they transform is a window the shipped plans
transform on a longer sequence (tests/cconv_ref.py, checked in numpy by tests/test_cconv_host.py). So the reference is shipped,
validated code, bit for bit, wherever such a sequence exists:

  1. without a context: TfftLongConvPlan / TfftLongConvGradPlan on the same shape, every bit of y, dx and dh,
  2. forward with a history: samples [hop, hop + L) of TfftLongConvPlan at length hop + L on [zeros(hop - Hn) | hist | x]; and the
     true linear convolution of [hist | x] within K_SCONV + 1 ulp of the window's peak (check 3 of tests/test_gpu_sconv.py),
  3. input gradient with a future: samples [0, L) of TfftLongConvGradPlan.input_grad at length L + Fn on [g | fut],
  4. tap gradient with a history: with partials = 1 on both sides the bits of TfftLongConvGradPlan(hop + L, partials = 1) on
     ([zeros(hop - Hn) | hist | x], [zeros(hop) | g]); with partials 0 and 2 within dh_bound of the fp64 sum over the plan's own
     items, and two executions give the same bits,
  5. chunk invariance: three hop-aligned chunks out of one buffer (hist = in - 64, future = g + L) give the bits of the
     whole-sequence plans; chunks that are not hop-aligned, with context carry_min, the true result within the bound,
  6. the contract: aliasing, set_taps first, launch_iters, stream capture, contexts never written,
  7. autograd over two chunks, 8. the example.

Every execution of 1 - 4 runs between NaN-filled guard zones; sequences and contexts have padded, unequal strides whose gaps
hold NaN bit patterns, so a read outside [0, L) of a sequence or [0, Hn) / [0, Fn) of a context poisons the result.
No tolerance constant of its own: K_SCONV, K_CONV_FUSED, A_SPECTRUM, the + 1 ulp / + 2^-11 allowance and dh_bound of
tests/sconv_ref.py and tests/bconv_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import bconv_ref as br
import cconv_ref as cr
import dist_emulate as de
import elementwise_bound as eb
import lconv_ref as lr
import sconv_ref as sr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
FWD_KERNELS = ["cconv4096::cconv4096_kernel"]
GRAD_KERNELS = ["cconv4096::dgrad_kernel", "cconv4096::wgrad_kernel", "cconv4096::wreduce_kernel"]
WITH_CONTEXT = [c for c in cr.CASES if c[4]]


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    return tensor_fft_amd


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and not np.isnan(a.astype(np.float32)).any() and np.array_equal(_bits(a), _bits(b))


class Seqs:
    """[B][C][n] binary16 on the device between guard zones, sequence s at s * stride, gaps and guards NaN"""

    def __init__(self, x, stride):
        self.shape = x.shape
        seqs, n = x.shape[0] * x.shape[1], x.shape[2]
        self.host = np.full((seqs - 1) * stride + n, de.SENTINEL, dtype=np.int16)
        self.idx = (np.arange(seqs) * stride)[:, None] + np.arange(n)[None, :]
        self.host[self.idx] = x.reshape(seqs, n).view(np.int16)
        self.buf = de._guarded(torch, self.host.size, self.host.view(np.float16))
        self.flat = self.buf[de.GUARD:de.GUARD + self.host.size]

    def untouched(self, what):
        assert de._guards_intact(torch, self.buf), what
        de._untouched(self.flat.cpu().numpy().view(np.int16), self.host, what)


class Out:
    """an output of [B][C][L] binary16 between guard zones, all sentinels before the execution"""

    def __init__(self, shape, stride):
        self.shape, seqs = shape, shape[0] * shape[1]
        self.n = (seqs - 1) * stride + shape[2]
        self.idx = (np.arange(seqs) * stride)[:, None] + np.arange(shape[2])[None, :]
        self.buf = de._guarded(torch, self.n)
        self.flat = self.buf[de.GUARD:de.GUARD + self.n]

    def result(self):
        assert de._guards_intact(torch, self.buf), "output guard zone written"
        out = self.flat.cpu().numpy().view(np.int16)
        gaps = np.ones(self.n, bool)
        gaps[self.idx.reshape(-1)] = False
        assert (out[gaps] == de.SENTINEL).all(), "halves between output sequences written"
        return out[self.idx].view(np.float16).reshape(self.shape)


def _dev(a):
    """a flat device copy (the shared case data is read-only on the host)"""
    return torch.from_numpy(np.array(a).reshape(-1)).to(DEV)


def _taps(h):
    return _dev(h)


def run_fwd(tf, x, h, hist=None, launch_iters=0, history=None):
    """one carried forward execution; history: the plan's Hn where hist is None (a NULL history on a plan that has one)"""
    rows, channels, length = x.shape
    taps = h.shape[1]
    hn = hist.shape[2] if hist is not None else (history or 0)
    plan = tf.TfftChunkedConvPlan(rows, channels, length, taps, 0, in_seq_stride=length + 8, out_seq_stride=length + 24, launch_iters=launch_iters,
                                  history=hn, hist_seq_stride=hn + 16 if hn else 0)
    assert (plan.halo, plan.hop, plan.segments) == sr.geometry(length, taps) and plan.carry_min == cr.carry_min(taps)
    assert plan.num_launches == 1 and plan.kernels == FWD_KERNELS
    plan.set_taps(_taps(h))
    d_x, d_y = Seqs(x, length + 8), Out(x.shape, length + 24)
    d_h = Seqs(hist, hn + 16) if hist is not None else None
    plan.exec(d_x.flat, d_y.flat, None if d_h is None else d_h.flat)
    torch.cuda.synchronize()
    y = d_y.result()
    d_x.untouched("input sequences")
    if d_h is not None:
        d_h.untouched("history")
    plan.close()
    return y


def run_dx(tf, g, h, fut=None, launch_iters=0, future=None):
    rows, channels, length = g.shape
    taps = h.shape[1]
    fn = fut.shape[2] if fut is not None else (future or 0)
    plan = tf.TfftChunkedConvGradPlan(rows, channels, length, taps, 0, g_seq_stride=length + 8, dx_seq_stride=length + 24, launch_iters=launch_iters,
                                      future=fn, fut_seq_stride=fn + 16 if fn else 0)
    assert plan.num_launches == 3 and plan.kernels == GRAD_KERNELS
    plan.set_taps(_taps(h))
    d_g, d_dx = Seqs(g, length + 8), Out(g.shape, length + 24)
    d_f = Seqs(fut, fn + 16) if fut is not None else None
    plan.input_grad(d_g.flat, d_dx.flat, None if d_f is None else d_f.flat)
    torch.cuda.synchronize()
    dx = d_dx.result()
    d_g.untouched("g")
    if d_f is not None:
        d_f.untouched("future")
    plan.close()
    return dx


def run_dh(tf, x, g, taps, hist=None, partials=0, history=None, twice=False):
    """one (or two) tap-gradient executions: dh [C][K] fp32 between guard words"""
    rows, channels, length = x.shape
    hn = hist.shape[2] if hist is not None else (history or 0)
    plan = tf.TfftChunkedConvGradPlan(rows, channels, length, taps, 0, x_seq_stride=length + 8, g_seq_stride=length + 24, partials=partials,
                                      history=hn, hist_seq_stride=hn + 16 if hn else 0)
    assert plan.partials == br.partials_of(rows, channels, length, taps, partials)
    d_x, d_g = Seqs(x, length + 8), Seqs(g, length + 24)
    d_h = Seqs(hist, hn + 16) if hist is not None else None
    outs = []
    for _ in range(2 if twice else 1):
        buf = torch.full((64 + channels * taps + 64,), float("nan"), dtype=torch.float32, device=DEV)
        plan.tap_grad(d_x.flat, d_g.flat, buf[64:64 + channels * taps], None if d_h is None else d_h.flat)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.isnan(host[:64]).all() and np.isnan(host[-64:]).all(), "tap gradient written outside [C][K]"
        outs.append(host[64:-64].reshape(channels, taps).copy())
    d_x.untouched("x")
    d_g.untouched("g")
    if d_h is not None:
        d_h.untouched("history")
    plan.close()
    return outs if twice else outs[0]


def long_fwd(tf, x, h):
    rows, channels, length = x.shape
    plan = tf.TfftLongConvPlan(rows, channels, length, h.shape[1], 0)
    plan.set_taps(_taps(h))
    d_x = _dev(x)
    d_y = torch.zeros_like(d_x)
    plan.exec(d_x, d_y)
    torch.cuda.synchronize()
    plan.close()
    return d_y.cpu().numpy().reshape(x.shape)


def long_dx(tf, g, h):
    rows, channels, length = g.shape
    plan = tf.TfftLongConvGradPlan(rows, channels, length, h.shape[1], 0)
    plan.set_taps(_taps(h))
    d_g = _dev(g)
    d_dx = torch.zeros_like(d_g)
    plan.input_grad(d_g, d_dx)
    torch.cuda.synchronize()
    plan.close()
    return d_dx.cpu().numpy().reshape(g.shape)


def long_dh(tf, x, g, taps, partials=0):
    rows, channels, length = x.shape
    plan = tf.TfftLongConvGradPlan(rows, channels, length, taps, 0, partials=partials)
    dh = torch.zeros((channels, taps), dtype=torch.float32, device=DEV)
    plan.tap_grad(_dev(x), _dev(g), dh)
    torch.cuda.synchronize()
    plan.close()
    return dh.cpu().numpy()


_data_cache = {}


def case(length, taps, rows, channels, ctx, kind, seed=1):
    """(x, h, g, hist, fut) of a case, computed once and shared (never written)"""
    key = (length, taps, rows, channels, ctx, kind, seed)
    if key not in _data_cache:
        x, h = lr.case_data(length, taps, rows, channels, kind, seed)
        g = br.grad_signal(rows, channels, length, taps, seed)
        hist = cr.context_signal(rows, channels, ctx, seed, 0) if ctx else None
        fut = cr.context_signal(rows, channels, ctx, seed, 1) if ctx else None
        for a in (x, h, g, hist, fut):
            if a is not None:
                a.setflags(write=False)
        _data_cache[key] = (x, h, g, hist, fut)
    return _data_cache[key]


def _zero_partner(ref, rows, channels, segs):
    if rows % 2:
        ref[-segs * channels:].imag = 0.0
    return ref


# ------------------------------------------------------------------------------------------- 1. no context is the shipped plan

@pytest.mark.parametrize("kind", lr.TAP_KINDS)
@pytest.mark.parametrize("length,taps,rows,channels,ctx,launch_iters", cr.CASES)
def test_no_context_is_the_shipped_plan(tf, length, taps, rows, channels, ctx, launch_iters, kind):
    """NULL contexts, on a plan created with and without room for one: every bit of the shipped plans on the same shape"""
    x, h, g, _, _ = case(length, taps, rows, channels, ctx, kind)
    want_y, want_dx = long_fwd(tf, x, h), long_dx(tf, g, h)
    want_dh = long_dh(tf, x, g, taps)
    for room in sorted({0, ctx}):
        assert _same_bits(run_fwd(tf, x, h, None, launch_iters, history=room), want_y), ("y", room)
        assert _same_bits(run_dx(tf, g, h, None, launch_iters, future=room), want_dx), ("dx", room)
        assert _same_bits(run_dh(tf, x, g, taps, None, 0, history=room), want_dh), ("dh", room)


def test_a_context_at_halo_0_is_refused(tf):
    with pytest.raises(tf.TfftError, match="history must not exceed the halo"):
        tf.TfftChunkedConvPlan(1, 1, 8, 1, 0, history=8)
    with pytest.raises(tf.TfftError, match="future must not exceed the halo"):
        tf.TfftChunkedConvGradPlan(1, 1, 8, 1, 0, future=8)
    x, h, _, _, _ = case(8, 1, 1, 1, 0, "delta")
    plan = tf.TfftChunkedConvPlan(1, 1, 8, 1, 0)
    plan.set_taps(_taps(h))
    d_x = _dev(x)
    d_y, d_hist = torch.zeros_like(d_x), torch.zeros_like(d_x)
    with pytest.raises(tf.TfftError, match="hist must be NULL"):
        plan.exec_ptr(d_x.data_ptr(), d_hist.data_ptr(), d_y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    plan.close()


# ------------------------------------------------------------------------------------------- 2. forward with history

@pytest.mark.parametrize("kind", lr.TAP_KINDS)
@pytest.mark.parametrize("length,taps,rows,channels,ctx,launch_iters", WITH_CONTEXT)
def test_forward_with_history(tf, length, taps, rows, channels, ctx, launch_iters, kind):
    x, h, _, hist, _ = case(length, taps, rows, channels, ctx, kind)
    halo, hop, segs = sr.geometry(length, taps)
    what = f"cconv L={length} K={taps} B={rows} C={channels} Hn={ctx} iters={launch_iters} {kind}"
    y = run_fwd(tf, x, h, hist, launch_iters)
    # bit for bit: segment s + 1 of the shipped plan on [zeros(hop - Hn) | hist | x] is window s here
    want = long_fwd(tf, cr.front_padded(x, hist, taps), h)[:, :, hop:hop + length]
    bad = np.argwhere(_bits(y) != _bits(want))
    assert _same_bits(y, want), f"{what}: differs from the long plan on the concatenated sequence in {len(bad)} samples, first (b, c, t) = {bad[:3].tolist()}"
    # the true linear convolution of [hist | x], window by window in ulps of the window's peak
    got_re, got_im = (sr.kept(p, rows, channels, length, taps) for p in sr.windows(y.astype(np.float64), taps))
    true = _zero_partner(cr.reference_taps(x, h, hist), rows, channels, segs)
    true_k = sr.kept(true, rows, channels, length, taps)
    worst = eb.check(got_re, got_im, true_k.real, true_k.imag, sr.K_SCONV + 1.0, rel_l2=eb.REL_L2 + 2.0 ** -11, peak=sr.window_peak(true),
                     what=what + " (true linear convolution)")
    print(f"{what}: worst {worst:.3f} ulp of the window's peak against the true linear convolution")


# ------------------------------------------------------------------------------------------- 3. input gradient with future

@pytest.mark.parametrize("kind", lr.TAP_KINDS)
@pytest.mark.parametrize("length,taps,rows,channels,ctx,launch_iters", WITH_CONTEXT)
def test_input_grad_with_future(tf, length, taps, rows, channels, ctx, launch_iters, kind):
    _, h, g, _, fut = case(length, taps, rows, channels, ctx, kind)
    what = f"cconv dgrad L={length} K={taps} B={rows} C={channels} Fn={ctx} iters={launch_iters} {kind}"
    dx = run_dx(tf, g, h, fut, launch_iters)
    want = long_dx(tf, cr.extend(g, fut=fut), h)[:, :, :length]
    bad = np.argwhere(_bits(dx) != _bits(want))
    assert _same_bits(dx, want), f"{what}: differs from the gradient plan on [g | fut] in {len(bad)} samples, first (b, c, t) = {bad[:3].tolist()}"


# ------------------------------------------------------------------------------------------- 4. tap gradient with history

@pytest.mark.parametrize("kind", lr.TAP_KINDS)
@pytest.mark.parametrize("length,taps,rows,channels,ctx,launch_iters", WITH_CONTEXT)
def test_tap_grad_with_history(tf, length, taps, rows, channels, ctx, launch_iters, kind):
    x, _, g, hist, _ = case(length, taps, rows, channels, ctx, kind)
    halo, hop, segs = sr.geometry(length, taps)
    what = f"cconv wgrad L={length} K={taps} B={rows} C={channels} Hn={ctx} {kind}"
    # partials = 1 on both sides: the same items in the same order, the extra items of the long plan are exact zeros
    dh1 = run_dh(tf, x, g, taps, hist, partials=1)
    want = long_dh(tf, cr.front_padded(x, hist, taps), cr.extend(g, np.zeros(g.shape[:2] + (hop,), g.dtype)), taps, partials=1)
    assert _same_bits(dh1, want), f"{what}: partials 1 differs from the gradient plan on the concatenated sequences in {(_bits(dh1) != _bits(want)).sum()} taps"
    # the fp64 sum over the plan's own items (tests/test_cconv_host.py holds it to the direct sums), within dh_bound
    items = cr.dh_items(x, g, taps, hist)
    ref = br.dh_from_items(items, channels, taps)
    bound = br.dh_bound(items, channels)
    for partials in (0, 2):
        a, b = run_dh(tf, x, g, taps, hist, partials=partials, twice=True)
        assert _same_bits(a, b), f"{what}: partials {partials}: two executions differ"
        err = np.abs(a.astype(np.float64) - ref)
        print(f"{what}: partials {partials}: worst {float((err / bound[:, None]).max()):.3f} of dh_bound")
        assert (err <= bound[:, None]).all(), f"{what}: partials {partials}: {float((err / bound[:, None]).max()):.3f} of dh_bound"
    assert (np.abs(dh1.astype(np.float64) - ref) <= bound[:, None]).all(), what


# ------------------------------------------------------------------------------------------- 5. chunk invariance

def _chunked(tf, x, g, h, chunk, ctx, partials=0):
    """y, dx and the chunks' dh of [B][C][L_total] run in chunks of `chunk` samples out of ONE device buffer each: in_seq_stride =
    L_total, hist = in - ctx, future = g + chunk; the outputs go to buffers of their own with the same stride"""
    rows, channels, total = x.shape
    taps = h.shape[1]
    d_x, d_g = _dev(x), _dev(g)
    d_y = torch.full_like(d_x, float("nan"))
    d_dx = torch.full_like(d_x, float("nan"))
    d_taps = _taps(h)
    n = total // chunk
    assert n * chunk == total
    dhs = []
    for k in range(n):
        t0 = k * chunk
        hn, fn = (ctx if k else 0), (ctx if k < n - 1 else 0)
        fwd = tf.TfftChunkedConvPlan(rows, channels, chunk, taps, 0, in_seq_stride=total, out_seq_stride=total, history=hn, hist_seq_stride=total if hn else 0)
        fwd.set_taps(d_taps)
        fwd.exec(d_x[t0:], d_y[t0:], d_x[t0 - hn:] if hn else None)
        grad = tf.TfftChunkedConvGradPlan(rows, channels, chunk, taps, 0, x_seq_stride=total, g_seq_stride=total, dx_seq_stride=total, partials=partials,
                                          history=hn, hist_seq_stride=total if hn else 0, future=fn, fut_seq_stride=total if fn else 0)
        grad.set_taps(d_taps)
        grad.input_grad(d_g[t0:], d_dx[t0:], d_g[t0 + chunk:] if fn else None)
        dh = torch.zeros((channels, taps), dtype=torch.float32, device=DEV)
        grad.tap_grad(d_x[t0:], d_g[t0:], dh, d_x[t0 - hn:] if hn else None)
        torch.cuda.synchronize()
        dhs.append(dh.cpu().numpy())
        fwd.close()
        grad.close()
    assert np.array_equal(d_x.cpu().numpy().view(np.uint16), x.reshape(-1).view(np.uint16)) and np.array_equal(d_g.cpu().numpy().view(np.uint16), g.reshape(-1).view(np.uint16))
    return d_y.cpu().numpy().reshape(x.shape), d_dx.cpu().numpy().reshape(x.shape), dhs


def test_chunk_invariance(tf):
    total, taps, rows, channels = 12096, 65, 3, 2
    halo, hop, segs = sr.geometry(total, taps)
    assert (halo, hop, segs) == (64, 4032, 3)
    x, h = lr.case_data(total, taps, rows, channels, "decay", 3)
    g = br.grad_signal(rows, channels, total, taps, 3)
    # hop-aligned chunks with context = halo: the whole-sequence plans' windows, so their bits
    y, dx, dhs = _chunked(tf, x, g, h, hop, halo)
    assert _same_bits(y, long_fwd(tf, x, h)), "y of three chunks differs from the whole-sequence plan"
    assert _same_bits(dx, long_dx(tf, g, h)), "dx of three chunks differs from the whole-sequence plan"
    items = br.dh_items(x, g, taps)
    dh = np.sum([d.astype(np.float64) for d in dhs], axis=0)
    err = np.abs(dh - br.dh_direct(x, g, taps))
    bound = br.dh_bound(items, channels)
    print(f"chunked dh: worst {float((err / bound[:, None]).max()):.3f} of dh_bound")
    assert (err <= bound[:, None]).all()
    # chunks of 4040 (not hop-aligned: two windows each, other windows than the whole-sequence plan's) with context carry_min: the
    # true result within K_SCONV + 1 ulp of the peak of the window that computed each sample
    chunk, cm = 4040, cr.carry_min(taps)
    total2 = 3 * chunk
    x2, _ = lr.case_data(total2, taps, rows, channels, "decay", 3)
    g2 = br.grad_signal(rows, channels, total2, taps, 3)
    y2, dx2, _ = _chunked(tf, x2, g2, h, chunk, cm)
    for k in range(3):
        t0 = k * chunk
        xc, gc = x2[:, :, t0:t0 + chunk], g2[:, :, t0:t0 + chunk]
        hist = x2[:, :, t0 - cm:t0] if k else None
        fut = g2[:, :, t0 + chunk:t0 + chunk + cm] if k < 2 else None
        segs2 = sr.geometry(chunk, taps)[2]
        true = _zero_partner(cr.reference_taps(xc, h, hist), rows, channels, segs2)
        got_re, got_im = (sr.kept(p, rows, channels, chunk, taps) for p in sr.windows(y2[:, :, t0:t0 + chunk].astype(np.float64), taps))
        true_k = sr.kept(true, rows, channels, chunk, taps)
        eb.check(got_re, got_im, true_k.real, true_k.imag, sr.K_SCONV + 1.0, rel_l2=eb.REL_L2 + 2.0 ** -11, peak=sr.window_peak(true), what=f"y chunk {k}")
        true = _zero_partner(cr.dx_reference_taps(gc, h, fut), rows, channels, segs2)
        got_re, got_im = (br.dx_kept(p, rows, channels, chunk, taps) for p in br.dx_windows(dx2[:, :, t0:t0 + chunk].astype(np.float64), taps))
        true_k = br.dx_kept(true, rows, channels, chunk, taps)
        eb.check(got_re, got_im, true_k.real, true_k.imag, sr.K_SCONV + 1.0, rel_l2=eb.REL_L2 + 2.0 ** -11, peak=sr.window_peak(true), what=f"dx chunk {k}")
    # ... and those true results are the whole sequence's: carry_min loses nothing
    assert np.abs(np.concatenate([cr.y_direct(x2[:, :, k * chunk:(k + 1) * chunk], h, x2[:, :, k * chunk - cm:k * chunk] if k else None) for k in range(3)], axis=-1)
                  - cr.y_direct(x2, h)).max() <= 1e-13


# ------------------------------------------------------------------------------------------- 6. the contract

def test_outputs_overlapping_inputs_or_contexts_are_refused_and_nothing_is_launched(tf):
    length, taps, rows, channels, hn = 4104, 7, 2, 2, 8
    x, h, _, _, _ = case(length, taps, rows, channels, hn, "noise", seed=8)
    seqs, stride = rows * channels, length + 64
    span = seqs * stride
    # one buffer of three spans; the sequences lie in the middle span, each with 64 halves (0.5) in front of it
    buf = torch.zeros(3 * span, dtype=torch.float16, device=DEV)
    mid = buf[span:2 * span].view(seqs, stride)
    mid[:, 64:] = _dev(x).view(seqs, length)
    mid[:, :64] = 0.5
    before = buf.cpu().numpy().view(np.uint16).copy()
    stream = torch.cuda.current_stream().cuda_stream
    src = buf.data_ptr() + 2 * (span + 64)
    hist = src - 2 * hn                                                          # the zero-copy call: a view into what lies in front ...
    fut = src + 2 * length                                                       # ... and behind: the 8 halves after every sequence
    fwd = tf.TfftChunkedConvPlan(rows, channels, length, taps, 0, in_seq_stride=stride, out_seq_stride=stride, history=hn, hist_seq_stride=stride)
    fwd.set_taps(_taps(h))
    grad = tf.TfftChunkedConvGradPlan(rows, channels, length, taps, 0, x_seq_stride=stride, g_seq_stride=stride, dx_seq_stride=stride,
                                      history=hn, hist_seq_stride=stride, future=hn, fut_seq_stride=stride)
    grad.set_taps(_taps(h))
    dh_ok = torch.zeros((channels, taps), dtype=torch.float32, device=DEV)
    # the output on the input: exact, shifted by a chunk, its first chunk on the input's last
    for dst in (src, src + 16, src + 2 * (length - 8)):
        with pytest.raises(tf.TfftError, match="input and output overlap"):
            fwd.exec_ptr(src, hist, dst, stream)
        with pytest.raises(tf.TfftError, match="g and dx overlap"):
            grad.input_grad_ptr(src, fut, dst, stream)
    # the tap gradient on x, on the history, on the end of the last sequence
    for bad_dh in (src, hist, src + 2 * (span - 64) - 4 * channels * taps):
        with pytest.raises(tf.TfftError, match="the tap gradient overlaps"):
            grad.tap_grad_ptr(src, hist, src, bad_dh, stream)
    # The output on a context alone, element-exact on the context's own length and stride: histories (futures) of 8 halves, `stride`
    # apart, in a buffer of their own. An output whose last chunk is the history is refused; one that starts right behind the
    # history (in the gap to the next one) shares nothing and runs.
    scr = torch.zeros(span + 2 * length, dtype=torch.float16, device=DEV)
    ctx = scr.data_ptr() + 2 * length
    with pytest.raises(tf.TfftError, match="hist and output overlap"):
        fwd.exec_ptr(src, ctx, ctx - 2 * (length - 8), stream)
    with pytest.raises(tf.TfftError, match="hist and output overlap"):
        fwd.exec_ptr(src, ctx, ctx, stream)
    with pytest.raises(tf.TfftError, match="g_future and dx overlap"):
        grad.input_grad_ptr(src, ctx, ctx - 2 * (length - 8), stream)
    with pytest.raises(tf.TfftError, match="the tap gradient overlaps"):
        grad.tap_grad_ptr(src, ctx, src, ctx + 2 * (seqs - 1) * stride, stream)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint16), before) and not scr.cpu().numpy().any()
    fwd.exec_ptr(src, ctx, ctx + 2 * hn, stream)                                 # a history of zeros: the shipped plan's result
    torch.cuda.synchronize()
    got = scr[length + hn:length + hn + span].view(seqs, stride)[:, :length].cpu().numpy().reshape(x.shape)
    assert _same_bits(got, long_fwd(tf, x, h)) and not scr[:length + hn].cpu().numpy().any()
    # hist = in - Hn (and future = g + L) with the input's own stride is accepted; outputs in the last span
    dst = buf.data_ptr() + 2 * (2 * span + 64)
    fwd.exec_ptr(src, hist, dst, stream)
    torch.cuda.synchronize()
    got = buf[2 * span:].view(seqs, stride)[:, 64:].cpu().numpy().reshape(x.shape)
    assert _same_bits(got, run_fwd(tf, x, h, np.full((rows, channels, hn), 0.5, np.float16)))
    grad.input_grad_ptr(src, fut, dst, stream)
    grad.tap_grad_ptr(src, hist, src, dh_ok.data_ptr(), stream)                  # x and g may be the same memory
    torch.cuda.synchronize()
    assert np.array_equal(buf[:2 * span].cpu().numpy().view(np.uint16), before[:2 * span])
    assert np.isfinite(dh_ok.cpu().numpy()).all()
    # misaligned contexts
    with pytest.raises(tf.TfftError, match="hist must be 16-byte aligned"):
        fwd.exec_ptr(src, hist + 2, dst, stream)
    with pytest.raises(tf.TfftError, match="g_future must be 16-byte aligned"):
        grad.input_grad_ptr(src, fut + 8, dst, stream)
    with pytest.raises(tf.TfftError, match="x_hist must be 16-byte aligned"):
        grad.tap_grad_ptr(src, hist + 4, src, dh_ok.data_ptr(), stream)
    fwd.close()
    grad.close()


def test_exec_needs_taps(tf):
    length, taps, rows, channels = 4104, 7, 2, 2
    fwd = tf.TfftChunkedConvPlan(rows, channels, length, taps, 0, history=8)
    grad = tf.TfftChunkedConvGradPlan(rows, channels, length, taps, 0, future=8)
    d_x = torch.zeros(rows * channels * length, dtype=torch.float16, device=DEV)
    d_y = torch.zeros_like(d_x)
    with pytest.raises(tf.TfftError, match="set_taps"):
        fwd.exec(d_x, d_y)
    with pytest.raises(tf.TfftError, match="set_taps"):
        fwd.spectrum()
    with pytest.raises(tf.TfftError, match="set_taps"):
        grad.input_grad(d_x, d_y)
    dh = torch.zeros((channels, taps), dtype=torch.float32, device=DEV)
    grad.tap_grad(d_x, d_x, dh)                                                   # the tap gradient needs no taps
    torch.cuda.synchronize()
    assert not dh.cpu().numpy().any()
    fwd.close()
    grad.close()


def test_launch_iters_never_changes_results(tf):
    length, taps, rows, channels, ctx = 6152, 130, 5, 3, 136
    x, h, g, hist, fut = case(length, taps, rows, channels, ctx, "decay", seed=4)
    y, dx = run_fwd(tf, x, h, hist, 0), run_dx(tf, g, h, fut, 0)
    for iters in (1, 2, 5, 65535):
        assert _same_bits(run_fwd(tf, x, h, hist, iters), y), iters
        assert _same_bits(run_dx(tf, g, h, fut, iters), dx), iters


def test_executions_with_contexts_under_stream_capture(tf):
    length, taps, rows, channels, ctx = 8064, 65, 2, 3, 64
    x, h, g, hist, fut = case(length, taps, rows, channels, ctx, "noise", seed=6)
    want_y, want_dx = run_fwd(tf, x, h, hist), run_dx(tf, g, h, fut)
    fwd = tf.TfftChunkedConvPlan(rows, channels, length, taps, 0, history=ctx)
    grad = tf.TfftChunkedConvGradPlan(rows, channels, length, taps, 0, future=ctx)
    fwd.set_taps(_taps(h))
    grad.set_taps(_taps(h))
    d = {k: _dev(v) for k, v in dict(x=x, g=g, hist=hist, fut=fut).items()}
    d_y, d_dx = torch.zeros_like(d["x"]), torch.zeros_like(d["x"])
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            fwd.exec(d["x"], d_y, d["hist"])
            grad.input_grad(d["g"], d_dx, d["fut"])
    for _ in range(2):
        d_y.zero_()
        d_dx.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(d_y.cpu().numpy().reshape(x.shape), want_y) and _same_bits(d_dx.cpu().numpy().reshape(x.shape), want_dx)
    fwd.close()
    grad.close()


# ------------------------------------------------------------------------------------------- 7. autograd

def test_autograd_over_two_chunks(tf):
    """Two chunks of (4104, 7, 3, 3), the second with the first one's end as its history. Loss = sum(g1 * y1) + sum(g2 * y2) with
    fixed binary16 g, so the gradients are the direct sums on the concatenated sequence. What autograd adds: x1.grad = dx of chunk 1
    (no future) + the history's gradient on its last Hn samples; h.grad = fp16(dh1) + fp16(dh2). The tolerance is the sum of the
    bounds of those terms, plus half a binary16 ulp of the result for autograd's own addition (and for the cast of each dh)."""
    length, taps, rows, channels = 4104, 7, 3, 3
    halo, hop, segs = sr.geometry(length, taps)
    x, h = lr.case_data(2 * length, taps, rows, channels, "noise", 7)
    g = br.grad_signal(rows, channels, 2 * length, taps, 7)
    tf.cconv_cache_clear()
    t_x1 = torch.from_numpy(x[:, :, :length].copy()).to(DEV).requires_grad_(True)
    t_x2 = torch.from_numpy(x[:, :, length:].copy()).to(DEV).requires_grad_(True)
    t_h = torch.from_numpy(h.copy()).to(DEV).requires_grad_(True)
    t_g = torch.from_numpy(g).to(DEV)
    y1 = tf.differentiable_chunked_causal_conv(t_x1, t_h)
    hist = tf.next_history(t_x1, None, halo)
    assert hist.data_ptr() == t_x1.data_ptr() + 2 * (length - halo)                       # a view, not a copy
    y2 = tf.differentiable_chunked_causal_conv(t_x2, t_h, hist)
    y = torch.cat([y1, y2], -1)
    assert _same_bits(y.detach().cpu().numpy()[:, :, :length], long_fwd(tf, x[:, :, :length], h))
    from tensor_fft_amd import cconv
    assert len(cconv._fwd_plans) == 2 and not cconv._dx_plans and not cconv._dh_plans
    (y.float() * t_g.float()).sum().backward()
    torch.cuda.synchronize()
    k = sr.K_SCONV + 1.0
    # x.grad: the direct sum on the whole sequence. Bounds: dx of each chunk within k ulp of its window's peak, the history's
    # gradient likewise (one window of Hn samples), autograd's addition half an ulp of the result
    want = br.dx_direct(g, h)
    got = np.concatenate([t_x1.grad.cpu().numpy(), t_x2.grad.cpu().numpy()], -1).astype(np.float64)
    tol = np.zeros_like(want)
    for c0 in (0, length):
        gc = g[:, :, c0:c0 + length]
        peak = sr.window_peak(_zero_partner(br.dx_reference_taps(gc, h), rows, channels, segs))
        full = np.repeat(eb.ulp16(peak)[:, None], sr.N, axis=1)
        tol[:, :, c0:c0 + length] = k * br.dx_unwindow(full, full, rows, channels, length, taps)
    fn = min(length, cr.carry_min(taps))
    hpeak = sr.window_peak(_zero_partner(cr.dx_reference_taps(np.zeros((rows, channels, halo), np.float16), h, g[:, :, length:length + fn]), rows, channels, 1))
    full = np.repeat(eb.ulp16(hpeak)[:, None], sr.N, axis=1)
    tol[:, :, length - halo:length] += k * br.dx_unwindow(full, full, rows, channels, halo, taps)
    tol[:, :, length - halo:length] += 0.5 * eb.ulp16(np.abs(want[:, :, length - halo:length]) + tol[:, :, length - halo:length])
    assert (np.abs(got - want) <= tol).all(), float((np.abs(got - want) / tol).max())
    # the history's gradient alone, against its direct sum
    hg = cr.dhist_direct(g[:, :, length:], h, halo)
    assert np.abs(hg - (want - np.concatenate([br.dx_direct(g[:, :, :length], h), br.dx_direct(g[:, :, length:], h)], -1))[:, :, length - halo:length]).max() <= 1e-13
    # h.grad: dh1 + dh2, each within its dh_bound and cast to binary16 (half an ulp each), added by autograd (half an ulp)
    want_dh = br.dh_direct(x, g, taps)
    b1 = br.dh_bound(br.dh_items(x[:, :, :length], g[:, :, :length], taps), channels)
    b2 = br.dh_bound(cr.dh_items(x[:, :, length:], g[:, :, length:], taps, x[:, :, length - halo:length]), channels)
    d1 = br.dh_direct(x[:, :, :length], g[:, :, :length], taps)
    d2 = cr.dh_direct(x[:, :, length:], g[:, :, length:], taps, x[:, :, length - halo:length])
    assert np.abs(d1 + d2 - want_dh).max() <= 1e-13 * max(1.0, np.abs(want_dh).max())
    tol_dh = (b1 + b2)[:, None] + 0.5 * (eb.ulp16(np.abs(d1) + b1[:, None]) + eb.ulp16(np.abs(d2) + b2[:, None]))
    tol_dh = tol_dh + 0.5 * eb.ulp16(np.abs(want_dh) + tol_dh)
    got_dh = t_h.grad.cpu().numpy().astype(np.float64)
    assert t_h.grad.dtype == torch.float16 and (np.abs(got_dh - want_dh) <= tol_dh).all(), float((np.abs(got_dh - want_dh) / tol_dh).max())
    tf.cconv_cache_clear()


def test_each_gradient_runs_only_when_asked(tf):
    from tensor_fft_amd import cconv

    length, taps, rows, channels = 4104, 7, 3, 3
    halo = sr.geometry(length, taps)[0]
    x, h = lr.case_data(length, taps, rows, channels, "noise", 7)
    t_hist = torch.from_numpy(cr.context_signal(rows, channels, halo, 7, 0)).to(DEV)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
        tf.cconv_cache_clear()
        t_x = torch.from_numpy(x.copy()).to(DEV).requires_grad_(need[0])
        t_h = torch.from_numpy(h.copy()).to(DEV).requires_grad_(need[1])
        hist = t_hist.clone().requires_grad_(need[2])
        tf.differentiable_chunked_causal_conv(t_x, t_h, hist).float().sum().backward()
        torch.cuda.synchronize()
        # the input gradient's cache holds dx's plan (length L) and the history's (length Hn)
        assert len(cconv._dx_plans) == int(need[0]) + int(need[2]) and len(cconv._dh_plans) == int(need[1]), need
        assert (t_x.grad is not None) == need[0] and (t_h.grad is not None) == need[1] and (hist.grad is not None) == need[2]
        if need[2]:
            want = cr.dhist_direct(np.ones((rows, channels, length), np.float16), h, halo)
            peak = sr.window_peak(_zero_partner(cr.dx_reference_taps(np.zeros((rows, channels, halo), np.float16), h, np.ones((rows, channels, 8), np.float16)), rows, channels, 1))
            full = np.repeat(eb.ulp16(peak)[:, None], sr.N, axis=1)
            tol = (sr.K_SCONV + 1.0) * br.dx_unwindow(full, full, rows, channels, halo, taps)
            assert (np.abs(hist.grad.cpu().numpy().astype(np.float64) - want) <= tol).all()
    tf.cconv_cache_clear()


def test_views_are_not_copied(tf):
    """the convenience functions hand a chunk of a longer buffer and its history to the plan as they are: the plan's strides are the
    buffer's, and the result is the bits of the plan run by hand"""
    from tensor_fft_amd import cconv

    total, taps, rows, channels = 12096, 65, 3, 2
    halo, hop, _ = sr.geometry(total, taps)
    x, h = lr.case_data(total, taps, rows, channels, "decay", 3)
    t_x, t_h = torch.from_numpy(x).to(DEV), torch.from_numpy(h).to(DEV)
    tf.cconv_cache_clear()
    ys = []
    hist = None
    for k in range(3):
        chunk = t_x[..., k * hop:(k + 1) * hop]
        ys.append(tf.chunked_causal_conv(chunk, t_h, hist))
        hist = tf.next_history(chunk, hist, halo)
        assert hist.data_ptr() == t_x.data_ptr() + 2 * ((k + 1) * hop - halo)
    torch.cuda.synchronize()
    keys = list(cconv._fwd_plans)
    assert [(k[5], k[6], k[7]) for k in keys] == [(total, 0, 0), (total, halo, total)], keys
    assert _same_bits(torch.cat(ys, -1).cpu().numpy(), long_fwd(tf, x, h))
    tf.cconv_cache_clear()


# ------------------------------------------------------------------------------------------- 8. the example

def test_example_chunked_conv_exits_0(tf):
    exe = os.path.join(ROOT, "examples", "example_chunked_conv")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
