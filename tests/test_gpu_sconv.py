"""Overlap-save causal convolution plans on the GPU (tfft_sconv_*, include/tfft_sconv.h): one kernel at transform length 4096 for
sequences of any length. Every case and tap kind is held, on ONE execution between guard zones, to

  1. the shipped tfft_conv_plan(4096, items, C) on windows built on the host (tests/sconv_ref.py) with the plan's own spectrum as
     filter, un-windowed, bit for bit (code that is already validated, not the code under test; it also pins
     sconv4096::filter_slot to conv4096::filter_slot and the item order to what that plan expects),
  2. fp64 with the same rounded spectrum, sample by sample (tests/elementwise_bound.py), every window in ulps of the largest
     magnitude of its own 4096-point circular convolution, K_SCONV of tests/sconv_ref.py,
  3. the true linear convolution of the binary16 taps in fp64, with the allowance for the spectrum's rounding
     (tests/test_sconv_host.py derives it on the CPU for these inputs),
  4. for delay taps the shifted input, within the same bound: a wrong segment, halo or filter index is a wrong delay,
  5. the layout: output between guard zones with out_seq_stride = L + 24, input with in_seq_stride = L + 8 whose gaps and guard
     zones hold NaN bit patterns (a read outside [0, L) of any sequence poisons the result), guards and gaps back bit for bit.

The plan's spectrum is held to tfft_lconv_spectrum_host at n = 4096 bit for bit on the way (the fp64 builder is restated in the
library). A fresh compute unit's LDS may read as zero, so a missing or misplaced zero fill shows only from a wave's second item on:
the cases with launch_iters make the waves loop.

Measured on the MI355X over three seeds: profiles/sconv_ulps.txt."""
import os
import subprocess

import numpy as np
import pytest

import dist_emulate as de
import elementwise_bound as eb
import lconv_ref as lr
import sconv_ref as sr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    return tensor_fft_amd


def _flat(x, stride, fill):
    """[B][C][L] -> one flat int16 array, sequence s at s * stride, everything else `fill`"""
    seqs, length = x.shape[0] * x.shape[1], x.shape[2]
    flat = np.full((seqs - 1) * stride + length, fill, dtype=np.int16)
    idx = (np.arange(seqs) * stride)[:, None] + np.arange(length)[None, :]
    flat[idx] = x.reshape(seqs, length).view(np.int16)
    return flat, idx


def run_sconv(tf, x, h, launch_iters=0):
    """One execution between guard zones with padded, unequal strides: returns (y [B][C][L] fp16, the plan's spectrum planes
    [C][4096] fp16). Checks on the way: guards and the gaps between output sequences untouched, the input bit-identical. The
    input's gaps and guards are NaNs."""
    rows, channels, length = x.shape
    taps = h.shape[1]
    in_stride, out_stride = length + 8, length + 24
    plan = tf.TfftLongConvPlan(rows, channels, length, taps, 0, in_seq_stride=in_stride, out_seq_stride=out_stride, launch_iters=launch_iters)
    assert (plan.halo, plan.hop, plan.segments) == sr.geometry(length, taps)
    assert plan.num_launches == 1 and plan.kernels == ["sconv4096::sconv4096_kernel"]
    d_h = torch.from_numpy(h.reshape(-1)).to(DEV)
    plan.set_taps(d_h)
    d_h.fill_(float("nan"))             # the plan owns its spectrum: the caller's taps are free after set_taps
    spec = tuple(t.cpu().numpy() for t in plan.spectrum())
    host_in, _ = _flat(x, in_stride, de.SENTINEL)
    assert np.isnan(np.int16(de.SENTINEL).view(np.float16))
    n_in = host_in.size
    n_out = (rows * channels - 1) * out_stride + length
    d_in = de._guarded(torch, n_in, host_in.view(np.float16))
    d_out = de._guarded(torch, n_out)
    g = de.GUARD
    plan.exec(d_in[g:g + n_in], d_out[g:g + n_out])
    torch.cuda.synchronize()
    assert de._guards_intact(torch, d_out), "output guard zone written"
    out = d_out[g:g + n_out].cpu().numpy().view(np.int16)
    _, idx = _flat(x, out_stride, 0)
    gaps = np.ones(n_out, bool)
    gaps[idx.reshape(-1)] = False
    assert (out[gaps] == de.SENTINEL).all(), "halves between output sequences written"
    assert de._guards_intact(torch, d_in)
    de._untouched(d_in[g:g + n_in].cpu().numpy().view(np.int16), host_in, "input sequences")
    plan.close()
    return out[idx].view(np.float16).reshape(rows, channels, length), spec


def via_conv_plan(tf, x, taps, spec):
    """the windows built on the host, the shipped TfftConvPlan(4096, items, C) with `spec` as its filter, un-windowed: [B][C][L] fp16"""
    rows, channels, length = x.shape
    w_re, w_im = sr.windows(x, taps)
    items = w_re.shape[0]
    plan = tf.TfftConvPlan(sr.N, items, channels, 0)
    plan.set_filter(torch.from_numpy(spec[0].reshape(-1)).to(DEV), torch.from_numpy(spec[1].reshape(-1)).to(DEV))
    d_x = torch.from_numpy(np.stack((w_re, w_im), axis=1).reshape(-1)).to(DEV)
    d_y = torch.empty_like(d_x)
    plan.exec(d_x, d_x[sr.N:], d_y, d_y[sr.N:])
    torch.cuda.synchronize()
    y = d_y.cpu().numpy().reshape(items, 2, sr.N)
    plan.close()
    return sr.unwindow(y[:, 0], y[:, 1], rows, channels, length, taps)


def _same_values(a, b):
    """equal as binary16 VALUES: -0 = +0, and no NaN on either side"""
    a, b = a.astype(np.float32), b.astype(np.float32)
    return not np.isnan(a).any() and not np.isnan(b).any() and np.array_equal(a, b)


def _per_sample(per_window, rows, channels, length, taps):
    """one value per window [items] -> the value of the window that holds each sample: [B][C][L]"""
    full = np.repeat(np.asarray(per_window, np.float64)[:, None], sr.N, axis=1)
    return sr.unwindow(full, full, rows, channels, length, taps)


def check_case(tf, length, taps, rows, channels, kind, launch_iters=0, seed=1, data=None, exact_taps=True):
    """data: (x, h) in place of the case's own (tests/test_gpu_conv_range.py: the same case at another amplitude); exact_taps = False:
    the taps were rounded again, so comparisons 3 and 4 are left out"""
    x, h = lr.case_data(length, taps, rows, channels, kind, seed) if data is None else data
    k = sr.K_SCONV
    what = f"sconv L={length} K={taps} B={rows} C={channels} iters={launch_iters} {kind}"
    y, spec = run_sconv(tf, x, h, launch_iters)
    # the restated fp64 spectrum builder: tfft_lconv_spectrum_host's n = 4096 spectrum, bit for bit
    for c in range(channels):
        want_re, want_im = tf.lconv_spectrum_host(h[c], sr.N)
        assert np.array_equal(spec[0][c].view(np.uint16), want_re.view(np.uint16)) and np.array_equal(spec[1][c].view(np.uint16), want_im.view(np.uint16)), (what, c)
    # 1. the shipped convolution plan on host-built windows, bit for bit
    want = via_conv_plan(tf, x, taps, spec)
    bad = np.argwhere(y.astype(np.float32) != want.astype(np.float32))
    assert _same_values(y, want), f"{what}: differs from windows -> TfftConvPlan -> un-window in {len(bad)} samples, first (b, c, t) = {bad[:3].tolist()}"
    # 2. fp64 with the same rounded spectrum; 3. the true linear convolution. Rows: the hop samples behind the halo of every window,
    #    zero on both sides where nothing is stored (beyond sample L, the zero partner)
    got_re, got_im = (sr.kept(p, rows, channels, length, taps) for p in sr.windows(y.astype(np.float64), taps))
    true = sr.reference_taps(x, h)
    peak = sr.window_peak(true)
    ref = sr.reference_spectrum(x, taps, spec[0], spec[1])
    if rows % 2:
        segs = sr.geometry(length, taps)[2]
        ref[-segs * channels:].imag = 0.0
        true[-segs * channels:].imag = 0.0
    ref_k, true_k = sr.kept(ref, rows, channels, length, taps), sr.kept(true, rows, channels, length, taps)
    worst = eb.check(got_re, got_im, ref_k.real, ref_k.imag, k, peak=peak, what=what)
    print(f"{what}: worst {worst:.3f} ulp")
    if exact_taps:
        eb.check(got_re, got_im, true_k.real, true_k.imag, k + 1.0, rel_l2=eb.REL_L2 + 2.0 ** -11, peak=peak, what=what + " (true linear convolution)")
    if kind == "delay" and exact_taps:
        # 4. the exact answer is the input shifted (times the tap: 1 in this file's cases)
        tol = (k + 1.0) * _per_sample(eb.ulp16(peak), rows, channels, length, taps)
        for c in range(channels):
            d = lr.delay_shift(c, taps)
            shifted = np.zeros((rows, length))
            shifted[:, d:] = float(h[c, d]) * x[:, c, :length - d].astype(np.float64) if d < length else 0.0
            assert (np.abs(y[:, c].astype(np.float64) - shifted) <= tol[:, c]).all(), (what, c)
    return worst


@pytest.mark.parametrize("kind", lr.TAP_KINDS)
@pytest.mark.parametrize("length,taps,rows,channels,launch_iters", sr.CASES)
def test_cases(tf, length, taps, rows, channels, launch_iters, kind):
    check_case(tf, length, taps, rows, channels, kind, launch_iters=launch_iters)


def test_launch_iters_never_changes_results(tf):
    length, taps, rows, channels = 6152, 130, 5, 3
    x, h = lr.case_data(length, taps, rows, channels, "decay", 4)
    a, _ = run_sconv(tf, x, h, 0)
    for iters in (1, 2, 5, 65535):
        b, _ = run_sconv(tf, x, h, iters)
        assert np.array_equal(a.view(np.uint16), b.view(np.uint16)), iters


def _plain_run(plan, x):
    d_x = torch.from_numpy(x.reshape(-1)).to(DEV)
    d_y = torch.zeros_like(d_x)
    plan.exec(d_x, d_y)
    torch.cuda.synchronize()
    return d_y.cpu().numpy().reshape(x.shape)


def test_exec_needs_taps_and_taps_can_be_replaced(tf):
    length, taps, rows, channels = 4104, 64, 4, 2
    x, h = lr.case_data(length, taps, rows, channels, "noise", 5)
    plan = tf.TfftLongConvPlan(rows, channels, length, taps, 0)
    d_x = torch.from_numpy(x.reshape(-1)).to(DEV)
    d_y = torch.empty_like(d_x)
    with pytest.raises(tf.TfftError, match="set_taps"):
        plan.exec(d_x, d_y)
    with pytest.raises(tf.TfftError, match="set_taps"):
        plan.spectrum()
    delta = np.zeros((channels, taps), np.float16)
    delta[:, 0] = 1.0
    plan.set_taps(torch.from_numpy(delta.reshape(-1)).to(DEV))
    first = _plain_run(plan, x)
    assert np.abs(first.astype(np.float64) - x.astype(np.float64)).max() <= sr.K_SCONV * eb.ulp16(1.5)     # y = x; |pair| < sqrt 2
    plan.set_taps(torch.from_numpy(h.reshape(-1)).to(DEV))
    second = _plain_run(plan, x)
    spec = tuple(t.cpu().numpy() for t in plan.spectrum())
    assert _same_values(second, via_conv_plan(tf, x, taps, spec))
    plan.close()
    # long_causal_conv: the convenience wrapper over the plan cache, bit for bit the plan
    t_x, t_h = torch.from_numpy(x).to(DEV), torch.from_numpy(h).to(DEV)
    y = tf.long_causal_conv(t_x, t_h)
    torch.cuda.synchronize()
    assert y.shape == t_x.shape and np.array_equal(y.cpu().numpy().view(np.uint16), second.view(np.uint16))
    # the same tensor, unchanged: the taps are not handed over again; changed in place: they are
    y2 = tf.long_causal_conv(t_x, t_h)
    t_h.copy_(torch.from_numpy(delta))
    y3 = tf.long_causal_conv(t_x, t_h)
    torch.cuda.synchronize()
    assert np.array_equal(y2.cpu().numpy().view(np.uint16), second.view(np.uint16))
    assert np.array_equal(y3.cpu().numpy().view(np.uint16), first.view(np.uint16))
    tf.sconv_cache_clear()


def test_in_place_and_partial_overlap_are_refused_and_nothing_is_launched(tf):
    length, taps, rows, channels = 4104, 7, 2, 2
    x, h = lr.case_data(length, taps, rows, channels, "noise", 8)
    plan = tf.TfftLongConvPlan(rows, channels, length, taps, 0)
    plan.set_taps(torch.from_numpy(h.reshape(-1)).to(DEV))
    total = rows * channels * length
    buf = torch.zeros(3 * total, dtype=torch.float16, device=DEV)            # the input in the middle third
    buf[total:2 * total] = torch.from_numpy(x.reshape(-1)).to(DEV)
    before = buf.cpu().numpy().view(np.uint16).copy()
    stream = torch.cuda.current_stream().cuda_stream
    src = buf.data_ptr() + 2 * total
    # exact in place; shifted by one chunk; the output's first chunk on the input's last; the output's last chunk on the input's first
    for dst in (src, src + 16, src + 2 * (total - 8), src - 2 * (total - 8)):
        with pytest.raises(tf.TfftError, match="overlap"):
            plan.exec_ptr(src, dst, stream)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint16), before)
    # disjoint thirds of one buffer are fine
    plan.exec(buf[total:2 * total], buf[2 * total:])
    torch.cuda.synchronize()
    assert np.array_equal(buf[2 * total:].cpu().numpy().view(np.uint16), _plain_run(plan, x).reshape(-1).view(np.uint16))
    assert np.array_equal(buf[:2 * total].cpu().numpy().view(np.uint16), before[:2 * total])
    plan.close()


def test_two_executions_under_stream_capture(tf):
    """An execution only launches a kernel, so it can be captured into a graph and replayed: two executions in a row on a single
    stream, the second on the first one's output."""
    length, taps, rows, channels = 8192, 2049, 5, 3
    x, h = lr.case_data(length, taps, rows, channels, "decay", 6)
    plan = tf.TfftLongConvPlan(rows, channels, length, taps, 0)
    plan.set_taps(torch.from_numpy(h.reshape(-1)).to(DEV))
    want1 = _plain_run(plan, x)
    want2 = _plain_run(plan, want1)
    d_x = torch.from_numpy(x.reshape(-1)).to(DEV)
    d_y1, d_y2 = torch.zeros_like(d_x), torch.zeros_like(d_x)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.exec(d_x, d_y1)
            plan.exec(d_y1, d_y2)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(d_y1.cpu().numpy().reshape(x.shape).view(np.uint16), want1.view(np.uint16))
    assert np.array_equal(d_y2.cpu().numpy().reshape(x.shape).view(np.uint16), want2.view(np.uint16))
    plan.close()


def test_long_causal_conv_agrees_with_causal_conv(tf):
    """(4096, 2049, 3, 2): the causal plan runs pack | n = 8192 | crop, the long plan two windows of 4096. Different transform
    lengths, so no bit equality: each lies within its own bound of the true linear convolution (its constant, plus the ulp the
    rounding of its own spectrum is allowed), each in its own unit, and the two differ by at most the sum."""
    length, taps, rows, channels = 4096, 2049, 3, 2
    x, h = lr.case_data(length, taps, rows, channels, "noise", 9)
    t_x, t_h = torch.from_numpy(x).to(DEV), torch.from_numpy(h).to(DEV)
    a = tf.long_causal_conv(t_x, t_h).cpu().numpy().astype(np.float64)
    b = tf.causal_conv(t_x, t_h).cpu().numpy().astype(np.float64)
    tf.sconv_cache_clear()
    tf.lconv_cache_clear()
    tol_a = (sr.K_SCONV + 1.0) * _per_sample(eb.ulp16(sr.window_peak(sr.reference_taps(x, h))), rows, channels, length, taps)
    n = lr.fft_length(length, taps)
    pair = eb.ulp16(lr.pair_peak(lr.reference_taps(x, h, n)))                       # item p * C + c
    tol_b = (lr.K_LCONV_COMPOSED + 1.0) * lr.unpair(np.repeat(pair[:, None], length, axis=1), np.repeat(pair[:, None], length, axis=1), rows, channels, length)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert (np.abs(a - b) <= tol_a + tol_b).all(), float((np.abs(a - b) / (tol_a + tol_b)).max())
    # and each against the true linear convolution on its own
    true = lr.reference_taps(x, h, n)
    want = lr.unpair(true.real, true.imag, rows, channels, length)
    assert (np.abs(a - want) <= tol_a).all() and (np.abs(b - want) <= tol_b).all()


def test_example_long_conv_exits_0(tf):
    exe = os.path.join(ROOT, "examples", "example_long_conv")
    r = subprocess.run([exe, "8192", "2049", "5", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout and "in place:" in r.stdout
