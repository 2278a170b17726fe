"""Gated overlap-save causal convolution plans on the GPU (tfft_gsconv_*, include/tfft_gsconv.h): y = g (.) (h * u + d u), u = p (.) x,
as ONE kernel at transform length 4096 for sequences of any length. Every case, tap kind and gate mode of tests/gsconv_ref.py is
held, on ONE execution between guard zones, to yardsticks that are code already validated, never the code under test:

  1. the plan's spectrum equals gconv_spectrum_host(h[c], 4096, skip[c]) in every bit (the fp64 builder is restated in the library),
  2. y equals g (.) un-window(TfftConvPlan(4096, items, C) on the windows of u = p (.) x built on the host, with the plan's own
     spectrum as filter) as binary16 values: gates formed on the CPU (exact: one binary16 rounding of an exact fp32 product). This
     also pins gsconv4096::filter_slot to conv4096::filter_slot, the item order, and BOTH gate indices: a pre gate taken at the
     window sample instead of the source sample, or a post gate taken at the window sample instead of the output sample, is a
     wrong gate wherever the halo is not zero,
  3. in the modes without a skip, y equals g (.) TfftLongConvPlan(u) as values,
  4. fp64 with the same rounded spectrum, every window in ulps of the largest magnitude of its own 4096-point circular convolution,
     K_SCONV of tests/sconv_ref.py: without a post gate on y sample by sample (tests/elementwise_bound.py), with one under
     |g| K ulp(peak) + 1/2 ulp16(|y|) per sample (tests/gsconv_ref.py derives it),
  5. the true result h * u + d u in fp64 with the binary16 taps and skip, with the "+ 1 ulp, + 2^-11 rel-L2" allowance for the
     spectrum's rounding (tests/test_gsconv_host.py measures what that rounding does on the CPU for these inputs), and for delay
     taps g (.) (shift(u) + d u),
  6. the layout: every array between guard zones, strides in L + 8, pre L + 16, post L + 32, out L + 24; the gaps and guards of all
     three inputs hold NaN bit patterns, so a read outside [0, L) of a sequence or gate, or of the gate of a row that does not
     exist, that gets used poisons the result; the output's guards and gaps untouched, the inputs back bit for bit.

With a post gate the rel-L2 part of 4 and 5 is not asserted: the error behind the gate is the error in front of it weighted sample
by sample with |g|, which bounds each sample (the bound above) but not the ratio of two weighted sums.

A fresh compute unit's LDS may read as zero, so a missing zero fill or a stale gate register shows only from a wave's second item
on: the cases with launch_iters make the waves loop, a full pair first and a zero partner after it."""
import os
import subprocess

import numpy as np
import pytest

import dist_emulate as de
import elementwise_bound as eb
import gsconv_ref as gs
import lconv_ref as lr
import sconv_ref as sr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LAUNCHED = set()            # kernels of every plan run_gsconv executed (test_all_four_instantiations_are_launched)
KERNELS = {f"gsconv4096::gsconv4096_kernel<{p}, {q}>" for p in ("true", "false") for q in ("true", "false")}


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    return tensor_fft_amd


def _tf_text(v):
    return "true" if v else "false"


def _flat(x, stride, fill):
    """[B][C][L] -> one flat int16 array, sequence s at s * stride, everything else `fill`"""
    seqs, length = x.shape[0] * x.shape[1], x.shape[2]
    flat = np.full((seqs - 1) * stride + length, fill, dtype=np.int16)
    idx = (np.arange(seqs) * stride)[:, None] + np.arange(length)[None, :]
    flat[idx] = x.reshape(seqs, length).view(np.int16)
    return flat, idx


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def run_gsconv(tf, x, h, p=None, g=None, skip=None, launch_iters=0):
    """One execution between guard zones with padded, unequal strides: returns (y [B][C][L] fp16, the plan's spectrum planes
    [C][4096] fp16). Checks on the way: the plan's kernel against its flags, guards and the gaps between output sequences
    untouched, the three inputs bit-identical. Gaps and guards of the inputs are NaNs."""
    rows, channels, length = x.shape
    taps = h.shape[1]
    in_stride, pre_stride, post_stride, out_stride = length + 8, length + 16, length + 32, length + 24
    plan = tf.TfftGatedLongConvPlan(rows, channels, length, taps, 0, pre_gate=p is not None, post_gate=g is not None, in_seq_stride=in_stride,
                                    out_seq_stride=out_stride, pre_seq_stride=pre_stride, post_seq_stride=post_stride, launch_iters=launch_iters)
    assert (plan.halo, plan.hop, plan.segments) == gs.geometry(length, taps)
    kernels = plan.kernels
    assert plan.num_launches == 1 and kernels == [f"gsconv4096::gsconv4096_kernel<{_tf_text(p is not None)}, {_tf_text(g is not None)}>"]
    LAUNCHED.update(kernels)
    d_h, d_skip = _dev(h), _dev(skip)
    plan.set_taps(d_h, d_skip)
    d_h.fill_(float("nan"))             # the plan owns its spectrum: the caller's taps and skip are free after set_taps
    if d_skip is not None:
        d_skip.fill_(float("nan"))
    spec = tuple(t.cpu().numpy() for t in plan.spectrum())
    assert np.isnan(np.int16(de.SENTINEL).view(np.float16))
    gd = de.GUARD
    hosts, bufs, views = {}, {}, {}
    for name, arr, stride in (("in", x, in_stride), ("pre", p, pre_stride), ("post", g, post_stride)):
        if arr is None:
            views[name] = None
            continue
        hosts[name], _ = _flat(arr, stride, de.SENTINEL)
        bufs[name] = de._guarded(torch, hosts[name].size, hosts[name].view(np.float16))
        views[name] = bufs[name][gd:gd + hosts[name].size]
    n_out = (rows * channels - 1) * out_stride + length
    d_out = de._guarded(torch, n_out)
    plan.exec(views["in"], d_out[gd:gd + n_out], pre=views["pre"], post=views["post"])
    torch.cuda.synchronize()
    assert de._guards_intact(torch, d_out), "output guard zone written"
    out = d_out[gd:gd + n_out].cpu().numpy().view(np.int16)
    _, idx = _flat(x, out_stride, 0)
    gaps = np.ones(n_out, bool)
    gaps[idx.reshape(-1)] = False
    assert (out[gaps] == de.SENTINEL).all(), "halves between output sequences written"
    for name in hosts:
        assert de._guards_intact(torch, bufs[name])
        de._untouched(views[name].cpu().numpy().view(np.int16), hosts[name], name + " sequences")
    plan.close()
    return out[idx].view(np.float16).reshape(rows, channels, length), spec


def via_conv_plan(tf, u, taps, spec):
    """yardstick 2: the windows of u built on the host, the shipped TfftConvPlan(4096, items, C) with `spec` as its filter,
    un-windowed: [B][C][L] fp16 (via_conv_plan of tests/test_gpu_sconv.py)"""
    rows, channels, length = u.shape
    w_re, w_im = sr.windows(u, taps)
    items = w_re.shape[0]
    plan = tf.TfftConvPlan(sr.N, items, channels, 0)
    plan.set_filter(_dev(spec[0]), _dev(spec[1]))
    d_x = _dev(np.stack((w_re, w_im), axis=1))
    d_y = torch.empty_like(d_x)
    plan.exec(d_x, d_x[sr.N:], d_y, d_y[sr.N:])
    torch.cuda.synchronize()
    y = d_y.cpu().numpy().reshape(items, 2, sr.N)
    plan.close()
    return sr.unwindow(y[:, 0], y[:, 1], rows, channels, length, taps)


def via_long_plan(tf, u, h, launch_iters=0):
    """yardstick 3: the shipped overlap-save plan on u, contiguous: [B][C][L] fp16"""
    rows, channels, length = u.shape
    plan = tf.TfftLongConvPlan(rows, channels, length, h.shape[1], 0, launch_iters=launch_iters)
    plan.set_taps(_dev(h))
    d_u = _dev(u)
    d_z = torch.zeros_like(d_u)
    plan.exec(d_u, d_z)
    torch.cuda.synchronize()
    plan.close()
    return d_z.cpu().numpy().reshape(u.shape)


def _same_values(a, b):
    """equal as binary16 VALUES: -0 = +0, and no NaN on either side"""
    a, b = a.astype(np.float32), b.astype(np.float32)
    return not np.isnan(a).any() and not np.isnan(b).any() and np.array_equal(a, b)


def _differs(y, want, what, yardstick):
    bad = np.argwhere(y.astype(np.float32) != want.astype(np.float32))
    return f"{what}: differs from {yardstick} in {len(bad)} samples, first (b, c, t) = {bad[:3].tolist()}"


def _within(y, want, tol, what):
    d = np.abs(y.astype(np.float64) - want)
    assert np.isfinite(y.astype(np.float64)).all(), what
    worst = float((d / tol).max())
    at = np.unravel_index(int(np.argmax(d / tol)), d.shape)
    assert (d <= tol).all(), f"{what}: {worst:.3f} x the bound at (b, c, t) = {at}"
    return worst


def check_case(tf, length, taps, rows, channels, kind, mode, launch_iters=0, seed=1, data=None, exact_taps=True):
    """data: (x, h, p, g, skip) in place of the case's own (tests/test_gpu_conv_range.py: the same case at another amplitude);
    exact_taps = False: the taps were rounded again, so the comparisons with the true result and the shifted input are left out.
    Returns the worst error of comparison 4 in its unit."""
    x, h, p, g, skip = gs.case_data(length, taps, rows, channels, kind, seed, mode) if data is None else data
    k = gs.K_SCONV
    what = f"gsconv L={length} K={taps} B={rows} C={channels} iters={launch_iters} {kind} {mode}"
    y, spec = run_gsconv(tf, x, h, p, g, skip, launch_iters)
    u = gs.gated_input(x, p)
    # 1. the restated fp64 spectrum builder with the skip folded in: tfft_gconv_spectrum_host's n = 4096 spectrum, bit for bit
    for c in range(channels):
        want_re, want_im = tf.gconv_spectrum_host(h[c], sr.N, None if skip is None else skip[c])
        assert np.array_equal(_bits(spec[0][c]), _bits(want_re)) and np.array_equal(_bits(spec[1][c]), _bits(want_im)), (what, c)
    # 2. the shipped convolution plan on host-built windows of u, then g on the CPU
    z = via_conv_plan(tf, u, taps, spec)
    want = gs.gated_output(z, g)
    assert _same_values(y, want), _differs(y, want, what, "g (.) un-window(TfftConvPlan(windows(p (.) x)))")
    # 3. without a skip: the shipped overlap-save plan on u, then g on the CPU
    if skip is None:
        want = gs.gated_output(via_long_plan(tf, u, h, launch_iters), g)
        assert _same_values(y, want), _differs(y, want, what, "g (.) TfftLongConvPlan(p (.) x)")
    # 4. fp64 with the same rounded spectrum; 5. the true result. Units: each window's circular-convolution peak
    true = gs.reference_true(u, h, skip)
    peak = sr.window_peak(true)
    ref = gs.reference_spectrum(u, taps, spec[0], spec[1])
    if rows % 2:
        segs = gs.geometry(length, taps)[2]
        ref[-segs * channels:].imag = 0.0               # the zero partner has no output: zeros on both sides
        true[-segs * channels:].imag = 0.0
    if g is None:
        got_re, got_im = (sr.kept(pl, rows, channels, length, taps) for pl in sr.windows(y.astype(np.float64), taps))
        ref_k, true_k = sr.kept(ref, rows, channels, length, taps), sr.kept(true, rows, channels, length, taps)
        worst = eb.check(got_re, got_im, ref_k.real, ref_k.imag, k, peak=peak, what=what)
        print(f"{what}: worst {worst:.3f} ulp")
        if exact_taps:
            eb.check(got_re, got_im, true_k.real, true_k.imag, k + 1.0, rel_l2=eb.REL_L2 + 2.0 ** -11, peak=peak, what=what + " (true result)")
    else:
        g64 = g.astype(np.float64)
        worst = _within(y, g64 * gs.joined(ref, rows, channels, length, taps), gs.post_gate_tolerance(y, g, k, peak, rows, channels, length, taps), what)
        print(f"{what}: worst {worst:.3f} x (|g| K ulp(peak) + 1/2 ulp(|y|))")
        if exact_taps:
            _within(y, g64 * gs.joined(true, rows, channels, length, taps), gs.post_gate_tolerance(y, g, k + 1.0, peak, rows, channels, length, taps),
                    what + " (true result)")
    if kind == "delay" and exact_taps:
        # a wrong segment, halo, filter or gate index is a wrong delay or a wrong gate: the exact answer is g (.) (shift(u) + d u)
        expected = gs.delay_expected(u, taps, skip, g, tap=[h[c, lr.delay_shift(c, taps)] for c in range(channels)])
        if g is None:
            tol = (k + 1.0) * gs.per_sample(eb.ulp16(peak), rows, channels, length, taps)
        else:
            tol = gs.post_gate_tolerance(y, g, k + 1.0, peak, rows, channels, length, taps)
        _within(y, expected, tol, what + " (delay)")
    return worst


@pytest.mark.parametrize("kind", gs.TAP_KINDS)
@pytest.mark.parametrize("length,taps,rows,channels,launch_iters,mode", gs.CASE_MODES)
def test_cases(tf, length, taps, rows, channels, launch_iters, mode, kind):
    check_case(tf, length, taps, rows, channels, kind, mode, launch_iters=launch_iters)


def _plain_run(plan, x, p=None, g=None):
    """contiguous tensors, default strides: [B][C][L] fp16"""
    d_x = _dev(x)
    d_y = torch.zeros_like(d_x)
    plan.exec(d_x, d_y, pre=_dev(p), post=_dev(g))
    torch.cuda.synchronize()
    return d_y.cpu().numpy().reshape(x.shape)


def test_ungated_plan_without_skip_is_the_overlap_save_plan(tf):
    """<false, false> keeps sconv4096_kernel's load and store: TfftLongConvPlan's bits outright, with looping waves and a zero partner"""
    length, taps, rows, channels, iters = 8192, 2049, 5, 3, 3
    x, h = lr.case_data(length, taps, rows, channels, "noise", 2)
    y, spec = run_gsconv(tf, x, h, launch_iters=iters)
    assert np.array_equal(_bits(y), _bits(via_long_plan(tf, x, h, iters)))
    for c in range(channels):
        want = tf.lconv_spectrum_host(h[c], sr.N)
        assert np.array_equal(_bits(spec[0][c]), _bits(want[0])) and np.array_equal(_bits(spec[1][c]), _bits(want[1]))


def test_launch_iters_never_changes_results(tf):
    length, taps, rows, channels = 8192, 2049, 5, 3
    x, h, p, g, skip = gs.case_data(length, taps, rows, channels, "noise", 4, "pre+post+skip")
    a, _ = run_gsconv(tf, x, h, p, g, skip, 0)
    for iters in (1, 3, 65535):                           # 65535: TFFT_LAUNCH_PERSISTENT
        b, _ = run_gsconv(tf, x, h, p, g, skip, iters)
        assert np.array_equal(_bits(a), _bits(b)), iters


def test_gates_may_alias_the_input_and_each_other(tf):
    """p = x and g = p, the same pointers and strides, equal passing copies: all three are only read"""
    length, taps, rows, channels = 6152, 130, 3, 3
    x, h, _, _, _ = gs.case_data(length, taps, rows, channels, "noise", 5, "pre+post")
    plan = tf.TfftGatedLongConvPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True)
    plan.set_taps(_dev(h))
    d_x = _dev(x)
    d_a, d_b = torch.zeros_like(d_x), torch.zeros_like(d_x)
    plan.exec(d_x, d_a, pre=d_x, post=d_x)
    plan.exec(d_x, d_b, pre=d_x.clone(), post=d_x.clone())
    torch.cuda.synchronize()
    a, b = d_a.cpu().numpy().reshape(x.shape), d_b.cpu().numpy().reshape(x.shape)
    assert np.array_equal(_bits(a), _bits(b))
    assert _same_values(a, gs.half_product(x, via_long_plan(tf, gs.half_product(x, x), h)))
    plan.close()


def test_refusals_launch_nothing(tf):
    length, taps, rows, channels = 4104, 7, 3, 2
    x, h, p, g, _ = gs.case_data(length, taps, rows, channels, "noise", 6, "pre+post")
    both = tf.TfftGatedLongConvPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True)
    none = tf.TfftGatedLongConvPlan(rows, channels, length, taps, 0)
    d_x, d_p, d_g = _dev(x), _dev(p), _dev(g)
    d_y = torch.full_like(d_x, 7.0)
    with pytest.raises(tf.TfftError, match="set_taps") as e:
        both.exec(d_x, d_y, pre=d_p, post=d_g)
    assert e.value.code == 5
    with pytest.raises(tf.TfftError, match="set_taps"):
        both.spectrum()
    both.set_taps(_dev(h))
    none.set_taps(_dev(h))
    stream = torch.cuda.current_stream().cuda_stream
    refused = [
        (lambda: both.exec(d_x, d_x, pre=d_p, post=d_g), "input and output overlap"),                       # exact in place
        (lambda: both.exec_ptr(d_x.data_ptr(), d_x.data_ptr() + 16, d_p.data_ptr(), d_g.data_ptr(), stream), "input and output overlap"),
        # the output's first chunk on the input's last one (refused before anything is launched, so nothing behind d_x is touched)
        (lambda: both.exec_ptr(d_x.data_ptr(), d_x.data_ptr() + 2 * (d_x.numel() - 8), d_p.data_ptr(), d_g.data_ptr(), stream), "input and output overlap"),
        (lambda: both.exec(d_x, d_y, pre=d_y, post=d_g), "pre gate and the output overlap"),                # a gate that is the output
        (lambda: both.exec(d_x, d_y, pre=d_p, post=d_y), "post gate and the output overlap"),
        (lambda: both.exec_ptr(d_x.data_ptr(), d_y.data_ptr(), d_p.data_ptr(), d_y.data_ptr() + 16, stream), "post gate and the output overlap"),
        (lambda: both.exec(d_x, d_y, pre=None, post=d_g), "pre gate"),                                     # a missing gate
        (lambda: both.exec(d_x, d_y, pre=d_p, post=None), "post gate"),
        (lambda: none.exec(d_x, d_y, pre=d_p), "no pre gate"),                                             # a surplus gate
        (lambda: none.exec(d_x, d_y, post=d_g), "no post gate"),
        (lambda: both.exec_ptr(d_x.data_ptr(), d_y.data_ptr(), d_p.data_ptr() + 2, d_g.data_ptr(), stream), "16-byte aligned"),
    ]
    for call, needle in refused:
        with pytest.raises(tf.TfftError, match=needle) as e:
            call()
        assert e.value.code == 5, needle                 # TFFT_ERR_ARG
    torch.cuda.synchronize()
    assert bool((d_y == 7.0).all())
    for t, host in ((d_x, x), (d_p, p), (d_g, g)):
        assert np.array_equal(_bits(t.cpu().numpy().reshape(x.shape)), _bits(host))
    both.close()
    none.close()


def test_taps_and_skip_can_be_replaced(tf):
    length, taps, rows, channels = 4104, 64, 4, 2
    x, h, p, g, skip = gs.case_data(length, taps, rows, channels, "noise", 7, "pre+post+skip")
    u = gs.gated_input(x, p)
    plan = tf.TfftGatedLongConvPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True)
    delta = np.zeros((channels, taps), np.float16)
    delta[:, 0] = 1.0
    plan.set_taps(_dev(delta))
    first = _plain_run(plan, x, p, g)
    assert _same_values(first, gs.gated_output(via_long_plan(tf, u, delta), g))
    plan.set_taps(_dev(h), _dev(skip))
    second = _plain_run(plan, x, p, g)
    spec = tuple(t.cpu().numpy() for t in plan.spectrum())
    for c in range(channels):
        want = tf.gconv_spectrum_host(h[c], 4096, skip[c])
        assert np.array_equal(_bits(spec[0][c]), _bits(want[0])) and np.array_equal(_bits(spec[1][c]), _bits(want[1]))
    assert _same_values(second, gs.gated_output(via_conv_plan(tf, u, taps, spec), g))
    plan.set_taps(_dev(h))                                    # the skip goes away again
    third = _plain_run(plan, x, p, g)
    assert _same_values(third, gs.gated_output(via_long_plan(tf, u, h), g)) and not _same_values(third, second)
    plan.close()


def test_execution_under_stream_capture(tf):
    """An execution only launches a kernel, so it can be captured into a graph and replayed (one stream, no parallel branches)."""
    length, taps, rows, channels = 8192, 2049, 5, 3
    x, h, p, g, skip = gs.case_data(length, taps, rows, channels, "noise", 8, "pre+post+skip")
    plan = tf.TfftGatedLongConvPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True)
    plan.set_taps(_dev(h), _dev(skip))
    assert plan.kernels == ["gsconv4096::gsconv4096_kernel<true, true>"]
    want = _plain_run(plan, x, p, g)
    d_x, d_p, d_g = _dev(x), _dev(p), _dev(g)
    d_y = torch.zeros_like(d_x)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.exec(d_x, d_y, pre=d_p, post=d_g)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d_y.cpu().numpy().reshape(x.shape)), _bits(want))
    plan.close()


def test_all_four_instantiations_are_launched(tf):
    """every kernel in the gfx950 code object of libtfft_gsconv.so is launched by one of the modes, and names itself as c++filt does"""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint

    for mode in ("pre", "post", "pre+post", "skip"):                 # (when this test is run on its own)
        length, taps, rows, channels, iters = gs.CASES[0]
        x, h, p, g, skip = gs.case_data(length, taps, rows, channels, "noise", 1, mode)
        run_gsconv(tf, x, h, p, g, skip, iters)
    mangled = [k for k in isa_lint.split_kernels(isa_lint.disassemble(tf.gsconv_lib_path())) if k.startswith("_Z")]
    demangled = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    shipped = {d.strip().removeprefix("void ").split("(")[0] for d in demangled if d.strip()}
    assert shipped == KERNELS, shipped
    assert shipped <= LAUNCHED, shipped - LAUNCHED


def test_gated_long_causal_conv(tf):
    from tensor_fft_amd import gsconv

    length, taps, rows, channels = 4104, 7, 3, 3
    x, h, p, g, skip = gs.case_data(length, taps, rows, channels, "noise", 10, "pre+post+skip")
    t_x, t_h, t_p, t_g, t_d = (torch.from_numpy(a).to(DEV) for a in (x, h, p, g, skip))
    tf.gsconv_cache_clear()
    for pre, post, d in ((p, g, skip), (p, None, None), (None, g, skip), (None, None, skip)):
        plan = tf.TfftGatedLongConvPlan(rows, channels, length, taps, 0, pre_gate=pre is not None, post_gate=post is not None)
        plan.set_taps(_dev(h), _dev(d))
        want = _plain_run(plan, x, pre, post)
        plan.close()
        y = tf.gated_long_causal_conv(t_x, t_h, pre=None if pre is None else t_p, post=None if post is None else t_g, skip=None if d is None else t_d)
        torch.cuda.synchronize()
        assert y.shape == t_x.shape and np.array_equal(_bits(y.cpu().numpy()), _bits(want))
    assert len(gsconv._plans) == 4
    # no gates, no skip: long_causal_conv, bit for bit
    y = tf.gated_long_causal_conv(t_x, t_h)
    z = tf.long_causal_conv(t_x, t_h)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(y.cpu().numpy()), _bits(z.cpu().numpy()))
    # the same tensors, unchanged: the cached plan is reused and taps and skip are not handed over again; the skip changed in place:
    # they are
    held = gsconv._plans[(rows, channels, length, taps, 0, True, True)][0]
    first = tf.gated_long_causal_conv(t_x, t_h, pre=t_p, post=t_g, skip=t_d)
    again = tf.gated_long_causal_conv(t_x, t_h, pre=t_p, post=t_g, skip=t_d)
    assert gsconv._plans[(rows, channels, length, taps, 0, True, True)][0] is held and len(gsconv._plans) == 4
    t_d.zero_()
    without = tf.gated_long_causal_conv(t_x, t_h, pre=t_p, post=t_g, skip=t_d)
    plain = tf.gated_long_causal_conv(t_x, t_h, pre=t_p, post=t_g)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(first.cpu().numpy()), _bits(again.cpu().numpy()))
    assert np.array_equal(_bits(without.cpu().numpy()), _bits(plain.cpu().numpy()))
    assert not np.array_equal(_bits(first.cpu().numpy()), _bits(plain.cpu().numpy()))
    # wrong dtypes, shapes and devices are refused
    for call in (lambda: tf.gated_long_causal_conv(t_x.float(), t_h), lambda: tf.gated_long_causal_conv(t_x, t_h.float()),
                 lambda: tf.gated_long_causal_conv(t_x, t_h, pre=t_p.float()), lambda: tf.gated_long_causal_conv(t_x, t_h, skip=t_d.float()),
                 lambda: tf.gated_long_causal_conv(t_x[0], t_h), lambda: tf.gated_long_causal_conv(t_x, t_h[:2]),
                 lambda: tf.gated_long_causal_conv(t_x, t_h, post=t_g[:, :, :8]), lambda: tf.gated_long_causal_conv(t_x, t_h, skip=t_d[:2]),
                 lambda: tf.gated_long_causal_conv(t_x.cpu(), t_h), lambda: tf.gated_long_causal_conv(t_x, t_h.cpu()),
                 lambda: tf.gated_long_causal_conv(t_x, t_h, pre=t_p.cpu()), lambda: tf.gated_long_causal_conv(t_x, t_h, skip=t_d.cpu())):
        with pytest.raises(tf.TfftError, match="gated_long_causal_conv takes"):
            call()
    # gated_causal_conv routes as before: the composed path of the gated causal plans at this length
    assert tf.TfftGatedConvPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True).kernels[0] == "gate_copy::pack_kernel<true>"
    tf.gsconv_cache_clear()
    assert not gsconv._plans
    tf.sconv_cache_clear()


def test_example_gated_long_conv_exits_0(tf):
    exe = os.path.join(ROOT, "examples", "example_gated_long_conv")
    r = subprocess.run([exe, "8192", "2049", "5", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout and "in place:" in r.stdout and "pre+post x 4" in r.stdout
