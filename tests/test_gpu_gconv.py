"""Gated causal convolution plans on the GPU (tfft_gconv_*, include/tfft_gconv.h): y = g (.) (h * u + d u), u = p (.) x, as one fused
kernel at transform length 4096 and on the composed path (gated pack, tfft_conv_plan, gated crop). Every case, tap kind and gate
mode is held, on ONE execution between guard zones, to yardsticks that are code already validated, never the code under test:

  1. gates: u = p (.) x formed on the CPU (exact: one binary16 rounding of an exact fp32 product), the shipped TfftCausalConvPlan on u
     on the same path, times g on the CPU: a gated plan without skip equals it bit for bit as binary16 values. hipcc's default
     kernel mode keeps fp16 subnormals, so no allowance is made for them.
  2. skip: the plan's own spectrum handed to the shipped TfftConvPlan on the zero-padded pair planes of u, cropped, times g on the
     CPU: bit for bit again (this also pins gconv4096::filter_slot to conv4096::filter_slot).
  3. truth: for the plans without a post gate, the fp64 linear convolution h * u + d u with the binary16 taps and skip, under
     K_LCONV_* + 1 ulp of the pair's peak and rel-L2 REL_L2 + 2^-11, the allowance tests/test_gpu_lconv.py grants for the rounding of
     the spectrum (tests/gconv_ref.py: the rounding of H' alone moves a kept sample by 0.54 ulp and rel-L2 2.2e-4 at most).
  4. the layout: every array between guard zones, strides in L + 8, pre L + 16, post L + 32, out L + 24; the gaps and guards of all
     three inputs hold NaN bit patterns, so a read beyond sample L of a sequence or gate, or of the gate of a row that does not
     exist, that gets used poisons the whole pair; the output's guards and gaps untouched, the inputs back bit for bit.

A fresh compute unit's LDS may read as zero, so a missing zero fill or a stale gate shows only from a wave's second item on: the
cases with launch_iters make the waves loop."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dist_emulate as de
import elementwise_bound as eb
import gconv_ref as gr
import lconv_ref as lr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LAUNCHED = set()            # kernels of every plan the cases below executed (test_every_kernel_of_the_add_on_is_launched)
FUSED = {f"gconv4096::gconv4096_kernel<{p}, {q}>" for p in ("true", "false") for q in ("true", "false")}
COPIES = {f"gate_copy::{k}_kernel<{v}>" for k in ("pack", "crop") for v in ("true", "false")}


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


def run_gconv(tf, x, h, p=None, g=None, skip=None, launch_iters=0, composed=False, in_place=False):
    """One execution out of place between guard zones with padded, unequal strides (or in place): returns (y [B][C][L] fp16, the
    plan's spectrum planes [C][n] fp16). Checks on the way: the plan's kernels against its flags, guards and the gaps between
    output sequences untouched, the three inputs bit-identical. Gaps and guards of the inputs are NaNs."""
    rows, channels, length = x.shape
    taps = h.shape[1]
    in_stride, pre_stride, post_stride = length + 8, length + 16, length + 32
    out_stride = in_stride if in_place else length + 24
    plan = tf.TfftGatedConvPlan(rows, channels, length, taps, 0, pre_gate=p is not None, post_gate=g is not None, composed=composed,
                                in_seq_stride=in_stride, out_seq_stride=out_stride, pre_seq_stride=pre_stride, post_seq_stride=post_stride,
                                launch_iters=launch_iters)
    kernels = plan.kernels
    assert plan.num_launches == len(kernels)
    if plan.n == 4096 and not composed:
        assert kernels == [f"gconv4096::gconv4096_kernel<{_tf_text(p is not None)}, {_tf_text(g is not None)}>"] and plan.workspace_bytes == 0
    else:
        assert kernels[0] == f"gate_copy::pack_kernel<{_tf_text(p is not None)}>" and kernels[-1] == f"gate_copy::crop_kernel<{_tf_text(g is not None)}>"
        assert plan.workspace_bytes >= (rows + 1) // 2 * channels * plan.n * 4
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
    d_out = bufs["in"] if in_place else de._guarded(torch, n_out)
    plan.exec(views["in"], d_out[gd:gd + n_out], pre=views["pre"], post=views["post"])
    torch.cuda.synchronize()
    assert de._guards_intact(torch, d_out), "output guard zone written"
    out = d_out[gd:gd + n_out].cpu().numpy().view(np.int16)
    _, idx = _flat(x, out_stride, 0)
    gaps = np.ones(n_out, bool)
    gaps[idx.reshape(-1)] = False
    assert (out[gaps] == de.SENTINEL).all(), "halves between output sequences written"
    for name in hosts:
        if in_place and name == "in":
            continue
        assert de._guards_intact(torch, bufs[name])
        de._untouched(views[name].cpu().numpy().view(np.int16), hosts[name], name + " sequences")
    plan.close()
    return out[idx].view(np.float16).reshape(rows, channels, length), spec


def via_lconv_plan(tf, u, h, launch_iters, composed):
    """yardstick 1: the shipped causal plan on u, contiguous: [B][C][L] fp16"""
    rows, channels, length = u.shape
    plan = tf.TfftCausalConvPlan(rows, channels, length, h.shape[1], 0, launch_iters=launch_iters, composed=composed)
    plan.set_taps(_dev(h))
    d_u = _dev(u)
    d_z = torch.zeros_like(d_u)
    plan.exec(d_u, d_z)
    torch.cuda.synchronize()
    plan.close()
    return d_z.cpu().numpy().reshape(u.shape)


def via_conv_plan(tf, u, spec, n):
    """yardstick 2: pad and interleave on the host, the shipped TfftConvPlan(n, items, C) with `spec` as its filter, crop (via_conv_plan
    of tests/test_gpu_lconv.py). Returns [B][C][L] fp16."""
    rows, channels, length = u.shape
    p_re, p_im = lr.pair_planes(u, n)
    items = p_re.shape[0]
    plan = tf.TfftConvPlan(n, items, channels, 0)
    plan.set_filter(_dev(spec[0]), _dev(spec[1]))
    d_x = _dev(np.stack((p_re, p_im), axis=1))
    d_y = torch.empty_like(d_x)
    plan.exec(d_x, d_x[n:], d_y, d_y[n:])
    torch.cuda.synchronize()
    y = d_y.cpu().numpy().reshape(items, 2, n)
    plan.close()
    return lr.unpair(y[:, 0], y[:, 1], rows, channels, length)


def _same_values(a, b):
    """equal as binary16 VALUES: -0 = +0, and no NaN on either side"""
    a, b = a.astype(np.float32), b.astype(np.float32)
    return not np.isnan(a).any() and not np.isnan(b).any() and np.array_equal(a, b)


def _differs(y, want, what, yardstick):
    bad = np.argwhere(y.astype(np.float32) != want.astype(np.float32))
    return f"{what}: differs from {yardstick} in {len(bad)} samples, first (b, c, t) = {bad[:3].tolist()}"


def check_case(tf, length, taps, rows, channels, kind, mode, k, launch_iters=0, composed=False, seed=1, data=None, exact_taps=True):
    """data: (x, h, p, g, skip) in place of the case's own (tests/test_gpu_conv_range.py: the same case at another amplitude);
    exact_taps = False: the taps were rounded again, so comparison 3 and the shifted input are left out. Returns the worst error of
    z = the shipped plan's result with this plan's spectrum (yardstick 2: y is g (.) z bit for bit) against fp64 with that spectrum."""
    x, h, p, g, skip = gr.case_data(length, taps, rows, channels, kind, seed, mode) if data is None else data
    n = gr.plan_length(length, taps, composed)
    path = "fused" if n == 4096 and not composed else "composed"
    what = f"gconv L={length} K={taps} B={rows} C={channels} iters={launch_iters} {path} {kind} {mode}"
    y, spec = run_gconv(tf, x, h, p, g, skip, launch_iters, composed)
    u = gr.gated_input(x, p)
    # 1. gates: the shipped causal plan on u, then g on the CPU
    if skip is None:
        want = gr.gated_output(via_lconv_plan(tf, u, h, launch_iters, composed), g)
        assert _same_values(y, want), _differs(y, want, what, "g (.) TfftCausalConvPlan(p (.) x)")
    # 2. skip: the plan's own spectrum through the shipped convolution plan on padded planes, then g on the CPU
    z = via_conv_plan(tf, u, spec, n)
    want = gr.gated_output(z, g)
    assert _same_values(y, want), _differs(y, want, what, "g (.) crop(TfftConvPlan(pad(p (.) x)))")
    true = gr.reference_true(u, h, skip, n)
    peak = lr.pair_peak(true)
    # 3. truth, where no second gate rounds the result again
    if g is None and exact_taps:
        got_re, got_im = lr.pair_planes(y.astype(np.float64), length)
        if rows % 2:
            true[-channels:].imag = 0.0             # the zero partner has no output: zeros on both sides
        worst = eb.check(got_re, got_im, true.real[:, :length], true.imag[:, :length], k + 1.0, rel_l2=eb.REL_L2 + 2.0 ** -11, peak=peak,
                         what=what + " (true linear convolution with skip)")
        print(f"{what}: worst {worst:.3f} ulp against the truth")
    if kind == "delay" and exact_taps:
        # a wrong filter index is a wrong delay: the exact answer in front of the post gate is the gated input shifted, plus d u,
        # under the bound of tests/test_gpu_lconv.py. Without a post gate that is y itself. With one, y has just been shown to be
        # g (.) z bit for bit, z the shipped plan's result with this plan's spectrum, so the check is made on that z: the gate's own
        # rounding needs no allowance, and a wrong gate index cannot pass yardstick 2.
        expected = gr.delay_expected(u, taps, skip, None, tap=[h[c, lr.delay_shift(c, taps)] for c in range(channels)])
        before_gate = y if g is None else z
        assert np.abs(before_gate.astype(np.float64) - expected).max() <= (k + 1.0) * eb.ulp16(peak.max()), what
    # what the amplitude tests and tools/range_accuracy.py record: z against fp64 with the plan's own spectrum, in the pair's unit
    ref = lr.reference_spectrum(u, spec[0], spec[1], n)[:, :length]
    if rows % 2:
        ref[-channels:].imag = 0.0
    z_re, z_im = lr.pair_planes(z.astype(np.float64), length)
    if data is not None:
        return eb.check(z_re, z_im, ref.real, ref.imag, k, peak=peak, what=what + " (z against fp64 with the plan's spectrum)")
    return float(eb.errors_in_ulps(z_re, z_im, ref.real, ref.imag, peak=peak).max())


@pytest.mark.parametrize("mode", list(gr.GATE_MODES))
@pytest.mark.parametrize("kind", gr.TAP_KINDS)
@pytest.mark.parametrize("length,taps,rows,channels,launch_iters", gr.FUSED_CASES)
def test_fused(tf, length, taps, rows, channels, launch_iters, kind, mode):
    pre, post, _ = gr.GATE_MODES[mode]
    plan = tf.TfftGatedConvPlan(rows, channels, length, taps, 0, pre_gate=pre, post_gate=post, launch_iters=launch_iters)
    assert plan.n == 4096 and plan.kernels == [f"gconv4096::gconv4096_kernel<{_tf_text(pre)}, {_tf_text(post)}>"]
    assert plan.num_launches == 1 and plan.workspace_bytes == 0
    plan.close()
    check_case(tf, length, taps, rows, channels, kind, mode, gr.K_LCONV_FUSED, launch_iters=launch_iters)


@pytest.mark.parametrize("mode", list(gr.GATE_MODES))
@pytest.mark.parametrize("kind", gr.TAP_KINDS)
@pytest.mark.parametrize("n,length,taps,rows,channels,flag", gr.COMPOSED_CASES)
def test_composed(tf, n, length, taps, rows, channels, flag, kind, mode):
    pre, post, _ = gr.GATE_MODES[mode]
    plan = tf.TfftGatedConvPlan(rows, channels, length, taps, 0, pre_gate=pre, post_gate=post, composed=flag)
    kernels = plan.kernels
    assert plan.n == n and kernels[0] == f"gate_copy::pack_kernel<{_tf_text(pre)}>" and kernels[-1] == f"gate_copy::crop_kernel<{_tf_text(post)}>"
    assert plan.num_launches == len(kernels) and plan.workspace_bytes >= (rows + 1) // 2 * channels * n * 4
    plan.close()
    check_case(tf, length, taps, rows, channels, kind, mode, gr.K_LCONV_COMPOSED, composed=flag)


@pytest.mark.parametrize("length,taps,rows,channels,launch_iters,composed", [(520, 7, 9, 3, 4, False), (96, 33, 5, 4, 0, True)])
def test_in_place_equals_out_of_place(tf, length, taps, rows, channels, launch_iters, composed):
    x, h, p, g, skip = gr.case_data(length, taps, rows, channels, "noise", 3, "pre+post+skip")
    a, _ = run_gconv(tf, x, h, p, g, skip, launch_iters, composed)
    b, _ = run_gconv(tf, x, h, p, g, skip, launch_iters, composed, in_place=True)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))


def test_launch_iters_never_changes_results(tf):
    length, taps, rows, channels = 520, 7, 9, 3
    x, h, p, g, skip = gr.case_data(length, taps, rows, channels, "noise", 4, "pre+post+skip")
    a, _ = run_gconv(tf, x, h, p, g, skip, 0)
    for iters in (1, 2, 5, 65535):
        b, _ = run_gconv(tf, x, h, p, g, skip, iters)
        assert np.array_equal(a.view(np.uint16), b.view(np.uint16)), iters


def _plain_run(plan, x, p=None, g=None):
    """contiguous tensors, default strides: [B][C][L] fp16"""
    d_x = _dev(x)
    d_y = torch.zeros_like(d_x)
    plan.exec(d_x, d_y, pre=_dev(p), post=_dev(g))
    torch.cuda.synchronize()
    return d_y.cpu().numpy().reshape(x.shape)


def test_pre_gate_may_alias_the_input(tf):
    """p = x, the same pointer and stride, equals passing a copy: both are only read"""
    length, taps, rows, channels = 520, 7, 3, 3
    x, h, _, g, _ = gr.case_data(length, taps, rows, channels, "noise", 5, "pre+post")
    plan = tf.TfftGatedConvPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True)
    plan.set_taps(_dev(h))
    d_x, d_g = _dev(x), _dev(g)
    d_a, d_b = torch.zeros_like(d_x), torch.zeros_like(d_x)
    plan.exec(d_x, d_a, pre=d_x, post=d_g)
    plan.exec(d_x, d_b, pre=d_x.clone(), post=d_g)
    torch.cuda.synchronize()
    a, b = d_a.cpu().numpy().reshape(x.shape), d_b.cpu().numpy().reshape(x.shape)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
    assert _same_values(a, gr.gated_output(via_lconv_plan(tf, gr.half_product(x, x), h, 0, False), g))
    plan.close()


@pytest.mark.parametrize("composed", [False, True])
def test_refusals_launch_nothing(tf, composed):
    length, taps, rows, channels = 96, 33, 3, 2
    x, h, p, g, _ = gr.case_data(length, taps, rows, channels, "noise", 6, "pre+post")
    both = tf.TfftGatedConvPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True, composed=composed)
    none = tf.TfftGatedConvPlan(rows, channels, length, taps, 0, composed=composed)
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
        (lambda: both.exec(d_x, d_y, pre=None, post=d_g), "pre gate"),                                     # a missing gate
        (lambda: both.exec(d_x, d_y, pre=d_p, post=None), "post gate"),
        (lambda: none.exec(d_x, d_y, pre=d_p), "no pre gate"),                                             # a surplus gate
        (lambda: none.exec(d_x, d_y, post=d_g), "no post gate"),
        (lambda: both.exec(d_x, d_y, pre=d_y, post=d_g), "pre gate and the output overlap"),                # a gate that is the output
        (lambda: both.exec(d_x, d_y, pre=d_p, post=d_y), "post gate and the output overlap"),
        (lambda: both.exec_ptr(d_x.data_ptr(), d_y.data_ptr(), d_p.data_ptr(), d_y.data_ptr() + 16, stream), "post gate and the output overlap"),
        (lambda: both.exec(d_x, d_x, pre=d_x, post=d_g), "pre gate and the output overlap"),                # in place with the gate on the input
        (lambda: both.exec_ptr(d_x.data_ptr(), d_x.data_ptr() + 16, d_p.data_ptr(), d_g.data_ptr(), stream), "input and output overlap"),
        (lambda: both.exec_ptr(d_x.data_ptr(), d_y.data_ptr(), d_p.data_ptr() + 2, d_g.data_ptr(), stream), "16-byte aligned"),
    ]
    for call, needle in refused:
        with pytest.raises(tf.TfftError, match=needle) as e:
            call()
        assert e.value.code == 5, needle                 # TFFT_ERR_ARG
    torch.cuda.synchronize()
    assert bool((d_y == 7.0).all()) and np.array_equal(d_x.cpu().numpy().reshape(x.shape).view(np.uint16), x.view(np.uint16))
    both.close()
    none.close()


def test_taps_and_skip_can_be_replaced(tf):
    length, taps, rows, channels = 2048, 64, 4, 2
    x, h, p, g, skip = gr.case_data(length, taps, rows, channels, "noise", 7, "pre+post+skip")
    u = gr.gated_input(x, p)
    plan = tf.TfftGatedConvPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True)
    delta = np.zeros((channels, taps), np.float16)
    delta[:, 0] = 1.0
    plan.set_taps(_dev(delta))
    first = _plain_run(plan, x, p, g)
    assert _same_values(first, gr.gated_output(via_lconv_plan(tf, u, delta, 0, False), g))
    plan.set_taps(_dev(h), _dev(skip))
    second = _plain_run(plan, x, p, g)
    spec = tuple(t.cpu().numpy() for t in plan.spectrum())
    for c in range(channels):
        want = tf.gconv_spectrum_host(h[c], 4096, skip[c])
        assert np.array_equal(spec[0][c].view(np.uint16), want[0].view(np.uint16)) and np.array_equal(spec[1][c].view(np.uint16), want[1].view(np.uint16))
    assert _same_values(second, gr.gated_output(via_conv_plan(tf, u, spec, 4096), g))
    plan.set_taps(_dev(h))                                    # the skip goes away again
    third = _plain_run(plan, x, p, g)
    assert _same_values(third, gr.gated_output(via_lconv_plan(tf, u, h, 0, False), g)) and not _same_values(third, second)
    plan.close()


@pytest.mark.parametrize("length,taps,rows,channels,composed", [(2048, 2049, 5, 3, False), (1000, 500, 3, 2, True)])
def test_execution_under_stream_capture(tf, length, taps, rows, channels, composed):
    """The fused plan directly, a composed plan after prepare: an execution only launches kernels, so it can be captured into a
    graph and replayed (the pattern of tests/test_gpu_lconv.py: one stream, no parallel branches)."""
    x, h, p, g, skip = gr.case_data(length, taps, rows, channels, "noise", 8, "pre+post+skip")
    plan = tf.TfftGatedConvPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True, composed=composed)
    plan.set_taps(_dev(h), _dev(skip))
    if plan.workspace_bytes:
        plan.prepare()
    else:
        assert plan.kernels == ["gconv4096::gconv4096_kernel<true, true>"]
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
    assert np.array_equal(d_y.cpu().numpy().reshape(x.shape).view(np.uint16), want.view(np.uint16))
    plan.close()


def test_workspace_can_be_handed_in(tf):
    length, taps, rows, channels = 96, 33, 5, 4
    x, h, p, g, skip = gr.case_data(length, taps, rows, channels, "noise", 9, "pre+post+skip")
    plan = tf.TfftGatedConvPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True, composed=True)
    plan.set_taps(_dev(h), _dev(skip))
    need = plan.workspace_bytes
    with pytest.raises(tf.TfftError, match="too small"):
        plan.set_workspace(torch.empty(need - 256, dtype=torch.uint8, device=DEV))
    plan.set_workspace(torch.empty(need, dtype=torch.uint8, device=DEV))
    a = _plain_run(plan, x, p, g)
    plan.close()
    b, _ = run_gconv(tf, x, h, p, g, skip, composed=True)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))


FAMILY = {"gconv4096": "gconv4096_kernel", "pack": "pack_kernel", "crop": "crop_kernel", "conv4096": "conv4096_kernel", "cmul": "cmul_kernel",
          "k4096": "fft4096_kernel", "k4096r": "fft4096r_kernel", "k256": "fft256_kernel", "k256r": "fft256r_kernel", "col": "col",
          "autosort": "stockham::"}


@pytest.mark.parametrize("pre,post", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("length,taps,rows,channels,composed", [c[:4] + (False,) for c in gr.FUSED_CASES[:3]] + [c[1:] for c in gr.COMPOSED_CASES])
def test_describe_is_what_the_plan_launches(tf, length, taps, rows, channels, composed, pre, post):
    words = [w for w in tf.gconv_describe(length, taps, rows, channels, pre_gate=pre, post_gate=post, composed=composed).split() if w != "|"]
    plan = tf.TfftGatedConvPlan(rows, channels, length, taps, 0, pre_gate=pre, post_gate=post, composed=composed)
    kernels = plan.kernels
    assert len(words) == plan.num_launches == len(kernels), (words, kernels)
    for word, kernel in zip(words, kernels):
        assert FAMILY[word.split(":")[0]] in kernel, (words, kernels)
    # the gate words of the description are the template arguments of the kernels at the two ends
    first, last = words[0].split(":"), words[-1].split(":")
    if len(kernels) == 1:
        assert kernels[0].endswith(f"<{_tf_text('pre' in first[-1].split('+') and len(first) == 3)}, {_tf_text('post' in first[-1].split('+') and len(first) == 3)}>")
        assert (len(first) == 3) == (pre or post)
    else:
        assert kernels[0].endswith(f"<{_tf_text(first == ['pack', 'pre'])}>") and kernels[-1].endswith(f"<{_tf_text(last == ['crop', 'post'])}>")
        assert (first == ["pack", "pre"]) == pre and (last == ["crop", "post"]) == post
    plan.close()


def test_every_kernel_of_the_add_on_is_launched(tf):
    """The rule of tests/test_gpu_kernel_matrix.py applied to the add-on: every kernel instantiation in the gfx950 code object of
    libtfft_gconv.so is launched by one of the cases above."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint

    for mode in ("pre", "post", "pre+post", "skip"):                 # (when this test is run on its own)
        for case, composed in ((gr.FUSED_CASES[1], False), (gr.COMPOSED_CASES[0][1:5] + (0,), True)):
            length, taps, rows, channels, iters = case
            x, h, p, g, skip = gr.case_data(length, taps, rows, channels, "noise", 1, mode)
            run_gconv(tf, x, h, p, g, skip, iters, composed)
    mangled = [k for k in isa_lint.split_kernels(isa_lint.disassemble(tf.gconv_lib_path())) if k.startswith("_Z")]
    demangled = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    shipped = {d.strip().removeprefix("void ").split("(")[0] for d in demangled if d.strip()}
    assert shipped == FUSED | COPIES, shipped
    assert shipped <= LAUNCHED, shipped - LAUNCHED


def test_gated_causal_conv(tf):
    length, taps, rows, channels = 520, 7, 3, 3
    x, h, p, g, skip = gr.case_data(length, taps, rows, channels, "noise", 10, "pre+post+skip")
    t_x, t_h, t_p, t_g, t_d = (torch.from_numpy(a).to(DEV) for a in (x, h, p, g, skip))
    for pre, post, d in ((p, g, skip), (p, None, None), (None, g, skip), (None, None, skip)):
        plan = tf.TfftGatedConvPlan(rows, channels, length, taps, 0, pre_gate=pre is not None, post_gate=post is not None)
        plan.set_taps(_dev(h), _dev(d))
        want = _plain_run(plan, x, pre, post)
        plan.close()
        y = tf.gated_causal_conv(t_x, t_h, pre=None if pre is None else t_p, post=None if post is None else t_g, skip=None if d is None else t_d)
        torch.cuda.synchronize()
        assert y.shape == t_x.shape and np.array_equal(y.cpu().numpy().view(np.uint16), want.view(np.uint16))
    # no gates, no skip: causal_conv, bit for bit
    y = tf.gated_causal_conv(t_x, t_h)
    z = tf.causal_conv(t_x, t_h)
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy().view(np.uint16), z.cpu().numpy().view(np.uint16))
    # the same tensors, unchanged: taps and skip are not handed over again; the skip changed in place: they are
    first = tf.gated_causal_conv(t_x, t_h, pre=t_p, post=t_g, skip=t_d)
    again = tf.gated_causal_conv(t_x, t_h, pre=t_p, post=t_g, skip=t_d)
    t_d.zero_()
    without = tf.gated_causal_conv(t_x, t_h, pre=t_p, post=t_g, skip=t_d)
    plain = tf.gated_causal_conv(t_x, t_h, pre=t_p, post=t_g)
    torch.cuda.synchronize()
    assert np.array_equal(first.cpu().numpy().view(np.uint16), again.cpu().numpy().view(np.uint16))
    assert np.array_equal(without.cpu().numpy().view(np.uint16), plain.cpu().numpy().view(np.uint16))
    assert not np.array_equal(first.cpu().numpy().view(np.uint16), plain.cpu().numpy().view(np.uint16))
    tf.gconv_cache_clear()
    tf.lconv_cache_clear()


def test_example_gated_conv_exits_0(tf):
    exe = os.path.join(ROOT, "examples", "example_gated_conv")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
