"""Causal real convolution plans on the GPU (tfft_lconv_*, include/tfft_lconv.h): the fused one-pass kernel at transform length 4096
and the composed path (pack, tfft_conv_plan, crop). Every case and tap kind is held, on ONE execution between guard zones, to

  1. the shipped tfft_conv_plan on the zero-padded planes with the plan's own spectrum as filter, bit for bit (code that is already
     validated, not the code under test; it also pins lconv4096::filter_slot to conv4096::filter_slot),
  2. fp64 with the same rounded spectrum, sample by sample (tests/elementwise_bound.py, constants of tests/lconv_ref.py),
  3. the true linear convolution of the binary16 taps in fp64, with the allowance for the spectrum's rounding,
  4. the layout: output between guard zones with out_seq_stride = L + 24, input with in_seq_stride = L + 8 whose gaps and guard
     zones hold NaN bit patterns (a read beyond sample L of any sequence poisons the result), guards and gaps back bit for bit.

A fresh compute unit's LDS may read as zero, so a missing or misplaced zero fill shows only from a wave's second item on: the
cases with launch_iters make the waves loop.

Measured on the MI355X over three seeds (profiles/lconv_ulps.txt): fused worst 2.113 ulp (L 2048, K 2049, 3 x 3, delay), composed worst
2.113 ulp (the same case under the flag; 2.048 at 2^16, box)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dist_emulate as de
import elementwise_bound as eb
import lconv_ref as lr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LAUNCHED = set()            # kernels of every plan the cases below executed (test_every_kernel_of_the_add_on_is_launched)


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


def run_lconv(tf, x, h, launch_iters=0, composed=False, in_place=False):
    """One execution out of place between guard zones with padded, unequal strides (or in place): returns (y [B][C][L] fp16, the
    plan's spectrum planes [C][n] fp16). Checks on the way: guards and the gaps between output sequences untouched, the input
    bit-identical. The input's gaps and guards are NaNs."""
    rows, channels, length = x.shape
    taps = h.shape[1]
    in_stride = length + 8
    out_stride = in_stride if in_place else length + 24
    plan = tf.TfftCausalConvPlan(rows, channels, length, taps, 0, in_seq_stride=in_stride, out_seq_stride=out_stride,
                                 launch_iters=launch_iters, composed=composed)
    assert plan.num_launches == len(plan.kernels)
    LAUNCHED.update(plan.kernels)
    d_h = torch.from_numpy(h.reshape(-1)).to(DEV)
    plan.set_taps(d_h)
    d_h.fill_(float("nan"))             # the plan owns its spectrum: the caller's taps are free after set_taps
    spec = tuple(t.cpu().numpy() for t in plan.spectrum())
    host_in, _ = _flat(x, in_stride, de.SENTINEL)
    assert np.isnan(np.int16(de.SENTINEL).view(np.float16))
    n_in = host_in.size
    n_out = (rows * channels - 1) * out_stride + length
    d_in = de._guarded(torch, n_in, host_in.view(np.float16))
    d_out = d_in if in_place else de._guarded(torch, n_out)
    g = de.GUARD
    plan.exec(d_in[g:g + n_in], d_out[g:g + n_out])
    torch.cuda.synchronize()
    assert de._guards_intact(torch, d_out), "output guard zone written"
    out = d_out[g:g + n_out].cpu().numpy().view(np.int16)
    _, idx = _flat(x, out_stride, 0)
    gaps = np.ones(n_out, bool)
    gaps[idx.reshape(-1)] = False
    assert (out[gaps] == de.SENTINEL).all(), "halves between output sequences written"
    if not in_place:
        assert de._guards_intact(torch, d_in)
        de._untouched(d_in[g:g + n_in].cpu().numpy().view(np.int16), host_in, "input sequences")
    plan.close()
    return out[idx].view(np.float16).reshape(rows, channels, length), spec


def via_conv_plan(tf, x, spec, n):
    """what a caller does today: pad and interleave on the host, the shipped TfftConvPlan(n, items, C) with `spec` as its filter,
    crop. Returns [B][C][L] fp16."""
    rows, channels, length = x.shape
    p_re, p_im = lr.pair_planes(x, n)
    items = p_re.shape[0]
    plan = tf.TfftConvPlan(n, items, channels, 0)
    plan.set_filter(torch.from_numpy(spec[0].reshape(-1)).to(DEV), torch.from_numpy(spec[1].reshape(-1)).to(DEV))
    d_x = torch.from_numpy(np.stack((p_re, p_im), axis=1).reshape(-1)).to(DEV)
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


def check_case(tf, length, taps, rows, channels, kind, k, launch_iters=0, composed=False, seed=1, data=None, exact_taps=True):
    """data: (x, h) in place of the case's own (tests/test_gpu_conv_range.py: the same case at another amplitude); exact_taps = False:
    the taps were rounded again, so comparisons 3 and the shifted input are left out"""
    x, h = lr.case_data(length, taps, rows, channels, kind, seed) if data is None else data
    n = lr.plan_length(length, taps, composed)
    path = "fused" if n == 4096 and not composed else "composed"
    what = f"lconv L={length} K={taps} B={rows} C={channels} iters={launch_iters} {path} {kind}"
    y, spec = run_lconv(tf, x, h, launch_iters, composed)
    # 1. the shipped convolution plan on padded planes, bit for bit
    want = via_conv_plan(tf, x, spec, n)
    bad = np.argwhere(y.astype(np.float32) != want.astype(np.float32))
    assert _same_values(y, want), f"{what}: differs from pad -> TfftConvPlan -> crop in {len(bad)} samples, first (b, c, t) = {bad[:3].tolist()}"
    # 2. fp64 with the same rounded spectrum; 3. the true linear convolution
    got_re, got_im = lr.pair_planes(y.astype(np.float64), length)
    true = lr.reference_taps(x, h, n)
    peak = lr.pair_peak(true)
    ref = lr.reference_spectrum(x, spec[0], spec[1], n)[:, :length]
    if rows % 2:
        ref[-channels:].imag = 0.0             # the zero partner has no output: zeros on both sides
        true[-channels:].imag = 0.0
    worst = eb.check(got_re, got_im, ref.real, ref.imag, k, peak=peak, what=what)
    print(f"{what}: worst {worst:.3f} ulp")
    if exact_taps:
        eb.check(got_re, got_im, true.real[:, :length], true.imag[:, :length], k + 1.0, rel_l2=eb.REL_L2 + 2.0 ** -11, peak=peak,
                 what=what + " (true linear convolution)")
    if kind == "delay" and exact_taps:
        # a wrong filter index is a wrong delay: the exact answer is the input shifted (times the tap: 1 in this file's cases)
        for c in range(channels):
            d = lr.delay_shift(c, taps)
            shifted = np.zeros((rows, length))
            shifted[:, d:] = float(h[c, d]) * x[:, c, :length - d].astype(np.float64) if d < length else 0.0
            assert np.abs(y[:, c].astype(np.float64) - shifted).max() <= (k + 1.0) * eb.ulp16(peak.max()), (what, c)
    return worst


@pytest.mark.parametrize("kind", lr.TAP_KINDS)
@pytest.mark.parametrize("length,taps,rows,channels,launch_iters", lr.FUSED_CASES)
def test_fused(tf, length, taps, rows, channels, launch_iters, kind):
    plan = tf.TfftCausalConvPlan(rows, channels, length, taps, 0, launch_iters=launch_iters)
    assert plan.n == 4096 and plan.kernels == ["lconv4096::lconv4096_kernel"] and plan.workspace_bytes == 0
    plan.close()
    check_case(tf, length, taps, rows, channels, kind, lr.K_LCONV_FUSED, launch_iters=launch_iters)


@pytest.mark.parametrize("kind", lr.TAP_KINDS)
@pytest.mark.parametrize("n,length,taps,rows,channels,flag", lr.COMPOSED_CASES)
def test_composed(tf, n, length, taps, rows, channels, flag, kind):
    plan = tf.TfftCausalConvPlan(rows, channels, length, taps, 0, composed=flag)
    assert plan.n == n and plan.kernels[0] == "lconv_copy::pack_kernel" and plan.kernels[-1] == "lconv_copy::crop_kernel"
    assert plan.workspace_bytes >= (rows + 1) // 2 * channels * n * 4
    plan.close()
    check_case(tf, length, taps, rows, channels, kind, lr.K_LCONV_COMPOSED, composed=flag)


@pytest.mark.parametrize("length,taps,rows,channels,launch_iters,composed", [(2048, 2049, 3, 3, 2, False), (520, 7, 9, 3, 4, False),
                                                                            (4096, 4097, 3, 2, 0, False), (2048, 2049, 3, 3, 0, True)])
def test_in_place_equals_out_of_place(tf, length, taps, rows, channels, launch_iters, composed):
    x, h = lr.case_data(length, taps, rows, channels, "noise", 3)
    a, _ = run_lconv(tf, x, h, launch_iters, composed)
    b, _ = run_lconv(tf, x, h, launch_iters, composed, in_place=True)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))


def test_launch_iters_never_changes_results(tf):
    length, taps, rows, channels = 520, 7, 9, 3
    x, h = lr.case_data(length, taps, rows, channels, "decay", 4)
    a, _ = run_lconv(tf, x, h, 0)
    for iters in (1, 2, 5, 65535):
        b, _ = run_lconv(tf, x, h, iters)
        assert np.array_equal(a.view(np.uint16), b.view(np.uint16)), iters


def _plain_run(plan, x):
    d_x = torch.from_numpy(x.reshape(-1)).to(DEV)
    d_y = torch.zeros_like(d_x)
    plan.exec(d_x, d_y)
    torch.cuda.synchronize()
    return d_y.cpu().numpy().reshape(x.shape)


def test_exec_needs_taps_and_taps_can_be_replaced(tf):
    length, taps, rows, channels = 2048, 64, 4, 2
    x, h = lr.case_data(length, taps, rows, channels, "noise", 5)
    plan = tf.TfftCausalConvPlan(rows, channels, length, taps, 0)
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
    assert np.abs(first.astype(np.float64) - x.astype(np.float64)).max() <= lr.K_LCONV_FUSED * eb.ulp16(1.5)     # y = x; |pair| < sqrt 2
    plan.set_taps(torch.from_numpy(h.reshape(-1)).to(DEV))
    second = _plain_run(plan, x)
    spec = tuple(t.cpu().numpy() for t in plan.spectrum())
    assert plan.n == 4096 and _same_values(second, via_conv_plan(tf, x, spec, 4096))
    with pytest.raises(tf.TfftError, match="overlap"):
        plan.exec_ptr(d_x.data_ptr(), d_x.data_ptr() + 16, torch.cuda.current_stream().cuda_stream)      # shifted by one chunk
    plan.close()
    # causal_conv: the convenience wrapper over the plan cache, bit for bit the plan
    t_x, t_h = torch.from_numpy(x).to(DEV), torch.from_numpy(h).to(DEV)
    y = tf.causal_conv(t_x, t_h)
    torch.cuda.synchronize()
    assert y.shape == t_x.shape and np.array_equal(y.cpu().numpy().view(np.uint16), second.view(np.uint16))
    # the same tensor, unchanged: the taps are not handed over again; changed in place: they are
    y2 = tf.causal_conv(t_x, t_h)
    t_h.copy_(torch.from_numpy(delta))
    y3 = tf.causal_conv(t_x, t_h)
    torch.cuda.synchronize()
    assert np.array_equal(y2.cpu().numpy().view(np.uint16), second.view(np.uint16))
    assert np.array_equal(y3.cpu().numpy().view(np.uint16), first.view(np.uint16))
    tf.lconv_cache_clear()


@pytest.mark.parametrize("length,taps,rows,channels,composed", [(2048, 2049, 5, 3, False), (1000, 500, 3, 2, True)])
def test_execution_under_stream_capture(tf, length, taps, rows, channels, composed):
    """The fused plan directly, a composed plan after prepare: an execution only launches kernels, so it can be captured into a
    graph and replayed."""
    x, h = lr.case_data(length, taps, rows, channels, "decay", 6)
    plan = tf.TfftCausalConvPlan(rows, channels, length, taps, 0, composed=composed)
    plan.set_taps(torch.from_numpy(h.reshape(-1)).to(DEV))
    if plan.workspace_bytes:
        plan.prepare()
    else:
        assert plan.kernels == ["lconv4096::lconv4096_kernel"]
    want = _plain_run(plan, x)
    d_x = torch.from_numpy(x.reshape(-1)).to(DEV)
    d_y = torch.zeros_like(d_x)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.exec(d_x, d_y)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(d_y.cpu().numpy().reshape(x.shape).view(np.uint16), want.view(np.uint16))
    plan.close()


def test_workspace_can_be_handed_in(tf):
    length, taps, rows, channels = 96, 33, 5, 4
    x, h = lr.case_data(length, taps, rows, channels, "box", 7)
    plan = tf.TfftCausalConvPlan(rows, channels, length, taps, 0, composed=True)
    plan.set_taps(torch.from_numpy(h.reshape(-1)).to(DEV))
    need = plan.workspace_bytes
    with pytest.raises(tf.TfftError, match="too small"):
        plan.set_workspace(torch.empty(need - 256, dtype=torch.uint8, device=DEV))
    plan.set_workspace(torch.empty(need, dtype=torch.uint8, device=DEV))
    a = _plain_run(plan, x)
    plan.close()
    b, _ = run_lconv(tf, x, h, composed=True)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))


FAMILY = {"lconv4096": "lconv4096_kernel", "pack": "pack_kernel", "crop": "crop_kernel", "conv4096": "conv4096_kernel", "cmul": "cmul_kernel",
          "k4096": "fft4096_kernel", "k4096r": "fft4096r_kernel", "k256": "fft256_kernel", "k256r": "fft256r_kernel", "col": "col",
          "autosort": "stockham::"}


@pytest.mark.parametrize("length,taps,rows,channels,composed",
                         [c[:4] + (False,) for c in lr.FUSED_CASES[:5]] + [c[1:] for c in lr.COMPOSED_CASES])
def test_describe_is_what_the_plan_launches(tf, length, taps, rows, channels, composed):
    words = [w for w in tf.lconv_describe(length, taps, rows, channels, composed=composed).split() if w != "|"]
    plan = tf.TfftCausalConvPlan(rows, channels, length, taps, 0, composed=composed)
    kernels = plan.kernels
    assert len(words) == plan.num_launches == len(kernels), (words, kernels)
    for word, kernel in zip(words, kernels):
        assert FAMILY[word.split(":")[0]] in kernel, (words, kernels)
    plan.close()


def test_every_kernel_of_the_add_on_is_launched(tf):
    """The rule of tests/test_gpu_kernel_matrix.py applied to the add-on: every kernel in the gfx950 code object of
    libtfft_lconv.so is launched by one of the cases above."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint

    for case, composed in ((lr.FUSED_CASES[1], False), (lr.COMPOSED_CASES[0][1:5] + (0,), True)):      # (when this test is run on its own)
        length, taps, rows, channels, iters = case
        x, h = lr.case_data(length, taps, rows, channels, "box", 1)
        run_lconv(tf, x, h, iters, composed)
    mangled = [k for k in isa_lint.split_kernels(isa_lint.disassemble(tf.lconv_lib_path())) if k.startswith("_Z")]
    demangled = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    shipped = {d.strip().removeprefix("void ").split("(")[0] for d in demangled if d.strip()}
    assert shipped == {"lconv4096::lconv4096_kernel", "lconv_copy::pack_kernel", "lconv_copy::crop_kernel"}, shipped
    assert shipped <= LAUNCHED, shipped - LAUNCHED


def test_example_causal_conv_exits_0(tf):
    exe = os.path.join(ROOT, "examples", "example_causal_conv")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
