"""FFT convolution plans on the GPU (tfft_conv_*, include/tfft_conv.h): the fused one-pass N = 4096 kernel and the composed path
(forward plan, cmul, inverse plan) against fp64 numpy, sample by sample (tests/elementwise_bound.py with the constants of
tests/conv_ref.py), the composed path bit for bit against the library's own transforms around the numpy restatement of cmul, the
layout conventions (padded unequal strides, guard zones, untouched input, in place), and the coverage of the add-on's kernels.

Measured on the MI355X with these seeds: fused worst 2.10 ulp (batch 1029, delays), composed worst 2.54 ulp (2^20, delays);
test_fused_is_not_worse_than_composed, same inputs: fused 1.95 ulp, composed 1.75 ulp. Three seeds: profiles/conv_ulps.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest

import conv_ref
import dist_emulate as de
import elementwise_bound as eb

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


def _block(re, im, stride):
    """[batch][n] planes -> one flat fp16 array, signal b as [RE n | IM n] at b * stride"""
    batch, n = re.shape
    flat = np.zeros((batch - 1) * stride + 2 * n, np.float16)
    for b in range(batch):
        flat[b * stride:b * stride + n] = re[b]
        flat[b * stride + n:b * stride + 2 * n] = im[b]
    return flat


def _unblock(flat, batch, n, stride):
    idx = (np.arange(batch) * stride)[:, None] + np.arange(n)[None, :]
    return flat[idx], flat[idx + n]


def run_conv(tf, n, batch, filters, composed, x_re, x_im, h_re, h_im, in_place=False, pad=True):
    """One execution out of place between guard zones with padded, unequal strides (or in place): returns the fp16 planes [batch][n].
    Checks on the way: the guards and the padding between the signals of the output are untouched, the input is bit-identical."""
    in_stride = 2 * n + (8 if pad else 0)
    out_stride = in_stride if in_place else 2 * n + (24 if pad else 0)
    plan = tf.TfftConvPlan(n, batch, filters, 0, in_batch_stride=in_stride, out_batch_stride=out_stride, composed=composed)
    assert plan.num_launches == len(plan.kernels)
    LAUNCHED.update(plan.kernels)
    d_hr, d_hi = torch.from_numpy(h_re.reshape(-1)).to(DEV), torch.from_numpy(h_im.reshape(-1)).to(DEV)
    plan.set_filter(d_hr, d_hi)
    d_hr.fill_(float("nan"))             # the plan owns its image: the caller's planes are free after set_filter
    d_hi.fill_(float("nan"))
    host_in = _block(x_re, x_im, in_stride)
    n_in, n_out = host_in.size, (batch - 1) * out_stride + 2 * n
    d_in = de._guarded(torch, n_in, host_in)
    d_out = d_in if in_place else de._guarded(torch, n_out)
    g = de.GUARD
    plan.exec(d_in[g:], d_in[g + n:], d_out[g:], d_out[g + n:])
    torch.cuda.synchronize()
    assert de._guards_intact(torch, d_out), "output guard zone written"
    out = d_out[g:g + n_out].cpu().numpy()
    if not in_place:
        assert de._guards_intact(torch, d_in)
        de._untouched(d_in[g:g + n_in].cpu().numpy().view(np.int16), host_in.view(np.int16), "input planes")
        if out_stride > 2 * n:
            gaps = out.view(np.int16).copy()[:(batch - 1) * out_stride].reshape(batch - 1, out_stride)[:, 2 * n:] if batch > 1 else np.empty(0, np.int16)
            assert (gaps == de.SENTINEL).all(), "padding between output signals written"
    plan.close()
    return _unblock(out, batch, n, out_stride)


def _case_data(n, batch, filters, kind, seed):
    return conv_ref.case_data(n, batch, filters, kind, seed)


def _check_case(tf, n, batch, filters, composed, kind, seed=1, data=None, exact_filter=True):
    """data: (x_re, x_im, h_re, h_im) in place of the case's own (tests/test_gpu_conv_range.py: the same case at another amplitude);
    exact_filter = False: the delay filters were rounded again, the comparison with numpy.roll is left out"""
    x_re, x_im, h_re, h_im = _case_data(n, batch, filters, kind, seed) if data is None else data
    y_re, y_im = run_conv(tf, n, batch, filters, composed, x_re, x_im, h_re, h_im)
    r_re, r_im = conv_ref.reference(x_re, x_im, h_re, h_im)
    k = conv_ref.K_CONV_COMPOSED if composed or n != 4096 else conv_ref.K_CONV_FUSED
    what = f"conv n={n} batch={batch} filters={filters} {'composed' if composed else 'fused'} {kind}"
    worst = eb.check(y_re, y_im, r_re, r_im, k, what=what)
    print(f"{what}: worst {worst:.3f} ulp")
    if kind == "ones":
        # y = x up to the arithmetic: the same bound against the input itself
        eb.check(y_re, y_im, x_re.astype(np.float64), x_im.astype(np.float64), k, what=what + " (y = x)")
    if kind == "delays" and exact_filter:
        # a wrong filter index or bin map is a wrong roll (times the filter's gain H_0: 1 in this file's cases)
        idx = np.arange(batch) % filters
        gain = h_re[:, 0].astype(np.float64)
        want_re = np.stack([gain[idx[b]] * np.roll(x_re[b].astype(np.float64), conv_ref.delay_shift(idx[b], n)) for b in range(batch)])
        want_im = np.stack([gain[idx[b]] * np.roll(x_im[b].astype(np.float64), conv_ref.delay_shift(idx[b], n)) for b in range(batch)])
        # The binary16 filter is not an exact delay: each component of H_k is rounded to 11 bits, |dH_k| <= 2^-11 |H_k|, rms about
        # 0.4 x that. The inverse transform spreads it over the samples: rel-L2 <= 2^-11 on top of the arithmetic, and per sample
        # sigma = 0.4 * 2^-11 * rms(y) = 0.12 ulp of a peak of 1.41 (y is x rolled: components of rms 0.58), 4.5 sigma over the
        # 2 n values of a signal = 0.55 ulp: one more ulp.
        eb.check(y_re, y_im, want_re, want_im, k + 1.0, rel_l2=eb.REL_L2 + 2.0 ** -11, what=what + " (numpy.roll)")
    return worst


@pytest.mark.parametrize("kind", conv_ref.FILTER_KINDS)
@pytest.mark.parametrize("n,batch,filters,composed", conv_ref.FUSED_CASES)
def test_fused_against_fp64(tf, n, batch, filters, composed, kind):
    plan = tf.TfftConvPlan(n, batch, filters, 0)
    assert plan.kernels == ["conv4096::conv4096_kernel"] and plan.workspace_bytes == 0
    plan.close()
    _check_case(tf, n, batch, filters, composed, kind)


@pytest.mark.parametrize("kind", conv_ref.FILTER_KINDS)
@pytest.mark.parametrize("n,batch,filters,composed", conv_ref.COMPOSED_CASES)
def test_composed_against_fp64(tf, n, batch, filters, composed, kind):
    _check_case(tf, n, batch, filters, composed, kind)


def test_fused_is_not_worse_than_composed(tf):
    """Same inputs, both paths, in one run: worst_fused <= worst_composed + 0.5 ulp (0.5 ulp = the final rounding alone, which the two
    paths take at different values), and the two results agree within the sum of their bounds."""
    n, batch, filters = 4096, 37, 3
    worst = {False: 0.0, True: 0.0}
    for kind in conv_ref.FILTER_KINDS:
        x_re, x_im, h_re, h_im = _case_data(n, batch, filters, kind, 2)
        r_re, r_im = conv_ref.reference(x_re, x_im, h_re, h_im)
        got = {}
        for composed in (False, True):
            got[composed] = run_conv(tf, n, batch, filters, composed, x_re, x_im, h_re, h_im)
            k = conv_ref.K_CONV_COMPOSED if composed else conv_ref.K_CONV_FUSED
            w = eb.check(*got[composed], r_re, r_im, k, what=f"{kind} composed={composed}")
            print(f"{kind}: {'composed' if composed else 'fused'} worst {w:.3f} ulp")
            worst[composed] = max(worst[composed], w)
        peak = np.sqrt(r_re ** 2 + r_im ** 2).max(axis=1)
        d = eb.errors_in_ulps(*got[False], got[True][0].astype(np.float64), got[True][1].astype(np.float64), peak=peak)
        assert d.max() <= conv_ref.K_CONV_FUSED + conv_ref.K_CONV_COMPOSED, (kind, d.max())
    print(f"worst over the five filters: fused {worst[False]:.3f} ulp, composed {worst[True]:.3f} ulp")
    assert worst[False] <= worst[True] + 0.5, worst


@pytest.mark.parametrize("composed", [False, True])
def test_real_filter_convolves_the_planes_independently(tf, composed):
    """A real filter (Hermitian H): the RE plane and the IM plane are two independent real circular convolutions. Each plane is
    judged in the ulp of the largest |y| of the complex signal it travelled in, the unit of the constants."""
    n, batch, filters = 4096, 12, 3
    rng = np.random.default_rng(11)
    x_re, x_im = conv_ref.signals(n, batch, rng)
    h = np.exp(-np.arange(n) / 40.0)[None, :] * rng.standard_normal((filters, n))
    spec = np.fft.fft(h, axis=-1)
    spec /= np.abs(spec).max(axis=1, keepdims=True)
    h_re, h_im = conv_ref.to_half_planes(spec)
    # the binary16 planes are still Hermitian: rounding is symmetric in sign and the two mirror bins round alike
    hh = h_re.astype(np.float64) + 1j * h_im.astype(np.float64)
    assert np.array_equal(hh[:, 1:], np.conj(hh[:, :0:-1]))
    taps = np.fft.ifft(hh, axis=-1).real
    y_re, y_im = run_conv(tf, n, batch, filters, composed, x_re, x_im, h_re, h_im)
    idx = np.arange(batch) % filters

    def circ(x):
        return np.fft.ifft(np.fft.fft(x.astype(np.float64), axis=-1) * np.fft.fft(taps[idx], axis=-1), axis=-1).real

    w_re, w_im = circ(x_re), circ(x_im)
    peak = np.sqrt(w_re ** 2 + w_im ** 2).max(axis=1)
    k = conv_ref.K_CONV_COMPOSED if composed else conv_ref.K_CONV_FUSED
    zero = np.zeros_like(w_re)
    eb.check(y_re, zero, w_re, zero, k, peak=peak, what="RE plane = x_re (*) h")
    eb.check(y_im, zero, w_im, zero, k, peak=peak, what="IM plane = x_im (*) h")


@pytest.mark.parametrize("n,batch,filters,composed", [(4096, 37, 3, False), (4096, 37, 3, True), (2048, 9, 2, True), (1 << 16, 5, 2, True)])
def test_in_place_equals_out_of_place(tf, n, batch, filters, composed):
    x_re, x_im, h_re, h_im = _case_data(n, batch, filters, "allpass", 3)
    a = run_conv(tf, n, batch, filters, composed, x_re, x_im, h_re, h_im)
    b = run_conv(tf, n, batch, filters, composed, x_re, x_im, h_re, h_im, in_place=True)
    assert np.array_equal(a[0].view(np.uint16), b[0].view(np.uint16)) and np.array_equal(a[1].view(np.uint16), b[1].view(np.uint16))


@pytest.mark.parametrize("n,batch,filters", [(4096, 37, 3), (2048, 9, 2), (1 << 16, 5, 2)])
def test_composed_is_forward_cmul_inverse_bit_for_bit(tf, n, batch, filters):
    """The composed path == the library's forward plan -> conv_ref.cmul -> the library's inverse, bit for bit (transposed order between
    the plans where the length has one, the filter permuted by tfft_conv_filter_slot)."""
    x_re, x_im, h_re, h_im = _case_data(n, batch, filters, "decay", 4)
    got_re, got_im = run_conv(tf, n, batch, filters, True, x_re, x_im, h_re, h_im, pad=False)
    w_re, w_im = forward_cmul_inverse(tf, n, batch, filters, x_re, x_im, h_re, h_im)
    assert np.array_equal(got_re.view(np.uint16), w_re.view(np.uint16)) and np.array_equal(got_im.view(np.uint16), w_im.view(np.uint16))


def forward_cmul_inverse(tf, n, batch, filters, x_re, x_im, h_re, h_im):
    """the composed path by its parts: the library's forward plan, conv_ref.cmul on the host, the library's inverse plan: the fp16
    planes [batch][n]"""
    order = "transposed" if tf.transposed_n2(n) else "natural"
    fwd = tf.TfftPlan(n, batch, 0, preserve_input=True, output_order=order)
    inv = tf.TfftPlan(n, batch, 0, input_order=order)
    d_x = torch.from_numpy(_block(x_re, x_im, 2 * n)).to(DEV)
    d_s = torch.empty_like(d_x)
    fwd.exec(d_x, d_x[n:], d_s, d_s[n:])
    torch.cuda.synchronize()
    s_re, s_im = _unblock(d_s.cpu().numpy(), batch, n, 2 * n)
    slot = np.array([tf.conv_filter_slot(n, k, composed=True) for k in range(n)])
    p_re, p_im = np.empty_like(h_re), np.empty_like(h_im)
    p_re[:, slot], p_im[:, slot] = h_re, h_im
    idx = np.arange(batch) % filters
    z_re, z_im = conv_ref.cmul(s_re, s_im, p_re[idx], p_im[idx], n)
    d_z = torch.from_numpy(_block(z_re, z_im, 2 * n)).to(DEV)
    d_y = torch.empty_like(d_z)
    inv.exec_inverse(d_z, d_z[n:], d_y, d_y[n:])
    torch.cuda.synchronize()
    return _unblock(d_y.cpu().numpy(), batch, n, 2 * n)


def test_filter_can_be_replaced_and_exec_needs_one(tf):
    n, batch = 4096, 8
    plan = tf.TfftConvPlan(n, batch, 1, 0)
    x = torch.zeros(batch * 2 * n, dtype=torch.float16, device=DEV)
    y = torch.empty_like(x)
    with pytest.raises(tf.TfftError, match="set_filter"):
        plan.exec(x, x[n:], y, y[n:])
    x_re, x_im, h_re, h_im = _case_data(n, batch, 1, "gauss", 5)
    x.copy_(torch.from_numpy(_block(x_re, x_im, 2 * n)))
    ones = torch.ones(n, dtype=torch.float16, device=DEV)
    plan.set_filter(ones, torch.zeros_like(ones))
    plan.set_filter(torch.from_numpy(h_re.reshape(-1)).to(DEV), torch.from_numpy(h_im.reshape(-1)).to(DEV))
    plan.exec(x, x[n:], y, y[n:])
    torch.cuda.synchronize()
    y_re, y_im = _unblock(y.cpu().numpy(), batch, n, 2 * n)
    eb.check(y_re, y_im, *conv_ref.reference(x_re, x_im, h_re, h_im), conv_ref.K_CONV_FUSED, what="second filter")
    with pytest.raises(tf.TfftError, match="overlap"):
        plan.exec(x, x[n:], x[8:], y[n:])
    # fftconv: the convenience wrapper over the plan cache
    f_re, f_im = tf.fftconv(torch.from_numpy(x_re).to(DEV), torch.from_numpy(x_im).to(DEV), torch.from_numpy(h_re).to(DEV), torch.from_numpy(h_im).to(DEV))
    torch.cuda.synchronize()
    assert np.array_equal(f_re.cpu().numpy().view(np.uint16), y_re.view(np.uint16)) and np.array_equal(f_im.cpu().numpy().view(np.uint16), y_im.view(np.uint16))
    tf.conv_cache_clear()


def test_prepared_plan_runs_under_stream_capture(tf):
    """After prepare (or set_workspace) an execution only launches kernels: it can be captured into a graph and replayed."""
    n, batch, filters = 2048, 9, 2
    x_re, x_im, h_re, h_im = _case_data(n, batch, filters, "allpass", 6)
    plan = tf.TfftConvPlan(n, batch, filters, 0)
    assert plan.workspace_bytes > 0 and "cmul::cmul_kernel" in plan.kernels
    plan.set_filter(torch.from_numpy(h_re.reshape(-1)).to(DEV), torch.from_numpy(h_im.reshape(-1)).to(DEV))
    plan.prepare()
    x = torch.from_numpy(_block(x_re, x_im, 2 * n)).to(DEV)
    y = torch.zeros_like(x)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.exec(x, x[n:], y, y[n:])
    graph.replay()
    torch.cuda.synchronize()
    y_re, y_im = _unblock(y.cpu().numpy(), batch, n, 2 * n)
    eb.check(y_re, y_im, *conv_ref.reference(x_re, x_im, h_re, h_im), conv_ref.K_CONV_COMPOSED, what="captured execution")


def test_every_kernel_of_the_add_on_is_launched(tf):
    """The rule of tests/test_gpu_kernel_matrix.py applied to the add-on: every kernel in the gfx950 code object of libtfft_conv.so
    is launched by one of the cases above."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint

    for case in (conv_ref.FUSED_CASES[1], conv_ref.COMPOSED_CASES[0]):           # (when this test is run on its own)
        n, batch, filters, composed = case
        plan = tf.TfftConvPlan(n, batch, filters, 0, composed=composed)
        LAUNCHED.update(plan.kernels)
        x_re, x_im, h_re, h_im = _case_data(n, batch, filters, "ones", 1)
        run_conv(tf, n, batch, filters, composed, x_re, x_im, h_re, h_im)
    mangled = [k for k in isa_lint.split_kernels(isa_lint.disassemble(tf.conv_lib_path())) if k.startswith("_Z")]
    demangled = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    shipped = {d.strip().removeprefix("void ").split("(")[0] for d in demangled if d.strip()}
    assert shipped == {"conv4096::conv4096_kernel", "cmul::cmul_kernel"}, shipped
    assert shipped <= LAUNCHED, shipped - LAUNCHED


FAMILY = {"conv4096": "conv4096_kernel", "cmul": "cmul_kernel", "k4096": "fft4096_kernel", "k4096r": "fft4096r_kernel", "k256": "fft256_kernel",
          "k256r": "fft256r_kernel", "col": "col", "autosort": "stockham::"}


@pytest.mark.parametrize("n,batch,filters,composed", conv_ref.CASES)
def test_describe_is_what_the_plan_launches(tf, n, batch, filters, composed):
    """tfft_conv_describe restates the planner's choice on the host: one word per launch, and word by word the kernel family that
    tfft_conv_plan_kernels names for a real plan of the same shape."""
    words = [w for w in tf.conv_describe(n, batch, filters, composed=composed).split() if w != "|"]
    plan = tf.TfftConvPlan(n, batch, filters, 0, composed=composed)
    kernels = plan.kernels
    assert len(words) == plan.num_launches == len(kernels), (words, kernels)
    for word, kernel in zip(words, kernels):
        assert FAMILY[word.split(":")[0]] in kernel, (words, kernels)
    plan.close()


def test_example_fft_conv_exits_0(tf):
    exe = os.path.join(ROOT, "examples", "example_fft_conv")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
