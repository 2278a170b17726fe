"""Gradient plans of the gated overlap-save causal convolution on the GPU (tfft_gbconv_*, include/tfft_gbconv.h).

Input gradient (gbconv4096::dgrad_kernel<Pre, Post>): every case and mode of tests/gsconv_ref.CASE_MODES and every tap kind, on ONE
execution between guard zones (padded, unequal strides; gaps and guards of every input hold NaN bit patterns; guards, the gaps
between output sequences and the inputs verified untouched):
  1. dx and dpre bit for bit by composition of shipped code: gz = half_product(post, gy) on the host, its windows
     (tests/bconv_ref.py), the shipped TfftConvPlan(4096, items, C) with the conjugate of the plan's own spectrum as filter,
     un-windowed, then half_product(pre, .) and half_product(x, .); without a skip also TfftLongConvGradPlan.input_grad(gz),
  2. the spectrum against tfft_gconv_spectrum_host bit for bit,
  3. fp64 of the same rounded gz with the plan's rounded spectrum: gsconv_ref.post_gate_tolerance with the gate pre (dx) or x
     (dpre) and K_SCONV; against the true correlation with the binary16 taps and skip, K_SCONV + 1.

Tap gradient (wgrad_kernel<Pre, Post>, wreduce_kernel), tests/gbconv_ref.DH_CASE_MODES:
  4. bit for bit the shipped TfftLongConvGradPlan.tap_grad on half_product(pre, x) and half_product(post, gy) built on the host, with
     the same partials; dskip = dh[:, 0] in every bit; within bconv_ref.dh_bound of the direct fp64 sums on those rounded inputs,
  5. determinism, prepare -> capture -> replay, a handed-in workspace, a lone gated sample in a halo counted once.

Life cycle and refusals; torch.autograd through differentiable_gated_long_causal_conv against the plans bit for bit and against
torch.autograd through an fp64 conv1d on the CPU within the tolerances derived in tests/gbconv_ref.py; the C example."""
import os
import subprocess

import numpy as np
import pytest

import bconv_ref as br
import dist_emulate as de
import elementwise_bound as eb
import gbconv_ref as gb
import gsconv_ref as gs
import lconv_ref as lr
import sconv_ref as sr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def kernel_names(pre, post):
    inst = f"<{'true' if pre else 'false'}, {'true' if post else 'false'}>"
    return [f"gbconv4096::dgrad_kernel{inst}", f"gbconv4096::wgrad_kernel{inst}", "gbconv4096::wreduce_kernel"]


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


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _same_values(a, b):
    """equal as VALUES: -0 = +0, and no NaN on either side"""
    a, b = a.astype(np.float32), b.astype(np.float32)
    return not np.isnan(a).any() and not np.isnan(b).any() and np.array_equal(a, b)


def _differs(y, want, what, yardstick):
    bad = np.argwhere(y.astype(np.float32) != want.astype(np.float32))
    return f"{what}: differs from {yardstick} in {len(bad)} samples, first (b, c, t) = {bad[:3].tolist()}"


def _within(y, want, tol, what):
    d = np.abs(y.astype(np.float64) - want)
    assert np.isfinite(y.astype(np.float64)).all(), what
    safe = np.maximum(tol, 1e-300)
    worst = float((d / safe).max())
    at = np.unravel_index(int(np.argmax(d / safe)), d.shape)
    print(f"{what}: {worst:.3f} x the bound")
    assert (d <= tol).all(), f"{what}: {worst:.3f} x the bound at {at}"
    return worst


class Guarded:
    """the inputs of one execution between guard zones, with padded strides; gaps and guards are NaN bit patterns"""

    def __init__(self, arrays):
        self.hosts, self.bufs, self.views = {}, {}, {}
        gd = de.GUARD
        for name, (arr, stride) in arrays.items():
            if arr is None:
                self.views[name] = None
                continue
            self.hosts[name], _ = _flat(arr, stride, de.SENTINEL)
            self.bufs[name] = de._guarded(torch, self.hosts[name].size, self.hosts[name].view(np.float16))
            self.views[name] = self.bufs[name][gd:gd + self.hosts[name].size]

    def check_untouched(self):
        for name in self.hosts:
            assert de._guards_intact(torch, self.bufs[name]), name
            de._untouched(self.views[name].cpu().numpy().view(np.int16), self.hosts[name], name + " sequences")


def _guarded_output(shape, stride):
    rows, channels, length = shape
    n = (rows * channels - 1) * stride + length
    buf = de._guarded(torch, n)
    return buf, buf[de.GUARD:de.GUARD + n], n


def _read_output(buf, view, n, shape, stride, what):
    assert de._guards_intact(torch, buf), what + ": output guard zone written"
    out = view.cpu().numpy().view(np.int16)
    _, idx = _flat(np.zeros(shape, np.float16), stride, 0)
    gaps = np.ones(n, bool)
    gaps[idx.reshape(-1)] = False
    assert (out[gaps] == de.SENTINEL).all(), what + ": halves between output sequences written"
    return out[idx].view(np.float16).reshape(shape)


# ---------------------------------------------------------------------------------------------------------------- input gradient

def run_dgrad(tf, gy, h, post=None, x=None, pre=None, skip=None, launch_iters=0, want_dpre=True):
    """One execution between guard zones: returns (dx, dpre or None, the plan's spectrum planes [C][4096] fp16)."""
    rows, channels, length = gy.shape
    taps = h.shape[1]
    strides = dict(gy=length + 8, post=length + 32, x=length + 16, pre=length + 40, dx=length + 24, dpre=length + 48)
    plan = tf.TfftGatedLongConvGradPlan(rows, channels, length, taps, 0, pre_gate=pre is not None, post_gate=post is not None,
                                        x_seq_stride=strides["x"], pre_seq_stride=strides["pre"], gy_seq_stride=strides["gy"],
                                        post_seq_stride=strides["post"], dx_seq_stride=strides["dx"], dpre_seq_stride=strides["dpre"],
                                        launch_iters=launch_iters)
    assert (plan.halo, plan.hop, plan.segments) == sr.geometry(length, taps)
    assert plan.num_launches == 3 and plan.kernels == kernel_names(pre is not None, post is not None)
    d_h, d_skip = _dev(h), _dev(skip)
    plan.set_taps(d_h, d_skip)
    d_h.fill_(float("nan"))             # the plan owns its spectrum: the caller's taps and skip are free after set_taps
    if d_skip is not None:
        d_skip.fill_(float("nan"))
    spec = tuple(t.cpu().numpy() for t in plan.spectrum())
    assert np.isnan(np.int16(de.SENTINEL).view(np.float16))
    ins = Guarded(dict(gy=(gy, strides["gy"]), post=(post, strides["post"]), x=(x if pre is not None else None, strides["x"]),
                       pre=(pre, strides["pre"])))
    dx_buf, dx_view, dx_n = _guarded_output(gy.shape, strides["dx"])
    with_dpre = pre is not None and want_dpre
    dp_buf, dp_view, dp_n = _guarded_output(gy.shape, strides["dpre"]) if with_dpre else (None, None, 0)
    plan.input_grad(ins.views["gy"], dx_view, post=ins.views["post"], x=ins.views["x"], pre=ins.views["pre"], dpre=dp_view)
    torch.cuda.synchronize()
    dx = _read_output(dx_buf, dx_view, dx_n, gy.shape, strides["dx"], "dx")
    dpre = _read_output(dp_buf, dp_view, dp_n, gy.shape, strides["dpre"], "dpre") if with_dpre else None
    ins.check_untouched()
    plan.close()
    return dx, dpre, spec


def du_via_conv_plan(tf, gz, taps, spec):
    """the gz windows built on the host, the shipped TfftConvPlan(4096, items, C) with conj(spec) as its filter, un-windowed"""
    rows, channels, length = gz.shape
    w_re, w_im = br.dx_windows(gz, taps)
    items = w_re.shape[0]
    c_re, c_im = br.conj_spectrum(*spec)
    plan = tf.TfftConvPlan(sr.N, items, channels, 0)
    plan.set_filter(_dev(c_re), _dev(c_im))
    d_x = _dev(np.stack((w_re, w_im), axis=1))
    d_y = torch.empty_like(d_x)
    plan.exec(d_x, d_x[sr.N:], d_y, d_y[sr.N:])
    torch.cuda.synchronize()
    y = d_y.cpu().numpy().reshape(items, 2, sr.N)
    plan.close()
    return br.dx_unwindow(y[:, 0], y[:, 1], rows, channels, length, taps)


def du_via_grad_plan(tf, gz, h, launch_iters=0):
    """the shipped ungated gradient plan on gz, contiguous: [B][C][L] fp16"""
    rows, channels, length = gz.shape
    plan = tf.TfftLongConvGradPlan(rows, channels, length, h.shape[1], 0, launch_iters=launch_iters)
    plan.set_taps(_dev(h))
    d_g = _dev(gz)
    d_dx = torch.zeros_like(d_g)
    plan.input_grad(d_g, d_dx)
    torch.cuda.synchronize()
    plan.close()
    return d_dx.cpu().numpy().reshape(gz.shape)


def check_dx_case(tf, length, taps, rows, channels, kind, mode, launch_iters=0, seed=1, data=None, exact_taps=True):
    """data: (x, h, pre, post, skip, gy) in place of the case's own (tests/test_gpu_conv_range.py: the same case at another
    amplitude); exact_taps = False: the taps were rounded again, so the comparison with the true correlation is left out. Returns
    the worst error of comparison 3 (rounded spectrum) as a ratio to its tolerance."""
    x, h, pre, post, skip, gy = gb.case_data(length, taps, rows, channels, kind, seed, mode) if data is None else data
    k = gb.K_SCONV
    what = f"gbconv dgrad L={length} K={taps} B={rows} C={channels} iters={launch_iters} {kind} {mode}"
    dx, dpre, spec = run_dgrad(tf, gy, h, post, x, pre, skip, launch_iters)
    gz = gb.gated(gy, post)
    # 2. the restated fp64 spectrum builder with the skip folded in: tfft_gconv_spectrum_host's n = 4096 spectrum, bit for bit
    for c in range(channels):
        want_re, want_im = tf.gconv_spectrum_host(h[c], sr.N, None if skip is None else skip[c])
        assert np.array_equal(_bits(spec[0][c]), _bits(want_re)) and np.array_equal(_bits(spec[1][c]), _bits(want_im)), (what, c)
    # 1. the shipped convolution plan on host-built windows of gz, then the gates on the CPU
    du = du_via_conv_plan(tf, gz, taps, spec)
    yardstick = "pre (.) un-window(TfftConvPlan(windows(post (.) gy), conj(H')))"
    assert _same_values(dx, gb.gated(du, pre)), _differs(dx, gb.gated(du, pre), what, yardstick)
    if pre is not None:
        assert _same_values(dpre, gb.half_product(x, du)), _differs(dpre, gb.half_product(x, du), what + " dpre", yardstick)
    else:
        assert dpre is None
    if skip is None:
        du2 = du_via_grad_plan(tf, gz, h, launch_iters)
        assert _same_values(dx, gb.gated(du2, pre)), _differs(dx, gb.gated(du2, pre), what, "pre (.) TfftLongConvGradPlan(post (.) gy)")
        if pre is not None:
            assert _same_values(dpre, gb.half_product(x, du2)), _differs(dpre, gb.half_product(x, du2), what + " dpre", "x (.) TfftLongConvGradPlan")
    # 3. fp64 with the same rounded gz and the plan's rounded spectrum, K_SCONV; the true correlation, K_SCONV + 1
    true = gb.du_windows_true(gz, h, skip)
    peak = sr.window_peak(true)
    ref = br.dx_reference_spectrum(gz, taps, *br.conj_spectrum(*spec))
    ref_du = br.dx_unwindow(ref.real, ref.imag, rows, channels, length, taps)
    true_du = br.dx_unwindow(true.real, true.imag, rows, channels, length, taps)
    worst = 0.0
    for got, gate, name in ((dx, pre, "dx"), (dpre, x, "dpre")):
        if got is None:
            continue
        if pre is None:
            tol = lambda kk: kk * gb.per_sample(eb.ulp16(peak), rows, channels, length, taps)      # noqa: E731
            scale = 1.0
        else:
            tol = lambda kk: gs.post_gate_tolerance(got, gate, kk, peak, rows, channels, length, taps)      # noqa: E731
            scale = gate.astype(np.float64)
        worst = max(worst, _within(got, scale * ref_du, tol(k), f"{what} {name}"))
        if exact_taps:
            _within(got, scale * true_du, tol(k + 1.0), f"{what} {name} (true correlation)")
    return worst


@pytest.mark.parametrize("kind", gb.TAP_KINDS)
@pytest.mark.parametrize("length,taps,rows,channels,launch_iters,mode", gb.DX_CASE_MODES)
def test_dx_cases(tf, length, taps, rows, channels, launch_iters, mode, kind):
    check_dx_case(tf, length, taps, rows, channels, kind, mode, launch_iters=launch_iters)


def test_ungated_plan_without_skip_is_the_gradient_plan_bit_for_bit(tf):
    length, taps, rows, channels = 6152, 130, 3, 3
    x, h, _, _, _, gy = gb.case_data(length, taps, rows, channels, "noise", 2, "pre")
    dx, dpre, _ = run_dgrad(tf, gy, h)
    assert dpre is None and np.array_equal(_bits(dx), _bits(du_via_grad_plan(tf, gy, h)))
    dh, dskip = run_wgrad(tf, x, None, gy, None, taps)
    assert np.array_equal(_bits(dh), _bits(dh_via_grad_plan(tf, x, gy, taps))) and np.array_equal(_bits(dskip), _bits(dh[:, 0]))


@pytest.mark.parametrize("mode", ["pre", "pre+post+skip"])
def test_dx_without_dpre_has_the_same_bits(tf, mode):
    length, taps, rows, channels = 6152, 130, 3, 3
    x, h, pre, post, skip, gy = gb.case_data(length, taps, rows, channels, "noise", 3, mode)
    a, dpre, _ = run_dgrad(tf, gy, h, post, x, pre, skip)
    b, none, _ = run_dgrad(tf, gy, h, post, x, pre, skip, want_dpre=False)
    assert dpre is not None and none is None and np.array_equal(_bits(a), _bits(b))


def test_dx_launch_iters_never_changes_results(tf):
    length, taps, rows, channels = 6152, 130, 5, 3
    x, h, pre, post, skip, gy = gb.case_data(length, taps, rows, channels, "noise", 4, "pre+post+skip")
    a, ap, _ = run_dgrad(tf, gy, h, post, x, pre, skip, 0)
    for iters in (1, 2, 5, 65535):
        b, bp, _ = run_dgrad(tf, gy, h, post, x, pre, skip, iters)
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(ap), _bits(bp)), iters


def _plain_dx(plan, gy, post=None, x=None, pre=None, dpre=True):
    d = {k: _dev(v) for k, v in (("gy", gy), ("post", post), ("x", x), ("pre", pre))}
    d_dx = torch.zeros_like(d["gy"])
    d_dpre = torch.zeros_like(d["gy"]) if pre is not None and dpre else None
    plan.input_grad(d["gy"], d_dx, post=d["post"], x=d["x"], pre=d["pre"], dpre=d_dpre)
    torch.cuda.synchronize()
    return d_dx.cpu().numpy().reshape(gy.shape), None if d_dpre is None else d_dpre.cpu().numpy().reshape(gy.shape)


def test_dx_needs_taps_and_refusals_launch_nothing(tf):
    length, taps, rows, channels = 4104, 7, 2, 2
    x, h, pre, post, skip, gy = gb.case_data(length, taps, rows, channels, "noise", 8, "pre+post+skip")
    plan = tf.TfftGatedLongConvGradPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True)
    plain = tf.TfftGatedLongConvGradPlan(rows, channels, length, taps, 0)
    total = rows * channels * length
    # one buffer: [spare | gy | post | x | pre | dx | dpre | spare]
    buf = torch.zeros(8 * total, dtype=torch.float16, device=DEV)
    for i, a in enumerate((gy, post, x, pre), start=1):
        buf[i * total:(i + 1) * total] = _dev(a)
    before = _bits(buf.cpu().numpy()).copy()
    at = lambda i: buf.data_ptr() + 2 * i * total      # noqa: E731
    p_gy, p_post, p_x, p_pre, p_dx, p_dpre = (at(i) for i in range(1, 7))
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(tf.TfftError, match="set_taps"):
        plan.input_grad_ptr(p_gy, p_dx, p_post, p_x, p_pre, p_dpre, stream)
    with pytest.raises(tf.TfftError, match="set_taps"):
        plan.spectrum()
    plan.set_taps(_dev(h), _dev(skip))
    plain.set_taps(_dev(h), _dev(skip))
    # each gate-pointer mismatch
    for args, needle in (((p_gy, p_dx, None, p_x, p_pre, p_dpre), "post pointer is null"), ((p_gy, p_dx, p_post, p_x, None, p_dpre), "pre pointer is null"),
                         ((p_gy, p_dx, p_post, None, p_pre, p_dpre), "x pointer is null")):
        with pytest.raises(tf.TfftError, match=needle):
            plan.input_grad_ptr(*args, stream)
    for args, needle in (((p_gy, p_dx, p_post, None, None, None), "no post gate"), ((p_gy, p_dx, None, None, p_pre, None), "no pre gate"),
                         ((p_gy, p_dx, None, p_x, None, None), "no pre gate"), ((p_gy, p_dx, None, None, None, p_dpre), "no pre gate")):
        with pytest.raises(tf.TfftError, match=needle):
            plain.input_grad_ptr(*args, stream)
    # every overlap of an output with an input or with the other output: exact in place; shifted by one chunk; the output's first
    # chunk on the input's last; the output's last chunk on the input's first
    for src in (p_gy, p_post, p_x, p_pre):
        for dst in (src, src + 16, src + 2 * (total - 8), src - 2 * (total - 8)):
            with pytest.raises(tf.TfftError, match="overlap"):
                plan.input_grad_ptr(p_gy, dst, p_post, p_x, p_pre, p_dpre, stream)
            with pytest.raises(tf.TfftError, match="overlap"):
                plan.input_grad_ptr(p_gy, p_dx, p_post, p_x, p_pre, dst, stream)
    for dst in (p_dx, p_dx + 16, p_dx + 2 * (total - 8), p_dx - 2 * (total - 8)):
        if dst == p_dx - 2 * (total - 8):
            continue                                     # that is pre's memory: refused above under another name
        with pytest.raises(tf.TfftError, match="dx and dpre overlap"):
            plan.input_grad_ptr(p_gy, p_dx, p_post, p_x, p_pre, dst, stream)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(buf.cpu().numpy()), before), "a refused call wrote"
    # disjoint parts of one buffer are fine, and inputs may alias each other: x is pre, gy is post
    plan.input_grad_ptr(p_gy, p_dx, p_post, p_x, p_pre, p_dpre, stream)
    torch.cuda.synchronize()
    want_dx, want_dpre = _plain_dx(plan, gy, post, x, pre)
    after = buf.cpu().numpy()
    assert np.array_equal(_bits(after[5 * total:6 * total]), _bits(want_dx.reshape(-1))) and np.array_equal(_bits(after[6 * total:7 * total]), _bits(want_dpre.reshape(-1)))
    assert np.array_equal(_bits(after[:5 * total]), before[:5 * total]) and np.array_equal(_bits(after[7 * total:]), before[7 * total:])
    plan.input_grad_ptr(p_gy, p_dx, p_gy, p_x, p_x, p_dpre, stream)
    torch.cuda.synchronize()
    want_dx, want_dpre = _plain_dx(plan, gy, gy, x, x)
    after = buf.cpu().numpy()
    assert np.array_equal(_bits(after[5 * total:6 * total]), _bits(want_dx.reshape(-1))) and np.array_equal(_bits(after[6 * total:7 * total]), _bits(want_dpre.reshape(-1)))
    plan.close()
    plain.close()


def test_dx_two_executions_under_stream_capture(tf):
    """The input gradient only launches a kernel: two executions in a row on a single stream, the second on the first one's output."""
    length, taps, rows, channels = 8192, 2049, 5, 3
    x, h, pre, post, skip, gy = gb.case_data(length, taps, rows, channels, "noise", 6, "pre+post+skip")
    plan = tf.TfftGatedLongConvGradPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True)
    plan.set_taps(_dev(h), _dev(skip))
    want1, want1p = _plain_dx(plan, gy, post, x, pre)
    want2, want2p = _plain_dx(plan, want1, post, x, pre)
    d = {k: _dev(v) for k, v in (("gy", gy), ("post", post), ("x", x), ("pre", pre))}
    outs = [torch.zeros_like(d["gy"]) for _ in range(4)]
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.input_grad(d["gy"], outs[0], post=d["post"], x=d["x"], pre=d["pre"], dpre=outs[1])
            plan.input_grad(outs[0], outs[2], post=d["post"], x=d["x"], pre=d["pre"], dpre=outs[3])
    graph.replay()
    torch.cuda.synchronize()
    for out, want in zip(outs, (want1, want1p, want2, want2p)):
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want.reshape(-1)))
    plan.close()


# ------------------------------------------------------------------------------------------------------------------ tap gradient

DH_PAD = 64      # floats behind dh and dskip that must stay untouched


def run_wgrad(tf, x, pre, gy, post, taps, partials=0, plan=None):
    """One execution with padded, unequal strides whose gaps and guard zones are NaNs: returns (dh [C][K], dskip [C]) float32. The
    inputs come back bit-identical, the floats behind dh and dskip untouched."""
    rows, channels, length = x.shape
    strides = dict(x=length + 8, pre=length + 24, gy=length + 16, post=length + 32)
    own = plan is None
    if own:
        plan = tf.TfftGatedLongConvGradPlan(rows, channels, length, taps, 0, pre_gate=pre is not None, post_gate=post is not None,
                                            x_seq_stride=strides["x"], pre_seq_stride=strides["pre"], gy_seq_stride=strides["gy"],
                                            post_seq_stride=strides["post"], partials=partials)
    assert plan.partials == br.partials_of(rows, channels, length, taps, partials)
    assert plan.workspace_bytes == channels * plan.partials * (-(-taps // 8) * 8) * 4
    assert plan.kernels == kernel_names(pre is not None, post is not None)
    ins = Guarded(dict(x=(x, strides["x"]), pre=(pre, strides["pre"]), gy=(gy, strides["gy"]), post=(post, strides["post"])))
    d_dh = torch.full((channels * taps + DH_PAD,), float("nan"), dtype=torch.float32, device=DEV)
    d_dskip = torch.full((channels + DH_PAD,), float("nan"), dtype=torch.float32, device=DEV)
    plan.tap_grad(ins.views["x"], ins.views["gy"], d_dh, pre=ins.views["pre"], post=ins.views["post"], dskip=d_dskip)       # no set_taps: not needed
    torch.cuda.synchronize()
    dh, dskip = d_dh.cpu().numpy(), d_dskip.cpu().numpy()
    assert np.isnan(dh[channels * taps:]).all() and np.isnan(dskip[channels:]).all(), "floats behind dh or dskip written"
    ins.check_untouched()
    if own:
        plan.close()
    return dh[:channels * taps].reshape(channels, taps), dskip[:channels]


def dh_via_grad_plan(tf, u, gz, taps, partials=0):
    """the shipped ungated gradient plan on the host-built products, contiguous, with the same cap on the partial sums"""
    rows, channels, length = u.shape
    plan = tf.TfftLongConvGradPlan(rows, channels, length, taps, 0, partials=partials)
    d_dh = torch.zeros(channels * taps, dtype=torch.float32, device=DEV)
    plan.tap_grad(_dev(u), _dev(gz), d_dh)
    torch.cuda.synchronize()
    plan.close()
    return d_dh.cpu().numpy().reshape(channels, taps)


@pytest.mark.parametrize("case", gb.DH_CASE_MODES, ids=lambda c: "-".join(map(str, c)))
def test_dh_cases(tf, case):
    check_dh_case(tf, case)


def check_dh_case(tf, case, data=None):
    """data: (x, pre, post, gy) in place of the case's own (tests/test_gpu_conv_range.py); returns the worst error / bound"""
    length, taps, rows, channels, partials, mode = case
    if data is None:
        x, _, pre, post, _, gy = gb.case_data(length, taps, rows, channels, "noise", 1, mode)
    else:
        x, pre, post, gy = data
    dh, dskip = run_wgrad(tf, x, pre, gy, post, taps, partials)
    assert np.isfinite(dh).all()
    u, gz = gb.gated(x, pre), gb.gated(gy, post)
    # 4. the shipped plan on the products built on the host: identical fp32 bits
    want = dh_via_grad_plan(tf, u, gz, taps, partials)
    bad = np.argwhere(_bits(dh) != _bits(want))
    assert np.array_equal(_bits(dh), _bits(want)), f"wgrad {case}: differs from TfftLongConvGradPlan.tap_grad in {len(bad)} taps, first (c, j) = {bad[:3].tolist()}"
    assert np.array_equal(_bits(dskip), _bits(dh[:, 0])), case
    # ... and the direct sums on those rounded inputs, within bconv's derived bound
    bound = br.dh_bound(br.dh_items(u, gz, taps), channels)
    return _within(dh, br.dh_direct(u, gz, taps), np.broadcast_to(bound[:, None], dh.shape), f"wgrad {case}")


def _plain_dh(plan, x, pre, gy, post):
    d_dh = torch.zeros(plan.channels * plan.taps, dtype=torch.float32, device=DEV)
    d_dskip = torch.zeros(plan.channels, dtype=torch.float32, device=DEV)
    plan.tap_grad(_dev(x), _dev(gy), d_dh, pre=_dev(pre), post=_dev(post), dskip=d_dskip)
    torch.cuda.synchronize()
    return d_dh.cpu().numpy(), d_dskip.cpu().numpy()


def test_dh_is_deterministic_and_replays_from_a_graph(tf):
    """two runs, then prepare -> capture -> replay: the same bits; a handed-in workspace too"""
    length, taps, rows, channels = 8192, 2049, 5, 3
    x, _, pre, post, _, gy = gb.case_data(length, taps, rows, channels, "noise", 2, "pre+post")
    make = lambda: tf.TfftGatedLongConvGradPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True, partials=2)      # noqa: E731
    plan = make()
    first, first_skip = _plain_dh(plan, x, pre, gy, post)
    again, again_skip = _plain_dh(plan, x, pre, gy, post)
    assert np.array_equal(_bits(again), _bits(first)) and np.array_equal(_bits(again_skip), _bits(first_skip))
    plan.close()
    plan = make()
    plan.prepare()
    d = {k: _dev(v) for k, v in (("x", x), ("pre", pre), ("gy", gy), ("post", post))}
    d_dh = torch.zeros(channels * taps, dtype=torch.float32, device=DEV)
    d_dskip = torch.zeros(channels, dtype=torch.float32, device=DEV)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.tap_grad(d["x"], d["gy"], d_dh, pre=d["pre"], post=d["post"], dskip=d_dskip)
    for _ in range(2):
        d_dh.zero_()
        d_dskip.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(d_dh.cpu().numpy()), _bits(first)) and np.array_equal(_bits(d_dskip.cpu().numpy()), _bits(first_skip))
    # a workspace of the caller's: too small is refused, large enough gives the same bits
    need = plan.workspace_bytes
    assert need == channels * 2 * 2056 * 4
    with pytest.raises(tf.TfftError, match="workspace too small"):
        plan.set_workspace(torch.empty(need // 4 - 1, dtype=torch.float32, device=DEV))
    plan.set_workspace(torch.full((need // 4,), float("nan"), dtype=torch.float32, device=DEV))
    assert np.array_equal(_bits(_plain_dh(plan, x, pre, gy, post)[0]), _bits(first))
    # dskip is optional
    d_dh.zero_()
    plan.tap_grad(d["x"], d["gy"], d_dh, pre=d["pre"], post=d["post"])
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d_dh.cpu().numpy()), _bits(first))
    plan.close()


def test_dh_refusals_launch_nothing_and_inputs_may_alias(tf):
    length, taps, rows, channels = 4104, 7, 3, 3
    x, _, pre, post, _, gy = gb.case_data(length, taps, rows, channels, "noise", 3, "pre+post")
    plan = tf.TfftGatedLongConvGradPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True)
    plain = tf.TfftGatedLongConvGradPlan(rows, channels, length, taps, 0)
    d_x, d_gy = _dev(x), _dev(gy)
    # x is pre, gy is post
    want, want_skip = _plain_dh(plan, x, x.copy(), gy, gy.copy())
    d_dh = torch.zeros(channels * taps, dtype=torch.float32, device=DEV)
    d_dskip = torch.zeros(channels, dtype=torch.float32, device=DEV)
    plan.tap_grad(d_x, d_gy, d_dh, pre=d_x, post=d_gy, dskip=d_dskip)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d_dh.cpu().numpy()), _bits(want)) and np.array_equal(_bits(d_dskip.cpu().numpy()), _bits(want_skip))
    before = _bits(d_x.cpu().numpy()).copy()
    stream = torch.cuda.current_stream().cuda_stream
    px, pg, pdh, pds = d_x.data_ptr(), d_gy.data_ptr(), d_dh.data_ptr(), d_dskip.data_ptr()
    for args, needle in (((px, pg, pdh, None, pg, pds), "pre pointer is null"), ((px, pg, pdh, px, None, pds), "post pointer is null")):
        with pytest.raises(tf.TfftError, match=needle):
            plan.tap_grad_ptr(*args, stream)
    for args, needle in (((px, pg, pdh, px, None, pds), "no pre gate"), ((px, pg, pdh, None, pg, pds), "no post gate")):
        with pytest.raises(tf.TfftError, match=needle):
            plain.tap_grad_ptr(*args, stream)
    # dh or dskip inside an input, or on each other: refused, nothing launched
    for bad in (px, px + 2 * (d_x.numel() - 2)):
        with pytest.raises(tf.TfftError, match="overlap"):
            plan.tap_grad_ptr(px, pg, bad, px, pg, pds, stream)
        with pytest.raises(tf.TfftError, match="overlap"):
            plan.tap_grad_ptr(px, pg, pdh, px, pg, bad, stream)
    with pytest.raises(tf.TfftError, match="overlap"):
        plan.tap_grad_ptr(px, pg, pdh, px, pg, pdh, stream)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d_x.cpu().numpy()), before)
    plan.close()
    plain.close()


def test_dh_counts_a_gated_sample_in_a_halo_exactly_once(tf):
    """gy's only non-zero sample sits in the halo of segment 1's window (it belongs to segment 0); the post gate is one everywhere
    but there: dh[j] = post[t0] gy[t0] x[t0 - j], not twice that, and not with the gate of another sample"""
    length, taps, rows, channels = 4104, 7, 1, 1
    halo, hop, segs = sr.geometry(length, taps)
    assert (halo, hop, segs) == (64, 4032, 2)
    x, _ = lr.case_data(length, taps, rows, channels, "noise", 5)
    for t0 in (hop - halo, hop - 10, hop - 1):
        gy = np.zeros_like(x)
        gy[0, 0, t0] = 1.0
        post = np.ones_like(x)
        post[0, 0, t0] = 0.5
        dh, dskip = run_wgrad(tf, x, None, gy, post, taps)
        want = 0.5 * x[0, 0, t0 - np.arange(taps)].astype(np.float64)
        bound = br.dh_bound(br.dh_items(x, gb.gated(gy, post), taps), channels)[0]
        assert bound < 0.02 and np.abs(want).max() > 0.05                    # twice the sample, or an ungated one, would be far outside
        assert np.abs(dh[0] - want).max() <= bound, t0
        assert _bits(dskip)[0] == _bits(dh)[0, 0]


def test_every_kernel_is_launched_by_some_mode_and_names_itself(tf):
    """the four modes of a small plan run both gradients; together they name all nine kernels of the code object as c++filt does"""
    from tensor_fft_amd import gbconv

    length, taps, rows, channels = 4104, 7, 3, 2
    named = set()
    for mode in ("skip", "pre", "post", "pre+post"):
        x, h, pre, post, skip, gy = gb.case_data(length, taps, rows, channels, "noise", 9, mode)
        plan = tf.TfftGatedLongConvGradPlan(rows, channels, length, taps, 0, pre_gate=pre is not None, post_gate=post is not None)
        plan.set_taps(_dev(h), _dev(skip))
        dx, _ = _plain_dx(plan, gy, post, x if pre is not None else None, pre)
        dh, _ = _plain_dh(plan, x, pre, gy, post)
        assert np.isfinite(dx.astype(np.float32)).all() and np.isfinite(dh).all() and np.abs(dh).max() > 0
        assert plan.kernels == kernel_names(pre is not None, post is not None) and plan.num_launches == 3
        named.update(plan.kernels)
        plan.close()
    lib = open(gbconv.gbconv_lib_path(), "rb").read()      # the code object's symbol table is part of the library's bytes
    assert len(named) == 9
    for name in named:
        kernel, _, inst = name.partition("<")
        mangled = f"_ZN10gbconv4096{len(kernel.split('::')[1])}{kernel.split('::')[1]}".encode()
        if inst:
            mangled += b"ILb" + (b"1" if inst.startswith("true") else b"0") + b"ELb" + (b"1" if inst.endswith("true>") else b"0") + b"EE"
        assert mangled in lib, name


# ---------------------------------------------------------------------------------------------------------------------- autograd

@pytest.mark.parametrize("length,taps,rows,channels", gb.AUTOGRAD_CASES)
def test_autograd_matches_the_plans_and_fp64_conv1d(tf, length, taps, rows, channels):
    from tensor_fft_amd import gbconv

    x, h, pre, post, skip, gy = gb.case_data(length, taps, rows, channels, "noise", 1, gb.AUTOGRAD_MODE)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in (("x", x), ("h", h), ("pre", pre), ("post", post), ("skip", skip), ("gy", gy))}
    tf.gbconv_cache_clear()
    tf.gsconv_cache_clear()
    leaves = {k: t[k].clone().requires_grad_() for k in ("x", "h", "pre", "post", "skip")}
    y = tf.differentiable_gated_long_causal_conv(leaves["x"], leaves["h"], pre=leaves["pre"], post=leaves["post"], skip=leaves["skip"])
    assert y.grad_fn is not None
    y.backward(t["gy"])
    torch.cuda.synchronize()
    forward = tf.gated_long_causal_conv(t["x"], t["h"], pre=t["pre"], post=t["post"], skip=t["skip"])
    assert np.array_equal(_bits(y.detach().cpu().numpy()), _bits(forward.cpu().numpy()))
    # the plans' own outputs, bit for bit
    plan = tf.TfftGatedLongConvGradPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True)
    plan.set_taps(t["h"].reshape(-1), t["skip"])
    dx, dpre = _plain_dx(plan, gy, post, x, pre)
    dh, dskip = _plain_dh(plan, x, pre, gy, post)
    dh = dh.reshape(channels, taps)
    plan.close()
    fwd = tf.TfftGatedLongConvPlan(rows, channels, length, taps, 0, pre_gate=True, post_gate=True)
    fwd.set_taps(t["h"].reshape(-1), t["skip"])
    d_dpost = torch.zeros_like(t["x"]).reshape(-1)
    fwd.exec(t["x"].reshape(-1), d_dpost, pre=t["pre"].reshape(-1), post=t["gy"].reshape(-1))
    torch.cuda.synchronize()
    dpost = d_dpost.cpu().numpy().reshape(x.shape)
    fwd.close()
    grads = {k: v.grad.cpu().numpy() for k, v in leaves.items()}
    assert all(grads[k].dtype == np.float16 and grads[k].shape == t[k].shape for k in grads)
    assert np.array_equal(_bits(grads["x"]), _bits(dx)) and np.array_equal(_bits(grads["pre"]), _bits(dpre))
    assert np.array_equal(_bits(grads["post"]), _bits(dpost))
    assert np.array_equal(_bits(grads["h"]), _bits(dh.astype(np.float16))) and np.array_equal(_bits(grads["skip"]), _bits(dskip.astype(np.float16)))
    assert np.array_equal(_bits(dskip), _bits(dh[:, 0]))
    # torch.autograd through an fp64 conv1d of the forward operator on the CPU; tolerances: tests/gbconv_ref.py
    want = gb.autograd_reference(x, h, pre, post, skip, gy)
    gz = gb.gated(gy, post)
    peak = gb.du_peak(gz, h, skip)
    moved = gb.du_input_rounding(gy, h, post, skip)
    what = f"autograd L={length} K={taps}"
    _within(dx, want["dx"], gb.dx_tolerance(dx, pre, gb.K_SCONV + 1.0, peak, rows, channels, length, taps, moved), what + " dx")
    _within(dpre, want["dpre"], gb.dx_tolerance(dpre, x, gb.K_SCONV + 1.0, peak, rows, channels, length, taps, moved), what + " dpre")
    bound = gb.dh_bound_rounded(x, pre, gy, post, taps)[:, None] + gb.dh_input_rounding(x, pre, gy, post, taps)
    _within(dh, want["dh"], bound, what + " dh")
    _within(dskip, want["dskip"], bound[:, 0], what + " dskip")
    _within(dpost, want["dpost"], gb.dpost_tolerance(dpost, x, h, pre, skip, gy), what + " dpost")
    # h.grad and skip.grad are those, rounded once more to the input's dtype: half a binary16 ulp of the value on top
    _within(grads["h"], want["dh"], bound + 0.5 * eb.ulp16(np.abs(want["dh"]) + bound), what + " h.grad")
    _within(grads["skip"], want["dskip"], bound[:, 0] + 0.5 * eb.ulp16(np.abs(want["dskip"]) + bound[:, 0]), what + " skip.grad")
    # a gradient nobody needs is not computed: no plan is created for it
    for need in (("x",), ("pre",), ("h",), ("skip",), ("post",)):
        tf.gbconv_cache_clear()
        tf.gsconv_cache_clear()
        args = {k: t[k].clone().requires_grad_(k in need) for k in ("x", "h", "pre", "post", "skip")}
        tf.differentiable_gated_long_causal_conv(args["x"], args["h"], pre=args["pre"], post=args["post"], skip=args["skip"]).backward(t["gy"])
        torch.cuda.synchronize()
        assert (len(gbconv._dx_plans), len(gbconv._dh_plans)) == (int(need[0] in ("x", "pre")), int(need[0] in ("h", "skip"))), need
        assert [k for k in args if args[k].grad is not None] == list(need)
        assert np.array_equal(_bits(args[need[0]].grad.cpu().numpy()), _bits(grads[need[0]])), need
    tf.gbconv_cache_clear()
    tf.gsconv_cache_clear()


def test_autograd_without_gates_and_skip_is_the_ungated_function_bit_for_bit(tf):
    length, taps, rows, channels = 4104, 7, 3, 3
    x, h = lr.case_data(length, taps, rows, channels, "noise", 1)
    gy = br.grad_signal(rows, channels, length, taps, 1)
    t_gy = torch.from_numpy(gy).to(DEV)
    results = []
    for fn in (tf.differentiable_gated_long_causal_conv, tf.differentiable_long_causal_conv):
        t_x, t_h = torch.from_numpy(x).to(DEV).requires_grad_(), torch.from_numpy(h).to(DEV).requires_grad_()
        y = fn(t_x, t_h)
        y.backward(t_gy)
        torch.cuda.synchronize()
        results.append([a.detach().cpu().numpy() for a in (y, t_x.grad, t_h.grad)])
    for a, b in zip(*results):
        assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))
    for clear in (tf.gbconv_cache_clear, tf.gsconv_cache_clear, tf.bconv_cache_clear, tf.sconv_cache_clear):
        clear()


def test_example_gated_conv_backward_exits_0(tf):
    exe = os.path.join(ROOT, "examples", "example_gated_conv_backward")
    r = subprocess.run([exe, "8192", "2049", "5", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
