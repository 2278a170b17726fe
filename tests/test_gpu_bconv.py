"""Gradient plans of the overlap-save causal convolution on the GPU (tfft_bconv_*, include/tfft_bconv.h).

Input gradient (bconv4096::dgrad_kernel): every case of tests/sconv_ref.py and every tap kind is held, on ONE execution between guard
zones, to what tests/test_gpu_sconv.py holds the forward pass to:
  1. the shipped tfft_conv_plan(4096, items, C) on g windows built on the host (tests/bconv_ref.py) with the plan's own spectrum,
     conjugated, as filter, un-windowed, bit for bit,
  2. fp64 with the same rounded spectrum, every window in ulps of the largest magnitude of its own circular result, K_SCONV,
  3. the true anticausal correlation with the binary16 taps in fp64, K_SCONV + 1,
  4. the layout: padded, unequal strides whose gaps and guard zones hold NaN bit patterns on the input side.

Tap gradient (bconv4096::wgrad_kernel, wreduce_kernel), tests/bconv_ref.DH_CASES:
  5. fp64, tap by tap, within the DERIVED bound of tests/bconv_ref.py (tests/test_bconv_host.py holds the numpy emulation to it),
  6. by composition of shipped code: fp16(Zx / 4096) from the default forward plan at N = 4096 on the host-built x windows, its
     conjugate as one filter per item of tfft_conv_plan(4096, items, items), run on the host-built, halo-zeroed g windows, the RE
     plane's first K samples summed in float32 in the plan's stated order and multiplied by 4096: bit for bit,
  7. determinism, capture and replay, aliased x and g, NaNs around the sequences, a lone sample in a halo counted once.

torch.autograd through differentiable_long_causal_conv: the plans' outputs bit for bit, and an fp64 conv1d reference on the CPU.

Measured on the MI355X over three seeds: profiles/bconv_ulps.txt."""
import os
import subprocess

import numpy as np
import pytest

import bconv_ref as br
import dist_emulate as de
import elementwise_bound as eb
import lconv_ref as lr
import sconv_ref as sr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
KERNELS = ["bconv4096::dgrad_kernel", "bconv4096::wgrad_kernel", "bconv4096::wreduce_kernel"]


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


def _same_values(a, b):
    """equal as VALUES: -0 = +0, and no NaN on either side"""
    a, b = a.astype(np.float32), b.astype(np.float32)
    return not np.isnan(a).any() and not np.isnan(b).any() and np.array_equal(a, b)


def _per_sample(per_window, rows, channels, length, taps):
    """one value per window [items] -> the value of the window that holds each sample of dx: [B][C][L]"""
    full = np.repeat(np.asarray(per_window, np.float64)[:, None], sr.N, axis=1)
    return br.dx_unwindow(full, full, rows, channels, length, taps)


# ---------------------------------------------------------------------------------------------------------------- input gradient

def run_dgrad(tf, g, h, launch_iters=0):
    """One execution between guard zones with padded, unequal strides: returns (dx [B][C][L] fp16, the plan's spectrum planes
    [C][4096] fp16). Guards and the gaps between output sequences untouched, the input bit-identical; its gaps and guards are NaNs."""
    rows, channels, length = g.shape
    taps = h.shape[1]
    in_stride, out_stride = length + 8, length + 24
    plan = tf.TfftLongConvGradPlan(rows, channels, length, taps, 0, g_seq_stride=in_stride, dx_seq_stride=out_stride, launch_iters=launch_iters)
    assert (plan.halo, plan.hop, plan.segments) == sr.geometry(length, taps)
    assert plan.num_launches == 3 and plan.kernels == KERNELS
    d_h = torch.from_numpy(h.reshape(-1)).to(DEV)
    plan.set_taps(d_h)
    d_h.fill_(float("nan"))             # the plan owns its spectrum: the caller's taps are free after set_taps
    spec = tuple(t.cpu().numpy() for t in plan.spectrum())
    host_in, _ = _flat(g, in_stride, de.SENTINEL)
    n_in = host_in.size
    n_out = (rows * channels - 1) * out_stride + length
    d_in = de._guarded(torch, n_in, host_in.view(np.float16))
    d_out = de._guarded(torch, n_out)
    gd = de.GUARD
    plan.input_grad(d_in[gd:gd + n_in], d_out[gd:gd + n_out])
    torch.cuda.synchronize()
    assert de._guards_intact(torch, d_out), "output guard zone written"
    out = d_out[gd:gd + n_out].cpu().numpy().view(np.int16)
    _, idx = _flat(g, out_stride, 0)
    gaps = np.ones(n_out, bool)
    gaps[idx.reshape(-1)] = False
    assert (out[gaps] == de.SENTINEL).all(), "halves between output sequences written"
    assert de._guards_intact(torch, d_in)
    de._untouched(d_in[gd:gd + n_in].cpu().numpy().view(np.int16), host_in, "input sequences")
    plan.close()
    return out[idx].view(np.float16).reshape(rows, channels, length), spec


def dx_via_conv_plan(tf, g, taps, spec):
    """the g windows built on the host, the shipped TfftConvPlan(4096, items, C) with conj(spec) as its filter, un-windowed"""
    rows, channels, length = g.shape
    w_re, w_im = br.dx_windows(g, taps)
    items = w_re.shape[0]
    c_re, c_im = br.conj_spectrum(*spec)
    plan = tf.TfftConvPlan(sr.N, items, channels, 0)
    plan.set_filter(torch.from_numpy(c_re.reshape(-1)).to(DEV), torch.from_numpy(c_im.reshape(-1)).to(DEV))
    d_x = torch.from_numpy(np.stack((w_re, w_im), axis=1).reshape(-1)).to(DEV)
    d_y = torch.empty_like(d_x)
    plan.exec(d_x, d_x[sr.N:], d_y, d_y[sr.N:])
    torch.cuda.synchronize()
    y = d_y.cpu().numpy().reshape(items, 2, sr.N)
    plan.close()
    return br.dx_unwindow(y[:, 0], y[:, 1], rows, channels, length, taps)


def check_dx_case(tf, length, taps, rows, channels, kind, launch_iters=0, seed=1, data=None, exact_taps=True):
    """data: (g, h) in place of the case's own (tests/test_gpu_conv_range.py: the same case at another amplitude); exact_taps = False:
    the taps were rounded again, so comparison 3 and the direct sums are left out"""
    if data is None:
        _, h = lr.case_data(length, taps, rows, channels, kind, seed)
        g = br.grad_signal(rows, channels, length, taps, seed)
    else:
        g, h = data
    k = sr.K_SCONV
    what = f"dgrad L={length} K={taps} B={rows} C={channels} iters={launch_iters} {kind}"
    dx, spec = run_dgrad(tf, g, h, launch_iters)
    # the restated fp64 spectrum builder: tfft_lconv_spectrum_host's n = 4096 spectrum, bit for bit (H, not conjugated)
    for c in range(channels):
        want_re, want_im = tf.lconv_spectrum_host(h[c], sr.N)
        assert np.array_equal(spec[0][c].view(np.uint16), want_re.view(np.uint16)) and np.array_equal(spec[1][c].view(np.uint16), want_im.view(np.uint16)), (what, c)
    # 1. the shipped convolution plan on host-built windows, bit for bit
    want = dx_via_conv_plan(tf, g, taps, spec)
    bad = np.argwhere(dx.astype(np.float32) != want.astype(np.float32))
    assert _same_values(dx, want), f"{what}: differs from windows -> TfftConvPlan -> un-window in {len(bad)} samples, first (b, c, t) = {bad[:3].tolist()}"
    # 2. fp64 with the same rounded spectrum; 3. the true anticausal correlation
    got_re, got_im = (br.dx_kept(p, rows, channels, length, taps) for p in br.dx_windows(dx.astype(np.float64), taps))
    true = br.dx_reference_taps(g, h)
    peak = sr.window_peak(true)
    ref = br.dx_reference_spectrum(g, taps, *br.conj_spectrum(*spec))
    if rows % 2:
        segs = sr.geometry(length, taps)[2]
        ref[-segs * channels:].imag = 0.0
        true[-segs * channels:].imag = 0.0
    ref_k, true_k = br.dx_kept(ref, rows, channels, length, taps), br.dx_kept(true, rows, channels, length, taps)
    worst = eb.check(got_re, got_im, ref_k.real, ref_k.imag, k, peak=peak, what=what)
    print(f"{what}: worst {worst:.3f} ulp")
    if exact_taps:
        eb.check(got_re, got_im, true_k.real, true_k.imag, k + 1.0, rel_l2=eb.REL_L2 + 2.0 ** -11, peak=peak, what=what + " (true correlation)")
        # ... and the same against direct sums, sample by sample
        tol = (k + 1.0) * _per_sample(eb.ulp16(peak), rows, channels, length, taps)
        assert (np.abs(dx.astype(np.float64) - br.dx_direct(g, h)) <= tol).all(), what
    return worst


@pytest.mark.parametrize("kind", lr.TAP_KINDS)
@pytest.mark.parametrize("length,taps,rows,channels,launch_iters", sr.CASES)
def test_dx_cases(tf, length, taps, rows, channels, launch_iters, kind):
    check_dx_case(tf, length, taps, rows, channels, kind, launch_iters=launch_iters)


def test_dx_launch_iters_never_changes_results(tf):
    length, taps, rows, channels = 6152, 130, 5, 3
    _, h = lr.case_data(length, taps, rows, channels, "decay", 4)
    g = br.grad_signal(rows, channels, length, taps, 4)
    a, _ = run_dgrad(tf, g, h, 0)
    for iters in (1, 2, 5, 65535):
        b, _ = run_dgrad(tf, g, h, iters)
        assert np.array_equal(a.view(np.uint16), b.view(np.uint16)), iters


def _plain_dx(plan, g):
    d_g = torch.from_numpy(g.reshape(-1)).to(DEV)
    d_dx = torch.zeros_like(d_g)
    plan.input_grad(d_g, d_dx)
    torch.cuda.synchronize()
    return d_dx.cpu().numpy().reshape(g.shape)


def test_dx_needs_taps_and_overlap_is_refused_and_nothing_is_launched(tf):
    length, taps, rows, channels = 4104, 7, 2, 2
    _, h = lr.case_data(length, taps, rows, channels, "noise", 8)
    g = br.grad_signal(rows, channels, length, taps, 8)
    plan = tf.TfftLongConvGradPlan(rows, channels, length, taps, 0)
    total = rows * channels * length
    buf = torch.zeros(3 * total, dtype=torch.float16, device=DEV)            # g in the middle third
    buf[total:2 * total] = torch.from_numpy(g.reshape(-1)).to(DEV)
    before = buf.cpu().numpy().view(np.uint16).copy()
    with pytest.raises(tf.TfftError, match="set_taps"):
        plan.input_grad(buf[total:2 * total], buf[2 * total:])
    with pytest.raises(tf.TfftError, match="set_taps"):
        plan.spectrum()
    plan.set_taps(torch.from_numpy(h.reshape(-1)).to(DEV))
    stream = torch.cuda.current_stream().cuda_stream
    src = buf.data_ptr() + 2 * total
    # exact in place; shifted by one chunk; dx's first chunk on g's last; dx's last chunk on g's first
    for dst in (src, src + 16, src + 2 * (total - 8), src - 2 * (total - 8)):
        with pytest.raises(tf.TfftError, match="overlap"):
            plan.input_grad_ptr(src, dst, stream)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint16), before)
    # disjoint thirds of one buffer are fine
    plan.input_grad(buf[total:2 * total], buf[2 * total:])
    torch.cuda.synchronize()
    assert np.array_equal(buf[2 * total:].cpu().numpy().view(np.uint16), _plain_dx(plan, g).reshape(-1).view(np.uint16))
    assert np.array_equal(buf[:2 * total].cpu().numpy().view(np.uint16), before[:2 * total])
    plan.close()


def test_dx_two_executions_under_stream_capture(tf):
    """The input gradient only launches a kernel: two executions in a row on a single stream, the second on the first one's output."""
    length, taps, rows, channels = 8192, 2049, 5, 3
    _, h = lr.case_data(length, taps, rows, channels, "decay", 6)
    g = br.grad_signal(rows, channels, length, taps, 6)
    plan = tf.TfftLongConvGradPlan(rows, channels, length, taps, 0)
    plan.set_taps(torch.from_numpy(h.reshape(-1)).to(DEV))
    want1 = _plain_dx(plan, g)
    want2 = _plain_dx(plan, want1)
    d_g = torch.from_numpy(g.reshape(-1)).to(DEV)
    d_1, d_2 = torch.zeros_like(d_g), torch.zeros_like(d_g)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.input_grad(d_g, d_1)
            plan.input_grad(d_1, d_2)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(d_1.cpu().numpy().reshape(g.shape).view(np.uint16), want1.view(np.uint16))
    assert np.array_equal(d_2.cpu().numpy().reshape(g.shape).view(np.uint16), want2.view(np.uint16))
    plan.close()


# ------------------------------------------------------------------------------------------------------------------ tap gradient

DH_PAD = 64      # floats behind dh that must stay untouched


def run_wgrad(tf, x, g, taps, partials=0, plan=None):
    """One execution with padded, unequal strides whose gaps and guard zones are NaNs (every half at or beyond sample L of a sequence
    is one): returns dh [C][K] float32. The inputs come back bit-identical, the floats behind dh untouched."""
    rows, channels, length = x.shape
    x_stride, g_stride = length + 8, length + 16
    own = plan is None
    if own:
        plan = tf.TfftLongConvGradPlan(rows, channels, length, taps, 0, x_seq_stride=x_stride, g_seq_stride=g_stride, partials=partials)
    assert plan.partials == br.partials_of(rows, channels, length, taps, partials)
    assert plan.workspace_bytes == channels * plan.partials * (-(-taps // 8) * 8) * 4
    bufs = []
    for t, stride in ((x, x_stride), (g, g_stride)):
        host, _ = _flat(t, stride, de.SENTINEL)
        bufs.append((de._guarded(torch, host.size, host.view(np.float16)), host))
    d_dh = torch.full((channels * taps + DH_PAD,), float("nan"), dtype=torch.float32, device=DEV)
    gd = de.GUARD
    plan.tap_grad(bufs[0][0][gd:gd + bufs[0][1].size], bufs[1][0][gd:gd + bufs[1][1].size], d_dh)       # no set_taps: not needed
    torch.cuda.synchronize()
    out = d_dh.cpu().numpy()
    assert np.isnan(out[channels * taps:]).all(), "floats behind dh written"
    for d_buf, host in bufs:
        assert de._guards_intact(torch, d_buf)
        de._untouched(d_buf[gd:gd + host.size].cpu().numpy().view(np.int16), host, "input sequences")
    if own:
        plan.close()
    return out[:channels * taps].reshape(channels, taps)


_dh_runs = {}


def dh_case(tf, case):
    """(x, g, dh of the GPU) of a case of DH_CASES, computed once"""
    if case not in _dh_runs:
        length, taps, rows, channels, partials = case
        x, _ = lr.case_data(length, taps, rows, channels, "noise", 1)
        g = br.grad_signal(rows, channels, length, taps, 1)
        _dh_runs[case] = (x, g, run_wgrad(tf, x, g, taps, partials))
    return _dh_runs[case]


@pytest.mark.parametrize("case", br.DH_CASES, ids=lambda c: "-".join(map(str, c)))
def test_dh_against_fp64(tf, case):
    """5. tap by tap within sum over the channel's items of (K_CONV_FUSED + A_SPECTRUM) ulp16(peak_i / 4096) * 4096"""
    check_dh_against_fp64(case, *dh_case(tf, case))


def check_dh_against_fp64(case, x, g, dh):
    """returns the worst error / bound"""
    length, taps, rows, channels, partials = case
    assert np.isfinite(dh).all()
    items = br.dh_items(x, g, taps)
    want, bound = br.dh_from_items(items, channels, taps), br.dh_bound(items, channels)
    direct = br.dh_direct(x, g, taps)
    assert np.abs(want - direct).max() <= 1e-12 * max(np.abs(direct).max(), 1.0)
    ratio = np.abs(dh.astype(np.float64) - direct) / bound[:, None]
    rel = np.sqrt(((dh - direct) ** 2).sum() / (direct ** 2).sum())
    print(f"wgrad {case}: worst error / bound {ratio.max():.3f}, rel-L2 {rel:.2e}")
    c, j = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio.max() <= 1.0, f"wgrad {case}: channel {c}, tap {j}: error {abs(dh[c, j] - direct[c, j]):.3e} > bound {bound[c]:.3e}"
    return float(ratio.max())


def dh_by_composition(tf, x, g, taps, partials):
    """6. shipped code only: the default forward plan's spectrum of the x windows, its conjugate as one filter per item of the shipped
    convolution plan on the halo-zeroed g windows, the RE plane's first K samples, summed in float32 in the plan's order.
    Returns (dh [C][K] float32, the items' RE planes [items][K] float16)."""
    rows, channels, length = x.shape
    halo = sr.geometry(length, taps)[0]
    x_re, x_im = sr.windows(x, taps)
    g_re, g_im = sr.windows(g, taps)
    g_re[:, :halo] = 0
    g_im[:, :halo] = 0
    items = x_re.shape[0]
    fwd = tf.TfftPlan(sr.N, items, 0)
    d_x = torch.from_numpy(np.stack((x_re, x_im), axis=1).reshape(-1)).to(DEV)
    d_s = torch.empty_like(d_x)
    fwd.exec(d_x, d_x[sr.N:], d_s, d_s[sr.N:])
    torch.cuda.synchronize()
    spec = d_s.cpu().numpy().reshape(items, 2, sr.N)                         # fp16(Zx / 4096), natural bin order
    conv = tf.TfftConvPlan(sr.N, items, items, 0)
    conv.set_filter(torch.from_numpy(np.ascontiguousarray(spec[:, 0]).reshape(-1)).to(DEV),
                    torch.from_numpy(np.ascontiguousarray(-spec[:, 1]).reshape(-1)).to(DEV))
    d_g = torch.from_numpy(np.stack((g_re, g_im), axis=1).reshape(-1)).to(DEV)
    d_y = torch.empty_like(d_g)
    conv.exec(d_g, d_g[sr.N:], d_y, d_y[sr.N:])
    torch.cuda.synchronize()
    y_re = d_y.cpu().numpy().reshape(items, 2, sr.N)[:, 0, :taps]
    fwd.close()
    conv.close()
    return br.sum_in_plan_order(y_re, channels, partials), y_re


@pytest.mark.parametrize("case", br.DH_CASES, ids=lambda c: "-".join(map(str, c)))
def test_dh_by_composition_bit_for_bit(tf, case):
    check_dh_by_composition(tf, case, *dh_case(tf, case))


def check_dh_by_composition(tf, case, x, g, dh):
    length, taps, rows, channels, partials = case
    p = br.partials_of(rows, channels, length, taps, partials)
    want, _ = dh_by_composition(tf, x, g, taps, p)
    bad = np.argwhere(dh != want)
    worst = np.abs(dh.astype(np.float64) - want).max()
    print(f"wgrad {case}: P = {p}, {len(bad)} of {dh.size} taps differ from the composition, by at most {worst:.3e}")
    assert _same_values(dh, want), f"wgrad {case}: differs from the composition of shipped plans in {len(bad)} taps, first (c, j) = {bad[:3].tolist()}"


def _plain_dh(plan, x, g):
    d_x, d_g = torch.from_numpy(x.reshape(-1)).to(DEV), torch.from_numpy(g.reshape(-1)).to(DEV)
    d_dh = torch.zeros(plan.channels * plan.taps, dtype=torch.float32, device=DEV)
    plan.tap_grad(d_x, d_g, d_dh)
    torch.cuda.synchronize()
    return d_dh.cpu().numpy()


def test_dh_is_deterministic_and_replays_from_a_graph(tf):
    """two runs, then prepare -> capture -> replay: the same bits; a handed-in workspace too"""
    length, taps, rows, channels = 8192, 2049, 5, 3
    x, _ = lr.case_data(length, taps, rows, channels, "noise", 2)
    g = br.grad_signal(rows, channels, length, taps, 2)
    plan = tf.TfftLongConvGradPlan(rows, channels, length, taps, 0, partials=2)
    first = _plain_dh(plan, x, g)
    assert np.array_equal(_plain_dh(plan, x, g).view(np.uint32), first.view(np.uint32))
    plan.close()
    plan = tf.TfftLongConvGradPlan(rows, channels, length, taps, 0, partials=2)
    plan.prepare()
    d_x, d_g = torch.from_numpy(x.reshape(-1)).to(DEV), torch.from_numpy(g.reshape(-1)).to(DEV)
    d_dh = torch.zeros(channels * taps, dtype=torch.float32, device=DEV)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.tap_grad(d_x, d_g, d_dh)
    for _ in range(2):
        d_dh.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_dh.cpu().numpy().view(np.uint32), first.view(np.uint32))
    # a workspace of the caller's: too small is refused, large enough gives the same bits
    need = plan.workspace_bytes
    assert need == channels * 2 * 2056 * 4
    with pytest.raises(tf.TfftError, match="workspace too small"):
        plan.set_workspace(torch.empty(need // 4 - 1, dtype=torch.float32, device=DEV))
    plan.set_workspace(torch.full((need // 4,), float("nan"), dtype=torch.float32, device=DEV))
    assert np.array_equal(_plain_dh(plan, x, g).view(np.uint32), first.view(np.uint32))
    plan.close()


def test_dh_with_x_and_g_aliased_and_overlap_with_dh_refused(tf):
    length, taps, rows, channels = 4104, 7, 3, 3
    x, _ = lr.case_data(length, taps, rows, channels, "noise", 3)
    plan = tf.TfftLongConvGradPlan(rows, channels, length, taps, 0)
    want = _plain_dh(plan, x, x.copy())
    d_x = torch.from_numpy(x.reshape(-1)).to(DEV)
    d_dh = torch.zeros(channels * taps, dtype=torch.float32, device=DEV)
    plan.tap_grad(d_x, d_x, d_dh)
    torch.cuda.synchronize()
    assert np.array_equal(d_dh.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # tap 0 of an autocorrelation is the energy
    energy = (x.astype(np.float64) ** 2).sum(axis=(0, 2))
    assert np.abs(want.reshape(channels, taps)[:, 0] - energy).max() <= br.dh_bound(br.dh_items(x, x, taps), channels).max()
    # dh inside x or g: refused, nothing launched
    before = d_x.cpu().numpy().view(np.uint16).copy()
    stream = torch.cuda.current_stream().cuda_stream
    for dh_ptr in (d_x.data_ptr(), d_x.data_ptr() + 2 * (d_x.numel() - 2)):
        with pytest.raises(tf.TfftError, match="overlaps"):
            plan.tap_grad_ptr(d_x.data_ptr(), d_x.data_ptr(), dh_ptr, stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_x.cpu().numpy().view(np.uint16), before)
    plan.close()


def test_dh_counts_a_sample_in_a_halo_exactly_once(tf):
    """g's only non-zero sample sits in the halo of segment 1's window (it belongs to segment 0, whose window holds it behind its
    own halo): dh[j] = g[t0] x[t0 - j], not twice that"""
    length, taps, rows, channels = 4104, 7, 1, 1
    halo, hop, segs = sr.geometry(length, taps)
    assert (halo, hop, segs) == (64, 4032, 2)
    x, _ = lr.case_data(length, taps, rows, channels, "noise", 5)
    for t0 in (hop - halo, hop - 10, hop - 1):
        g = np.zeros_like(x)
        g[0, 0, t0] = 1.0
        dh = run_wgrad(tf, x, g, taps)
        want = x[0, 0, t0 - np.arange(taps)].astype(np.float64)
        bound = br.dh_bound(br.dh_items(x, g, taps), channels)[0]
        assert bound < 0.02 and np.abs(want).max() > 0.1                    # twice the sample would be far outside
        assert np.abs(dh[0] - want).max() <= bound, t0


# ---------------------------------------------------------------------------------------------------------------------- autograd

@pytest.mark.parametrize("length,taps,rows,channels", [(4104, 7, 3, 3), (2048, 2049, 3, 3)])
def test_autograd_matches_the_plans_and_fp64_conv1d(tf, length, taps, rows, channels):
    from tensor_fft_amd import bconv

    x, h = lr.case_data(length, taps, rows, channels, "noise", 1)
    g = br.grad_signal(rows, channels, length, taps, 1)
    t_x, t_h, t_g = (torch.from_numpy(a).to(DEV) for a in (x, h, g))
    tf.bconv_cache_clear()
    tf.sconv_cache_clear()
    t_x.requires_grad_()
    t_h.requires_grad_()
    y = tf.differentiable_long_causal_conv(t_x, t_h)
    assert y.grad_fn is not None
    y.backward(t_g)
    torch.cuda.synchronize()
    assert np.array_equal(y.detach().cpu().numpy().view(np.uint16), tf.long_causal_conv(t_x.detach(), t_h.detach()).cpu().numpy().view(np.uint16))
    # the plans' own outputs, bit for bit
    plan = tf.TfftLongConvGradPlan(rows, channels, length, taps, 0)
    plan.set_taps(t_h.detach().reshape(-1))
    dx = _plain_dx(plan, g)
    dh = _plain_dh(plan, x, g).reshape(channels, taps)
    plan.close()
    assert t_x.grad.dtype == torch.float16 and t_h.grad.dtype == t_h.dtype and t_h.grad.shape == t_h.shape
    assert np.array_equal(t_x.grad.cpu().numpy().view(np.uint16), dx.view(np.uint16))
    assert np.array_equal(t_h.grad.cpu().numpy().view(np.uint16), dh.astype(np.float16).view(np.uint16))
    # torch.autograd through an fp64 conv1d on the CPU
    r_x = torch.from_numpy(x.astype(np.float64)).requires_grad_()
    r_h = torch.from_numpy(h.astype(np.float64)).requires_grad_()
    r_y = torch.nn.functional.conv1d(torch.nn.functional.pad(r_x, (taps - 1, 0)), r_h.flip(-1).unsqueeze(1), groups=channels)
    r_y.backward(torch.from_numpy(g.astype(np.float64)))
    tol_x = (sr.K_SCONV + 1.0) * _per_sample(eb.ulp16(sr.window_peak(br.dx_reference_taps(g, h))), rows, channels, length, taps)
    assert (np.abs(dx.astype(np.float64) - r_x.grad.numpy()) <= tol_x).all()
    bound = br.dh_bound(br.dh_items(x, g, taps), channels)[:, None]
    want_h = r_h.grad.numpy()
    assert (np.abs(dh.astype(np.float64) - want_h) <= bound).all()
    # h.grad is that, rounded once more to h.dtype: half a binary16 ulp of the value on top
    cast = 0.5 * eb.ulp16(np.abs(want_h) + bound)
    assert (np.abs(t_h.grad.cpu().numpy().astype(np.float64) - want_h) <= bound + cast).all()
    # a gradient nobody needs is not computed: no plan is created for it
    for need_x, need_h in ((True, False), (False, True)):
        tf.bconv_cache_clear()
        a = t_x.detach().clone().requires_grad_(need_x)
        b = t_h.detach().clone().requires_grad_(need_h)
        tf.differentiable_long_causal_conv(a, b).backward(t_g)
        torch.cuda.synchronize()
        assert (len(bconv._dx_plans), len(bconv._dh_plans)) == (int(need_x), int(need_h))
        assert (a.grad is not None, b.grad is not None) == (need_x, need_h)
        if need_x:
            assert np.array_equal(a.grad.cpu().numpy().view(np.uint16), dx.view(np.uint16))
        if need_h:
            assert np.array_equal(b.grad.cpu().numpy().view(np.uint16), dh.astype(np.float16).view(np.uint16))
    tf.bconv_cache_clear()
    tf.sconv_cache_clear()


def test_example_conv_backward_exits_0(tf):
    exe = os.path.join(ROOT, "examples", "example_conv_backward")
    r = subprocess.run([exe, "8192", "2049", "5", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
