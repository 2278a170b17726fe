"""Short-frame ISTFT plans on the GPU (tfft_istftn_*, include/tfft_istftn.h): half spectra of hopped frames of 512, 1024 and 2048
samples back to real signals, by a one-pass C2R of every frame into a workspace and a windowed overlap-add in a fixed order. Every
case runs ONCE between guard zones (module-scoped cache) with a caller's workspace, and is held to

  1. frames: the workspace equals, bit for bit, the shipped TfftPlan(n, items, 0).exec_inverse (the default plan of n, one launch of
     fft256r_kernel) on tests/istftn_ref.merge_items of the input, uploaded from the host (code that is already validated, not the
     code under test; it pins the pairing of frames 2b and 2b + 1, the self-paired last frame of an odd total, the gain and the merge),
  2. output: y equals, bit for bit, tests/istftn_ref.ola of those same workspace frames as read back, with and without raw_sum,
  3. the layout: input with in_frame_stride = 2 h + 16 whose halves beyond bin n / 2, gaps, guards and the IM of bins 0 and n / 2 hold
     NaN bit patterns (a read of any of them poisons the result) and which is bit-identical afterwards; output with out_sig_stride =
     L + 64 prefilled with NaN patterns, whose gaps and guards come back bit for bit; a NaN-prefilled workspace of (R F + 1) n halves
     whose tail (the slot behind a self-paired frame) and guards come back bit for bit,
  4. fp64 on two Hann shapes per n, per signal.

A fresh compute unit's LDS may read as zero, so a slot of the image the merge misses shows only from a wave's second group on
(tests/test_gpu_sconv.py has the note): the cases with launch_iters make the waves loop.

Measured on the MI355X (seed 1), worst signal of the two accuracy shapes, rel-L2 against the fp64 ISTFT of the same binary16 spectra
and for istft(stft(x)) against x: 2.85e-04 and 4.12e-04 (n = 512), 2.84e-04 and 4.02e-04 (1024), 2.80e-04 and 4.02e-04 (2048)
(DESIGN.md 3.20)."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import dist_emulate as de
import istftn_ref as inr
import stftn_ref as sn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
K_C2R = 1.5e-3                     # what tests/test_gpu_rfft.py asserts per pair for the C2R arithmetic: rel-L2 against fp64
K_FWD = 1.5e-3 + 2.0 ** -10        # what tests/test_gpu_stftn.py grants the forward transform against fp64 of the unrounded products
LENGTHS = inr.LENGTHS
CASES = [(n,) + c for n in LENGTHS for c in inr.cases(n)]
HUGE_HOP_CASES = [(n,) + c for n in LENGTHS for c in inr.huge_hop_cases(n)]


def _in_stride(n):
    return 2 * sn.pitch(n) + 16


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    return tensor_fft_amd


def _flat_spectra(n, re, im):
    """[G][n / 2 + 1] x 2 -> one flat int16 array, frame g: RE at g * in_stride, IM h halves on; NaN sentinels in everything that must
    not be read: the halves beyond bin n / 2, the gaps, the IM of bins 0 and n / 2"""
    total, bins, pitch, stride = re.shape[0], sn.bins(n), sn.pitch(n), _in_stride(n)
    flat = np.full((total - 1) * stride + 2 * pitch, de.SENTINEL, dtype=np.int16)
    idx = (np.arange(total) * stride)[:, None] + np.arange(bins)[None, :]
    flat[idx] = re.view(np.int16)
    poisoned = im.view(np.int16).copy()
    poisoned[:, 0] = poisoned[:, n // 2] = de.SENTINEL
    flat[idx + pitch] = poisoned
    return flat


def run_istftn(tf, n, re, im, w, rows, length, hop, pad, launch_iters=0, raw=False):
    """One execution between guard zones with padded strides and a caller's workspace: returns (frames [R * F][n], y [R][L]) as int16
    bit patterns. Checks on the way: guards, gaps and the workspace behind the frames untouched, the input bit-identical, two launches
    of the two kernels. The window tensor is poisoned after set_window: the plan owns its copy."""
    out_stride = length + 64
    plan = tf.TfftShortIstftPlan(n, rows, length, hop, pad, 0, in_frame_stride=_in_stride(n), out_sig_stride=out_stride, launch_iters=launch_iters,
                                 raw_sum=raw)
    total = rows * plan.frames
    assert plan.frames == inr.geometry(n, length, hop, pad) and re.shape == im.shape == (total, sn.bins(n))
    assert plan.num_launches == 2 and plan.kernels == [f"istft256r::frames_kernel<{n // 256}>", "olan::ola_kernel"]
    assert plan.workspace_bytes() == total * n * 2
    d_w = torch.from_numpy(w.copy()).to(DEV)
    plan.set_window(d_w)
    torch.cuda.synchronize()
    d_w.fill_(float("nan"))
    host_in = _flat_spectra(n, re, im)
    assert np.isnan(np.int16(de.SENTINEL).view(np.float16))
    n_in, n_out, n_ws = host_in.size, (rows - 1) * out_stride + length, (total + 1) * n
    d_in = de._guarded(torch, n_in, host_in.view(np.float16))
    d_out = de._guarded(torch, n_out)
    d_ws = de._guarded(torch, n_ws)
    g = de.GUARD
    plan.set_workspace(d_ws[g:g + n_ws])
    body = d_in[g:g + n_in]
    plan.exec(body, body[sn.pitch(n):], d_out[g:g + n_out])
    torch.cuda.synchronize()
    assert de._guards_intact(torch, d_out), "output guard zone written"
    assert de._guards_intact(torch, d_ws), "workspace guard zone written"
    assert de._guards_intact(torch, d_in)
    de._untouched(body.cpu().numpy().view(np.int16), host_in, "input spectra")
    ws = d_ws[g:g + n_ws].cpu().numpy().view(np.int16)
    assert (ws[total * n:] == de.SENTINEL).all(), "workspace written beyond R F * n halves"
    out = d_out[g:g + n_out].cpu().numpy().view(np.int16)
    idx = (np.arange(rows) * out_stride)[:, None] + np.arange(length)[None, :]
    written = np.zeros(n_out, bool)
    written[idx.reshape(-1)] = True
    assert (out[~written] == de.SENTINEL).all(), "gaps between the output signals written"
    plan.close()
    return ws[:total * n].reshape(total, n).copy(), out[idx]


def via_inverse_plan(tf, n, zr, zi, total):
    """the shipped TfftPlan(n, items, 0), the default plan of n, exec_inverse on Z' [items][n] x 2 uploaded from the host: the frames
    [total][n] as int16 bit patterns (RE result = frame 2b, IM result = frame 2b + 1)"""
    items = zr.shape[0]
    plan = tf.TfftPlan(n, items, 0)
    assert plan.num_launches == 1 and "fft256r_kernel" in plan.kernels[0], plan.kernels
    d_z = torch.from_numpy(np.ascontiguousarray(np.stack([zr, zi], axis=1)).reshape(-1)).to(DEV)
    d_v = torch.zeros(items * 2 * n, dtype=torch.float16, device=DEV)
    plan.exec_inverse(d_z, d_z[n:], d_v, d_v[n:])
    torch.cuda.synchronize()
    v = d_v.cpu().numpy().view(np.int16).reshape(2 * items, n)[:total].copy()
    plan.close()
    return v


_inputs, _results, _wanted = {}, {}, {}


def inputs(n, rows, length, hop, pad, window):
    """(x, w, re, im) of one shape, computed once per module and left unchanged"""
    key = (n, rows, length, hop, pad, window)
    if key not in _inputs:
        x, w = sn.case_data(n, rows, length, window=window)
        # (one frame per signal: the frame does not depend on the hop, and numpy's int64 framing does not carry a hop of 2^63)
        _inputs[key] = (x, w) + inr.spectra16(x, w, hop if inr.geometry(n, length, hop, pad) > 1 else min(hop, length + 2 * pad), pad)
        for a in _inputs[key]:
            a.setflags(write=False)
    return _inputs[key]


def result(tf, n, rows, length, hop, pad, iters, window, raw=False):
    """(frames, y) of one case, computed once per module"""
    key = (n, rows, length, hop, pad, iters, window, raw)
    if key not in _results:
        _, w, re, im = inputs(n, rows, length, hop, pad, window)
        _results[key] = run_istftn(tf, n, re, im, w, rows, length, hop, pad, iters, raw)
    return _results[key]


def wanted_frames(tf, n, rows, length, hop, pad, window):
    """the reference of comparison 1, computed once per shape and left unchanged"""
    key = (n, rows, length, hop, pad, window)
    if key not in _wanted:
        _, _, re, im = inputs(n, rows, length, hop, pad, window)
        zr, zi = inr.merge_items(re, im, n)
        _wanted[key] = via_inverse_plan(tf, n, zr, zi, re.shape[0])
        _wanted[key].setflags(write=False)
    return _wanted[key]


def _assert_bits(what, got, want, names=("frame", "sample")):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: differs in {len(bad)} halves, first ({names[0]}, {names[1]}) = {bad[:3].tolist()}"


def _check_case(tf, n, rows, length, hop, pad, iters, window, raw=False):
    _, w, _, _ = inputs(n, rows, length, hop, pad, window)
    frames, y = result(tf, n, rows, length, hop, pad, iters, window, raw)
    what = f"istft n={n} R={rows} L={length} hop={hop} pad={pad} iters={iters} {window}{' raw' if raw else ''}"
    assert not np.isnan(frames.view(np.float16)).any(), what + ": a NaN of the input's padding reached the frames"
    _assert_bits(what + ", frames against merge_items -> TfftPlan.exec_inverse", frames, wanted_frames(tf, n, rows, length, hop, pad, window))
    want_y = inr.ola(frames.view(np.float16), w, n, rows, length, hop, pad, raw=raw).view(np.int16)
    _assert_bits(what + ", output against istftn_ref.ola of the workspace frames", y, want_y, ("signal", "sample"))
    return frames, y


@pytest.mark.parametrize("n,rows,length,hop,pad,iters,window", CASES)
def test_frames_and_output_bit_for_bit(tf, n, rows, length, hop, pad, iters, window):
    _, w, _, _ = inputs(n, rows, length, hop, pad, window)
    _, y = _check_case(tf, n, rows, length, hop, pad, iters, window)
    bare = inr.envelope(w, n, length, hop, pad) == 0
    assert (y[:, bare] == 0).all(), "a sample no frame covers must be +0"
    assert np.isfinite(y.view(np.float16)).all()


@pytest.mark.parametrize("n,rows,length,hop,pad,iters,window", HUGE_HOP_CASES)
def test_one_frame_plans_carry_any_hop(tf, n, rows, length, hop, pad, iters, window):
    """A plan with one frame per signal may have any hop that 64 bits hold: the samples behind the frame are +0, nothing outside the
    window buffer or the workspace is read (NaN guards around both would poison the sums) and the guards of the output are intact
    (run_istftn asserts them)."""
    assert inr.geometry(n, length, hop, pad) == 1 and hop + length + pad >= 1 << 63      # beyond what signed 64-bit arithmetic on hop holds
    for raw in (False, True):
        _, y = _check_case(tf, n, rows, length, hop, pad, iters, window, raw=raw)
        assert (y[:, n - pad:] == 0).all(), "a sample behind the one frame must be +0"
        assert np.isfinite(y.view(np.float16)).all() and (y[:, :n - pad] != 0).any()


@pytest.mark.parametrize("n,rows,length,hop,pad,iters,window", CASES)
def test_raw_sum_bit_for_bit(tf, n, rows, length, hop, pad, iters, window):
    _, y = _check_case(tf, n, rows, length, hop, pad, iters, window, raw=True)
    _, divided = result(tf, n, rows, length, hop, pad, iters, window)
    assert (y != divided).any()          # the flag does something


@pytest.mark.parametrize("iters", [0, 1, 3, 65535])
@pytest.mark.parametrize("n", LENGTHS)
def test_launch_iters_never_changes_a_bit(tf, n, iters):
    rows, length, hop, pad = sn.looping_case(n)
    _check_case(tf, n, rows, length, hop, pad, iters, "random")


def _accuracy_bound(w, n, length, hop, pad):
    """e_y = sum w e_f / sum w^2; Cauchy-Schwarz with sum_f |u_f|^2 <= env_max |x|^2 gives |e_y| <= K sqrt(2 env_max / env_min) |x|,
    K per pair and the factor 2 for a pair's weaker frame, plus 2^-11 for the rounding of the output"""
    env = inr.envelope(w, n, length, hop, pad)
    assert env.min() >= 1.25 * (1 - 2.0 ** -10) and env.max() <= 1.5 * (1 + 2.0 ** -10)
    return K_C2R * np.sqrt(2 * env.max() / env.min()) + 2.0 ** -11


@pytest.mark.parametrize("n", LENGTHS)
def test_accuracy_against_fp64(tf, n):
    """Per signal, rel-L2 against the fp64 ISTFT of the same binary16 spectra, Hann window, shapes (3, 2n, n / 4, n / 2) and
    (4, 3n, n / 4, n / 2); bound K sqrt(2 env_max / env_min) + 2^-11 = 2.81e-03 (derived in _accuracy_bound). And
    istft(stft(x, n_fft=n), n_fft=n) against x itself, the same bound plus the forward allowance of tests/test_gpu_stftn.py
    (1.5e-3 + 2^-10): 5.29e-03. Measured on the MI355X, worst signal: 2.72e-04 and 4.12e-04 (n = 512, 3 x 1024), 2.85e-04 and 4.11e-04
    (512, 4 x 1536), 2.76e-04 and 3.97e-04 (1024, 3 x 2048), 2.84e-04 and 4.02e-04 (1024, 4 x 3072), 2.74e-04 and 4.01e-04 (2048,
    3 x 4096), 2.80e-04 and 4.02e-04 (2048, 4 x 6144)."""
    for rows, length, hop, pad in inr.accuracy_shapes(n):
        x, w, re, im = inputs(n, rows, length, hop, pad, "hann")
        _, y = result(tf, n, rows, length, hop, pad, 0, "hann")
        bound = _accuracy_bound(w, n, length, hop, pad)
        want = inr.istft64(re, im, w, rows, length, hop, pad)
        e_inv = inr.rel_l2(y.view(np.float16), want).max()
        d_w = torch.from_numpy(w.copy()).to(DEV)
        g_re, g_im = tf.stft(torch.from_numpy(x.copy()).to(DEV), d_w, hop, center=True, n_fft=n)
        back = tf.istft(g_re, g_im, d_w, hop, length, center=True, n_fft=n).cpu().numpy()
        e_trip = inr.rel_l2(back, x).max()
        print(f"istft n={n} R={rows} L={length} hop={hop}: worst signal rel-L2 {e_inv:.2e} against fp64 ISTFT of the binary16 spectra (bound "
              f"{bound:.2e}), istft(stft(x)) against x {e_trip:.2e} (bound {bound + K_FWD:.2e})")
        tf.stftn_cache_clear()
        tf.istftn_cache_clear()
        assert e_inv <= bound and e_trip <= bound + K_FWD


def _stft_layout(n, re, im, rows):
    """[R * F][n / 2 + 1] x 2 -> the (re, im) views of one [R, F, 2, h] device buffer, as stft(n_fft=n) returns them"""
    frames, bins = re.shape[0] // rows, sn.bins(n)
    buf = np.full((rows, frames, 2, sn.pitch(n)), de.SENTINEL, np.int16)
    buf[:, :, 0, :bins] = re.view(np.int16).reshape(rows, frames, bins)
    buf[:, :, 1, :bins] = im.view(np.int16).reshape(rows, frames, bins)
    d = torch.from_numpy(buf).to(DEV).view(torch.float16)
    return d[:, :, 0, :bins], d[:, :, 1, :bins]


def _plan_y(tf, n, re, im, w, rows, length, hop, pad):
    return run_istftn(tf, n, re, im, w, rows, length, hop, pad)[1]


@pytest.mark.parametrize("n", LENGTHS)
def test_functions_match_the_plan(tf, monkeypatch, n):
    mod = importlib.import_module("tensor_fft_amd.istftn")
    uploads = []
    real_set = mod.TfftShortIstftPlan.set_window
    monkeypatch.setattr(mod.TfftShortIstftPlan, "set_window", lambda self, w, stream=None: (uploads.append(1), real_set(self, w, stream))[1])
    tf.istftn_cache_clear()
    rows, length, hop, pad = 2, 2 * n, n // 2, n // 2
    _, w, re, im = inputs(n, rows, length, hop, pad, "hann")
    _, y = result(tf, n, rows, length, hop, pad, 0, "hann")
    v_re, v_im = _stft_layout(n, re, im, rows)
    d_w = torch.from_numpy(w.copy()).to(DEV)
    # center=True is pad = n / 2; the views are taken as they are
    got = tf.short_istft(v_re, v_im, d_w, hop, length, n, center=True)
    assert got.shape == (rows, length) and got.dtype == torch.float16
    assert np.array_equal(got.cpu().numpy().view(np.int16), y) and len(uploads) == 1
    # istft(n_fft=n) is the same call; the same window again: no upload; any other layout is copied first and gives the same bits
    routed = tf.istft(v_re, v_im, d_w, hop, length, center=True, n_fft=n)
    assert np.array_equal(routed.cpu().numpy().view(np.int16), y) and len(uploads) == 1
    again = tf.short_istft(v_re.contiguous(), v_im.contiguous(), d_w, hop, length, n, center=True)
    assert np.array_equal(again.cpu().numpy().view(np.int16), y) and len(uploads) == 1
    # the views stft(n_fft=n) returns, taken as they are: the same bits as the plan on the same spectra
    x = inputs(n, rows, length, hop, pad, "hann")[0]
    f_re, f_im = tf.stft(torch.from_numpy(x.copy()).to(DEV), d_w, hop, center=True, n_fft=n)
    trip = tf.istft(f_re, f_im, d_w, hop, length, center=True, n_fft=n)
    assert len(uploads) == 1
    h_re, h_im = np.ascontiguousarray(f_re.cpu().numpy()).reshape(-1, sn.bins(n)), np.ascontiguousarray(f_im.cpu().numpy()).reshape(-1, sn.bins(n))
    _assert_bits("istft(stft(x)) against the plan on the same spectra", trip.cpu().numpy().view(np.int16), _plan_y(tf, n, h_re, h_im, w, rows, length, hop, pad))
    # modified in place: uploaded again (the plan of the comparison above took an upload of its own)
    del uploads[1:]
    d_w.mul_(0.5)
    halved = tf.short_istft(v_re, v_im, d_w, hop, length, n, center=True)
    assert len(uploads) == 2
    w_half = (w.astype(np.float32) * 0.5).astype(np.float16)
    _assert_bits("short_istft() after an in-place change of the window", halved.cpu().numpy().view(np.int16),
                 _plan_y(tf, n, re, im, w_half, rows, length, hop, pad))
    raw = tf.short_istft(v_re, v_im, d_w, hop, length, n, center=True, raw_sum=True)
    assert (raw.cpu().numpy().view(np.int16) != halved.cpu().numpy().view(np.int16)).any()
    # center=False is pad = 0, and a window of n / 4 samples is centred in the n: most samples lie under its zeros only and are +0
    rng = np.random.default_rng([5, n])
    short = rng.uniform(0, 1, n // 4).astype(np.float16)
    full = np.zeros(n, np.float16)
    lo = (n - n // 4) // 2
    full[lo:lo + n // 4] = short
    _, _, re0, im0 = inputs(n, rows, length, hop, 0, "hann")
    s_re, s_im = _stft_layout(n, re0, im0, rows)
    s = tf.short_istft(s_re, s_im, torch.from_numpy(short).to(DEV), hop, length, n).cpu().numpy().view(np.int16)
    _assert_bits("short_istft() with a window of n / 4 samples", s, _plan_y(tf, n, re0, im0, full, rows, length, hop, 0))
    assert (s[:, :lo] == 0).all() and (s[:, lo:lo + n // 4] != 0).any()
    with pytest.raises(tf.TfftError):
        tf.short_istft(s_re, s_im, torch.zeros(n + 8, dtype=torch.float16, device=DEV), hop, length, n)
    with pytest.raises(tf.TfftError):              # F does not fit the length
        tf.short_istft(s_re, s_im, d_w, hop, length + n // 2, n)
    with pytest.raises(tf.TfftError):              # the spectra of another frame length
        tf.istft(s_re, s_im, d_w, hop, length, n_fft=2 * n if n < 2048 else 512)
    tf.istftn_cache_clear()
    tf.stftn_cache_clear()


@pytest.mark.parametrize("n", LENGTHS)
def test_replay_under_graph_capture(tf, n):
    rows, length, hop, pad = 3, 3 * n // 2, n // 4, 0
    _, w, re, im = inputs(n, rows, length, hop, pad, "random")
    _, y = result(tf, n, rows, length, hop, pad, 0, "random")
    plan = tf.TfftShortIstftPlan(n, rows, length, hop, pad, 0, in_frame_stride=_in_stride(n))
    plan.set_window(torch.from_numpy(w.copy()).to(DEV))
    plan.prepare()                                   # the plan's own workspace, settled before the capture
    d_in = torch.from_numpy(_flat_spectra(n, re, im)).to(DEV).view(torch.float16)
    d_out = torch.zeros(rows * length, dtype=torch.float16, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            plan.exec(d_in, d_in[sn.pitch(n):], d_out)
    torch.cuda.synchronize()
    assert not d_out.any(), "a captured execution ran at capture time"
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.int16).reshape(rows, length), y)
    del graph
    plan.close()


@pytest.mark.parametrize("n", LENGTHS)
def test_refusals_leave_the_output_untouched(tf, n):
    rows, length, hop, pitch = 2, 2 * n, n // 4, sn.pitch(n)
    plan = tf.TfftShortIstftPlan(n, rows, length, hop)
    total = rows * plan.frames
    d_in = torch.zeros(total * 2 * pitch + 8, dtype=torch.float16, device=DEV)
    d_out = torch.from_numpy(np.full(rows * length + 8, de.SENTINEL, np.int16)).to(DEV).view(torch.float16)
    d_ws = torch.from_numpy(np.full(total * n, de.SENTINEL, np.int16)).to(DEV).view(torch.float16)
    re_p, im_p, out_p = d_in.data_ptr(), d_in.data_ptr() + 2 * pitch, d_out.data_ptr()

    def refused(needle, *args):
        with pytest.raises(tf.TfftError) as e:
            plan.exec_ptr(*args)
        assert needle in str(e.value), str(e.value)

    # before a window was set
    refused("tfft_istftn_plan_set_window", re_p, im_p, out_p)
    plan.set_window(torch.ones(n, dtype=torch.float16, device=DEV))
    # a pointer that is not 16-byte aligned: each of the three
    refused("16-byte aligned", re_p + 2, im_p, out_p)
    refused("16-byte aligned", re_p, im_p + 8, out_p)
    refused("16-byte aligned", re_p, im_p, out_p + 2)
    # the output inside an input plane's extent, and an input plane inside the output's
    refused("output and input overlap", re_p, im_p, re_p)
    refused("output and input overlap", re_p, im_p, re_p + 2 * total * 2 * pitch - 16)
    refused("output and input overlap", out_p, im_p, out_p)
    refused("output and input overlap", re_p, out_p + 2 * rows * length - 16, out_p)
    # a caller's workspace that is too small, one on the output, and one on the input
    with pytest.raises(tf.TfftError) as e:
        plan.set_workspace(d_ws[:n])
    assert e.value.code != 0 and "workspace" in str(e.value)
    plan.set_workspace(d_ws)
    refused("the workspace overlaps the output", re_p, im_p, d_ws.data_ptr() + 4096)
    big = torch.zeros(max(total * n, d_in.numel()) + 128, dtype=torch.float16, device=DEV)
    plan.set_workspace(big)
    refused("the workspace overlaps the input", big.data_ptr(), big.data_ptr() + 2 * pitch, out_p)
    plan.set_workspace(d_ws)
    torch.cuda.synchronize()
    assert (d_out.view(torch.int16) == de.SENTINEL).all() and (d_ws.view(torch.int16) == de.SENTINEL).all() and not d_in.any()
    # and the call that is legal runs: zero spectra give zeros
    plan.exec_ptr(re_p, im_p, out_p)
    torch.cuda.synchronize()
    assert not d_out[:rows * length].any() and (d_out[rows * length:].view(torch.int16) == de.SENTINEL).all()
    assert not d_ws.any()
    plan.close()


def test_example_runs():
    exe = os.path.join(ROOT, "examples", "example_istftn")
    assert os.path.exists(exe), "build() did not build examples/example_istftn"
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("OK"), run.stdout + run.stderr
