"""Short-frame STFT plans on the GPU (tfft_stftn_*, include/tfft_stftn.h): hopped, windowed frames of 512, 1024 and 2048 samples to
half spectra in one kernel. Every case runs ONCE between guard zones (module-scoped cache) and is held to

  1. the shipped TfftRealPlan(n, R * F) (default plan, sequential scaling) on the frames built on the host (tests/stftn_ref.py: the
     binary16 products in the flat order g), bit for bit in bins 0 .. n / 2 of both planes (code that is already validated, not the
     code under test; it pins the pairing of frames 2b and 2b + 1, the self-paired last frame of an odd total, and the arithmetic),
  2. the layout: output prefilled with NaN bit patterns with out_frame_stride = 2 h + 16, whose halves beyond bin n / 2, gaps and
     guard zones come back bit for bit; input with in_sig_stride = L + 64 whose gaps and guard zones hold NaNs (a read outside
     [0, L) of any signal poisons the result) and which is bit-identical afterwards,
  3. fp64 on the pad-0 shapes, frame by frame.

A fresh compute unit's LDS may read as zero, so a missing or misplaced zero fill shows only from a wave's second group on: in the
last case of stftn_ref.cases(n) every live wave of the launch takes three groups (stftn_ref.looping_case derives its 93, 45 and 21
frames from conv_shape), and the launch_iters test runs that shape in every launch mode.

The two-pass R2C leaves a sum of -0 as +0 (stftn/stft256r.hpp, split_bin, has the reason), and so does the plan: case 5 at n = 2048
holds such a bin (frame 0, bin 0).

Measured on the MI355X (seed 1), worst frame of the two pad-0 shapes, against fp64 of the binary16 products / of the unrounded
products: n = 512 4.29e-04 / 4.80e-04, n = 1024 4.15e-04 / 4.65e-04, n = 2048 4.12e-04 / 4.65e-04."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import dist_emulate as de
import stftn_ref as sn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
K_RFFT = 1.5e-3                    # what tests/test_gpu_rfft.py asserts for this arithmetic: rel-L2 of a half spectrum against fp64


def out_stride(n):
    return 2 * sn.pitch(n) + 16


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    return tensor_fft_amd


def _flat_in(x, stride):
    """[R][L] -> one flat int16 array, signal r at r * stride, NaN sentinels between"""
    rows, length = x.shape
    flat = np.full((rows - 1) * stride + length, de.SENTINEL, dtype=np.int16)
    idx = (np.arange(rows) * stride)[:, None] + np.arange(length)[None, :]
    flat[idx] = x.view(np.int16)
    return flat


def run_stftn(tf, n, x, w, hop, pad, launch_iters=0):
    """One execution between guard zones with padded strides: returns (re, im), [R * F][n / 2 + 1] int16 bit patterns. Checks on the
    way: guards, the halves beyond bin n / 2 and the gaps between frames untouched, the input bit-identical, one launch of the one
    kernel. The window tensor is poisoned after set_window: the plan owns its copy."""
    rows, length = x.shape
    in_stride, ostride, bins, pitch = length + 64, out_stride(n), sn.bins(n), sn.pitch(n)
    plan = tf.TfftShortStftPlan(n, rows, length, hop, pad, 0, in_sig_stride=in_stride, out_frame_stride=ostride, launch_iters=launch_iters)
    total = rows * plan.frames
    assert plan.frames == sn.geometry(n, length, hop, pad) and (plan.bins, plan.pitch) == (bins, pitch)
    assert plan.num_launches == 1 and plan.kernels == [f"stft256r::stft256r_kernel<{n // 256}>"]
    d_w = torch.from_numpy(w).to(DEV)
    plan.set_window(d_w)
    torch.cuda.synchronize()
    d_w.fill_(float("nan"))
    host_in = _flat_in(x, in_stride)
    assert np.isnan(np.int16(de.SENTINEL).view(np.float16))
    n_in, n_out = host_in.size, (total - 1) * ostride + 2 * pitch          # the last frame's [RE | IM] block in full
    d_in = de._guarded(torch, n_in, host_in.view(np.float16))
    d_out = de._guarded(torch, n_out)
    g = de.GUARD
    body = d_out[g:g + n_out]
    plan.exec(d_in[g:g + n_in], body, body[pitch:])
    torch.cuda.synchronize()
    assert de._guards_intact(torch, d_out), "output guard zone written"
    out = body.cpu().numpy().view(np.int16)
    idx = (np.arange(total) * ostride)[:, None] + np.arange(bins)[None, :]
    written = np.zeros(n_out, bool)
    written[idx.reshape(-1)] = True
    written[(idx + pitch).reshape(-1)] = True
    assert (out[~written] == de.SENTINEL).all(), "halves beyond bin n / 2 or between frames written"
    assert de._guards_intact(torch, d_in)
    de._untouched(d_in[g:g + n_in].cpu().numpy().view(np.int16), host_in, "input signals")
    plan.close()
    return out[idx], out[idx + pitch]


def via_real_plan(tf, n, u):
    """the shipped TfftRealPlan(n, G) on frames [G][n] fp16 uploaded from the host: (re, im), [G][n / 2 + 1] int16 bit patterns"""
    total, pitch, bins = u.shape[0], sn.pitch(n), sn.bins(n)
    plan = tf.TfftRealPlan(n, total, 0)
    d_u = torch.from_numpy(np.ascontiguousarray(u).reshape(-1)).to(DEV)
    d_s = torch.zeros(total * 2 * pitch, dtype=torch.float16, device=DEV)
    plan.r2c(d_u, d_s, d_s[pitch:])
    torch.cuda.synchronize()
    s = d_s.cpu().numpy().view(np.int16).reshape(total, 2, pitch)
    plan.close()
    return s[:, 0, :bins].copy(), s[:, 1, :bins].copy()


_results = {}


def result(tf, n, rows, length, hop, pad, iters, window="hann"):
    """(x, w, re, im) of one case, computed once per module"""
    key = (n, rows, length, hop, pad, iters, window)
    if key not in _results:
        x, w = sn.case_data(n, rows, length, window=window)
        _results[key] = (x, w) + run_stftn(tf, n, x, w, hop, pad, iters)
    return _results[key]


_wanted = {}


def wanted(tf, n, rows, length, hop, pad, window="hann"):
    """the reference of comparison 1, computed once per shape and left unchanged"""
    key = (n, rows, length, hop, pad, window)
    if key not in _wanted:
        x, w = sn.case_data(n, rows, length, window=window)
        _wanted[key] = via_real_plan(tf, n, sn.frames(x, w, hop, pad))
        for a in _wanted[key]:
            a.setflags(write=False)
    return _wanted[key]


def _assert_bits(what, got, want):
    for name, a, b in (("RE", got[0], want[0]), ("IM", got[1], want[1])):
        bad = np.argwhere(a != b)
        assert bad.size == 0, f"{what}: {name} plane differs from frames -> TfftRealPlan in {len(bad)} halves, first (frame, bin) = {bad[:3].tolist()}"


def _bits(t, bins):
    return t.cpu().numpy().view(np.int16).reshape(-1, bins)


@pytest.mark.parametrize("case", range(8))
@pytest.mark.parametrize("n", sn.LENGTHS)
def test_bit_for_bit_with_the_real_plan_on_host_built_frames(tf, n, case):
    rows, length, hop, pad, iters = sn.cases(n)[case]
    if case == 7:         # the derivation of the looping case, on this chip's compute units
        assert sn.looping_case(n, torch.cuda.get_device_properties(0).multi_processor_count) == (rows, length, hop, pad)
    _, _, re, im = result(tf, n, rows, length, hop, pad, iters)
    assert not np.isnan(re.view(np.float16)).any() and not np.isnan(im.view(np.float16)).any()
    _assert_bits(f"stftn n={n} R={rows} L={length} hop={hop} pad={pad} iters={iters}", (re, im), wanted(tf, n, rows, length, hop, pad))


@pytest.mark.parametrize("case", sn.RANDOM_WINDOW_CASES)
@pytest.mark.parametrize("n", sn.LENGTHS)
def test_a_random_window_shows_what_a_symmetric_one_hides(tf, n, case):
    rows, length, hop, pad, iters = sn.cases(n)[case]
    _, _, re, im = result(tf, n, rows, length, hop, pad, iters, "random")
    _assert_bits(f"stftn random window n={n} R={rows} L={length} hop={hop} pad={pad}", (re, im), wanted(tf, n, rows, length, hop, pad, "random"))


@pytest.mark.parametrize("iters", [0, 1, 3, 65535])
@pytest.mark.parametrize("n", sn.LENGTHS)
def test_launch_iters_never_changes_a_bit(tf, n, iters):
    rows, length, hop, pad, _ = sn.cases(n)[7]
    _, _, re, im = result(tf, n, rows, length, hop, pad, iters)
    _assert_bits(f"stftn n={n} iters={iters}", (re, im), wanted(tf, n, rows, length, hop, pad))


@pytest.mark.parametrize("shape", range(2))
@pytest.mark.parametrize("n", sn.LENGTHS)
def test_accuracy_against_fp64(tf, n, shape):
    """Per frame, rel-L2 of bins 0 .. n / 2 against fp64 rfft / n of the binary16 products (K_RFFT, the bound tests/test_gpu_rfft.py
    holds R2C to) and of the unrounded products (+ 2^-10, tests/test_stftn_host.py derives it). Pad-0 shapes: every frame is full
    and a pair's two frames have like magnitude."""
    rows, length, hop, pad = sn.accuracy_shapes(n)[shape]
    x, w, re, im = result(tf, n, rows, length, hop, pad, 0)
    _assert_bits(f"stftn n={n} R={rows} L={length}", (re, im), wanted(tf, n, rows, length, hop, pad))
    got = re.view(np.float16).astype(np.float64) + 1j * im.view(np.float16).astype(np.float64)
    rounded = np.fft.rfft(sn.frames(x, w, hop, pad).astype(np.float64), axis=-1) / n
    exact = np.fft.rfft(sn.windows(n, x.astype(np.float64), hop, pad) * w.astype(np.float64)[None, :], axis=-1) / n
    e_rounded, e_exact = sn.rel_l2(got, rounded).max(), sn.rel_l2(got, exact).max()
    print(f"stftn n={n} R={rows} L={length} hop={hop}: worst frame rel-L2 {e_rounded:.2e} against fp64 of the binary16 products, "
          f"{e_exact:.2e} against fp64 of the unrounded products")
    assert e_rounded <= K_RFFT and e_exact <= K_RFFT + 2.0 ** -10


@pytest.mark.parametrize("n", sn.LENGTHS)
def test_short_stft_and_stft_match_the_plan(tf, n, monkeypatch):
    stftn_mod = importlib.import_module("tensor_fft_amd.stftn")
    uploads = []
    real_set = stftn_mod.TfftShortStftPlan.set_window
    monkeypatch.setattr(stftn_mod.TfftShortStftPlan, "set_window", lambda self, w, stream=None: (uploads.append(1), real_set(self, w, stream))[1])
    tf.stftn_cache_clear()
    bins, pitch = sn.bins(n), sn.pitch(n)
    rows, length, hop, pad, _ = sn.cases(n)[3]                  # (1, 2 n, n / 2, n / 2): center=True is pad = n / 2
    x, w, re, im = result(tf, n, rows, length, hop, pad, 0)
    frames = sn.geometry(n, length, hop, pad)
    d_x, d_w = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)
    g_re, g_im = tf.short_stft(d_x, d_w, hop, n, center=True)
    assert g_re.shape == g_im.shape == (rows, frames, bins) and g_re.data_ptr() + 2 * pitch == g_im.data_ptr()
    assert np.array_equal(_bits(g_re, bins), re) and np.array_equal(_bits(g_im, bins), im)
    assert len(uploads) == 1
    # stft(n_fft=n) is the same call and the same cached plan; the same window again: no upload; modified in place: uploaded again
    s_re, s_im = tf.stft(d_x, d_w, hop, center=True, n_fft=n)
    assert np.array_equal(_bits(s_re, bins), re) and np.array_equal(_bits(s_im, bins), im)
    assert len(uploads) == 1
    d_w.mul_(0.5)
    h_re, h_im = tf.short_stft(d_x, d_w, hop, n, center=True)
    assert len(uploads) == 2
    half = via_real_plan(tf, n, sn.frames(x, (w.astype(np.float32) * 0.5).astype(np.float16), hop, pad))
    _assert_bits("short_stft() after an in-place change of the window", (_bits(h_re, bins), _bits(h_im, bins)), half)
    # center=False is pad = 0, and a window of n / 4 samples is centred in the n
    rng = np.random.default_rng([n, 5])
    short = rng.uniform(0, 1, n // 4).astype(np.float16)
    full = np.zeros(n, np.float16)
    full[3 * n // 8:5 * n // 8] = short
    c_re, c_im = tf.stft(d_x, torch.from_numpy(short).to(DEV), hop, n_fft=n)
    assert c_re.shape == (rows, sn.geometry(n, length, hop, 0), bins)
    want = via_real_plan(tf, n, sn.frames(x, full, hop, 0))
    _assert_bits("stft(n_fft) with a window of n / 4 samples", (_bits(c_re, bins), _bits(c_im, bins)), want)
    with pytest.raises(tf.TfftError):
        tf.short_stft(d_x, torch.zeros(n + 8, dtype=torch.float16, device=DEV), hop, n)
    with pytest.raises(tf.TfftError):
        tf.stft(d_x, d_w, hop, n_fft=768)
    tf.stftn_cache_clear()


@pytest.mark.parametrize("n", sn.LENGTHS)
def test_replay_under_graph_capture(tf, n):
    rows, length, hop, pad, _ = sn.cases(n)[2]
    x, w, re, im = result(tf, n, rows, length, hop, pad, 0)
    ostride, bins, pitch = out_stride(n), sn.bins(n), sn.pitch(n)
    plan = tf.TfftShortStftPlan(n, rows, length, hop, pad, 0, out_frame_stride=ostride)
    total = rows * plan.frames
    plan.set_window(torch.from_numpy(w).to(DEV))
    d_x = torch.from_numpy(x).to(DEV).view(-1)
    d_out = torch.zeros(total * ostride, dtype=torch.float16, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            plan.exec(d_x, d_out, d_out[pitch:])
    torch.cuda.synchronize()
    assert not d_out.any(), "a captured execution ran at capture time"
    graph.replay()
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.int16).reshape(total, ostride)
    assert np.array_equal(out[:, :bins], re) and np.array_equal(out[:, pitch:pitch + bins], im)
    del graph
    plan.close()


@pytest.mark.parametrize("n", sn.LENGTHS)
def test_refusals_leave_the_output_untouched(tf, n):
    rows, length, hop = 2, 4 * n, n // 4
    bins, pitch = sn.bins(n), sn.pitch(n)
    plan = tf.TfftShortStftPlan(n, rows, length, hop)
    total = rows * plan.frames
    d_x = torch.zeros(rows * length + 8, dtype=torch.float16, device=DEV)
    d_out = torch.from_numpy(np.full(total * 2 * pitch + 8, de.SENTINEL, np.int16)).to(DEV).view(torch.float16)

    def refused(needle, *args):
        with pytest.raises(tf.TfftError) as e:
            plan.exec_ptr(*args)
        assert needle in str(e.value), str(e.value)

    # before a window was set
    refused("tfft_stftn_plan_set_window", d_x.data_ptr(), d_out.data_ptr(), d_out.data_ptr() + 2 * pitch)
    plan.set_window(torch.ones(n, dtype=torch.float16, device=DEV))
    # a pointer that is not 16-byte aligned: each of the three
    refused("16-byte aligned", d_x.data_ptr() + 2, d_out.data_ptr(), d_out.data_ptr() + 2 * pitch)
    refused("16-byte aligned", d_x.data_ptr(), d_out.data_ptr() + 8, d_out.data_ptr() + 2 * pitch)
    refused("16-byte aligned", d_x.data_ptr(), d_out.data_ptr(), d_out.data_ptr() + 2 * pitch + 2)
    # an output plane inside the input, the input inside the output, and the two planes on each other
    refused("input and output overlap", d_x.data_ptr(), d_x.data_ptr(), d_out.data_ptr())
    refused("input and output overlap", d_x.data_ptr(), d_out.data_ptr(), d_x.data_ptr() + 2 * length)
    refused("input and output overlap", d_out.data_ptr() + 16, d_out.data_ptr(), d_out.data_ptr() + 2 * pitch)
    refused("RE and IM output planes overlap", d_x.data_ptr(), d_out.data_ptr(), d_out.data_ptr())
    refused("RE and IM output planes overlap", d_x.data_ptr(), d_out.data_ptr(), d_out.data_ptr() + 2 * (n // 2))
    torch.cuda.synchronize()
    assert (d_out.view(torch.int16) == de.SENTINEL).all() and not d_x.any()
    # and the call that is legal runs
    plan.exec_ptr(d_x.data_ptr(), d_out.data_ptr(), d_out.data_ptr() + 2 * pitch)
    torch.cuda.synchronize()
    assert not d_out.view(-1)[:total * 2 * pitch].view(total, 2, pitch)[:, :, :bins].any()
    plan.close()


def test_example_runs():
    exe = os.path.join(ROOT, "examples", "example_stftn")
    assert os.path.exists(exe), "build() did not build examples/example_stftn"
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("OK"), run.stdout + run.stderr
