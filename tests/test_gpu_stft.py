"""STFT plans on the GPU (tfft_stft_*, include/tfft_stft.h): hopped, windowed frames of 4096 samples to half spectra in one kernel.
Every case runs ONCE between guard zones (module-scoped cache) and is held to

  1. the shipped TfftRealPlan(4096, R * F) on the frames built on the host (tests/stft_ref.py: the binary16 products in the flat
     order g), bit for bit in bins 0 .. 2048 of both planes (code that is already validated, not the code under test; it pins the
     pairing of frames 2i and 2i + 1, the self-paired last frame of an odd total, and the arithmetic),
  2. the layout: output prefilled with NaN bit patterns with out_frame_stride = 2 * 2056 + 16, whose halves beyond bin 2048, gaps
     and guard zones come back bit for bit; input with in_sig_stride = L + 64 whose gaps and guard zones hold NaNs (a read outside
     [0, L) of any signal poisons the result) and which is bit-identical afterwards,
  3. fp64 on the pad-0 shapes, frame by frame.

A fresh compute unit's LDS may read as zero, so a missing or misplaced zero fill shows only from a wave's second item on
(tests/test_gpu_sconv.py has the note): the cases with launch_iters make the waves loop.

Measured on the MI355X (seed 1), worst frame of the two pad-0 shapes: rel-L2 4.9e-04 against fp64 of the binary16 products, 5.3e-04
against fp64 of the unrounded products."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import dist_emulate as de
import stft_ref as st

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
OUT_STRIDE = 2 * st.PITCH + 16
K_RFFT = 1.5e-3                    # what tests/test_gpu_rfft.py asserts for this arithmetic: rel-L2 of a half spectrum against fp64


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


def run_stft(tf, x, w, hop, pad, launch_iters=0):
    """One execution between guard zones with padded strides: returns (re, im), [R * F][2049] int16 bit patterns. Checks on the way:
    guards, the halves beyond bin 2048 and the gaps between frames untouched, the input bit-identical, one launch of the one
    kernel. The window tensor is poisoned after set_window: the plan owns its copy."""
    rows, length = x.shape
    in_stride = length + 64
    plan = tf.TfftStftPlan(rows, length, hop, pad, 0, in_sig_stride=in_stride, out_frame_stride=OUT_STRIDE, launch_iters=launch_iters)
    total = rows * plan.frames
    assert plan.frames == st.geometry(length, hop, pad) and (plan.bins, plan.pitch) == (st.BINS, st.PITCH)
    assert plan.num_launches == 1 and plan.kernels == ["stft4096::stft4096_kernel"]
    d_w = torch.from_numpy(w).to(DEV)
    plan.set_window(d_w)
    torch.cuda.synchronize()
    d_w.fill_(float("nan"))
    host_in = _flat_in(x, in_stride)
    assert np.isnan(np.int16(de.SENTINEL).view(np.float16))
    n_in, n_out = host_in.size, (total - 1) * OUT_STRIDE + 2 * st.PITCH          # the last frame's [RE | IM] block in full
    d_in = de._guarded(torch, n_in, host_in.view(np.float16))
    d_out = de._guarded(torch, n_out)
    g = de.GUARD
    body = d_out[g:g + n_out]
    plan.exec(d_in[g:g + n_in], body, body[st.PITCH:])
    torch.cuda.synchronize()
    assert de._guards_intact(torch, d_out), "output guard zone written"
    out = body.cpu().numpy().view(np.int16)
    idx = (np.arange(total) * OUT_STRIDE)[:, None] + np.arange(st.BINS)[None, :]
    written = np.zeros(n_out, bool)
    written[idx.reshape(-1)] = True
    written[(idx + st.PITCH).reshape(-1)] = True
    assert (out[~written] == de.SENTINEL).all(), "halves beyond bin 2048 or between frames written"
    assert de._guards_intact(torch, d_in)
    de._untouched(d_in[g:g + n_in].cpu().numpy().view(np.int16), host_in, "input signals")
    plan.close()
    return out[idx], out[idx + st.PITCH]


def via_real_plan(tf, u):
    """the shipped TfftRealPlan(4096, G) on frames [G][4096] fp16 uploaded from the host: (re, im), [G][2049] int16 bit patterns"""
    total = u.shape[0]
    plan = tf.TfftRealPlan(st.N, total, 0)
    d_u = torch.from_numpy(np.ascontiguousarray(u).reshape(-1)).to(DEV)
    d_s = torch.zeros(total * 2 * st.PITCH, dtype=torch.float16, device=DEV)
    plan.r2c(d_u, d_s, d_s[st.PITCH:])
    torch.cuda.synchronize()
    assert plan.num_launches() == 1            # the fused one-pass R2C, the kernel the STFT kernel restates
    s = d_s.cpu().numpy().view(np.int16).reshape(total, 2, st.PITCH)
    plan.close()
    return s[:, 0, :st.BINS].copy(), s[:, 1, :st.BINS].copy()


_results = {}


def result(tf, rows, length, hop, pad, iters, window="hann"):
    """(x, w, re, im) of one case, computed once per module"""
    key = (rows, length, hop, pad, iters, window)
    if key not in _results:
        x, w = st.case_data(rows, length, window=window)
        _results[key] = (x, w) + run_stft(tf, x, w, hop, pad, iters)
    return _results[key]


_wanted = {}


def wanted(tf, rows, length, hop, pad, window="hann"):
    """the reference of comparison 1, computed once per shape and left unchanged"""
    key = (rows, length, hop, pad, window)
    if key not in _wanted:
        x, w = st.case_data(rows, length, window=window)
        _wanted[key] = via_real_plan(tf, st.frames(x, w, hop, pad))
        for a in _wanted[key]:
            a.setflags(write=False)
    return _wanted[key]


def _assert_bits(what, got, want):
    for name, a, b in (("RE", got[0], want[0]), ("IM", got[1], want[1])):
        bad = np.argwhere(a != b)
        assert bad.size == 0, f"{what}: {name} plane differs from frames -> TfftRealPlan in {len(bad)} halves, first (frame, bin) = {bad[:3].tolist()}"


@pytest.mark.parametrize("rows,length,hop,pad,iters", st.CASES)
def test_bit_for_bit_with_the_real_plan_on_host_built_frames(tf, rows, length, hop, pad, iters):
    _, _, re, im = result(tf, rows, length, hop, pad, iters)
    assert not np.isnan(re.view(np.float16)).any() and not np.isnan(im.view(np.float16)).any()
    _assert_bits(f"stft R={rows} L={length} hop={hop} pad={pad} iters={iters}", (re, im), wanted(tf, rows, length, hop, pad))


@pytest.mark.parametrize("rows,length,hop,pad,iters", [(3, 6144, 1024, 0, 0), (2, 8192, 2048, 2048, 0), (2, 4096, 512, 4088, 0)])
def test_a_random_window_shows_what_a_symmetric_one_hides(tf, rows, length, hop, pad, iters):
    _, _, re, im = result(tf, rows, length, hop, pad, iters, "random")
    _assert_bits(f"stft random window R={rows} L={length} hop={hop} pad={pad}", (re, im), wanted(tf, rows, length, hop, pad, "random"))


@pytest.mark.parametrize("iters", [0, 1, 3, 65535])
def test_launch_iters_never_changes_a_bit(tf, iters):
    rows, length, hop, pad = 5, 8192, 2048, 2048
    _, _, re, im = result(tf, rows, length, hop, pad, iters)
    _assert_bits(f"stft iters={iters}", (re, im), wanted(tf, rows, length, hop, pad))


@pytest.mark.parametrize("rows,length,hop,pad", [(3, 6144, 1024, 0), (4, 11264, 1024, 0)])
def test_accuracy_against_fp64(tf, rows, length, hop, pad):
    """Per frame, rel-L2 of bins 0 .. 2048 against fp64 rfft / 4096 of the binary16 products (K_RFFT, the bound of the real-input
    transform) and of the unrounded products (+ 2^-10, tests/test_stft_host.py derives it). Pad-0 shapes: every frame is full and a
    pair's two frames have like magnitude. Measured on the MI355X, worst frame: 4.90e-04 and 5.28e-04 (3 x 6144), 4.92e-04 and 5.34e-04 (4 x 11264)."""
    x, w, re, im = result(tf, rows, length, hop, pad, 0)
    got = re.view(np.float16).astype(np.float64) + 1j * im.view(np.float16).astype(np.float64)
    rounded = np.fft.rfft(st.frames(x, w, hop, pad).astype(np.float64), axis=-1) / st.N
    exact = np.fft.rfft(st.windows(x.astype(np.float64), hop, pad) * w.astype(np.float64)[None, :], axis=-1) / st.N
    e_rounded, e_exact = st.rel_l2(got, rounded).max(), st.rel_l2(got, exact).max()
    print(f"stft R={rows} L={length} hop={hop}: worst frame rel-L2 {e_rounded:.2e} against fp64 of the binary16 products, "
          f"{e_exact:.2e} against fp64 of the unrounded products")
    assert e_rounded <= K_RFFT and e_exact <= K_RFFT + 2.0 ** -10


def test_stft_function_matches_the_plan(tf, monkeypatch):
    stft_mod = importlib.import_module("tensor_fft_amd.stft")
    uploads = []
    real_set = stft_mod.TfftStftPlan.set_window
    monkeypatch.setattr(stft_mod.TfftStftPlan, "set_window", lambda self, w, stream=None: (uploads.append(1), real_set(self, w, stream))[1])
    tf.stft_cache_clear()
    rows, length, hop = 2, 8192, 2048
    x, w, re, im = result(tf, rows, length, hop, 2048, 0)
    frames = st.geometry(length, hop, 2048)
    d_x, d_w = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)
    # center=True is pad = 2048
    g_re, g_im = tf.stft(d_x, d_w, hop, center=True)
    assert g_re.shape == g_im.shape == (rows, frames, st.BINS) and g_re.data_ptr() + 2 * st.PITCH == g_im.data_ptr()
    assert np.array_equal(g_re.cpu().numpy().view(np.int16).reshape(-1, st.BINS), re) and np.array_equal(g_im.cpu().numpy().view(np.int16).reshape(-1, st.BINS), im)
    assert len(uploads) == 1
    # the same window again: no upload; modified in place: uploaded again
    tf.stft(d_x, d_w, hop, center=True)
    assert len(uploads) == 1
    d_w.mul_(0.5)
    h_re, h_im = tf.stft(d_x, d_w, hop, center=True)
    assert len(uploads) == 2
    half = via_real_plan(tf, st.frames(x, (w.astype(np.float32) * 0.5).astype(np.float16), hop, 2048))
    _assert_bits("stft() after an in-place change of the window", (h_re.cpu().numpy().view(np.int16).reshape(-1, st.BINS), h_im.cpu().numpy().view(np.int16).reshape(-1, st.BINS)), half)
    # center=False is pad = 0, and a window of 1024 samples is centred in the 4096
    rng = np.random.default_rng(5)
    short = rng.uniform(0, 1, 1024).astype(np.float16)
    full = np.zeros(st.N, np.float16)
    full[1536:2560] = short
    s_re, s_im = tf.stft(d_x, torch.from_numpy(short).to(DEV), hop)
    assert s_re.shape == (rows, st.geometry(length, hop, 0), st.BINS)
    want = via_real_plan(tf, st.frames(x, full, hop, 0))
    _assert_bits("stft() with a window of 1024 samples", (s_re.cpu().numpy().view(np.int16).reshape(-1, st.BINS), s_im.cpu().numpy().view(np.int16).reshape(-1, st.BINS)), want)
    with pytest.raises(tf.TfftError):
        tf.stft(d_x, torch.zeros(4104, dtype=torch.float16, device=DEV), hop)
    tf.stft_cache_clear()


def test_replay_under_graph_capture(tf):
    rows, length, hop, pad = 3, 6144, 1024, 0
    x, w, re, im = result(tf, rows, length, hop, pad, 0)
    plan = tf.TfftStftPlan(rows, length, hop, pad, 0, out_frame_stride=OUT_STRIDE)
    total = rows * plan.frames
    plan.set_window(torch.from_numpy(w).to(DEV))
    d_x = torch.from_numpy(x).to(DEV).view(-1)
    d_out = torch.zeros(total * OUT_STRIDE, dtype=torch.float16, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            plan.exec(d_x, d_out, d_out[st.PITCH:])
    torch.cuda.synchronize()
    assert not d_out.any(), "a captured execution ran at capture time"
    graph.replay()
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.int16).reshape(total, OUT_STRIDE)
    assert np.array_equal(out[:, :st.BINS], re) and np.array_equal(out[:, st.PITCH:st.PITCH + st.BINS], im)
    del graph
    plan.close()


def test_refusals_leave_the_output_untouched(tf):
    rows, length, hop = 2, 8192, 1024
    plan = tf.TfftStftPlan(rows, length, hop)
    total = rows * plan.frames
    d_x = torch.zeros(rows * length + 8, dtype=torch.float16, device=DEV)
    d_out = torch.from_numpy(np.full(total * 2 * st.PITCH + 8, de.SENTINEL, np.int16)).to(DEV).view(torch.float16)

    def refused(needle, *args):
        with pytest.raises(tf.TfftError) as e:
            plan.exec_ptr(*args)
        assert needle in str(e.value), str(e.value)

    # before a window was set
    refused("tfft_stft_plan_set_window", d_x.data_ptr(), d_out.data_ptr(), d_out.data_ptr() + 2 * st.PITCH)
    plan.set_window(torch.ones(st.N, dtype=torch.float16, device=DEV))
    # a pointer that is not 16-byte aligned: each of the three
    refused("16-byte aligned", d_x.data_ptr() + 2, d_out.data_ptr(), d_out.data_ptr() + 2 * st.PITCH)
    refused("16-byte aligned", d_x.data_ptr(), d_out.data_ptr() + 8, d_out.data_ptr() + 2 * st.PITCH)
    refused("16-byte aligned", d_x.data_ptr(), d_out.data_ptr(), d_out.data_ptr() + 2 * st.PITCH + 2)
    # an output plane inside the input, the input inside the output, and the two planes on each other
    refused("input and output overlap", d_x.data_ptr(), d_x.data_ptr(), d_out.data_ptr())
    refused("input and output overlap", d_x.data_ptr(), d_out.data_ptr(), d_x.data_ptr() + 2 * length)
    refused("input and output overlap", d_out.data_ptr() + 16, d_out.data_ptr(), d_out.data_ptr() + 2 * st.PITCH)
    refused("RE and IM output planes overlap", d_x.data_ptr(), d_out.data_ptr(), d_out.data_ptr())
    refused("RE and IM output planes overlap", d_x.data_ptr(), d_out.data_ptr(), d_out.data_ptr() + 2 * 2048)
    torch.cuda.synchronize()
    assert (d_out.view(torch.int16) == de.SENTINEL).all() and not d_x.any()
    # and the call that is legal runs
    plan.exec_ptr(d_x.data_ptr(), d_out.data_ptr(), d_out.data_ptr() + 2 * st.PITCH)
    torch.cuda.synchronize()
    assert not d_out.view(-1)[:total * 2 * st.PITCH].view(total, 2, st.PITCH)[:, :, :st.BINS].any()
    plan.close()


def test_example_runs():
    exe = os.path.join(ROOT, "examples", "example_stft")
    assert os.path.exists(exe), "build() did not build examples/example_stft"
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("OK"), run.stdout + run.stderr
