"""Spectrogram plans on the GPU (tfft_spec_*, include/tfft_spec.h): the power of every bin and the energies of bands of it, from the
one-pass short-frame STFT, at n = 512, 1024 and 2048. Every case is held to

  1. the float32 restatement of tests/spec_ref.py on the binary16 (re, im) that TfftShortStftPlan writes for the same input in the
     same process (code that is already validated, not the code under test), in every bit: power with gain 1 and gain n^2, bands by
     the sequential sum;
  2. the layout: output prefilled with a NaN bit pattern and a stride beyond what a frame holds; the floats behind bin n / 2, behind
     band B - 1 and between frames come back bit for bit, and so do the guard zones around the buffer;
  3. fp64 on the pad-0 shapes, frame by frame, by the bounds spec_ref derives (the worst ratios go to profiles/spec_ulps.txt).

A fresh compute unit's LDS may read as zero and a band kernel leaves powers where the next group's frames go: in the last shape of
spec_ref.shapes(n) ONE wave takes all 2, 4 and 7 groups of the launch.

Measured on the MI355X (seed 1, gain n^2), worst frame of the two pad-0 shapes: sum |P - P64| / sum P64 = 5.3e-04 .. 5.6e-04 at all
three n (0.18 .. 0.19 of the bound), the band sets 0.001 .. 0.12 of theirs (profiles/spec_ulps.txt)."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import dist_emulate as de
import spec_ref as sr
import stftn_ref as sn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NAN_BITS = 0x7FC5A5A5              # a float32 NaN payload no kernel writes
GUARD = 1024                       # sentinel floats before and after an output
SETS = ("mel80", "all", "edges", "desc37")


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    return tensor_fft_amd


def _bands(tf, band_list):
    return tf.Bands(*sr.arrays_of(band_list))


_half = {}


def half_spectra(tf, n, shape):
    """(x, w, re, im): the case's data and what TfftShortStftPlan writes for it, [G, bins] float16; computed once, left unchanged"""
    key = (n, shape)
    if key not in _half:
        rows, length, hop, pad, _ = sr.shapes(n)[shape]
        x, w = sn.case_data(n, rows, length)
        plan = tf.TfftShortStftPlan(n, rows, length, hop, pad)
        total, pitch, bins = rows * plan.frames, sn.pitch(n), sn.bins(n)
        plan.set_window(torch.tensor(w, device=DEV))
        d_out = torch.zeros(total * 2 * pitch, dtype=torch.float16, device=DEV)
        plan.exec(torch.tensor(x, device=DEV).view(-1), d_out, d_out[pitch:])
        torch.cuda.synchronize()
        s = d_out.cpu().numpy().reshape(total, 2, pitch)
        plan.close()
        re, im = s[:, 0, :bins].copy(), s[:, 1, :bins].copy()
        for a in (x, w, re, im):
            a.setflags(write=False)
        _half[key] = (x, w, re, im)
    return _half[key]


def run_spec(tf, n, shape, gain, band_list=None, extra=0, in_extra=0):
    """run_spec_on for shape `shape` of spec_ref.shapes(n) and its case data"""
    rows, length, hop, pad, iters = sr.shapes(n)[shape]
    x, w, _, _ = half_spectra(tf, n, shape)
    return run_spec_on(tf, n, x, w, hop, pad, iters, gain, band_list, extra, in_extra)


def run_spec_on(tf, n, x, w, hop, pad, iters, gain, band_list=None, extra=0, in_extra=0):
    """One execution on the signals x [R, L] under the window w into a NaN-prefilled buffer between guard zones, frame stride =
    default + extra, signal stride = L + in_extra (NaN halves in the gaps). Returns the [G, per_frame] uint32 bit patterns. Checks on
    the way: the guards and every float a frame does not hold untouched, one launch of the one kernel."""
    rows, length = x.shape
    nb = len(band_list) if band_list else 0
    per_frame = nb or sn.bins(n)
    stride = (nb or sn.pitch(n)) + extra
    plan = tf.TfftSpectrogramPlan(n, rows, length, hop, pad, bands=nb, gain=gain, out_frame_stride=stride if extra else 0,
                                  in_sig_stride=length + in_extra if in_extra else 0, launch_iters=iters)
    total = rows * plan.frames
    assert plan.frames == sn.geometry(n, length, hop, pad) and plan.out_frame_stride == stride and plan.per_frame == per_frame
    assert plan.num_launches == 1 and plan.kernels == [f"spec256r::spec_kernel<{n // 256}, {'true' if nb else 'false'}>"]
    d_w = torch.tensor(w, device=DEV)
    plan.set_window(d_w)
    if nb:
        plan.set_bands(_bands(tf, band_list))
    torch.cuda.synchronize()
    d_w.fill_(float("nan"))                    # the plan owns its copy
    host_in = np.full((rows - 1) * (length + in_extra) + length, de.SENTINEL, np.int16)
    idx_in = (np.arange(rows) * (length + in_extra))[:, None] + np.arange(length)[None, :]
    host_in[idx_in] = x.view(np.int16)
    d_in = torch.from_numpy(host_in).to(DEV).view(torch.float16)
    n_out = (total - 1) * stride + per_frame
    d_out = torch.from_numpy(np.full(GUARD + n_out + GUARD, NAN_BITS, np.uint32).view(np.int32)).to(DEV).view(torch.float32)
    plan.exec(d_in, d_out[GUARD:GUARD + n_out])
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    assert (out[:GUARD] == NAN_BITS).all() and (out[-GUARD:] == NAN_BITS).all(), "output guard zone written"
    body = out[GUARD:GUARD + n_out]
    idx = (np.arange(total) * stride)[:, None] + np.arange(per_frame)[None, :]
    written = np.zeros(n_out, bool)
    written[idx.reshape(-1)] = True
    assert (body[~written] == NAN_BITS).all(), "floats a frame does not hold were written"
    assert np.array_equal(d_in.cpu().numpy().view(np.int16), host_in), "input changed"
    plan.close()
    return body[idx]


def _assert_bits(what, got, want):
    want = np.ascontiguousarray(want).view(np.uint32)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} floats differ from the restatement, first (frame, index) = {bad[:3].tolist()}"


_power = {}


def power_bits(tf, n, shape, gain):
    key = (n, shape, gain)
    if key not in _power:
        _power[key] = run_spec(tf, n, shape, gain, extra=8)          # a frame every pitch + 8 floats
    return _power[key]


@pytest.mark.parametrize("gain", ["one", "n2"])
@pytest.mark.parametrize("shape", range(5))
@pytest.mark.parametrize("n", sr.LENGTHS)
def test_power_is_the_restatement_on_short_stfts_halves(tf, n, shape, gain):
    g = 1.0 if gain == "one" else float(n) ** 2
    _, _, re, im = half_spectra(tf, n, shape)
    got = power_bits(tf, n, shape, g)
    assert not np.isnan(got.view(np.float32)).any()
    _assert_bits(f"power n={n} shape {sr.shapes(n)[shape]} gain {g:g}", got, sr.power(re, im, g))


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("shape", range(5))
@pytest.mark.parametrize("n", sr.LENGTHS)
def test_bands_are_the_sequential_restatement(tf, n, shape, name):
    band_list = sr.band_sets(n)[name]
    g = float(n) ** 2
    _, _, re, im = half_spectra(tf, n, shape)
    got = run_spec(tf, n, shape, g, band_list, extra=3)              # a frame every B + 3 floats
    _assert_bits(f"bands {name} n={n} shape {sr.shapes(n)[shape]}", got, sr.band_energies(sr.power(re, im, g), band_list))


@pytest.mark.parametrize("n", sr.LENGTHS)
def test_default_strides_and_gain_one_bands(tf, n):
    """the default frame strides (pitch, B) and a band plan at gain 1"""
    _, _, re, im = half_spectra(tf, n, 0)
    _assert_bits(f"power n={n}, default stride", run_spec(tf, n, 0, 1.0), sr.power(re, im, 1.0))
    band_list = sr.band_sets(n)["mel80"]
    _assert_bits(f"mel80 n={n}, default stride, gain 1", run_spec(tf, n, 0, 1.0, band_list), sr.band_energies(sr.power(re, im, 1.0), band_list))


@pytest.mark.parametrize("n", sr.LENGTHS)
def test_a_strided_input_gives_the_dense_bits(tf, n):
    """in_sig_stride = L + 64 with NaN halves between the signals: a read outside a signal would poison a frame"""
    for shape in (0, 2):
        _, _, re, im = half_spectra(tf, n, shape)
        g = float(n) ** 2
        _assert_bits(f"power n={n} shape {shape}, strided input", run_spec(tf, n, shape, g, in_extra=64), sr.power(re, im, g))
        band_list = sr.band_sets(n)["desc37"]
        _assert_bits(f"desc37 n={n} shape {shape}, strided input", run_spec(tf, n, shape, g, band_list, in_extra=64),
                     sr.band_energies(sr.power(re, im, g), band_list))


_ratios = {}


@pytest.mark.parametrize("n", sr.LENGTHS)
def test_accuracy_against_fp64(tf, n):
    """Per frame of the pad-0 shapes against fp64 of the binary16 products: sum |P - P64| <= POWER_BOUND * sum P64, and the bands
    within spec_ref.band_bound (every set has non-negative weights)."""
    nbins = sn.bins(n)
    g = float(n) ** 2
    for shape in sr.ACCURACY_SHAPES:
        rows, length, hop, pad, _ = sr.shapes(n)[shape]
        x, w, re, im = half_spectra(tf, n, shape)
        want = sr.p64(n, x, w, hop, pad, g)
        got = power_bits(tf, n, shape, g).view(np.float32).astype(np.float64)
        ratio = (np.abs(got - want).sum(-1) / want.sum(-1)).max()
        _ratios[(n, shape, "power")] = ratio / sr.POWER_BOUND
        print(f"spec n={n} shape {shape}: worst frame sum|P - P64| / sum P64 = {ratio:.3e} (bound {sr.POWER_BOUND:.3e})")
        assert ratio <= sr.POWER_BOUND
        for name in SETS:
            band_list = sr.band_sets(n)[name]
            bound, e64 = sr.band_bound(want, band_list, nbins)
            e = run_spec(tf, n, shape, g, band_list).view(np.float32).astype(np.float64)
            worst = (np.abs(e - e64).sum(-1) / bound).max()
            _ratios[(n, shape, name)] = worst
            print(f"spec n={n} shape {shape} {name}: worst frame sum|E - E64| / bound = {worst:.3e}")
            assert worst <= 1.0
    if len(_ratios) == len(sr.LENGTHS) * len(sr.ACCURACY_SHAPES) * (1 + len(SETS)):
        lines = ["# tests/test_gpu_spec.py::test_accuracy_against_fp64: worst frame of each pad-0 shape, error / bound against fp64 of the",
                 "# binary16 products (tests/spec_ref.py: POWER_BOUND for the power, band_bound for a band set), gain n^2, seed 1",
                 "# n shape what error/bound"]
        lines += [f"{k[0]} {k[1]} {k[2]} {v:.4f}" for k, v in sorted(_ratios.items())]
        try:
            with open(os.path.join(ROOT, "profiles", "spec_ulps.txt"), "w") as f:
                f.write("\n".join(lines) + "\n")
        except OSError as e:                      # a read-only checkout: the figures are in the output above
            print(f"profiles/spec_ulps.txt not written: {e}")


@pytest.mark.parametrize("n", sr.LENGTHS)
def test_two_executions_and_a_graph_replay_give_the_same_bits(tf, n):
    shape = 1
    rows, length, hop, pad, _ = sr.shapes(n)[shape]
    x, w, re, im = half_spectra(tf, n, shape)
    g = float(n) ** 2
    band_list = sr.band_sets(n)["mel80"]
    d_x = torch.tensor(x, device=DEV).view(-1)
    for nb, want in ((0, sr.power(re, im, g)), (80, sr.band_energies(sr.power(re, im, g), band_list))):
        plan = tf.TfftSpectrogramPlan(n, rows, length, hop, pad, bands=nb, gain=g)
        plan.set_window(torch.tensor(w, device=DEV))
        if nb:
            plan.set_bands(_bands(tf, band_list))
        total, stride, per = rows * plan.frames, plan.out_frame_stride, plan.per_frame
        outs = [torch.zeros(total * stride, dtype=torch.float32, device=DEV) for _ in range(3)]
        plan.exec(d_x, outs[0])
        plan.exec(d_x, outs[1])
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                plan.exec(d_x, outs[2])
        torch.cuda.synchronize()
        assert not outs[2].any(), "a captured execution ran at capture time"
        graph.replay()
        torch.cuda.synchronize()
        for o in outs:
            _assert_bits(f"n={n} bands={nb}", o.cpu().numpy().view(np.uint32).reshape(total, stride)[:, :per], want)
        del graph
        plan.close()


@pytest.mark.parametrize("n", sr.LENGTHS)
def test_tensor_functions_and_their_caches(tf, n, monkeypatch):
    spec_mod = importlib.import_module("tensor_fft_amd.spec")
    windows, bands_set = [], []
    real_w, real_b = spec_mod.TfftSpectrogramPlan.set_window, spec_mod.TfftSpectrogramPlan.set_bands
    monkeypatch.setattr(spec_mod.TfftSpectrogramPlan, "set_window", lambda self, w, stream=None: (windows.append(1), real_w(self, w, stream))[1])
    monkeypatch.setattr(spec_mod.TfftSpectrogramPlan, "set_bands", lambda self, b, stream=None: (bands_set.append(1), real_b(self, b, stream))[1])
    tf.spec_cache_clear()
    shape = 2                                                    # (2, n, 160, n / 2): center=True is pad = n / 2
    rows, length, hop, pad, _ = sr.shapes(n)[shape]
    x, w, re, im = half_spectra(tf, n, shape)
    frames, bins, g = sn.geometry(n, length, hop, pad), sn.bins(n), float(n) ** 2
    d_x, d_w = torch.tensor(x, device=DEV), torch.tensor(w, device=DEV)
    p = tf.power_spectrogram(d_x, d_w, hop, n, center=True, gain=g)
    assert p.shape == (rows, frames, bins) and p.dtype == torch.float32
    _assert_bits("power_spectrogram", p.cpu().numpy().view(np.uint32).reshape(-1, bins), sr.power(re, im, g))
    tf.power_spectrogram(d_x, d_w, hop, n, center=True, gain=g)
    assert len(windows) == 1                                     # the same window again: not handed over
    tf.power_spectrogram(d_x, d_w, hop, n, center=True)          # another gain is another plan
    assert len(windows) == 2
    band_list = sr.band_sets(n)["mel80"]
    mel = tf.mel_bands(n, 16000, 80)
    want = sr.band_energies(sr.power(re, im, g), band_list)
    e = tf.band_spectrogram(d_x, d_w, hop, n, mel, center=True, gain=g)
    assert e.shape == (rows, frames, 80) and e.dtype == torch.float32 and e.is_contiguous()
    _assert_bits("band_spectrogram", e.cpu().numpy().view(np.uint32).reshape(-1, 80), want)
    assert (len(windows), len(bands_set)) == (3, 1)
    tf.band_spectrogram(d_x, d_w, hop, n, mel, center=True, gain=g)
    assert (len(windows), len(bands_set)) == (3, 1)              # the same window and Bands object: neither handed over
    other = _bands(tf, [(s, (wt * np.float32(0.5))) for s, wt in band_list])     # halved weights: every product and sum scales exactly
    h = tf.band_spectrogram(d_x, d_w, hop, n, other, center=True, gain=g)
    assert (len(windows), len(bands_set)) == (3, 2)              # another Bands object of as many bands: handed over to the same plan
    _assert_bits("band_spectrogram, other bands", h.cpu().numpy().view(np.uint32).reshape(-1, 80), want * np.float32(0.5))
    d_w.mul_(0.5)                                                # the window modified in place: handed over again
    tf.band_spectrogram(d_x, d_w, hop, n, other, center=True, gain=g)
    assert (len(windows), len(bands_set)) == (4, 2)
    with pytest.raises(tf.TfftError):
        tf.power_spectrogram(d_x, d_w, hop, 4096)
    with pytest.raises(tf.TfftError):
        tf.band_spectrogram(d_x, d_w, hop, n, sr.dense_of(band_list, bins))      # a matrix is not a Bands object
    tf.spec_cache_clear()


def test_refusals_of_bands_and_executions_leave_the_output_untouched(tf):
    n, rows, length, hop = 1024, 2, 4096, 256
    plan = tf.TfftSpectrogramPlan(n, rows, length, hop, bands=3)
    power_plan = tf.TfftSpectrogramPlan(n, rows, length, hop)
    total = rows * plan.frames
    d_x = torch.zeros(rows * length + 8, dtype=torch.float16, device=DEV)
    d_out = torch.from_numpy(np.full(total * sn.pitch(n) + 8, NAN_BITS, np.uint32).view(np.int32)).to(DEV).view(torch.float32)

    def refused(needle, call, *args):
        with pytest.raises(tf.TfftError) as e:
            call(*args)
        assert needle in str(e.value), str(e.value)

    good = tf.Bands([0, 5, 512], [2, 3, 1], np.ones(6, np.float32))
    refused("tfft_spec_plan_set_window", plan.exec_ptr, d_x.data_ptr(), d_out.data_ptr())
    plan.set_window(torch.ones(n, dtype=torch.float16, device=DEV))
    power_plan.set_window(torch.ones(n, dtype=torch.float16, device=DEV))
    refused("tfft_spec_plan_set_bands", plan.exec_ptr, d_x.data_ptr(), d_out.data_ptr())
    refused("takes no bands", power_plan.set_bands, good)
    refused("created for 3 bands", plan.set_bands, tf.Bands([0, 5], [2, 3], np.ones(5, np.float32)))
    refused("count 0", plan.set_bands, tf.Bands([0, 5, 512], [2, 0, 4], np.ones(6, np.float32)))
    refused("reaches past bin n / 2 = 512", plan.set_bands, tf.Bands([0, 5, 512], [2, 2, 2], np.ones(6, np.float32)))
    refused("reaches past bin n / 2 = 512", plan.set_bands, tf.Bands([0, 513, 5], [2, 1, 3], np.ones(6, np.float32)))
    refused("reaches past bin n / 2 = 512", plan.set_bands, tf.Bands([0, 2 ** 32 - 1, 5], [2, 2, 2], np.ones(6, np.float32)))
    for bad in (np.inf, -np.inf, np.nan):
        weights = np.ones(6, np.float32)
        weights[4] = bad
        refused("weight 4 is not finite", plan.set_bands, tf.Bands([0, 5, 512], [2, 3, 1], weights))
    refused("tfft_spec_plan_set_bands", plan.exec_ptr, d_x.data_ptr(), d_out.data_ptr())      # a refused set_bands set nothing
    plan.set_bands(good)
    for p in (plan, power_plan):
        refused("16-byte aligned", p.exec_ptr, d_x.data_ptr() + 2, d_out.data_ptr())
        refused("16-byte aligned", p.exec_ptr, d_x.data_ptr(), d_out.data_ptr() + 4)
        refused("null data pointer", p.exec_ptr, None, d_out.data_ptr())
        refused("input and output overlap", p.exec_ptr, d_x.data_ptr(), d_x.data_ptr())
        refused("input and output overlap", p.exec_ptr, d_x.data_ptr(), d_x.data_ptr() + 2 * rows * length - 16)
        refused("input and output overlap", p.exec_ptr, d_out.data_ptr() + 16, d_out.data_ptr())
    with pytest.raises(tf.TfftError):
        plan.exec(d_x, d_out.view(torch.int32))
    with pytest.raises(tf.TfftError):
        plan.exec(d_x, d_out[:total * 3 - 1])
    torch.cuda.synchronize()
    assert (d_out.view(torch.int32) == int(np.uint32(NAN_BITS).view(np.int32))).all() and not d_x.any()
    # and the calls that are legal run: all-zero signals have no power
    plan.exec(d_x, d_out)
    torch.cuda.synchronize()
    assert not d_out[:total * 3].any()
    power_plan.exec(d_x, d_out)
    torch.cuda.synchronize()
    assert not d_out[:total * sn.pitch(n)].view(total, sn.pitch(n))[:, :sn.bins(n)].any()
    plan.close()
    power_plan.close()


def test_example_runs():
    exe = os.path.join(ROOT, "examples", "example_spec")
    assert os.path.exists(exe), "build() did not build examples/example_spec"
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("OK"), run.stdout + run.stderr
