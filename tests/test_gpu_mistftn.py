"""Masked short-frame ISTFT plans on the GPU (tfft_mistftn_*, include/tfft_mistftn.h) and the gradients built on them
(tensor-fft_amd/stft_autograd.py). The cases are tests/istftn_ref.cases(n) at n = 512, 1024 and 2048, the smallest shapes at which
pairing, ragged groups, self-pairing, trimming and wave loops go wrong. Every execution runs between guard zones with padded strides
(spectra 2 h + 16, mask h + 16, output L + 64), NaN sentinels in everything that must not be read (the halves beyond bin n / 2 of every
spectrum and mask frame, the gaps, the IM of bins 0 and n / 2) and a caller's NaN-prefilled workspace of (R F + 1) n halves, and
asserts: guards intact, spectra and mask bit-identical afterwards, nothing written outside [0, L) of each signal and outside R F n
halves of the workspace. Results are held to

  1. frames: the workspace equals, bit for bit, the shipped TfftPlan(n, items, 0).exec_inverse on tests/mistftn_ref.merge_items_masked
     of the inputs; output: y equals tests/istftn_ref.ola of those workspace frames; per frame and per bin, divided and raw,
  2. a mask of ones: the frames and the output of TfftShortIstftPlan, in every bit,
  3. a mask drawn from {0, +-1, +-2}: TfftShortIstftPlan's bits on the planes multiplied on the host,
  4. launch_iters: never a bit,
  5. fp64, and the two-pass path re * M, im * M in torch -> TfftShortIstftPlan beside it, to the same bound,
  6. / 7. the gradients of short_stft and power_spectrogram against the fp64 adjoint and float64 torch autograd,
  8. - 11. graph capture, the refusals that need a device, masked_istft / mask_buffer, the example.

A fresh compute unit's LDS may read as zero, so a slot of the image the merge misses shows only from a wave's second group on: the
cases with launch_iters make the waves loop (tests/test_gpu_istftn.py has the note)."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import dist_emulate as de
import istftn_ref as inr
import mistftn_ref as mr
import stftn_ref as sn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_istftn as tn  # noqa: E402  (its helpers: the inputs of a case, the shipped inverse plan, the bound)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LENGTHS = mr.LENGTHS
CASES = tn.CASES
MODES = ("frame", "bin")
K_C2R, K_FWD = tn.K_C2R, tn.K_FWD
K_MASK = 2.0 ** -10            # the rounding of a mask entry M / s to binary16, relative (2^-11) with room for its subnormals


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    return tensor_fft_amd


def _mask_stride(n):
    return sn.pitch(n) + 16


def _flat_mask(n, mask):
    """[G][n / 2 + 1] -> flat int16, frame g at g * (h + 16); [n / 2 + 1] -> h halves. NaN sentinels beyond bin n / 2 and in the gaps"""
    bins, pitch = sn.bins(n), sn.pitch(n)
    if mask.ndim == 1:
        flat = np.full(pitch, de.SENTINEL, dtype=np.int16)
        flat[:bins] = mask.view(np.int16)
        return flat
    total, stride = mask.shape[0], _mask_stride(n)
    flat = np.full((total - 1) * stride + pitch, de.SENTINEL, dtype=np.int16)
    flat[(np.arange(total) * stride)[:, None] + np.arange(bins)[None, :]] = mask.view(np.int16)
    return flat


def run_mistftn(tf, n, re, im, mask, w, rows, length, hop, pad, launch_iters=0, raw=False):
    """tn.run_istftn with the mask: one execution between guard zones with padded strides and a caller's workspace. Returns (frames
    [R * F][n], y [R][L]) as int16 bit patterns. mask [R * F][n / 2 + 1] (a per-frame plan) or [n / 2 + 1] (per bin)."""
    out_stride, per_bin = length + 64, mask.ndim == 1
    plan = tf.TfftMaskedIstftPlan(n, rows, length, hop, pad, 0, in_frame_stride=tn._in_stride(n), mask_frame_stride=0 if per_bin else _mask_stride(n),
                                  out_sig_stride=out_stride, launch_iters=launch_iters, raw_sum=raw, per_bin=per_bin)
    total = rows * plan.frames
    assert plan.frames == inr.geometry(n, length, hop, pad) and re.shape == im.shape == (total, sn.bins(n))
    assert plan.num_launches == 2 and plan.kernels == [f"mistft256r::frames_kernel<{n // 256}>", "olan::ola_kernel"]
    assert plan.workspace_bytes() == total * n * 2
    d_w = torch.from_numpy(w.copy()).to(DEV)
    plan.set_window(d_w)
    torch.cuda.synchronize()
    d_w.fill_(float("nan"))
    host_in, host_mask = tn._flat_spectra(n, re, im), _flat_mask(n, mask)
    n_in, n_mask, n_out, n_ws = host_in.size, host_mask.size, (rows - 1) * out_stride + length, (total + 1) * n
    assert plan.mask_halves <= n_mask
    d_in = de._guarded(torch, n_in, host_in.view(np.float16))
    d_mask = de._guarded(torch, n_mask, host_mask.view(np.float16))
    d_out = de._guarded(torch, n_out)
    d_ws = de._guarded(torch, n_ws)
    g = de.GUARD
    plan.set_workspace(d_ws[g:g + n_ws])
    body = d_in[g:g + n_in]
    plan.exec(body, body[sn.pitch(n):], d_mask[g:g + n_mask], d_out[g:g + n_out])
    torch.cuda.synchronize()
    assert de._guards_intact(torch, d_out), "output guard zone written"
    assert de._guards_intact(torch, d_ws), "workspace guard zone written"
    assert de._guards_intact(torch, d_in) and de._guards_intact(torch, d_mask)
    de._untouched(body.cpu().numpy().view(np.int16), host_in, "input spectra")
    de._untouched(d_mask[g:g + n_mask].cpu().numpy().view(np.int16), host_mask, "mask")
    ws = d_ws[g:g + n_ws].cpu().numpy().view(np.int16)
    assert (ws[total * n:] == de.SENTINEL).all(), "workspace written beyond R F * n halves"
    out = d_out[g:g + n_out].cpu().numpy().view(np.int16)
    idx = (np.arange(rows) * out_stride)[:, None] + np.arange(length)[None, :]
    written = np.zeros(n_out, bool)
    written[idx.reshape(-1)] = True
    assert (out[~written] == de.SENTINEL).all(), "gaps between the output signals written"
    plan.close()
    return ws[:total * n].reshape(total, n).copy(), out[idx]


_masks, _results, _wanted = {}, {}, {}


def mask_of(n, rows, length, hop, pad, mode, kind="random"):
    """the mask of one shape, computed once per module and left unchanged: kind "random" (mistftn_ref.random_mask with its planted
    values), "unit" (random in [0, 1], nothing planted), "ones" or "sign" ({0, +-1, +-2})"""
    key = (n, rows, length, hop, pad, mode, kind)
    if key not in _masks:
        total = rows * inr.geometry(n, length, hop, pad)
        shape = (sn.bins(n),) if mode == "bin" else (total, sn.bins(n))
        seed = n + 7 * total + (1 if mode == "bin" else 0)
        _masks[key] = {"random": lambda: mr.random_mask(shape, seed), "unit": lambda: mr.random_mask(shape, seed, planted=False),
                       "ones": lambda: np.ones(shape, np.float16), "sign": lambda: mr.sign_mask(shape, seed)}[kind]()
        _masks[key].setflags(write=False)
    return _masks[key]


def result(tf, n, rows, length, hop, pad, iters, window, mode, raw=False, kind="random"):
    """(frames, y) of one case, computed once per module"""
    key = (n, rows, length, hop, pad, iters, window, mode, raw, kind)
    if key not in _results:
        _, w, re, im = tn.inputs(n, rows, length, hop, pad, window)
        _results[key] = run_mistftn(tf, n, re, im, mask_of(n, rows, length, hop, pad, mode, kind), w, rows, length, hop, pad, iters, raw)
    return _results[key]


def wanted_frames(tf, n, rows, length, hop, pad, window, mode, kind="random"):
    """the reference of comparison 1, computed once per shape and mask and left unchanged"""
    key = (n, rows, length, hop, pad, window, mode, kind)
    if key not in _wanted:
        _, _, re, im = tn.inputs(n, rows, length, hop, pad, window)
        zr, zi = mr.merge_items_masked(re, im, mask_of(n, rows, length, hop, pad, mode, kind), n)
        _wanted[key] = tn.via_inverse_plan(tf, n, zr, zi, re.shape[0])
        _wanted[key].setflags(write=False)
    return _wanted[key]


def _check_case(tf, n, rows, length, hop, pad, iters, window, mode, raw=False):
    _, w, _, _ = tn.inputs(n, rows, length, hop, pad, window)
    frames, y = result(tf, n, rows, length, hop, pad, iters, window, mode, raw)
    what = f"mistft n={n} R={rows} L={length} hop={hop} pad={pad} iters={iters} {window} per {mode}{' raw' if raw else ''}"
    assert not np.isnan(frames.view(np.float16)).any(), what + ": a NaN of the padding of the spectra or the mask reached the frames"
    tn._assert_bits(what + ", frames against merge_items_masked -> TfftPlan.exec_inverse", frames, wanted_frames(tf, n, rows, length, hop, pad, window, mode))
    want_y = inr.ola(frames.view(np.float16), w, n, rows, length, hop, pad, raw=raw).view(np.int16)
    tn._assert_bits(what + ", output against istftn_ref.ola of the workspace frames", y, want_y, ("signal", "sample"))
    return frames, y


# ---- 1
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,rows,length,hop,pad,iters,window", CASES)
def test_frames_and_output_bit_for_bit(tf, n, rows, length, hop, pad, iters, window, mode):
    _, w, _, _ = tn.inputs(n, rows, length, hop, pad, window)
    frames, y = _check_case(tf, n, rows, length, hop, pad, iters, window, mode)
    bare = inr.envelope(w, n, length, hop, pad) == 0
    assert (y[:, bare] == 0).all(), "a sample no frame covers must be +0"
    assert np.isfinite(y.view(np.float16)).all()
    # the mask does something: the unmasked plan's frames differ
    assert (frames != tn.result(tf, n, rows, length, hop, pad, iters, window)[0]).any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,rows,length,hop,pad,iters,window", CASES)
def test_raw_sum_bit_for_bit(tf, n, rows, length, hop, pad, iters, window, mode):
    _, y = _check_case(tf, n, rows, length, hop, pad, iters, window, mode, raw=True)
    _, divided = result(tf, n, rows, length, hop, pad, iters, window, mode)
    assert (y != divided).any()          # the flag does something


# ---- 2
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,rows,length,hop,pad,iters,window", CASES)
def test_a_mask_of_ones_gives_the_unmasked_plans_bits(tf, n, rows, length, hop, pad, iters, window, mode):
    frames, y = result(tf, n, rows, length, hop, pad, iters, window, mode, kind="ones")
    want_frames, want_y = tn.result(tf, n, rows, length, hop, pad, iters, window)
    what = f"mistft n={n} R={rows} L={length} hop={hop} pad={pad} per {mode}, a mask of ones against TfftShortIstftPlan"
    tn._assert_bits(what + ", frames", frames, want_frames)
    tn._assert_bits(what + ", output", y, want_y, ("signal", "sample"))


# ---- 3
@pytest.mark.parametrize("n,rows,length,hop,pad,iters,window", CASES)
def test_a_mask_of_signs_and_doublings_is_exact(tf, n, rows, length, hop, pad, iters, window):
    _, w, re, im = tn.inputs(n, rows, length, hop, pad, window)
    m = mask_of(n, rows, length, hop, pad, "frame", "sign")
    pre_re, pre_im = (m.astype(np.float32) * re).astype(np.float16), (m.astype(np.float32) * im).astype(np.float16)
    assert np.isfinite(pre_re).all() and np.isfinite(pre_im).all() and set(np.unique(m).tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    frames, y = result(tf, n, rows, length, hop, pad, iters, window, "frame", kind="sign")
    want_frames, want_y = tn.run_istftn(tf, n, pre_re, pre_im, w, rows, length, hop, pad, iters)
    what = f"mistft n={n} R={rows} L={length} hop={hop} pad={pad}, a mask of 0, +-1, +-2 against TfftShortIstftPlan on the premultiplied planes"
    tn._assert_bits(what + ", frames", frames, want_frames)
    tn._assert_bits(what + ", output", y, want_y, ("signal", "sample"))


# ---- 4
@pytest.mark.parametrize("iters", [0, 1, 3, 65535])
@pytest.mark.parametrize("n", LENGTHS)
def test_launch_iters_never_changes_a_bit(tf, n, iters):
    rows, length, hop, pad = sn.looping_case(n)
    for mode in MODES:
        _check_case(tf, n, rows, length, hop, pad, iters, "random", mode)


# ---- 5
@pytest.mark.parametrize("n", LENGTHS)
def test_accuracy_against_fp64(tf, n):
    """Per signal, rel-L2 against the fp64 ISTFT of the fp64-masked binary16 spectra (mistftn_ref.istft64_masked), Hann window, shapes
    (3, 2n, n / 4, n / 2) and (4, 3n, n / 4, n / 2), a random per-frame mask in [0, 1]. The bound is tests/test_gpu_istftn.py's
    _accuracy_bound, K sqrt(2 env_max / env_min) + 2^-11 = 2.81e-03: the error of the output is e_y = sum w e_f / sum w^2 with e_f the
    error of frame f; a pair's frames come out of one C2R whose rel-L2 error against fp64 is at most K = 1.5e-3 of the PAIR (hence the
    factor 2 for the weaker frame), Cauchy-Schwarz over the covering frames gives |e_y| <= K sqrt(2 env_max / env_min) |y|, and 2^-11
    is the rounding of the output. A mask with |m| <= 1 does not enlarge a pair's error: the masked merge rounds Z' once, as the
    unmasked one does, relative to the MASKED spectrum, which is the reference's input too. The two-pass path (b), re * M and im * M
    rounded to binary16 in torch and then TfftShortIstftPlan, is held to the same bound in the same test; its extra rounding of the
    products is inside K's margin.
    Measured on the MI355X, worst signal, (a) the masked plan / (b) the torch products: 3.37e-04 / 3.63e-04 (n = 512, 3 x 1024),
    3.44e-04 / 3.67e-04 (512, 4 x 1536), 3.40e-04 / 3.58e-04 (1024, 3 x 2048), 3.36e-04 / 3.62e-04 (1024, 4 x 3072), 3.35e-04 /
    3.56e-04 (2048, 3 x 4096), 3.35e-04 / 3.57e-04 (2048, 4 x 6144) (profiles/mistftn_ulps.txt)."""
    lines = []
    for rows, length, hop, pad in inr.accuracy_shapes(n):
        _, w, re, im = tn.inputs(n, rows, length, hop, pad, "hann")
        m = mask_of(n, rows, length, hop, pad, "frame", "unit")
        assert m.min() >= 0 and m.max() <= 1
        _, y = result(tf, n, rows, length, hop, pad, 0, "hann", "frame", kind="unit")
        bound = tn._accuracy_bound(w, n, length, hop, pad)
        want = mr.istft64_masked(re, im, m, w, rows, length, hop, pad)
        e_a = inr.rel_l2(y.view(np.float16), want).max()
        # (b): two torch passes over both planes, then the unmasked plan
        d_re, d_im = tn._stft_layout(n, re, im, rows)
        d_m = torch.from_numpy(m.copy()).to(DEV).reshape(d_re.shape)
        d_w = torch.from_numpy(w.copy()).to(DEV)
        y_b = tf.short_istft(d_re * d_m, d_im * d_m, d_w, hop, length, n, center=True).cpu().numpy()
        e_b = inr.rel_l2(y_b, want).max()
        # and masked_istft is path (a)
        y_f = tf.masked_istft(d_re, d_im, d_m, d_w, hop, length, n, center=True).cpu().numpy()
        assert np.array_equal(y_f.view(np.int16), y)
        lines.append(f"mistft n={n} R={rows} L={length} hop={hop}: worst signal rel-L2 against the fp64 ISTFT of the fp64-masked binary16 spectra: "
                     f"(a) masked plan {e_a:.2e}, (b) torch products + short_istft {e_b:.2e} (bound {bound:.2e})")
        print(lines[-1])
        tf.istftn_cache_clear()
        tf.mistftn_cache_clear()
        assert e_a <= bound and e_b <= bound


# ---- 6, 7: the gradients
GRAD_SHAPES = [("pad0", lambda n: (3, 3 * n // 2, n // 4, 0), "random"), ("centred", lambda n: (2, 2 * n, n // 2, n // 2), "hann")]


def _grad_bound(w, n, length, hop, pad):
    """dx = sum_f w[j] v_f[j] over the covering frames, v_f the frames of the adjoint. The plan's frames carry errors e_f with
    sum_f |e_f|^2 <= 2 K^2 sum_f |v_f|^2 (K = K_C2R per pair of frames of one C2R, the factor 2 for a pair's weaker frame), and
    Cauchy-Schwarz over the covering frames, |sum_f w[j] e_f[j]|^2 <= (sum_f w[j]^2) (sum_f e_f[j]^2) <= env_max sum_f e_f[j]^2, gives
    |e_dx|_2 <= K sqrt(2 env_max) |v|_2; 2^-11 |dx|_2 is the rounding of the output. Relative to max(|v|_2, |dx|_2)."""
    return K_C2R * np.sqrt(2 * inr.envelope(w, n, length, hop, pad).max()) + 2.0 ** -11


def _per_signal(a, rows):
    return np.sqrt((np.asarray(a, np.float64).reshape(rows, -1) ** 2).sum(-1))


@pytest.mark.parametrize("name,shape,window", GRAD_SHAPES)
@pytest.mark.parametrize("n", LENGTHS)
def test_differentiable_short_stft(tf, n, name, shape, window):
    """Forward: short_stft's bits. Backward: per signal against the fp64 adjoint (mistftn_ref.adjoint64) of the same binary16
    (g_re, g_im), |dx - dx64|_2 <= (K sqrt(2 env_max) + 2^-11) max(|v64|_2, |dx64|_2) (_grad_bound has the derivation).
    Measured on the MI355X, worst signal, pad0 / centred: 2.66e-04 / 2.52e-04 (n = 512; bounds 3.74e-03 / 2.61e-03), 2.74e-04 / 2.48e-04
    (1024; 3.83e-03 / 2.61e-03), 2.57e-04 / 2.42e-04 (2048; 3.89e-03 / 2.61e-03) (profiles/mistftn_ulps.txt)."""
    rows, length, hop, pad = shape(n)
    x, w = sn.case_data(n, rows, length, window=window)
    frames = inr.geometry(n, length, hop, pad)
    rng = np.random.default_rng([29, n, rows])
    g_re, g_im = (rng.uniform(-1, 1, (rows, frames, sn.bins(n))).astype(np.float16) for _ in range(2))
    d_x = torch.from_numpy(x.copy()).to(DEV).requires_grad_(True)
    d_w = torch.from_numpy(w.copy()).to(DEV).requires_grad_(True)
    tf.mistftn_cache_clear()
    re, im = tf.differentiable_short_stft(d_x, d_w, hop, n, center=pad > 0)
    p_re, p_im = tf.short_stft(d_x.detach(), d_w.detach(), hop, n, center=pad > 0)
    assert re.grad_fn is not None and torch.equal(re.view(torch.int16), p_re.view(torch.int16)) and torch.equal(im.view(torch.int16), p_im.view(torch.int16))
    torch.autograd.backward((re, im), (torch.from_numpy(g_re).to(DEV), torch.from_numpy(g_im).to(DEV)))
    assert d_w.grad is None, "the window's gradient is None"
    assert d_x.grad is not None and d_x.grad.shape == d_x.shape and d_x.grad.dtype == torch.float16
    dx = d_x.grad.cpu().numpy()
    flat_re, flat_im = g_re.reshape(rows * frames, -1), g_im.reshape(rows * frames, -1)
    dx64 = mr.adjoint64(flat_re, flat_im, w, rows, length, hop, pad)
    v64 = mr.adjoint_frames64(flat_re, flat_im, n)
    err, scale = _per_signal(dx.astype(np.float64) - dx64, rows), np.maximum(_per_signal(v64, rows), _per_signal(dx64, rows))
    bound = _grad_bound(w, n, length, hop, pad)
    print(f"differentiable_short_stft n={n} {name}: worst signal |dx - dx64| / max(|v64|, |dx64|) = {(err / scale).max():.2e} (bound {bound:.2e})")
    assert np.isfinite(dx).all() and (err <= bound * scale).all()
    # the IM of bins 0 and n / 2 carries no gradient: any value there gives the same bits
    d_x.grad = None
    re, im = tf.differentiable_short_stft(d_x, d_w, hop, n, center=pad > 0)
    g2 = g_im.copy()
    g2[:, :, 0], g2[:, :, n // 2] = 7.0, -3.0
    torch.autograd.backward((re, im), (torch.from_numpy(g_re).to(DEV), torch.from_numpy(g2).to(DEV)))
    assert np.array_equal(d_x.grad.cpu().numpy().view(np.int16), dx.view(np.int16))
    # one cached plan serves both backward passes; an x that does not require grad gets none
    assert len(importlib.import_module("tensor_fft_amd.mistftn")._plans) == 1
    plain = torch.from_numpy(x.copy()).to(DEV)
    re, im = tf.differentiable_short_stft(plain, d_w.detach(), hop, n, center=pad > 0)
    assert not re.requires_grad and plain.grad is None
    tf.mistftn_cache_clear()
    tf.stftn_cache_clear()


def _power64(x, w, n, hop, pad, gain, g_p):
    """float64 torch autograd on the CPU: frames -> rfft / n -> gain |.|^2, backward with g_p. Returns (dx64 [R][L], v64 [R * F][n], the
    gradient with respect to the windowed frames)"""
    rows, length = x.shape
    frames = inr.geometry(n, length, hop, pad)
    tail = max(0, (frames - 1) * hop + n - pad - length)
    x64 = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    u = torch.nn.functional.pad(x64, (pad, tail)).unfold(1, n, hop)[:, :frames] * torch.from_numpy(w.astype(np.float64))
    u.retain_grad()
    s = torch.fft.rfft(u, dim=-1) / n
    p = gain * (s.real ** 2 + s.imag ** 2)
    p.backward(torch.from_numpy(g_p.astype(np.float64)))
    return x64.grad.numpy(), u.grad.numpy().reshape(rows * frames, n)


@pytest.mark.parametrize("name,shape,window", GRAD_SHAPES)
@pytest.mark.parametrize("n", LENGTHS)
def test_differentiable_power_spectrogram(tf, n, name, shape, window):
    """Forward: power_spectrogram's bits. Backward: per signal against float64 torch autograd on the CPU (frames -> rfft / n ->
    gain |.|^2, the same gP), |dx - dx64|_2 <= (K sqrt(2 env_max) + 2^-11 + K_FWD + 2^-10) max(|v64|_2, |dx64|_2): the bound of
    test_differentiable_short_stft, the forward allowance of tests/test_gpu_stftn.py for the recomputed S (1.5e-3 + 2^-10) and 2^-10
    for the rounding of the mask M / s to binary16. gP = 0 gives +0 everywhere (the s = 1 path).
    Measured on the MI355X, worst signal, pad0 (gain 1) / centred (gain n^2): 3.99e-04 / 3.84e-04 (n = 512; bounds 7.19e-03 /
    6.06e-03), 4.06e-04 / 3.79e-04 (1024; 7.28e-03 / 6.06e-03), 4.05e-04 / 3.81e-04 (2048; 7.34e-03 / 6.06e-03)
    (profiles/mistftn_ulps.txt)."""
    rows, length, hop, pad = shape(n)
    gain = 1.0 if pad == 0 else float(n) ** 2
    x, w = sn.case_data(n, rows, length, window=window)
    frames = inr.geometry(n, length, hop, pad)
    g_p = np.random.default_rng([31, n, rows]).uniform(-1, 1, (rows, frames, sn.bins(n))).astype(np.float32)
    d_x = torch.from_numpy(x.copy()).to(DEV).requires_grad_(True)
    d_w = torch.from_numpy(w.copy()).to(DEV).requires_grad_(True)
    p = tf.differentiable_power_spectrogram(d_x, d_w, hop, n, center=pad > 0, gain=gain)
    plain = tf.power_spectrogram(d_x.detach(), d_w.detach(), hop, n, center=pad > 0, gain=gain)
    assert p.grad_fn is not None and p.dtype == torch.float32 and torch.equal(p.view(torch.int32), plain.view(torch.int32))
    p.backward(torch.from_numpy(g_p).to(DEV))
    assert d_w.grad is None and d_x.grad.dtype == torch.float16 and d_x.grad.shape == d_x.shape
    dx = d_x.grad.cpu().numpy()
    dx64, v64 = _power64(x, w, n, hop, pad, gain, g_p)
    err, scale = _per_signal(dx.astype(np.float64) - dx64, rows), np.maximum(_per_signal(v64, rows), _per_signal(dx64, rows))
    bound = _grad_bound(w, n, length, hop, pad) + K_FWD + K_MASK
    print(f"differentiable_power_spectrogram n={n} {name} gain={gain:g}: worst signal |dx - dx64| / max(|v64|, |dx64|) = {(err / scale).max():.2e} "
          f"(bound {bound:.2e})")
    assert np.isfinite(dx).all() and (err <= bound * scale).all()
    # gP = 0: the maximum is 0, s = 1, dx = +0 everywhere and no NaN
    d_x.grad = None
    p = tf.differentiable_power_spectrogram(d_x, d_w, hop, n, center=pad > 0, gain=gain)
    p.backward(torch.zeros_like(p))
    assert not d_x.grad.view(torch.int16).any(), "gP = 0 must give +0 everywhere"
    tf.mistftn_cache_clear()
    tf.stftn_cache_clear()
    tf.spec_cache_clear()


# ---- 8
@pytest.mark.parametrize("n", LENGTHS)
def test_replay_under_graph_capture(tf, n):
    rows, length, hop, pad = 3, 3 * n // 2, n // 4, 0
    _, w, re, im = tn.inputs(n, rows, length, hop, pad, "random")
    _, y = result(tf, n, rows, length, hop, pad, 0, "random", "frame")
    plan = tf.TfftMaskedIstftPlan(n, rows, length, hop, pad, 0, in_frame_stride=tn._in_stride(n), mask_frame_stride=_mask_stride(n))
    plan.set_window(torch.from_numpy(w.copy()).to(DEV))
    plan.prepare()                                   # the plan's own workspace, settled before the capture
    d_in = torch.from_numpy(tn._flat_spectra(n, re, im)).to(DEV).view(torch.float16)
    d_mask = torch.from_numpy(_flat_mask(n, mask_of(n, rows, length, hop, pad, "frame"))).to(DEV).view(torch.float16)
    d_out = torch.zeros(rows * length, dtype=torch.float16, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            plan.exec(d_in, d_in[sn.pitch(n):], d_mask, d_out)
    torch.cuda.synchronize()
    assert not d_out.any(), "a captured execution ran at capture time"
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.int16).reshape(rows, length), y)
    del graph
    plan.close()


# ---- 9
@pytest.mark.parametrize("n", LENGTHS)
def test_refusals_leave_the_output_untouched(tf, n):
    rows, length, hop, pitch = 2, 2 * n, n // 4, sn.pitch(n)
    plan = tf.TfftMaskedIstftPlan(n, rows, length, hop)
    total = rows * plan.frames
    d_in = torch.zeros(total * 2 * pitch + 8, dtype=torch.float16, device=DEV)
    # (room behind the mask and, below, behind the workspace: an extent that starts at their last 16 bytes stays inside the allocation)
    d_mask = torch.ones(total * pitch + rows * length + 8, dtype=torch.float16, device=DEV)
    d_out = torch.from_numpy(np.full(rows * length + 8, de.SENTINEL, np.int16)).to(DEV).view(torch.float16)
    d_ws = torch.from_numpy(np.full(total * n, de.SENTINEL, np.int16)).to(DEV).view(torch.float16)
    re_p, im_p, m_p, out_p = d_in.data_ptr(), d_in.data_ptr() + 2 * pitch, d_mask.data_ptr(), d_out.data_ptr()

    def refused(needle, *args):
        with pytest.raises(tf.TfftError) as e:
            plan.exec_ptr(*args)
        assert needle in str(e.value), str(e.value)

    # before a window was set
    refused("tfft_mistftn_plan_set_window", re_p, im_p, m_p, out_p)
    plan.set_window(torch.ones(n, dtype=torch.float16, device=DEV))
    plan.set_workspace(d_ws)
    # a mask that is missing or not 16-byte aligned; the other three as tfft_istftn_exec
    refused("null mask", re_p, im_p, None, out_p)
    refused("the mask must be 16-byte aligned", re_p, im_p, m_p + 2, out_p)
    refused("the mask must be 16-byte aligned", re_p, im_p, m_p + 8, out_p)
    refused("16-byte aligned", re_p, im_p + 8, m_p, out_p)
    refused("output and input overlap", re_p, im_p, m_p, re_p)
    # the output inside the mask's extent, at its start and at its last 16 bytes; the mask inside the output's
    refused("output and mask overlap", re_p, im_p, m_p, m_p)
    refused("output and mask overlap", re_p, im_p, m_p, m_p + 2 * ((total - 1) * pitch + sn.bins(n)) - 2 & ~15)
    refused("output and mask overlap", re_p, im_p, out_p + 2 * rows * length - 16, out_p)
    # the workspace on the mask
    big = torch.ones(total * n + d_mask.numel() + 128, dtype=torch.float16, device=DEV)
    plan.set_workspace(big)
    refused("the workspace overlaps the mask", re_p, im_p, big.data_ptr(), out_p)
    refused("the workspace overlaps the mask", re_p, im_p, big.data_ptr() + 2 * total * n - 16, out_p)
    plan.set_workspace(d_ws)
    torch.cuda.synchronize()
    assert (d_out.view(torch.int16) == de.SENTINEL).all() and (d_ws.view(torch.int16) == de.SENTINEL).all() and not d_in.any()
    assert (d_mask == 1).all() and (big == 1).all()
    # the mask may alias the spectra, and the call that is legal runs: zero spectra give zeros
    plan.exec_ptr(re_p, im_p, re_p, out_p)
    plan.exec_ptr(re_p, im_p, m_p, out_p)
    torch.cuda.synchronize()
    assert not d_out[:rows * length].any() and (d_out[rows * length:].view(torch.int16) == de.SENTINEL).all()
    assert not d_ws.any() and (d_mask == 1).all()
    plan.close()


# ---- 10
@pytest.mark.parametrize("n", LENGTHS)
def test_masked_istft_and_mask_buffer(tf, monkeypatch, n):
    mod = importlib.import_module("tensor_fft_amd.mistftn")
    seen = []
    real_exec = mod.TfftMaskedIstftPlan.exec_ptr
    monkeypatch.setattr(mod.TfftMaskedIstftPlan, "exec_ptr",
                        lambda self, in_re, in_im, mask, out, stream=0: (seen.append((id(self), mask)), real_exec(self, in_re, in_im, mask, out, stream))[1])
    tf.mistftn_cache_clear()
    rows, length, hop, pad = 2, 2 * n, n // 2, n // 2
    _, w, re, im = tn.inputs(n, rows, length, hop, pad, "hann")
    frames = inr.geometry(n, length, hop, pad)
    m = mask_of(n, rows, length, hop, pad, "frame")
    _, y = result(tf, n, rows, length, hop, pad, 0, "hann", "frame")
    v_re, v_im = tn._stft_layout(n, re, im, rows)
    d_w = torch.from_numpy(w.copy()).to(DEV)
    # a mask written into mask_buffer's view is read where it lies
    view = tf.mask_buffer(rows, frames, n, DEV)
    assert view.shape == (rows, frames, sn.bins(n)) and view.stride() == (frames * sn.pitch(n), sn.pitch(n), 1) and view.dtype == torch.float16
    view.copy_(torch.from_numpy(m.copy()).to(DEV).reshape(view.shape))
    got = tf.masked_istft(v_re, v_im, view, d_w, hop, length, n, center=True)
    assert got.shape == (rows, length) and got.dtype == torch.float16 and np.array_equal(got.cpu().numpy().view(np.int16), y)
    assert seen[-1][1] == view.data_ptr(), "the mask of mask_buffer was copied"
    # a contiguous [R, F, n / 2 + 1] mask (an odd frame stride) is copied once and gives the same bits, through the same cached plan
    dense = torch.from_numpy(m.copy()).to(DEV).reshape(view.shape)
    again = tf.masked_istft(v_re, v_im, dense, d_w, hop, length, n, center=True)
    assert np.array_equal(again.cpu().numpy().view(np.int16), y) and seen[-1][1] != dense.data_ptr()
    assert seen[-1][0] == seen[-2][0] and len(mod._plans) == 1, "the plan cache was not reused"
    # a frame stride that is another multiple of 8 is read in place too, by a plan of that stride
    wide = torch.zeros((rows, frames, sn.pitch(n) + 16), dtype=torch.float16, device=DEV)[:, :, :sn.bins(n)]
    wide.copy_(dense)
    third = tf.masked_istft(v_re, v_im, wide, d_w, hop, length, n, center=True)
    assert np.array_equal(third.cpu().numpy().view(np.int16), y) and seen[-1][1] == wide.data_ptr() and len(mod._plans) == 2
    # a 1-D mask selects per-bin mode
    mb = mask_of(n, rows, length, hop, pad, "bin")
    per_bin = tf.masked_istft(v_re, v_im, torch.from_numpy(mb.copy()).to(DEV), d_w, hop, length, n, center=True)
    assert np.array_equal(per_bin.cpu().numpy().view(np.int16), result(tf, n, rows, length, hop, pad, 0, "hann", "bin")[1])
    raw = tf.masked_istft(v_re, v_im, view, d_w, hop, length, n, center=True, raw_sum=True)
    assert np.array_equal(raw.cpu().numpy().view(np.int16), result(tf, n, rows, length, hop, pad, 0, "hann", "frame", raw=True)[1])
    with pytest.raises(tf.TfftError):              # a mask of another shape
        tf.masked_istft(v_re, v_im, dense[:, :-1], d_w, hop, length, n, center=True)
    with pytest.raises(tf.TfftError):              # float32
        tf.masked_istft(v_re, v_im, dense.float(), d_w, hop, length, n, center=True)
    with pytest.raises(tf.TfftError):
        tf.masked_istft(v_re, v_im, view, d_w, hop, length, 4096, center=True)
    tf.mistftn_cache_clear()
    assert not mod._plans


# ---- 11
def test_example_runs():
    exe = os.path.join(ROOT, "examples", "example_masked_istft")
    assert os.path.exists(exe), "build() did not build examples/example_masked_istft"
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("OK"), run.stdout + run.stderr
    found = re.search(r"residual of the removed tone \(amplitude [0-9.]+\): ([0-9.e+-]+) \(threshold ([0-9.e+-]+)\)", run.stdout)
    assert found and float(found.group(1)) <= float(found.group(2)), run.stdout
    assert "output and mask overlap" in run.stdout
