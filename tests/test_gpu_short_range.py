"""The short ISTFT, the masked short ISTFT, the spectrogram plans and the two gradients built on them at the edges of their range
contract, on the GPU (include/tfft_istftn.h, tfft_mistftn.h, tfft_spec.h, tensor-fft_amd/stft_autograd.py), at n = 512, 1024 and 2048.
Every other GPU test of these add-ons feeds spectra of uniform(-1, 1) signals under a window of at most 1, masks in [0, 1] and
gradients in (-1, 1). Here the data sets of tests/short_range_ref.py run through the runners of tests/test_gpu_istftn.py,
test_gpu_mistftn.py, test_gpu_stftn.py and test_gpu_spec.py (guard zones, NaN gaps, inputs unchanged, all kept):

  short ISTFT   every set, divided and raw: the workspace frames against istftn_ref.merge_items -> TfftPlan(n).exec_inverse, y
                against istftn_ref.ola of the frames as read back, bit for bit. spectra-high (noise at 2^10, 2^10, 2^9) and the
                tones at the input condition's limit also against fp64; a window times 2^k gives fp16(2^-k q_unit) in every bit;
                the subnormal sets return non-zero output, output-subnormal at least 0.9 non-zero subnormals.
  masked ISTFT  per frame and per bin: the same two bit yardsticks with mistftn_ref.merge_items_masked. mask-rescues (spectra whose
                unmasked merge is inf, brought back by a mask of 2^-4 .. 2^-6), mask-lifts (subnormal spectra under a mask of 2^15),
                mask-subnormal (every mask entry a subnormal) also against fp64; mask-uneven (2^6 and 2^-6 on the two frames of a
                pair) by bits alone. With the uniform factor dropped the mask is +-2^k and the plan returns TfftShortIstftPlan's
                bits on the planes multiplied on the host.
  spectrograms  the forward sets of tests/stft_range_ref.py: power at gain 1 and n^2 and the band sets all, edges and signed
                (weights uniform(-1, 1): cancellation shows a fused multiply-add) against spec_ref's fp32 restatement on the halves
                TfftShortStftPlan writes in the same process, bit for bit; the upper sets against fp64; bin 0 of the lower sets
                non-zero; gain 2^100 and 2^110: +inf exactly where the restatement has it, never a NaN.
  gradients     differentiable_short_stft on gradients of 2^15 and of 2^-14 (every half a subnormal): the bits of a hand-run raw-sum
                per-bin plan with the adjoint mask, and fp64 at the upper scale; differentiable_power_spectrogram under gP 2^k
                and gain 2^k: dx_k = dx_0 2^k wherever both are normal; one entry of gP 2^20 times the rest.

No bound here was chosen by looking at the kernels: each is a constant or formula of the existing suites (asserted to be the same)
or a bit comparison. tests/test_short_range_host.py checks every input of this file on the CPU first, and shows that each lower-edge
and mask set differs from its expectation under the fault it is there for. The worst ratios measured against fp64 are printed and
written to profiles/short_range.txt.

Measured on the MI355X (seed 1), error over bound, worst signal or frame, over the three n: spectra-high 0.097 .. 0.098, the tones at
most 0.076 (the constant comes back exactly); mask-rescues, mask-lifts and mask-subnormal 0.12 .. 0.14; the power of the upper forward
sets at most 0.18 of POWER_BOUND at either gain, their bands at most 0.11 of band_bound; grad-high 0.093 .. 0.098; the power gradient
with one dominant entry 0.061, 0.074, 0.149. output-subnormal: 0.995, 0.992, 0.990 of y are non-zero subnormals, as the model has it
(DESIGN.md 3.20 - 3.22). That the sets see the faults they are there for is shown on the CPU models only; no faulty build of the
add-ons was run on a GPU."""
import os

import numpy as np
import pytest

import istftn_ref as inr
import short_range_ref as q
import spec_ref as spr
import stft_range_ref as sr
import stftn_ref as sn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_istftn as tn  # noqa: E402
import test_gpu_mistftn as tm  # noqa: E402
import test_gpu_spec as ts  # noqa: E402
import test_gpu_stftn as t_stftn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
_ids = lambda v: str(v)      # noqa: E731
INVERSE = lambda corners: [(c, n) for n in q.LENGTHS for c in corners]      # noqa: E731
_ratios = {}


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    yield tensor_fft_amd
    lines = ["# tests/test_gpu_short_range.py: the worst signal (frame for the spectrograms) of every set that is held to fp64, error / bound,",
             "# seed 1. Bounds: _accuracy_bound and _grad_bound (+ K_FWD + K_MASK) of the ISTFT suites, POWER_BOUND and band_bound of spec_ref",
             "# what n error/bound"]
    lines += [f"{k[0]} {k[1]} {v:.4f}" for k, v in sorted(_ratios.items())]
    try:
        with open(os.path.join(ROOT, "profiles", "short_range.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError as e:                      # a read-only checkout: the figures are in the output
        print(f"profiles/short_range.txt not written: {e}")


def _record(what, n, error, bound):
    print(f"short range {what} n={n}: worst {error:.2e} against fp64 (bound {bound:.2e}, ratio {error / bound:.3f})")
    _ratios[(what, n)] = error / bound


def test_the_constants_are_the_suites_own():
    assert (q.K_C2R, q.K_FWD) == (tn.K_C2R, tn.K_FWD) == (tm.K_C2R, tm.K_FWD) and q.K_MASK == tm.K_MASK
    for n in q.LENGTHS:
        rows, length, hop, pad = q.MASK_SHAPE(n)
        w = sn.hann(n)
        assert q.accuracy_bound(w, n, length, hop, pad) == tn._accuracy_bound(w, n, length, hop, pad)
        rows, length, hop, pad = q.LOWER_SHAPE(n)
        assert q.grad_bound(w, n, length, hop, pad) == tm._grad_bound(w, n, length, hop, pad)
        assert (rows, length, hop, pad) == dict((name, shape) for name, shape, _ in tm.GRAD_SHAPES)["centred"](n)


# ------------------------------------------------------------------------------------------------- the ISTFT plans, masked or not

_runs = {}


def check_inverse(tf, d, raw=False):
    """(frames, y) int16 bit patterns of one set through its plan, run once per module and held to the two bit yardsticks on the way:
    the workspace frames against the host merge -> TfftPlan(n).exec_inverse, y against istftn_ref.ola of the frames as read back"""
    key = (d["corner"], d["n"], d.get("mode"), d.get("pure"), raw)
    if key in _runs:
        return _runs[key]
    n, rows, length, hop, pad = q.geo(d)
    re, im, w = d["re"].copy(), d["im"].copy(), d["w"].copy()
    if d.get("mask") is None:
        frames, y = tn.run_istftn(tf, n, re, im, w, rows, length, hop, pad, 0, raw)
    else:
        frames, y = tm.run_mistftn(tf, n, re, im, d["mask"].copy(), w, rows, length, hop, pad, 0, raw)
    what = f"short range {d['corner']} n={n}{' per ' + d['mode'] if d.get('mode') else ''}{' pure' if d.get('pure') else ''}{' raw' if raw else ''}"
    assert not np.isnan(frames.view(np.float16)).any(), what + ": a NaN reached the frames"
    zr, zi = q.merged(d)
    tn._assert_bits(what + ", frames against the host merge -> TfftPlan.exec_inverse", frames, tn.via_inverse_plan(tf, n, zr, zi, re.shape[0]))
    want_y = q.ola(d, frames.view(np.float16), raw).view(np.int16)
    tn._assert_bits(what + ", output against istftn_ref.ola of the workspace frames", y, want_y, ("signal", "sample"))
    _runs[key] = (frames, y)
    return _runs[key]


def both_ways(tf, d):
    frames, y = check_inverse(tf, d)
    raw_frames, raw_y = check_inverse(tf, d, raw=True)
    assert np.array_equal(frames, raw_frames)
    assert np.isfinite(frames.view(np.float16)).all() and np.isfinite(y.view(np.float16)).all() and np.isfinite(raw_y.view(np.float16)).all()
    return frames, y


@pytest.mark.parametrize("corner,n", INVERSE(q.UPPER_INVERSE), ids=_ids)
def test_inverse_at_the_input_condition(tf, corner, n):
    """spectra-high: noise spectra with max |Z'| within a factor 2 of 64512. tone-edge-a, -b, -c (k0 = 0, 1, n / 32): the largest
    constant (89.06, 44.53, 22.27) and tone (178.1, 89.06, 44.53) a rectangular window lets through. Finite, and per signal within
    the bound of tests/test_gpu_istftn.py against the fp64 ISTFT of the same spectra (a rectangular window: K_C2R sqrt 2 + 2^-11)."""
    d = q.inverse(corner, n)
    assert q.holds(d) and q.binding(d)[1] >= 0.5
    _, y = both_ways(tf, d)
    if corner == "spectra-high":
        bound = tn._accuracy_bound(d["w"], n, d["length"], d["hop"], d["pad"])
    else:
        bound = tn.K_C2R * np.sqrt(2.0) + 2.0 ** -11
    worst = float(sr.rel_l2(y.view(np.float16).astype(np.float64), q.reference(d)).max())
    _record(f"istftn {corner}", n, worst, bound)
    assert worst <= bound


@pytest.mark.parametrize("corner,n", INVERSE(q.WINDOW_INVERSE), ids=_ids)
def test_a_power_of_two_on_the_window_changes_no_bit_of_the_quotient(tf, corner, n):
    """Hann 2^15 and uniform(0.5, 1) 2^-8: num scales by 2^k and den by 2^2k, exactly in fp32 (tests/test_short_range_host.py), so
    y = fp16(2^-k q_unit) with q_unit the fp32 quotient of the unit window's run: the unit window's y in every bit wherever 2^-k
    y_unit is a binary16 number, and one rounding of the same quotient where it is not (k = 15: most of y is subnormal). The raw
    sum is held to the composition alone."""
    d = q.inverse(corner, n)
    unit = q.unit_window(d)
    frames, y = both_ways(tf, d)
    unit_frames, unit_y = check_inverse(tf, unit)
    assert np.array_equal(frames, unit_frames)                             # the frames do not depend on the window
    want = q.scaled_window_output(unit_frames.view(np.float16), d)
    tn._assert_bits(f"short range {corner} n={n}, y against 2^{-d['k']} x the unit window's quotient", y, want.view(np.int16), ("signal", "sample"))
    y_unit = unit_y.view(np.float16)
    exact = y_unit.astype(np.float64) * 2.0 ** -d["k"]
    with np.errstate(over="ignore"):
        same = (exact.astype(np.float16).astype(np.float64) == exact) & ~sr.subnormal(y_unit)
    assert same.any() and np.array_equal(y.view(np.float16).astype(np.float64)[same], exact[same])


@pytest.mark.parametrize("corner,n", INVERSE(q.LOWER_INVERSE), ids=_ids)
def test_inverse_keeps_subnormals(tf, corner, n):
    """spectra-subnormal: the input halves are subnormal; output-subnormal: so are the frames and y. The yardsticks keep them, so a
    load, a conversion around the gain or an output conversion that flushes differs in every signal (tests/test_short_range_host.py)."""
    d = q.inverse(corner, n)
    _, y = both_ways(tf, d)
    assert (y & 0x7FFF != 0).any(axis=1).all()
    if corner == "output-subnormal":
        share = float(sr.subnormal(y.view(np.float16)).mean())
        print(f"short range output-subnormal n={n}: {share:.3f} of y are non-zero subnormals")
        assert share >= 0.9


@pytest.mark.parametrize("corner,n,mode", q.mask_params(), ids=_ids)
def test_masked_inverse_at_the_edges(tf, corner, n, mode):
    """The bit yardsticks, divided and raw; finite; mask-rescues, mask-lifts and mask-subnormal per signal within _accuracy_bound of
    the fp64 ISTFT of the fp64-masked spectra; mask-subnormal returns non-zero output in every signal."""
    d = q.masked(corner, n, mode)
    assert q.holds(d)
    _, y = both_ways(tf, d)
    if corner in q.MASK_FP64:
        bound = tn._accuracy_bound(d["w"], n, d["length"], d["hop"], d["pad"])
        worst = float(sr.rel_l2(y.view(np.float16).astype(np.float64), q.reference(d)).max())
        _record(f"mistftn {corner} per {mode}", n, worst, bound)
        assert worst <= bound
    if corner == "mask-subnormal":
        assert (y & 0x7FFF != 0).any(axis=1).all()


@pytest.mark.parametrize("corner,n,mode", q.mask_params(), ids=_ids)
def test_a_mask_of_powers_of_two_gives_the_unmasked_plans_bits(tf, corner, n, mode):
    """the set with the uniform factor dropped: the mask is +-2^k and the spectra lie where the product is a binary16 number
    (asserted on the host), so the frames and the output are TfftShortIstftPlan's on the premultiplied planes, in every bit"""
    d = q.masked(corner, n, mode, pure=True)
    assert d["exact"] and q.holds(d)
    plain = dict(d, re=d["pre_re"], im=d["pre_im"], mask=None, mode=None, corner=d["corner"] + "-premultiplied-" + mode)
    for raw in (False, True):
        frames, y = check_inverse(tf, d, raw)
        want_frames, want_y = check_inverse(tf, plain, raw)
        what = f"short range {corner} n={n} per {mode}{' raw' if raw else ''}, a mask of +-2^k against TfftShortIstftPlan on the premultiplied planes"
        tn._assert_bits(what + ", frames", frames, want_frames)
        tn._assert_bits(what + ", output", y, want_y, ("signal", "sample"))
        assert np.isfinite(y.view(np.float16)).all()


# ------------------------------------------------------------------------------------------------------------------- spectrograms

_halves = {}


def halves(tf, d):
    """(re, im) binary16 [G, bins]: what TfftShortStftPlan writes for the forward set, in this process, once"""
    key = (d["corner"], d["n"])
    if key not in _halves:
        re, im = t_stftn.run_stftn(tf, d["n"], d["x"].copy(), d["w"].copy(), d["hop"], d["pad"])
        _halves[key] = (re.view(np.float16), im.view(np.float16))
    return _halves[key]


def run_spec(tf, d, gain, band_list=None):
    """test_gpu_spec.run_spec_on (NaN prefill, guard zones, one launch) on the forward set: power every pitch + 8 floats, bands every
    B + 3 floats"""
    return ts.run_spec_on(tf, d["n"], d["x"], d["w"], d["hop"], d["pad"], 0, gain, band_list, extra=3 if band_list else 8)


@pytest.mark.parametrize("corner,n", INVERSE(q.SPEC_UPPER + q.SPEC_LOWER), ids=_ids)
def test_spectrograms_at_the_edges(tf, corner, n):
    """Power at gain 1 and n^2 and the bands all, edges, signed at gain n^2 are spec_ref's restatement on TfftShortStftPlan's halves, bit
    for bit. Upper sets: finite, per frame sum |P - P64| <= POWER_BOUND sum P64 and the non-negative band sets within band_bound.
    Lower sets: P of bin 0 is non-zero in every frame."""
    d = sr.forward(corner, n)
    re, im = halves(tf, d)
    nbins, sets = sn.bins(n), q.band_sets(n)
    for name, gain in q.gains(n).items():
        got = run_spec(tf, d, gain)
        p = spr.power(re, im, gain)
        ts._assert_bits(f"short range power {corner} n={n} gain {gain:g}", got, p)
        if corner in q.SPEC_UPPER:
            p_ref = q.p64(d, gain)
            assert np.isfinite(got.view(np.float32)).all()
            worst = float((np.abs(got.view(np.float32).astype(np.float64) - p_ref).sum(-1) / p_ref.sum(-1)).max())
            _record(f"spec {corner} power gain {name}", n, worst, spr.POWER_BOUND)
            assert worst <= spr.POWER_BOUND
        else:
            assert (got[:, 0] & 0x7FFFFFFF != 0).all(), f"{corner} n={n}: P of bin 0 of a frame is zero"
    gain = float(n) ** 2
    p = spr.power(re, im, gain)
    for band_name in q.BAND_SETS:
        got = run_spec(tf, d, gain, sets[band_name])
        ts._assert_bits(f"short range bands {band_name} {corner} n={n}", got, spr.band_energies(p, sets[band_name]))
        if corner in q.SPEC_UPPER:
            assert np.isfinite(got.view(np.float32)).all()
            if band_name != "signed":
                bound, e64 = spr.band_bound(q.p64(d, gain), sets[band_name], nbins)
                worst = float((np.abs(got.view(np.float32).astype(np.float64) - e64).sum(-1) / bound).max())
                _record(f"spec {corner} bands {band_name}", n, worst, 1.0)
                assert worst <= 1.0


@pytest.mark.parametrize("n", q.LENGTHS)
def test_a_gain_that_overflows_gives_inf_and_no_nan(tf, n):
    """signal-high under gain 2^100 (finite: the halves reach 2^10) and 2^110: P is +inf exactly where the restatement is, nowhere a
    NaN, and every other float has the restatement's bits. Power mode only: 0 * inf in a band would leave NaN payloads unpinned."""
    d = sr.forward("signal-high", n)
    re, im = halves(tf, d)
    for gain in (2.0 ** 100, 2.0 ** 110):
        got = run_spec(tf, d, gain)
        with np.errstate(over="ignore"):
            want = spr.power(re, im, gain)
        assert not np.isnan(got.view(np.float32)).any()
        assert np.array_equal(np.isposinf(got.view(np.float32)), np.isposinf(want)) and not np.isneginf(got.view(np.float32)).any()
        ts._assert_bits(f"short range gain-overflow n={n} gain {gain:g}", got, want)
    assert np.isposinf(want).any() and np.isfinite(want).any()


# ---------------------------------------------------------------------------------------------------------------------- gradients

def _clear(tf):
    tf.mistftn_cache_clear()
    tf.stftn_cache_clear()
    tf.spec_cache_clear()


@pytest.mark.parametrize("n", q.LENGTHS)
@pytest.mark.parametrize("corner", ["grad-high", "grad-low"])
def test_differentiable_short_stft_at_scale(tf, corner, n):
    """grad-high: (g_re, g_im) = uniform(-1, 1) 2^15, the largest power of two at which the adjoint plan's contract holds on c_k G (the
    gradient itself ends there). dx is finite, within _grad_bound of mistftn_ref.adjoint64, and equals, bit for bit, a hand-run
    raw-sum per-bin plan with the adjoint mask. grad-low: the same at 2^-14, every half a subnormal: the bits, and dx non-zero in
    every signal."""
    d = q.grad(corner, n)
    _, rows, length, hop, pad = q.geo(d)
    frames, bins = inr.geometry(n, length, hop, pad), sn.bins(n)
    x = sn.case_data(n, rows, length)[0]
    d_x = torch.from_numpy(x.copy()).to(DEV).requires_grad_(True)
    d_w = torch.from_numpy(d["w"].copy()).to(DEV)
    _clear(tf)
    try:
        re, im = tf.differentiable_short_stft(d_x, d_w, hop, n, center=True)
        g_re, g_im = (torch.from_numpy(d[k].reshape(rows, frames, bins).copy()).to(DEV) for k in ("re", "im"))
        torch.autograd.backward((re, im), (g_re, g_im))
        dx = d_x.grad.cpu().numpy()
    finally:
        _clear(tf)
    assert dx.dtype == np.float16 and dx.shape == (rows, length)
    _, by_hand = check_inverse(tf, d, raw=True)
    tn._assert_bits(f"short range {corner} n={n}, dx against a hand-run raw-sum per-bin plan with the adjoint mask", dx.view(np.int16), by_hand,
                    ("signal", "sample"))
    assert np.isfinite(dx).all() and (dx.view(np.int16) & 0x7FFF != 0).any(axis=1).all()
    if corner == "grad-high":
        assert q.binding(d)[1] >= 0.5
        dx64 = q.mr.adjoint64(d["re"], d["im"], d["w"], rows, length, hop, pad)
        v64 = q.mr.adjoint_frames64(d["re"], d["im"], n)
        scale = np.maximum(q.per_signal(v64, rows), q.per_signal(dx64, rows))
        worst = float((q.per_signal(dx.astype(np.float64) - dx64, rows) / scale).max())
        bound = tm._grad_bound(d["w"], n, length, hop, pad)
        _record("grad-high", n, worst, bound)
        assert worst <= bound


def _power_dx(tf, p):
    """dx of differentiable_power_spectrogram for one case of short_range_ref.power_case, binary16 [R][L]"""
    d_x = torch.from_numpy(p["x"].copy()).to(DEV).requires_grad_(True)
    d_w = torch.from_numpy(p["w"].copy()).to(DEV)
    out = tf.differentiable_power_spectrogram(d_x, d_w, p["hop"], p["n"], center=True, gain=p["gain"])
    out.backward(torch.from_numpy(p["g_p"].copy()).to(DEV))
    dx = d_x.grad.cpu().numpy()
    assert dx.dtype == np.float16 and dx.shape == (p["rows"], p["length"])
    return dx


@pytest.mark.parametrize("n", q.LENGTHS)
def test_power_gradient_under_powers_of_two(tf, n):
    """gP 2^k and gain 2^k at gain n^2: only the device-side scale s changes, fp16(M / s) does not and y s is exact in fp32, so
    dx_k = dx_0 2^k bit for bit wherever both are normal binary16 numbers. k = -8 and 6 (tests/test_short_range_host.py: at least
    half of the samples qualify by the fp64 gradient; at k = -30 none do, so it is not asserted)."""
    gain = float(n) ** 2
    ks = q.power_exponents(n, gain)
    assert set(ks) == {-8, 6}
    _clear(tf)
    try:
        dx0 = _power_dx(tf, q.power_case(n, gain)).astype(np.float64)
        assert np.isfinite(dx0).all()
        for k in ks:
            for what, case in (("gP", q.power_case(n, gain, k)), ("gain", q.power_case(n, gain * 2.0 ** k))):
                dxk = _power_dx(tf, case).astype(np.float64)
                both = q.normal16(dx0) & q.normal16(dx0 * 2.0 ** k)
                print(f"short range power gradient n={n}, {what} 2^{k}: {both.mean():.3f} of the samples are normal at both scales")
                assert both.mean() >= 0.5
                bad = np.argwhere(both & (dxk != dx0 * 2.0 ** k))
                assert bad.size == 0, f"n={n} {what} 2^{k}: {len(bad)} samples differ from dx_0 2^k, first (signal, sample) = {bad[:3].tolist()}"
    finally:
        _clear(tf)


@pytest.mark.parametrize("n", q.LENGTHS)
def test_power_gradient_with_one_dominant_entry(tf, n):
    """gP = uniform(-1, 1) with one entry of 2^20 (gain 1): every other entry of fp16(M / s) is a subnormal or zero. dx is finite and
    within the existing bound _grad_bound + K_FWD + K_MASK of the fp64 gradient, relative to the scale of the signal that holds the
    dominant entry."""
    p = q.power_case(n, 1.0, dominant=True)
    _clear(tf)
    try:
        dx = _power_dx(tf, p)
    finally:
        _clear(tf)
    dx64, v64 = q.power_grad64(p)
    scale = np.maximum(q.per_signal(v64, p["rows"]), q.per_signal(dx64, p["rows"])).max()
    worst = float((q.per_signal(dx.astype(np.float64) - dx64, p["rows"]) / scale).max())
    bound = tm._grad_bound(p["w"], n, p["length"], p["hop"], p["pad"]) + tm.K_FWD + tm.K_MASK
    _record("power gradient, one entry 2^20", n, worst, bound)
    assert np.isfinite(dx).all() and worst <= bound
