"""The range contract of the STFT family on the CPU (tests/stft_range_ref.py): every input that tests/test_gpu_stft_range.py hands to a
GPU is checked here first. For every data set

  * the contract holds (the one set marked `outside` breaks it in exactly one quantity), upper-edge sets bind within a factor 2,
    subnormal sets hold the shares of subnormals they are named for;
  * the REFERENCE ALONE stays within what the GPU test asserts: the numpy model of the kernels (tests/stage_model.py between framing,
    split, merge and overlap-add) is finite and meets every asserted tolerance with the margin 1.5, the project's rule for a
    constant. The real plans that serve as the GPU test's bit-for-bit yardstick were never run near full scale, so a bit
    comparison alone would prove little there;
  * the bit comparison can SEE the fault it is there for: the expectation recomputed with a flushing multiply, flushed loads or a
    flushed output conversion differs from the true one in at least one half of every frame (of every signal for the inverse).

The input condition of the forward plans. They are TfftRealPlan on frame pairs, so the sequential-scaling bound of include/tfft.h
applies to the complex sample u_2i + i u_2i+1 of a pair: |.| <= 64512 (tests/test_conv_range_host.py derives the figure). Both
frames of a pair may reach A_PAIR = 45600 at once. A self-paired last frame is paired with ITSELF, not with zeros, so it is not the
exempt "row without partner" of the convolution add-ons: its limit is 45600 as well. The set `corner-self-outside` (the k = 1 corner
signal at 65504, |u + i u| = 92636) is decided here: the model stays finite at every n, the largest value in front of a rounding
being 41954, 41826, 41762 and 58923 at n = 512 .. 4096. That is this signal's luck, not a bound: both planes carry the same real
signal, a stage turns u (1 + i) into S (1 + i), and for real input |S| <= B where S is real but up to 0.7072 B (1 + 2^-11) where it is
complex (tests/test_conv_range_host.py), whose components sqrt 2 |S| may pass 65504 by a hair. The finite result is recorded, the
condition is not relaxed for it, and a pair of two DIFFERENT signals at that amplitude does overflow (asserted below).

The ISTFT input condition binds early: |4096 (A[k] + i B[k])| <= 64512 lets a tone c cos(2 pi k0 t / 4096) under a rectangular
window reach c = 22.27 (A[k0] = B[k0] = c / 2), a constant only 11.13 (A[0] = B[0] = c), and uniform(-1, 1) noise under Hann 2^8.
"""
import numpy as np
import pytest

import istft_ref as ir
import stage_model as sm
import stft_range_ref as sr

_ids = lambda v: str(v)      # noqa: E731
FORWARD_ALL = sr.forward_params()
INVERSE_ALL = sr.UPPER_INVERSE + sr.WINDOW_INVERSE + sr.LOWER_INVERSE


def _finite(*arrays):
    return all(np.isfinite(np.asarray(a, np.float64)).all() for a in arrays)


def _bits(a):
    return np.asarray(a, np.float16).view(np.int16)


# ------------------------------------------------------------------------------------------------------------------------ forward

@pytest.mark.parametrize("corner,n", FORWARD_ALL, ids=_ids)
def test_forward_inputs_meet_the_contract(corner, n):
    d = sr.forward(corner, n)
    c = sr.contract(d)
    name, ratio = sr.binding(d)
    print(f"forward {corner} n={n}: {name} at {ratio:.3f} of its limit; " + ", ".join(f"{k} {v:.4g} / {lim:.0f}" for k, (v, lim) in c.items()))
    assert sr.holds(d), c
    assert sr.frames(d).shape == (d["rows"] * sr.frames_per_signal(d), n) and d["rows"] * sr.frames_per_signal(d) <= 9
    if corner in sr.UPPER_FORWARD:
        assert 0.5 <= ratio <= 1.0, (name, ratio)
    if corner in ("signal-high", "window-high", "split-high"):
        # the scale is the largest power of two that holds, and it sits where the name says
        e = d["exponent"]
        base_x, base_w = sr.case_data(n, d["rows"], d["length"])
        ex, ew = {"signal-high": (e, 0), "window-high": (0, e), "split-high": (-(-e // 2), e // 2)}[corner]
        assert ex + ew == e and np.array_equal(d["x"], sr.times(base_x, ex)) and np.array_equal(d["w"], sr.times(base_w, ew))
        with np.errstate(over="ignore"):
            over = dict(d, x=sr.times(d["x"], 1))
        assert not (np.isfinite(over["x"]).all() and sr.holds(over))


@pytest.mark.parametrize("corner,n", FORWARD_ALL, ids=_ids)
def test_forward_model_stays_within_what_the_gpu_test_asserts(corner, n):
    d = sr.forward(corner, n)
    re, im = sr.model(d)
    assert _finite(re, im)
    got, want = sr.as_complex(re, im), sr.reference(d)
    if corner in sr.UPPER_FORWARD:
        worst = float(sr.rel_l2(got, want).max())
        print(f"forward {corner} n={n}: model's worst frame rel-L2 {worst:.2e} (asserted on the GPU: {sr.K_RFFT:.1e})")
        assert worst * sr.MARGIN <= sr.K_RFFT
    if corner == "mixed-pair":
        u = sr.frames(d).astype(np.float64)
        top = np.abs(np.fft.fft(u[0] + 1j * u[1]) / n).max()
        worst = float(np.abs(got - want).max() / top)
        print(f"forward mixed-pair n={n}: model's max abs error {worst:.2e} of the pair's largest bin (asserted on the GPU: {sr.K_PAIR:.1e})")
        assert worst * sr.MARGIN <= sr.K_PAIR
    if corner in sr.LOWER_FORWARD:
        # what the GPU test asserts beside the bits: bin 0 of no frame is zero
        assert (_bits(re[:, 0]) & 0x7FFF != 0).all()


@pytest.mark.parametrize("n", sr.LENGTHS)
def test_lower_edge_sets_hold_the_subnormals_they_are_named_for(n):
    d = sr.forward("products-subnormal", n)
    u = sr.frames(d)
    assert (sr.subnormal(u).sum(-1) >= 0.9 * (u != 0).sum(-1)).all() and ((u != 0).mean(-1) > 0.9).all()
    # bin 0 of every frame stands well above the quantum 2^-24: x has one sign
    assert (np.abs(sr.reference(d)[:, 0]) >= 64 * 2.0 ** -24).all()
    d = sr.forward("x-subnormal", n)
    assert sr.subnormal(d["x"]).all()
    u = sr.frames(d)
    assert (sr.subnormal(u).mean(-1) < 0.05).all() and ((u != 0).mean(-1) > 0.9).all()          # u is normal but for the window's foot
    d = sr.forward("mixed-pair", n)
    u = sr.frames(d)
    assert u.shape[0] == 2 and sr.subnormal(u[1]).mean() > 0.5 and sr.subnormal(u[0]).mean() < 0.02


@pytest.mark.parametrize("corner,n", sr.forward_params(sr.LOWER_FORWARD), ids=_ids)
def test_forward_bit_comparison_sees_a_flush(corner, n):
    d = sr.forward(corner, n)
    re, im = sr.model(d)
    for fault in sr.FAULTS[("forward", corner)]:
        f_re, f_im = sr.faulty(d, fault)
        differing = ((_bits(f_re) != _bits(re)) | (_bits(f_im) != _bits(im))).sum(-1)
        print(f"forward {corner} n={n}, {fault} flushed: {differing.tolist()} of {2 * re.shape[1]} halves differ per frame")
        assert (differing > 0).all(), (corner, n, fault)


@pytest.mark.parametrize("n", sr.LENGTHS)
def test_self_paired_frame_at_65504_is_outside_the_contract(n):
    """decided on the CPU: the contract excludes it (pair magnitude 92636 of 64512, nothing else), the model's answer is recorded"""
    d = sr.forward("corner-self-outside", n)
    c = sr.contract(d)
    assert d["outside"] and [k for k, (v, lim) in c.items() if v > lim] == ["pair"], c
    assert abs(c["pair"][0] - 65504.0 * np.sqrt(2.0)) < 1e-6
    u = sr.frames(d)
    acc = sm.accumulators(n, u, u)[1]
    largest = max(float(max(np.abs(a.real).max(), np.abs(a.imag).max())) for a in acc)
    re, im = sr.model(d)
    print(f"corner-self-outside n={n}: largest value in front of a rounding {largest:.1f}, model finite: {_finite(re, im)}")
    # the recorded answer: it does not overflow, with at least 10 % to spare in front of every rounding
    assert largest <= 0.9 * 65504.0 and _finite(re, im)
    assert float(sr.rel_l2(sr.as_complex(re, im), sr.reference(d)).max()) * sr.MARGIN <= sr.K_RFFT
    # ... which is this signal's luck, not the contract's: two different signals at that amplitude do overflow
    pair = sr._forward(n, "pair-65504", 2, n, n, 0, np.stack(sr.rr.corner_signals(sr.A_FULL, 1, n)), np.ones(n, np.float16))
    assert not sr.holds(pair) and not _finite(*sr.model(pair))


# ------------------------------------------------------------------------------------------------------------------------ inverse

@pytest.mark.parametrize("corner", INVERSE_ALL)
def test_inverse_inputs_meet_the_contract(corner):
    d = sr.inverse(corner)
    c = sr.contract(d)
    name, ratio = sr.binding(d)
    print(f"inverse {corner}: {name} at {ratio:.3f} of its limit; " + ", ".join(f"{k} {v:.4g} / {lim:.0f}" for k, (v, lim) in c.items()))
    assert sr.holds(d), c
    assert d["re"].shape[0] == d["rows"] * sr.frames_per_signal(d) <= 27
    if corner in sr.UPPER_INVERSE:
        assert 0.5 <= ratio <= 1.0 and name == "input", (name, ratio)
    if corner == "window-high":
        assert 0.49 <= sr.binding(d, ("raw", "data"))[1] <= 1.0
    if corner == "spectra-high":
        x, w = sr.st.case_data(*sr.ROUND_TRIP_SHAPE[:2])
        re, im = ir.spectra16(sr.times(x, d["exponent"] + 1), w, d["hop"], d["pad"])
        assert not sr.holds(dict(d, re=re, im=im))


def test_tone_amplitudes_make_the_round_trip_limit_concrete():
    """|4096 (A + i B)| <= 64512 with A = B: a tone may reach 64512 sqrt 2 / 4096 = 22.27, a constant half of that; the next binary16
    value breaks the contract"""
    limit = sr.M * np.sqrt(2.0) / ir.N
    for k0 in sr.TONES:
        d = sr.inverse(f"tone-edge-{k0}")
        c = np.float16(d["amplitude"])
        want = limit / 2 if k0 == 0 else limit
        print(f"tone-edge k0={k0}: c = {float(c)} (limit {want:.4f})")
        assert float(c) <= want < float(c) * (1 + 2.0 ** -9)
        assert np.array_equal(d["re"][0], d["re"][1]) and np.array_equal(d["im"][0], d["im"][1])          # one pair, A = B
        up = np.nextafter(c, np.float16(np.inf))
        assert not sr.holds(sr._inverse("up", 1, 2 * ir.N, ir.N, 0, sr.tone(up, k0), d["w"]))
    # the header's example: a constant of 22 under a rectangular window ends in inf
    d = sr._inverse("constant-22", 1, 2 * ir.N, ir.N, 0, sr.tone(22.0, 0), np.ones(ir.N, np.float16))
    assert not sr.holds(d) and not _finite(sr.model_inverse(d)[1])


@pytest.mark.parametrize("corner", INVERSE_ALL)
def test_inverse_model_stays_within_what_the_gpu_test_asserts(corner):
    d = sr.inverse(corner)
    v, y = sr.model(d)
    assert _finite(v, y) and _finite(sr.model_inverse(d, raw=True)[1])
    if corner in sr.UPPER_INVERSE:
        bound = sr.istft_bound(d["w"], d["length"], d["hop"], d["pad"])
        worst = float(sr.rel_l2(y.astype(np.float64), sr.reference(d)).max())
        print(f"inverse {corner}: model's worst signal rel-L2 {worst:.2e} (asserted on the GPU: {bound:.2e})")
        assert worst * sr.MARGIN <= bound
        if corner.startswith("tone-edge"):
            assert abs(bound - (sr.K_C2R * np.sqrt(2.0) + 2.0 ** -11)) < 1e-12          # a rectangular window: envelope 1


def test_inverse_lower_edge_sets_hold_the_subnormals_they_are_named_for():
    d = sr.inverse("spectra-subnormal")
    halves = np.concatenate((d["re"].reshape(-1), d["im"].reshape(-1)))
    share = sr.subnormal(halves).sum() / (halves != 0).sum()
    print(f"spectra-subnormal: {share:.3f} of the non-zero input halves are subnormal")
    assert share >= 0.9 and (halves != 0).mean() > 0.5
    d = sr.inverse("output-subnormal")
    y = sr.model(d)[1]
    print(f"output-subnormal: {sr.subnormal(y).mean():.3f} of the expected y are non-zero subnormals")
    assert sr.subnormal(y).mean() >= 0.9


@pytest.mark.parametrize("corner", [c for k, c in sr.FAULTS if k == "inverse"])
def test_inverse_bit_comparison_sees_a_flush(corner):
    d = sr.inverse(corner)
    y = sr.model(d)[1]
    for fault in sr.FAULTS[("inverse", corner)]:
        f_y = sr.faulty(d, fault)[1]
        differing = (_bits(f_y) != _bits(y)).sum(-1)
        print(f"inverse {corner}, {fault} flushed: {differing.tolist()} of {d['length']} samples differ per signal")
        assert (differing > 0).all(), (corner, fault)


@pytest.mark.parametrize("corner", sr.WINDOW_INVERSE)
def test_a_power_of_two_on_the_window_scales_the_quotient_exactly(corner):
    """num scales by 2^k, den by 2^2k, and neither overflows nor underflows in fp32: the fp32 quotient under the scaled window is 2^-k
    times the unit window's, exactly, so istft_ref.ola under the scaled window is fp16(2^-k q_unit) in every bit, and the unit
    window's output itself wherever 2^-k y_unit is a binary16 number."""
    d = sr.inverse(corner)
    unit = sr.unit_window(d)
    k = d["k"]
    geo = (d["rows"], d["length"], d["hop"], d["pad"])
    v = sr.model_frames(d)                                             # the frames do not depend on the window
    total = v.shape[0]
    f32 = lambda a: np.asarray(a, np.float16).astype(np.float32)      # noqa: E731
    num = {name: ir.ola(f32(v), f32(s["w"]), *geo, raw=True) for name, s in (("scaled", d), ("unit", unit))}
    den = {name: ir.ola(np.tile(f32(s["w"]), (total, 1)), f32(s["w"]), *geo, raw=True) for name, s in (("scaled", d), ("unit", unit))}
    tiny = float(np.finfo(np.float32).tiny)
    for a in (num["scaled"], den["scaled"], num["unit"], den["unit"]):
        mag = np.abs(a.astype(np.float64))
        assert a.dtype == np.float32 and np.isfinite(a).all() and (mag[mag > 0] >= tiny).all()
    assert np.array_equal(num["scaled"].astype(np.float64), num["unit"].astype(np.float64) * 2.0 ** k)
    assert np.array_equal(den["scaled"].astype(np.float64), den["unit"].astype(np.float64) * 2.0 ** (2 * k)) and (den["unit"] > 0).all()
    q_scaled, q_unit = sr.quotient32(v, d["w"], *geo), sr.quotient32(v, d["w_unit"], *geo)
    assert np.array_equal(q_scaled.astype(np.float64), q_unit.astype(np.float64) * 2.0 ** -k)
    y, y_unit = ir.ola(v, d["w"], *geo), ir.ola(v, d["w_unit"], *geo)
    assert np.array_equal(_bits(y), _bits(sr.scaled_window_output(v, d)))
    exact = y_unit.astype(np.float64) * 2.0 ** -k
    with np.errstate(over="ignore"):
        representable = exact.astype(np.float16).astype(np.float64) == exact
    print(f"inverse {corner}: 2^{-k} y_unit is a binary16 number in {representable.mean():.3f} of the samples")
    assert np.array_equal(y.astype(np.float64)[representable & ~sr.subnormal(y_unit)], exact[representable & ~sr.subnormal(y_unit)])
    # the raw sum is held to the composition alone; it is finite
    assert _finite(ir.ola(v, d["w"], *geo, raw=True))


# -------------------------------------------------------------------------------------------------------------------- round trip

def test_round_trip_table_from_the_model():
    """istft(stft(x 2^e)) against x 2^e by the two models, (3, 8192, 1024, 2048) Hann. Where both contracts hold the error is finite and
    does not grow with e: above underflow the arithmetic is covariant under powers of two, below about |x| = 2^-6 the spectra
    DFT(u) / 4096 enter the subnormals and the error grows as e falls. "Does not grow" up to 1 %: at e >= -4 the only thing that moves
    with e is the handful of window-foot products and spectrum halves that leave the subnormals, far below 1 % of the L2 norm over
    8192 samples. One step beyond the largest exponent the ISTFT input condition is broken."""
    rows = [(e, sr.round_trip(e)) for e in sr.ROUND_TRIP_EXPONENTS]
    for e, r in rows:
        print(f"round trip x 2^{e:+d}: rel-L2 {r['error']:.2e}, contracts hold: {r['holds']}, istft input at {sr.binding(r['inverse'], ('input',))[1]:.3f}")
    held = [r["error"] for _, r in rows if r["holds"]]
    assert len(held) == len(rows) and np.isfinite(held).all()
    assert all(b <= a * 1.01 for a, b in zip(held, held[1:])), held
    assert held[0] > 10 * held[-1]                                          # the lower side does lose accuracy
    high = sr.inverse("spectra-high")["exponent"]
    assert high == max(sr.ROUND_TRIP_EXPONENTS) and not sr.round_trip(high + 1)["holds"]
    # what the GPU test asserts for the round trip at the spectra-high scale
    x, w = sr.st.case_data(*sr.ROUND_TRIP_SHAPE[:2])
    bound = sr.istft_bound(w, *sr.ROUND_TRIP_SHAPE[1:]) + sr.K_FWD
    assert sr.round_trip(high)["error"] * sr.MARGIN <= bound


def test_the_round_trip_condition_a_caller_can_check():
    """include/tfft_istft.h: |A[k] + i B[k]| <= mean_j |u_2i[j] + i u_2i+1[j]|, so a pair is safe when that mean is <= 15.75, in
    particular when both frames have rms(u) <= 11.1 or mean |u| <= 7.875. mean |u| <= 11.1 alone is not enough: a cosine and a sine
    of one bin at that mean break the condition."""
    ones = np.ones(ir.N, np.float16)
    t = np.arange(ir.N)

    def pair(c, k0=100):
        x = np.concatenate((c * np.cos(2 * np.pi * k0 * t / ir.N), c * np.sin(2 * np.pi * k0 * t / ir.N))).astype(np.float16)[None]
        return sr._inverse("quadrature", 1, 2 * ir.N, ir.N, 0, x, ones)

    for d in [sr.inverse(c) for c in sr.UPPER_INVERSE + sr.LOWER_INVERSE] + [sr.round_trip(e)["inverse"] for e in sr.ROUND_TRIP_EXPONENTS]:
        u = sr.frames(dict(d, kind="forward")).astype(np.float64)
        a, b = sr.rfft_ref.pair_rows(u.shape[0])
        mean = np.abs(u[a] + 1j * u[b]).mean(-1).max()
        assert sr.contract(d)["input"][0] <= ir.N * mean * (1 + 2.0 ** -9), d["corner"]          # (the spectra and Z' are rounded to binary16)
    at_mean = pair(11.1 * np.pi / 2)                       # both frames: mean |u| = 11.1, rms = 12.3
    print(f"cosine and sine of one bin with mean |u| = 11.1: max |Z'| = {sr.contract(at_mean)['input'][0]:.0f}")
    assert not sr.holds(at_mean) and 71000 < ir.N * 11.1 * np.pi / 2 < 72000
    at_rms = pair(float(sr.rr.floor16(11.1 * np.sqrt(2.0))))            # both frames: rms = 11.1, the mean of the pair's magnitude 15.7
    assert sr.holds(at_rms) and sr.binding(at_rms) == ("input", sr.contract(at_rms)["input"][0] / sr.M) and sr.binding(at_rms)[1] > 0.99
    # the lower-side note: at |x| = 2^-10 nearly all of the forward spectrum's non-zero halves are subnormal
    r = sr.round_trip(-10)["inverse"]
    halves = np.concatenate((r["re"].reshape(-1), r["im"].reshape(-1)))
    share = sr.subnormal(halves).sum() / (halves != 0).sum()
    print(f"round trip x 2^-10: {share:.3f} of the forward spectrum's non-zero halves are subnormal")
    assert share >= 0.9
