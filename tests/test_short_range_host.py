"""The range contract of the short ISTFT, the masked short ISTFT, the spectrogram plans and their gradients on the CPU
(tests/short_range_ref.py): every input that tests/test_gpu_short_range.py hands to a GPU is checked here first. For every data set

  * the inputs are finite, the contract holds, and the upper-edge sets bind within a factor 2;
  * the REFERENCE ALONE stays within what the GPU test asserts: the numpy model (tests/stage_model.py between the merges, splits and
    overlap-adds of the ref modules; spec_ref in fp32) is finite and meets every asserted bound with the margin 1.5;
  * the bit comparison can SEE the fault the set is there for: the expectation recomputed with flushed loads of the spectra, of the
    mask or of the frames, a flushed output conversion, flushed halves in front of the power, or n A rounded to binary16 in front of
    the mask, differs from the true one in every signal (every frame for the spectrograms);
  * the power-of-two identities the GPU test leans on (a window times 2^k, a mask of +-2^k, gP times 2^k) are exact.

What the search found (seed 1). The short ISTFT's input condition |n (A + i B)| <= 64512 lets uniform(-1, 1) noise under Hann reach
2^10, 2^10 and 2^9 at n = 512, 1024, 2048, a tone under a rectangular window 178.1, 89.06, 44.53 and a constant half of that
(64512 sqrt 2 / n). Spectra of x 2^15 are finite binary16 numbers whose unmasked merge is inf at every n; a mask of 2^-4 .. 2^-6
brings them back. No k of {-30, -8, 6} survives at gain 1 and n = 2048 for the power gradient's scaling identity, so the GPU test
takes gain n^2, where -8 and 6 qualify at every n and -30 at none (the fp64 gradient times 2^-30 lies below binary16's normal range)."""
import numpy as np
import pytest

import istftn_ref as inr
import short_range_ref as q
import spec_ref as spr
import stft_range_ref as sr
import stftn_ref as sn

_ids = lambda v: str(v)      # noqa: E731
INVERSE_ALL = [(c, n) for n in q.LENGTHS for c in q.UPPER_INVERSE + q.WINDOW_INVERSE + q.LOWER_INVERSE]
SPEC_ALL = [(c, n) for n in q.LENGTHS for c in q.SPEC_UPPER + q.SPEC_LOWER]
TINY32 = 2.0 ** -126


def _finite(*arrays):
    return all(np.isfinite(np.asarray(a, np.float64)).all() for a in arrays)


def _bits(a):
    return np.asarray(a, np.float16).view(np.int16)


def _shape(d):
    return d["n"], d["length"], d["hop"], d["pad"]


def test_the_helpers_of_the_range_module_kept_their_defaults():
    """the arguments this work added to stft_range_ref (ok, n) default to what the n = 4096 sets were built with"""
    assert np.array_equal(sr.tone(3.0, 100), sr.tone(3.0, 100, 2 * 4096, 4096))
    d = sr.inverse("tone-edge-1")
    assert sr.holds(d) and d["amplitude"] == 22.265625


# -------------------------------------------------------------------------------------------------------------------- short ISTFT

@pytest.mark.parametrize("corner,n", INVERSE_ALL, ids=_ids)
def test_inverse_inputs_meet_the_contract(corner, n):
    d = q.inverse(corner, n)
    c = q.contract(d)
    name, ratio = q.binding(d)
    print(f"istftn {corner} n={n}: {name} at {ratio:.3f} of its limit; " + ", ".join(f"{k} {v:.4g} / {lim:.0f}" for k, (v, lim) in c.items()))
    assert q.finite(d) and q.holds(d), c
    assert d["re"].shape[0] <= 27 and d["rows"] <= 4 and d["length"] <= 4 * n
    if corner in q.UPPER_INVERSE:
        assert 0.5 <= ratio <= 1.0 and name == "input", (name, ratio)
    if corner == "spectra-high":
        assert (d["rows"], d["length"], d["hop"], d["pad"]) == inr.accuracy_shapes(n)[0]
        x, w = sn.case_data(n, d["rows"], d["length"])
        with np.errstate(over="ignore", invalid="ignore"):
            re, im = inr.spectra16(sr.times(x, d["exponent"] + 1), w, d["hop"], d["pad"])
        assert not q._ok(dict(d, re=re, im=im))
    if corner.startswith("tone-edge"):
        limit = q.M * np.sqrt(2.0) / n
        want = limit / 2 if d["k0"] == 0 else limit
        c16 = np.float16(d["amplitude"])
        print(f"istftn {corner} n={n}: k0 = {d['k0']}, c = {float(c16)} (limit {want:.4f})")
        assert float(c16) <= want < float(c16) * (1 + 2.0 ** -9)
        up = np.nextafter(c16, np.float16(np.inf))
        assert not q.holds(q._from_signal("up", n, 1, 2 * n, n, 0, sr.tone(up, d["k0"], 2 * n, n), d["w"]))
    if corner == "window-high":
        assert 0.49 <= q.binding(d, ("raw", "data"))[1] <= 1.0


@pytest.mark.parametrize("corner,n", INVERSE_ALL, ids=_ids)
def test_inverse_model_stays_within_what_the_gpu_test_asserts(corner, n):
    d = q.inverse(corner, n)
    v, y = q.model(d)
    assert _finite(v, y) and _finite(q.model(d, raw=True)[1])
    if corner in q.UPPER_INVERSE:
        bound = q.accuracy_bound(d["w"], *_shape(d))
        worst = float(sr.rel_l2(y.astype(np.float64), q.reference(d)).max())
        print(f"istftn {corner} n={n}: model's worst signal rel-L2 {worst:.2e} (asserted on the GPU: {bound:.2e})")
        assert worst * q.MARGIN <= bound
        if corner.startswith("tone-edge"):
            assert abs(bound - (q.K_C2R * np.sqrt(2.0) + 2.0 ** -11)) < 1e-12          # a rectangular window: envelope 1
    if corner in q.LOWER_INVERSE:
        assert (_bits(y) & 0x7FFF != 0).any(axis=1).all()


@pytest.mark.parametrize("n", q.LENGTHS)
def test_inverse_lower_edge_sets_hold_the_subnormals_they_are_named_for(n):
    d = q.inverse("spectra-subnormal", n)
    halves = np.concatenate((d["re"].reshape(-1), d["im"].reshape(-1)))
    share = sr.subnormal(halves).sum() / (halves != 0).sum()
    print(f"istftn spectra-subnormal n={n}: {share:.3f} of the non-zero input halves are subnormal")
    assert share >= 0.9 and (halves != 0).mean() > 0.5
    y = q.model(q.inverse("output-subnormal", n))[1]
    print(f"istftn output-subnormal n={n}: {sr.subnormal(y).mean():.3f} of the expected y are non-zero subnormals")
    assert sr.subnormal(y).mean() >= 0.9


@pytest.mark.parametrize("n", q.LENGTHS)
@pytest.mark.parametrize("corner", ["spectra-subnormal", "output-subnormal", "window-high"])
def test_inverse_bit_comparison_sees_a_flush(corner, n):
    d = q.inverse(corner, n)
    y = q.model(d)[1]
    for fault in q.FAULTS[corner]:
        f_y = q.faulty(d, fault)[1]
        differing = (_bits(f_y) != _bits(y)).sum(-1)
        print(f"istftn {corner} n={n}, {fault} flushed: {differing.tolist()} of {d['length']} samples differ per signal")
        assert (differing > 0).all(), (corner, n, fault)


@pytest.mark.parametrize("n", q.LENGTHS)
@pytest.mark.parametrize("corner", q.WINDOW_INVERSE)
def test_a_power_of_two_on_the_window_scales_the_quotient_exactly(corner, n):
    """num scales by 2^k, den by 2^2k, and neither leaves fp32's normal range: the fp32 quotient under the scaled window is 2^-k times
    the unit window's, exactly, so istftn_ref.ola under the scaled window is fp16(2^-k q_unit) in every bit, and the unit window's
    output itself wherever 2^-k y_unit is a binary16 number (such samples exist)."""
    d = q.inverse(corner, n)
    unit = q.unit_window(d)
    k = d["k"]
    v = q.model_frames(d)                                              # the frames do not depend on the window
    total = v.shape[0]
    f32 = lambda a: np.asarray(a, np.float16).astype(np.float32)      # noqa: E731
    num = {name: inr.ola(f32(v), f32(s["w"]), *q.geo(d), raw=True) for name, s in (("scaled", d), ("unit", unit))}
    den = {name: inr.ola(np.tile(f32(s["w"]), (total, 1)), f32(s["w"]), *q.geo(d), raw=True) for name, s in (("scaled", d), ("unit", unit))}
    for a in (num["scaled"], den["scaled"], num["unit"], den["unit"]):
        mag = np.abs(a.astype(np.float64))
        assert a.dtype == np.float32 and np.isfinite(a).all() and (mag[mag > 0] >= TINY32).all()
    assert np.array_equal(num["scaled"].astype(np.float64), num["unit"].astype(np.float64) * 2.0 ** k)
    assert np.array_equal(den["scaled"].astype(np.float64), den["unit"].astype(np.float64) * 2.0 ** (2 * k)) and (den["unit"] > 0).all()
    q_scaled, q_unit = q.quotient32(d, v, d["w"]), q.quotient32(d, v, d["w_unit"])
    assert np.array_equal(q_scaled.astype(np.float64), q_unit.astype(np.float64) * 2.0 ** -k)
    y, y_unit = q.ola(d, v), q.ola(unit, v)
    assert np.array_equal(_bits(y), _bits(q.scaled_window_output(v, d)))
    exact = y_unit.astype(np.float64) * 2.0 ** -k
    with np.errstate(over="ignore"):
        same = (exact.astype(np.float16).astype(np.float64) == exact) & ~sr.subnormal(y_unit)
    print(f"istftn {corner} n={n}: 2^{-k} y_unit is a binary16 number in {same.mean():.3f} of the samples")
    assert same.any() and np.array_equal(y.astype(np.float64)[same], exact[same])
    assert _finite(q.ola(d, v, raw=True))


# ------------------------------------------------------------------------------------------------------------------- masked ISTFT

@pytest.mark.parametrize("corner,n,mode", q.mask_params(), ids=_ids)
def test_masked_inputs_meet_the_contract(corner, n, mode):
    d = q.masked(corner, n, mode)
    c = q.contract(d)
    name, ratio = q.binding(d)
    print(f"mistftn {corner} n={n} per {mode}: {name} at {ratio:.3f} of its limit, spectra 2^{d['exponent']}, mask exponent "
          f"{np.unique(d['k']).tolist()}; " + ", ".join(f"{k} {v:.4g} / {lim:.0f}" for k, (v, lim) in c.items()))
    assert q.finite(d) and q.holds(d), c
    assert d["re"].shape[0] == 27 and d["mask"].shape == ((sn.bins(n),) if mode == "bin" else d["re"].shape)
    mag = np.abs(d["mask"].astype(np.float64))
    assert (mag > 0).all() and 0.2 < (d["mask"] < 0).mean() < 0.3
    unmasked = sr.as_complex(*q.merged(dict(d, mask=None)))
    if corner == "mask-rescues":
        print(f"mistftn mask-rescues n={n}: the largest |re| is {np.abs(d['re'].astype(np.float64)).max():.0f}")
        assert not np.isfinite(unmasked.real).all(), "the unmasked merge must overflow"
        assert ratio >= 0.5 and d["k"] < 0
        assert not q._ok(d["remake"](d["k"] + 1))
    if corner == "mask-lifts":
        halves = np.concatenate((d["re"].reshape(-1), d["im"].reshape(-1)))
        assert sr.subnormal(halves).sum() >= 0.9 * (halves != 0).sum() and d["k"] >= 15
        assert not q._ok(d["remake"](d["k"] + 1))
        lifted = np.abs(sr.as_complex(*q.merged(d))).max() / np.abs(unmasked).max()
        assert lifted >= 2.0 ** 13
    if corner == "mask-subnormal":
        assert sr.subnormal(d["mask"]).all()
        assert ratio >= 0.5
    if corner == "mask-uneven":
        even, odd = mag[0::2], mag[1::2]
        assert even.min() >= 32 and odd.max() <= 2.0 ** -6 and d["re"].shape[0] % 2 == 1


@pytest.mark.parametrize("corner,n,mode", q.mask_params(), ids=_ids)
def test_masked_model_stays_within_what_the_gpu_test_asserts(corner, n, mode):
    d = q.masked(corner, n, mode)
    v, y = q.model(d)
    assert _finite(v, y) and _finite(q.model(d, raw=True)[1])
    if corner in q.MASK_FP64:
        bound = q.accuracy_bound(d["w"], *_shape(d))
        worst = float(sr.rel_l2(y.astype(np.float64), q.reference(d)).max())
        print(f"mistftn {corner} n={n} per {mode}: model's worst signal rel-L2 {worst:.2e} (asserted on the GPU: {bound:.2e})")
        assert worst * q.MARGIN <= bound
    if corner == "mask-subnormal":
        assert (_bits(y) & 0x7FFF != 0).any(axis=1).all()


@pytest.mark.parametrize("corner,n,mode", q.mask_params(), ids=_ids)
def test_masked_bit_comparison_sees_the_fault(corner, n, mode):
    """mask-rescues: n A rounded to binary16 before the mask is inf, and the result holds inf or NaN in every signal. mask-lifts: a
    flushed load of the spectra; mask-subnormal: a flushed load of the mask, which zeroes the output; mask-uneven: the two masks of a
    pair exchanged."""
    d = q.masked(corner, n, mode)
    y = q.model(d)[1]
    for fault in q.FAULTS[corner]:
        f_y = q.faulty(d, fault)[1]
        differing = (_bits(f_y) != _bits(y)).sum(-1)
        print(f"mistftn {corner} n={n} per {mode}, fault {fault}: {differing.tolist()} of {d['length']} samples differ per signal")
        assert (differing > 0).all(), (corner, n, mode, fault)
        if fault == "rounded-gain":
            assert (~np.isfinite(f_y.astype(np.float64))).any(axis=1).all()
        if corner == "mask-subnormal":
            assert not f_y.any()


@pytest.mark.parametrize("corner,n,mode", q.mask_params(), ids=_ids)
def test_a_mask_of_powers_of_two_is_a_product_on_the_host(corner, n, mode):
    """the pure variant: the mask is +-2^k, the spectra lie on the grid on which their product with it is a binary16 number, so the
    masked merge and the unmasked merge of the premultiplied planes are the same fp32 sums: the same Z' in every bit"""
    d = q.masked(corner, n, mode, pure=True)
    assert q.finite(d) and q.holds(d) and d["exact"] and _finite(d["pre_re"], d["pre_im"])
    mag = np.abs(d["mask"].astype(np.float64))
    assert np.array_equal(np.log2(mag), np.round(np.log2(mag))) and 0.2 < (d["mask"] < 0).mean() < 0.3
    plain = dict(d, re=d["pre_re"], im=d["pre_im"], mask=None)
    assert q.holds(plain)
    for a, b in zip(q.merged(d), q.merged(plain)):
        assert np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------------- spectrograms

@pytest.mark.parametrize("corner,n", SPEC_ALL, ids=_ids)
def test_spectrogram_model_stays_within_what_the_gpu_test_asserts(corner, n):
    d = sr.forward(corner, n)
    re, im = sr.model(d)
    nbins = sn.bins(n)
    sets = q.band_sets(n)
    assert set(sets) == set(q.BAND_SETS) and [s for s, _ in sets["signed"]] == [s for s, _ in spr.band_sets(n)["desc37"]]
    assert min(w.min() for _, w in sets["signed"]) < -0.9 and max(w.max() for _, w in sets["signed"]) > 0.9
    for name, gain in q.gains(n).items():
        p = spr.power(re, im, gain)
        assert _finite(p)
        p_ref = q.p64(d, gain)
        if corner in q.SPEC_UPPER:
            worst = float((np.abs(p.astype(np.float64) - p_ref).sum(-1) / p_ref.sum(-1)).max())
            print(f"spec {corner} n={n} gain {name}: model's worst frame sum|P - P64| / sum P64 = {worst:.2e} (asserted on the GPU: {spr.POWER_BOUND:.2e})")
            assert worst * q.MARGIN <= spr.POWER_BOUND
        else:
            assert (p[:, 0] != 0).all()
        # every step of both restatements stays a normal fp32 number (include/tfft_spec.h pins nothing below 2^-126)
        for band_name in q.BAND_SETS if name == "n2" else ():
            e = spr.band_energies(p, sets[band_name])
            assert _finite(e) and q.smallest_step(p, sets[band_name]) >= TINY32
            if corner in q.SPEC_UPPER and band_name != "signed":
                bound, e64 = spr.band_bound(p_ref, sets[band_name], nbins)
                worst = float((np.abs(e.astype(np.float64) - e64).sum(-1) / bound).max())
                assert worst * q.MARGIN <= 1.0, (band_name, worst)
        assert np.abs(p[p != 0]).min() >= TINY32


@pytest.mark.parametrize("corner,n", [(c, n) for n in q.LENGTHS for c in q.SPEC_LOWER], ids=_ids)
def test_spectrogram_bits_see_a_flush(corner, n):
    """the flushes stft_range_ref names for the set (the multiply's result or its operands) change P in every frame; on
    products-subnormal, whose bin 0 is a subnormal half in every frame, a conversion that flushes the halves in front of the power
    returns P[0] = 0"""
    d = sr.forward(corner, n)
    re, im = sr.model(d)
    p = spr.power(re, im, float(n) ** 2)
    for fault in sr.FAULTS[("forward", corner)]:
        f_re, f_im = sr.faulty(d, fault)
        differing = (spr.power(f_re, f_im, float(n) ** 2).view(np.uint32) != p.view(np.uint32)).sum(-1)
        print(f"spec {corner} n={n}, {fault} flushed: {differing.tolist()} of {p.shape[1]} powers differ per frame")
        assert (differing > 0).all()
    if corner == "products-subnormal":
        assert sr.subnormal(re[:, 0]).all()
        flushed = spr.power(sr.flush(re), sr.flush(im), float(n) ** 2)
        assert not flushed[:, 0].any() and (p[:, 0] != 0).all()


@pytest.mark.parametrize("n", q.LENGTHS)
def test_signed_bands_tell_a_fused_sum_from_the_stated_one(n):
    d = sr.forward("signal-high", n)
    p = spr.power(*sr.model(d), float(n) ** 2)
    bands = q.band_sets(n)["signed"]
    stated, fused = spr.band_energies(p, bands), q.band_energies_fused(p, bands)
    differing = (stated.view(np.uint32) != fused.view(np.uint32)).sum(-1)
    print(f"spec signed n={n}: a fused sum differs in {differing.tolist()} of 37 bands per frame")
    assert (differing > 0).all()


@pytest.mark.parametrize("n", q.LENGTHS)
def test_gain_overflow_set(n):
    """signal-high under gain 2^100 stays finite (max |S| about 2^10: P up to 2^121); under 2^110 part of every frame is +inf and
    part is finite; never a NaN"""
    re, im = sr.model(sr.forward("signal-high", n))
    with np.errstate(over="ignore"):
        low, high = spr.power(re, im, 2.0 ** 100), spr.power(re, im, 2.0 ** 110)
    assert not np.isnan(low).any() and not np.isnan(high).any()
    assert np.isposinf(high).any(axis=1).all() and np.isfinite(high).any(axis=1).all()
    print(f"spec gain-overflow n={n}: {int(np.isinf(low).sum())} / {int(np.isinf(high).sum())} of {low.size} powers are inf at gain 2^100 / 2^110")


# ---------------------------------------------------------------------------------------------------------------------- gradients

@pytest.mark.parametrize("n", q.LENGTHS)
@pytest.mark.parametrize("corner", ["grad-high", "grad-low"])
def test_gradient_sets(corner, n):
    """the adjoint plan's contract on c_k G: the docstring of differentiable_short_stft claims it holds for every finite binary16
    gradient between the edge bins; grad-high is the largest power of two on uniform(-1, 1), 2^15, where the gradient itself ends"""
    d = q.grad(corner, n)
    name, ratio = q.binding(d)
    print(f"grad {corner} n={n}: 2^{d['exponent']}, {name} at {ratio:.3f} of its limit")
    assert q.finite(d) and q.holds(d) and d["raw_only"] and "y" not in q.contract(d)
    v, dx = q.model(d, raw=True)
    assert _finite(v, dx) and (_bits(dx) & 0x7FFF != 0).any(axis=1).all()
    if corner == "grad-high":
        assert ratio >= 0.5 and d["exponent"] == 15
        dx64 = q.reference(d, raw=True)
        assert np.allclose(dx64, q.mr.adjoint64(d["re"], d["im"], d["w"], d["rows"], d["length"], d["hop"], d["pad"]), rtol=1e-12, atol=1e-9)
        scale = np.maximum(q.per_signal(q.frames64(d), d["rows"]), q.per_signal(dx64, d["rows"]))
        worst = float((q.per_signal(dx.astype(np.float64) - dx64, d["rows"]) / scale).max())
        bound = q.grad_bound(d["w"], *_shape(d))
        print(f"grad grad-high n={n}: model's worst signal {worst:.2e} (asserted on the GPU: {bound:.2e})")
        assert worst * q.MARGIN <= bound
    else:
        halves = np.concatenate((d["re"].reshape(-1), d["im"].reshape(-1)))
        assert (sr.subnormal(halves) | (halves == 0)).all() and sr.subnormal(halves).mean() > 0.99
        for fault in q.FAULTS[corner]:
            f_dx = q.faulty(d, fault, raw=True)[1]
            assert ((_bits(f_dx) != _bits(dx)).sum(-1) > 0).all(), fault


@pytest.mark.parametrize("n", q.LENGTHS)
def test_power_gradient_scales_with_powers_of_two(n):
    """gP 2^k (or gain 2^k) moves s alone: fp16(M / s) keeps its bits and y s is exact in fp32, so dx_k = dx_0 2^k wherever both are
    normal binary16 numbers. The fp64 gradient decides which k of {-30, -8, 6} the GPU test asserts: those at which at least half of
    the samples qualify."""
    gain = float(n) ** 2
    ks = q.power_exponents(n, gain)
    print(f"power gradient n={n}, gain n^2: share of samples normal at both scales {ks}; at gain 1 {q.power_exponents(n, 1.0)}")
    assert set(ks) == {-8, 6}
    dx0, d0 = q.power_grad_model(q.power_case(n, gain))
    assert _finite(dx0)
    for k in ks:
        for case in (q.power_case(n, gain, k), q.power_case(n, gain * 2.0 ** k)):
            dxk, dk = q.power_grad_model(case)
            assert np.array_equal(_bits(dk["mask"]), _bits(d0["mask"])) and dk["s"] == d0["s"] * 2.0 ** k
            both = q.normal16(dx0.astype(np.float64)) & q.normal16(dx0.astype(np.float64) * 2.0 ** k)
            assert both.mean() >= 0.5 and np.array_equal(dxk.astype(np.float64)[both], dx0.astype(np.float64)[both] * 2.0 ** k)


@pytest.mark.parametrize("n", q.LENGTHS)
def test_power_gradient_with_one_dominant_entry(n):
    """gP = uniform(-1, 1) with one entry of 2^20, gain 1: s = 2^(21 - log2 n) and the other entries of fp16(M / s) are subnormal or
    zero. The model is finite and within the bound of tests/test_gpu_mistftn.py relative to the dominant signal's scale."""
    p = q.power_case(n, 1.0, dominant=True)
    dx, d = q.power_grad_model(p)
    others = np.delete(d["mask"].reshape(-1), np.abs(d["mask"].astype(np.float64)).argmax())
    assert _finite(dx) and q.holds(d) and (sr.subnormal(others) | (others == 0)).all()
    dx64, v64 = q.power_grad64(p)
    scale = np.maximum(q.per_signal(v64, p["rows"]), q.per_signal(dx64, p["rows"])).max()
    worst = float((q.per_signal(dx.astype(np.float64) - dx64, p["rows"]) / scale).max())
    bound = q.grad_bound(p["w"], n, p["length"], p["hop"], p["pad"]) + q.K_FWD + q.K_MASK
    print(f"power gradient n={n}, one entry 2^20: model's worst signal {worst:.2e} of the dominant scale (asserted on the GPU: {bound:.2e})")
    assert worst * q.MARGIN <= bound
