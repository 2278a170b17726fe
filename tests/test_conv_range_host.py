"""The range contract of the convolution add-ons on the CPU (tests/range_ref.py): every input that tests/test_gpu_conv_range.py hands
to a GPU is checked here first, and the input condition of the sequentially scaled forward transform is derived and modelled.

The input condition. include/tfft.h used to say that sequential scaling keeps |intermediate| <= max |x| "so no finite input
overflows". That holds for the complex MAGNITUDE of a sample, not for one component: a radix-16 stage forms

    a = sum_{m < 16} c_m x_m,      c_m = fp16(w^(m k) / 16)   (component by component),

a mean of rotated samples. With |x_m| <= B it has |a| <= B (1 + 2^-11) (each component of c_m is a normal binary16 number with a
relative error of at most 2^-11, so |c_m| <= (1 + 2^-11) / 16), but Re a alone can reach that value although every Re x_m, Im x_m is
only B / sqrt 2: for x_m = A (sgn cos + i sgn sin)(2 pi m / 16), Re a = (A / 16) sum_m (|cos| + |sin|)(2 pi m / 16) = 1.2568 A.
The kernels round both components to binary16 behind every stage and do not clamp, so the condition is on the magnitude:

  * the fp32 accumulation of 16 products adds at most 16 x 2^-24 = 2^-20 relative to sum |c_m| |x_m|, the fp32 twiddle of the
    second stage (|w| <= 1 + 2^-23, one fma per component) 2^-22: together below a factor 1 + 2^-19 per stage;
  * the rounding of the two components to binary16 grows the magnitude by at most 1 + 2^-11.

So with |x| <= M the largest fp32 value in front of the rounding of stage s is at most M (1 + 2^-11)^(2 s - 1) (1 + 2^-19)^s, and it
becomes a finite binary16 number when it is below 65520. For the S = 3 stages of the N = 4096 kernels that is M < 65359.9; the
contract states M = 63 * 2^10 = 64512 (range_ref.M), which holds up to S = 16 stages:
(1 + 2^-11)^31 (1 + 2^-19)^16 = 1.01527 < 65520 / 64512 = 1.015625, more stages than any plan of the library has (a radix-16 stage
per four bits of the length, plus at most one front-end or combine stage). Both rows of a pair may therefore be as large as
A_PAIR = the largest binary16 <= M / sqrt 2 = 45600 at once.

A transform of N = 4096 with an all-zero plane (the zero partner of an odd row count, a real signal) is exempt: any finite input
passes. The argument and the model below cover the three radix-16 stages of the N = 4096 kernels, which is where the convolution
add-ons meet a row without partner (every overlap-save window and every fused causal plan); for other lengths the exemption rests
only on the full-scale constant and alternating rows of tests/test_gpu_parity.py::test_full_scale_inputs_do_not_overflow.
Real x_m have the phase 0 or pi. Where the w^(m k) of a stage are all +-1 (k = 0, 8) or +-1, +-i (k = 4, 12) the constants are exact
in binary16: a is real with |a| <= B exactly, or complex with both components <= B / 2. At every other k the rotations point in
at least eight directions, and sum_m |Re(w^(m k) e^(-i phi))| / 16 <= (cos(pi / 8) + sin(pi / 8)) / 2 = 0.6533 in every direction
phi (test_model_full_scale_real_rows_stay_finite evaluates it). So behind a stage with real input a value is real and at most B, or
complex and at most 0.7072 B (1 + 2^-11); the real ones meet the next stage the same way (its constants for them are again powers
of w16, or 16 of the 32 directions of w32 with the bound 0.6533), the complex ones keep their magnitude up to the factors above.

M is derived, not tuned on a GPU. The numpy model of tests/stage_model.py (three stages, binary16 constants, one rounding per stage; the
layout of tensor-fft_amd/csrc/k4096.hpp) is held to it: finite at |x| = M for tones, whose stages all add in phase, and for the corner
signals at A_PAIR, finite for full-scale real rows, and NOT finite for the corner signals at A = 65504, the one place in the
repository where that input is computed: no GPU test feeds it.
"""
import numpy as np
import pytest

import bconv_ref as br
import conv_ref
import elementwise_bound as eb
import range_ref as rr
import sconv_ref as sr
from stage_model import F1, G2, H3, TW, _I, _c16, _cexp, _stages, stage_model     # noqa: F401

N = rr.N


# ---- every GPU input: the contract holds within a factor 2 of binding, the reference is finite, the tolerances are usable

def _check_reference_and_tolerance(d):
    y, peak = rr.reference(d)
    assert np.isfinite(y.real).all() and np.isfinite(y.imag).all()
    if d["addon"] in rr.TAP_GRADS:
        # the derived bound of the tap gradient, from the items NOT divided by 4096
        tol = br.dh_bound(y * N, d["x"].shape[1])
    else:
        tol = rr.constant_of(d) * eb.ulp16(peak)
    assert np.isfinite(tol).all() and (tol > 0).all()
    return peak


@pytest.mark.parametrize("addon,case,kind,corner", rr.upper_edge_params(), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_upper_edge_inputs_meet_the_contract_within_a_factor_2(addon, case, kind, corner):
    d = rr.upper_edge_data(addon, case, kind, corner)         # scaled() asserts: finite, exact scaling, binding in (1/2, 1]
    c = rr.contract(d)
    assert all(v <= limit for v, limit in c.values()), c
    assert max(v / limit for v, limit in c.values()) > 0.5, c
    _check_reference_and_tolerance(d)
    # the corner is what its name says: relative to the amplitude-1 case max |X H| moved by the power of two of the scaling
    # (up to what the gates' subnormal products at amplitude 1 gain in precision)
    if corner != rr.GATE_CORNER:
        base = rr.base(addon, case, kind, 1, rr.UPPER_MODE.get(addon, ""))
        ratio = rr.contract(d)["xh"][0] / rr.contract(base)["xh"][0]
        assert ratio > 1.0 and (corner == "signal-full" or abs(np.log2(ratio) - round(np.log2(ratio))) < 1e-6), ratio


def test_upper_edge_covers_the_top_two_decades():
    """the host tests of the add-ons record max |X H| = 137 .. 222 of 32752; here the signal-full corners carry samples beyond 2^14
    (that every case binds within a factor 2 is asserted case by case above)"""
    for addon, case, kind, corner in rr.upper_edge_params(rr.FORWARD):
        d = rr.upper_edge_data(addon, case, kind, corner)
        if corner == "signal-full":
            assert max(float(np.abs(d[k].astype(np.float64)).max()) for k in rr.SIGNAL[addon]) > 2.0 ** 14, (addon, case, kind)


CORNER_CONV = [(N, False), (256, True), (1 << 16, True)]
CORNER_ADDONS = ("sconv", "gsconv", "bconv_dx", "gbconv_dx")


@pytest.mark.parametrize("k", rr.CORNER_K)
def test_corner_signal_inputs_meet_the_corrected_contract(k):
    for amplitude, partner in ((rr.A_PAIR, True), (rr.A_FULL, False)):
        sets = [rr.corner_conv(amplitude, k, n, composed, partner) for n, composed in CORNER_CONV]
        sets += [rr.corner_case(addon, amplitude, k, partner) for addon in CORNER_ADDONS]
        for d in sets:
            c = rr.contract(d)
            assert all(v <= limit for v, limit in c.values()), (d["addon"], d["case"], c)
            peak = _check_reference_and_tolerance(d)
            # the answer is the stated power of two times the input: the reference says so too
            assert np.isfinite(peak).all() and (peak > 2.0 ** -14).all()
    # ... and the pair at full scale meets the contract AS IT WAS WRITTEN, and only misses the new quantity
    for d in [rr.corner_conv(rr.A_FULL, k, N, False)] + [rr.corner_case(addon, rr.A_FULL, k) for addon in CORNER_ADDONS]:
        c = rr.contract(d)
        assert [name for name, (v, limit) in c.items() if v > limit] == ["input"], c
        assert 20000 < c["xh"][0] < 21000 and c["y"][0] < 8                  # about 20 900 of 32752; max |y| about 4


def test_corner_answers_are_exact_powers_of_two():
    d = rr.corner_case("gbconv_dx", rr.A_PAIR, 16)
    gz = rr.gr.half_product(d["post"], d["gy"]).astype(np.float64)
    assert np.array_equal(2.0 ** -15 * gz, d["expected"]["dx"]) and np.array_equal(2.0 ** -12 * gz, d["expected"]["dpre"])
    d = rr.corner_case("gsconv", rr.A_FULL, 1, partner=False)
    u = rr.gr.half_product(d["p"], d["x"]).astype(np.float64)
    assert np.abs(u).max() == 65504.0 and np.array_equal(2.0 ** -15 * u, d["expected"]["y"])
    for n, composed in CORNER_CONV:
        d = rr.corner_conv(rr.A_PAIR, 256, n, composed)
        y, _ = rr.reference(d)
        assert np.allclose(y.real, d["expected"][0], rtol=0, atol=1e-9) and np.allclose(y.imag, d["expected"][1], rtol=0, atol=1e-9)


@pytest.mark.parametrize("addon,side", [(a, s) for s in ("out", "in") for a in ("gconv", "gsconv", "gbconv_dx")] + [("gbconv_dh", "in")])
def test_gate_inputs_reach_the_subnormal_range_and_a_flushing_multiply_would_differ(addon, side):
    d = rr.subnormal_gate_data(addon, side)          # asserts the contract and where the subnormals are
    c = rr.contract(d)
    assert all(v <= limit for v, limit in c.values()), c
    y, peak = rr.reference(d)
    assert np.isfinite(y.real).all() and np.isfinite(y.imag).all() and (peak > 0).all()
    if side == "out":
        # the products the kernel forms with the small gate: subnormal and not zero, so flushing inputs or outputs changes them
        gate = d["g"] if "g" in d else d["pre"]
        tiny = rr.gr.half_product(gate, np.float16(0.5))
        assert (rr._subnormal(tiny).mean() > 0.9) and (np.abs(tiny.astype(np.float64)) > 0).mean() > 0.9


def test_the_yardstick_product_keeps_subnormals():
    """half_product, the host side of every bit-for-bit comparison of the gate tests, is an IEEE multiply: (3/4 x 2^-14) x 1/2 =
    3 x 2^-17, a subnormal; 2^-24 x 1/2 is a tie that rounds to the even neighbour zero, 3 x 2^-24 x 1/2 to 2 x 2^-24"""
    h, product = np.float16, rr.gr.half_product
    assert float(product(h(0.75 * 2.0 ** -14), h(0.5))) == 3 * 2.0 ** -17
    assert float(product(h(2.0 ** -24), h(0.5))) == 0.0 and float(product(h(3 * 2.0 ** -24), h(0.5))) == 2.0 ** -23
    assert float(product(h(2.0 ** -24), h(1024.0))) == 2.0 ** -14


# ---- the numpy model of the forward transform at N = 4096 (tests/stage_model.py, which also models the other single-pass kernels)


def fused_route_model(re, im, h):
    """conv4096's route for a filter that is the real constant h at every bin: the three stages with the last one left in fp32,
    times h * 4096, ONE rounding, the planes exchanged, the same three stages, rounded: six roundings in all"""
    x = np.asarray(re, np.float16).astype(np.float64) + 1j * np.asarray(im, np.float16).astype(np.float64)
    z = _c16(_stages(x, False) * (h * N))
    y = _stages(z.imag + 1j * z.real, True)
    return y.imag + 1j * y.real


def test_model_of_the_fused_route_on_the_lone_full_scale_row():
    """What tests/test_gpu_conv_range.py measured on the corner signals, from the arithmetic alone: both rows at A_PAIR stay within
    2 ulp of the exact answer, the lone row at 65504 reaches exactly 4.0 ulp for k = 1 (2.0 for k = 16, 1.0 for k = 256). That row is
    +-3.998 at every sample: the top of a binade, so the unit is half the spacing of the intermediates above it, and the roundings
    of its one dominant tone add up. K_CONV_FUSED = 3.5 and K_LCONV_FUSED = 3.5 are constants for signals whose peak is 2 to 3 x
    their rms (profiles/conv_ulps.txt) and do not cover this row; K_SCONV = 4.0 just does."""
    gain = rr.corner_gain(N)
    worst = {}
    for amplitude, partner in ((float(rr.A_PAIR), True), (65504.0, False)):
        for k in rr.CORNER_K:
            re, im = rr.corner_signals(amplitude, k)
            im = im if partner else np.zeros_like(im)
            y = fused_route_model(re, im, gain)
            want = gain * (re.astype(np.float64) + 1j * im.astype(np.float64))
            worst[partner, k] = float(eb.errors_in_ulps(y.real, y.imag, want.real, want.imag).max())
    assert max(worst[True, k] for k in rr.CORNER_K) <= 2.0, worst
    # (4.0 with this summation order; another order of the fp32 sums may move single roundings, not the class)
    assert conv_ref.K_CONV_FUSED < worst[False, 1] <= sr.K_SCONV and worst[False, 16] <= 2.0 and worst[False, 256] <= 2.0, worst


def test_stage_model_is_the_transform():
    rng = np.random.default_rng(5)
    re, im = rng.uniform(-1, 1, N).astype(np.float16), rng.uniform(-1, 1, N).astype(np.float16)
    got, _ = stage_model(re, im)
    want = np.fft.fft(re.astype(np.float64) + 1j * im.astype(np.float64)) / N
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag)).max() / eb.ulp16(np.abs(want).max())
    assert err <= eb.K_TABLE, err
    # a tone lands in one bin
    tone = rr.M * _cexp(-273 * np.arange(N), N)
    got, _ = stage_model(*_towards_zero(tone))
    assert np.argmax(np.abs(got)) == 273 and abs(abs(got[273]) - rr.M) < 64


def _towards_zero(z):
    """the complex samples as binary16 planes, each component rounded towards zero: the magnitude does not grow"""
    def down(v):
        h = v.astype(np.float16)
        over = np.abs(h.astype(np.float64)) > np.abs(v)
        return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float16)
    return down(z.real), down(z.imag)


def test_the_bound_m_of_the_derivation():
    s = 3
    assert rr.M * (1 + 2.0 ** -11) ** (2 * s - 1) * (1 + 2.0 ** -19) ** s < 65520
    assert 65359 * (1 + 2.0 ** -11) ** (2 * s - 1) * (1 + 2.0 ** -19) ** s < 65520 < 65361 * (1 + 2.0 ** -11) ** (2 * s - 1) * (1 + 2.0 ** -19) ** s
    s = 16
    assert rr.M * (1 + 2.0 ** -11) ** (2 * s - 1) * (1 + 2.0 ** -19) ** s < 65520
    assert rr.M == 63 * 1024 and float(rr.A_PAIR) == 45600.0 and float(rr.A_PAIR) * np.sqrt(2) <= rr.M < (float(rr.A_PAIR) + 32) * np.sqrt(2)
    # the binary16 constants: every non-zero component is normal, every |c_m| <= (1 + 2^-11) / 16
    for table in (F1, G2, H3):
        parts = np.concatenate((np.abs(table.real).ravel(), np.abs(table.imag).ravel()))
        assert parts[parts > 0].min() >= 2.0 ** -14 and np.abs(table).max() <= (1 + 2.0 ** -11) / 16


@pytest.mark.parametrize("k", [1, 16, 256, 273, 4095])
def test_model_tones_at_the_bound_stay_finite(k):
    """all 16 terms of every stage add in phase: the magnitude stays at M through the three stages, on one axis where the phase allows"""
    for phase in (0.0, np.pi / 4, 1.0):
        got, peaks = stage_model(*_towards_zero(rr.M * np.exp(1j * phase) * _cexp(-k * np.arange(N), N)))
        assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
        assert max(peaks) <= rr.M * (1 + 2.0 ** -11) ** 5 * (1 + 2.0 ** -19) ** 3 < 65520


@pytest.mark.parametrize("k", rr.CORNER_K)
def test_model_corner_signals(k):
    """finite at A_PAIR with a component of 1.2568 A behind the stage whose stride matches k (stride 256: k = 1, stride 16: k = 16,
    contiguous: k = 256); NOT finite at A = 65504: the overflow the contract now excludes"""
    a = float(rr.A_PAIR)
    got, peaks = stage_model(*rr.corner_signals(a, k))
    assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
    stage = {1: 0, 16: 1, 256: 2}[k]
    assert 1.2568 - 2e-3 < peaks[stage] / a < 1.2814 + 2e-3, peaks         # 1.2568 from the sum; stage 2's twiddle can add to it
    # behind it the fp32 twiddle may turn the value (magnitude 1.2813 A = 0.906 of the input's A sqrt 2) onto an axis
    assert 1.2568 - 2e-3 < max(peaks) / a < 1.2814 + 2e-3 and max(peaks) < 65504
    got, peaks = stage_model(*rr.corner_signals(65504.0, k))
    assert not (np.isfinite(got.real).all() and np.isfinite(got.imag).all())
    assert peaks[stage] > 1.25 * 65504


def test_model_full_scale_real_rows_stay_finite():
    t = np.arange(N)
    zero = np.zeros(N, np.float16)
    rows = [np.full(N, 65504.0), 65504.0 * (-1.0) ** t, 65504.0 * (-1.0) ** (t // 16), 65504.0 * (-1.0) ** (t // 256)]
    rows += [rr.corner_signals(65504.0, k)[0].astype(np.float64) for k in rr.CORNER_K + (3, 273)]
    rng = np.random.default_rng(9)
    rows += [65504.0 * rng.choice([-1.0, 1.0], N) for _ in range(8)]
    for row in rows:
        row = row.astype(np.float16)
        for planes in ((row, zero), (zero, row)):
            got, peaks = stage_model(*planes)
            assert np.isfinite(got.real).all() and np.isfinite(got.imag).all() and max(peaks) <= 65504.0
    # the per-stage worst case of a real input in the direction phi: sum_m |Re(w^(m k) e^(-i phi))| / 16
    phis = np.linspace(0, np.pi, 2881)
    gain = {k: max(np.abs((_cexp(_I * k, 16) * np.exp(-1j * phi)).real).sum() / 16 for phi in phis) for k in range(16)}
    assert gain[0] == gain[8] == 1.0 and abs(gain[4] - np.sqrt(0.5)) < 1e-6 and abs(gain[12] - np.sqrt(0.5)) < 1e-6
    assert max(g for k, g in gain.items() if k % 4) <= (np.cos(np.pi / 8) + np.sin(np.pi / 8)) / 2 + 1e-9
    # ... and of the second stage's tile k0 = 8 (w32^(n1 (1 + 2 k1))): 16 of 32 directions
    assert max(np.abs((_cexp(_I * (1 + 2 * k1), 32) * np.exp(-1j * phi)).real).sum() / 16 for k1 in range(16) for phi in phis[::8]) <= 0.6533
