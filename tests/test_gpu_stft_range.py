"""The STFT, short-frame STFT and ISTFT plans at the edges of their range contract, on the GPU (include/tfft_stft.h, tfft_stftn.h,
tfft_istft.h). Every other GPU test of these plans feeds uniform(-1, 1) signals under a window of at most 1. Here the data sets of
tests/stft_range_ref.py run through the runners of tests/test_gpu_stft.py, test_gpu_stftn.py and test_gpu_istft.py (guard zones, NaN
gaps, input unchanged, all kept):

  forward   every set bit for bit TfftRealPlan(n, R F).r2c on host-built frames. That yardstick was never run near full scale, so the
            upper-edge sets (signal-high, window-high, split-high: the pair magnitude within a factor 2 of 64512; the corner
            signals at A_PAIR = 45600 on both frames of a pair and on a self-paired frame) are ALSO held to fp64 rfft / n of the
            binary16 products: finite, per-frame rel-L2 <= K_RFFT, the suites' own constant, not widened (arithmetic away from
            underflow is covariant under powers of two). The lower-edge sets (products-subnormal, x-subnormal, mixed-pair) are held
            by the bits alone, which tests/test_stft_range_host.py shows to differ in every frame for a flushing multiply or load;
            bin 0 of no frame is zero, and mixed-pair meets the pair-relative bound of tests/test_gpu_rfft.py.
  inverse   every set through the two comparisons of test_gpu_istft._check_case, with and without raw_sum: the workspace frames
            against merge_gain -> TfftPlan.exec_inverse, y against istft_ref.ola of the frames as read back. spectra-high and the
            tones at the input condition's limit also against fp64; a window times 2^k gives fp16(2^-k q_unit) in every bit, q_unit
            the unit window's fp32 quotient (the unit window's own output wherever 2^-k y_unit is a binary16 number);
            output-subnormal returns non-zero subnormals.
  wrappers  stft(), istft() and the round trip at the upper scale.

That the lower-edge cases see what they are there for was also tried on the GPU, once and by hand: builds of the add-ons whose `mul8`
flushes subnormal products fail products-subnormal, x-subnormal and mixed-pair at every n (2032 .. 8027 halves of the RE plane at
n = 4096) while every upper-edge case still passes; a build whose merge flushes its loaded spectra, and one whose overlap-add flushes
its output conversion, fail both subnormal sets and both window sets of the inverse.

No bound here was chosen by looking at the kernels: each is a constant of the existing suites (asserted to be the same) or a bit
comparison. tests/test_stft_range_host.py checks every input of this file on the CPU first. Measured over three seeds:
profiles/stft_range.txt (tools/stft_range_accuracy.py)."""
import numpy as np
import pytest

import istft_ref as ir
import stft_range_ref as sr
import stft_ref as st
import test_gpu_istft as t_istft
import test_gpu_stft as t_stft
import test_gpu_stftn as t_stftn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    return tensor_fft_amd


def test_the_constants_are_the_suites_own():
    assert (sr.K_RFFT, sr.K_RFFT) == (t_stft.K_RFFT, t_stftn.K_RFFT) and (sr.K_C2R, sr.K_FWD) == (t_istft.K_C2R, t_istft.K_FWD)


# ------------------------------------------------------------------------------------------------------------------------ forward

def run_forward(tf, d):
    """(re, im) int16 bit patterns [R F][n / 2 + 1] of the set through its plan, between guard zones (the suites' runners)"""
    x, w = d["x"].copy(), d["w"].copy()
    if d["n"] == st.N:
        return t_stft.run_stft(tf, x, w, d["hop"], d["pad"])
    return t_stftn.run_stftn(tf, d["n"], x, w, d["hop"], d["pad"])


def via_real_plan(tf, d):
    u = sr.frames(d)
    return t_stft.via_real_plan(tf, u) if d["n"] == st.N else t_stftn.via_real_plan(tf, d["n"], u)


_forward = {}


def forward_result(tf, d):
    """(re, im) of one forward set, run once per module and held to the composition on the way"""
    key = (d["corner"], d["n"])
    if key not in _forward:
        got = run_forward(tf, d)
        t_stft._assert_bits(f"stft range {d['corner']} n={d['n']}", got, via_real_plan(tf, d))
        _forward[key] = got
    return _forward[key]


def check_forward(tf, d):
    """the composition, and for an upper-edge set fp64: returns the worst frame's rel-L2 against fp64 of the binary16 products"""
    re, im = forward_result(tf, d)
    got = sr.as_complex(re.view(np.float16), im.view(np.float16))
    with np.errstate(invalid="ignore"):
        worst = float(sr.rel_l2(got, sr.reference(d)).max())
    if d["corner"] in sr.UPPER_FORWARD or d["outside"]:
        assert np.isfinite(got.real).all() and np.isfinite(got.imag).all(), f"{d['corner']} n={d['n']}: inf or NaN inside the input condition"
        print(f"stft range {d['corner']} n={d['n']}: worst frame rel-L2 {worst:.2e} against fp64 of the binary16 products")
        assert worst <= sr.K_RFFT, (d["corner"], d["n"], worst)
    return worst


@pytest.mark.parametrize("corner,n", sr.forward_params(sr.UPPER_FORWARD), ids=str)
def test_forward_upper_edge(tf, corner, n):
    d = sr.forward(corner, n)
    name, ratio = sr.binding(d)
    assert sr.holds(d) and ratio >= 0.5
    check_forward(tf, d)


@pytest.mark.parametrize("corner,n", sr.forward_params(sr.LOWER_FORWARD), ids=str)
def test_forward_keeps_subnormals(tf, corner, n):
    """u = fp16(w x) with subnormal products (products-subnormal, frame 1 of mixed-pair) or subnormal operands (x-subnormal): the
    frames built on the host keep them (one IEEE rounding), so a multiply or a load in a flushing mode differs from the yardstick in
    every frame (tests/test_stft_range_host.py), and returns zeros where bin 0 is asserted not to be."""
    d = sr.forward(corner, n)
    check_forward(tf, d)
    re, im = forward_result(tf, d)
    assert (re[:, 0] & 0x7FFF != 0).all(), f"{corner} n={n}: bin 0 of a frame is zero"
    if corner == "mixed-pair":
        got, want = sr.as_complex(re.view(np.float16), im.view(np.float16)), sr.reference(d)
        u = sr.frames(d).astype(np.float64)
        top = np.abs(np.fft.fft(u[0] + 1j * u[1]) / n).max()
        worst = float(np.abs(got - want).max() / top)
        print(f"stft range mixed-pair n={n}: max abs error {worst:.2e} of the pair's largest bin")
        assert worst <= sr.K_PAIR


def test_self_paired_frame_at_65504_where_the_model_stays_finite(tf):
    """The one set outside the contract, decided on the CPU (tests/test_stft_range_host.py): the self-paired frame holding the k = 1
    corner signal at 65504. It is fed only at the lengths at which the model does not overflow (all four, as recorded there), and
    then meets what the sets inside the contract meet."""
    for n in sr.LENGTHS:
        d = sr.forward("corner-self-outside", n)
        assert d["outside"] and not sr.holds(d)
        m_re, m_im = sr.model(d)
        if np.isfinite(m_re.astype(np.float64)).all() and np.isfinite(m_im.astype(np.float64)).all():
            check_forward(tf, d)


# ------------------------------------------------------------------------------------------------------------------------ inverse

_inverse = {}


def check_inverse(tf, d, raw=False):
    """test_gpu_istft._check_case with the data passed in: (frames, y) int16 bit patterns, run once per module. The workspace frames
    against merge_gain -> TfftPlan.exec_inverse, y against istft_ref.ola of the frames as read back."""
    key = (d["corner"], raw)
    if key in _inverse:
        return _inverse[key]
    rows, length, hop, pad = d["rows"], d["length"], d["hop"], d["pad"]
    re, im, w = d["re"].copy(), d["im"].copy(), d["w"].copy()
    frames, y = t_istft.run_istft(tf, re, im, w, rows, length, hop, pad, 0, raw)
    what = f"istft range {d['corner']}{' raw' if raw else ''}"
    assert not np.isnan(frames.view(np.float16)).any(), what + ": a NaN reached the frames"
    zr, zi = ir.merge_items(re, im)
    t_istft._assert_bits(what + ", frames against merge_gain -> TfftPlan.exec_inverse", frames, t_istft.via_inverse_plan(tf, zr, zi, re.shape[0]))
    want_y = ir.ola(frames.view(np.float16), w, rows, length, hop, pad, raw=raw).view(np.int16)
    t_istft._assert_bits(what + ", output against istft_ref.ola of the workspace frames", y, want_y, ("signal", "sample"))
    _inverse[key] = (frames, y)
    return _inverse[key]


def both_ways(tf, d):
    frames, y = check_inverse(tf, d)
    raw_frames, raw_y = check_inverse(tf, d, raw=True)
    assert np.array_equal(frames, raw_frames)
    assert np.isfinite(y.view(np.float16)).all() and np.isfinite(raw_y.view(np.float16)).all()
    return frames, y


@pytest.mark.parametrize("corner", sr.UPPER_INVERSE)
def test_inverse_at_the_input_condition(tf, corner):
    """spectra-high: noise spectra with max |Z'| within a factor 2 of 64512. tone-edge: the largest tone (22.27) and constant (11.13) a
    rectangular window lets through, max |Z'| at 0.9996 of the limit. Finite, and per signal within the bound of
    tests/test_gpu_istft.py against the fp64 ISTFT of the same spectra (a rectangular window: K_C2R sqrt 2 + 2^-11)."""
    d = sr.inverse(corner)
    assert sr.holds(d) and sr.binding(d)[1] >= 0.5
    _, y = both_ways(tf, d)
    if corner == "spectra-high":
        bound = t_istft._accuracy_bound(d["w"], d["length"], d["hop"], d["pad"])
        assert bound == sr.istft_bound(d["w"], d["length"], d["hop"], d["pad"])
    else:
        bound = sr.K_C2R * np.sqrt(2.0) + 2.0 ** -11
    worst = float(sr.rel_l2(y.view(np.float16).astype(np.float64), sr.reference(d)).max())
    print(f"istft range {corner}: worst signal rel-L2 {worst:.2e} against the fp64 ISTFT of the same spectra (bound {bound:.2e})")
    assert worst <= bound


@pytest.mark.parametrize("corner", sr.WINDOW_INVERSE)
def test_a_power_of_two_on_the_window_changes_no_bit_of_the_quotient(tf, corner):
    """Hann 2^15 and uniform(0.5, 1) 2^-8: num scales by 2^k and den by 2^2k, exactly in fp32 (tests/test_stft_range_host.py), so
    y = fp16(2^-k q_unit) with q_unit the fp32 quotient of the unit window's run: the unit window's y in every bit wherever 2^-k
    y_unit is a binary16 number, and one rounding of the same quotient where it is not (k = 15: most of y is subnormal). The raw
    sum is held to the composition alone."""
    d = sr.inverse(corner)
    unit = sr.unit_window(d)
    frames, y = both_ways(tf, d)
    unit_frames, unit_y = check_inverse(tf, unit)
    assert np.array_equal(frames, unit_frames)                             # the frames do not depend on the window
    want = sr.scaled_window_output(unit_frames.view(np.float16), d)
    t_istft._assert_bits(f"istft range {corner}, y against 2^{-d['k']} x the unit window's quotient", y, want.view(np.int16), ("signal", "sample"))
    y_unit = unit_y.view(np.float16)
    exact = y_unit.astype(np.float64) * 2.0 ** -d["k"]
    with np.errstate(over="ignore"):
        same = (exact.astype(np.float16).astype(np.float64) == exact) & ~sr.subnormal(y_unit)
    assert same.any() and np.array_equal(y.view(np.float16).astype(np.float64)[same], exact[same])


@pytest.mark.parametrize("corner", sr.LOWER_INVERSE)
def test_inverse_keeps_subnormals(tf, corner):
    """spectra-subnormal: the input halves are subnormal; output-subnormal: so are the frames and y. The yardsticks keep them (the
    shipped inverse plan on host-merged spectra, istft_ref.ola in IEEE arithmetic), so a load, a conversion in front of the gain or
    an output conversion that flushes differs in every signal (tests/test_stft_range_host.py)."""
    d = sr.inverse(corner)
    _, y = both_ways(tf, d)
    assert (y & 0x7FFF != 0).any(axis=1).all()
    if corner == "output-subnormal":
        share = float(sr.subnormal(y.view(np.float16)).mean())
        print(f"istft range output-subnormal: {share:.3f} of y are non-zero subnormals")
        assert share >= 0.9


# ----------------------------------------------------------------------------------------------------------------------- wrappers

def test_wrappers_at_the_upper_scale(tf):
    """stft() and istft() at the signal-high / spectra-high scale match the plans' bits, and the round trip istft(stft(x 2^e)) meets
    the existing bound _accuracy_bound + K_FWD against x 2^e."""
    tf.stft_cache_clear()
    tf.stftn_cache_clear()
    tf.istft_cache_clear()
    try:
        for n in sr.LENGTHS:
            d = sr.forward("signal-high", n)
            re, im = forward_result(tf, d)
            g_re, g_im = tf.stft(torch.from_numpy(d["x"].copy()).to(DEV), torch.from_numpy(d["w"].copy()).to(DEV), d["hop"], n_fft=n)
            bins = n // 2 + 1
            assert np.array_equal(g_re.cpu().numpy().view(np.int16).reshape(-1, bins), re) and np.array_equal(g_im.cpu().numpy().view(np.int16).reshape(-1, bins), im)
        d = sr.inverse("spectra-high")
        _, y = check_inverse(tf, d)
        v_re, v_im = t_istft._stft_layout(d["re"], d["im"], d["rows"])
        d_w = torch.from_numpy(d["w"].copy()).to(DEV)
        got = tf.istft(v_re, v_im, d_w, d["hop"], d["length"], center=True)
        assert np.array_equal(got.cpu().numpy().view(np.int16), y)
        # the round trip at that scale: x 2^e, e the exponent of spectra-high
        x = d["x"]
        g_re, g_im = tf.stft(torch.from_numpy(x.copy()).to(DEV), d_w, d["hop"], center=True)
        trip = dict(d, re=g_re.cpu().numpy(), im=g_im.cpu().numpy().copy())
        trip["re"] = trip["re"].reshape(-1, st.BINS)
        trip["im"] = trip["im"].reshape(-1, st.BINS)
        trip["im"][:, [0, st.BINS - 1]] = 0                                # (ignored by the plan; keep the contract's fp64 side clean)
        assert sr.holds(trip), sr.contract(trip)
        back = tf.istft(g_re, g_im, d_w, d["hop"], d["length"], center=True).cpu().numpy()
        bound = t_istft._accuracy_bound(d["w"], d["length"], d["hop"], d["pad"]) + t_istft.K_FWD
        worst = float(ir.rel_l2(back, x).max())
        print(f"istft(stft(x 2^{d['exponent']})) against x 2^{d['exponent']}: worst signal rel-L2 {worst:.2e} (bound {bound:.2e})")
        assert np.isfinite(back).all() and worst <= bound
    finally:
        tf.stft_cache_clear()
        tf.stftn_cache_clear()
        tf.istft_cache_clear()
