"""The seven convolution add-ons at the edges of their range contract, on the GPU (include/tfft_conv.h, tfft_lconv.h, tfft_gconv.h,
tfft_sconv.h, tfft_gsconv.h, tfft_bconv.h, tfft_gbconv.h). Every other GPU test of these add-ons feeds uniform(-1, 1) signals and taps that
sum to about 1: max |X H| = 137 .. 222 of the allowed 32752. Here the same small cases run

  a. at the upper edge: signal-high, filter-high, signal-full and (gated plans) gates-high of tests/range_ref.py, every contract
     quantity within a factor 2 of its limit, through the add-on's OWN check function with its own constants (bit for bit against
     the composition of shipped code, fp64 with the plan's spectrum, rel-L2, the true result, the exact shifted input) and nothing
     widened: arithmetic away from underflow is covariant under powers of two. A pack to binary16 in front of the exact
     power-of-two factor, the x 4096 of wreduce_kernel in the wrong precision or a stage without its 1 / R fail here;
  b. on the adversarial signals of the forward transform's input condition, A (sgn cos + i sgn sin), whose stage sums put
     1.2568 A on one component: finite, the known answer and bit for bit the composition at A_PAIR = 45600 (the contract's bound
     M / sqrt 2 on both rows of a pair), and for the overlap-save plans at 65504 on a row without partner. The pair at 65504 is NOT fed: the contract excludes it, and
     tests/test_conv_range_host.py shows on the CPU that it overflows;
  c. with gates that put binary16 subnormals into u = p (.) x (or gz) and into y, dx and dpre: bit for bit the ungated shipped
     plan between host-built IEEE products (subnormals kept). A gate multiply in a flushing mode fails each of these.

tests/test_conv_range_host.py checks every input of this file on the CPU first (contract, finite reference, usable tolerances).
Measured over three seeds: profiles/range_ulps.txt (tools/range_accuracy.py)."""
import numpy as np
import pytest

import elementwise_bound as eb
import range_ref as rr
import sconv_ref as sr
import test_gpu_bconv as t_bconv
import test_gpu_conv as t_conv
import test_gpu_gbconv as t_gbconv
import test_gpu_gconv as t_gconv
import test_gpu_gsconv as t_gsconv
import test_gpu_lconv as t_lconv
import test_gpu_sconv as t_sconv

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    return tensor_fft_amd


def _ids(v):
    return "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


constant_of = rr.constant_of


def run_checks(tf, d):
    """the data set through its add-on's own checks (tests/test_gpu_<add-on>.py); returns the worst error the add-on reports: ulps
    of the unit of its constant, or for the gated input gradient and the tap gradients the ratio to the asserted bound"""
    addon, case, kind, exact = d["addon"], d["case"], d["kind"], d["exact_taps"]
    if addon == "conv":
        n, batch, filters, composed = case
        return t_conv._check_case(tf, n, batch, filters, composed, kind, data=(d["x_re"], d["x_im"], d["h_re"], d["h_im"]), exact_filter=exact)
    length, taps, rows, channels = case[:4]
    if addon == "lconv":
        return t_lconv.check_case(tf, length, taps, rows, channels, kind, constant_of(d), launch_iters=case[4], composed=case[5],
                                  data=(d["x"], d["h"]), exact_taps=exact)
    if addon == "gconv":
        return t_gconv.check_case(tf, length, taps, rows, channels, kind, d["mode"], constant_of(d), launch_iters=case[4], composed=case[5],
                                  data=(d["x"], d["h"], d.get("p"), d.get("g"), d.get("skip")), exact_taps=exact)
    if addon == "sconv":
        return t_sconv.check_case(tf, length, taps, rows, channels, kind, launch_iters=case[4], data=(d["x"], d["h"]), exact_taps=exact)
    if addon == "gsconv":
        return t_gsconv.check_case(tf, length, taps, rows, channels, kind, d["mode"], launch_iters=case[4],
                                   data=(d["x"], d["h"], d.get("p"), d.get("g"), d.get("skip")), exact_taps=exact)
    if addon == "bconv_dx":
        return t_bconv.check_dx_case(tf, length, taps, rows, channels, kind, launch_iters=case[4], data=(d["gy"], d["h"]), exact_taps=exact)
    if addon == "gbconv_dx":
        return t_gbconv.check_dx_case(tf, length, taps, rows, channels, kind, d["mode"], launch_iters=case[4],
                                      data=(d.get("x"), d["h"], d.get("pre"), d.get("post"), d.get("skip"), d["gy"]), exact_taps=exact)
    if addon == "bconv_dh":
        dh = t_bconv.run_wgrad(tf, d["x"], d["gy"], taps, case[4])
        t_bconv.check_dh_by_composition(tf, case, d["x"], d["gy"], dh)
        return t_bconv.check_dh_against_fp64(case, d["x"], d["gy"], dh)
    if addon == "gbconv_dh":
        return t_gbconv.check_dh_case(tf, tuple(case) + (d["mode"],), data=(d["x"], d.get("pre"), d.get("post"), d["gy"]))
    raise ValueError(addon)


# ------------------------------------------------------------------------------------------------------------------ a. upper edge

@pytest.mark.parametrize("addon,case,kind,corner", rr.upper_edge_params(), ids=_ids)
def test_upper_edge(tf, addon, case, kind, corner):
    d = rr.upper_edge_data(addon, case, kind, corner)
    name, ratio = rr.binding(d)
    worst = run_checks(tf, d)
    print(f"{addon} {case} {kind} {corner}: {name} at {ratio:.3f} of its limit, worst {worst:.3f}")
    assert np.isfinite(worst)                # the bounds themselves are asserted by the add-on's checks


# -------------------------------------------------------------------------------------------------------------- b. corner signals

def _bit_for_bit(got, want, what):
    a, b = got.astype(np.float32), want.astype(np.float32)
    assert not np.isnan(a).any() and not np.isnan(b).any() and np.array_equal(a, b), f"{what}: differs from the composition of shipped code in {int((a != b).sum())} samples"


@pytest.mark.parametrize("k", rr.CORNER_K)
@pytest.mark.parametrize("n,composed", [(rr.N, False), (256, True), (1 << 16, True)])
def test_corner_signal_conv(tf, n, composed, k):
    """a complex signal with both components at A_PAIR; H = corner_gain(n) at every bin, so y = gain * x exactly"""
    d = rr.corner_conv(rr.A_PAIR, k, n, composed)
    assert rr.holds(d)
    what = f"conv n={n} corner signal k={k} A={float(rr.A_PAIR)}"
    y_re, y_im = t_conv.run_conv(tf, n, 1, 1, composed, d["x_re"], d["x_im"], d["h_re"], d["h_im"])
    assert np.isfinite(y_re.astype(np.float64)).all() and np.isfinite(y_im.astype(np.float64)).all()
    worst = eb.check(y_re, y_im, *d["expected"], constant_of(d), what=what)
    print(f"{what}: worst {worst:.3f} ulp")
    if composed:
        # the composition yardstick of tests/test_gpu_conv.py: forward plan, cmul on the host, inverse plan
        w_re, w_im = t_conv.forward_cmul_inverse(tf, n, 1, 1, d["x_re"], d["x_im"], d["h_re"], d["h_im"])
        _bit_for_bit(y_re, w_re, what + " RE")
        _bit_for_bit(y_im, w_im, what + " IM")
    run_checks(tf, d)                      # ... and fp64 with the filter, the long way round


@pytest.mark.parametrize("k", rr.CORNER_K)
def test_lone_full_scale_row_through_conv4096(tf, k):
    """The row +-65504 without partner (IM plane zero) through the fused kernel itself, H = 2^-14: finite and within 4.0 ulp of the
    exact answer, the ceiling of the project's rule for a constant, NOT K_CONV_FUSED = 3.5: k = 1 measures 4.000 ulp (2.0 and 1.0 for
    k = 16 and 256). K_CONV_FUSED is a constant for signals whose peak is 2 to 3 x their rms (tests/conv_ref.py); every sample of
    this row sits at its peak, 3.998, the top of a binade, and the six roundings of its one dominant tone add up
    (tests/test_conv_range_host.py::test_model_of_the_fused_route_on_the_lone_full_scale_row restates them in numpy). This pins the
    figure where it arises; the overlap-save plans below meet the same arithmetic through their yardstick."""
    d = rr.corner_conv(rr.A_FULL, k, rr.N, False, partner=False)
    assert rr.holds(d)
    y_re, y_im = t_conv.run_conv(tf, rr.N, 1, 1, False, d["x_re"], d["x_im"], d["h_re"], d["h_im"])
    worst = eb.check(y_re, y_im, *d["expected"], 4.0, what=f"conv4096 lone row k={k} A=65504")
    print(f"conv4096 lone row k={k} A=65504: worst {worst:.3f} ulp")         # (the IM plane: rounding noise within the same bound)


def _expected_within(got, want, gate, k, peak, what):
    """|got - want| <= |gate| k ulp16(peak) + 1/2 ulp16(|got|) (tests/gsconv_ref.py); without a gate k ulp16(peak)"""
    got = got.astype(np.float64)
    assert np.isfinite(got).all(), what
    tol = k * eb.ulp16(peak) if gate is None else np.abs(gate.astype(np.float64)) * k * eb.ulp16(peak) + 0.5 * eb.ulp16(np.abs(got))
    err = np.abs(got - want)
    print(f"{what}: {float((err / tol).max()):.3f} x the bound")
    assert (err <= tol).all(), f"{what}: {float((err / tol).max()):.3f} x the bound"


@pytest.mark.parametrize("amplitude,partner", [(rr.A_PAIR, True), (rr.A_FULL, False)], ids=["pair-45600", "lone-65504"])
@pytest.mark.parametrize("k", rr.CORNER_K)
@pytest.mark.parametrize("addon", ["sconv", "gsconv", "bconv_dx", "gbconv_dx"])
def test_corner_signal_overlap_save(tf, addon, k, amplitude, partner):
    """L = 4096, K = 1, C = 1: one full window without halo, B = 2 with both rows at A_PAIR or B = 1 (a zero partner) at 65504. Taps,
    skip and gates are powers of two: the answer is a power of two times the input, exactly. Finite, within K_SCONV ulps of the
    window's peak of that answer, and bit for bit the add-on's composition yardstick (the shipped TfftConvPlan on host-built
    windows with the plan's own spectrum, the gates as host products).

    Measured: at most 2.0 ulp, except the lone row at 65504 with k = 1, where sconv and the input gradient reach exactly 4.000 ulp
    = K_SCONV. That is the arithmetic, not a fault: the numpy restatement of the six roundings of conv4096's route gives the same
    4.0 (tests/test_conv_range_host.py::test_model_of_the_fused_route_on_the_lone_full_scale_row). Every sample of that row sits
    at its peak, 65504 / 2^14 = 3.998, the top of a binade, so the unit is half the spacing of the intermediates above it (the
    fundamental alone is 4 / pi x 3.998 = 5.09), and the roundings of the one dominant tone add up where those of noise average out."""
    d = rr.corner_case(addon, amplitude, k, partner)
    assert rr.holds(d)
    what = f"{addon} corner signal k={k} A={float(amplitude)} B={d['case'][2]}"
    kk, root = sr.K_SCONV, np.sqrt(2.0 if partner else 1.0)
    taps = 1
    if addon == "sconv":
        y, spec = t_sconv.run_sconv(tf, d["x"], d["h"])
        _expected_within(y, d["expected"]["y"], None, kk, np.abs(d["expected"]["y"]).max() * root, what)
        _bit_for_bit(y, t_sconv.via_conv_plan(tf, d["x"], taps, spec), what)
    elif addon == "gsconv":
        y, spec = t_gsconv.run_gsconv(tf, d["x"], d["h"], d["p"], d["g"], d["skip"])
        z_peak = 2.0 * np.abs(d["expected"]["y"]).max() * root              # z = y / g, g = 1/2
        _expected_within(y, d["expected"]["y"], d["g"], kk, z_peak, what)
        z = t_gsconv.via_conv_plan(tf, rr.gr.gated_input(d["x"], d["p"]), taps, spec)
        _bit_for_bit(y, rr.gr.gated_output(z, d["g"]), what)
    elif addon == "bconv_dx":
        dx, spec = t_bconv.run_dgrad(tf, d["gy"], d["h"])
        _expected_within(dx, d["expected"]["dx"], None, kk, np.abs(d["expected"]["dx"]).max() * root, what)
        _bit_for_bit(dx, t_bconv.dx_via_conv_plan(tf, d["gy"], taps, spec), what)
    else:
        dx, dpre, spec = t_gbconv.run_dgrad(tf, d["gy"], d["h"], d["post"], d["x"], d["pre"], d["skip"])
        du_peak = 2.0 * np.abs(d["expected"]["dx"]).max() * root            # du = dx / pre, pre = 1/2
        _expected_within(dx, d["expected"]["dx"], d["pre"], kk, du_peak, what + " dx")
        _expected_within(dpre, d["expected"]["dpre"], d["x"], kk, du_peak, what + " dpre")
        du = t_gbconv.du_via_conv_plan(tf, rr.gb.gated(d["gy"], d["post"]), taps, spec)
        _bit_for_bit(dx, rr.gb.gated(du, d["pre"]), what + " dx")
        _bit_for_bit(dpre, rr.gb.half_product(d["x"], du), what + " dpre")


# --------------------------------------------------------------------------------------------------- c. gates keep subnormals

def _outputs(tf, d):
    addon = d["addon"]
    if addon == "gconv":
        return [t_gconv.run_gconv(tf, d["x"], d["h"], d.get("p"), d.get("g"), None)[0]]
    if addon == "gsconv":
        return [t_gsconv.run_gsconv(tf, d["x"], d["h"], d.get("p"), d.get("g"), None)[0]]
    dx, dpre, _ = t_gbconv.run_dgrad(tf, d["gy"], d["h"], d.get("post"), d.get("x"), d.get("pre"), None)
    return [dx, dpre]


@pytest.mark.parametrize("addon", ["gconv", "gsconv", "gbconv_dx"])
def test_output_gate_of_2_to_minus_14_lands_in_the_subnormal_range(tf, addon):
    """y = g (.) z (dx = pre (.) du, dpre = x (.) du) with the gate times 2^-14: the add-on's own composition yardstick,
    half_product(gate, the shipped plan's output without that gate), bit for bit, needs no tolerance. The outputs are subnormal
    and not zero: a multiply that flushes its operands or its result returns zeros."""
    d = rr.subnormal_gate_data(addon, "out")
    run_checks(tf, d)
    for out in _outputs(tf, d):
        v = np.abs(out.astype(np.float64))
        assert ((v > 0) & (v < 2.0 ** -14)).mean() > 0.9, (addon, float((v == 0).mean()))


@pytest.mark.parametrize("addon", ["gconv", "gsconv", "gbconv_dx", "gbconv_dh"])
def test_input_gate_that_makes_part_of_u_subnormal(tf, addon):
    """one row's input-side gate times 2^-12: that row of u = p (.) x (gz = post (.) gy) is subnormal, its pair partner is not. The
    gated plan equals the ungated shipped plan on the host-built half_product bit for bit (the add-on's own yardstick), for the tap
    gradient TfftLongConvGradPlan.tap_grad on both products."""
    d = rr.subnormal_gate_data(addon, "in")
    run_checks(tf, d)
