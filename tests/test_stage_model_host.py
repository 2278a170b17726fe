"""What the models of the single-pass kernels (tests/stage_model.py) say on their own, on the CPU: the figures that
tests/test_gpu_basis_sweep.py holds the kernels to, and the derivation of its bound.

Unit: u = ulp16(A / N) with A = 1024, the binary16 ulp of the magnitude every output of x = A delta_p has.

The deviation bound (2 u). For an impulse every contraction has one non-zero input, so a kernel can differ from the model only
where its fp32 order of operations puts a value on the other side of a binary16 rounding:

  * N = 4096: stage 1 is A F1, exact (A is a power of two): no rounding at all. Stage 2 forms a two-term sum per component
    inside the MFMA and the product with the fp32 twiddle by one fmaf and one rounded product: r2, the operand of stage 3, may be
    the neighbouring binary16 number in either component. N = 256, 256 R: stage 1 is exact, the twiddle product is rounded
    to r1, the operand of the last MFMA stage, which may move the same way; everything behind it (N = 256 R: stage 2, the
    twiddle w_N^(r kk), the radix-R butterfly) stays in fp32.
  * So ONE binary16 intermediate r = (r_re, r_im) moves by at most one ulp per component, and the value in front of the last
    rounding, c r with the last stage's constant c (and factors of magnitude 1 behind it), moves in each component by at most
        |c_re| ulp(r_re) + |c_im| ulp(r_im) <= 2^-10 (|c_re| |r_re| + |c_im| |r_im|) <= 2^-10 |c| |r|,
    and |c| |r| = (A / N) (1 + O(2^-11)): for 4096, |r2| = A / 256 and |H3| = 1/16. A / N is a power of two, so that is
    1 u (1 + O(2^-11)); test_deviation_bound evaluates the left-hand side over every (p, k).
  * The last rounding adds at most half an ulp of the model's component and half an ulp of the kernel's, and no output component
    reaches 2 A / N, so each is at most u / 2. Both results are binary16 numbers below 2 A / N, their difference is a multiple
    of the finer of their two ulps, and the largest such multiple not above (2 + O(2^-11)) u is 2 u.
  * The differences at the fp32 level themselves (2^-24 relative) are 2^-14 u and change nothing above.
test_deviation_bound also runs the model with r moved to each diagonal neighbour and finds no output more than 2 u away.
"""
import functools

import numpy as np
import pytest

import elementwise_bound as eb
import stage_model as sm

A = 1024.0
POSITIONS = (0, 1, 17, 131, 255)           # and N - 1, N / 2 + 3: every digit of every length non-zero somewhere

# the worst component error of x = A delta_p over every p and k against the exact (A / N) w_N^(p k), in u: the model gives 0.707,
# 0.707, 0.707, 0.725, 1.120 for N = 256 .. 4096, in the RE and in the IM plane
IMPULSE_BOUND = {256: 0.75, 512: 0.75, 1024: 0.75, 2048: 0.75, 4096: 1.25}
# the worst error of x_t = h16(exp(+2 pi i f t / N)) over every f against fp64 of the rounded input, in binary16 ulps of the line
# (elementwise_bound.errors_in_ulps): the model gives 0.317, 0.315, 0.184, 0.187, 0.317; asserted with a tenth of slack
TONE_FIGURE = {256: 0.317, 512: 0.315, 1024: 0.184, 2048: 0.187, 4096: 0.317}
TONE_BOUND = {n: round(1.1 * v + 0.005, 2) for n, v in TONE_FIGURE.items()}


def _positions(n):
    return list(POSITIONS) + [n // 2 + 3, n - 1]


@functools.lru_cache(maxsize=None)
def _sweep(n, a):
    """the sequential sweep of x = a delta_p as float32 planes, computed once and shared by the tests below (never written)"""
    re, im = sm.impulse_sweep(n, a)
    re, im = re.astype(np.float32), im.astype(np.float32)
    re.setflags(write=False), im.setflags(write=False)
    return re, im


@pytest.fixture(scope="module", autouse=True)
def _drop_the_sweeps():
    yield
    _sweep.cache_clear()


def test_table_entries_are_rounded_once():
    """build_tables converts fp64 to binary16 in one step. Rounding through fp32 first (what _c16 does, right for accumulators)
    could land elsewhere at a tie of the second rounding: for these tables it does not, at any scale mode, so the tables of
    tests/test_conv_range_host.py, which were built that way, were the kernels' all along."""
    for mode in sm.MODES:
        for once, twice in zip(sm.tables4096(mode), sm.tables4096(mode, sm._c16)):
            assert np.array_equal(once, twice)
        w16 = sm._cexp(sm._I[:, None] * sm._I[None, :], 16)
        for f in (1.0, 1.0 / 16):
            assert np.array_equal(sm._t16(w16 * f), sm._c16(w16 * f))
    # every non-zero component of a binary16 table is a normal number, in every mode
    for mode in sm.MODES:
        tabs = [sm.tables4096(mode)[i] for i in (0, 1, 3)] + [sm.tables256(mode)[0]] + [t for n in (512, 1024, 2048) for t in sm.tables256r(n, mode)[:2]]
        for t in tabs:
            parts = np.abs(np.concatenate((t.real.ravel(), t.imag.ravel())))
            assert parts[parts > 0].min() >= 2.0 ** -14


def test_the_butterfly_matrices_are_dfts():
    for r in (2, 4, 8):
        idx = np.arange(r)
        assert np.abs(sm.butterfly(r) - np.exp(-2j * np.pi * idx[:, None] * idx[None, :] / r)).max() < 2.0 ** -24


@pytest.mark.parametrize("n", sm.SIZES)
def test_general_model_is_the_transform(n):
    rng = np.random.default_rng(n)
    re, im = rng.uniform(-1, 1, (3, n)).astype(np.float16), rng.uniform(-1, 1, (3, n)).astype(np.float16)
    x = re.astype(np.float64) + 1j * im.astype(np.float64)
    for mode, gain in (("sequential", 1.0), ("once", 1.0), ("none", float(n))):
        scaled = (re * np.float16(16.0 / n), im * np.float16(16.0 / n)) if mode == "none" else (re, im)        # N max |x| <= 65504
        want = np.fft.fft(scaled[0].astype(np.float64) + 1j * scaled[1].astype(np.float64), axis=1) / n * gain
        got = sm.forward(n, *scaled, mode)
        assert eb.errors_in_ulps(got.real, got.imag, want.real, want.imag).max() <= eb.K_TABLE, mode
    got = sm.inverse(n, re, im)
    want = np.fft.ifft(x, axis=1)
    assert eb.errors_in_ulps(got.real, got.imag, want.real, want.imag).max() <= eb.K_TABLE


@pytest.mark.parametrize("n", sm.SIZES)
def test_closed_form_equals_the_general_model(n):
    pos = _positions(n)
    for mode in sm.MODES:
        amp = 8.0 if mode == "none" else A
        for a in (amp, 1j * amp)[:1 if (n == 4096 and mode != "sequential") else 2]:
            x = np.zeros((len(pos), n), complex)
            x[np.arange(len(pos)), pos] = a
            re, im = _sweep(n, a) if mode == "sequential" else sm.impulse_sweep(n, a, mode)
            got = sm.forward(n, x.real, x.imag, mode)
            assert np.array_equal(got.real, re[pos]) and np.array_equal(got.imag, im[pos]), (mode, a)
            if mode == "sequential":
                im, re = _sweep(n, complex(a.imag, a.real))             # impulse_sweep_inverse, from the shared sweeps
                got = sm.inverse(n, x.real, x.imag)
                assert np.array_equal(got.real, re[pos]) and np.array_equal(got.imag, im[pos]), a


@pytest.mark.parametrize("n", sm.SIZES)
def test_impulses_against_the_exact_answer(n):
    u = sm.ulp16(A / n)
    for a in (A, 1j * A):
        for inverse in (False, True):
            re, im = _sweep(n, complex(a.imag, a.real))[::-1] if inverse else _sweep(n, a)
            e_re, e_im = sm.impulse_exact(n, a, inverse)
            worst = max(np.abs(re - e_re).max(), np.abs(im - e_im).max()) / u
            print(f"N = {n}, a = {a}, {'inverse' if inverse else 'forward'}: worst error {worst:.3f} u")
            assert worst <= IMPULSE_BOUND[n], (a, inverse, worst)
            # the plane of p = 0 that the exact answer leaves empty is empty, and so is every component where the exact answer
            # and the last stage's constant are zero
            assert not (im if a == A else re)[0].any()
            assert np.abs(re)[e_re == 0].max() <= u and np.abs(im)[e_im == 0].max() <= u


@pytest.mark.parametrize("n", sm.SIZES)
def test_tones_against_fp64_of_the_rounded_input(n):
    t = np.arange(n)
    ang = 2.0 * np.pi * ((t[:, None] * t[None, :]) % n) / n
    re, im = np.cos(ang).astype(np.float16), np.sin(ang).astype(np.float16)
    want = np.fft.fft(re.astype(np.float64) + 1j * im.astype(np.float64), axis=1) / n
    assert (np.argmax(np.abs(want), axis=1) == t).all()
    got = sm.forward(n, re, im)
    worst = float(eb.errors_in_ulps(got.real, got.imag, want.real, want.imag).max())
    print(f"N = {n}: worst tone error {worst:.3f} ulp of the line")
    assert abs(worst - TONE_FIGURE[n]) < 5e-4 and worst <= TONE_BOUND[n], worst


@pytest.mark.parametrize("n", sm.SIZES)
def test_deviation_bound(n):
    u = sm.ulp16(A / n)
    r, c, t, acc = sm.impulse_operands(n, A)
    if n == 4096:
        assert np.array_equal(sm._c16(acc[0]), acc[0])            # stage 1 is exact: r2 is the only rounding that can move
    if t is not None:
        assert np.abs(np.abs(t) - 1).max() < 2.0 ** -22           # behind the last MFMA stage: factors of magnitude 1
        c = c * t
    ulp_re, ulp_im = eb.ulp16(np.abs(r.real)), eb.ulp16(np.abs(r.imag))
    assert (ulp_re <= 2.0 ** -10 * np.maximum(np.abs(r.real), 2.0 ** -14)).all()
    shift = max((np.abs(c.real) * ulp_re + np.abs(c.imag) * ulp_im).max(), (np.abs(c.real) * ulp_im + np.abs(c.imag) * ulp_re).max())
    size = (np.abs(c) * np.abs(r)).max()
    print(f"N = {n}: one ulp of the last binary16 intermediate moves the value in front of the last rounding by at most {shift / u:.4f} u; "
          f"|c| |r| <= {size / (A / n):.5f} A / N")
    assert shift <= 2.0 ** -10 * size * (1 + 1e-12) and size <= (A / n) * (1 + 2.0 ** -11) ** 4
    assert shift <= u * (1 + 2.0 ** -9)
    re, im = _sweep(n, A)
    assert max(np.abs(re).max(), np.abs(im).max()) < 2 * A / n          # every output component's ulp is at most u
    # ... and the experiment: the intermediate on its diagonal neighbours (both components moved, the worst case of the sum above)
    for d_re in (-1, 1):
        for d_im in (-1, 1):
            n_re, n_im = sm.impulse_sweep(n, A, nudge=(d_re, d_im))
            worst = max(np.abs(n_re.astype(np.float32) - re).max(), np.abs(n_im.astype(np.float32) - im).max()) / u
            assert 0 < worst <= 2.0, (d_re, d_im, worst)


SUBNORMAL_A2 = 2636       # N = 4096, sequential and once: components of the second stage's accumulators in the subnormal range


@pytest.mark.parametrize("n", sm.SIZES)
def test_scale_modes_of_the_impulse_sweep(n):
    """With A = 1024 no non-zero output component of any mode is subnormal, and no binary16 intermediate is, except behind the
    second stage of N = 4096 under sequential scaling and scale once: where the exact component of that intermediate is zero,
    the product of the ROUNDED constants F1 G2 leaves a residue of about 2^-11 x A / 256, and 2636 of the 2 x 2^20 components
    fall below 2^-14 (2.0e-6 at the least: up to five bits lost). Unscaled they are 256 times larger and normal. The outputs of the
    three modes still differ by exact powers of two, component for component: asserted here over all of them. (What is below
    2^-40 is cos(pi / 2) = 6e-17 of the fp64 tables in an fp32 twiddle: it rounds to zero in every mode.)"""
    out = {}
    for mode in sm.MODES:
        re, im, acc = sm.impulse_sweep(n, A, mode, with_accumulators=True)
        out[mode] = (re.astype(np.float32), im.astype(np.float32))
        for plane in out[mode]:
            assert np.abs(plane)[plane != 0].min() >= 2.0 ** -14 and np.isfinite(plane).all()
        for i, arr in enumerate(acc):
            parts = np.abs(np.concatenate((arr.real.ravel(), arr.imag.ravel()))) if np.iscomplexobj(arr) else np.abs(arr.ravel())
            assert parts.max() < 65504
            count = int(((parts > 2.0 ** -40) & (parts < 2.0 ** -14)).sum())
            expect = SUBNORMAL_A2 if (n == 4096 and i == 1 and mode != "none") else 0
            assert count == expect, (mode, i, count)
            if count:
                assert parts[(parts > 2.0 ** -40) & (parts < 2.0 ** -14)].min() > 2.0 ** -19
    for plane in (0, 1):
        assert np.array_equal(out["once"][plane], out["sequential"][plane])
        assert np.array_equal(out["none"][plane], out["sequential"][plane] * n)
    if n >= 512:
        # scale once: the operand of the last stage IS the sequential one (tfft.hip apply_scale_mode keeps the last stage's 1/16)
        assert np.array_equal(sm.impulse_operands(n, A, "once")[0], sm.impulse_operands(n, A, "sequential")[0])


def test_scale_once_with_the_whole_factor_on_the_twiddle():
    """Why the last stage of N = 512 .. 4096 keeps its 1/16 under TFFT_SCALE_ONCE (tfft.hip apply_scale_mode). The fp32 twiddle lies
    in FRONT of the last MFMA stage, whose operand is rounded to binary16. With the whole 1 / N on it that operand is 1/16 of the
    sequential one: at N = 4096, A = 1024, 16356 of its components are subnormal instead of 2636, and 240 output components are
    not the sequential ones any more (232 on the MI355X, whose fp32 order differs from exact sums at a few ties): not "exact
    powers of two apart", and less precise than sequential scaling for small inputs, not more."""
    n = 4096
    r_old = sm.impulse_operands(n, A, sm.ONCE_ON_TWIDDLE)[0]
    r_seq = sm.impulse_operands(n, A, "sequential")[0]
    parts = np.abs(np.concatenate((r_old.real.ravel(), r_old.imag.ravel())))
    assert int(((parts > 0) & (parts < 2.0 ** -14)).sum()) == 16356
    assert np.abs(np.abs(r_old[np.abs(r_seq) > 1]) * 16 / np.abs(r_seq[np.abs(r_seq) > 1]) - 1).max() < 2.0 ** -9
    old, seq = sm.impulse_sweep(n, A, sm.ONCE_ON_TWIDDLE), _sweep(n, A)
    differ = sum(int((o.astype(np.float32) != s).sum()) for o, s in zip(old, seq))
    assert differ == 240
    worst = max(np.abs(o.astype(np.float32) - s).max() for o, s in zip(old, seq)) / sm.ulp16(A / n)
    assert worst <= 0.25                      # a quarter of u at the most: no bound on the error sees it, only a comparison of bits
