"""How sensitive tests/elementwise_bound.py is (CPU only): synthetic outputs of the library's quality, built from exact fp64 spectra
(rounded to binary16, then +-1 ulp of noise per element), pass the per-element check; each fault a kernel could plausibly make
fails it at 2^12, 2^20 and 2^24 bins. The rel-L2 criterion the GPU tests used alone before lets a single wrong bin through."""
import numpy as np
import pytest

import elementwise_bound as eb

ROWS = 256          # a column pass's tile geometry: bins viewed as [256 rows][n / 256 columns], 16-column tiles


def _spectra(n, batch, seed):
    """fp64 spectra with the statistics of DFT(x)/n for x uniform(-1, 1) (the GPU cases' input): complex Gaussian bins of
    variance 2 / (3 n), and the DC bin of such an input."""
    rng = np.random.default_rng(seed)
    s = np.sqrt(1.0 / (3.0 * n))
    re, im = rng.normal(0.0, s, (batch, n)), rng.normal(0.0, s, (batch, n))
    return re, im


def _as_output(re, im, seed):
    """What a kernel of the library's quality returns: round to binary16, then move each element by -1, 0 or +1 binary16 ulp."""
    rng = np.random.default_rng(seed + 1)
    out = []
    for p in (re, im):
        h = p.astype(np.float16)
        step = rng.integers(-1, 2, p.shape)
        h = np.where(step > 0, np.nextafter(h, np.float16(np.inf)), np.where(step < 0, np.nextafter(h, np.float16(-np.inf)), h))
        out.append(h.astype(np.float64))
    return out


def _fails(got_re, got_im, re, im):
    with pytest.raises(AssertionError, match=r"fault: transform \d+"):
        eb.check(got_re, got_im, re, im, eb.K_TABLE, what="fault")


def _typical_bin(re, im, t, rng, neighbour=False):
    """a bin of transform t of median magnitude (or whose difference to the next bin is of median size): neither one a fault could
    hide in nor the easiest to catch"""
    mag = np.hypot(re[t], im[t]) if not neighbour else np.hypot(np.diff(re[t]), np.diff(im[t]))
    cand = rng.integers(0, re.shape[1] - 1, 64)
    return int(cand[np.argsort(mag[cand])[32]])


def _old_rel_l2(re, im, faults):
    """rel-L2 over all transforms of the binary16-rounded spectra with single-bin faults (t, k, source bin or None = negate)"""
    g_re, g_im = re.astype(np.float16).astype(np.float64), im.astype(np.float16).astype(np.float64)
    for t, k, src in faults:
        g_re[t, k], g_im[t, k] = (g_re[t, src], g_im[t, src]) if src is not None else (-g_re[t, k], -g_im[t, k])
    return np.sqrt(((g_re - re) ** 2 + (g_im - im) ** 2).sum() / (re ** 2 + im ** 2).sum())


SIZES = [1 << 12, 1 << 20, 1 << 24]


@pytest.fixture(scope="module", params=SIZES, ids=lambda n: f"n2^{n.bit_length() - 1}")
def case(request):
    n = request.param
    batch = 2 if n <= 1 << 20 else 1           # (2^24: one transform; its neighbour's tile is drawn on its own)
    re, im = _spectra(n, batch, n)
    got_re, got_im = _as_output(re, im, n)
    return n, re, im, got_re, got_im


def test_clean_outputs_pass(case):
    n, re, im, got_re, got_im = case
    worst = eb.check(got_re, got_im, re, im, eb.K_TABLE, what="clean")
    assert 0.5 <= worst <= 1.5 + 1e-9, worst     # half an ulp of rounding plus one of noise, in ulps of the largest bin at most


def test_one_bin_replaced_by_its_neighbour(case):
    n, re, im, got_re, got_im = case
    t = re.shape[0] - 1
    k = _typical_bin(re, im, t, np.random.default_rng(n + 2), neighbour=True)
    g_re, g_im = got_re.copy(), got_im.copy()
    g_re[t, k], g_im[t, k] = g_re[t, k + 1], g_im[t, k + 1]
    _fails(g_re, g_im, re, im)
    if n >= 1 << 20:
        # the old criterion, rel-L2 of the whole output <= 1.5e-3, lets the same fault in an output rounded once (the library's
        # rel-L2 is 3e-4 to 6e-4) through
        assert _old_rel_l2(re, im, [(t, k, k + 1)]) <= 1.5e-3


def test_one_bin_negated(case):
    n, re, im, got_re, got_im = case
    k = _typical_bin(re, im, 0, np.random.default_rng(n + 3))
    g_re, g_im = got_re.copy(), got_im.copy()
    g_re[0, k], g_im[0, k] = -g_re[0, k], -g_im[0, k]
    _fails(g_re, g_im, re, im)
    if n >= 1 << 24:
        assert _old_rel_l2(re, im, [(0, k, None)]) <= 1.5e-3


def test_one_tile_from_the_next_transform(case):
    n, re, im, got_re, got_im = case
    cols = n // ROWS
    c0 = 16 * int(np.random.default_rng(n + 4).integers(0, max(1, cols // 16)))
    g_re, g_im = got_re.copy(), got_im.copy()
    v_re, v_im = g_re[0].reshape(ROWS, cols), g_im[0].reshape(ROWS, cols)
    if re.shape[0] > 1:
        src_re, src_im = g_re[1].reshape(ROWS, cols)[:, c0:c0 + 16], g_im[1].reshape(ROWS, cols)[:, c0:c0 + 16]
    else:
        o_re, o_im = _spectra(ROWS * 16, 1, n + 5)
        src_re, src_im = o_re.reshape(ROWS, 16) / np.sqrt(n / (ROWS * 16)), o_im.reshape(ROWS, 16) / np.sqrt(n / (ROWS * 16))
    v_re[:, c0:c0 + 16], v_im[:, c0:c0 + 16] = src_re, src_im
    _fails(g_re, g_im, re, im)


def test_twiddle_error_on_one_tile(case):
    """a twiddle 2^-9 off in phase on the 256-row tile that holds the transform's largest bin: that tile's outputs come out rotated
    by 2^-9 rad (a relative error of 2^-9, two to four ulps of the largest bin there)"""
    n, re, im, got_re, got_im = case
    cols = n // ROWS
    k_max = int(np.argmax(np.maximum(np.abs(re[0]), np.abs(im[0]))))
    c0 = (k_max % cols) // 16 * 16
    g_re, g_im = got_re.copy(), got_im.copy()
    v_re, v_im = g_re[0].reshape(ROWS, cols), g_im[0].reshape(ROWS, cols)
    z = (re[0] + 1j * im[0]).reshape(ROWS, cols)[:, c0:c0 + 16] * np.exp(1j * 2.0 ** -9)
    v_re[:, c0:c0 + 16] = z.real.astype(np.float16).astype(np.float64)
    v_im[:, c0:c0 + 16] = z.imag.astype(np.float16).astype(np.float64)
    _fails(g_re, g_im, re, im)


def test_missing_factor_two_on_one_column(case):
    n, re, im, got_re, got_im = case
    cols = n // ROWS
    c = int(np.random.default_rng(n + 6).integers(0, cols))
    g_re, g_im = got_re.copy(), got_im.copy()
    g_re[0].reshape(ROWS, cols)[:, c] *= 0.5
    g_im[0].reshape(ROWS, cols)[:, c] *= 0.5
    _fails(g_re, g_im, re, im)


def test_real_plans_are_bounded_by_the_pair():
    """K_REAL's unit: the ulp of the larger of the two largest bins of a signal pair, so a quiet signal beside a loud one is
    judged in the loud one's ulps (the pair shares one complex transform)."""
    re, im = _spectra(4096, 2, 7)
    re[1] *= 2.0 ** -6
    im[1] *= 2.0 ** -6
    got_re, got_im = re.copy(), im.copy()
    got_re[1, 5] += 2 * eb.ulp16(np.hypot(re[0], im[0]).max())
    with pytest.raises(AssertionError):
        eb.check(got_re, got_im, re, im, eb.K_REAL, what="alone")
    assert eb.check(got_re, got_im, re, im, eb.K_REAL, rel_l2=1.0, pairs=True, what="pair") == pytest.approx(2.0, rel=0.5)


def test_sparse_spectrum_raises_no_false_alarm():
    """A few tones: most 16-column tiles hold nothing but rounding noise. Judged against the average tile's energy, they pass; a
    wrong tone still fails."""
    n = 1 << 16
    re, im = np.zeros((1, n)), np.zeros((1, n))
    for k, a in ((3, 0.25), (n // 2 - 1, 0.125), (n // 3, 0.0625), (40000, 0.03)):
        re[0, k], im[0, k] = a, -a / 3
    re += np.random.default_rng(9).normal(0.0, 1e-6, re.shape)       # the input's own quantisation noise in every bin
    got_re, got_im = _as_output(re, im, 9)
    eb.check(got_re, got_im, re, im, eb.K_TABLE, what="sparse")
    got_re[0, 40000] *= 1.0 + 2.0 ** -6
    _fails(got_re, got_im, re, im)
