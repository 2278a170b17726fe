"""What the checks of tests/test_gpu_dist_elementwise.py catch and the per-rank rel-L2 bound before them did not (CPU only), and the
fp64 references of tests/dist_emulate.py against a full fp64 FFT.

Synthetic outputs of the library's quality (exact fp64 values rounded to binary16, then +-1 ulp of noise per element, as in
tests/test_elementwise_bound_host.py) laid out as one rank's [K][N2] share of a 2^26-point spectrum pass; each fault fails. Two of
the faults are shown to pass "rel-L2 of the rank's share <= 1.5e-3" on the same data. The send-buffer faults are shown to
vanish in the row transforms' output, which is why the send buffer is checked on its own."""
import numpy as np
import pytest

import dist_emulate as de
import elementwise_bound as eb
from test_elementwise_bound_host import _as_output, _spectra

N = 1 << 26
N1, N2 = 256, 1 << 18


def _share(world, seed):
    """one rank's share of a 2^26-point spectrum of uniform(-1, 1) input, [K][N2], and an output of the library's quality"""
    k = N1 // world
    re, im = _spectra(N, 1, seed)
    re, im = (p[0, :k * N2] * 1.0 for p in (re, im))        # any K N2 bins of the spectrum have its statistics
    re, im = re.reshape(k, N2), im.reshape(k, N2)
    got_re, got_im = _as_output(re, im, seed)
    return re, im, got_re, got_im


@pytest.fixture(scope="module", params=[8, 2], ids=lambda w: f"2^26-over-{w}")
def share(request):
    return (request.param,) + _share(request.param, 100 + request.param)


def _check(got_re, got_im, re, im, **kw):
    want = re + 1j * im
    return de.check_output(got_re, got_im, want, float(np.abs(want).max()), eb.K_DIST, "fault", **kw)


def _old_rel_l2(got_re, got_im, re, im):
    return float(np.sqrt(((got_re - re) ** 2 + (got_im - im) ** 2).sum() / (re ** 2 + im ** 2).sum()))


def test_clean_share_passes(share):
    world, re, im, got_re, got_im = share
    worst, rel = _check(got_re, got_im, re, im)
    assert 0.5 <= worst <= 1.5 + 1e-9 and rel < 1.5e-3, (worst, rel)


def test_one_bin_replaced_by_its_neighbour(share):
    world, re, im, got_re, got_im = share
    rng = np.random.default_rng(world)
    row = int(rng.integers(0, re.shape[0]))
    cand = rng.integers(0, N2 - 1, 64)
    step = np.hypot(np.diff(re[row]), np.diff(im[row]))
    k = int(cand[np.argsort(step[cand])[32]])                # a pair of neighbours whose difference is of median size
    g_re, g_im = got_re.copy(), got_im.copy()
    g_re[row, k], g_im[row, k] = g_re[row, k + 1], g_im[row, k + 1]
    with pytest.raises(AssertionError, match=rf"transform {row}, bin {k}"):
        _check(g_re, g_im, re, im)
    assert _old_rel_l2(g_re, g_im, re, im) <= 1.5e-3            # what the distributed tests asserted alone


def test_sixteen_wrong_input_samples_of_one_row():
    """128 rows per rank (2^26 over 2 ranks). 16 of the 2^18 input samples of one row transform come from somewhere else (a piece
    of a segment read at a wrong offset): that row's output is off by rel-L2 1e-2, the rank's share by 1.2e-3."""
    world = 2
    re, im, _, _ = _share(world, 7)
    # (an output rounded once, rel-L2 8e-4: the library's own is 3e-4 to 6e-4, as in test_elementwise_bound_host._old_rel_l2)
    got_re, got_im = re.astype(np.float16).astype(np.float64), im.astype(np.float16).astype(np.float64)
    rng = np.random.default_rng(8)
    row = 77
    # the row transform's input S[k1][:] has variance N2 * var(X) per sample; a wrong sample is an independent one of that
    # distribution, so it is off by the difference of two
    s = np.sqrt(N2 / (3.0 * N))
    cols = rng.choice(N2, 16, replace=False)
    delta = (rng.normal(0, s, 16) + 1j * rng.normal(0, s, 16)) - (rng.normal(0, s, 16) + 1j * rng.normal(0, s, 16))
    k2 = np.arange(N2, dtype=np.int64)
    err = sum(d * np.exp((-2j * np.pi / N2) * ((c * k2) % N2)) for c, d in zip(cols, delta)) / N2
    g_re, g_im = got_re.copy(), got_im.copy()
    g_re[row] = (re[row] + err.real).astype(np.float16).astype(np.float64)
    g_im[row] = (im[row] + err.imag).astype(np.float16).astype(np.float64)
    old = _old_rel_l2(g_re, g_im, re, im)
    row_rel = _old_rel_l2(g_re[row], g_im[row], re[row], im[row])
    print(f"rel-L2 of the rank's share {old:.3e}, of the row {row_rel:.3e}")
    assert old <= 1.5e-3 < row_rel
    with pytest.raises(AssertionError, match=rf"transform {row}: rel-L2"):         # the per-row rel-L2 alone ...
        de.check_output(g_re, g_im, re + 1j * im, float(np.hypot(re, im).max()), 1e9, "fault")
    with pytest.raises(AssertionError, match=rf"transform {row}, bin \d+: error"):  # ... and the per-element bound alone
        eb.check(g_re, g_im, re, im, eb.K_DIST, rel_l2=1.0, peak=float(np.hypot(re, im).max()), what="fault")


def _signal(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, n).astype(np.float16), rng.uniform(-1, 1, n).astype(np.float16)


def _h(z):
    """binary16 rounding of a complex fp64 array, as planes of float64"""
    return z.real.astype(np.float16).astype(np.float64), z.imag.astype(np.float16).astype(np.float64)


def test_two_peers_chunks_swapped_in_the_receive_buffer():
    n, world, q = 1 << 20, 4, 1
    x = _signal(n, 11)
    g = de.make_geometry(n, 256, world)
    exact = np.fft.fft(x[0].astype(np.float64) + 1j * x[1].astype(np.float64)) / n
    sends = [de.send_reference(x, g, r) for r in range(world)]
    want = de.rank_rows(exact, g, q)
    peak = float(np.abs(exact).max())
    recv = de.receive_layout(sends, g, q)
    out = np.fft.fft(de.rows_from_receive(recv, g), axis=1) / g.n2
    worst, _ = de.check_output(*_h(out), want, peak, eb.K_DIST, "clean")
    assert worst <= 0.5 + 1e-9
    recv = recv.reshape(world, g.chunk)[[0, 1, 3, 2]].reshape(-1)          # the chunks of peers 2 and 3 in each other's slot
    out = np.fft.fft(de.rows_from_receive(recv, g), axis=1) / g.n2
    with pytest.raises(AssertionError, match="output after post: transform 0"):
        de.check_output(*_h(out), want, peak, eb.K_DIST, "swapped")


def test_send_buffer_check_sees_what_the_row_transforms_dilute():
    """2^24 over 8 ranks: rank 5's column pass applies a four-step twiddle that is 2^-9 rad off on one 128-column block."""
    n, world, rank = 1 << 24, 8, 5
    x = _signal(n, 12)
    g = de.make_geometry(n, 256, world)
    ref = de.send_reference(x, g, rank)
    clean = de.check_send(*_h(ref), ref, g, eb.K_PRE, "clean")
    assert 0.4 <= clean <= 0.5 + 1e-9, clean                    # one rounding: half an ulp of a column's largest bin at most
    y = de.send_columns(ref, g).copy()
    c0 = 1024
    y[:, c0:c0 + 128] *= np.exp(1j * 2.0 ** -9)
    bad = de.send_layout(y, g)
    with pytest.raises(AssertionError, match=rf"send buffer after pre: transform {c0}: rel-L2 1.9\d\de-03"):
        de.check_send(*_h(bad), ref, g, eb.K_PRE, "rotated")
    # the same fault after the row transforms: each row holds 128 wrong samples of 2^16, rotated by 2^-9 rad
    rows = [0, 100, 255]
    cols = slice(rank * g.cols + c0, rank * g.cols + c0 + 128)
    s_rows = np.zeros((len(rows), g.n2), dtype=np.complex128)
    s_rows[:, cols] = de.send_columns(ref, g)[rows, c0:c0 + 128]
    err = np.fft.fft(s_rows * (np.exp(1j * 2.0 ** -9) - 1), axis=1) / g.n2
    want = de.spectrum_rows(x, g, rows)
    rel = np.sqrt((np.abs(err) ** 2).sum(axis=1) / (np.abs(want) ** 2).sum(axis=1))
    print("rel-L2 of the fault in the output rows:", rel)
    assert (rel < 1e-4).all(), rel                           # binary16 rounding noise is 3e-4: no check of the output can see it


def test_send_buffer_in_the_wrong_slab_layout():
    n, world, rank = 1 << 24, 8, 2
    x = _signal(n, 13)
    g = de.make_geometry(n, 256, world, slabs=2)
    ref = de.send_reference(x, g, rank)
    assert de.check_send(*_h(ref), ref, g, eb.K_PRE, "clean") <= 0.5 + 1e-9
    flat = de.send_layout(de.send_columns(ref, g), g, slabs=1)       # [q][k][c] where [q][s][k][c_s] is expected
    assert not np.array_equal(flat, ref)
    with pytest.raises(AssertionError, match="send buffer after pre: transform"):
        de.check_send(*_h(flat), ref, g, eb.K_PRE, "flat")


@pytest.mark.parametrize("lg,n1,worlds", [(16, 256, (1, 2, 4)), (18, 256, (1, 2, 4, 8, 16)), (18, 512, (1, 2, 4, 8)), (15, 256, (1, 2))])
@pytest.mark.parametrize("slabs", [1, 2])
def test_references_against_a_full_fp64_fft(lg, n1, worlds, slabs):
    """send_reference -> exchange -> N2-point transforms, and spectrum_rows, against numpy.fft.fft(x) / N"""
    n = 1 << lg
    x = _signal(n, lg)
    exact = np.fft.fft(x[0].astype(np.float64) + 1j * x[1].astype(np.float64)) / n
    for world in worlds:
        g = de.make_geometry(n, n1, world, slabs)
        if (g.cols // slabs) % 32:
            continue
        sends = [de.send_reference(x, g, r) for r in range(world)]
        for q in range(world):
            out = np.fft.fft(de.rows_from_receive(de.receive_layout(sends, g, q), g), axis=1) / g.n2
            assert np.abs(out - de.rank_rows(exact, g, q)).max() < 1e-16
            rows = sorted({0, g.rows - 1, g.rows // 2})
            got = de.spectrum_rows(x, g, [q * g.rows + k for k in rows])
            assert np.abs(got - de.rank_rows(exact, g, q, rows)).max() < 1e-16
        # and as complex input
        z = x[0].astype(np.float64) + 1j * x[1].astype(np.float64)
        assert np.array_equal(de.send_reference(z, g, world - 1), sends[world - 1])


def test_peak_none_is_the_old_check():
    """peak=None: errors_in_ulps / check as before; peak = each transform's own largest bin: the same numbers"""
    re, im = _spectra(4096, 3, 5)
    got_re, got_im = _as_output(re, im, 5)
    d0 = eb.errors_in_ulps(got_re, got_im, re, im)
    d1 = eb.errors_in_ulps(got_re, got_im, re, im, peak=np.hypot(re, im).max(axis=1))
    assert np.array_equal(d0, d1)
    assert eb.check(got_re, got_im, re, im, eb.K_TABLE) == eb.check(got_re, got_im, re, im, eb.K_TABLE, peak=np.hypot(re, im).max(axis=1)) == d0.max()
    # a scalar unit four times as large: a quarter of the ulps
    big = 4 * np.hypot(re, im).max()
    assert eb.errors_in_ulps(got_re, got_im, re, im, peak=big).max() <= d0.max() / 2
