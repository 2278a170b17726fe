"""Per-element accuracy bound against an fp64 reference (test infrastructure, importable like accuracy_protocol.py).

A rel-L2 bound cannot see one wrong bin at large N: a wholly wrong bin among 2^20 moves rel-L2 by about 1/1024. This checks
every element instead. For each transform t:

    max_k max(|dRe[k]|, |dIm[k]|) <= K * u(max_k |X_t[k]|),   u(v) = 2^(floor(log2 v) - 10)

u is the binary16 ulp of the largest output bin, the unit of profiles/r2_ulp_distances.txt. A rel-L2 bound is kept as well, per
transform and, from 8192 bins on, per 16-column tile of the [256][bins / 256] view (a column pass's unit of work in natural-order
1D output): a relative error of 2^-9 on one tile, a wrong twiddle, is 2 to 4 ulps of the largest bin at most and can hide under K
(for the single-pass kernels N = 256 .. 4096 tests/test_gpu_basis_sweep.py closes that: every basis vector against the stage arithmetic).
A tile is judged against its own energy or the average tile's, whichever is larger, so a near-empty tile of a sparse spectrum
raises no false alarm. K is set per arithmetic class from profiles/per_kernel_ulps.txt (tools/accuracy_per_kernel.py: the worst error of every
kernel instantiation over tests/test_gpu_kernel_matrix.py's cases and three seeds; K = the smallest half-integer >= 1.5 x the
worst measured value of the class, at most 4):

    K_TABLE    twiddles from the library's tables (every kernel not named below)
    K_SINCOS   twiddles from hardware v_sin / v_cos (collat256_kernel, colfft256_kernel<.., .., .., false> of COL_WAVE_SINCOS)
    K_REAL     real-input plans (R2C / C2R), bounded against the largest bin of the signal PAIR that shares one complex transform
               (include/tfft.h); the scale modes none and once use the class's K relative to their own output

The distributed plans (tfft_dist_*, tests/test_gpu_dist_elementwise.py) have their own profile, profiles/dist_ulps.txt
(tools/accuracy_dist.py: per case, world and rank over three seeds), and the same rule:

    K_PRE      the send buffer after tfft_dist_exec_pre (one column kernel with the four-step twiddle, one rounding), each column in
               ulps of its own largest bin
    K_DIST     the output after tfft_dist_exec_post with table twiddles, in ulps of the largest bin of the whole spectrum (peak=);
               plans with a hardware sin / cos kernel among their row passes stay under K_SINCOS
"""
import numpy as np

# profiles/per_kernel_ulps.txt, "class worst" lines: table 1.84 ulp (colfft1024_wg_kernel<1, 0, ..> behind a radix-512 pass),
# sin / cos 1.64, real 2.75 (the C2R of N = 4096: the merged spectrum is binary16, and the inverse transform spreads its rounding
# over every sample of a signal whose peak is only about twice its rms. Measured, last line of the profile: the same spectrum
# merged in fp64, rounded once and run through the complex inverse has the same error. 1.5 x 2.75 would exceed the ceiling of
# 4, so K_REAL is the ceiling)
K_TABLE = 3.0
K_SINCOS = 2.5
K_REAL = 4.0
# profiles/dist_ulps.txt, "class worst" lines: send buffer 1.572 ulp (2^27 over 4 ranks; 1.07 at 2^15 to 1.57 at 2^27, growing with
# the length, not with the rank: 16 ranks of 2^26 lie between 1.24 and 1.49 without order). Output: sin / cos 0.912, at most the
# kernel matrix's 1.64, so K_SINCOS holds; table 1.996, above the kernel matrix's 1.84, so the distributed plans get a constant
# of their own by the same rule instead of a wider K_TABLE. The 1.996 is 2^28 over 4 ranks, checked on sampled rows in ulps of
# THEIR largest bin, a unit that may be one binade below the whole spectrum's; every length up to 2^27 stays at or below 1.48.
K_PRE = 2.5
K_DIST = 3.0
REL_L2 = 1.5e-3          # what the rel-L2-only tests assert today, now per transform and per tile
TILE_ROWS, TILE_COLS = 256, 16     # a column pass's unit of work: 16 columns of the [256][bins / 256] view of a transform


def ulp16(v):
    """binary16 ulp of magnitude v (> 0): 2^(floor(log2 v) - 10); the subnormal spacing 2^-24 at the bottom."""
    v = np.asarray(v, dtype=np.float64)
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def _as2d(a):
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(1, -1) if a.ndim == 1 else a.reshape(a.shape[0], -1)


def errors_in_ulps(got_re, got_im, ref_re, ref_im, pairs=False, peak=None):
    """Per transform: (worst error in ulps, bin of it, |delta| in ulps of every bin). Arrays: [transforms][bins] (or one transform).
    pairs: the unit of transforms 2p and 2p + 1 is the ulp of the larger of their largest bins (real-input plans).
    peak: the magnitude whose ulp is the unit, one per transform or a scalar, in place of the largest bin of each `ref` row: rows
    that are parts of one longer transform (a rank's [K][N2] share of a distributed N-point spectrum) are judged in the ulp of
    the largest bin of the whole, the unit the K values were measured in."""
    g_re, g_im, r_re, r_im = _as2d(got_re), _as2d(got_im), _as2d(ref_re), _as2d(ref_im)
    assert g_re.shape == r_re.shape == g_im.shape == r_im.shape, (g_re.shape, r_re.shape)
    if peak is not None:
        assert not pairs, "peak= and pairs= exclude each other"
        peak = np.broadcast_to(np.asarray(peak, dtype=np.float64).reshape(-1), (g_re.shape[0],)) if np.ndim(peak) else np.full(g_re.shape[0], float(peak))
    else:
        peak = np.sqrt(r_re * r_re + r_im * r_im).max(axis=1)
    if pairs:
        p = peak.copy()
        for t in range(0, len(p) - 1, 2):
            p[t] = p[t + 1] = max(peak[t], peak[t + 1])
        peak = p
    u = ulp16(peak)[:, None]
    d = np.maximum(np.abs(g_re - r_re), np.abs(g_im - r_im)) / u
    d[~np.isfinite(g_re) | ~np.isfinite(g_im)] = np.inf
    return d


def check(got_re, got_im, ref_re, ref_im, k, rel_l2=REL_L2, pairs=False, what="", peak=None):
    """Asserts the per-element bound and the per-transform and per-tile rel-L2 bounds; returns the worst error in ulps over all
    transforms. The tiles are 16 columns of the [256][bins / 256] view of a transform: a column pass's unit of work where the
    output is one natural-order 1D transform, only a partition of the bins for other layouts (transposed order, strided axes,
    2D images). A tile's error energy is compared with its own energy or, if larger, the average tile's. peak: see
    errors_in_ulps; the rel-L2 bounds stay relative to each transform's (each tile's) own energy."""
    d = errors_in_ulps(got_re, got_im, ref_re, ref_im, pairs, peak)
    g_re, g_im, r_re, r_im = _as2d(got_re), _as2d(got_im), _as2d(ref_re), _as2d(ref_im)
    worst = 0.0
    if d.shape[0] >= 64 and d.shape[1] < TILE_ROWS * TILE_COLS * 2:
        # many short transforms (the columns of a send buffer): all of them at once where every one passes with room to spare;
        # anything near a bound goes through the loop below, which alone decides and words the failure
        e_all = d.max(axis=1)
        num = np.sqrt(((g_re - r_re) ** 2 + (g_im - r_im) ** 2).sum(axis=1))
        den = np.sqrt((r_re ** 2 + r_im ** 2).sum(axis=1))
        rel = np.where(den > 0, num / np.where(den > 0, den, 1.0), num)
        if bool((e_all <= k).all()) and bool((rel <= rel_l2 * (1 - 1e-9)).all()):
            return float(e_all.max())
    for t in range(d.shape[0]):
        k_bin = int(np.argmax(d[t]))
        e = float(d[t, k_bin])
        if not e <= k:
            over_half = int((d[t] > k / 2).sum())
            raise AssertionError(f"{what}: transform {t}, bin {k_bin}: error {e:.2f} ulp > K = {k}; {over_half} of {d.shape[1]} bins "
                                 f"exceed K/2 ({'a localized fault' if over_half <= 16 else 'a general loss of precision'})")
        num = np.sqrt(((g_re[t] - r_re[t]) ** 2 + (g_im[t] - r_im[t]) ** 2).sum())
        den = np.sqrt((r_re[t] ** 2 + r_im[t] ** 2).sum())
        rel = float(num / den) if den > 0 else float(num)
        assert rel <= rel_l2, f"{what}: transform {t}: rel-L2 {rel:.3e} > {rel_l2:.1e}"
        # ... and per tile: a systematic error of one tile (a wrong twiddle: 2^-9 relative is only 2 to 4 ulps of the largest bin)
        cols = d.shape[1] // TILE_ROWS
        if d.shape[1] % (TILE_ROWS * TILE_COLS) == 0 and cols > TILE_COLS:
            def tiles(a):
                return (a.reshape(TILE_ROWS, cols // TILE_COLS, TILE_COLS) ** 2).sum(axis=(0, 2))
            num_t = tiles(g_re[t] - r_re[t]) + tiles(g_im[t] - r_im[t])
            den_t = tiles(r_re[t]) + tiles(r_im[t])
            # (a tile quieter than the average one is judged against the average: no false alarm on a sparse spectrum)
            rel_t = np.sqrt(num_t / np.maximum(np.maximum(den_t, den_t.mean()), 1e-300))
            j = int(np.argmax(rel_t))
            assert rel_t[j] <= rel_l2, f"{what}: transform {t}, tile of columns {16 * j} .. {16 * j + 15}: rel-L2 {rel_t[j]:.3e} > {rel_l2:.1e}"
        worst = max(worst, e)
    return worst
