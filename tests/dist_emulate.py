"""All ranks of one distributed transform (tfft_dist_*) in one process, phase by phase, with fp64 references for both phases
(test infrastructure, importable like accuracy_protocol.py).

run() creates one plan per rank with comm = None and caller-owned exchange buffers, puts every plane (input, send, receive,
output) between guard zones of sentinel halves, runs tfft_dist_exec_pre on every rank, keeps a copy of the send planes, performs
the exchange by device copies (chunk q of rank p' -> slot p' of rank q), runs tfft_dist_exec_post, and reports per rank what it
saw. Nothing is asserted here except through check_send / check_output, which the tests and tools/accuracy_dist.py share.

Four-step FFT, N = N1 N2, x viewed as [N1][N2], w_M = exp(-2 pi i / M), rank p owns columns [p C, (p + 1) C), C = N2 / P:

    send buffer of rank p   S[k1][c] = (1 / N1) sum_n1 x[n1 N2 + p C + c] w_N1^(n1 k1) * w_N^((k1 (p C + c)) mod N)
                            stored [q][k][c] with k1 = q K + k, K = N1 / P (= [N1][C] row-major), and with S slabs
                            [q][s][k][c_s], column c = s C / S + c_s (include/tfft.h, TFFT_DIST_SLABS_*)
    exchange                rank q's row k = the P segments send_p'[q K + k][:] side by side: S[k1][p' C + c], all N2 columns
    output of rank q        X[k1 + N1 k2] = (1 / N2) sum_col S[k1][col] w_N2^(col k2), k1 = q K + k, stored [K][N2]

send_reference and spectrum_rows restate these two lines in numpy fp64 (the twiddle's exponent is reduced mod N in int64 before
it becomes a float). spectrum_rows gives chosen rows k1 of the output without an N-point fp64 FFT, for lengths whose full
spectrum does not fit the host; tests/test_dist_check_host.py checks both against numpy.fft.fft(x) / N."""
import types

import numpy as np

import elementwise_bound as eb

GUARD = 4096                    # sentinel halves before and after every buffer (8 KiB)
SENTINEL = 0x7E5A               # a binary16 NaN payload no kernel writes
COL_CHUNK = 1 << 14             # columns per step of the host references (256 x 16384 complex128 = 64 MiB)


def _untouched(after, before, what):
    bad = np.nonzero(after != before)[0]
    assert bad.size == 0, f"{what}: {bad.size} halves changed, first at {bad[:4]}"


def geometry(g):
    """tfft_dist_geometry (ctypes or any object with its fields) -> plain ints"""
    return types.SimpleNamespace(n=int(g.n), n1=int(g.n1), n2=int(g.n2), cols=int(g.cols), rows=int(g.rows), chunk=int(g.chunk),
                                 world=int(g.world), rank=int(g.rank), reorder=int(g.reorder), local_passes=int(g.local_passes),
                                 slabs=int(getattr(g, "slabs", 1)))


def make_geometry(n, n1, world, slabs=1, reorder=0):
    """a geometry for the host tests (no library needed)"""
    n2 = n // n1
    return types.SimpleNamespace(n=n, n1=n1, n2=n2, cols=n2 // world, rows=n1 // world, chunk=(n1 // world) * (n2 // world),
                                 world=world, rank=0, reorder=reorder, local_passes=0, slabs=slabs)


# ---------------------------------------------------------------------------------------------------------------------
# fp64 references (numpy only)
# ---------------------------------------------------------------------------------------------------------------------
def _columns(x, g, c0, c1):
    """columns [c0, c1) of the [N1][N2] view of x as complex128 [N1][c1 - c0]; x: complex array of N, or (re, im) of N each"""
    if isinstance(x, tuple):
        re, im = (np.asarray(p).reshape(g.n1, g.n2)[:, c0:c1] for p in x)
        return re.astype(np.float64) + 1j * im.astype(np.float64)
    return np.asarray(x).reshape(g.n1, g.n2)[:, c0:c1].astype(np.complex128)


def _fourstep_twiddle(g, k1s, c0, c1):
    """w_N^((k1 col) mod N) for k1 in k1s, col in [c0, c1): the exponent reduced in int64"""
    e = (np.asarray(k1s, dtype=np.int64)[:, None] * np.arange(c0, c1, dtype=np.int64)[None, :]) % g.n
    return np.exp((-2j * np.pi / g.n) * e)


def send_layout(y, g, slabs=None):
    """Y[k1][c] of one rank ([N1][C]) -> the order of its send plane: [q][k][c], with S slabs [q][s][k][c_s]"""
    s = g.slabs if slabs is None else slabs
    if s == 1:
        return y.reshape(-1)
    return np.ascontiguousarray(y.reshape(g.world, g.rows, s, g.cols // s).transpose(0, 2, 1, 3)).reshape(-1)


def send_columns(plane, g, slabs=None):
    """inverse of send_layout: a send plane (N / P values) -> [N1][C]"""
    s = g.slabs if slabs is None else slabs
    if s == 1:
        return plane.reshape(g.n1, g.cols)
    return np.ascontiguousarray(plane.reshape(g.world, s, g.rows, g.cols // s).transpose(0, 2, 1, 3)).reshape(g.n1, g.cols)


def send_reference(x, g, rank, col0=None):
    """fp64 send buffer of `rank` after tfft_dist_exec_pre, complex128, laid out as the plan's send planes"""
    col0 = rank * g.cols if col0 is None else col0
    y = np.empty((g.n1, g.cols), dtype=np.complex128)
    for c in range(0, g.cols, COL_CHUNK):
        c1 = min(g.cols, c + COL_CHUNK)
        y[:, c:c1] = np.fft.fft(_columns(x, g, col0 + c, col0 + c1), axis=0) / g.n1
        y[:, c:c1] *= _fourstep_twiddle(g, np.arange(g.n1), col0 + c, col0 + c1)
    return send_layout(y, g)


def spectrum_rows(x, g, k1s):
    """rows X[k1 + N1 k2], k2 < N2, of DFT(x) / N for the given k1, complex128 [len(k1s)][N2], without an N-point FFT"""
    k1s = np.asarray(k1s, dtype=np.int64)
    w = np.exp((-2j * np.pi / g.n1) * ((k1s[:, None] * np.arange(g.n1, dtype=np.int64)[None, :]) % g.n1)) / g.n1
    s = np.empty((k1s.size, g.n2), dtype=np.complex128)
    for c in range(0, g.n2, COL_CHUNK):
        c1 = min(g.n2, c + COL_CHUNK)
        s[:, c:c1] = (w @ _columns(x, g, c, c1)) * _fourstep_twiddle(g, k1s, c, c1)
    return np.fft.fft(s, axis=1) / g.n2


def rank_rows(exact, g, rank, rows=None):
    """rank's share of the full spectrum `exact` in its output layout [K][N2] (or the chosen rows k of it)"""
    k = np.arange(g.rows) if rows is None else np.asarray(rows)
    return exact[((rank * g.rows + k)[:, None] + g.n1 * np.arange(g.n2)[None, :])]


def receive_layout(sends, g, q):
    """what rank q's receive plane holds after a correct exchange of the ranks' send planes: slot p' = chunk q of rank p'"""
    return np.concatenate([sends[p][q * g.chunk:(q + 1) * g.chunk] for p in range(g.world)])


def rows_from_receive(recv, g):
    """the input rows of a rank's row transforms, [K][N2], out of its receive plane [p'][s][k][c_s]"""
    s = g.slabs
    return np.ascontiguousarray(recv.reshape(g.world, s, g.rows, g.cols // s).transpose(2, 0, 1, 3)).reshape(g.rows, g.n2)


# ---------------------------------------------------------------------------------------------------------------------
# the checks of one rank (shared by the GPU tests, the host tests and tools/accuracy_dist.py)
# ---------------------------------------------------------------------------------------------------------------------
def k_of(kernels):
    """K of the output by arithmetic class of the kernels of both phases, as tests/test_gpu_kernel_matrix.py classifies them"""
    from test_gpu_kernel_matrix import arithmetic_class

    return {"sincos": eb.K_SINCOS, "table": eb.K_DIST}[arithmetic_class(kernels, {"kind": "c"})]


def check_send(send_re, send_im, ref, g, k, what):
    """Send planes against send_reference: the C columns as transforms of N1 bins (a column is the column kernel's unit of
    work and carries one twiddle column), each in the ulp of its own largest bin. Returns the worst error in ulps."""
    got_re, got_im = (np.ascontiguousarray(send_columns(np.asarray(p), g).T, dtype=np.float64) for p in (send_re, send_im))
    r = np.ascontiguousarray(send_columns(ref, g).T)
    return eb.check(got_re, got_im, r.real, r.imag, k, what=f"{what}: send buffer after pre")


def check_output(out_re, out_im, want, peak, k, what, rows=None):
    """A rank's [K][N2] output (or the chosen rows of it) against fp64 rows: each row transform is a transform for the per-transform
    and per-tile rel-L2 bounds, the per-element unit is the ulp of `peak`, the largest bin of the whole N-point spectrum.
    Returns (worst error in ulps, rel-L2 of everything compared)."""
    k_rows, n2 = want.shape
    g_re, g_im = (np.asarray(p).reshape(-1, n2) for p in (out_re, out_im))
    if rows is not None:
        g_re, g_im = g_re[np.asarray(rows)], g_im[np.asarray(rows)]
    g_re, g_im = g_re.astype(np.float64), g_im.astype(np.float64)
    worst = eb.check(g_re, g_im, want.real, want.imag, k, peak=peak, what=f"{what}: output after post")
    rel = float(np.sqrt(((g_re - want.real) ** 2 + (g_im - want.imag) ** 2).sum() / (want.real ** 2 + want.imag ** 2).sum()))
    return worst, rel


# ---------------------------------------------------------------------------------------------------------------------
# the emulator (needs torch and a GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _guarded(torch, n_halves, fill=None):
    """device buffer of GUARD + n_halves + GUARD sentinel halves, the middle optionally filled from fill (numpy float16)"""
    host = np.full(GUARD + n_halves + GUARD, SENTINEL, dtype=np.int16)
    if fill is not None:
        host[GUARD:GUARD + n_halves] = np.asarray(fill, dtype=np.float16).reshape(-1).view(np.int16)
    return torch.from_numpy(host).cuda().view(torch.float16)


def _guards_intact(torch, buf):
    b = buf.view(torch.int16)
    return bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all())


def _sentinels_left(torch, plane):
    return int((plane.view(torch.int16) == SENTINEL).sum())


def exchange(bufs, world, chunk):
    """the all-to-all by device copies: chunk q of rank p' -> slot p' of rank q (both planes); world 1 has nothing to move"""
    if world == 1:
        return
    for q in range(world):
        for pp in range(world):
            bufs[q][2][pp * chunk:(pp + 1) * chunk].copy_(bufs[pp][0][q * chunk:(q + 1) * chunk])
            bufs[q][3][pp * chunk:(pp + 1) * chunk].copy_(bufs[pp][1][q * chunk:(q + 1) * chunk])


def run(torch, capi, xr, xi, world, slabs=1, keep_send=True):
    """Runs all `world` ranks of the transform of x = xr + i xi (float16, N each). Returns a list with one namespace per rank:
    g (geometry), kernels_pre, kernels_post, send_re / send_im (host float16 copies of the send planes after pre; None without
    keep_send), out_re / out_im (host float16), faults (what the guard zones, the input and the sentinel prefill showed: a list
    of messages that name rank and phase, empty when all is well)."""
    n = xr.size
    loc = n // world
    inside = slice(GUARD, GUARD + loc)
    plans, bufs, raw, ins, res = [], [], [], [], []
    for r in range(world):
        send = [_guarded(torch, loc) for _ in range(2)]
        recv = [_guarded(torch, loc) for _ in range(2)] if world > 1 else send
        b = tuple(t[inside] for t in send + recv)
        p = capi.DistPlan(n, world, r, 0, buffers=b, slabs=slabs)
        plans.append(p)
        bufs.append(b)
        raw.append(send + (recv if world > 1 else []))
        g = geometry(p.geometry)
        assert g.slabs == slabs and g.rank == r, (g.slabs, g.rank)
        res.append(types.SimpleNamespace(g=g, kernels_pre=p.kernels(0), kernels_post=p.kernels(1), faults=[], send_re=None,
                                         send_im=None, out_re=None, out_im=None))
    g = res[0].g
    x2r, x2i = xr.reshape(g.n1, g.n2), xi.reshape(g.n1, g.n2)
    for r, p in enumerate(plans):       # input layout "columns": rank r holds columns [r C, (r + 1) C) of the [N1][N2] view
        host = [np.ascontiguousarray(x2[:, r * g.cols:(r + 1) * g.cols]).reshape(-1) for x2 in (x2r, x2i)]
        dev = [_guarded(torch, loc, h) for h in host]
        ins.append((host, dev))
        p.pre(dev[0][inside], dev[1][inside])
    torch.cuda.synchronize()
    for r in range(world):
        f = res[r].faults
        for name, t in zip(("send RE", "send IM"), raw[r][:2]):
            if not _guards_intact(torch, t):
                f.append(f"rank {r}, pre: guard zones of the {name} plane were written")
            left = _sentinels_left(torch, t[inside])
            if left:
                f.append(f"rank {r}, pre: {left} halves of the {name} plane were never written")
        for name, t in zip(("receive RE", "receive IM"), raw[r][2:]):
            if _sentinels_left(torch, t) != t.numel():
                f.append(f"rank {r}, pre: the {name} plane was written before the exchange")
        if keep_send:
            res[r].send_re, res[r].send_im = (t.cpu().numpy() for t in bufs[r][:2])
    exchange(bufs, world, g.chunk)
    torch.cuda.synchronize()
    for r, p in enumerate(plans):
        out = [_guarded(torch, loc) for _ in range(2)]
        p.post(out[0][inside], out[1][inside])
        torch.cuda.synchronize()
        f = res[r].faults
        for name, t in zip(("output RE", "output IM"), out):
            if not _guards_intact(torch, t):
                f.append(f"rank {r}, post: guard zones of the {name} plane were written")
            left = _sentinels_left(torch, t[inside])
            if left:
                f.append(f"rank {r}, post: {left} halves of the {name} plane were never written")
        for name, t in zip(("send RE", "send IM", "receive RE", "receive IM"), raw[r]):
            if not _guards_intact(torch, t):
                f.append(f"rank {r}, post: guard zones of the {name} plane were written")
        host, dev = ins[r]
        for name, h, t in zip(("input RE", "input IM"), host, dev):
            if not _guards_intact(torch, t):
                f.append(f"rank {r}: guard zones of the {name} plane were written")
            if not np.array_equal(t[inside].cpu().numpy().view(np.int16), h.view(np.int16)):
                f.append(f"rank {r}: the {name} plane was changed (preserve_input)")
        res[r].out_re, res[r].out_im = (t[inside].cpu().numpy() for t in out)
        ins[r] = None
    for p in plans:
        p.close()
    return res
