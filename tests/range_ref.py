"""Test infrastructure of the range contract of the seven convolution add-ons (include/tfft_conv.h, tfft_lconv.h, tfft_gconv.h,
tfft_sconv.h, tfft_gsconv.h, tfft_bconv.h, tfft_gbconv.h): the contract's quantities in fp64, the corners of the contract built from the
amplitude-1 cases of the *_ref.py files, and the adversarial signals of the forward transform's input condition. Host only; shared
by tests/test_conv_range_host.py (which checks every input on the CPU), tests/test_gpu_conv_range.py and tools/range_accuracy.py.

A data set is a dict: "addon", the shape of its case, and the binary16 arrays the add-on's GPU test hands to its plan. The add-ons:

    conv       x_re, x_im [batch][n], h_re, h_im [filters][n] (the filter is a spectrum)            tests/conv_ref.py
    lconv      x [B][C][L], h [C][K]                                                                 tests/lconv_ref.py
    gconv      x, h, p, g (gates, or None), skip (or None)                                           tests/gconv_ref.py
    sconv      x, h                                                                                  tests/sconv_ref.py
    gsconv     x, h, p, g, skip                                                                      tests/gsconv_ref.py
    bconv_dx   gy [B][C][L], h         (the input gradient)                                          tests/bconv_ref.py
    gbconv_dx  x, h, pre, post, skip, gy                                                             tests/gbconv_ref.py
    bconv_dh   x, gy, taps             (the tap gradient)
    gbconv_dh  x, pre, gy, post, taps

contract(data) returns {name: (value, limit)}; the contract holds when every value <= its limit:

    xh     max_k |X_k| |H'_k| over the transformed items (the signal's spectrum, its pair's, or its window's; H' the binary16 spectrum
           of the taps with the skip folded in, or its conjugate), <= 32752; tap gradient: max_k |G_k| |fp16(U_k / 4096)|
    y      the peak of the full circular (conv, windows) or linear (pairs) result, discarded samples included, <= 65504; tap gradient:
           the item's peak / 4096
    gz     gated forward plans: max |g z| <= 65504; gated input gradient: pre_du = max |pre du| and x_du = max |x du|
    input  the NEW quantity: the largest complex magnitude |x_2p + i x_2p+1| of any transformed sample, after the pre gate, over the
           items whose two planes are both in use, <= M. An item with an all-zero plane (a zero partner, a real signal) is exempt: see
           tests/test_conv_range_host.py, where M is derived.
    data   the largest magnitude of any binary16 input, <= 65504 (it has to be a finite binary16 value)

The spectrum is numpy's fp64 FFT of the binary16 taps rounded to binary16: the library's host builders (tfft_lconv_spectrum_host,
tfft_gconv_spectrum_host) restate the same thing and agree with it up to the sign of a zero.
"""
import numpy as np

import bconv_ref as br
import conv_ref
import gbconv_ref as gb
import gconv_ref as gr
import lconv_ref as lr
import sconv_ref as sr

LIMIT_XH = 32752.0
LIMIT_Y = 65504.0
# The input condition of a sequentially scaled forward transform with S rounded stages: M (1 + 2^-11)^(2 S - 1) (1 + 2^-19)^S < 65520
# (derived in tests/test_conv_range_host.py). M = 63 * 2^10 holds up to S = 16; the N = 4096 kernels have S = 3.
M = 64512.0
N = sr.N

FORWARD = ("conv", "lconv", "gconv", "sconv", "gsconv", "bconv_dx", "gbconv_dx")
TAP_GRADS = ("bconv_dh", "gbconv_dh")
GATED = ("gconv", "gsconv", "gbconv_dx")
CORNERS = ("signal-high", "filter-high", "signal-full")
GATE_CORNER = "gates-high"
DH_CORNERS = ("x-high", "gy-high")
# which arrays "the signal" and "the taps" of a corner are
SIGNAL = {"conv": ("x_re", "x_im"), "lconv": ("x",), "gconv": ("x",), "sconv": ("x",), "gsconv": ("x",), "bconv_dx": ("gy",), "gbconv_dx": ("gy",)}
TAPS = {"conv": ("h_re", "h_im"), "lconv": ("h",), "gconv": ("h", "skip"), "sconv": ("h",), "gsconv": ("h", "skip"), "bconv_dx": ("h",),
        "gbconv_dx": ("h", "skip")}
ARRAYS = ("x_re", "x_im", "h_re", "h_im", "x", "h", "p", "g", "skip", "pre", "post", "gy")


# What tests/test_gpu_conv_range.py runs at the upper edge: the smallest shapes at which each kernel can still go wrong (see the
# *_ref.py files for what each shape is there for). conv's filters are spectra: "delays" is its delay kind and "decay", the spectrum
# of decaying noise taps, stands in for the noise kind. lconv and gconv: (L, K, B, C, launch_iters, composed flag).
KINDS = {"conv": ("decay", "delays")}
TAP_KINDS = ("noise", "delay")
_CAUSAL = [(520, 7, 3, 3, 0, False), (2048, 2049, 3, 3, 2, False), (96, 33, 5, 4, 0, True), (4096, 4097, 3, 2, 0, False)]
_LONG = [(6152, 130, 3, 3, 0), (2048, 2049, 3, 3, 2)]
_DH = sorted(br.DH_CASES, key=gb.items_per_channel)[:2]          # the fewest items per channel
UPPER_CASES = {"conv": [(4096, 37, 3, False), (256, 21, 4, True), (1 << 16, 5, 2, True)], "lconv": _CAUSAL, "gconv": _CAUSAL, "sconv": _LONG,
               "gsconv": _LONG, "bconv_dx": _LONG, "gbconv_dx": _LONG, "bconv_dh": _DH, "gbconv_dh": _DH}
UPPER_MODE = {"gconv": "pre+post+skip", "gsconv": "pre+post+skip", "gbconv_dx": "pre+post+skip", "gbconv_dh": "pre+post"}


def constant_of(d):
    """the add-on's own accuracy constant for the data set's path (the tap gradients and the gated input gradient have derived
    tolerances instead)"""
    addon = d["addon"]
    if addon == "conv":
        return conv_ref.K_CONV_COMPOSED if d["case"][3] or d["case"][0] != N else conv_ref.K_CONV_FUSED
    if addon in ("lconv", "gconv"):
        return lr.K_LCONV_COMPOSED if plan_length(d) != N or d["case"][5] else lr.K_LCONV_FUSED
    return sr.K_SCONV


def corners_of(addon):
    if addon in TAP_GRADS:
        return DH_CORNERS
    return CORNERS + ((GATE_CORNER,) if addon in GATED else ())


def floor16(v):
    """the largest binary16 value <= v (v > 0)"""
    h = np.float16(v)
    return h if float(h) <= v else np.nextafter(h, np.float16(0))


A_PAIR = floor16(M / np.sqrt(2.0))          # the largest amplitude both rows of a pair may have at once: 45600
A_FULL = np.float16(65504.0)


# ---- the amplitude-1 cases

def base(addon, case, kind, seed=1, mode="pre+post+skip"):
    """the amplitude-1 data of a case as the add-on's GPU test generates it. case: conv (n, batch, filters, composed); lconv and
    gconv (L, K, B, C, launch_iters, composed); sconv, gsconv and the input gradients (L, K, B, C, launch_iters); tap gradients
    (L, K, B, C, partials cap), always with noise taps' signals (the tap gradient has no taps)."""
    d = {"addon": addon, "case": tuple(case), "kind": kind, "corner": "amplitude-1", "exact_taps": True}
    if addon == "conv":
        n, batch, filters, _ = case
        d["x_re"], d["x_im"], d["h_re"], d["h_im"] = conv_ref.case_data(n, batch, filters, kind, seed)
        return d
    length, taps, rows, channels = case[:4]
    if addon in ("lconv", "sconv"):
        d["x"], d["h"] = lr.case_data(length, taps, rows, channels, kind, seed)
    elif addon in ("gconv", "gsconv"):
        d["x"], d["h"], d["p"], d["g"], d["skip"] = gr.case_data(length, taps, rows, channels, kind, seed, mode)
        d["mode"] = mode
    elif addon == "bconv_dx":
        d["h"] = lr.case_data(length, taps, rows, channels, kind, seed)[1]
        d["gy"] = br.grad_signal(rows, channels, length, taps, seed)
    elif addon == "gbconv_dx":
        d["x"], d["h"], d["pre"], d["post"], d["skip"], d["gy"] = gb.case_data(length, taps, rows, channels, kind, seed, mode)
        d["mode"] = mode
    elif addon == "bconv_dh":
        d["x"] = lr.case_data(length, taps, rows, channels, "noise", seed)[0]
        d["gy"] = br.grad_signal(rows, channels, length, taps, seed)
    elif addon == "gbconv_dh":
        d["x"], _, d["pre"], d["post"], _, d["gy"] = gb.case_data(length, taps, rows, channels, "noise", seed, mode)
        d["mode"] = mode
    else:
        raise ValueError(addon)
    return d


# ---- the contract's quantities

def _f64(a):
    return np.asarray(a, np.float16).astype(np.float64)


def spectrum16(taps64, n):
    """fp16(fft(taps, n)) component by component, as complex128: [C][n]"""
    s = np.fft.fft(np.asarray(taps64, np.float64), n, axis=-1)
    return s.real.astype(np.float16).astype(np.float64) + 1j * s.imag.astype(np.float16).astype(np.float64)


def _input_magnitude(z):
    """the largest magnitude over the items [items][n] with both planes in use; 0 where there is none"""
    both = (z.real != 0).any(axis=1) & (z.imag != 0).any(axis=1)
    return float(np.abs(z[both]).max()) if both.any() else 0.0


def _items(z, spec):
    """(max |X| |H|, the complex results [items][n]) of items z [items][n] against the spectrum of each item"""
    zx = np.fft.fft(z, axis=-1)
    return float((np.abs(zx) * np.abs(spec)).max()), np.fft.ifft(zx * spec, axis=-1)


def plan_length(d):
    """the transform length of the data set's plan"""
    if d["addon"] == "conv":
        return d["case"][0]
    if d["addon"] in ("lconv", "gconv"):
        length, taps = d["case"][:2]
        return lr.plan_length(length, taps, d["case"][5])
    return N


def contract(d, data=None):
    """contract(data), or contract(addon, data) with the add-on named again"""
    if data is not None:
        assert data["addon"] == d, (d, data["addon"])
        d = data
    return _evaluate(d)[0]


def reference(d):
    """(the fp64 result of every transformed item [items][n] with the rounded spectrum, discarded samples included, and each item's
    peak: the unit of the add-on's constant); tap gradients: the items / 4096"""
    y = _evaluate(d)[1]
    return y, np.abs(y).max(axis=1)


def _evaluate(d):
    addon = d["addon"]
    out = {"data": (max(float(np.abs(_f64(d[k])).max()) for k in ARRAYS if d.get(k) is not None), LIMIT_Y)}
    n = plan_length(d)
    if addon == "conv":
        z = _f64(d["x_re"]) + 1j * _f64(d["x_im"])
        spec = _f64(d["h_re"]) + 1j * _f64(d["h_im"])
        xh, y = _items(z, spec[np.arange(z.shape[0]) % spec.shape[0]])
    elif addon in ("lconv", "gconv", "sconv", "gsconv"):
        rows, channels, length = d["x"].shape
        taps = d["h"].shape[1]
        u = gr.gated_input(d["x"], d.get("p"))
        re, im = lr.pair_planes(_f64(u), n) if addon in ("lconv", "gconv") else sr.windows(_f64(u), taps)
        z = re + 1j * im
        spec = spectrum16(gr.taps_with_skip(d["h"], d.get("skip")), n)
        xh, y = _items(z, spec[np.arange(z.shape[0]) % channels])
        if d.get("g") is not None:
            # the kept samples: what the post gate multiplies
            zz = lr.unpair(y.real, y.imag, rows, channels, length) if addon == "gconv" else sr.unwindow(y.real, y.imag, rows, channels, length, taps)
            out["gz"] = (float(np.abs(_f64(d["g"]) * zz).max()), LIMIT_Y)
    elif addon in ("bconv_dx", "gbconv_dx"):
        rows, channels, length = d["gy"].shape
        taps = d["h"].shape[1]
        gz = gb.gated(d["gy"], d.get("post"))
        re, im = br.dx_windows(_f64(gz), taps)
        z = re + 1j * im
        spec = np.conj(spectrum16(gr.taps_with_skip(d["h"], d.get("skip")), N))
        xh, y = _items(z, spec[np.arange(z.shape[0]) % channels])
        if d.get("pre") is not None:
            du = br.dx_unwindow(y.real, y.imag, rows, channels, length, taps)
            out["pre_du"] = (float(np.abs(_f64(d["pre"]) * du).max()), LIMIT_Y)
            out["x_du"] = (float(np.abs(_f64(d["x"]) * du).max()), LIMIT_Y)
    elif addon in TAP_GRADS:
        taps = d["case"][1]
        u, gz = gb.gated(d["x"], d.get("pre")), gb.gated(d["gy"], d.get("post"))
        zu, zg = br.dh_windows(u, gz, taps)
        su = br.half_spectrum(zu)                                       # fp16(U / 4096): the "filter" of the tap gradient
        sg = np.fft.fft(zg, axis=-1)
        xh = float((np.abs(sg) * np.abs(su)).max())
        y = np.fft.ifft(np.conj(su) * sg, axis=-1)                      # the item / 4096
        z = np.concatenate((zu, zg))
    else:
        raise ValueError(addon)
    out["xh"] = (xh, LIMIT_XH)
    out["y"] = (float(np.abs(y).max()), LIMIT_Y)
    out["input"] = (_input_magnitude(z), M)
    return out, y


def holds(d):
    return all(v <= limit for v, limit in contract(d).values())


def binding(d, names=None):
    """(name, value / limit) of the quantity nearest its limit (among `names`)"""
    c = contract(d)
    name = max((k for k in c if names is None or k in names), key=lambda k: c[k][0] / c[k][1])
    return name, c[name][0] / c[name][1]


# ---- the corners

def _times(d, keys, e):
    """a copy of d with the arrays `keys` times 2^e, rounded to binary16; upwards the scaling must be exact"""
    out = dict(d)
    for k in keys:
        if d.get(k) is None:
            continue
        with np.errstate(over="ignore"):
            out[k] = (_f64(d[k]) * 2.0 ** e).astype(np.float16)
        if e >= 0:
            assert np.isinf(out[k]).any() or np.array_equal(out[k].astype(np.float64), _f64(d[k]) * 2.0 ** e), (k, e)
    return out


def _finite(d):
    return all(np.isfinite(d[k]).all() for k in ARRAYS if d.get(k) is not None)


def _largest(make, start=0, lo=-40, hi=40):
    """the largest exponent e in [lo, hi] for which make(e) is finite and meets the contract (the quantities grow with e)"""
    def ok(e):
        d = make(e)
        return _finite(d) and holds(d)

    e = start
    if ok(e):
        while e < hi and ok(e + 1):
            e += 1
    else:
        while e > lo and not ok(e):
            e -= 1
        assert ok(e), "no exponent meets the contract"
    return e


def scaled(d, corner):
    """the data set at a corner of the contract: the exponent is the largest for which every quantity of contract() stays within
    its limit, so the binding quantity lies in (1/2, 1] of its limit (asserted); scalings upwards leave the binary16 data exact
    (asserted)."""
    addon = d["addon"]
    assert corner in corners_of(addon), (addon, corner)
    names = None
    if corner == "signal-high":
        make = lambda e: _times(d, SIGNAL[addon], e)      # noqa: E731
        out = make(_largest(make))
    elif corner == "filter-high":
        make = lambda e: _times(d, TAPS[addon], e)      # noqa: E731
        out = make(_largest(make))
    elif corner == "signal-full":
        full = _times(d, SIGNAL[addon], 15)
        make = lambda e: _times(full, TAPS[addon], e)      # noqa: E731
        b = _largest(make, start=-8)
        assert b < 0, b
        out = make(b)
        # re-rounded: the small values of most taps and spectra are subnormal now and lost bits; a delay's single tap 2^b did not
        out["exact_taps"] = all(np.array_equal(_f64(out[k]), _f64(full[k]) * 2.0 ** b) for k in TAPS[addon] if full.get(k) is not None)
    elif corner == GATE_CORNER:
        # the input-side gate up by 2^10 and what it multiplies down by 2^10 (re-rounded), so that their product keeps its size; every
        # output-side gate up as far as its product allows
        # (binding: the gated product, or the gate itself where the end of binary16 comes first: "data")
        if addon == "gbconv_dx":
            out = _times(_times(d, ("post",), 10), ("gy",), -10)
            for key in ("pre", "x"):
                make = lambda e, o=out, k=key: _times(o, (k,), e)      # noqa: E731
                out = make(_largest(make))
            names = ("pre_du", "x_du", "data")
        else:
            out = _times(_times(d, ("p",), 10), ("x",), -10)
            make = lambda e: _times(out, ("g",), e)      # noqa: E731
            out = make(_largest(make))
            names = ("gz", "data")
    elif corner in DH_CORNERS:
        key = "x" if corner == "x-high" else "gy"
        make = lambda e: _times(d, (key,), e)      # noqa: E731
        out = make(_largest(make))
    else:
        raise ValueError(corner)
    out["corner"] = corner
    assert _finite(out) and holds(out), (addon, corner)
    name, ratio = binding(out, names)
    assert 0.5 < ratio <= 1.0, (addon, corner, name, ratio)
    return out


def upper_edge_params(addons=FORWARD + TAP_GRADS):
    """[(addon, case, kind, corner)]: every case, tap kind and corner of the upper edge"""
    return [(a, c, k, corner) for a in addons for c in UPPER_CASES[a]
            for k in (("noise",) if a in TAP_GRADS else KINDS.get(a, TAP_KINDS)) for corner in corners_of(a)]


_cache = {}


def upper_edge_data(addon, case, kind, corner, seed=1):
    """the data set of one upper-edge test, built (and checked: scaled() asserts the contract) once"""
    key = (addon, tuple(case), kind, corner, seed)
    if key not in _cache:
        _cache[key] = scaled(base(addon, case, kind, seed, UPPER_MODE.get(addon, "")), corner)
    return _cache[key]


# ---- gates that produce binary16 subnormals

GATE_CASES = {"gconv": (520, 7, 3, 3, 0, False), "gsconv": (6152, 130, 3, 3, 0), "gbconv_dx": (6152, 130, 3, 3, 0), "gbconv_dh": (6152, 130, 3, 3, 0)}


def _subnormal(a):
    a = np.abs(_f64(a))
    return (a > 0) & (a < 2.0 ** -14)


def subnormal_gate_data(addon, side, seed=1):
    """noise taps, gates only (no skip, so that the ungated shipped plan is a yardstick too).
    side "out": the gate applied behind the transform (g; pre and x of the input gradient) times 2^-14, rounded: the outputs y, dx
    and dpre land in binary16's subnormal range. side "in": one row's gate in front of the transform (row 1 of p; of post for the
    input gradient; of both for the tap gradient) times 2^-12, rounded: part of u (gz) is subnormal, the other rows are untouched.
    Asserted here: the gates, or the products they form, do hold non-zero subnormals."""
    mode = {"out": {"gconv": "post", "gsconv": "post", "gbconv_dx": "pre"}, "in": {"gconv": "pre", "gsconv": "pre", "gbconv_dx": "post",
                                                                                     "gbconv_dh": "pre+post"}}[side][addon]
    d = base(addon, GATE_CASES[addon], "noise", seed, mode)
    d["corner"] = "subnormal-" + side
    keys = {"out": {"gconv": ("g",), "gsconv": ("g",), "gbconv_dx": ("pre", "x")}, "in": {"gconv": ("p",), "gsconv": ("p",), "gbconv_dx": ("post",),
                                                                                           "gbconv_dh": ("pre", "post")}}[side][addon]
    for k in keys:
        a = _f64(d[k])
        if side == "out":
            a = a * 2.0 ** -14
        else:
            a[1] = a[1] * 2.0 ** -12
        d[k] = a.astype(np.float16)
    if side == "out":
        assert all(_subnormal(d[k]).mean() > 0.9 for k in keys)
    else:
        products = {"gconv": [("p", "x")], "gsconv": [("p", "x")], "gbconv_dx": [("post", "gy")], "gbconv_dh": [("pre", "x"), ("post", "gy")]}[addon]
        for a, b in products:
            u = gr.half_product(d[a], d[b])
            assert _subnormal(u[1]).mean() > 0.5 and not _subnormal(u[0]).mean() > 0.01 and not _subnormal(u[2]).mean() > 0.01, (addon, a, b)
    assert holds(d)
    return d


# ---- the adversarial signals of the forward transform

def corner_signals(amplitude, k, n=N):
    """(re, im) binary16 [n]: x_t = A (sgn cos(2 pi k t / n) + i sgn sin(2 pi k t / n)), the signs taken from the integer phase
    q = k t mod n (cos: + on [0, n/4) and [3n/4, n); sin: + on [0, n/2)), so that no sample is zero. Every sample has the
    magnitude A sqrt 2, and one 1/16-scaled radix-16 stage over samples n / 16 k apart turns it into a component of 1.2568 A."""
    q = (k * np.arange(n)) % n
    re = np.where((4 * q < n) | (4 * q >= 3 * n), 1.0, -1.0)
    im = np.where(2 * q < n, 1.0, -1.0)
    a = float(np.float16(amplitude))
    return (a * re).astype(np.float16), (a * im).astype(np.float16)


CORNER_K = (1, 16, 256)


def corner_gain(n):
    """the delta filter of the corner-signal cases, a power of two: with it max |X H| = (4 / pi) A n gain = 0.318 A at every n, and the
    answer is gain * x exactly"""
    return 2.0 ** -14 * N / n


def corner_conv(amplitude, k, n, composed, partner=True):
    """the conv data set of one corner signal: one signal (IM plane zero without partner), one filter H = corner_gain(n) at every
    bin; "expected": the exact answer gain * x, (re, im) fp64"""
    re, im = corner_signals(amplitude, k, n)
    if not partner:
        im = np.zeros_like(im)
    h = np.full((1, n), corner_gain(n), np.float16)
    assert float(h[0, 0]) == corner_gain(n)
    return {"addon": "conv", "case": (n, 1, 1, composed), "kind": "corner", "corner": f"k={k}", "exact_taps": True,
            "x_re": re[None], "x_im": im[None], "h_re": h, "h_im": np.zeros_like(h),
            "expected": (corner_gain(n) * _f64(re)[None], corner_gain(n) * _f64(im)[None])}


CORNER_CASE = (N, 1, 2, 1, 0)       # L = 4096, K = 1, B = 2, C = 1: halo 0, one full window


def corner_case(addon, amplitude, k, partner=True):
    """the corner signal as the rows 0 and 1 of one channel (B = 2) or as row 0 alone (B = 1: a zero partner) of an overlap-save plan
    at L = 4096, K = 1: one full window without halo. Taps, skip and gates are powers of two, so "expected" ([B][1][L] fp64 per
    output) is exact: sconv y = 2^-14 x; gsconv (pre+post+skip) u = 2 (x / 2), h' = 2^-15 + 2^-15, y = u / 2^15; bconv dx = 2^-14 gy;
    gbconv gz = 2 (gy / 2), du = 2^-14 gz, dx = du / 2, dpre = 4 du."""
    re, im = corner_signals(amplitude, k)
    rows = (np.stack((re, im)) if partner else re[None])[:, None, :]
    shape = rows.shape
    half = (_f64(rows) / 2).astype(np.float16)
    assert np.array_equal(_f64(half) * 2, _f64(rows))
    full = lambda v: np.full(shape, v, np.float16)      # noqa: E731
    tap = lambda v: np.full((1, 1), v, np.float16)      # noqa: E731
    d = {"addon": addon, "case": (N, 1, shape[0], 1, 0), "kind": "corner", "corner": f"k={k}", "exact_taps": True}
    if addon == "sconv":
        d.update(x=rows, h=tap(2.0 ** -14), expected={"y": 2.0 ** -14 * _f64(rows)})
    elif addon == "gsconv":
        d.update(x=half, p=full(2.0), g=full(0.5), h=tap(2.0 ** -15), skip=np.full(1, 2.0 ** -15, np.float16), mode="pre+post+skip",
                 expected={"y": 2.0 ** -15 * _f64(rows)})
    elif addon == "bconv_dx":
        d.update(gy=rows, h=tap(2.0 ** -14), expected={"dx": 2.0 ** -14 * _f64(rows)})
    elif addon == "gbconv_dx":
        d.update(gy=half, post=full(2.0), x=full(4.0), pre=full(0.5), h=tap(2.0 ** -15), skip=np.full(1, 2.0 ** -15, np.float16),
                 mode="pre+post+skip", expected={"dx": 2.0 ** -15 * _f64(rows), "dpre": 2.0 ** -12 * _f64(rows)})
    else:
        raise ValueError(addon)
    return d
