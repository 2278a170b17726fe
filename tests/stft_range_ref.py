"""Test infrastructure of the range contract of the STFT family (include/tfft_stft.h, tfft_stftn.h, tfft_istft.h): the data sets at the
edges of the contract, the contract's quantities in fp64, and the CPU prediction of what the GPU returns (tests/stage_model.py between
the framing, split, merge and overlap-add of stft_ref.py, stftn_ref.py, rfft_ref.py and istft_ref.py). Host only; shared by
tests/test_stft_range_host.py (which checks every input on the CPU), tests/test_gpu_stft_range.py and tools/stft_range_accuracy.py.

A data set is a dict: "kind" ("forward" or "inverse"), "corner" (its name), the geometry "n", "rows", "length", "hop", "pad", the
binary16 arrays "x" [R, L] and "w" [n], for the inverse the half spectra "re", "im" [R F][2049] the plan is fed, and "outside" where
the set is meant to break the contract (one set: the self-paired frame at 65504). Builders are deterministic (seed = 1 by default)
and cached; every scale factor is a power of two found by search, the largest that keeps holds(d).

contract(d) returns {name: (value, limit)}; the contract holds when every value <= its limit:

  forward   pair    max over pairs and samples of |u_2i + i u_2i+1|, u = fp16(w x) in the flat order g, frame G of an odd total
                    being frame G - 1 (the self-paired last frame is its own partner), <= 64512: the TFFT_SCALE_SEQUENTIAL bound
            out     the largest component of DFT(u) / n in fp64, <= 65504
            data    the largest |x|, |w|, <= 65504
  inverse   input   max_k |Z'[k]|, Z' = istft_ref.merge_items of the spectra: |4096 (A[k] + i B[k])| <= 64512
            frames  the largest time-domain sample of any frame (fp64), <= 65504
            y, raw  the largest divided output and the largest raw sum (fp64), <= 65504
            data    the largest |re|, |im|, |w|, <= 65504

The forward sets (n = 512, 1024, 2048, 4096):

  signal-high, window-high, split-high   the first pad-0 accuracy shape of n under Hann with 2^e on x, on w, or shared
  corner-k (k = 1, 16, 256)              R = 2, L = hop = n, w = 1: one pair of range_ref.corner_signals(A_PAIR, k, n), one plane per signal
  corner-self                            R = 1, L = n: ONE self-paired frame, the RE plane of the k = 1 corner signal at A_PAIR; the same at
                                         65504 is the set marked "outside"
  products-subnormal                     R = 2, L = 2 n, hop = n / 2: x uniform(0.5, 1), w = Hann 2^-14: every product is subnormal
  x-subnormal                            the same x times 2^-14, every sample a non-zero subnormal, w = Hann 2^12: u is normal
  mixed-pair                             R = 2, L = n: uniform(-1, 1), signal 1 times 2^-12 (frame 1 subnormal for the most part, frame 0 not)

The inverse sets (n = 4096):

  spectra-high                           (3, 8192, 1024, 2048) Hann: istft_ref.spectra16 of x 2^e
  tone-edge (k0 = 0, 1, 100)             R = 1, L = 8192, hop = 4096, w = 1: x = c cos(2 pi k0 t / 4096), c the largest binary16 that holds
  window-high, window-low                (2, 8192, 2048, 2048): spectra at unit scale, the plan's window Hann 2^15 or uniform(0.5, 1) 2^-8;
                                         "w_unit" is the unscaled window and "k" the exponent
  spectra-subnormal, output-subnormal    (2, 8192, 2048, 2048) Hann, x times 2^-10 and 2^-14

What a window times 2^k does to the ISTFT: num scales by 2^k and den by 2^2k, both exactly in fp32, so the fp32 quotient is 2^-k times
the unit window's quotient, exactly, and y = fp16(2^-k q_unit): the unit-window output in every bit where 2^-k y_unit is a binary16
number, and q_unit's own rounding where it is not (k = 15 puts most of y into the subnormals). scaled_window_output() restates that.
"""
import numpy as np

import istft_ref as ir
import range_ref as rr
import rfft_ref
import stage_model as sm
import stft_ref as st
import stftn_ref as sn

M = rr.M                       # 64512: the input condition of a sequentially scaled transform (tests/test_conv_range_host.py derives it)
LIMIT = rr.LIMIT_Y             # 65504
A_PAIR = rr.A_PAIR             # 45600: the largest amplitude both planes of a pair may have at once
A_FULL = rr.A_FULL
LENGTHS = sn.LENGTHS + (st.N,)
CORNER_K = rr.CORNER_K

# the project's constants that tests/test_gpu_stft_range.py asserts (it checks that they are the GPU suites' own)
K_RFFT = 1.5e-3                # tests/test_gpu_stft.py, test_gpu_stftn.py: per-frame rel-L2 of a half spectrum against fp64
K_C2R = 1.5e-3                 # tests/test_gpu_istft.py: per pair, the C2R arithmetic
K_FWD = 1.5e-3 + 2.0 ** -10    # tests/test_gpu_istft.py: the forward allowance of a round trip
K_PAIR = 2e-3                  # tests/test_gpu_rfft.py::test_mismatched_pair_meets_the_pair_relative_bound: max abs error / the pair's largest bin
MARGIN = 1.5                   # the project's rule for constants: the model alone stays this far inside every asserted bound

UPPER_FORWARD = ("signal-high", "window-high", "split-high") + tuple(f"corner-{k}" for k in CORNER_K) + ("corner-self",)
LOWER_FORWARD = ("products-subnormal", "x-subnormal", "mixed-pair")
TONES = (0, 1, 100)
UPPER_INVERSE = ("spectra-high",) + tuple(f"tone-edge-{k0}" for k0 in TONES)
WINDOW_INVERSE = ("window-high", "window-low")
LOWER_INVERSE = ("spectra-subnormal", "output-subnormal")
WINDOW_EXPONENT = {"window-high": 15, "window-low": -8}
ROUND_TRIP_EXPONENTS = (-14, -12, -10, -8, -4, 0, 4, 8)
ROUND_TRIP_SHAPE = (3, 8192, 1024, 2048)

# the fault each lower-edge set is there to see (faulty() restates it in numpy)
FAULTS = {("forward", "products-subnormal"): ("products",), ("forward", "x-subnormal"): ("inputs",), ("forward", "mixed-pair"): ("products",),
          ("inverse", "spectra-subnormal"): ("spectra",), ("inverse", "output-subnormal"): ("spectra", "frames", "output"),
          ("inverse", "window-high"): ("output",)}


def _f64(a):
    return np.asarray(a, np.float16).astype(np.float64)


def hann(n):
    return st.hann() if n == st.N else sn.hann(n)


def case_data(n, rows, length, seed=1):
    """the uniform(-1, 1) signals and the Hann window of the GPU suites' own cases"""
    return st.case_data(rows, length, seed) if n == st.N else sn.case_data(n, rows, length, seed)


def accuracy_shape(n):
    """(rows, length, hop, pad) of the first pad-0 accuracy shape of the GPU suite of n"""
    return (3, 6144, 1024, 0) if n == st.N else sn.accuracy_shapes(n)[0]


def frames_per_signal(d):
    n, length, hop, pad = d["n"], d["length"], d["hop"], d["pad"]
    return st.geometry(length, hop, pad) if n == st.N else sn.geometry(n, length, hop, pad)


def frames(d, x=None, w=None):
    """u [R F][n] binary16 in the flat order g: stft_ref.frames / stftn_ref.frames of the set (or of other x, w in its geometry)"""
    x, w = d["x"] if x is None else x, d["w"] if w is None else w
    with np.errstate(over="ignore"):
        return st.frames(x, w, d["hop"], d["pad"]) if d["n"] == st.N else sn.frames(x, w, d["hop"], d["pad"])


def subnormal(a):
    """where a binary16 array holds non-zero subnormals"""
    a = np.abs(_f64(a))
    return (a > 0) & (a < 2.0 ** -14)


def flush(a):
    """a with every subnormal replaced by zero: what a load, a multiply or a conversion in a flushing mode makes of it"""
    a = np.asarray(a, np.float16)
    return np.where(subnormal(a), np.float16(0), a)


def rel_l2(got, want):
    """per row over complex or real rows"""
    got, want = np.asarray(got), np.asarray(want)
    return np.sqrt((np.abs(got - want) ** 2).sum(-1) / (np.abs(want) ** 2).sum(-1))


def as_complex(re, im):
    with np.errstate(invalid="ignore"):          # (an inf component: the sets beyond the contract)
        return _f64(re) + 1j * _f64(im)


# ---- the references in fp64

def reference(d):
    """forward: rfft / n of the binary16 products, complex128 [R F][n / 2 + 1]; inverse: istft_ref.istft64 of the spectra, [R][L]"""
    if d["kind"] == "forward":
        return np.fft.rfft(frames(d).astype(np.float64), axis=-1) / d["n"]
    return ir.istft64(d["re"], d["im"], d["w"], d["rows"], d["length"], d["hop"], d["pad"])


def _frames64(d):
    s = as_complex(d["re"][:, :ir.BINS], d["im"][:, :ir.BINS])
    return np.fft.irfft(s, n=ir.N, axis=-1) * ir.N


# ---- the contract

def contract(d):
    if d["kind"] == "forward":
        u = frames(d).astype(np.float64)
        a, b = rfft_ref.pair_rows(u.shape[0])
        ref = reference(d) if np.isfinite(u).all() else np.full(1, np.inf + 0j)
        return {"pair": (float(np.abs(u[a] + 1j * u[b]).max()), M),
                "out": (float(max(np.abs(ref.real).max(), np.abs(ref.imag).max())), LIMIT),
                "data": (float(max(np.abs(_f64(d["x"])).max(), np.abs(_f64(d["w"])).max())), LIMIT)}
    zr, zi = ir.merge_items(d["re"], d["im"])
    geo = (d["rows"], d["length"], d["hop"], d["pad"])
    v = _frames64(d)
    w64 = _f64(d["w"])
    return {"input": (float(np.abs(as_complex(zr, zi)).max()), M),
            "frames": (float(np.abs(v).max()), LIMIT),
            "y": (float(np.abs(ir.ola(v, w64, *geo)).max()), LIMIT),
            "raw": (float(np.abs(ir.ola(v, w64, *geo, raw=True)).max()), LIMIT),
            "data": (float(max(np.abs(_f64(d[k])).max() for k in ("re", "im", "w"))), LIMIT)}


def holds(d):
    return all(v <= limit for v, limit in contract(d).values())


def binding(d, names=None):
    """(name, value / limit) of the quantity nearest its limit (among `names`)"""
    c = contract(d)
    name = max((k for k in c if names is None or k in names), key=lambda k: c[k][0] / c[k][1])
    return name, c[name][0] / c[name][1]


# ---- the CPU prediction of the GPU result

def _interleave(first, second, total):
    out = np.empty((2 * first.shape[0],) + first.shape[1:], np.float16)
    with np.errstate(over="ignore", invalid="ignore"):
        out[0::2], out[1::2] = first, second
    return out[:total]


def model_forward(d, u=None):
    """(re, im) binary16 [R F][n / 2 + 1]: stage_model.forward of every pair of frames, rounded, then rfft_ref.split"""
    u = frames(d) if u is None else u
    total = u.shape[0]
    a, b = rfft_ref.pair_rows(total)
    z = sm.forward(d["n"], u[a], u[b])
    with np.errstate(over="ignore", invalid="ignore"):
        ar, ai, br, bi = rfft_ref.split(z.real.astype(np.float16), z.imag.astype(np.float16))
    return _interleave(ar, br, total), _interleave(ai, bi, total)


def model_frames(d, re=None, im=None):
    """the workspace frames [R F][4096] binary16: istft_ref.merge_items, stage_model.inverse, one rounding per plane"""
    re, im = d["re"] if re is None else re, d["im"] if im is None else im
    zr, zi = ir.merge_items(re, im)
    with np.errstate(invalid="ignore"):
        v = sm.inverse(ir.N, zr, zi)
    return _interleave(v.real, v.imag, re.shape[0])


def model_inverse(d, re=None, im=None, raw=False, window=None):
    """(frames, y): model_frames, then istft_ref.ola with the set's window (or another)"""
    v = model_frames(d, re, im)
    return v, ir.ola(v, d["w"] if window is None else window, d["rows"], d["length"], d["hop"], d["pad"], raw=raw)


def model(d):
    """forward: (re, im); inverse: (frames, y)"""
    return model_forward(d) if d["kind"] == "forward" else model_inverse(d)


def faulty(d, fault):
    """model(d) with one flushing fault in place: "products" (the multiply's result), "inputs" (its operands), "spectra" (the loads or
    the conversion in front of the merge), "frames" (the overlap-add's loads of the workspace), "output" (the conversion of y)"""
    if fault == "products":
        return model_forward(d, flush(frames(d)))
    if fault == "inputs":
        return model_forward(d, frames(d, flush(d["x"]), flush(d["w"])))
    if fault == "spectra":
        return model_inverse(d, flush(d["re"]), flush(d["im"]))
    v, y = model_inverse(d)
    if fault == "frames":
        return v, ir.ola(flush(v), d["w"], d["rows"], d["length"], d["hop"], d["pad"])
    if fault == "output":
        return v, flush(y)
    raise ValueError(fault)


def quotient32(v, w, rows, length, hop, pad):
    """the fp32 quotient num / den of istft_ref.ola on binary16 frames, NOT rounded to binary16 (+0 where den = 0)"""
    assert v.dtype == np.float16 and w.dtype == np.float16
    return ir.ola(v.astype(np.float32), w.astype(np.float32), rows, length, hop, pad)


def scaled_window_output(v, d):
    """what a plan whose window is w_unit 2^k returns on the frames v: fp16(2^-k q_unit), q_unit the fp32 quotient under the unit
    window; the factor is exact in fp32 (asserted: no quotient leaves fp32's normal range)"""
    q = quotient32(v, d["w_unit"], d["rows"], d["length"], d["hop"], d["pad"])
    out = q * np.float32(2.0 ** -d["k"])
    assert np.array_equal(out.astype(np.float64), q.astype(np.float64) * 2.0 ** -d["k"])
    with np.errstate(over="ignore"):
        return out.astype(np.float16)


def istft_bound(w_unit, length, hop, pad):
    """the formula of tests/test_gpu_istft.py::_accuracy_bound for any window: K_C2R sqrt(2 env_max / env_min) + 2^-11"""
    env = ir.envelope(w_unit, length, hop, pad)
    assert env.min() > 0
    return K_C2R * np.sqrt(2 * env.max() / env.min()) + 2.0 ** -11


# ---- scaling by powers of two found by search

def times(a, e):
    """a 2^e rounded to binary16; upwards the scaling must be exact unless it overflows"""
    with np.errstate(over="ignore"):
        out = (_f64(a) * 2.0 ** e).astype(np.float16)
    if e >= 0:
        assert np.isinf(out).any() or np.array_equal(out.astype(np.float64), _f64(a) * 2.0 ** e), e
    return out


def _finite(d):
    return all(np.isfinite(d[k]).all() for k in ("x", "w", "re", "im") if d.get(k) is not None)


def _ok(d):
    return _finite(d) and holds(d)


def _largest(make, start=0, lo=-40, hi=40, ok=None):
    """the largest exponent e in [lo, hi] for which make(e) is finite and meets the contract (the quantities grow with e); `ok` is the
    test of another module's contract (tests/short_range_ref.py)"""
    ok = _ok if ok is None else ok
    e = start
    if ok(make(e)):
        while e < hi and ok(make(e + 1)):
            e += 1
    else:
        while e > lo and not ok(make(e)):
            e -= 1
        assert ok(make(e)), "no exponent meets the contract"
    return e


def _largest16(make, ok=None):
    """the largest positive finite binary16 c for which make(c) meets the contract, by bisection over the bit patterns"""
    ok = _ok if ok is None else ok
    lo, hi = 1, 0x7BFF
    val = lambda b: np.array(b, np.uint16).view(np.float16)[()]      # noqa: E731
    assert ok(make(val(lo))) and not ok(make(val(hi)))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(make(val(mid))) else (lo, mid)
    return val(lo)


# ---- the data sets

def _forward(n, corner, rows, length, hop, pad, x, w, **more):
    d = {"kind": "forward", "corner": corner, "n": n, "rows": rows, "length": length, "hop": hop, "pad": pad,
         "x": np.ascontiguousarray(x, np.float16), "w": np.ascontiguousarray(w, np.float16), "outside": False}
    d.update(more)
    assert d["x"].shape == (rows, length) and d["w"].shape == (n,)
    return d


def _inverse(corner, rows, length, hop, pad, x, w_forward, w=None, **more):
    """spectra16 of x under w_forward; the plan's window is w (w_forward unless given)"""
    re, im = ir.spectra16(x, w_forward, hop, pad)
    d = {"kind": "inverse", "corner": corner, "n": ir.N, "rows": rows, "length": length, "hop": hop, "pad": pad, "x": np.ascontiguousarray(x, np.float16),
         "w": np.ascontiguousarray(w_forward if w is None else w, np.float16), "re": re, "im": im, "outside": False}
    d.update(more)
    return d


def _below(a, top):
    """a with every value above `top` replaced by `top`"""
    return np.minimum(a, np.float16(top))


def _make_forward(corner, n, seed):
    if corner in ("signal-high", "window-high", "split-high"):
        rows, length, hop, pad = accuracy_shape(n)
        x, w = case_data(n, rows, length, seed)
        split = {"signal-high": lambda e: (e, 0), "window-high": lambda e: (0, e), "split-high": lambda e: (-(-e // 2), e // 2)}[corner]
        make = lambda e: _forward(n, corner, rows, length, hop, pad, times(x, split(e)[0]), times(w, split(e)[1]), exponent=e)      # noqa: E731
        return make(_largest(make))
    if corner.startswith("corner-") and not corner.startswith("corner-self"):
        re, im = rr.corner_signals(A_PAIR, int(corner.split("-")[1]), n)
        return _forward(n, corner, 2, n, n, 0, np.stack((re, im)), np.ones(n, np.float16))
    if corner in ("corner-self", "corner-self-outside"):
        amplitude = A_PAIR if corner == "corner-self" else A_FULL
        return _forward(n, corner, 1, n, n, 0, rr.corner_signals(amplitude, 1, n)[0][None], np.ones(n, np.float16), outside=corner != "corner-self")
    rng = np.random.default_rng([n, seed, LOWER_FORWARD.index(corner)])
    if corner in ("products-subnormal", "x-subnormal"):
        x = rng.uniform(0.5, 1, (2, 2 * n)).astype(np.float16)
        if corner == "products-subnormal":
            return _forward(n, corner, 2, 2 * n, n // 2, 0, x, times(hann(n), -14))
        # (0.99995 2^-14 rounds to 2^-14, a normal number: the largest subnormal instead)
        return _forward(n, corner, 2, 2 * n, n // 2, 0, _below(times(x, -14), 2.0 ** -14 - 2.0 ** -24), times(hann(n), 12))
    if corner == "mixed-pair":
        x = rng.uniform(-1, 1, (2, n)).astype(np.float16)
        x[1] = times(x[1], -12)
        return _forward(n, corner, 2, n, n, 0, x, hann(n))
    raise ValueError(corner)


def tone(c, k0, length=2 * ir.N, n=ir.N):
    """c cos(2 pi k0 t / n) rounded to binary16, [1, length]; n = 4096 unless given"""
    return (float(c) * np.cos(2 * np.pi * ((k0 * np.arange(length)) % n) / n)).astype(np.float16)[None]


def _make_inverse(corner, seed):
    if corner == "spectra-high":
        rows, length, hop, pad = ROUND_TRIP_SHAPE
        x, w = st.case_data(rows, length, seed)
        make = lambda e: _inverse(corner, rows, length, hop, pad, times(x, e), w, exponent=e)      # noqa: E731
        return make(_largest(make))
    if corner.startswith("tone-edge-"):
        k0 = int(corner.split("-")[2])
        ones = np.ones(ir.N, np.float16)
        make = lambda c: _inverse(corner, 1, 2 * ir.N, ir.N, 0, tone(c, k0), ones, amplitude=float(c), k0=k0)      # noqa: E731
        return make(_largest16(make))
    rows, length, hop, pad = 2, 8192, 2048, 2048
    x, w = st.case_data(rows, length, seed)
    if corner in WINDOW_INVERSE:
        k = WINDOW_EXPONENT[corner]
        if corner == "window-low":
            w = np.random.default_rng([seed, 8]).uniform(0.5, 1, ir.N).astype(np.float16)
        scaled = times(w, k)
        assert np.array_equal(scaled.astype(np.float64), w.astype(np.float64) * 2.0 ** k)         # exact downwards too
        return _inverse(corner, rows, length, hop, pad, x, w, scaled, w_unit=w, k=k)
    if corner in LOWER_INVERSE:
        return _inverse(corner, rows, length, hop, pad, times(x, {"spectra-subnormal": -10, "output-subnormal": -14}[corner]), w)
    raise ValueError(corner)


_cache = {}


def forward(corner, n, seed=1):
    """the forward data set `corner` at frame length n, built once; everything but the `outside` set meets the contract (asserted)"""
    key = ("forward", corner, n, seed)
    if key not in _cache:
        d = _make_forward(corner, n, seed)
        assert _finite(d) and (holds(d) or d["outside"]), key
        _cache[key] = d
    return _cache[key]


def inverse(corner, seed=1):
    key = ("inverse", corner, seed)
    if key not in _cache:
        d = _make_inverse(corner, seed)
        assert _finite(d) and holds(d), key
        _cache[key] = d
    return _cache[key]


def unit_window(d):
    """the window-high / window-low set with the unscaled window in the plan"""
    out = dict(d)
    out["w"], out["corner"], out["k"] = d["w_unit"], d["corner"] + "-unit", 0
    return out


def forward_params(corners=UPPER_FORWARD + LOWER_FORWARD):
    return [(c, n) for n in LENGTHS for c in corners]


# ---- the round trip

def round_trip(e, seed=1):
    """istft(stft(x 2^e)) by the two models, (3, 8192, 1024, 2048) Hann: {"error": worst signal's rel-L2 against x 2^e, "holds": whether
    both plans' contracts hold, "forward", "inverse": the data sets}"""
    key = ("trip", e, seed)
    if key not in _cache:
        rows, length, hop, pad = ROUND_TRIP_SHAPE
        x, w = st.case_data(rows, length, seed)
        f = _forward(st.N, f"round-trip{e:+d}", rows, length, hop, pad, times(x, e), w)
        re, im = model_forward(f)
        i = dict(f, kind="inverse", re=re, im=im)
        ok = _finite(i) and holds(f) and holds(i)
        y = model_inverse(i)[1]
        _cache[key] = {"error": float(rel_l2(_f64(y), _f64(f["x"])).max()), "holds": ok, "forward": f, "inverse": i}
    return _cache[key]
