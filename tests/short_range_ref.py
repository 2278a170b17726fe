"""Test infrastructure of the range contract of the three short-frame add-ons that came after tests/stft_range_ref.py: the short
ISTFT (include/tfft_istftn.h), the masked short ISTFT (tfft_mistftn.h), the spectrogram plans (tfft_spec.h) and the two gradients
built on them (tensor-fft_amd/stft_autograd.py), at n = 512, 1024 and 2048. Host only; shared by tests/test_short_range_host.py (which
checks every input on the CPU) and tests/test_gpu_short_range.py. The generic pieces (times, _largest, _largest16, subnormal, flush,
rel_l2, as_complex, MARGIN, the forward sets) are stft_range_ref's.

A data set is a dict: "kind" ("inverse" or "masked"), "corner", "n", "rows", "length", "hop", "pad", the binary16 arrays "x" [R, L]
(where the spectra come from a signal), "w" [n] (the plan's window), "re", "im" [R F][n / 2 + 1] the plan is fed, for a masked set
"mask" ([R F][n / 2 + 1] per frame, [n / 2 + 1] per bin) and "mode", and "raw_only" where the plan is a raw-sum plan (the adjoints).
Builders are deterministic (seed = 1) and cached; every scale is a power of two found by search, the largest that keeps holds(d).

contract(d) is stft_range_ref.contract's inverse side with n in place of 4096: {name: (value, limit)},

  input   max_k |Z'[k]|, Z' = istftn_ref.merge_items (mistftn_ref.merge_items_masked) of the spectra, <= 64512
  frames  the largest time-domain sample of any frame in fp64 (of the fp64-masked spectra), <= 65504
  y, raw  the largest divided output and the largest raw sum in fp64, <= 65504 (raw alone for a raw-sum plan)
  data    the largest |re|, |im|, |w|, |mask|, <= 65504

The sets, at each n:

  short ISTFT   spectra-high (3, 2n, n / 4, n / 2) Hann, spectra16 of x 2^e; tone-edge-k0 (k0 = 0, 1, n / 32), R = 1, L = 2n, hop = n,
                w = 1, the largest binary16 amplitude that holds; window-high / window-low (2, 2n, n / 2, n / 2), unit spectra, the
                plan's window Hann 2^15 / uniform(0.5, 1) 2^-8; spectra-subnormal / output-subnormal, x 2^-10 / x 2^-14
  masked ISTFT  per frame and per bin on (3, 2n, n / 4, n / 2) Hann (27 frames: the last one self-paired). Every mask is
                2^k uniform(0.5, 1) rounded to binary16 with a random sign on a quarter of the entries, so both frames of a pair
                keep like magnitude. mask-rescues: spectra of x 2^15, whose UNMASKED merge overflows, under the largest k that
                holds (-4 .. -6). mask-lifts: spectra of x 2^-10 under the largest k that holds: 15 or 16, where the mask itself
                ends at 65504; the headroom of the input condition lies beyond that. mask-subnormal: every mask entry a non-zero
                subnormal, 2^-15 uniform(0.5, 1), on the unit spectra times the largest power of two that holds (2^20, 2^21: the
                spectra themselves end at 65504). mask-uneven (per frame only): frame 2b under 2^6, frame 2b + 1 under 2^-6, unit
                spectra; held to bits only.
                pure=True drops the uniform factor (the mask is +-2^k) and puts the spectra on the grid on which the product with
                the mask is a binary16 number ("pre_re", "pre_im": the planes multiplied in fp64 and rounded once, exactly).
  spectrograms  stft_range_ref.forward(corner, n) as they are; band_sets(n) adds "signed": desc37's geometry, weights uniform(-1, 1)
  gradients     grad-high / grad-low: (g_re, g_im) = uniform(-1, 1) 2^e on (2, 2n, n / 2, n / 2) Hann as a per-bin raw-sum set with
                the adjoint mask c; power_case(n, ...): the inputs of differentiable_power_spectrogram and its CPU model

A window times 2^k: num scales by 2^k and den by 2^2k, exactly in fp32, so y = fp16(2^-k q_unit) (scaled_window_output)."""
import numpy as np

import istftn_ref as inr
import mistftn_ref as mr
import rfft_ref
import spec_ref as spr
import stage_model as sm
import stft_range_ref as sr
import stftn_ref as sn

M, LIMIT, MARGIN = sr.M, sr.LIMIT, sr.MARGIN
LENGTHS = inr.LENGTHS
# the constants of the GPU suites that tests/test_gpu_short_range.py asserts (it checks that they are the suites' own)
K_C2R, K_FWD = sr.K_C2R, sr.K_FWD      # tests/test_gpu_istftn.py
K_MASK = 2.0 ** -10                    # tests/test_gpu_mistftn.py: the rounding of a mask entry M / s

UPPER_INVERSE = ("spectra-high", "tone-edge-a", "tone-edge-b", "tone-edge-c")      # the tones k0 = 0, 1, n / 32
WINDOW_INVERSE = sr.WINDOW_INVERSE
LOWER_INVERSE = sr.LOWER_INVERSE
WINDOW_EXPONENT = sr.WINDOW_EXPONENT
MASK_SETS = ("mask-rescues", "mask-lifts", "mask-subnormal", "mask-uneven")
MASK_FP64 = MASK_SETS[:3]
MODES = ("frame", "bin")
MASK_SHAPE = lambda n: (3, 2 * n, n // 4, n // 2)        # noqa: E731  (the first of istftn_ref.accuracy_shapes(n))
LOWER_SHAPE = lambda n: (2, 2 * n, n // 2, n // 2)       # noqa: E731  ("centred" of tests/test_gpu_mistftn.py's GRAD_SHAPES)
SPEC_UPPER, SPEC_LOWER = sr.UPPER_FORWARD, sr.LOWER_FORWARD
BAND_SETS = ("all", "edges", "signed")
POWER_EXPONENTS = (-30, -8, 6)
DOMINANT = 2.0 ** 20

# the fault each lower-edge and mask set is there to see (faulty() restates it in numpy)
FAULTS = {"spectra-subnormal": ("spectra",), "output-subnormal": ("spectra", "frames", "output"), "window-high": ("output",),
          "mask-rescues": ("rounded-gain",), "mask-lifts": ("spectra",), "mask-subnormal": ("mask",), "mask-uneven": ("mask-swapped",),
          "grad-low": ("spectra", "frames", "output")}


def tone_k0(corner, n):
    return {"a": 0, "b": 1, "c": n // 32}[corner.split("-")[2]]


def mask_params():
    return [(c, n, mode) for n in LENGTHS for c in MASK_SETS for mode in MODES if not (c == "mask-uneven" and mode == "bin")]


def geo(d):
    return d["n"], d["rows"], d["length"], d["hop"], d["pad"]


def _f64(a):
    return np.asarray(a, np.float16).astype(np.float64)


# ---- the merges, the contract

def merged(d, re=None, im=None, mask=None):
    """Z' (zr, zi) binary16 [ceil(G / 2)][n]: the merge the set's plan performs, of the set's arrays or of the ones given"""
    re, im = d["re"] if re is None else re, d["im"] if im is None else im
    mask = d.get("mask") if mask is None else mask
    with np.errstate(over="ignore", invalid="ignore"):
        return inr.merge_items(re, im, d["n"]) if mask is None else mr.merge_items_masked(re, im, mask, d["n"])


def spectra64(d):
    """the (masked) half spectra in fp64, complex [G][n / 2 + 1]"""
    k = sn.bins(d["n"])
    if d.get("mask") is None:
        return sr.as_complex(d["re"][:, :k], d["im"][:, :k])
    m_re, m_im = mr.masked64(d["re"], d["im"], d["mask"], d["n"])
    return m_re + 1j * m_im


def frames64(d):
    return np.fft.irfft(spectra64(d), n=d["n"], axis=-1) * d["n"]


def reference(d, raw=False):
    """the fp64 (masked) ISTFT of the set's binary16 arrays, [R][L]: istftn_ref.istft64 / mistftn_ref.istft64_masked"""
    return inr.ola(frames64(d), _f64(d["w"]), *geo(d), raw=raw)


def contract(d):
    zr, zi = merged(d)
    with np.errstate(invalid="ignore"):
        c = {"input": (float(np.abs(sr.as_complex(zr, zi)).max()), M), "frames": (float(np.abs(frames64(d)).max()), LIMIT)}
    if not d.get("raw_only"):
        c["y"] = (float(np.abs(reference(d)).max()), LIMIT)
    c["raw"] = (float(np.abs(reference(d, raw=True)).max()), LIMIT)
    c["data"] = (float(max(np.abs(_f64(d[k])).max() for k in ("re", "im", "w", "mask") if d.get(k) is not None)), LIMIT)
    return c


def holds(d):
    return all(v <= limit for v, limit in contract(d).values())


def binding(d, names=None):
    c = contract(d)
    name = max((k for k in c if names is None or k in names), key=lambda k: c[k][0] / c[k][1])
    return name, c[name][0] / c[name][1]


def finite(d):
    return all(np.isfinite(d[k]).all() for k in ("x", "w", "re", "im", "mask") if d.get(k) is not None)


def _ok(d):
    return finite(d) and holds(d)


# ---- the CPU prediction of the GPU result

def model_frames(d, re=None, im=None, mask=None, z=None):
    """the workspace frames [R F][n] binary16: the merge, stage_model.inverse, one rounding per plane"""
    zr, zi = merged(d, re, im, mask) if z is None else z
    with np.errstate(invalid="ignore", over="ignore"):
        v = sm.inverse(d["n"], zr, zi)
    return sr._interleave(v.real, v.imag, d["re"].shape[0])


def ola(d, v, raw=False, w=None):
    return inr.ola(v, d["w"] if w is None else w, *geo(d), raw=raw)


def model(d, raw=False, **kw):
    """(frames, y) of the set by the model"""
    v = model_frames(d, **kw)
    return v, ola(d, v, raw)


def rounded_gain_merge(d):
    """the merge of an implementation that rounds n A to binary16 BEFORE the mask: Z' = fp16(fp32(mA fp16(n A.re) - ...))"""
    n, k = d["n"], sn.bins(d["n"])
    a, b = rfft_ref.pair_rows(d["re"].shape[0])
    with np.errstate(over="ignore", invalid="ignore"):
        pre_re = (np.float32(n) * d["re"][:, :k].astype(np.float32)).astype(np.float16)
        pre_im = (np.float32(n) * d["im"][:, :k].astype(np.float32)).astype(np.float16)
        mask = d["mask"]
        ma, mb = (np.broadcast_to(mask[None, :k], (a.size, k)),) * 2 if mask.ndim == 1 else (mask[a, :k], mask[b, :k])
        zr, zi = mr._sums(ma, mb, pre_re[a], pre_im[a], pre_re[b], pre_im[b], n, np.float32)
        return zr.astype(np.float16), zi.astype(np.float16)


def faulty(d, fault, raw=False):
    """model(d) with one fault in place: "spectra" (the loads of the spectra flush), "mask" (the loads of the mask flush), "frames"
    (the overlap-add's loads of the workspace flush), "output" (the conversion of y flushes), "rounded-gain" (n A rounded to binary16
    in front of the mask), "mask-swapped" (frame 2b read under the mask of frame 2b + 1 and the reverse)"""
    if fault == "spectra":
        return model(d, raw, re=sr.flush(d["re"]), im=sr.flush(d["im"]))
    if fault == "mask":
        return model(d, raw, mask=sr.flush(d["mask"]))
    if fault == "rounded-gain":
        return model(d, raw, z=rounded_gain_merge(d))
    if fault == "mask-swapped":
        swapped = d["mask"].copy()
        pairs = swapped.shape[0] // 2
        swapped[0:2 * pairs:2], swapped[1:2 * pairs:2] = d["mask"][1:2 * pairs:2], d["mask"][0:2 * pairs:2]
        return model(d, raw, mask=swapped)
    v, y = model(d, raw)
    if fault == "frames":
        return v, ola(d, sr.flush(v), raw)
    if fault == "output":
        return v, sr.flush(y)
    raise ValueError(fault)


def quotient32(d, v, w):
    """the fp32 quotient num / den of istftn_ref.ola on binary16 frames, NOT rounded to binary16"""
    assert v.dtype == np.float16 and w.dtype == np.float16
    return inr.ola(v.astype(np.float32), w.astype(np.float32), *geo(d))


def scaled_window_output(v, d):
    """what a plan whose window is w_unit 2^k returns on the frames v: fp16(2^-k q_unit); the factor is exact in fp32 (asserted)"""
    q = quotient32(d, v, d["w_unit"])
    out = q * np.float32(2.0 ** -d["k"])
    assert np.array_equal(out.astype(np.float64), q.astype(np.float64) * 2.0 ** -d["k"])
    with np.errstate(over="ignore"):
        return out.astype(np.float16)


def unit_window(d):
    return dict(d, w=d["w_unit"], corner=d["corner"] + "-unit", k=0)


def accuracy_bound(w_unit, n, length, hop, pad):
    """the formula of tests/test_gpu_istftn.py::_accuracy_bound for any window: K_C2R sqrt(2 env_max / env_min) + 2^-11"""
    env = inr.envelope(w_unit, n, length, hop, pad)
    assert env.min() > 0
    return K_C2R * np.sqrt(2 * env.max() / env.min()) + 2.0 ** -11


def grad_bound(w, n, length, hop, pad):
    """the formula of tests/test_gpu_mistftn.py::_grad_bound"""
    return K_C2R * np.sqrt(2 * inr.envelope(w, n, length, hop, pad).max()) + 2.0 ** -11


# ---- the data sets

def _set(kind, corner, n, rows, length, hop, pad, re, im, w, **more):
    d = {"kind": kind, "corner": corner, "n": n, "rows": rows, "length": length, "hop": hop, "pad": pad, "re": re, "im": im,
         "w": np.ascontiguousarray(w, np.float16)}
    d.update(more)
    assert re.shape == im.shape == (rows * inr.geometry(n, length, hop, pad), sn.bins(n)) and d["w"].shape == (n,)
    return d


def _from_signal(corner, n, rows, length, hop, pad, x, w_forward, w=None, **more):
    """spectra16 of x under w_forward; the plan's window is w (w_forward unless given)"""
    re, im = inr.spectra16(x, w_forward, hop, pad)
    return _set("inverse", corner, n, rows, length, hop, pad, re, im, w_forward if w is None else w, x=np.ascontiguousarray(x, np.float16), **more)


def _make_inverse(corner, n, seed):
    if corner == "spectra-high":
        rows, length, hop, pad = MASK_SHAPE(n)
        x, w = sn.case_data(n, rows, length, seed)
        make = lambda e: _from_signal(corner, n, rows, length, hop, pad, sr.times(x, e), w, exponent=e)      # noqa: E731
        return make(sr._largest(make, ok=_ok))
    if corner.startswith("tone-edge-"):
        k0 = tone_k0(corner, n)
        ones = np.ones(n, np.float16)
        make = lambda c: _from_signal(corner, n, 1, 2 * n, n, 0, sr.tone(c, k0, 2 * n, n), ones, amplitude=float(c), k0=k0)      # noqa: E731
        return make(sr._largest16(make, ok=_ok))
    rows, length, hop, pad = LOWER_SHAPE(n)
    x, w = sn.case_data(n, rows, length, seed)
    if corner in WINDOW_INVERSE:
        k = WINDOW_EXPONENT[corner]
        if corner == "window-low":
            w = np.random.default_rng([n, seed, 8]).uniform(0.5, 1, n).astype(np.float16)
        scaled = sr.times(w, k)
        assert np.array_equal(scaled.astype(np.float64), w.astype(np.float64) * 2.0 ** k)         # exact downwards too
        return _from_signal(corner, n, rows, length, hop, pad, x, w, scaled, w_unit=w, k=k)
    if corner in LOWER_INVERSE:
        return _from_signal(corner, n, rows, length, hop, pad, sr.times(x, {"spectra-subnormal": -10, "output-subnormal": -14}[corner]), w)
    raise ValueError(corner)


def _below_normal(a):
    """a with every magnitude of 2^-14 and above replaced by the largest subnormal, signs kept"""
    return np.copysign(np.minimum(np.abs(a), np.float16(2.0 ** -14 - 2.0 ** -24)), a)


def _on_grid(a, k):
    """binary16 a moved onto the grid on which a 2^k is a binary16 number: multiples of 2^(-24 - k) (k < 0; values of 2^(-14 - k) and
    above lie on it already)"""
    if not (np.isfinite(a).all() and np.isfinite(k).all()):
        return a                                                           # (a step of the search beyond binary16: refused by finite())
    q = 2.0 ** (-24 - np.minimum(k, 0.0))
    out = (np.round(_f64(a) / q) * q).astype(np.float16)
    assert np.array_equal(out.astype(np.float64), np.round(_f64(a) / q) * q)
    return out


def _make_masked(corner, n, mode, pure, seed):
    rows, length, hop, pad = MASK_SHAPE(n)
    total, bins = rows * inr.geometry(n, length, hop, pad), sn.bins(n)
    assert total % 2 == 1                                                  # a self-paired last frame
    x, w = sn.case_data(n, rows, length, seed)
    shape = (bins,) if mode == "bin" else (total, bins)
    rng = np.random.default_rng([n, seed, MASK_SETS.index(corner), MODES.index(mode)])
    base = (1.0 if pure else rng.uniform(0.5, 1, shape)) * np.where(rng.random(shape) < 0.25, -1.0, 1.0)

    def mask(k):
        """base 2^k in binary16; k a number or an array that broadcasts against the mask"""
        with np.errstate(over="ignore"):
            return (base * 2.0 ** np.asarray(k, np.float64)).astype(np.float16)

    def make(e, k, up=0):
        """spectra16 of x 2^e, times 2^up (exact), under the mask of exponent k"""
        re, im = (sr.times(a, up) for a in inr.spectra16(sr.times(x, e), w, hop, pad))
        if pure:
            re, im = _on_grid(re, k), _on_grid(im, k)
        return _set("masked", corner, n, rows, length, hop, pad, re, im, w, x=sr.times(x, e), mask=mask(k), mode=mode, exponent=e + up, k=k, pure=pure)

    if corner in ("mask-rescues", "mask-lifts"):
        e = 15 if corner == "mask-rescues" else -10
        d = make(e, sr._largest(lambda k: make(e, k), ok=_ok))
        d["remake"] = lambda k: make(e, k)                                 # the same set under another mask exponent
    elif corner == "mask-subnormal":
        sub = lambda up: dict(make(0, -15, up), mask=_below_normal(mask(-15)))      # noqa: E731
        d = sub(sr._largest(sub, ok=_ok))
    elif corner == "mask-uneven":
        assert mode == "frame"
        d = make(0, np.where(np.arange(total) % 2 == 0, 6.0, -6.0)[:, None])
    else:
        raise ValueError(corner)
    if pure:
        m64 = _f64(d["mask"])
        with np.errstate(over="ignore"):
            d["pre_re"], d["pre_im"] = (m64 * _f64(d["re"])).astype(np.float16), (m64 * _f64(d["im"])).astype(np.float16)
        d["exact"] = bool(np.array_equal(d["pre_re"].astype(np.float64), m64 * _f64(d["re"])) and np.array_equal(d["pre_im"].astype(np.float64), m64 * _f64(d["im"])))
    return d


ADJOINT_MASK = lambda n: np.where(np.isin(np.arange(sn.bins(n)), (0, n // 2)), 1.0 / n, 1.0 / (2 * n)).astype(np.float16)      # noqa: E731


def _make_grad(corner, n, seed):
    rows, length, hop, pad = LOWER_SHAPE(n)
    total, bins = rows * inr.geometry(n, length, hop, pad), sn.bins(n)
    w = sn.hann(n)
    rng = np.random.default_rng([n, seed, 41])
    g_re, g_im = (rng.uniform(-1, 1, (total, bins)).astype(np.float16) for _ in range(2))
    c = ADJOINT_MASK(n)
    assert np.array_equal(c.astype(np.float64), np.where(np.isin(np.arange(bins), (0, n // 2)), 1.0 / n, 1.0 / (2 * n)))
    make = lambda e: _set("masked", corner, n, rows, length, hop, pad, sr.times(g_re, e), sr.times(g_im, e), w, mask=c, mode="bin",      # noqa: E731
                          raw_only=True, exponent=e)
    if corner == "grad-high":
        return make(sr._largest(make, ok=_ok))
    d = make(-14)                                                          # (0.99995 2^-14 rounds to 2^-14, a normal number)
    d["re"], d["im"] = _below_normal(d["re"]), _below_normal(d["im"])
    return d


_cache = {}


def _cached(key, build):
    if key not in _cache:
        d = build()
        assert finite(d) and holds(d), (key, contract(d))
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = d
    return _cache[key]


def inverse(corner, n, seed=1):
    """the short-ISTFT data set `corner` at frame length n, built once; it meets the contract (asserted)"""
    return _cached(("inverse", corner, n, seed), lambda: _make_inverse(corner, n, seed))


def masked(corner, n, mode, pure=False, seed=1):
    return _cached(("masked", corner, n, mode, pure, seed), lambda: _make_masked(corner, n, mode, pure, seed))


def grad(corner, n, seed=1):
    return _cached(("grad", corner, n, seed), lambda: _make_grad(corner, n, seed))


# ---- spectrograms

def band_sets(n):
    """"all" and "edges" of spec_ref.band_sets(n), and "signed": the 37 overlapping bands of desc37 with weights uniform(-1, 1), whose
    sums cancel: a fused multiply-add shows in their bits"""
    sets = spr.band_sets(n)
    rng = np.random.default_rng([n, 23])
    return {"all": sets["all"], "edges": sets["edges"], "signed": [(s, rng.uniform(-1, 1, len(w)).astype(np.float32)) for s, w in sets["desc37"]]}


def gains(n):
    return {"one": 1.0, "n2": float(n) ** 2}


def p64(d, gain):
    """gain |rfft(u) / n|^2 in fp64 on the binary16 products of the forward set: [G, bins]"""
    z = sr.reference(d)
    return float(gain) * (z.real ** 2 + z.imag ** 2)


def band_energies_fused(p, bands):
    """spec_ref.band_energies with every step contracted into a fused multiply-add (the product unrounded): what the header excludes"""
    out = np.empty((p.shape[0], len(bands)), np.float32)
    for j, (start, w) in enumerate(bands):
        acc = w[0] * p[:, start]
        for i in range(1, len(w)):
            acc = (acc.astype(np.float64) + np.float64(w[i]) * p[:, start + i].astype(np.float64)).astype(np.float32)
        out[:, j] = acc
    return out


def smallest_step(p, bands):
    """the smallest non-zero magnitude among the gained powers, the products w[i] P and the partial sums of the band restatement"""
    small = [np.abs(p[p != 0]).min()]
    for start, w in bands:
        acc = w[0] * p[:, start]
        for i in range(len(w)):
            prod = w[i] * p[:, start + i]
            acc = prod if i == 0 else acc + prod
            small += [np.abs(a[a != 0]).min() for a in (prod, acc) if (a != 0).any()]
    return float(min(small))


# ---- the gradients of the power spectrogram

def power_weight(n, gain):
    """PowerSpectrogram.backward's fp32 weight: gain / n, and 2 gain / n on bins 0 and n / 2"""
    weight = np.full(sn.bins(n), np.float32(gain / n), np.float32)
    weight[0] = weight[n // 2] = np.float32(2.0 * gain / n)
    return weight


def power_case(n, gain=1.0, k=0, dominant=False, seed=1):
    """the inputs of differentiable_power_spectrogram on the centred shape: x, w, gP (float32 [R, F, bins], uniform(-1, 1) 2^k; with
    `dominant`, entry (0, 1, n / 8) is 2^20), the gain, and the forward set of (x, w)"""
    key = ("power", n, gain, k, dominant, seed)
    if key not in _cache:
        rows, length, hop, pad = LOWER_SHAPE(n)
        x, w = sn.case_data(n, rows, length, seed)
        frames, bins = inr.geometry(n, length, hop, pad), sn.bins(n)
        g_p = np.random.default_rng([n, seed, 43]).uniform(-1, 1, (rows, frames, bins)).astype(np.float32)
        if dominant:
            g_p[0, 1, n // 8] = DOMINANT
        g_p = g_p * np.float32(2.0 ** k)
        fwd = sr._forward(n, "power-grad", rows, length, hop, pad, x, w)
        assert sr.holds(fwd)
        _cache[key] = {"n": n, "rows": rows, "length": length, "hop": hop, "pad": pad, "x": x, "w": w, "g_p": g_p, "gain": float(gain), "forward": fwd}
    return _cache[key]


def power_grad_model(p):
    """(dx binary16 [R][L], the masked raw-sum set the backward pass runs) by the models: S = stft_range_ref.model_forward, M in fp32,
    s = 2^exp of max |M| = mant 2^exp, fp16(M / s), the masked model, dx = fp16(fp32(y) s)"""
    n = p["n"]
    re, im = sr.model_forward(p["forward"])
    m = p["g_p"].reshape(-1, sn.bins(n)) * power_weight(n, p["gain"])[None, :]
    assert m.dtype == np.float32
    s = np.float32(2.0 ** np.frexp(np.abs(m).max())[1])
    mask = (m / s).astype(np.float16)
    d = _set("masked", "power-grad", n, p["rows"], p["length"], p["hop"], p["pad"], re, im, p["w"], mask=mask, mode="frame", raw_only=True, s=float(s))
    y = model(d, raw=True)[1]
    with np.errstate(over="ignore"):
        return (y.astype(np.float32) * s).astype(np.float16), d


def power_grad64(p):
    """(dx64 [R][L], v64 [R F][n]): P = gain |S|^2 has dP / dS = 2 gain S, so the gradient is the adjoint of G = 2 gain gP S, S the
    fp64 STFT of the unrounded products"""
    n = p["n"]
    s = mr.stft64(p["x"], p["w"], p["hop"], p["pad"])
    g = 2.0 * p["gain"] * p["g_p"].reshape(-1, sn.bins(n)).astype(np.float64) * s
    geometry = (p["rows"], p["length"], p["hop"], p["pad"])
    return mr.adjoint64(g.real, g.imag, p["w"], *geometry), mr.adjoint_frames64(g.real, g.imag, n)


def per_signal(a, rows):
    return np.sqrt((np.asarray(a, np.float64).reshape(rows, -1) ** 2).sum(-1))


def normal16(a):
    """where fp64 values are normal binary16 magnitudes"""
    a = np.abs(np.asarray(a, np.float64))
    return (a >= 2.0 ** -14) & (a <= LIMIT)


def power_exponents(n, gain):
    """the k of POWER_EXPONENTS at which the fp64 gradient predicts that at least half of the samples of dx_0 and dx_0 2^k are both
    normal binary16 numbers: {k: share}"""
    dx64 = power_grad64(power_case(n, gain))[0]
    out = {}
    for k in POWER_EXPONENTS:
        share = float((normal16(dx64) & normal16(dx64 * 2.0 ** k)).mean())
        if share >= 0.5:
            out[k] = share
    return out
