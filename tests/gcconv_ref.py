"""Test infrastructure of the gated carried convolution plans (include/tfft_gcconv.h): the cases and modes that
tests/test_gcconv_host.py and tests/test_gpu_gcconv.py share, the contexts of the gates, the concatenations that turn a carried
execution into a whole-sequence execution of the shipped GATED plans, and the fp64 direct sums of the extended sequences.

No constant of its own: shapes are tests/cconv_ref.py's, gates, skips, modes and tap kinds tests/gconv_ref.py's, every numeric bound
K_SCONV, dh_bound and the derived gate tolerances of tests/gsconv_ref.py and tests/gbconv_ref.py. The proof technique is
tests/cconv_ref.py's with the gates concatenated alongside: the kernels are the shipped gated ones with their load ends re-indexed,
and every window they transform is a window the shipped gated plans transform on a concatenated sequence:

    forward        window s of the carried plan = segment s + 1 of TfftGatedLongConvPlan at length hop + L on
                   [zeros(hop - Hn) | hist | x], [ones(hop - Hn) | pre_hist | pre] and [ones(hop) | post]
    input gradient window s of the carried plan = segment s of TfftGatedLongConvGradPlan at length L + Fn on [gy | fut],
                   [post | post_fut], [x | ones(Fn)] and [pre | ones(Fn)], first L samples
    tap gradient   item (p, s) = item (p, s + 1) of that plan at length hop + L on the front-padded x and pre and on
                   [zeros(hop) | gy], [ones(hop) | post]; the items (p, 0) there hold only zeros of gz and add exact zeros

The -0 trap. The padding of a gate must be +1: the shipped kernels WRITE the product 0 * gate where the carried kernels write +0, and
a negative gate there would give -0, which transforms like +0 but is another bit pattern wherever it reaches an output unchanged.
"""
import numpy as np

import bconv_ref as br
import cconv_ref as cr
import gbconv_ref as gb
import gconv_ref as gr
import sconv_ref as sr

N = sr.N
K_SCONV = sr.K_SCONV
TAP_KINDS = gr.TAP_KINDS
CASES = cr.CASES
WITH_CONTEXT = [c for c in CASES if c[4]]
EVERY_CASE_MODE = "pre+post+skip"
# either gate alone: the three smallest cases with a context
SINGLE_GATE_CASES = sorted(WITH_CONTEXT, key=lambda c: ((c[2] + 1) // 2 * sr.geometry(c[0], c[1])[2] * c[3], c[0]))[:3]
# (L, K, B, C, context, launch_iters, mode)
CASE_MODES = [tuple(c) + (EVERY_CASE_MODE,) for c in WITH_CONTEXT] + [tuple(c) + (m,) for c in SINGLE_GATE_CASES for m in ("pre", "post")]

half_product = gr.half_product
gated = gb.gated
extend = cr.extend
carry_min = cr.carry_min


def case_data(length, taps, rows, channels, ctx, kind, seed, mode):
    """dict of a case: x, h, gy and, where the mode has them, pre, post, skip; with a context also hist, fut and the gates' contexts
    pre_hist, post_fut (None where the mode lacks the gate). Every array binary16."""
    x, h, pre, post, skip, gy = gb.case_data(length, taps, rows, channels, kind, seed, mode)
    d = dict(x=x, h=h, pre=pre, post=post, skip=skip, gy=gy, hist=None, fut=None, pre_hist=None, post_fut=None)
    if ctx:
        d["hist"] = cr.context_signal(rows, channels, ctx, seed, 0)
        d["fut"] = cr.context_signal(rows, channels, ctx, seed, 1)
        p, g = gr.gates(rows, channels, ctx, seed + 4099)
        d["pre_hist"] = p if pre is not None else None
        d["post_fut"] = g if post is not None else None
    return d


def ones_like_front(a, n):
    return np.ones(a.shape[:2] + (n,), np.float16)


def front_padded_gate(gate, gate_hist, taps, pad=1.0):
    """[pad(hop - Hn) | gate_hist | gate]: the pre gate (or, with gate_hist = None, [pad(hop) | post]) of the shipped plan at hop + L"""
    hop = sr.geometry(gate.shape[2], taps)[1]
    hn = 0 if gate_hist is None else gate_hist.shape[2]
    return extend(gate, extend(np.full(gate.shape[:2] + (hop - hn,), pad, np.float16), fut=gate_hist))


def forward_concat(d, taps):
    """(x, pre, post) of the shipped gated plan at length hop + L whose output from sample hop on is the carried plan's"""
    x = cr.front_padded(d["x"], d["hist"], taps)
    pre = None if d["pre"] is None else front_padded_gate(d["pre"], d["pre_hist"], taps)
    post = None if d["post"] is None else front_padded_gate(d["post"], None, taps)
    return x, pre, post


def input_grad_concat(d):
    """(gy, post, x, pre) of the shipped gated gradient plan at length L + Fn whose first L samples of dx and dpre are the carried
    plan's"""
    fn = 0 if d["fut"] is None else d["fut"].shape[2]
    ones = ones_like_front(d["gy"], fn)
    gy = extend(d["gy"], fut=d["fut"])
    post = None if d["post"] is None else extend(d["post"], fut=d["post_fut"] if fn else None)
    x = None if d["pre"] is None else extend(d["x"], fut=ones)
    pre = None if d["pre"] is None else extend(d["pre"], fut=ones)
    return gy, post, x, pre


def tap_grad_concat(d, taps):
    """(x, pre, gy, post) of the shipped gated gradient plan at length hop + L whose items (p, s + 1) are the carried plan's (p, s)"""
    hop = sr.geometry(d["x"].shape[2], taps)[1]
    x, pre, _ = forward_concat(dict(d, post=None), taps)
    gy = extend(d["gy"], np.zeros(d["gy"].shape[:2] + (hop,), np.float16))
    post = None if d["post"] is None else front_padded_gate(d["post"], None, taps)
    return x, pre, gy, post


# ---- the gated sequences the kernels transform

def ue(d):
    """(u, u_hist): pre (.) x and pre_hist (.) hist as the kernels form them, one binary16 multiply each"""
    return gated(d["x"], d["pre"]), None if d["hist"] is None else gated(d["hist"], d["pre_hist"])


def gze(d):
    """(gz, gz_fut): post (.) gy and post_fut (.) fut"""
    return gated(d["gy"], d["post"]), None if d["fut"] is None else gated(d["fut"], d["post_fut"])


def windows(d, taps):
    """the complex windows the carried forward plan (and pass (a) of its tap gradient) transforms: cconv_ref.windows of the gated
    sequence and the gated history, binary16 values, (re, im) each [items][4096]"""
    u, uh = ue(d)
    return cr.windows(u, taps, uh)


def dx_windows(d, taps):
    gz, gf = gze(d)
    return cr.dx_windows(gz, taps, gf)


# ---- the definitions of include/tfft_gcconv.h by direct fp64 sums (of the exact products: nothing is rounded)

def _prod(a, gate):
    return np.asarray(a).astype(np.float64) if gate is None else np.asarray(a).astype(np.float64) * np.asarray(gate).astype(np.float64)


def _ue64(d):
    return _prod(d["x"], d["pre"]), None if d["hist"] is None else _prod(d["hist"], d["pre_hist"])


def _gze64(d):
    return _prod(d["gy"], d["post"]), None if d["fut"] is None else _prod(d["fut"], d["post_fut"])


def y_direct(d):
    u, uh = _ue64(d)
    z = cr.y_direct(u, gb.taps_with_skip(d["h"], d["skip"]), uh)
    return z if d["post"] is None else z * d["post"].astype(np.float64)


def input_grad_direct(d):
    """(dx, dpre or None)"""
    gz, gf = _gze64(d)
    du = cr.dx_direct(gz, gb.taps_with_skip(d["h"], d["skip"]), gf)
    if d["pre"] is None:
        return du, None
    return du * d["pre"].astype(np.float64), du * d["x"].astype(np.float64)


def dh_direct(d, taps):
    u, uh = _ue64(d)
    return cr.dh_direct(u, _gze64(d)[0], taps, uh)


def dh_items(d, taps):
    """the fp64 circular correlations of the plan's own items, of the ROUNDED products the kernel sees: [items][4096]"""
    u, uh = ue(d)
    return cr.dh_items(u, gze(d)[0], taps, uh)


# ---- the units and rounding terms of tests/gsconv_ref.py and tests/gbconv_ref.py on the carried plans' own windows

def _spec(d):
    return np.fft.fft(gb.taps_with_skip(d["h"], d["skip"]), N, axis=-1)


def reference_true(d):
    """the circular convolution of every window of the carried forward plan with the binary16 taps and skip, in fp64: [items][4096]
    (gsconv_ref.reference_true with the gated history in the windows)"""
    re, im = (p.astype(np.float64) for p in windows(d, d["h"].shape[1]))
    return np.fft.ifft(np.fft.fft(re + 1j * im, axis=-1) * _spec(d)[np.arange(re.shape[0]) % d["x"].shape[1]], axis=-1)


def du_windows_true(d):
    """the circular correlation of every window of the carried input gradient with the binary16 taps and skip, in fp64
    (gbconv_ref.du_windows_true with the gated future in the windows)"""
    re, im = (p.astype(np.float64) for p in dx_windows(d, d["h"].shape[1]))
    return np.fft.ifft(np.fft.fft(re + 1j * im, axis=-1) * np.conj(_spec(d))[np.arange(re.shape[0]) % d["gy"].shape[1]], axis=-1)


def du_input_rounding(d):
    """gbconv_ref.du_input_rounding with the future: sum_j |h'[j]| 2^-11 |qe gye|[t + j], [B][C][L]; zero without a post gate"""
    if d["post"] is None:
        return np.zeros(d["gy"].shape)
    gz, gf = _gze64(d)
    return 2.0 ** -11 * cr.dx_direct(np.abs(gz), np.abs(gb.taps_with_skip(d["h"], d["skip"])), None if gf is None else np.abs(gf))


def dh_input_rounding(d, taps):
    """gbconv_ref.dh_input_rounding with the history: (2^-10 + 2^-22) sum |gz|[t] |ue|[t - j], [C][K]; zero without gates"""
    if d["pre"] is None and d["post"] is None:
        return np.zeros((d["x"].shape[1], taps))
    u, uh = _ue64(d)
    return (2.0 ** -10 + 2.0 ** -22) * cr.dh_direct(np.abs(u), np.abs(_gze64(d)[0]), taps, None if uh is None else np.abs(uh))
