"""Test infrastructure of the gradient plans of the gated overlap-save causal convolution (include/tfft_gbconv.h): the cases and
modes that tests/test_gbconv_host.py and tests/test_gpu_gbconv.py share, the numpy model of the kernels' route, the fp64
torch.autograd reference of the forward operator, and the derived tolerances of the autograd comparison.

Nothing here is new data or a new constant: signals and taps are tests/lconv_ref.py's, gates, skips and modes tests/gconv_ref.py's,
gy tests/bconv_ref.py's, shapes, windows and K_SCONV tests/sconv_ref.py's, the tap gradient's bound tests/bconv_ref.py's (all
imported read-only). The gated kernels restate bconv4096's arithmetic between exact-to-one-rounding multiplies, and the GPU test holds
them bit for bit to shipped code on host-built products, which ties them to the classes profiles/bconv_ulps.txt measured.

The operator and its gradients (pre, post: the gates; d: the skip; gy = d loss / d y):

    u = pre (.) x      z = h' * u   (h' = h with d[c] added to tap 0)      y = post (.) z
    gz = post (.) gy
    du[b][c][t] = sum_{j < K, t + j < L} h'[c][j] gz[b][c][t + j]          dx = pre (.) du      dpre = x (.) du
    dh[c][j]    = sum_b sum_{t >= j} gz[b][c][t] u[b][c][t - j]            dskip[c] = dh[c][0]
    dpost = gy (.) z

The kernels' route. Input gradient: the post gate is applied BEFORE the windows are cut (window chunk j of segment s is source chunk
s * hop / 8 + j of gy AND of post), the windows start at s * hop with no front halo, are correlated circularly with h', the first hop
samples are kept and joined, and the pre gate (and x) is applied AFTER, by output sample. A kernel that takes either gate at the
forward pass's window origin, s * hop - halo, is wrong wherever halo != 0. Tap gradient: both gates by source sample before the
forward pass's windows are cut (they start at s * hop - halo), the gz window with its first halo samples zeroed.

Tolerances of the autograd comparison. The reference is torch.autograd through an fp64 conv1d of the forward operator, which rounds
nothing; the kernels round gz = post gy and u = pre x to binary16 first. With round16(v) = v (1 + e), |e| <= 2^-11:

  du    The kernel's du lies within (K_SCONV + 1) ulp16(peak) of the correlation of the ROUNDED gz with the binary16 taps and skip
        (peak: the largest magnitude of the window's circular correlation; tests/bconv_ref.py, tests/sconv_ref.py). The rounding of
        gz moves that correlation by at most sum_j |h'[c][j]| 2^-11 |post gy|[t + j]                       (du_input_rounding)
  dx    = round16(pre du): |pre| times the two terms above, plus 1/2 ulp16(|dx|) for the gate's one rounding
        (tests/gsconv_ref.py, post_gate_tolerance, with the input rounding added before the gate's factor); dpre the same with x
        in the place of pre. Without a pre gate dx = du and the two terms stand alone.
  dh    The kernel's dh lies within bconv_ref.dh_bound of the direct sum over the ROUNDED gz and u. Both factors of every product
        are rounded: (1 + 2^-11)^2 - 1 = 2^-10 + 2^-22 times sum_{b, t} |post gy|[t] |pre x|[t - j]        (dh_input_rounding)
        (with one gate only one factor is rounded; the test keeps the two-factor term whenever a gate is present, and zero
        without gates.) dskip = dh[:, 0], bit for bit.
  dpost the forward plan with gy as its post gate: tests/gsconv_ref.py's tolerance, K_SCONV + 1.

tests/test_gbconv_host.py checks that the numpy model with the two binary16 products (fp64 everywhere else) stays inside each of
these bounds on the GPU test's inputs, so the rounding terms alone cover what they are there for.
"""
import numpy as np

import bconv_ref as br
import elementwise_bound as eb
import gconv_ref as gr
import gsconv_ref as gs
import lconv_ref as lr
import sconv_ref as sr

N = sr.N
K_SCONV = sr.K_SCONV
TAP_KINDS = gr.TAP_KINDS
GATE_MODES = gr.GATE_MODES

# (L, K, B, C, launch_iters, mode): the input gradient's cases
DX_CASE_MODES = gs.CASE_MODES


def items_per_channel(case):
    length, taps, rows = case[:3]
    return (rows + 1) // 2 * sr.geometry(length, taps)[2]


# (L, K, B, C, partials cap, mode): the tap gradient's cases: every case of bconv_ref.DH_CASES with both gates, and the four with the
# fewest items per channel with either gate alone
SINGLE_GATE_CASES = sorted(br.DH_CASES, key=items_per_channel)[:4]
DH_CASE_MODES = [tuple(c) + ("pre+post",) for c in br.DH_CASES] + [tuple(c) + (m,) for c in SINGLE_GATE_CASES for m in ("pre", "post")]
# the autograd cases
AUTOGRAD_CASES = [(4104, 7, 3, 3), (2048, 2049, 3, 3)]
AUTOGRAD_MODE = "pre+post+skip"

half_product = gr.half_product


def case_data(length, taps, rows, channels, kind, seed, mode):
    """(x, h, pre or None, post or None, skip or None, gy) of a case"""
    x, h, pre, post, skip = gr.case_data(length, taps, rows, channels, kind, seed, mode)
    return x, h, pre, post, skip, br.grad_signal(rows, channels, length, taps, seed)


def gated(a, gate):
    """a (.) gate as the kernels form it: one binary16 multiply, or a itself without a gate"""
    return a if gate is None else half_product(gate, a)


def taps_with_skip(h, skip):
    """[C][K] fp64: the taps with the skip weight added to tap 0 (gconv_ref.taps_with_skip for binary16 taps; fp64 taps are kept as
    they are)"""
    h = np.array(h, np.float64)
    if skip is not None:
        h[:, 0] += np.asarray(skip).astype(np.float64)
    return h


def f64(a):
    return None if a is None else np.asarray(a).astype(np.float64)


# ---- the numpy model of the kernels' route (fp64; `rounded` forms the two input products in binary16, as the kernels do)

def model_du(gy, h, post, skip, rounded=False, post_origin=0):
    """gate -> windows from s * hop -> circular correlation with h' -> the first hop samples joined: [B][C][L] fp64.
    post_origin = -halo takes the post gate at the forward pass's window origin: the wrong route."""
    rows, channels, length = gy.shape
    taps = h.shape[1]
    if post is None:
        gz = f64(gy)
    elif post_origin == 0:
        gz = f64(half_product(post, gy)) if rounded else f64(post) * f64(gy)
    else:
        shifted = np.zeros(gy.shape)
        shifted[:, :, -post_origin:] = f64(post)[:, :, :length + post_origin]           # post[t + post_origin]
        gz = shifted * f64(gy)
    re, im = br.dx_windows(gz, taps)
    spec = np.conj(np.fft.fft(f64(taps_with_skip(h, skip)), N, axis=-1))
    y = np.fft.ifft(np.fft.fft(re + 1j * im, axis=-1) * spec[np.arange(re.shape[0]) % channels], axis=-1)
    return br.dx_unwindow(y.real, y.imag, rows, channels, length, taps)


def model_input_grad(x, h, pre, post, skip, gy, rounded=False, post_origin=0, pre_origin=0):
    """(dx, dpre or None) by the kernel's route. rounded: the output products rounded to binary16 too. pre_origin = halo takes the
    pre gate (and x) at the forward pass's window origin on the store side: the wrong route."""
    du = model_du(gy, h, post, skip, rounded, post_origin)
    if pre is None:
        return du, None
    length = du.shape[2]

    def at(a):
        if pre_origin == 0:
            return f64(a)
        out = np.zeros(du.shape)
        out[:, :, :length - pre_origin] = f64(a)[:, :, pre_origin:]                     # a[t + pre_origin]
        return out

    dx, dpre = at(pre) * du, at(x) * du
    if rounded:
        dx, dpre = f64(dx.astype(np.float16)), f64(dpre.astype(np.float16))
    return dx, dpre


def model_tap_grad(x, pre, gy, post, taps, rounded=False):
    """(dh [C][K], dskip [C]) by the kernel's route: gates -> the forward windows of u and gz, the latter with its halo zeroed ->
    conj(fft(Zu)) fft(Zg) -> the RE plane's lags 0 .. K - 1 summed over a channel's items"""
    channels = x.shape[1]
    u = f64(gated(x, pre)) if rounded or pre is None else f64(pre) * f64(x)
    gz = f64(gated(gy, post)) if rounded or post is None else f64(post) * f64(gy)
    dh = br.dh_from_items(br.dh_items(u, gz, taps), channels, taps)
    return dh, dh[:, 0].copy()


def model_dpost(x, h, pre, skip, gy, rounded=False):
    """gy (.) z by the forward kernel's route (gsconv_ref.model)"""
    u = f64(gated(x, pre)) if rounded else (f64(x) if pre is None else f64(pre) * f64(x))
    return f64(gy) * gs.model(u, f64(h), None, None, f64(skip))


# ---- the fp64 reference: torch.autograd through conv1d on the CPU

def autograd_reference(x, h, pre, post, skip, gy):
    """dict of the gradients of y = post (.) (h' * (pre (.) x)) for d loss / d y = gy, all fp64 numpy: dx, dh, and dpre, dpost, dskip
    where that input exists"""
    import torch

    taps, channels = h.shape[1], h.shape[0]
    leaves = {k: torch.from_numpy(f64(v)).requires_grad_() for k, v in (("x", x), ("h", h), ("pre", pre), ("post", post), ("skip", skip)) if v is not None}
    u = leaves["x"] * leaves["pre"] if pre is not None else leaves["x"]
    z = torch.nn.functional.conv1d(torch.nn.functional.pad(u, (taps - 1, 0)), leaves["h"].flip(-1).unsqueeze(1), groups=channels)
    if skip is not None:
        z = z + leaves["skip"][None, :, None] * u
    y = z * leaves["post"] if post is not None else z
    y.backward(torch.from_numpy(f64(gy)))
    return {"d" + k: v.grad.numpy() for k, v in leaves.items()}


# ---- tolerances

def per_sample(per_window, rows, channels, length, taps):
    """one value per window of the input gradient [items] -> the value of the window that holds each sample of dx: [B][C][L]"""
    full = np.repeat(np.asarray(per_window, np.float64)[:, None], N, axis=1)
    return br.dx_unwindow(full, full, rows, channels, length, taps)


def du_windows_true(gz, h, skip):
    """the circular correlation of every window of gz with the binary16 taps and skip, in fp64: [items][4096]"""
    return br._correlate_windows(gz, h.shape[1], np.conj(np.fft.fft(taps_with_skip(h, skip), N, axis=-1)))


def du_peak(gz, h, skip):
    """the unit of K_SCONV for the input gradient: the largest magnitude of each window's circular correlation, [items]"""
    return sr.window_peak(du_windows_true(gz, h, skip))


def du_input_rounding(gy, h, post, skip):
    """sum_j |h'[c][j]| 2^-11 |post gy|[t + j]: what rounding gz to binary16 moves du by at most, [B][C][L]; zero without a post gate"""
    if post is None:
        return np.zeros(gy.shape)
    return 2.0 ** -11 * br.dx_direct(np.abs(f64(post) * f64(gy)), np.abs(taps_with_skip(h, skip)))


def gated_tolerance(y, gate, before):
    """|gate| * (the error bound in front of the gate) + 1/2 ulp16(|y|) per sample; without a gate the bound in front alone"""
    if gate is None:
        return before
    return np.abs(f64(gate)) * before + 0.5 * eb.ulp16(np.abs(f64(y)))


def dx_tolerance(y, gate, k, peak, rows, channels, length, taps, input_rounding=0.0):
    """the tolerance of dx (gate = pre) or dpre (gate = x) against fp64: gsconv_ref.post_gate_tolerance with the propagated input
    rounding added before the gate's factor"""
    return gated_tolerance(y, gate, k * per_sample(eb.ulp16(peak), rows, channels, length, taps) + input_rounding)


def dh_input_rounding(x, pre, gy, post, taps):
    """(2^-10 + 2^-22) sum_{b, t} |post gy|[t] |pre x|[t - j]: [C][K]; zero without gates"""
    if pre is None and post is None:
        return np.zeros((x.shape[1], taps))
    u = np.abs(f64(x) if pre is None else f64(pre) * f64(x))
    gz = np.abs(f64(gy) if post is None else f64(post) * f64(gy))
    return (2.0 ** -10 + 2.0 ** -22) * br.dh_direct(u, gz, taps)


def dh_bound_rounded(x, pre, gy, post, taps):
    """bconv_ref.dh_bound on the rounded products the kernel sees: [C]"""
    return br.dh_bound(br.dh_items(gated(x, pre), gated(gy, post), taps), x.shape[1])


def dpost_tolerance(dpost, x, h, pre, skip, gy):
    """gsconv_ref.post_gate_tolerance of the forward plan run with gy as its post gate, K_SCONV + 1 (against the true result)"""
    rows, channels, length = x.shape
    taps = h.shape[1]
    peak = sr.window_peak(gs.reference_true(gated(x, pre), h, skip))
    return gs.post_gate_tolerance(dpost, gy, K_SCONV + 1.0, peak, rows, channels, length, taps)
