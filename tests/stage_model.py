"""numpy models of the single-pass kernels N = 256 .. 4096: the stage arithmetic of tensor-fft_amd/csrc/k256.hpp, k256r.hpp and k4096.hpp
read off their headers and build_tables (test infrastructure, host only, importable like elementwise_bound.py).

Every kernel is a chain of 16 x 16 contractions with binary16 constant operands, fp32 accumulators, fp32 twiddles between the
stages and ONE rounding to binary16 behind each stage:

    N = 256       n = n0 + 16 n1, k = k0 + 16 k1
                  X[k0 + 16 k1] = h16(sum_n0 F[n0][k1] * h16(TW[n0][k0] * sum_n1 F[n1][k0] x[n0 + 16 n1]))
                  F = h16(w16 f), TW = fp32(w256^(n0 k0) tw)
    N = 256 R     n = R (n0 + 16 n1) + r, k = k0 + 16 k1 + 256 s (R = 2, 4, 8)
                  t_r = h16(S[n0][k0] * sum_n1 Fa[n1][k0] x),  S = fp32(w256^(n0 k0) s)
                  o_r = fp32(sum_n0 Fb[n0][k1] t_r),  v_r = o_r * fp32(w_N^(r (k0 + 16 k1)))   (r = 0: no multiply)
                  X[.. + 256 s] = h16(sum_r W_R[r][s] v_r): the radix-R butterfly of stockham.hpp in fp32, exact factors +-1, +-i
                  for R = 2, 4; dft<8> multiplies by (+-h, -h) with h = fp32(sqrt 1/2)
    N = 4096      n = n0 + 16 n1 + 256 n2, k = k0 + 16 k1 + 256 k2
                  stage 1 contracts n2 (F1), stage 2 n1 (G2) with the fp32 twiddle TW = w256^(n0 k1) tw on its accumulators,
                  stage 3 n0 (H3); h16 behind each

The factors f, g, h, tw (fa, fb, s) are what apply_scale_mode (tfft.hip) makes of tfft_plan_opts.scale: sequential 1/16 per MFMA
stage (and 1/R on S); none all 1; once as none with 1/N on the fp32 twiddle block at N = 256, and at N = 512 .. 4096 with 16/N on
that block and 1/16 in the last stage's constants (Fb, H3), which makes the operand of the last stage the sequential one. The
inverse is the forward model with the planes exchanged on both sides (tfft_exec_inverse).

Two conversions, on purpose: a TABLE entry is rounded once from fp64 (_t16, as static_cast<_Float16>(double) in build_tables), an
ACCUMULATOR goes through fp32 (_c16, as v_cvt_pk_f16_f32 of an fp32 register). Sums are exact to fp64: where the hardware's fp32
order of operations (the MFMA's rounding of a two-term sum, the fmaf of the twiddle product, the butterfly's additions) lands on
the other side of a binary16 rounding tie, a kernel may differ from the model by one ulp of that intermediate
(tests/test_stage_model_host.py derives what that does to the output).

For an impulse x = a delta_p every contraction has one non-zero input, so the result is a product of table entries and
roundings: impulse_sweep() evaluates that closed form for every p at once by broadcasting over the digit indices.
"""
import functools

import numpy as np

MODES = ("sequential", "none", "once")
# not a mode of the library: scale once with the WHOLE 1/N on the fp32 twiddle at every length, as the single kernels had it before
# the last stage of N = 512 .. 4096 kept its 1/16. Modelled to show why it went (tests/test_stage_model_host.py).
ONCE_ON_TWIDDLE = "once, 1/N on the twiddle"
SIZES = (256, 512, 1024, 2048, 4096)
SQRT_HALF = float(np.float32(0.70710678118654752))     # stockham.hpp dft<8>


def _cexp(num, den):
    a = -2.0 * np.pi * (np.asarray(num) % den) / den
    return np.cos(a) + 1j * np.sin(a)


def _c16(z):
    """component by component to binary16 (through fp32, as the kernels convert their accumulators), back as complex128"""
    with np.errstate(over="ignore"):
        return (z.real.astype(np.float32).astype(np.float16).astype(np.float64)
                + 1j * z.imag.astype(np.float32).astype(np.float16).astype(np.float64))


def _t16(z):
    """a table entry: ONE rounding from fp64 to binary16 (build_tables: static_cast<_Float16>(double)), back as complex128"""
    return z.real.astype(np.float16).astype(np.float64) + 1j * z.imag.astype(np.float16).astype(np.float64)


def _f32(z):
    """an fp32 table entry or accumulator, back as complex128"""
    with np.errstate(over="ignore"):
        return z.real.astype(np.float32).astype(np.float64) + 1j * z.imag.astype(np.float32).astype(np.float64)


_I = np.arange(16)


def factors(n, mode="sequential"):
    """apply_scale_mode for a single-kernel plan of length n: the factors folded into the constant operands"""
    assert mode in MODES + (ONCE_ON_TWIDDLE,) and n in SIZES
    s16 = 1.0 / 16 if mode == "sequential" else 1.0
    fin = 1.0 / n if mode in ("once", ONCE_ON_TWIDDLE) else 1.0
    last = 1.0 / 16 if mode == "once" else s16             # N = 512 .. 4096, once: the last stage keeps its 1/16, the twiddle has 16/N
    if n == 4096:
        return {"f": s16, "g": s16, "h": last, "tw": fin * (s16 / last)}
    if n == 256:
        return {"f": s16, "tw": fin}
    return {"fa": s16, "fb": last, "s": (256.0 / n if mode == "sequential" else 1.0) * fin * (s16 / last)}


@functools.lru_cache(maxsize=None)
def tables4096(mode="sequential", table16=_t16):
    """F1[n2][k0], G2[k0][n1][k1], TW[n0][k1] (fp32), H3[k0][n0][k2] of k4096::build_tables"""
    s = factors(4096, mode)
    f1 = table16(_cexp(_I[:, None] * _I[None, :], 16) * s["f"])
    g2 = table16(_cexp(_I[None, :, None] * (_I[:, None, None] + 16 * _I[None, None, :]), 256) * s["g"])
    tw = _f32(_cexp(_I[:, None] * _I[None, :], 256) * s["tw"])
    h3 = table16(_cexp(_I[None, :, None] * (_I[:, None, None] + 256 * _I[None, None, :]), 4096) * s["h"])
    return f1, g2, tw, h3


@functools.lru_cache(maxsize=None)
def tables256(mode="sequential"):
    """F[n][k] (both stages) and TW[n0][k0] (fp32): the natural-order F and the twiddle block of k4096::build_tables"""
    s = factors(256, mode)
    return _t16(_cexp(_I[:, None] * _I[None, :], 16) * s["f"]), _f32(_cexp(_I[:, None] * _I[None, :], 256) * s["tw"])


def butterfly(r):
    """W[r][s]: what stockham::dft<R> multiplies input r by on its way to output s"""
    idx = np.arange(r)
    if r in (2, 4):
        return np.array([1, -1j, -1, 1j])[(idx[:, None] * idx[None, :] * (4 // r)) % 4].astype(np.complex128)
    # dft<8>: n = n0 + 4 n1, k = k0 + 2 k1: y[n0][k0] = sum_n1 (-1)^(n1 k0) v, y[n0][1] *= c8[n0], then a DFT-4 over n0
    h = SQRT_HALF
    c8 = np.array([1.0, h - 1j * h, -1j, -h - 1j * h])
    w = np.empty((8, 8), np.complex128)
    for n in range(8):
        for k in range(8):
            n0, n1, k0, k1 = n % 4, n // 4, k % 2, k // 2
            w[n, k] = (-1.0) ** (n1 * k0) * (c8[n0] if k0 else 1.0) * (-1j) ** (n0 * k1)
    return w


@functools.lru_cache(maxsize=None)
def tables256r(n, mode="sequential"):
    """Fa[n1][k0], Fb[n0][k1], S[n0][k0] (fp32), T[r][kk] (fp32, row 0 = 1), W[r][s] of k256r::build_tables and dft<R>"""
    s = factors(n, mode)
    r = n // 256
    w16 = _cexp(_I[:, None] * _I[None, :], 16)
    t = _f32(_cexp(np.arange(r)[:, None] * np.arange(256)[None, :], n))
    t[0] = 1.0
    return _t16(w16 * s["fa"]), _t16(w16 * s["fb"]), _f32(_cexp(_I[:, None] * _I[None, :], 256) * s["s"]), t, butterfly(r)


# legacy names: the sequential tables of N = 4096 (tests/test_conv_range_host.py)
F1, G2, TW, H3 = tables4096()


def _planes(re, im):
    return np.asarray(re, np.float16).astype(np.float64) + 1j * np.asarray(im, np.float16).astype(np.float64)


def _stages4096(x, mode="sequential", round_last=True):
    """x: complex128 [..., 4096] -> (a3 rounded [..., 4096] in natural order, (a1, a2, a3) in front of the roundings, in the
    layouts [k0][n1][b][n0], [k0][k1][b][n0], [k0][k1][b][k2] over the flattened leading axes b)"""
    f1, g2, tw, h3 = tables4096(mode)
    lead = x.shape[:-1]
    x = x.reshape(-1, 16, 256)                                            # [b][n2][n1 n0]
    b = x.shape[0]
    # 16 large matrix products per stage, one per tile k0 (a whole batch of 4096 transforms in about a second)
    with np.errstate(invalid="ignore", over="ignore"):                    # (the overflow tests feed inputs that end in inf and nan)
        a1 = (f1.T @ x).reshape(b, 16, 16, 16).transpose(1, 2, 0, 3)      # [k0][n1][b][n0] = sum_n2 F1[n2][k0] x[n2][n1][n0]
        r1 = _c16(a1).reshape(16, 16, b * 16)
        a2 = (g2.transpose(0, 2, 1) @ r1).reshape(16, 16, b, 16) * tw.T[None, :, None, :]   # [k0][k1][b][n0], sum over n1 of G2[k0][n1][k1]
        r2 = _c16(a2).reshape(16, 16 * b, 16)
        a3 = (r2 @ h3).reshape(16, 16, b, 16)                             # [k0][k1][b][k2], sum over n0 of H3[k0][n0][k2]
    out = _c16(a3) if round_last else _f32(a3)
    return out.transpose(2, 3, 1, 0).reshape(lead + (4096,)), (a1, a2, a3)


def stage_model(re, im):
    """DFT(x) / 4096 by three 1/16-scaled radix-16 stages with binary16 constants and one rounding to binary16 behind each
    (n = n0 + 16 n1 + 256 n2, k = k0 + 16 k1 + 256 k2; stage 1 contracts n2, stage 2 n1 with the fp32 twiddle w256^(n0 k1) on its
    accumulators, stage 3 n0). Returns (the spectrum as complex128 in natural order, [the largest |component| in front of each
    stage's rounding])."""
    out, acc = _stages4096(_planes(re, im))
    return out, [float(max(np.abs(a.real).max(), np.abs(a.imag).max())) for a in acc]


def _stages(x, round_last):
    """the three sequential stages on complex128 samples; round_last = False leaves stage 3 in fp32 (conv4096's first half)"""
    return _stages4096(x, "sequential", round_last)[0]


def _stages256(x, mode="sequential"):
    f, tw = tables256(mode)
    x = x.reshape(x.shape[:-1] + (16, 16))                               # [n1][n0]
    a1 = np.einsum("ak,...ab->...bk", f, x) * tw                         # [n0][k0]
    a2 = np.einsum("bj,...bk->...jk", f, _c16(a1))                       # [k1][k0]
    return _c16(a2).reshape(a2.shape[:-2] + (256,)), (a1, a2)


def _stages256r(x, n, mode="sequential"):
    fa, fb, s, t, w = tables256r(n, mode)
    r = n // 256
    x = x.reshape(x.shape[:-1] + (16, 16, r))                            # [n1][n0][r]
    a1 = np.einsum("ak,...abr->...bkr", fa, x) * s[:, :, None]           # [n0][k0][r]
    o = _f32(np.einsum("bj,...bkr->...jkr", fb, _c16(a1)))               # [k1][k0][r], fp32
    v = o * np.moveaxis(t.reshape(r, 16, 16), 0, -1)                     # T[r][k0 + 16 k1] as [k1][k0][r]
    a3 = np.einsum("rs,...jkr->...sjk", w, v)                            # [s][k1][k0]
    return _c16(a3).reshape(a3.shape[:-3] + (n,)), (a1, o, a3)


def accumulators(n, re, im, mode="sequential"):
    """(the spectrum, the values in front of every rounding) of the forward model: for range and subnormal checks"""
    x = _planes(re, im)
    if n == 4096:
        return _stages4096(x, mode)
    return _stages256(x, mode) if n == 256 else _stages256r(x, n, mode)


def forward(n, re, im, mode="sequential"):
    """the model of the plan of length n on binary16 planes [..., n]: the spectrum as complex128"""
    return accumulators(n, re, im, mode)[0]


def inverse(n, re, im, mode="sequential"):
    """tfft_exec_inverse: the forward transform with the planes exchanged on both sides"""
    y = forward(n, im, re, mode)
    return y.imag + 1j * y.real


# ---- closed forms for x = a delta_p, every p at once

def _bc(a, axes, ndim):
    """a, whose axes are the listed axes of an ndim-dimensional result, shaped for broadcasting"""
    order = np.argsort(axes)
    shape = [1] * ndim
    for ax, size in zip(axes, a.shape):
        shape[ax] = size
    return a.transpose(order).reshape(shape)


def impulse_operands(n, a=1024.0, mode="sequential"):
    """x = a delta_p, every p: (r, c, t, acc). r is the LAST binary16 intermediate (the rounded operand of the last MFMA stage), c
    the constant of that stage, t what multiplies the fp32 result behind it (N = 256 R: the twiddle T and the butterfly's factor;
    None otherwise), all shaped for broadcasting over the result's digit axes; the value in front of the final rounding is
    r c (t). acc: the arrays in front of the earlier roundings."""
    a = complex(a)
    if n == 4096:
        f1, g2, tw, h3 = tables4096(mode)
        # result axes [n2][n1][n0][k2][k1][k0]
        a1 = f1 * a                                                                    # [n2][k0]
        a2 = _bc(_c16(a1), (0, 4), 5) * _bc(g2, (4, 1, 3), 5) * _bc(tw, (2, 3), 5)      # [n2][n1][n0][k1][k0]
        return _c16(a2).reshape(16, 16, 16, 1, 16, 16), _bc(h3, (5, 2, 3), 6), None, [a1, a2]
    if n == 256:
        f, tw = tables256(mode)
        # result axes [n1][n0][k1][k0]
        a1 = _bc(f, (0, 3), 4) * a * _bc(tw, (1, 3), 4)                                # [n1][n0][1][k0]
        return _c16(a1), _bc(f, (1, 2), 4), None, [a1]
    fa, fb, s, t, w = tables256r(n, mode)
    # result axes [n1][n0][r][s][k1][k0]
    a1 = _bc(fa, (0, 5), 6) * a * _bc(s, (1, 5), 6)                                    # [n1][n0][1][1][1][k0]
    return _c16(a1), _bc(fb, (1, 4), 6), _bc(t.reshape(n // 256, 16, 16), (2, 4, 5), 6) * _bc(w, (2, 3), 6), [a1]


def nudge16(z, d_re, d_im):
    """z (binary16 values as complex128) with its components moved by d_re, d_im (-1, 0, 1) binary16 neighbours: the other
    side of a rounding tie"""
    def move(v, d):
        h = v.astype(np.float16)
        return (np.nextafter(h, np.float16(np.inf * d)) if d else h).astype(np.float64)
    return move(z.real, d_re) + 1j * move(z.imag, d_im)


def impulse_sweep(n, a=1024.0, mode="sequential", with_accumulators=False, nudge=(0, 0)):
    """The model's answer to x = a delta_p for every p (a: complex, 1024 = RE plane, 1024j = IM plane): (re, im) as binary16
    [p][k]. with_accumulators: also the list of arrays in front of every rounding (any shape), for range checks. nudge: the
    last binary16 intermediate moved to a neighbour first (nudge16): what a different fp32 order of operations may do."""
    r, c, t, acc = impulse_operands(n, a, mode)
    if nudge != (0, 0):
        r = nudge16(r, *nudge)
    if n == 4096:
        # the last stage in fp32 planes: the products of two binary16 numbers are exact in fp32, their sum is rounded once to
        # fp32 and then to binary16, which is _c16 of the exact value
        cr, ci = c.real.astype(np.float32), c.imag.astype(np.float32)
        rr, ri = r.real.astype(np.float32), r.imag.astype(np.float32)
        o_re, o_im = cr * rr - ci * ri, cr * ri + ci * rr
        acc = acc + [o_re, o_im]
    elif n == 256:
        last = c * r
        o_re, o_im = last.real, last.imag
        acc = acc + [last]
    else:
        o = _f32(c * r)                                                                # stage 2 stays in fp32
        last = o * t
        o_re, o_im = last.real, last.imag
        acc = acc + [o, last]
    with np.errstate(over="ignore"):
        out = (o_re.astype(np.float32).astype(np.float16).reshape(n, n), o_im.astype(np.float32).astype(np.float16).reshape(n, n))
    return out + (acc,) if with_accumulators else out


def impulse_sweep_inverse(n, a=1024.0, mode="sequential"):
    """exec_inverse of x = a delta_p: the planes exchanged on both sides of the forward model"""
    a = complex(a)
    re, im = impulse_sweep(n, complex(a.imag, a.real), mode)
    return im, re


def impulse_exact(n, a=1024.0, inverse=False):
    """(a / n) w_n^(+-p k) in fp64 as (re, im) [p][k], from a table of the n roots"""
    idx = np.arange(n)
    e = (idx[:, None] * idx[None, :]) % n
    ang = (2.0 if inverse else -2.0) * np.pi * np.arange(n) / n
    w = np.cos(ang) + 1j * np.sin(ang)
    # exact zeros where the angle is a multiple of a quarter turn (cos(pi / 2) is 6e-17 in fp64)
    q = n // 4
    w[[0, q, 2 * q, 3 * q]] = [1, 1j if inverse else -1j, -1, -1j if inverse else 1j]
    z = (complex(a) / n) * w
    return z.real[e], z.imag[e]


def ulp16(v):
    """binary16 ulp of the magnitude v (normal range)"""
    return 2.0 ** (np.floor(np.log2(v)) - 10)
