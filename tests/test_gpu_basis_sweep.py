"""The single-pass kernels N = 256 .. 4096 on EVERY basis vector, against their stage arithmetic. Needs an MI355X: `-m gpu`.

The accuracy tests elsewhere feed white noise and bound the error in ulps of the largest bin: one wrong twiddle, a constant kept
too narrow or a truncating conversion hides under those bounds (tests/elementwise_bound.py says so itself). Here every case is ONE
plan execution of batch N whose transform p holds basis vector p, compared with tests/stage_model.py, the kernels' arithmetic
written out in numpy: three (two) 16 x 16 contractions with binary16 constants, fp32 twiddles, one rounding per stage.

a. x = 1024 delta_p in the RE and in the IM plane, forward and exec_inverse. The arithmetic is then fully determined (one non-zero
   input per contraction), so every output component equals the model's unless an fp32 operation order put an intermediate on
   the other side of a binary16 rounding: at most 2 u = 2 ulp16(1024 / N) away (derived and checked in
   tests/test_stage_model_host.py), and rare. How rare is a fixed number: profiles/basis_ulps.txt (tools/basis_accuracy.py)
   has 0, 16, 128, 856 and 8 of the 2 N^2 components for N = 256 .. 4096, the same in both planes and directions; the cap
   is 4 x that share (room for a later, legitimate change of an fp32 summation order) and never more than 1 %. One table entry
   off by one index or by one binary16 ulp moves every output it serves: N / 16 or more components per p.
b. TFFT_SCALE_ONCE equals the sequential output and TFFT_SCALE_NONE equals N times it, bit for bit, on the same sweep.
c. x_t = h16(exp(+2 pi i f t / N)) for every f through elementwise_bound.check against fp64 of the rounded input, with K_TONE in
   place of K_TABLE, and no bin other than f above K_TONE ulp of the line.
"""
import numpy as np
import pytest

import basis_sweep as bs
import elementwise_bound as eb
import stage_model as sm

pytestmark = pytest.mark.gpu

SHARE_CAP = bs.SHARE_CAP       # 4 x the share measured in profiles/basis_ulps.txt, per N (tests/basis_sweep.py)
# profiles/basis_ulps.txt, "class worst tones": 0.317 ulp (N = 256 and 4096; the model gives the same figures) -> the smallest
# half-integer >= 1.5 x 0.317, the rule of tests/elementwise_bound.py
K_TONE = 0.5


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import torch

    assert torch.cuda.is_available()
    import tensor_fft_amd as t

    t.device_check(0)
    return t


@pytest.fixture(scope="module")
def torch():
    import torch as t

    return t


def test_the_caps_follow_the_profile():
    assert all(4 * c <= 0.01 * 2 * n * n and c <= 0.0025 * 2 * n * n for n, c in bs.DIFFERING.items()) and K_TONE < eb.K_TABLE


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("plane", bs.PLANES)
@pytest.mark.parametrize("n", sm.SIZES)
def test_impulse_at_every_position(tf, torch, n, plane, inverse):
    bs.check_impulses(tf, torch, n, plane, inverse, SHARE_CAP[n])


@pytest.mark.parametrize("n", [256, 1024, 4096])
def test_scale_modes_bit_for_bit(tf, torch, n):
    """include/tfft.h: the modes differ by exact powers of two away from over- and underflow. (With the whole 1 / N on the fp32
    twiddle in front of the last stage, ONCE missed this at N = 4096 in 232 components: that stage's binary16 operand was 1/16
    of the sequential one and 16356 of its components subnormal; tfft.hip apply_scale_mode, tests/test_stage_model_host.py.)"""
    re, im = bs.impulse_planes(n, "re")
    seq = bs.run(tf, torch, n, re, im)
    once = bs.run(tf, torch, n, re, im, scale="once")
    none = bs.run(tf, torch, n, re, im, scale="none")
    for name, s, o, f in zip(bs.PLANES, seq, once, none):
        assert np.isfinite(f.astype(np.float32)).all()
        bad = int((o.view(np.uint16) != s.view(np.uint16)).sum())
        assert bad == 0, f"once, {name}: {bad} components differ from sequential:\n" + "\n".join(bs.differing((o,), (s,), n, names=(name,)))
        times_n = (s.astype(np.float32) * n).astype(np.float16)                # exact: 1024 / N x N = 1024
        bad = int((f.view(np.uint16) != times_n.view(np.uint16)).sum())
        assert bad == 0, f"none, {name}: {bad} components differ from N x sequential:\n" + "\n".join(bs.differing((f,), (times_n,), n, names=(name,)))


@pytest.mark.parametrize("n", sm.SIZES)
def test_tone_at_every_bin(tf, torch, n):
    re, im = bs.tone_planes(n)
    got_re, got_im = bs.run(tf, torch, n, re, im)
    ref = np.fft.fft(re.astype(np.float64) + 1j * im.astype(np.float64), axis=1) / n
    f = np.arange(n)
    assert (np.argmax(np.abs(ref), axis=1) == f).all()
    worst = eb.check(got_re, got_im, ref.real, ref.imag, K_TONE, what=f"tones, N = {n}")
    mag = np.hypot(got_re.astype(np.float64), got_im.astype(np.float64))
    mag[f, f] = 0.0
    other = mag.max(axis=1) / eb.ulp16(np.abs(ref).max(axis=1))
    print(f"N = {n}: worst tone error {worst:.3f} ulp of the line, largest other bin {other.max():.3f} ulp")
    assert other.max() <= K_TONE, (int(np.argmax(other)), float(other.max()))
