"""Real-input plans (tfft_rplan_*) on the host: the default half-spectrum pitch, the planner's description, every refusal of
tfft_rplan_create that needs no device, and the numpy restatement of the split / merge arithmetic that the GPU tests compare the
kernels with (tests/rfft_ref.py)."""
import ctypes

import numpy as np
import pytest

import rfft_ref
import tensor_fft_amd as tf
from tensor_fft_amd import capi


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def test_spectrum_pitch_is_the_aligned_half_length():
    for lg in range(4, 31):
        n = 1 << lg
        h = tf.rplan_spectrum_pitch(n)
        assert h % 8 == 0 and n // 2 + 1 <= h < n // 2 + 9, (n, h)
        assert h == n // 2 + 8
    assert tf.rplan_spectrum_pitch(4096) == 2056
    for bad in (0, 1, 2, 8, 15, 24, 4095):
        assert tf.rplan_spectrum_pitch(bad) == 0, bad


def test_describe_names_the_fused_kernel_at_4096_only():
    assert tf.rplan_describe(4096, 131072) == "r2c: k4096:4096+split | c2r: merge k4096:4096"
    assert tf.rplan_describe(4096, 1).startswith("r2c: k4096:4096+split")
    two = tf.rplan_describe(4096, 131072, two_pass=True)
    assert two.startswith("r2c: k4096:4096 split") and "+split" not in two
    for n in (16, 256, 1024, 8192, 1 << 16, 1 << 20):
        d = tf.rplan_describe(n, 8)
        assert d.startswith("r2c: ") and " split | c2r: merge " in d and "+split" not in d, (n, d)
    assert tf.rplan_describe(1 << 20, 65).split(" | ")[0].split(": ")[1].startswith("col:")


def _create(n=4096, batch=4, flags=0, **fields):
    """tfft_rplan_create with a hand-filled tfft_plan_opts; returns (rc, message). Refusals come back before any device call."""
    L = capi.load_library()
    o = capi.PlanOpts()
    o.struct_size = ctypes.sizeof(capi.PlanOpts)
    for k, v in fields.items():
        setattr(o, k, v)
    h = ctypes.c_void_p()
    rc = L.tfft_rplan_create(int(n), int(batch), 0, ctypes.byref(o), int(flags), ctypes.byref(h))
    if rc == 0:
        L.tfft_rplan_destroy(h)
    return rc, capi.last_error()


@pytest.mark.parametrize("args, code", [
    (dict(n=8), 2), (dict(n=2), 2), (dict(n=4095), 1), (dict(n=3000), 1), (dict(n=1 << 31), 5),
    (dict(batch=0), 5), (dict(batch=1 << 32), 5),
    (dict(inner=8), 5), (dict(inner=64), 5),
    (dict(output_order=1), 5), (dict(input_order=1), 5),
    (dict(fourstep_n=1 << 16), 5), (dict(fourstep_col0=3), 5),
    (dict(variant=capi.VARIANT_K4096_STAGE_OUT), 5), (dict(variant=capi.VARIANT_AUTOSORT_ONLY), 5),
    (dict(variant=capi.VARIANT_K4096_PLAIN), 5),
    (dict(in_batch_stride=4088), 5), (dict(in_batch_stride=4100), 5),
    (dict(out_batch_stride=2048), 5), (dict(out_batch_stride=2052), 5), (dict(n=16, out_batch_stride=4), 5),
    (dict(preserve_input=1), 5), (dict(scale=3), 5), (dict(launch_iters=65536), 5), (dict(reserved_=1), 5),
    (dict(flags=2), 5), (dict(flags=-1), 5),
])
def test_create_refuses_bad_arguments_without_a_device(args, code):
    rc, msg = _create(**args)
    assert rc == code, (args, rc, msg)
    assert msg


def test_create_refuses_unknown_struct_size():
    L = capi.load_library()
    o = capi.PlanOpts()
    o.struct_size = 80
    h = ctypes.c_void_p()
    assert L.tfft_rplan_create(4096, 2, 0, ctypes.byref(o), 0, ctypes.byref(h)) == 5
    assert L.tfft_rplan_create(4096, 2, 0, None, 0, None) == 5


def test_describe_keeps_the_fused_kernel_under_plan_wisdom():
    """Wisdom for n = 4096 (AUTOSORT_ONLY at batch 0: every batch gets the plain autosort chain) changes the complex plans, the C2R
    chain with them, but not the forward transform of a real plan, which the fused launch and the two-pass path pin to the N = 4096
    kernel."""
    tf.tuning_clear()
    tf.tuning_add(4096, 0, capi.VARIANT_AUTOSORT_ONLY, 0)
    try:
        assert tf.plan_describe(4096, 1, tf.plan_default_variant(4096, 1, 65536)).startswith("autosort")
        fused = tf.rplan_describe(4096, 131072)
        two = tf.rplan_describe(4096, 131072, two_pass=True)
    finally:
        tf.tuning_clear()
    assert fused.startswith("r2c: k4096:4096+split | c2r: merge autosort"), fused
    assert two.startswith("r2c: k4096:4096 split | c2r: merge autosort"), two
    assert tf.rplan_describe(4096, 131072) == "r2c: k4096:4096+split | c2r: merge k4096:4096"


def test_convenience_functions_refuse_cpu_tensors():
    import torch

    with pytest.raises(tf.TfftError):
        tf.rfft(torch.zeros(2, 64, dtype=torch.float16))
    with pytest.raises(tf.TfftError):
        tf.irfft(torch.zeros(2, 33, dtype=torch.float16), torch.zeros(2, 33, dtype=torch.float16), 64)
    with pytest.raises(tf.TfftError):
        tf.irfft([0.0], [0.0], 64)


def test_describe_refuses_what_create_refuses():
    buf = ctypes.create_string_buffer(256)
    L = capi.load_library()
    assert L.tfft_rplan_describe(8, 1, 0, buf, len(buf)) == 2
    assert L.tfft_rplan_describe(4096, 0, 0, buf, len(buf)) == 5
    assert L.tfft_rplan_describe(4096, 1, 4, buf, len(buf)) == 5
    assert L.tfft_rplan_describe(4096, 1, 0, buf, 8) == 5


def _exact_z(rng, shape):
    """fp16 values k / 64 with |k| <= 512: every sum of two is exact in fp16 after the halving, so merge(split(Z)) must return Z."""
    return (rng.integers(-512, 513, shape) / 64.0).astype(np.float16)


@pytest.mark.parametrize("n", [16, 32, 256, 4096, 1 << 14])
def test_merge_undoes_split_bit_for_bit(n):
    rng = np.random.default_rng(n)
    zr, zi = _exact_z(rng, (5, n)), _exact_z(rng, (5, n))
    ar, ai, br, bi = rfft_ref.split(zr, zi)
    assert ar.dtype == np.float16 and ar.shape == (5, n // 2 + 1)
    assert not ai[:, 0].any() and not bi[:, 0].any() and not ai[:, n // 2].any() and not bi[:, n // 2].any()
    mr, mi = rfft_ref.merge(ar, ai, br, bi, n)
    assert np.array_equal(mr.view(np.uint16), zr.view(np.uint16))
    assert np.array_equal(mi.view(np.uint16), zi.view(np.uint16))


def test_merge_ignores_the_imaginary_part_of_bins_0_and_nyquist():
    n = 64
    rng = np.random.default_rng(1)
    ar, ai, br, bi = (rng.standard_normal((3, n // 2 + 1)).astype(np.float16) for _ in range(4))
    z0 = rfft_ref.merge(ar, ai, br, bi, n)
    for plane in (ai, bi):
        plane[:, 0] = np.float16(7.5)
        plane[:, n // 2] = np.float16(-3.25)
    z1 = rfft_ref.merge(ar, ai, br, bi, n)
    for a, b in zip(z0, z1):
        assert np.array_equal(a.view(np.uint16), b.view(np.uint16))


@pytest.mark.parametrize("n", [16, 256, 4096])
def test_split_and_merge_are_the_rfft_algebra_in_float64(n):
    rng = np.random.default_rng(n + 1)
    a, b = rng.standard_normal((2, 7, n))
    z = np.fft.fft(a + 1j * b, axis=-1)
    ar, ai, br, bi = rfft_ref.split(z.real, z.imag, dtype=np.float64, to16=False)
    fa, fb = np.fft.rfft(a, axis=-1), np.fft.rfft(b, axis=-1)
    scale = np.abs(z).max()
    assert np.abs(ar + 1j * ai - fa).max() < 1e-12 * scale
    assert np.abs(br + 1j * bi - fb).max() < 1e-12 * scale
    zr, zi = rfft_ref.merge(fa.real, fa.imag, fb.real, fb.imag, n, dtype=np.float64, to16=False)
    assert np.abs(zr + 1j * zi - z).max() < 1e-12 * scale
    # C2R convention: irfft drops the IM of bins 0 and N/2, so does merge
    x = np.fft.ifft(zr + 1j * zi, axis=-1)
    assert np.allclose(x.real, np.fft.irfft(fa, n, axis=-1), atol=1e-12) and np.allclose(x.imag, np.fft.irfft(fb, n, axis=-1), atol=1e-12)


def test_pairing_of_an_odd_batch():
    a, b = rfft_ref.pair_rows(5)
    assert list(a) == [0, 2, 4] and list(b) == [1, 3, 4]
    a, b = rfft_ref.pair_rows(1)
    assert list(a) == [0] and list(b) == [0]
