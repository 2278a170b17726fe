"""FFT convolution add-on (include/tfft_conv.h, libtfft_conv.so) on the host: the exported symbols, the planner's description, every
refusal that needs no device, the filter-image map, and the numpy restatement of the pointwise kernel (tests/conv_ref.py) against fp64."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import conv_ref
import elementwise_bound as eb
import tensor_fft_amd as tf
from tensor_fft_amd import conv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 5


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def test_header_library_and_binding_name_the_same_symbols():
    header = open(os.path.join(ROOT, "include", "tfft_conv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                # declarations only: the comments name tfft_* calls too
    declared = set(re.findall(r"\b(tfft_conv_[a-z0-9_]+)\s*\(", code))
    assert declared == set(conv.SYMBOLS), declared ^ set(conv.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", conv.conv_lib_path()], capture_output=True, text=True, check=True).stdout
    text_syms = {line.split()[2] for line in nm.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    # -fvisibility=hidden: nothing but the entry points is exported as code
    assert text_syms == declared, text_syms ^ declared
    lib = conv.load_conv_library()
    for name in declared:
        assert hasattr(lib, name), name


def test_library_holds_a_gfx950_code_object_and_links_the_main_library():
    blob = open(conv.conv_lib_path(), "rb").read()
    assert b"gfx950" in blob and b"conv4096_kernel" in blob and b"cmul_kernel" in blob
    dyn = subprocess.run(["readelf", "-d", conv.conv_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "libtfft.so" in dyn and "$ORIGIN" in dyn


def test_describe_names_the_fused_kernel_at_4096_only():
    assert tf.conv_describe(4096, 65536, 64) == "conv4096:4096"
    assert tf.conv_describe(4096, 1, 1) == "conv4096:4096"
    assert tf.conv_describe(4096, 8, 2, composed=True) == "k4096:4096 | cmul | k4096:4096"
    for n in (256, 2048, 8192, 1 << 16, 1 << 20, 1 << 26):
        fwd, mid, inv = tf.conv_describe(n, 8, 3).split(" | ")
        assert mid == "cmul" and "conv4096" not in fwd + inv, n
        # the two chains are the same transforms; the transposed-input plan runs them rows first
        assert sorted(fwd.split()) == sorted(inv.split()), (fwd, inv)
    # 2^20: the spectrum stays in the transposed order between the plans, 2 + 1 + 2 launches
    fwd, _, inv = tf.conv_describe(1 << 20, 4, 1).split(" | ")
    assert len(fwd.split()) == 2 and len(inv.split()) == 2
    assert fwd.split()[0].startswith("col:") and inv.split()[-1].startswith("col:")
    # from 2^21 on natural order would take three passes each way
    assert len(tf.plan_describe(1 << 22).split()) == 3 and len(tf.conv_describe(1 << 22, 4, 1).split(" | ")[0].split()) == 2


@pytest.mark.parametrize("n,batch,filters,flags,needle", [
    (4095, 8, 1, 0, "power of two"), (3000, 8, 1, 0, "power of two"), (0, 8, 1, 0, "power of two"),
    (128, 8, 1, 0, "256"), (1 << 27, 8, 1, 0, "2^26"),
    (4096, 8, 0, 0, "filters"), (4096, 8, 9, 0, "filters"), (4096, 0, 1, 0, "batch"), (4096, 1 << 32, 1, 0, "batch"),
    (4096, 8, 1, 2, "flag"), (4096, 8, 1, -1, "flag"),
])
def test_describe_and_create_refuse_with_a_message(n, batch, filters, flags, needle):
    lib = conv.load_conv_library()
    buf = ctypes.create_string_buffer(256)
    assert lib.tfft_conv_describe(n, batch, filters, flags, buf, len(buf)) == ERR_ARG
    assert needle in lib.tfft_conv_last_error().decode()
    h = ctypes.c_void_p()
    assert lib.tfft_conv_plan_create(n, batch, filters, 0, 0, 0, flags, ctypes.byref(h)) == ERR_ARG     # before any device call
    assert needle in lib.tfft_conv_last_error().decode() and not h.value


@pytest.mark.parametrize("in_stride,out_stride", [(8188, 0), (8196, 0), (0, 8200 - 4), (4096, 0), (0, 8)])
def test_create_refuses_bad_strides(in_stride, out_stride):
    lib = conv.load_conv_library()
    h = ctypes.c_void_p()
    assert lib.tfft_conv_plan_create(4096, 8, 2, 0, in_stride, out_stride, 0, ctypes.byref(h)) == ERR_ARG
    assert "batch_stride" in lib.tfft_conv_last_error().decode()


def test_null_arguments_are_refused():
    lib = conv.load_conv_library()
    assert lib.tfft_conv_plan_create(4096, 8, 1, 0, 0, 0, 0, None) == ERR_ARG
    assert lib.tfft_conv_describe(4096, 8, 1, 0, None, 0) == ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert lib.tfft_conv_describe(4096, 8, 1, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_conv_exec(None, None, None, None, None, None) == ERR_ARG
    assert lib.tfft_conv_plan_set_filter(None, None, None, None) == ERR_ARG
    assert lib.tfft_conv_plan_num_launches(None) == 0 and lib.tfft_conv_plan_workspace_bytes(None) == 0
    lib.tfft_conv_plan_destroy(None)


def test_no_gpu_means_errors_not_fallbacks():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(tf.TfftError):
        tf.TfftConvPlan(4096, 8, 2, 0)
    with pytest.raises(tf.TfftError):
        tf.TfftConvPlan(1 << 16, 8, 2, 0)


@pytest.mark.parametrize("n,composed", [(4096, False), (4096, True), (256, False), (1 << 16, False), (1 << 20, False), (1 << 21, True)])
def test_filter_slot_is_a_bijection(n, composed):
    lib = conv.load_conv_library()
    flags = conv.CONV_COMPOSED if composed else 0
    slots = np.array([lib.tfft_conv_filter_slot(n, flags, k) for k in range(n)], dtype=np.uint64)
    assert np.array_equal(np.sort(slots), np.arange(n, dtype=np.uint64))
    k = np.arange(n, dtype=np.uint64)
    n2 = tf.transposed_n2(n)
    if n == 4096 and not composed:
        # the fragment a lane of conv4096_kernel owns: k = k0 + 16 k1 + 256 k2
        k0, k1, k2 = k & 15, (k >> 4) & 15, k >> 8
        want = (((k0 >> 3) * 4 + (k2 & 3)) * 64 + 16 * (k2 >> 2) + k1) * 8 + (k0 & 7)
    elif n2:
        n1 = n // n2
        want = (k % n1) * n2 + k // n1                  # slot k1 n2 + k2 holds bin k1 + n1 k2
    else:
        want = k
    assert np.array_equal(slots, want.astype(np.uint64))
    for bad in ((n, flags, n), (n, 2, 0), (100, 0, 0), (128, 0, 0), (1 << 27, 0, 0)):
        assert lib.tfft_conv_filter_slot(*bad) == 2 ** 64 - 1, bad
    with pytest.raises(tf.TfftError):
        tf.conv_filter_slot(n, n, composed)


def test_cmul_restatement_against_fp64():
    """conv_ref.cmul = (x * H * scale) rounded once: within half a binary16 ulp of the fp64 product plus the fp32 rounding in front
    of it (2^-24 relative), for spectra of the size a sequentially scaled transform leaves and filters up to the top of the range."""
    rng = np.random.default_rng(3)
    for n, amp in ((256, 1.0), (4096, 1.0), (1 << 20, 4.0)):
        x_re = (rng.standard_normal((4, 4096)) * 0.6 / np.sqrt(n)).astype(np.float16)
        x_im = (rng.standard_normal((4, 4096)) * 0.6 / np.sqrt(n)).astype(np.float16)
        h_re = (rng.uniform(-1, 1, (4, 4096)) * amp).astype(np.float16)
        h_im = (rng.uniform(-1, 1, (4, 4096)) * amp).astype(np.float16)
        z_re, z_im = conv_ref.cmul(x_re, x_im, h_re, h_im, n)
        z = (x_re.astype(np.float64) + 1j * x_im.astype(np.float64)) * (h_re.astype(np.float64) + 1j * h_im.astype(np.float64)) * n
        assert np.isfinite(z_re.astype(np.float64)).all() and np.abs(z).max() < 32752
        for got, want in ((z_re, z.real), (z_im, z.imag)):
            ulp = eb.ulp16(np.abs(want))               # of the exact value's binade
            assert (np.abs(got.astype(np.float64) - want) <= 0.5 * ulp * (1 + 2.0 ** -12)).all()
    # one filter per channel, b mod filters, is the caller's indexing: the restatement is elementwise
    one = conv_ref.cmul(np.float16([1.5]), np.float16([-2.0]), np.float16([0.5]), np.float16([0.25]), 4)
    assert float(one[0][0]) == 4 * (1.5 * 0.5 + 2.0 * 0.25) and float(one[1][0]) == 4 * (1.5 * 0.25 - 2.0 * 0.5)
    # overflow is not hidden: a product beyond the range contract is inf
    big = conv_ref.cmul(np.float16([60000.0]), np.float16([0.0]), np.float16([2.0]), np.float16([0.0]), 1)
    assert np.isinf(big[0][0])


def test_case_lists_cover_what_the_paths_promise():
    """the shared case list of the GPU tests and tools/conv_accuracy.py: fused at batch 1, 37, 1029 with 1, 3, 8 filters, composed at
    4096 (flag) and at lengths with and without the transposed order"""
    assert {(b, f) for _, b, f, _ in conv_ref.FUSED_CASES} == {(1, 1), (37, 1), (37, 3), (37, 8), (1029, 1), (1029, 3), (1029, 8)}
    assert {n for n, _, _, _ in conv_ref.COMPOSED_CASES} == {4096, 256, 2048, 8192, 1 << 16, 1 << 20}
    assert all(f <= b for _, b, f, _ in conv_ref.CASES)
    rng = np.random.default_rng(0)
    for kind in conv_ref.FILTER_KINDS:
        spec = conv_ref.make_filters(kind, 4096, 3, rng)
        assert spec.shape == (3, 4096) and np.abs(spec).max() <= 1 + 1e-12
        x_re, x_im = conv_ref.signals(4096, 3, rng)
        big = np.abs(np.fft.fft(x_re.astype(np.float64) + 1j * x_im.astype(np.float64), axis=-1) * spec).max()
        assert big < 200, (kind, big)           # far inside the range contract (32752)
    assert len({conv_ref.delay_shift(c, 4096) for c in range(8)}) == 8
