"""Causal real convolution add-on (include/tfft_lconv.h, libtfft_lconv.so) on the host: the exported symbols, the kernels and the
gfx950 ISA of its code object (tools/isa_lint.py, the rules tests/test_conv_isa.py holds libtfft_conv.so to), the transform length,
the planner's description, every refusal that needs no device, and the host spectrum against numpy."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import lconv_ref as lr
import tensor_fft_amd as tf
from tensor_fft_amd import lconv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_ARG = 5


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def test_header_library_and_binding_name_the_same_symbols():
    header = open(os.path.join(ROOT, "include", "tfft_lconv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                # declarations only: the comments name calls too
    declared = set(re.findall(r"\b(tfft_lconv_[a-z0-9_]+)\s*\(", code))
    assert declared == set(lconv.SYMBOLS), declared ^ set(lconv.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", lconv.lconv_lib_path()], capture_output=True, text=True, check=True).stdout
    text_syms = {line.split()[2] for line in nm.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    # -fvisibility=hidden: nothing but the entry points is exported as code
    assert text_syms == declared, text_syms ^ declared
    lib = lconv.load_lconv_library()
    for name in declared:
        assert hasattr(lib, name), name


def test_library_links_the_other_two():
    dyn = subprocess.run(["readelf", "-d", lconv.lconv_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "libtfft_conv.so" in dyn and "libtfft.so" in dyn and "$ORIGIN" in dyn
    assert ctypes.sizeof(lconv.LconvOpts) == 32                       # tfft_lconv_opts as the header lays it out


@pytest.fixture(scope="module")
def report():
    import isa_lint

    return isa_lint.lint_text(isa_lint.disassemble(lconv.lconv_lib_path()))


def _one(report, needle):
    names = [k for k in report if needle in k]
    assert len(names) == 1, names
    return report[names[0]]


def test_code_object_holds_exactly_the_three_kernels(report):
    assert len(report) == 3, list(report)
    names = subprocess.run(["c++filt"], input="\n".join(report), capture_output=True, text=True, check=True).stdout.split("\n")
    assert {n.strip().split("(")[0] for n in names if n.strip()} == {"lconv4096::lconv4096_kernel", "lconv_copy::pack_kernel",
                                                                     "lconv_copy::crop_kernel"}
    fused, pack, crop = _one(report, "lconv4096_kernel"), _one(report, "pack_kernel"), _one(report, "crop_kernel")
    # two transforms of 16 stage-1 tiles and 16 stage-2/3 tiles, two MFMAs per complex product: conv4096_kernel's count
    assert fused["mfma"] == 2 * (16 * 2 + 16 * 4) == 192
    # one LDS-DMA per 1-KiB block and plane
    assert fused["lds_dma"] == 16
    for k in (pack, crop):
        assert k["mfma"] == 0 and not k["lds_dma"]


def test_no_packed_fp32_wait_states_and_dma_drain(report):
    fused = _one(report, "lconv4096_kernel")
    assert fused["pk_f32"] == 0
    assert not fused["findings"], fused["findings"]
    assert not _one(report, "pack_kernel")["findings"] and not _one(report, "crop_kernel")["findings"]


def test_fused_kernel_resources():
    """no scratch, no spills and at most 256 VGPRs (the bounds of tests/test_conv_isa.py), from the kernel metadata notes"""
    import isa_lint

    tmp = tempfile.mkdtemp(prefix="tfft_lconv_isa_")
    try:
        local = os.path.join(tmp, "libtfft_lconv.so")
        shutil.copy(lconv.lconv_lib_path(), local)
        subprocess.check_call([os.path.join(isa_lint.LLVM_BIN, "llvm-objdump"), "--offloading", local], cwd=tmp,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f][0]
        notes = subprocess.check_output([os.path.join(isa_lint.LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(tmp, co)], text=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    blocks = [b for b in notes.split("- .agpr_count") if "lconv4096_kernel" in b]
    assert len(blocks) == 1
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", blocks[0]).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blocks[0]).group(1))
    spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blocks[0]).group(1))
    sgpr_spills = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blocks[0]).group(1))
    assert scratch == 0 and spills == 0 and sgpr_spills == 0 and vgprs <= 256, (vgprs, scratch, spills, sgpr_spills)


def test_fft_length():
    for length, taps, n in ((8, 1, 256), (96, 33, 256), (128, 129, 256), (128, 130, 512), (2048, 2049, 4096), (2040, 2057, 4096),
                            (2048, 2050, 8192), (2056, 1, 4096), (4096, 1, 4096), (40000, 20000, 1 << 16), (1 << 25, (1 << 25) + 1, 1 << 26)):
        assert tf.lconv_fft_length(length, taps) == n == lr.fft_length(length, taps), (length, taps)
    for length, taps in ((0, 1), (8, 0), (1 << 26, 2), (1 << 27, 1), (8, 1 << 27)):
        assert tf.lconv_fft_length(length, taps) == 0, (length, taps)
    # the fused kernel takes L <= 2048 with L + K - 1 <= 4096 at n = 4096, whatever the shortest length would be
    assert all(lr.plan_length(c[0], c[1]) == 4096 for c in lr.FUSED_CASES)
    assert all(lr.plan_length(c[1], c[2], c[5]) == c[0] == lr.fft_length(c[1], c[2]) for c in lr.COMPOSED_CASES)
    assert lr.plan_length(2056, 1) == 4096 == lr.fft_length(2056, 1) and lr.plan_length(8, 1, True) == 256


def test_describe():
    assert tf.lconv_describe(2048, 2049, 131072, 1) == "lconv4096:4096"
    for length, taps in ((8, 1), (520, 7), (1024, 1025), (2040, 2057), (8, 4089), (2048, 1)):
        assert tf.lconv_describe(length, taps, 3, 2) == "lconv4096:4096", (length, taps)
    assert tf.lconv_describe(2048, 2049, 3, 3, composed=True) == "pack | conv4096:4096 | crop"
    # beyond the fused kernel's shapes, and with the flag: the sub-plan of the shortest transform length between the two copies
    for length, taps, rows, channels, composed in ((96, 33, 5, 4, True), (1000, 500, 3, 2, True), (2056, 1, 2, 2, False), (8, 4090, 1, 1, False),
                                                   (4096, 4097, 3, 2, False), (40000, 20000, 3, 2, False)):
        n = lr.fft_length(length, taps)
        sub = tf.conv_describe(n, (rows + 1) // 2 * channels, channels)
        assert tf.lconv_describe(length, taps, rows, channels, composed=composed) == f"pack | {sub} | crop"
    assert tf.lconv_describe(2056, 1, 2, 2) == "pack | conv4096:4096 | crop"


def _opts(**kw):
    o = lconv.LconvOpts(ctypes.sizeof(lconv.LconvOpts), 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("rows,channels,length,taps,flags,needle", [
    (1, 1, 0, 1, 0, "multiple of 8"), (1, 1, 4, 1, 0, "multiple of 8"), (1, 1, 2044, 1, 0, "multiple of 8"),
    (1, 1, 8, 0, 0, "taps"), (0, 1, 8, 1, 0, "rows"), (1 << 32, 1, 8, 1, 0, "rows"), (1, 0, 8, 1, 0, "channels"),
    (1 << 16, 1 << 16, 8, 1, 0, "rows * channels"), (1, 1, 8, 1, 2, "flag"), (1, 1, 8, 1, -1, "flag"),
    (1, 1, 1 << 26, 2, 0, "2^26"), (1, 1, 8, (1 << 26) + 1, 0, "2^26"),
])
def test_describe_and_create_refuse_with_a_message(rows, channels, length, taps, flags, needle):
    lib = lconv.load_lconv_library()
    buf = ctypes.create_string_buffer(256)
    assert lib.tfft_lconv_describe(length, taps, rows, channels, flags, buf, len(buf)) == ERR_ARG
    assert needle in lib.tfft_lconv_last_error().decode()
    h = ctypes.c_void_p()
    o = _opts(flags=flags)
    assert lib.tfft_lconv_plan_create(rows, channels, length, taps, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG    # before any device call
    assert needle in lib.tfft_lconv_last_error().decode() and not h.value


@pytest.mark.parametrize("kw,needle", [
    (dict(in_seq_stride=2040), "in_seq_stride"), (dict(in_seq_stride=2052), "in_seq_stride"), (dict(out_seq_stride=8), "out_seq_stride"),
    (dict(out_seq_stride=2049), "out_seq_stride"), (dict(struct_size=0), "struct_size"), (dict(struct_size=24), "struct_size"),
    (dict(struct_size=40), "struct_size"), (dict(reserved_=1), "reserved_"), (dict(launch_iters=65536), "launch_iters"),
])
def test_create_refuses_bad_options(kw, needle):
    lib = lconv.load_lconv_library()
    h = ctypes.c_void_p()
    o = _opts(**kw)
    assert lib.tfft_lconv_plan_create(4, 2, 2048, 64, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG
    assert needle in lib.tfft_lconv_last_error().decode() and not h.value


def test_null_arguments_are_refused():
    lib = lconv.load_lconv_library()
    assert lib.tfft_lconv_plan_create(1, 1, 8, 1, 0, None, None) == ERR_ARG
    assert lib.tfft_lconv_describe(8, 1, 1, 1, 0, None, 0) == ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert lib.tfft_lconv_describe(8, 1, 1, 1, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_lconv_exec(None, None, None, None) == ERR_ARG
    assert lib.tfft_lconv_plan_set_taps(None, None, None) == ERR_ARG
    assert lib.tfft_lconv_plan_spectrum(None, None, None) == ERR_ARG
    assert lib.tfft_lconv_plan_prepare(None) == ERR_ARG and lib.tfft_lconv_plan_set_workspace(None, None, 0) == ERR_ARG
    assert lib.tfft_lconv_plan_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_lconv_plan_num_launches(None) == 0 and lib.tfft_lconv_plan_workspace_bytes(None) == 0
    lib.tfft_lconv_plan_destroy(None)
    one = np.ones(1, np.float16)
    out = np.empty(8, np.float16)
    for args in ((None, 1, 8, out.ctypes.data, out.ctypes.data), (one.ctypes.data, 1, 8, None, out.ctypes.data),
                 (one.ctypes.data, 0, 8, out.ctypes.data, out.ctypes.data), (one.ctypes.data, 9, 8, out.ctypes.data, out.ctypes.data),
                 (one.ctypes.data, 1, 12, out.ctypes.data, out.ctypes.data), (one.ctypes.data, 1, 1 << 27, out.ctypes.data, out.ctypes.data)):
        assert lib.tfft_lconv_spectrum_host(*args) == ERR_ARG, args


def test_no_gpu_means_errors_not_fallbacks():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(tf.TfftError):
        tf.TfftCausalConvPlan(4, 2, 2048, 64, 0)
    with pytest.raises(tf.TfftError):
        tf.TfftCausalConvPlan(4, 2, 4096, 64, 0)
    assert lconv.load_lconv_library().tfft_lconv_plan_fft_length(None) == 0


def _ulp_of(v):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14))) - 10)


@pytest.mark.parametrize("taps,n", [(1, 4096), (7, 4096), (2049, 4096), (20000, 1 << 16)])
@pytest.mark.parametrize("kind", ["decay", "noise", "delay"])
def test_spectrum_host_against_numpy(taps, n, kind):
    rng = np.random.default_rng([taps, n])
    h = lr.make_taps(kind, 2, taps, rng)[1]
    re, im = tf.lconv_spectrum_host(h, n)
    ref = np.fft.fft(h.astype(np.float64), n)
    assert (np.abs(re.astype(np.float64) - ref.real) <= _ulp_of(ref.real)).all()
    assert (np.abs(im.astype(np.float64) - ref.imag) <= _ulp_of(ref.imag)).all()
    # exactly Hermitian, as bit patterns up to the sign of zero, and real where a real signal's spectrum is real
    assert np.array_equal(re[1:], re[:0:-1]) and np.array_equal(im[1:], -im[:0:-1])
    assert im.view(np.uint16)[0] == 0 and im.view(np.uint16)[n // 2] == 0


def test_tap_kinds_stay_inside_the_range_contract():
    """the shared inputs of the GPU tests and tools/lconv_accuracy.py: sum |h| <= 1 up to the rounding of the taps, so |y| <= 1 per
    row, and max |X H| far inside 32752"""
    assert len({lr.delay_shift(c, 2049) for c in range(8)}) == 8
    for length, taps, rows, channels, _ in lr.FUSED_CASES:
        for kind in lr.TAP_KINDS:
            x, h = lr.case_data(length, taps, rows, channels, kind, 1)
            assert x.shape == (rows, channels, length) and h.shape == (channels, taps)
            assert np.abs(h.astype(np.float64)).sum(axis=1).max() <= 1.0 + 2.0 ** -9
            re, im = lr.pair_planes(x.astype(np.float64), 4096)
            spec = np.fft.fft(h.astype(np.float64), 4096, axis=-1)
            big = np.abs(np.fft.fft(re + 1j * im, axis=-1) * spec[np.arange(re.shape[0]) % channels]).max()
            assert big <= 200, (length, taps, kind, big)
    # pair_planes / unpair are inverse to each other on the kept samples, odd row counts included
    x = lr.signals(5, 3, 16, np.random.default_rng(0))
    re, im = lr.pair_planes(x, 64)
    assert re.shape == (9, 64) and not im[6:].any() and not re[:, 16:].any()
    assert np.array_equal(lr.unpair(re, im, 5, 3, 16), x)
