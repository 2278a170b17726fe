"""Overlap-save causal convolution add-on (include/tfft_sconv.h, libtfft_sconv.so) on the host: the exported symbols, the one kernel
and the gfx950 ISA of its code object (tools/isa_lint.py, the rules tests/test_lconv_host.py holds libtfft_lconv.so to), the
geometry and the description, every refusal that needs no device, and the segment indexing in pure numpy against numpy.convolve."""
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
import sconv_ref as sr
import tensor_fft_amd as tf
from tensor_fft_amd import sconv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_ARG = 5


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def test_header_library_and_binding_name_the_same_symbols():
    header = open(os.path.join(ROOT, "include", "tfft_sconv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                # declarations only: the comments name calls too
    declared = set(re.findall(r"\b(tfft_sconv_[a-z0-9_]+)\s*\(", code))
    assert declared == set(sconv.SYMBOLS), declared ^ set(sconv.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", sconv.sconv_lib_path()], capture_output=True, text=True, check=True).stdout
    text_syms = {line.split()[2] for line in nm.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    # -fvisibility=hidden: nothing but the entry points is exported as code
    assert text_syms == declared, text_syms ^ declared
    lib = sconv.load_sconv_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert set(tf.__all__) >= {"TfftLongConvPlan", "long_causal_conv", "sconv_geometry", "sconv_describe", "sconv_cache_clear"}


def test_library_links_the_other_two():
    dyn = subprocess.run(["readelf", "-d", sconv.sconv_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "libtfft_conv.so" in dyn and "libtfft.so" in dyn and "$ORIGIN" in dyn
    assert "libtfft_lconv.so" not in dyn and "libtfft_gconv.so" not in dyn
    assert ctypes.sizeof(sconv.SconvOpts) == 32                       # tfft_sconv_opts as the header lays it out


@pytest.fixture(scope="module")
def report():
    import isa_lint

    return isa_lint.lint_text(isa_lint.disassemble(sconv.sconv_lib_path()))


def test_code_object_holds_exactly_the_one_kernel(report):
    assert len(report) == 1, list(report)
    names = subprocess.run(["c++filt"], input="\n".join(report), capture_output=True, text=True, check=True).stdout.split("\n")
    assert {n.strip().split("(")[0] for n in names if n.strip()} == {"sconv4096::sconv4096_kernel"}
    kernel = next(iter(report.values()))
    # two transforms of 16 stage-1 tiles and 16 stage-2/3 tiles, two MFMAs per complex product: conv4096_kernel's count
    assert kernel["mfma"] == 2 * (16 * 2 + 16 * 4) == 192
    # one LDS-DMA per 1-KiB block and plane
    assert kernel["lds_dma"] == 16


def test_no_packed_fp32_wait_states_and_dma_drain(report):
    kernel = next(iter(report.values()))
    assert kernel["pk_f32"] == 0
    assert not kernel["findings"], kernel["findings"]


def test_kernel_resources():
    """no scratch, no spills and at most 256 VGPRs (the bounds of tests/test_conv_isa.py), from the kernel metadata notes"""
    import isa_lint

    tmp = tempfile.mkdtemp(prefix="tfft_sconv_isa_")
    try:
        local = os.path.join(tmp, "libtfft_sconv.so")
        shutil.copy(sconv.sconv_lib_path(), local)
        subprocess.check_call([os.path.join(isa_lint.LLVM_BIN, "llvm-objdump"), "--offloading", local], cwd=tmp,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f][0]
        notes = subprocess.check_output([os.path.join(isa_lint.LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(tmp, co)], text=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    blocks = [b for b in notes.split("- .agpr_count") if "sconv4096_kernel" in b]
    assert len(blocks) == 1
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", blocks[0]).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blocks[0]).group(1))
    spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blocks[0]).group(1))
    sgpr_spills = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blocks[0]).group(1))
    print(f"sconv4096_kernel: {vgprs} VGPRs, scratch {scratch}, spills {spills} / {sgpr_spills}")
    assert scratch == 0 and spills == 0 and sgpr_spills == 0 and vgprs <= 256, (vgprs, scratch, spills, sgpr_spills)


GEOMETRY = [  # (L, K, halo, hop, segments)
    (8, 1, 0, 4096, 1), (4096, 1, 0, 4096, 1), (4104, 1, 0, 4096, 2), (8192, 1, 0, 4096, 2),          # K = 1: no halo; L = hop, hop + 8, 2 hop
    (4032, 2, 64, 4032, 1), (4040, 2, 64, 4032, 2), (8064, 2, 64, 4032, 2),                            # K = 2: one sample of history costs 64
    (4032, 65, 64, 4032, 1), (4040, 65, 64, 4032, 2), (8064, 65, 64, 4032, 2),
    (3968, 66, 128, 3968, 1), (3976, 66, 128, 3968, 2), (7936, 66, 128, 3968, 2),
    (2048, 2049, 2048, 2048, 1), (2056, 2049, 2048, 2048, 2), (4096, 2049, 2048, 2048, 2), (16384, 2049, 2048, 2048, 8),
    (6152, 130, 192, 3904, 2), (1 << 26, 2049, 2048, 2048, 1 << 15),
]


@pytest.mark.parametrize("length,taps,halo,hop,segments", GEOMETRY)
def test_geometry_and_describe(length, taps, halo, hop, segments):
    assert tf.sconv_geometry(length, taps) == (halo, hop, segments) == sr.geometry(length, taps)
    assert halo % 64 == 0 and halo >= taps - 1 and halo - 64 < taps - 1 and hop + halo == 4096 and 2048 <= hop <= 4096
    assert tf.sconv_describe(length, taps, 3, 2) == f"sconv4096:4096 x {segments}"
    # each pointer of tfft_sconv_geometry may be NULL
    lib = sconv.load_sconv_library()
    one = ctypes.c_uint64()
    assert lib.tfft_sconv_geometry(length, taps, None, None, ctypes.byref(one)) == 0 and one.value == segments
    assert lib.tfft_sconv_geometry(length, taps, None, None, None) == 0


def test_cases_cover_what_they_say():
    geo = {c[:2]: sr.geometry(c[0], c[1]) for c in sr.CASES}
    assert geo[(8, 1)] == (0, 4096, 1) and geo[(2056, 1)] == (0, 4096, 1) and geo[(2048, 2049)] == (2048, 2048, 1)
    assert geo[(4104, 7)] == (64, 4032, 2) and (4104 - 4032) // 8 == 9
    assert geo[(4096, 2049)] == (2048, 2048, 2) and geo[(8064, 65)] == (64, 4032, 2) and geo[(6152, 130)] == (192, 3904, 2)
    assert geo[(8192, 2049)][2] == 4 and geo[(12288, 65)][2] == 4
    # the causal plans do not fuse these lengths (all but the first and the third, which pin the single-segment ends)
    assert tf.lconv_describe(2056, 1, 2, 2).startswith("pack |")


def _opts(**kw):
    o = sconv.SconvOpts(ctypes.sizeof(sconv.SconvOpts), 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("rows,channels,length,taps,flags,needle", [
    (1, 1, 0, 1, 0, "multiple of 8"), (1, 1, 4, 1, 0, "multiple of 8"), (1, 1, 4100, 1, 0, "multiple of 8"),
    (1, 1, 8, 0, 0, "taps must be at least 1"), (1, 1, 8, 2050, 0, "tfft_lconv_plan_create"), (1, 1, 16384, 1 << 20, 0, "tfft_lconv_plan_create"),
    (0, 1, 8, 1, 0, "rows"), (1 << 32, 1, 8, 1, 0, "rows"), (1, 0, 8, 1, 0, "channels"),
    (1 << 16, 1 << 16, 8, 1, 0, "rows * channels"), (1, 1, 8, 1, 1, "flag"), (1, 1, 8, 1, -1, "flag"),
    (1, 1, (1 << 26) + 8, 2, 0, "2^26"), (1 << 20, 1 << 10, 1 << 20, 2049, 0, "item count"),
])
def test_describe_and_create_refuse_with_a_message(rows, channels, length, taps, flags, needle):
    lib = sconv.load_sconv_library()
    buf = ctypes.create_string_buffer(256)
    assert lib.tfft_sconv_describe(length, taps, rows, channels, flags, buf, len(buf)) == ERR_ARG
    assert needle in lib.tfft_sconv_last_error().decode()
    h = ctypes.c_void_p()
    o = _opts(flags=flags)
    assert lib.tfft_sconv_plan_create(rows, channels, length, taps, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG    # before any device call
    assert needle in lib.tfft_sconv_last_error().decode() and not h.value


@pytest.mark.parametrize("length,taps,needle", [(0, 1, "multiple of 8"), (12, 1, "multiple of 8"), (8, 0, "taps"), (8, 2050, "tfft_lconv_plan_create"),
                                                ((1 << 26) + 8, 1, "2^26")])
def test_geometry_refuses_what_create_refuses(length, taps, needle):
    lib = sconv.load_sconv_library()
    halo = ctypes.c_uint64(77)
    assert lib.tfft_sconv_geometry(length, taps, ctypes.byref(halo), None, None) == ERR_ARG and halo.value == 77
    assert needle in lib.tfft_sconv_last_error().decode()
    with pytest.raises(tf.TfftError):
        tf.sconv_geometry(length, taps)


@pytest.mark.parametrize("kw,needle", [
    (dict(in_seq_stride=8184), "in_seq_stride"), (dict(in_seq_stride=8196), "in_seq_stride"), (dict(out_seq_stride=8), "out_seq_stride"),
    (dict(out_seq_stride=8193), "out_seq_stride"), (dict(struct_size=0), "struct_size"), (dict(struct_size=24), "struct_size"),
    (dict(struct_size=40), "struct_size"), (dict(reserved_=1), "reserved_"), (dict(launch_iters=65536), "launch_iters"),
    (dict(flags=1), "flags must be 0"), (dict(flags=1 << 30), "flags must be 0"),
])
def test_create_refuses_bad_options(kw, needle):
    lib = sconv.load_sconv_library()
    h = ctypes.c_void_p()
    o = _opts(**kw)
    assert lib.tfft_sconv_plan_create(4, 2, 8192, 64, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG
    assert needle in lib.tfft_sconv_last_error().decode() and not h.value


def test_null_arguments_are_refused():
    lib = sconv.load_sconv_library()
    assert lib.tfft_sconv_plan_create(1, 1, 8, 1, 0, None, None) == ERR_ARG
    assert lib.tfft_sconv_describe(8, 1, 1, 1, 0, None, 0) == ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert lib.tfft_sconv_describe(8, 1, 1, 1, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_sconv_exec(None, None, None, None) == ERR_ARG
    assert lib.tfft_sconv_plan_set_taps(None, None, None) == ERR_ARG
    assert lib.tfft_sconv_plan_spectrum(None, None, None) == ERR_ARG
    assert lib.tfft_sconv_plan_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_sconv_plan_num_launches(None) == 0
    lib.tfft_sconv_plan_destroy(None)
    assert lib.tfft_sconv_last_error().decode()


def test_no_gpu_means_errors_not_fallbacks():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(tf.TfftError):
        tf.TfftLongConvPlan(4, 2, 16384, 2049, 0)
    with pytest.raises(tf.TfftError):
        tf.TfftLongConvPlan(1, 1, 8, 1, 0)
    with pytest.raises(tf.TfftError):
        tf.long_causal_conv(torch.zeros((2, 2, 4096), dtype=torch.float16), torch.zeros((2, 7), dtype=torch.float16))


@pytest.mark.parametrize("length,taps", sr.INDEX_CASES + [c[:2] for c in sr.CASES if c[:2] not in sr.INDEX_CASES])
def test_segment_indexing_against_numpy_convolve(length, taps):
    """pure numpy: windows -> circular convolution of every window in fp64 -> the samples behind the halo, joined = the linear causal
    convolution; rows 3 (odd: a zero partner) x channels 2"""
    rows, channels = 3, 2
    rng = np.random.default_rng([length, taps])
    x = rng.uniform(-1, 1, (rows, channels, length))
    h = rng.standard_normal((channels, taps))
    h /= np.abs(h).sum(axis=1, keepdims=True)
    re, im = sr.windows(x, taps)
    halo, hop, segs = sr.geometry(length, taps)
    assert re.shape == im.shape == (sr.items_of(rows, channels, length, taps), 4096) == (2 * segs * channels, 4096)
    assert not im[segs * channels:].any()                                  # the zero partner of row 2
    assert not re[:channels, :halo].any()                                  # in front of sample 0
    # windows / unwindow are inverse to each other on the kept samples
    assert np.array_equal(sr.unwindow(re, im, rows, channels, length, taps), x)
    y = np.fft.ifft(np.fft.fft(re + 1j * im, axis=-1) * np.fft.fft(h, 4096, axis=-1)[np.arange(re.shape[0]) % channels], axis=-1)
    got = sr.unwindow(y.real, y.imag, rows, channels, length, taps)
    for b in range(rows):
        for c in range(channels):
            assert np.abs(got[b, c] - np.convolve(x[b, c], h[c])[:length]).max() <= 1e-13, (b, c)
    # kept(): zero beyond sample L of the last segment, the kept samples elsewhere
    k = sr.kept(y.real, rows, channels, length, taps).reshape(2, segs, channels, hop)
    tail = length - (segs - 1) * hop
    assert not k[:, -1, :, tail:].any() and np.array_equal(k[0, -1, 0, :tail], y.real.reshape(2, segs, channels, 4096)[0, -1, 0, halo:halo + tail])


def test_spectrum_rounding_stays_inside_the_allowance():
    """What tests/test_gpu_sconv.py grants the comparison with the true linear convolution on top of K_SCONV, + 1 ulp and + 2^-11 of
    rel-L2, is what the binary16 rounding of H may move the kept samples by. On the CPU, for the test data (the spectrum is
    tfft_lconv_spectrum_host's at n = 4096, which the GPU test holds the plan's to): fp64 with that spectrum against fp64 with the
    taps, in ulps of each window's peak. Also the range contract: max |X H| far inside 32752."""
    worst, worst_rel, big = 0.0, 0.0, 0.0
    for length, taps, rows, channels, _ in sr.CASES:
        for kind in lr.TAP_KINDS:
            x, h = lr.case_data(length, taps, rows, channels, kind, 1)
            assert np.abs(h.astype(np.float64)).sum(axis=1).max() <= 1.0 + 2.0 ** -9
            spec = [tf.lconv_spectrum_host(h[c], 4096) for c in range(channels)]
            h_re, h_im = np.stack([s[0] for s in spec]), np.stack([s[1] for s in spec])
            true = sr.reference_taps(x, h)
            ref = sr.reference_spectrum(x, taps, h_re, h_im)
            re, im = sr.windows(x.astype(np.float64), taps)
            big = max(big, np.abs(np.fft.fft(re + 1j * im, axis=-1) * (h_re.astype(np.float64) + 1j * h_im)[np.arange(re.shape[0]) % channels]).max())
            a, b = sr.kept(true, rows, channels, length, taps), sr.kept(ref, rows, channels, length, taps)
            unit = 2.0 ** (np.floor(np.log2(np.maximum(sr.window_peak(true), 2.0 ** -14))) - 10)
            worst = max(worst, (np.maximum(np.abs((a - b).real), np.abs((a - b).imag)) / unit[:, None]).max())
            den = np.sqrt((np.abs(a) ** 2).sum(-1))
            worst_rel = max(worst_rel, (np.sqrt((np.abs(a - b) ** 2).sum(-1))[den > 0] / den[den > 0]).max())
    print(f"rounding of H alone: {worst:.3f} ulp of the window's peak, rel-L2 {worst_rel:.2e}; max |X H| = {big:.1f}")
    assert worst <= 1.0 and worst_rel <= 2.0 ** -11 and big <= 32752 / 32
