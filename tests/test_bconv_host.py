"""Gradient add-on of the overlap-save causal convolution (include/tfft_bconv.h, libtfft_bconv.so) on the host: the exported symbols,
the three kernels and the gfx950 ISA of the code object (tools/isa_lint.py, the rules tests/test_sconv_host.py holds libtfft_sconv.so
to), the geometry with the partial sums P, every refusal that needs no device, the two window identities in pure numpy against
direct fp64 sums, and the numbers the bound of the tap gradient rests on (tests/bconv_ref.py)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import bconv_ref as br
import lconv_ref as lr
import sconv_ref as sr
import tensor_fft_amd as tf
from tensor_fft_amd import bconv
from test_sconv_host import GEOMETRY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_ARG = 5
KERNELS = ("dgrad_kernel", "wgrad_kernel", "wreduce_kernel")


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def test_header_library_and_binding_name_the_same_symbols():
    header = open(os.path.join(ROOT, "include", "tfft_bconv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                # declarations only: the comments name calls too
    declared = set(re.findall(r"\b(tfft_bconv_[a-z0-9_]+)\s*\(", code))
    assert declared == set(bconv.SYMBOLS), declared ^ set(bconv.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", bconv.bconv_lib_path()], capture_output=True, text=True, check=True).stdout
    text_syms = {line.split()[2] for line in nm.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    # -fvisibility=hidden: nothing but the entry points is exported as code
    assert text_syms == declared, text_syms ^ declared
    lib = bconv.load_bconv_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert set(tf.__all__) >= {"TfftLongConvGradPlan", "bconv_geometry", "bconv_describe", "bconv_cache_clear", "long_causal_conv_input_grad",
                               "long_causal_conv_tap_grad", "differentiable_long_causal_conv"}


def test_library_links_the_other_two_and_none_of_the_other_three():
    dyn = subprocess.run(["readelf", "-d", bconv.bconv_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "libtfft_conv.so" in dyn and "libtfft.so" in dyn and "$ORIGIN" in dyn
    assert "libtfft_lconv.so" not in dyn and "libtfft_gconv.so" not in dyn and "libtfft_sconv.so" not in dyn
    assert ctypes.sizeof(bconv.BconvOpts) == 48                       # tfft_bconv_opts as the header lays it out
    assert bconv.BconvOpts.partials.offset == 36 and bconv.BconvOpts.flags.offset == 40


@pytest.fixture(scope="module")
def report():
    import isa_lint

    rep = isa_lint.lint_text(isa_lint.disassemble(bconv.bconv_lib_path()))
    names = subprocess.run(["c++filt"], input="\n".join(rep), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n.strip().split("(")[0]: r for n, r in zip(names, rep.values())}


def test_code_object_holds_exactly_the_three_kernels(report):
    assert set(report) == {"bconv4096::" + k for k in KERNELS}, list(report)
    # two transforms of 16 stage-1 tiles and 16 stage-2/3 tiles, two MFMAs per complex product: sconv4096_kernel's count;
    # one LDS-DMA per 1-KiB block and plane
    assert report["bconv4096::dgrad_kernel"]["mfma"] == 2 * (16 * 2 + 16 * 4) == 192
    assert report["bconv4096::dgrad_kernel"]["lds_dma"] == 16
    # three transforms (the x window, then sconv's two passes over the g window), two windows
    assert report["bconv4096::wgrad_kernel"]["mfma"] == 3 * (16 * 2 + 16 * 4) == 288
    assert report["bconv4096::wgrad_kernel"]["lds_dma"] == 32
    assert report["bconv4096::wreduce_kernel"]["mfma"] == 0 and report["bconv4096::wreduce_kernel"]["lds_dma"] == 0


def test_no_packed_fp32_wait_states_and_dma_drain(report):
    for name, kernel in report.items():
        assert kernel["pk_f32"] == 0, name
        assert not kernel["findings"], (name, kernel["findings"])


def test_kernel_resources():
    """no scratch and no spills in any kernel, from the kernel metadata notes. dgrad_kernel and wreduce_kernel stay within the 256
    registers of two waves per SIMD (the bounds of tests/test_sconv_host.py). wgrad_kernel runs in workgroups of four waves, one per
    SIMD, because it could not be had without spills under __launch_bounds__(512, 2): its budget is the 512
    registers of a lane, of which at most 256 are architectural VGPRs, the rest AGPRs the compiler parks values in."""
    import isa_lint

    tmp = tempfile.mkdtemp(prefix="tfft_bconv_isa_")
    try:
        local = os.path.join(tmp, "libtfft_bconv.so")
        shutil.copy(bconv.bconv_lib_path(), local)
        subprocess.check_call([os.path.join(isa_lint.LLVM_BIN, "llvm-objdump"), "--offloading", local], cwd=tmp,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f][0]
        notes = subprocess.check_output([os.path.join(isa_lint.LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(tmp, co)], text=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for kernel in KERNELS:
        blocks = [b for b in notes.split("- .agpr_count") if kernel in b]
        assert len(blocks) == 1, kernel
        agprs = int(re.match(r":\s+(\d+)", blocks[0]).group(1))
        total = int(re.search(r"\.vgpr_count:\s+(\d+)", blocks[0]).group(1))            # VGPRs and AGPRs of the unified file
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blocks[0]).group(1))
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blocks[0]).group(1))
        sgpr_spills = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blocks[0]).group(1))
        wg = int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", blocks[0]).group(1))
        print(f"{kernel}: {total} registers ({total - agprs} VGPRs + {agprs} AGPRs), workgroup {wg}, scratch {scratch}, spills {spills} / {sgpr_spills}")
        assert scratch == 0 and spills == 0 and sgpr_spills == 0, (kernel, scratch, spills, sgpr_spills)
        if kernel == "wgrad_kernel":
            assert wg == 256 and total - agprs <= 256 and total <= 512, (kernel, total, agprs, wg)
        else:
            assert agprs == 0 and total <= 256, (kernel, total, agprs)


@pytest.mark.parametrize("length,taps,halo,hop,segments", GEOMETRY)
def test_geometry_and_describe(length, taps, halo, hop, segments):
    lib = bconv.load_bconv_library()
    for rows, channels in ((3, 2), (1, 1), (5, 3), (64, 256), (2, 4096)):
        per_channel = (rows + 1) // 2 * segments
        default = min(per_channel, -(-2048 // channels))
        assert tf.bconv_geometry(length, taps, rows, channels) == (halo, hop, segments, default) == sr.geometry(length, taps) + (br.partials_of(rows, channels, length, taps),)
        assert 1 <= default <= per_channel and (default == per_channel or (default - 1) * channels < 2048 <= default * channels)
        for cap in (1, 2):
            assert tf.bconv_geometry(length, taps, rows, channels, cap)[3] == min(default, cap) == br.partials_of(rows, channels, length, taps, cap)
        assert tf.bconv_describe(length, taps, rows, channels) == f"bconv4096:4096 x {segments} | partials {default}"
        assert tf.bconv_describe(length, taps, rows, channels, 2) == f"bconv4096:4096 x {segments} | partials {min(default, 2)}"
    assert tf.bconv_geometry(length, taps)[:3] == tf.sconv_geometry(length, taps)
    # each pointer of tfft_bconv_geometry may be NULL
    one = ctypes.c_uint64()
    assert lib.tfft_bconv_geometry(length, taps, 3, 2, 0, None, None, ctypes.byref(one), None) == 0 and one.value == segments
    assert lib.tfft_bconv_geometry(length, taps, 3, 2, 0, None, None, None, None) == 0


def test_cases_cover_what_they_say():
    geo = {c[:2]: sr.geometry(c[0], c[1]) for c in br.DH_CASES}
    assert geo[(8, 1)] == (0, 4096, 1) and geo[(2056, 1)] == (0, 4096, 1) and geo[(2048, 2049)] == (2048, 2048, 1)
    assert geo[(4104, 7)] == (64, 4032, 2) and (4104 - 4032) // 8 == 9
    assert geo[(4096, 2049)] == (2048, 2048, 2) and geo[(6152, 130)] == (192, 3904, 2)
    # the accumulation loop of a wave runs 12, 6 and 10 times under the caps, once by default
    assert [(3 * 4) // p for p in (1, 2)] == [12, 6] and br.partials_of(5, 3, 8192, 2049) == 12
    assert br.partials_of(9, 3, 12288, 65, 2) == 2 and br.partials_of(9, 3, 12288, 65) == 20
    assert all(br.partials_of(c[2], c[3], c[0], c[1]) == (c[2] + 1) // 2 * geo[c[:2]][2] for c in br.DH_CASES)


def _opts(**kw):
    o = bconv.BconvOpts(ctypes.sizeof(bconv.BconvOpts), 0, 0, 0, 0, 0, 0, 0)
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
def test_describe_and_create_refuse_with_the_messages_of_sconv(rows, channels, length, taps, flags, needle):
    lib = bconv.load_bconv_library()
    buf = ctypes.create_string_buffer(256)
    assert lib.tfft_bconv_describe(length, taps, rows, channels, 0, flags, buf, len(buf)) == ERR_ARG
    message = lib.tfft_bconv_last_error().decode()
    assert needle in message
    h = ctypes.c_void_p()
    o = _opts(flags=flags)
    assert lib.tfft_bconv_plan_create(rows, channels, length, taps, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG    # before any device call
    assert lib.tfft_bconv_last_error().decode() == message and not h.value
    # the same refusal, word for word, as the forward plan's (its own struct's name apart)
    s_lib = tf.load_sconv_library()
    assert s_lib.tfft_sconv_describe(length, taps, rows, channels, flags, buf, len(buf)) == ERR_ARG
    assert s_lib.tfft_sconv_last_error().decode().replace("tfft_sconv_opts", "tfft_bconv_opts") == message
    if not flags:
        assert lib.tfft_bconv_geometry(length, taps, rows, channels, 0, None, None, None, None) == ERR_ARG
        assert lib.tfft_bconv_last_error().decode() == message


def test_geometry_leaves_its_outputs_alone_when_it_refuses():
    lib = bconv.load_bconv_library()
    halo = ctypes.c_uint64(77)
    assert lib.tfft_bconv_geometry(12, 1, 1, 1, 0, ctypes.byref(halo), None, None, None) == ERR_ARG and halo.value == 77
    with pytest.raises(tf.TfftError):
        tf.bconv_geometry(8, 2050)


@pytest.mark.parametrize("kw,needle", [
    (dict(x_seq_stride=8184), "x_seq_stride"), (dict(x_seq_stride=8196), "x_seq_stride"), (dict(g_seq_stride=8), "g_seq_stride"),
    (dict(g_seq_stride=8193), "g_seq_stride"), (dict(dx_seq_stride=8184), "dx_seq_stride"), (dict(dx_seq_stride=8201), "dx_seq_stride"),
    (dict(struct_size=0), "struct_size"), (dict(struct_size=40), "struct_size"), (dict(struct_size=56), "struct_size"),
    (dict(reserved_=1), "reserved_"), (dict(launch_iters=65536), "launch_iters"),
    (dict(flags=1), "flags must be 0"), (dict(flags=1 << 30), "flags must be 0"),
])
def test_create_refuses_bad_options(kw, needle):
    lib = bconv.load_bconv_library()
    h = ctypes.c_void_p()
    o = _opts(**kw)
    assert lib.tfft_bconv_plan_create(4, 2, 8192, 64, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG
    assert needle in lib.tfft_bconv_last_error().decode() and not h.value


def test_null_arguments_are_refused():
    lib = bconv.load_bconv_library()
    assert lib.tfft_bconv_plan_create(1, 1, 8, 1, 0, None, None) == ERR_ARG
    assert lib.tfft_bconv_describe(8, 1, 1, 1, 0, 0, None, 0) == ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert lib.tfft_bconv_describe(8, 1, 1, 1, 0, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_bconv_exec_input_grad(None, None, None, None) == ERR_ARG
    assert lib.tfft_bconv_exec_tap_grad(None, None, None, None, None) == ERR_ARG
    assert lib.tfft_bconv_plan_set_taps(None, None, None) == ERR_ARG
    assert lib.tfft_bconv_plan_spectrum(None, None, None) == ERR_ARG
    assert lib.tfft_bconv_plan_set_workspace(None, None, 0) == ERR_ARG
    assert lib.tfft_bconv_plan_prepare(None) == ERR_ARG
    assert lib.tfft_bconv_plan_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_bconv_plan_num_launches(None) == 0 and lib.tfft_bconv_plan_workspace_bytes(None) == 0
    lib.tfft_bconv_plan_destroy(None)
    assert lib.tfft_bconv_last_error().decode()


def test_no_gpu_means_errors_not_fallbacks():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(tf.TfftError):
        tf.TfftLongConvGradPlan(4, 2, 16384, 2049, 0)
    with pytest.raises(tf.TfftError):
        tf.TfftLongConvGradPlan(1, 1, 8, 1, 0)
    x, h = torch.zeros((2, 2, 4096), dtype=torch.float16), torch.zeros((2, 7), dtype=torch.float16)
    with pytest.raises(tf.TfftError):
        tf.long_causal_conv_input_grad(x, h)
    with pytest.raises(tf.TfftError):
        tf.long_causal_conv_tap_grad(x, x, 7)
    with pytest.raises(tf.TfftError):
        tf.differentiable_long_causal_conv(x.requires_grad_(), h)


@pytest.mark.parametrize("length,taps", sr.INDEX_CASES)
def test_window_identities_against_direct_sums(length, taps):
    """pure numpy, fp64: both gradients through their windows against direct sums, to 1e-12 relative; rows 3 (odd: a zero partner) x
    channels 2"""
    rows, channels = 3, 2
    rng = np.random.default_rng([length, taps, 5])
    x = rng.uniform(-1, 1, (rows, channels, length))
    g = rng.uniform(-1, 1, (rows, channels, length))
    h = rng.standard_normal((channels, taps))
    h /= np.abs(h).sum(axis=1, keepdims=True)
    halo, hop, segs = sr.geometry(length, taps)
    # dx: windows from s * hop, conj(H), the first hop samples kept
    re, im = br.dx_windows(g, taps)
    assert re.shape == im.shape == (sr.items_of(rows, channels, length, taps), 4096)
    assert not im[segs * channels:].any()                                  # the zero partner of row 2
    assert np.array_equal(br.dx_unwindow(re, im, rows, channels, length, taps), g)
    y = np.fft.ifft(np.fft.fft(re + 1j * im, axis=-1) * np.conj(np.fft.fft(h, 4096, axis=-1))[np.arange(re.shape[0]) % channels], axis=-1)
    got = br.dx_unwindow(y.real, y.imag, rows, channels, length, taps)
    want = br.dx_direct(g, h)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # dh: conj(fft(Zx)) fft(Zg) with the halo of Zg zeroed, RE plane, lags 0 .. K - 1, summed over the items of a channel
    zx, zg = br.dh_windows(x, g, taps)
    assert not zg[:, :halo].any() and np.array_equal(zx.real, sr.windows(x, taps)[0])
    items = np.fft.ifft(np.conj(np.fft.fft(zx, axis=-1)) * np.fft.fft(zg, axis=-1), axis=-1)
    got = br.dh_from_items(items, channels, taps)
    want = br.dh_direct(x, g, taps)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the order the plan adds in: by_channel puts a channel's items in increasing i = p * S + s
    idx = br.by_channel(np.arange(items.shape[0]), channels)
    assert all(np.array_equal(idx[c], np.arange(items.shape[0] // channels) * channels + c) for c in range(channels))


@pytest.fixture(scope="module")
def dh_numbers():
    """per distinct (L, K, B, C) of DH_CASES, on the GPU test's data (seed 1): the rounding of Zx / 4096 alone in ulps of the item's
    peak, the emulation's error over the derived bound, max |G| |Zx / 4096|"""
    out = {}
    for length, taps, rows, channels, _ in br.DH_CASES:
        if (length, taps, rows, channels) in out:
            continue
        x, _h = lr.case_data(length, taps, rows, channels, "noise", 1)
        g = br.grad_signal(rows, channels, length, taps, 1)
        true, emulated = br.dh_items(x, g, taps), br.dh_items(x, g, taps, rounded=True)
        rounding = (np.abs((emulated - true).real[:, :taps]) / br.item_unit(true)[:, None]).max()
        ratio = (np.abs(br.dh_from_items(emulated, channels, taps) - br.dh_from_items(true, channels, taps)) / br.dh_bound(true, channels)[:, None]).max()
        zx, zg = br.dh_windows(x, g, taps)
        big = (np.abs(np.fft.fft(zg, axis=-1)) * np.abs(br.half_spectrum(zx))).max()
        out[(length, taps, rows, channels)] = (rounding, ratio, big)
    return out


def test_spectrum_rounding_is_inside_the_allowance(dh_numbers):
    """A_SPECTRUM of tests/bconv_ref.py is the next half-integer above what rounding Zx / 4096 to binary16 alone does"""
    worst = max(v[0] for v in dh_numbers.values())
    print(f"rounding of Zx / 4096 alone: {worst:.3f} ulp of the item's peak; A_SPECTRUM = {br.A_SPECTRUM}")
    assert br.A_SPECTRUM - 0.5 < worst <= br.A_SPECTRUM
    assert br.K_CONV_FUSED == __import__("conv_ref").K_CONV_FUSED


def test_emulation_meets_the_derived_bound(dh_numbers):
    """fp64 arithmetic with the binary16 Zx spectrum, against fp64 throughout, in units of the bound the GPU test asserts: the
    emulation has only the spectrum's rounding, A_SPECTRUM of the K_CONV_FUSED + A_SPECTRUM ulps, and the errors of a channel's items
    add up at random where the bound adds them in magnitude"""
    worst = max(v[1] for v in dh_numbers.values())
    print(f"emulation / bound: {worst:.3f}")
    assert worst <= br.A_SPECTRUM / (br.K_CONV_FUSED + br.A_SPECTRUM)


def test_range_contract(dh_numbers):
    big = max(v[2] for v in dh_numbers.values())
    print(f"max |G| |Zx / 4096| = {big:.2f}")
    assert big <= 32752 / 32
