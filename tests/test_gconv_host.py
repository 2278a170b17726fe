"""Gated causal convolution add-on (include/tfft_gconv.h, libtfft_gconv.so) on the host, as tests/test_lconv_host.py checks its
sibling: the exported symbols, the kernels and the gfx950 ISA of its code object (tools/isa_lint.py), the transform length, the
planner's description, every refusal that needs no device, the host spectrum with and without a skip weight, and the range
contract over the data of the GPU tests."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import elementwise_bound as eb
import gconv_ref as gr
import lconv_ref as lr
import tensor_fft_amd as tf
from tensor_fft_amd import gconv, lconv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_ARG = 5
FUSED = {f"gconv4096::gconv4096_kernel<{p}, {q}>" for p in ("true", "false") for q in ("true", "false")}
COPIES = {f"gate_copy::{k}_kernel<{v}>" for k in ("pack", "crop") for v in ("true", "false")}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def test_header_library_and_binding_name_the_same_symbols():
    header = open(os.path.join(ROOT, "include", "tfft_gconv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                # declarations only: the comments name calls too
    declared = set(re.findall(r"\b(tfft_gconv_[a-z0-9_]+)\s*\(", code))
    assert declared == set(gconv.SYMBOLS), declared ^ set(gconv.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", gconv.gconv_lib_path()], capture_output=True, text=True, check=True).stdout
    text_syms = {line.split()[2] for line in nm.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    # -fvisibility=hidden: nothing but the entry points is exported as code
    assert text_syms == declared, text_syms ^ declared
    lib = gconv.load_gconv_library()
    for name in declared:
        assert hasattr(lib, name), name
    for name in ("TfftGatedConvPlan", "gated_causal_conv", "gconv_cache_clear", "gconv_describe", "gconv_fft_length", "gconv_lib_path",
                 "gconv_spectrum_host", "load_gconv_library"):
        assert getattr(tf, name) is getattr(gconv, name) and name in tf.__all__


def test_library_links_the_two_below_and_not_the_causal_one():
    dyn = subprocess.run(["readelf", "-d", gconv.gconv_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "libtfft_conv.so" in dyn and "libtfft.so" in dyn and "$ORIGIN" in dyn and "libtfft_lconv.so" not in dyn
    # tfft_gconv_opts as the header lays it out: two uint32, four uint64 strides, launch_iters and flags
    assert ctypes.sizeof(gconv.GconvOpts) == 48 and gconv.GconvOpts.flags.offset == 44 and gconv.GconvOpts.post_seq_stride.offset == 32


@pytest.fixture(scope="module")
def report():
    import isa_lint

    rep = isa_lint.lint_text(isa_lint.disassemble(gconv.gconv_lib_path()))
    names = subprocess.run(["c++filt"], input="\n".join(rep), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n.strip().removeprefix("void ").split("(")[0]: rep[k] for n, k in zip(names, rep)}


def test_code_object_holds_exactly_the_eight_instantiations(report):
    assert set(report) == FUSED | COPIES and len(report) == 8, sorted(report)
    for name in FUSED:
        # two transforms of 16 stage-1 tiles and 16 stage-2/3 tiles, two MFMAs per complex product: lconv4096_kernel's count
        assert report[name]["mfma"] == 2 * (16 * 2 + 16 * 4) == 192, name
        # Without a pre gate the load is lconv4096_kernel's: one LDS-DMA per 1-KiB block and plane. With one, x and the gate come in
        # through registers and the product is written with ds_write_b128: no LDS-DMA at all.
        assert report[name]["lds_dma"] == (0 if name.startswith("gconv4096::gconv4096_kernel<true") else 16), name
    for name in COPIES:
        assert report[name]["mfma"] == 0 and not report[name]["lds_dma"], name


def test_no_packed_fp32_wait_states_and_dma_drain(report):
    for name in FUSED:
        assert report[name]["pk_f32"] == 0, name
    for name in FUSED | COPIES:
        assert not report[name]["findings"], (name, report[name]["findings"])


def test_fused_kernel_resources():
    """no scratch, no spills and at most 256 VGPRs for every fused instantiation, from the kernel metadata notes"""
    import isa_lint

    tmp = tempfile.mkdtemp(prefix="tfft_gconv_isa_")
    try:
        local = os.path.join(tmp, "libtfft_gconv.so")
        shutil.copy(gconv.gconv_lib_path(), local)
        subprocess.check_call([os.path.join(isa_lint.LLVM_BIN, "llvm-objdump"), "--offloading", local], cwd=tmp,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f][0]
        notes = subprocess.check_output([os.path.join(isa_lint.LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(tmp, co)], text=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    blocks = [b for b in notes.split("- .agpr_count") if "gconv4096_kernel" in b]
    assert len(blocks) == 4
    for b in blocks:
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1))
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1))
        sgpr_spills = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", b).group(1))
        assert scratch == 0 and spills == 0 and sgpr_spills == 0 and vgprs <= 256, (vgprs, scratch, spills, sgpr_spills)


def test_fft_length():
    for length, taps, n in ((8, 1, 256), (96, 33, 256), (128, 129, 256), (128, 130, 512), (2048, 2049, 4096), (2040, 2057, 4096),
                            (2048, 2050, 8192), (2056, 1, 4096), (4096, 1, 4096), (40000, 20000, 1 << 16), (1 << 25, (1 << 25) + 1, 1 << 26)):
        assert tf.gconv_fft_length(length, taps) == n == tf.lconv_fft_length(length, taps), (length, taps)
    for length, taps in ((0, 1), (8, 0), (1 << 26, 2), (1 << 27, 1), (8, 1 << 27)):
        assert tf.gconv_fft_length(length, taps) == 0, (length, taps)
    assert all(gr.plan_length(c[0], c[1]) == 4096 for c in gr.FUSED_CASES)
    assert all(gr.plan_length(c[1], c[2], c[5]) == c[0] == gr.fft_length(c[1], c[2]) for c in gr.COMPOSED_CASES)


def test_describe():
    assert tf.gconv_describe(2048, 2049, 131072, 64) == "gconv4096:4096"
    assert tf.gconv_describe(2048, 2049, 131072, 64, pre_gate=True) == "gconv4096:4096:pre"
    assert tf.gconv_describe(2048, 2049, 131072, 64, post_gate=True) == "gconv4096:4096:post"
    assert tf.gconv_describe(2048, 2049, 131072, 64, pre_gate=True, post_gate=True) == "gconv4096:4096:pre+post"
    for length, taps in ((8, 1), (520, 7), (1024, 1025), (2040, 2057), (8, 4089), (2048, 1)):
        assert tf.gconv_describe(length, taps, 3, 2, pre_gate=True) == "gconv4096:4096:pre", (length, taps)
    assert tf.gconv_describe(2048, 2049, 3, 3, composed=True) == "pack | conv4096:4096 | crop"
    assert tf.gconv_describe(2048, 2049, 3, 3, pre_gate=True, post_gate=True, composed=True) == "pack:pre | conv4096:4096 | crop:post"
    # beyond the fused kernel's shapes, and with the flag: the sub-plan of the shortest transform length between the two copies
    for length, taps, rows, channels, composed in ((96, 33, 5, 4, True), (1000, 500, 3, 2, True), (2056, 1, 2, 2, False), (8, 4090, 1, 1, False),
                                                   (4096, 4097, 3, 2, False), (40000, 20000, 3, 2, False)):
        n = gr.fft_length(length, taps)
        sub = tf.conv_describe(n, (rows + 1) // 2 * channels, channels)
        assert tf.gconv_describe(length, taps, rows, channels, composed=composed) == f"pack | {sub} | crop"
        assert tf.gconv_describe(length, taps, rows, channels, pre_gate=True, composed=composed) == f"pack:pre | {sub} | crop"
        assert tf.gconv_describe(length, taps, rows, channels, post_gate=True, composed=composed) == f"pack | {sub} | crop:post"


def _opts(**kw):
    o = gconv.GconvOpts(ctypes.sizeof(gconv.GconvOpts), 0, 0, 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("rows,channels,length,taps,flags,needle", [
    (1, 1, 0, 1, 0, "multiple of 8"), (1, 1, 4, 1, 3, "multiple of 8"), (1, 1, 2044, 1, 0, "multiple of 8"),
    (1, 1, 8, 0, 0, "taps"), (0, 1, 8, 1, 0, "rows"), (1 << 32, 1, 8, 1, 0, "rows"), (1, 0, 8, 1, 0, "channels"),
    (1 << 16, 1 << 16, 8, 1, 0, "rows * channels"), (1, 1, 8, 1, 8, "flag"), (1, 1, 8, 1, 16 | 3, "flag"), (1, 1, 8, 1, -1, "flag"),
    (1, 1, 1 << 26, 2, 0, "2^26"), (1, 1, 8, (1 << 26) + 1, 4, "2^26"),
])
def test_describe_and_create_refuse_with_a_message(rows, channels, length, taps, flags, needle):
    lib = gconv.load_gconv_library()
    buf = ctypes.create_string_buffer(256)
    assert lib.tfft_gconv_describe(length, taps, rows, channels, flags, buf, len(buf)) == ERR_ARG
    assert needle in lib.tfft_gconv_last_error().decode()
    h = ctypes.c_void_p()
    o = _opts(flags=flags)
    assert lib.tfft_gconv_plan_create(rows, channels, length, taps, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG    # before any device call
    assert needle in lib.tfft_gconv_last_error().decode() and not h.value
    # the same refusal, in the same words, as the causal plans give (flags apart: they have other bits)
    if needle != "flag":
        lc = lconv.load_lconv_library()
        assert lc.tfft_lconv_describe(length, taps, rows, channels, 0, buf, len(buf)) == ERR_ARG
        assert lc.tfft_lconv_last_error() == lib.tfft_gconv_last_error()


@pytest.mark.parametrize("kw,needle", [
    (dict(in_seq_stride=2040), "in_seq_stride"), (dict(in_seq_stride=2052), "in_seq_stride"), (dict(out_seq_stride=8), "out_seq_stride"),
    (dict(out_seq_stride=2049), "out_seq_stride"), (dict(pre_seq_stride=2040), "pre_seq_stride"), (dict(pre_seq_stride=2052), "pre_seq_stride"),
    (dict(post_seq_stride=8), "post_seq_stride"), (dict(post_seq_stride=2049), "post_seq_stride"),
    (dict(struct_size=0), "struct_size"), (dict(struct_size=32), "struct_size"), (dict(struct_size=40), "struct_size"),
    (dict(struct_size=56), "struct_size"), (dict(reserved_=1), "reserved_"), (dict(launch_iters=65536), "launch_iters"),
])
def test_create_refuses_bad_options(kw, needle):
    lib = gconv.load_gconv_library()
    h = ctypes.c_void_p()
    o = _opts(**kw)
    assert lib.tfft_gconv_plan_create(4, 2, 2048, 64, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG
    assert needle in lib.tfft_gconv_last_error().decode() and not h.value


def test_null_arguments_are_refused():
    lib = gconv.load_gconv_library()
    assert lib.tfft_gconv_plan_create(1, 1, 8, 1, 0, None, None) == ERR_ARG
    assert lib.tfft_gconv_describe(8, 1, 1, 1, 0, None, 0) == ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert lib.tfft_gconv_describe(8, 1, 1, 1, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_gconv_exec(None, None, None, None, None, None) == ERR_ARG
    assert lib.tfft_gconv_plan_set_taps(None, None, None, None) == ERR_ARG
    assert lib.tfft_gconv_plan_spectrum(None, None, None) == ERR_ARG
    assert lib.tfft_gconv_plan_prepare(None) == ERR_ARG and lib.tfft_gconv_plan_set_workspace(None, None, 0) == ERR_ARG
    assert lib.tfft_gconv_plan_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_gconv_plan_num_launches(None) == 0 and lib.tfft_gconv_plan_workspace_bytes(None) == 0
    assert lib.tfft_gconv_plan_fft_length(None) == 0
    lib.tfft_gconv_plan_destroy(None)
    one = np.ones(1, np.float16)
    out = np.empty(8, np.float16)
    for args in ((None, 1, None, 8, out.ctypes.data, out.ctypes.data), (one.ctypes.data, 1, None, 8, None, out.ctypes.data),
                 (one.ctypes.data, 0, None, 8, out.ctypes.data, out.ctypes.data), (one.ctypes.data, 9, None, 8, out.ctypes.data, out.ctypes.data),
                 (one.ctypes.data, 1, one.ctypes.data, 12, out.ctypes.data, out.ctypes.data),
                 (one.ctypes.data, 1, None, 1 << 27, out.ctypes.data, out.ctypes.data)):
        assert lib.tfft_gconv_spectrum_host(*args) == ERR_ARG, args


def test_no_gpu_means_errors_not_fallbacks():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(tf.TfftError):
        tf.TfftGatedConvPlan(4, 2, 2048, 64, 0, pre_gate=True, post_gate=True)
    with pytest.raises(tf.TfftError):
        tf.TfftGatedConvPlan(4, 2, 4096, 64, 0, post_gate=True)
    with pytest.raises(tf.TfftError):
        tf.gated_causal_conv(np.zeros((2, 2, 8), np.float16), np.zeros((2, 1), np.float16))


def _ulp_of(v):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14))) - 10)


@pytest.mark.parametrize("taps,n", [(1, 4096), (7, 4096), (2049, 4096), (20000, 1 << 16)])
@pytest.mark.parametrize("kind", ["decay", "noise", "delay"])
def test_spectrum_host(taps, n, kind):
    rng = np.random.default_rng([taps, n])
    h = lr.make_taps(kind, 2, taps, rng)[1]
    # no skip, and a skip of zero of either sign: bit for bit the causal plans' spectrum
    want = tf.lconv_spectrum_host(h, n)
    for skip in (None, 0.0, -0.0):
        got = tf.gconv_spectrum_host(h, n, skip)
        assert np.array_equal(got[0].view(np.uint16), want[0].view(np.uint16)), skip
        assert np.array_equal(got[1].view(np.uint16), want[1].view(np.uint16)), skip
    # with a skip: numpy's FFT of the taps plus d in every bin, within the bound test_spectrum_host_against_numpy uses
    for d in (0.5, -0.375, 0.125):
        re, im = tf.gconv_spectrum_host(h, n, d)
        ref = np.fft.fft(h.astype(np.float64), n) + d
        assert (np.abs(re.astype(np.float64) - ref.real) <= _ulp_of(ref.real)).all(), d
        assert (np.abs(im.astype(np.float64) - ref.imag) <= _ulp_of(ref.imag)).all(), d
        assert np.array_equal(re[1:], re[:0:-1]) and np.array_equal(im[1:], -im[:0:-1])
        assert im.view(np.uint16)[0] == 0 and im.view(np.uint16)[n // 2] == 0


def test_skip_is_added_before_the_one_rounding():
    """tap 0 = 1 + 2^-10 and skip = 2^-11 sum to 1 + 2^-10 + 2^-11 in fp64, which every bin of the spectrum of a one-tap filter then
    rounds ONCE, to even: 1 + 2^-9. Adding in binary16 first, or rounding the spectrum before the skip goes in, gives 1 + 2^-10."""
    h = np.array([1.0 + 2.0 ** -10], np.float16)
    re, im = tf.gconv_spectrum_host(h, 256, 2.0 ** -11)
    assert (re.astype(np.float64) == 1.0 + 2.0 ** -9).all() and not im.any()


def test_range_contract_and_spectrum_rounding():
    """Over the cases, tap kinds and gate modes of the GPU tests (seed 1): max |U_k| |H'_k| stays a factor 64 inside the 32752 of the
    range contract (tests/gconv_ref.py: 222 over three seeds), |g z| <= |z| because |g| <= 1, and the rounding of H' to binary16 alone
    stays inside the allowance the comparison with the true result grants for it: 1 ulp of the pair's peak and rel-L2 2^-11 (0.54 ulp
    and 2.2e-4 over three seeds)."""
    assert np.array_equal(gr.skip_values(5).astype(np.float64), [0.5, -0.375, 0.25, -0.125, 0.5])
    big = worst = worst_l2 = 0.0
    cases = [c[:4] + (False,) for c in gr.FUSED_CASES] + [c[1:] for c in gr.COMPOSED_CASES]
    for length, taps, rows, channels, composed in cases:
        n = gr.plan_length(length, taps, composed)
        for kind in gr.TAP_KINDS:
            for mode in gr.GATE_MODES:
                x, h, p, g, skip = gr.case_data(length, taps, rows, channels, kind, 1, mode)
                assert all(t is None or (t.shape == x.shape and t.dtype == np.float16 and np.abs(t).max() <= 1.0) for t in (p, g))
                u = gr.gated_input(x, p)
                spec = [tf.gconv_spectrum_host(h[c], n, None if skip is None else skip[c]) for c in range(channels)]
                h_re, h_im = np.stack([s[0] for s in spec]), np.stack([s[1] for s in spec])
                re, im = lr.pair_planes(u.astype(np.float64), n)
                idx = np.arange(re.shape[0]) % channels
                spectrum = np.fft.fft(re + 1j * im, axis=-1)
                big = max(big, np.abs(spectrum * (h_re.astype(np.float64) + 1j * h_im.astype(np.float64))[idx]).max())
                rounded = lr.reference_spectrum(u, h_re, h_im, n)[:, :length]
                true = gr.reference_true(u, h, skip, n)
                unit = eb.ulp16(lr.pair_peak(true))[:, None]
                true = true[:, :length]
                worst = max(worst, (np.abs(rounded - true) / unit).max())
                worst_l2 = max(worst_l2, np.sqrt((np.abs(rounded - true) ** 2).sum(-1) / (np.abs(true) ** 2).sum(-1)).max())
    print(f"max |U H'| = {big:.1f}, rounding of H' alone: {worst:.3f} ulp, rel-L2 {worst_l2:.2e}")
    assert big <= 32752 / 64, big
    assert worst <= 1.0 and worst_l2 <= 2.0 ** -11, (worst, worst_l2)
    # the two gates of a case differ from each other and from sample to sample
    p, g = gr.gates(3, 2, 64, 1)
    assert len(np.unique(np.concatenate((p.reshape(-1), g.reshape(-1))))) > 100 and not np.array_equal(p, g)
    # half_product is one binary16 multiply: subnormal products are kept, ties go to even
    a = np.array([2.0 ** -12, 2.0 ** -14, 1.0 + 2.0 ** -10, 3.0], np.float16)
    b = np.array([2.0 ** -12, 2.0 ** -11, 1.0 + 2.0 ** -10, 2.0 ** -24], np.float16)
    assert np.array_equal(gr.half_product(a, b).astype(np.float64), [2.0 ** -24, 0.0, 1.0 + 2.0 ** -9, 3 * 2.0 ** -24])
