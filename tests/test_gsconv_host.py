"""Gated overlap-save causal convolution add-on (include/tfft_gsconv.h, libtfft_gsconv.so) on the host, as tests/test_sconv_host.py
and tests/test_gconv_host.py check its two parents: the exported symbols, the four instantiations and the gfx950 ISA of its code
object (tools/isa_lint.py), the geometry against tfft_sconv_geometry, the description, every refusal that needs no device, the
index arithmetic of the two gates in pure numpy against numpy.convolve, and the range contract over the data of the GPU tests."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import gsconv_ref as gs
import sconv_ref as sr
import tensor_fft_amd as tf
import test_sconv_host as tsh
from tensor_fft_amd import gsconv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_ARG = 5
KERNELS = {f"gsconv4096::gsconv4096_kernel<{p}, {q}>" for p in ("true", "false") for q in ("true", "false")}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def test_header_library_and_binding_name_the_same_symbols():
    header = open(os.path.join(ROOT, "include", "tfft_gsconv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                # declarations only: the comments name calls too
    declared = set(re.findall(r"\b(tfft_gsconv_[a-z0-9_]+)\s*\(", code))
    assert declared == set(gsconv.SYMBOLS), declared ^ set(gsconv.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", gsconv.gsconv_lib_path()], capture_output=True, text=True, check=True).stdout
    text_syms = {line.split()[2] for line in nm.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    # -fvisibility=hidden: nothing but the entry points is exported as code
    assert text_syms == declared, text_syms ^ declared
    lib = gsconv.load_gsconv_library()
    for name in declared:
        assert hasattr(lib, name), name
    for name in ("TfftGatedLongConvPlan", "gated_long_causal_conv", "gsconv_cache_clear", "gsconv_describe", "gsconv_geometry", "gsconv_lib_path",
                 "load_gsconv_library"):
        assert getattr(tf, name) is getattr(gsconv, name) and name in tf.__all__


def test_library_links_the_two_below_and_none_of_the_other_four():
    dyn = subprocess.run(["readelf", "-d", gsconv.gsconv_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "libtfft_conv.so" in dyn and "libtfft.so" in dyn and "$ORIGIN" in dyn
    for other in ("libtfft_lconv.so", "libtfft_gconv.so", "libtfft_sconv.so", "libtfft_bconv.so"):
        assert other not in dyn, other
    # tfft_gsconv_opts as the header lays it out, the fields of tfft_gconv_opts: two uint32, four uint64 strides, launch_iters and flags
    assert ctypes.sizeof(gsconv.GsconvOpts) == 48 and gsconv.GsconvOpts.flags.offset == 44 and gsconv.GsconvOpts.post_seq_stride.offset == 32
    assert [f[0] for f in gsconv.GsconvOpts._fields_] == [f[0] for f in tf.gconv.GconvOpts._fields_]
    assert (gsconv.GSCONV_PRE_GATE, gsconv.GSCONV_POST_GATE) == (1, 2)
    header = open(os.path.join(ROOT, "include", "tfft_gsconv.h")).read()
    assert re.search(r"TFFT_GSCONV_PRE_GATE = 1,", header) and re.search(r"TFFT_GSCONV_POST_GATE = 2\b", header)


@pytest.fixture(scope="module")
def report():
    import isa_lint

    rep = isa_lint.lint_text(isa_lint.disassemble(gsconv.gsconv_lib_path()))
    names = subprocess.run(["c++filt"], input="\n".join(rep), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n.strip().removeprefix("void ").split("(")[0]: rep[k] for n, k in zip(names, rep)}


def test_code_object_holds_exactly_the_four_instantiations(report):
    assert set(report) == KERNELS and len(report) == 4, sorted(report)
    for name in KERNELS:
        # two transforms of 16 stage-1 tiles and 16 stage-2/3 tiles, two MFMAs per complex product: sconv4096_kernel's count
        assert report[name]["mfma"] == 2 * (16 * 2 + 16 * 4) == 192, name
        # Without a pre gate the load is sconv4096_kernel's: one LDS-DMA per 1-KiB block and plane. With one, x and the gate come in
        # through registers and the product is written with ds_write_b128: no LDS-DMA at all.
        assert report[name]["lds_dma"] == (0 if name.startswith("gsconv4096::gsconv4096_kernel<true") else 16), name


def test_no_packed_fp32_wait_states_and_dma_drain(report):
    for name in KERNELS:
        assert report[name]["pk_f32"] == 0, name
        assert not report[name]["findings"], (name, report[name]["findings"])


def test_kernel_resources():
    """no scratch, no spills and at most 256 VGPRs for every instantiation at two waves per SIMD, from the kernel metadata notes"""
    import isa_lint

    tmp = tempfile.mkdtemp(prefix="tfft_gsconv_isa_")
    try:
        local = os.path.join(tmp, "libtfft_gsconv.so")
        shutil.copy(gsconv.gsconv_lib_path(), local)
        subprocess.check_call([os.path.join(isa_lint.LLVM_BIN, "llvm-objdump"), "--offloading", local], cwd=tmp,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f][0]
        notes = subprocess.check_output([os.path.join(isa_lint.LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(tmp, co)], text=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    blocks = [b for b in notes.split("- .agpr_count") if "gsconv4096_kernel" in b]
    assert len(blocks) == 4
    for b in blocks:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1))
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1))
        sgpr_spills = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", b).group(1))
        threads = int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", b).group(1))
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, spills {spills} / {sgpr_spills}, workgroup {threads}")
        assert scratch == 0 and spills == 0 and sgpr_spills == 0 and vgprs <= 256, (name, vgprs, scratch, spills, sgpr_spills)
        assert threads == 512, (name, threads)              # __launch_bounds__(512, 2): no instantiation took the one-wave fallback


@pytest.mark.parametrize("length,taps,halo,hop,segments", tsh.GEOMETRY)
def test_geometry_is_sconv_geometry(length, taps, halo, hop, segments):
    assert tf.gsconv_geometry(length, taps) == (halo, hop, segments) == tf.sconv_geometry(length, taps) == gs.geometry(length, taps)
    lib = gsconv.load_gsconv_library()
    one = ctypes.c_uint64()
    assert lib.tfft_gsconv_geometry(length, taps, None, None, ctypes.byref(one)) == 0 and one.value == segments
    assert lib.tfft_gsconv_geometry(length, taps, None, None, None) == 0


def test_describe():
    for length, taps, _, _, segments in tsh.GEOMETRY:
        assert tf.gsconv_describe(length, taps, 3, 2) == f"gsconv4096:4096 x {segments}"
        assert tf.gsconv_describe(length, taps, 3, 2, pre_gate=True) == f"gsconv4096:4096:pre x {segments}"
        assert tf.gsconv_describe(length, taps, 3, 2, post_gate=True) == f"gsconv4096:4096:post x {segments}"
        assert tf.gsconv_describe(length, taps, 3, 2, pre_gate=True, post_gate=True) == f"gsconv4096:4096:pre+post x {segments}"
    assert tf.gsconv_describe(16384, 2049, 256, 64, pre_gate=True, post_gate=True) == "gsconv4096:4096:pre+post x 8"
    # the existing planners route as before: the gated causal plan still composes these lengths
    assert tf.gconv_describe(16384, 2049, 4, 2, pre_gate=True, post_gate=True).startswith("pack:pre |")


def _opts(**kw):
    o = gsconv.GsconvOpts(ctypes.sizeof(gsconv.GsconvOpts), 0, 0, 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("rows,channels,length,taps,flags,needle", [
    (1, 1, 0, 1, 0, "multiple of 8"), (1, 1, 4, 1, 3, "multiple of 8"), (1, 1, 4100, 1, 0, "multiple of 8"),
    (1, 1, 8, 0, 0, "taps must be at least 1"), (1, 1, 8, 2050, 3, "tfft_gconv_plan_create"), (1, 1, 16384, 1 << 20, 0, "tfft_gconv_plan_create"),
    (0, 1, 8, 1, 0, "rows"), (1 << 32, 1, 8, 1, 0, "rows"), (1, 0, 8, 1, 0, "channels"),
    (1 << 16, 1 << 16, 8, 1, 0, "rows * channels"), (1, 1, 8, 1, 4, "flag"), (1, 1, 8, 1, 8 | 3, "flag"), (1, 1, 8, 1, -1, "flag"),
    (1, 1, (1 << 26) + 8, 2, 0, "2^26"), (1 << 20, 1 << 10, 1 << 20, 2049, 0, "item count"),
])
def test_describe_and_create_refuse_with_a_message(rows, channels, length, taps, flags, needle):
    lib = gsconv.load_gsconv_library()
    buf = ctypes.create_string_buffer(256)
    assert lib.tfft_gsconv_describe(length, taps, rows, channels, flags, buf, len(buf)) == ERR_ARG
    assert needle in lib.tfft_gsconv_last_error().decode()
    h = ctypes.c_void_p()
    o = _opts(flags=flags)
    assert lib.tfft_gsconv_plan_create(rows, channels, length, taps, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG    # before any device call
    assert needle in lib.tfft_gsconv_last_error().decode() and not h.value
    # the same refusal, in the same words, as the overlap-save plans give (flags and the too-long filter apart: those name other things)
    if needle not in ("flag", "tfft_gconv_plan_create"):
        sc = tf.sconv.load_sconv_library()
        assert sc.tfft_sconv_describe(length, taps, rows, channels, 0, buf, len(buf)) == ERR_ARG
        assert sc.tfft_sconv_last_error() == lib.tfft_gsconv_last_error()


@pytest.mark.parametrize("length,taps,needle", [(0, 1, "multiple of 8"), (12, 1, "multiple of 8"), (8, 0, "taps"), (8, 2050, "tfft_gconv_plan_create"),
                                                ((1 << 26) + 8, 1, "2^26")])
def test_geometry_refuses_what_create_refuses(length, taps, needle):
    lib = gsconv.load_gsconv_library()
    halo = ctypes.c_uint64(77)
    assert lib.tfft_gsconv_geometry(length, taps, ctypes.byref(halo), None, None) == ERR_ARG and halo.value == 77
    assert needle in lib.tfft_gsconv_last_error().decode()
    with pytest.raises(tf.TfftError):
        tf.gsconv_geometry(length, taps)


@pytest.mark.parametrize("kw,needle", [
    (dict(in_seq_stride=8184), "in_seq_stride"), (dict(in_seq_stride=8196), "in_seq_stride"), (dict(out_seq_stride=8), "out_seq_stride"),
    (dict(out_seq_stride=8193), "out_seq_stride"), (dict(pre_seq_stride=8184), "pre_seq_stride"), (dict(pre_seq_stride=8196), "pre_seq_stride"),
    (dict(post_seq_stride=8), "post_seq_stride"), (dict(post_seq_stride=8193), "post_seq_stride"),
    (dict(struct_size=0), "struct_size"), (dict(struct_size=32), "struct_size"), (dict(struct_size=40), "struct_size"),
    (dict(struct_size=56), "struct_size"), (dict(reserved_=1), "reserved_"), (dict(launch_iters=65536), "launch_iters"),
    (dict(flags=4), "TFFT_GSCONV_PRE_GATE and TFFT_GSCONV_POST_GATE only"), (dict(flags=1 << 30), "unknown flag bits"),
])
def test_create_refuses_bad_options(kw, needle):
    lib = gsconv.load_gsconv_library()
    h = ctypes.c_void_p()
    o = _opts(**kw)
    assert lib.tfft_gsconv_plan_create(4, 2, 8192, 64, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG
    assert needle in lib.tfft_gsconv_last_error().decode() and not h.value


def test_null_arguments_are_refused():
    lib = gsconv.load_gsconv_library()
    assert lib.tfft_gsconv_plan_create(1, 1, 8, 1, 0, None, None) == ERR_ARG
    assert lib.tfft_gsconv_describe(8, 1, 1, 1, 0, None, 0) == ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert lib.tfft_gsconv_describe(8, 1, 1, 1, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_gsconv_exec(None, None, None, None, None, None) == ERR_ARG
    assert lib.tfft_gsconv_plan_set_taps(None, None, None, None) == ERR_ARG
    assert lib.tfft_gsconv_plan_spectrum(None, None, None) == ERR_ARG
    assert lib.tfft_gsconv_plan_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_gsconv_plan_num_launches(None) == 0
    lib.tfft_gsconv_plan_destroy(None)
    assert lib.tfft_gsconv_last_error().decode()


def test_no_gpu_means_errors_not_fallbacks():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(tf.TfftError):
        tf.TfftGatedLongConvPlan(4, 2, 16384, 2049, 0, pre_gate=True, post_gate=True)
    with pytest.raises(tf.TfftError):
        tf.TfftGatedLongConvPlan(1, 1, 8, 1, 0)
    with pytest.raises(tf.TfftError):
        tf.gated_long_causal_conv(torch.zeros((2, 2, 4096), dtype=torch.float16), torch.zeros((2, 7), dtype=torch.float16))


def test_cases_and_modes_are_the_issue_s():
    assert gs.CASES is sr.CASES and len(gs.CASES) == 9 and gs.CASES[0] == (8, 1, 1, 1, 0) and gs.CASES[-1] == (12288, 65, 9, 3, 4)
    assert gs.TAP_KINDS == ("delay", "noise") and list(gs.GATE_MODES) == ["pre", "post", "pre+post", "skip", "pre+post+skip"]
    assert all((c + ("pre+post+skip",)) in gs.CASE_MODES for c in gs.CASES)
    assert len(gs.CASE_MODES) == 5 + 4 * 5
    for c in ((8, 1, 1, 1, 0), (2048, 2049, 3, 3, 2), (6152, 130, 3, 3, 0), (8192, 2049, 5, 3, 3)):
        assert all((c + (m,)) in gs.CASE_MODES for m in gs.GATE_MODES)


@pytest.mark.parametrize("mode", list(gs.GATE_MODES))
@pytest.mark.parametrize("length,taps", sr.INDEX_CASES)
def test_gate_indexing_against_numpy_convolve(length, taps, mode):
    """pure numpy fp64: gate -> windows -> circular convolution of every window -> un-window -> gate (gsconv_ref.model, the
    kernel's route: the pre gate by source sample before the windows are cut, the post gate by output sample after they are
    joined) against numpy.convolve on u plus the skip, times g; rows 3 (odd: a zero partner) x channels 2. Then the two wrong
    routes, a gate indexed by the WINDOW sample: each must differ wherever the halo is not zero."""
    rows, channels = 3, 2
    pre, post, has_skip = gs.GATE_MODES[mode]
    rng = np.random.default_rng([length, taps, 7])
    x = rng.uniform(-1, 1, (rows, channels, length))
    p = rng.uniform(-1, 1, x.shape) if pre else None
    g = rng.uniform(-1, 1, x.shape) if post else None
    skip = rng.uniform(-0.5, 0.5, channels) if has_skip else None
    h = rng.standard_normal((channels, taps))
    h /= np.abs(h).sum(axis=1, keepdims=True)
    got = gs.model(x, h, p, g, skip)
    u = x if p is None else p * x
    for b in range(rows):
        for c in range(channels):
            z = np.convolve(u[b, c], h[c])[:length] + (skip[c] * u[b, c] if has_skip else 0.0)
            want = z if g is None else g[b, c] * z
            assert np.abs(got[b, c] - want).max() <= 1e-12, (b, c)
    halo, hop, segs = sr.geometry(length, taps)
    hs = h.copy()
    if has_skip:
        hs[:, 0] += skip
    spec = np.fft.fft(hs, 4096, axis=-1)
    if pre and halo and length > halo:
        # the pre gate taken at the window sample: window sample w of segment s times p[s * hop + w] instead of p[s * hop - halo + w]
        p_shift = np.zeros_like(p)
        p_shift[:, :, :length - halo] = p[:, :, halo:]
        (x_re, x_im), (p_re, p_im) = sr.windows(x, taps), sr.windows(p_shift, taps)
        y = np.fft.ifft(np.fft.fft(x_re * p_re + 1j * x_im * p_im, axis=-1) * spec[np.arange(x_re.shape[0]) % channels], axis=-1)
        wrong = sr.unwindow(y.real, y.imag, rows, channels, length, taps)
        assert np.abs((wrong if g is None else g * wrong) - got).max() > 1e-3
    if post and halo and length > halo:
        # the post gate taken at the window sample: output sample t times g[t + halo] instead of g[t]
        z = gs.model(x, h, p, None, skip)
        g_shift = np.zeros_like(g)
        g_shift[:, :, :length - halo] = g[:, :, halo:]
        assert np.abs(g_shift * z - got).max() > 1e-3


def test_range_contract_and_spectrum_rounding():
    """Over the cases, tap kinds and gate modes of the GPU tests (seed 1), per window: max |U_k| |H'_k| stays a factor 64 inside the
    32752 of the range contract, |g z| <= |z| because |g| <= 1, and the rounding of H' to binary16 alone (fp64 with
    gconv_spectrum_host's n = 4096 spectrum against fp64 with the taps and the skip) stays inside the allowance the comparison with
    the true result grants for it: 1 ulp of the window's peak and rel-L2 2^-11. Measured on the CPU for exactly these cases, kinds
    and modes: max |U H'| = 235.7, 0.725 ulp, rel-L2 2.39e-4; the test asserts the allowances, not these figures."""
    big = worst = worst_rel = 0.0
    for length, taps, rows, channels, _, mode in gs.CASE_MODES:
        for kind in gs.TAP_KINDS:
            x, h, p, g, skip = gs.case_data(length, taps, rows, channels, kind, 1, mode)
            assert all(t is None or (t.shape == x.shape and t.dtype == np.float16 and np.abs(t).max() <= 1.0) for t in (p, g))
            u = gs.gated_input(x, p)
            spec = [tf.gconv_spectrum_host(h[c], 4096, None if skip is None else skip[c]) for c in range(channels)]
            h_re, h_im = np.stack([s[0] for s in spec]), np.stack([s[1] for s in spec])
            true = gs.reference_true(u, h, skip)
            ref = gs.reference_spectrum(u, taps, h_re, h_im)
            re, im = sr.windows(u.astype(np.float64), taps)
            big = max(big, np.abs(np.fft.fft(re + 1j * im, axis=-1) * (h_re.astype(np.float64) + 1j * h_im)[np.arange(re.shape[0]) % channels]).max())
            a, b = sr.kept(true, rows, channels, length, taps), sr.kept(ref, rows, channels, length, taps)
            unit = 2.0 ** (np.floor(np.log2(np.maximum(sr.window_peak(true), 2.0 ** -14))) - 10)
            worst = max(worst, (np.maximum(np.abs((a - b).real), np.abs((a - b).imag)) / unit[:, None]).max())
            den = np.sqrt((np.abs(a) ** 2).sum(-1))
            worst_rel = max(worst_rel, (np.sqrt((np.abs(a - b) ** 2).sum(-1))[den > 0] / den[den > 0]).max())
    print(f"max |U H'| = {big:.1f}; rounding of H' alone: {worst:.3f} ulp of the window's peak, rel-L2 {worst_rel:.2e}")
    assert big <= 32752 / 64, big
    assert worst <= 1.0 and worst_rel <= 2.0 ** -11, (worst, worst_rel)
