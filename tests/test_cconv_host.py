"""Carried convolution add-on (include/tfft_cconv.h, libtfft_cconv.so) on the host: the exported symbols, the four kernels and the
gfx950 ISA of its code object (tools/isa_lint.py, what tests/test_sconv_host.py and tests/test_bconv_host.py hold the originals
to), the geometry and the descriptions, every refusal that needs no device, and the windows with a history and a future in pure
numpy: against numpy.convolve and direct sums, and against the concatenations that tests/test_gpu_cconv.py runs through the
shipped plans."""
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
import cconv_ref as cr
import lconv_ref as lr
import sconv_ref as sr
import tensor_fft_amd as tf
from tensor_fft_amd import cconv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_ARG = 5
KERNELS = ("cconv4096_kernel", "dgrad_kernel", "wgrad_kernel", "wreduce_kernel")


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def test_header_library_and_binding_name_the_same_symbols():
    header = open(os.path.join(ROOT, "include", "tfft_cconv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                # declarations only: the comments name calls too
    declared = set(re.findall(r"\b(tfft_cconv_[a-z0-9_]+)\s*\(", code))
    assert declared == set(cconv.SYMBOLS), declared ^ set(cconv.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", cconv.cconv_lib_path()], capture_output=True, text=True, check=True).stdout
    text_syms = {line.split()[2] for line in nm.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    # -fvisibility=hidden: nothing but the entry points is exported as code
    assert text_syms == declared, text_syms ^ declared
    lib = cconv.load_cconv_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert set(tf.__all__) >= {"TfftChunkedConvPlan", "TfftChunkedConvGradPlan", "cconv_geometry", "cconv_describe", "cconv_cache_clear",
                               "chunked_causal_conv", "chunked_causal_conv_input_grad", "chunked_causal_conv_tap_grad", "next_history",
                               "differentiable_chunked_causal_conv"}


def test_library_links_the_other_two_only():
    dyn = subprocess.run(["readelf", "-d", cconv.cconv_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "libtfft_conv.so" in dyn and "libtfft.so" in dyn and "$ORIGIN" in dyn
    ours = set(re.findall(r"\[(libtfft[a-z_]*\.so)\]", dyn))
    assert ours == {"libtfft_conv.so", "libtfft.so"}, ours


def test_option_structs_match_the_header():
    """tfft_sconv_opts (32 bytes) + two uint64; tfft_bconv_opts (48 bytes, its int padded to 8) + four uint64. The compiler that
    builds the library lays the header out the same way."""
    assert ctypes.sizeof(cconv.CconvOpts) == 48 and cconv.CconvOpts.history.offset == 32 and cconv.CconvOpts.hist_seq_stride.offset == 40
    assert ctypes.sizeof(cconv.CconvGradOpts) == 80 and cconv.CconvGradOpts.partials.offset == 36 and cconv.CconvGradOpts.flags.offset == 40
    assert [getattr(cconv.CconvGradOpts, f).offset for f in ("history", "hist_seq_stride", "future", "fut_seq_stride")] == [48, 56, 64, 72]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:
        tmp = tempfile.mkdtemp(prefix="tfft_cconv_sizeof_")
        try:
            src = os.path.join(tmp, "s.c")
            with open(src, "w") as f:
                f.write('#include <stdio.h>\n#include "tfft_cconv.h"\nint main(void) { printf("%zu %zu\\n", sizeof(tfft_cconv_opts), '
                        'sizeof(tfft_cconv_grad_opts)); return 0; }\n')
            subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", os.path.join(tmp, "s"), src])
            out = subprocess.check_output([os.path.join(tmp, "s")], text=True).split()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        assert [int(v) for v in out] == [ctypes.sizeof(cconv.CconvOpts), ctypes.sizeof(cconv.CconvGradOpts)]


@pytest.fixture(scope="module")
def report():
    import isa_lint

    rep = isa_lint.lint_text(isa_lint.disassemble(cconv.cconv_lib_path()))
    names = subprocess.run(["c++filt"], input="\n".join(rep), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n.strip().split("(")[0]: r for n, r in zip(names, rep.values())}


def test_code_object_holds_exactly_the_four_kernels(report):
    assert set(report) == {"cconv4096::" + k for k in KERNELS}, list(report)
    # the counts of the originals (tests/test_sconv_host.py, tests/test_bconv_host.py): two transforms and one LDS-DMA per 1-KiB
    # block and plane; the context is a select on the DMA's address, not a second DMA
    for k in ("cconv4096_kernel", "dgrad_kernel"):
        assert report["cconv4096::" + k]["mfma"] == 2 * (16 * 2 + 16 * 4) == 192, k
        assert report["cconv4096::" + k]["lds_dma"] == 16, k
    assert report["cconv4096::wgrad_kernel"]["mfma"] == 3 * (16 * 2 + 16 * 4) == 288
    assert report["cconv4096::wgrad_kernel"]["lds_dma"] == 32
    assert report["cconv4096::wreduce_kernel"]["mfma"] == 0 and report["cconv4096::wreduce_kernel"]["lds_dma"] == 0


def test_no_packed_fp32_wait_states_and_dma_drain(report):
    for name, kernel in report.items():
        assert kernel["pk_f32"] == 0, name
        assert not kernel["findings"], (name, kernel["findings"])


def test_kernel_resources():
    """no scratch and no spills in any kernel, within the register budgets of the originals (tests/test_bconv_host.py)"""
    import isa_lint

    tmp = tempfile.mkdtemp(prefix="tfft_cconv_isa_")
    try:
        local = os.path.join(tmp, "libtfft_cconv.so")
        shutil.copy(cconv.cconv_lib_path(), local)
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


GEOMETRY = [(c[0], c[1]) for c in cr.CASES] + [(4032, 2), (4040, 65), (16384, 2049), (16384, 128), (1 << 26, 2049)]


@pytest.mark.parametrize("length,taps", GEOMETRY)
def test_geometry_and_describe(length, taps):
    lib = cconv.load_cconv_library()
    halo, hop, segments = sr.geometry(length, taps)
    out = [ctypes.c_uint64() for _ in range(4)]
    assert lib.tfft_cconv_geometry(length, taps, *[ctypes.byref(o) for o in out]) == 0
    assert tuple(o.value for o in out) == (halo, hop, segments, cr.carry_min(taps))
    assert cr.carry_min(taps) % 8 == 0 and taps - 1 <= cr.carry_min(taps) < taps + 7 and cr.carry_min(taps) <= halo
    assert lib.tfft_cconv_geometry(length, taps, None, None, None, None) == 0
    assert tf.sconv_geometry(length, taps) == (halo, hop, segments)
    for rows, channels, cap in ((3, 2, 0), (1, 1, 0), (5, 3, 2), (64, 256, 0), (2, 4096, 1)):
        p = br.partials_of(rows, channels, length, taps, cap)
        assert tf.cconv_geometry(length, taps, rows, channels, cap) == (halo, hop, segments, p, cr.carry_min(taps))
        assert tf.cconv_geometry(length, taps, rows, channels, cap)[:4] == tf.bconv_geometry(length, taps, rows, channels, cap)
        assert tf.cconv_describe(length, taps, rows, channels, cap) == (f"cconv4096:4096 x {segments}", f"cconv4096:4096 x {segments} | partials {p}")
    one = ctypes.c_uint64()
    assert lib.tfft_cconv_grad_geometry(length, taps, 3, 2, 0, None, None, None, None, ctypes.byref(one)) == 0 and one.value == cr.carry_min(taps)


def test_cases_cover_what_they_say():
    by = {c[:2]: c for c in cr.CASES}
    geo = {k: sr.geometry(*k) for k in by}
    assert geo[(8, 1)][0] == 0 and by[(8, 1)][4] == 0
    assert geo[(8, 9)] == (64, 4032, 1) and by[(8, 9)][4] == 8 == cr.carry_min(9) < 64                  # zeros in front of the context
    assert geo[(2048, 2049)] == (2048, 2048, 1) and by[(2048, 2049)][4] == 2048 and by[(2048, 2049)][2] % 2 == 1
    assert geo[(4104, 7)][0] == 64 and by[(4104, 7)][4] == 8                                             # block 0: 7 chunks of zeros, 1 of context, 56 of x
    assert geo[(6152, 130)][0] == 192 and by[(6152, 130)][4] == cr.carry_min(130) == 136
    assert by[(4096, 2049)][4] == 1024 < 2048 and geo[(8064, 65)] == (64, 4032, 2) and geo[(12288, 65)][2] == 4
    for length, taps, _, _, ctx, _ in cr.CASES:
        assert ctx % 8 == 0 and ctx <= geo[(length, taps)][0]


def _opts(**kw):
    o = cconv.CconvOpts(ctypes.sizeof(cconv.CconvOpts), 0, 0, 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _gopts(**kw):
    o = cconv.CconvGradOpts(ctypes.sizeof(cconv.CconvGradOpts), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _refused(rc, needle, handle=None):
    lib = cconv.load_cconv_library()
    msg = lib.tfft_cconv_last_error().decode()
    assert rc == ERR_ARG and needle in msg and msg, (rc, needle, msg)
    assert handle is None or not handle.value


# everything tfft_sconv_plan_create and tfft_bconv_plan_create refuse (tests/test_sconv_host.py), with their messages
@pytest.mark.parametrize("rows,channels,length,taps,flags,needle", [
    (1, 1, 0, 1, 0, "multiple of 8"), (1, 1, 4, 1, 0, "multiple of 8"), (1, 1, 4100, 1, 0, "multiple of 8"),
    (1, 1, 8, 0, 0, "taps must be at least 1"), (1, 1, 8, 2050, 0, "tfft_lconv_plan_create"), (1, 1, 16384, 1 << 20, 0, "tfft_lconv_plan_create"),
    (0, 1, 8, 1, 0, "rows"), (1 << 32, 1, 8, 1, 0, "rows"), (1, 0, 8, 1, 0, "channels"),
    (1 << 16, 1 << 16, 8, 1, 0, "rows * channels"), (1, 1, 8, 1, 1, "flag"), (1, 1, 8, 1, -1, "flag"),
    (1, 1, (1 << 26) + 8, 2, 0, "2^26"), (1 << 20, 1 << 10, 1 << 20, 2049, 0, "item count"),
])
def test_describe_and_create_refuse_with_a_message(rows, channels, length, taps, flags, needle):
    lib = cconv.load_cconv_library()
    buf = ctypes.create_string_buffer(256)
    _refused(lib.tfft_cconv_describe(length, taps, rows, channels, flags, buf, len(buf)), needle)
    _refused(lib.tfft_cconv_grad_describe(length, taps, rows, channels, 0, flags, buf, len(buf)), needle)
    h = ctypes.c_void_p()
    _refused(lib.tfft_cconv_plan_create(rows, channels, length, taps, 0, ctypes.byref(_opts(flags=flags)), ctypes.byref(h)), needle, h)
    _refused(lib.tfft_cconv_grad_create(rows, channels, length, taps, 0, ctypes.byref(_gopts(flags=flags)), ctypes.byref(h)), needle, h)


@pytest.mark.parametrize("length,taps,needle", [(0, 1, "multiple of 8"), (12, 1, "multiple of 8"), (8, 0, "taps"), (8, 2050, "tfft_lconv_plan_create"),
                                                ((1 << 26) + 8, 1, "2^26")])
def test_geometry_refuses_what_create_refuses(length, taps, needle):
    lib = cconv.load_cconv_library()
    halo = ctypes.c_uint64(77)
    _refused(lib.tfft_cconv_geometry(length, taps, ctypes.byref(halo), None, None, None), needle)
    _refused(lib.tfft_cconv_grad_geometry(length, taps, 1, 1, 0, ctypes.byref(halo), None, None, None, None), needle)
    assert halo.value == 77
    with pytest.raises(tf.TfftError):
        tf.cconv_geometry(length, taps)


# (4, 2, 8192, 130): halo 192
@pytest.mark.parametrize("kw,needle", [
    (dict(in_seq_stride=8184), "in_seq_stride"), (dict(in_seq_stride=8196), "in_seq_stride"), (dict(out_seq_stride=8), "out_seq_stride"),
    (dict(struct_size=0), "struct_size"), (dict(struct_size=32), "struct_size"), (dict(struct_size=56), "struct_size"),
    (dict(reserved_=1), "reserved_"), (dict(launch_iters=65536), "launch_iters"), (dict(flags=1), "flags must be 0"),
    (dict(history=4), "history must be a multiple of 8"), (dict(history=129), "history must be a multiple of 8"),
    (dict(history=200), "history must not exceed the halo"), (dict(history=1 << 40), "history must not exceed the halo"),
    (dict(history=136, hist_seq_stride=128), "hist_seq_stride"), (dict(history=136, hist_seq_stride=140), "hist_seq_stride"),
    (dict(history=0, hist_seq_stride=4), "hist_seq_stride"),
])
def test_forward_create_refuses_bad_options(kw, needle):
    lib = cconv.load_cconv_library()
    h = ctypes.c_void_p()
    _refused(lib.tfft_cconv_plan_create(4, 2, 8192, 130, 0, ctypes.byref(_opts(**kw)), ctypes.byref(h)), needle, h)


@pytest.mark.parametrize("kw,needle", [
    (dict(x_seq_stride=8184), "x_seq_stride"), (dict(g_seq_stride=8196), "g_seq_stride"), (dict(dx_seq_stride=8), "dx_seq_stride"),
    (dict(struct_size=0), "struct_size"), (dict(struct_size=48), "struct_size"), (dict(struct_size=88), "struct_size"),
    (dict(reserved_=1), "reserved_"), (dict(launch_iters=65536), "launch_iters"), (dict(flags=1 << 30), "flags must be 0"),
    (dict(history=4), "history must be a multiple of 8"), (dict(history=200), "history must not exceed the halo"),
    (dict(history=136, hist_seq_stride=128), "hist_seq_stride"), (dict(history=136, hist_seq_stride=140), "hist_seq_stride"),
    (dict(future=12), "future must be a multiple of 8"), (dict(future=256), "future must not exceed the halo"),
    (dict(future=136, fut_seq_stride=128), "fut_seq_stride"), (dict(future=192, fut_seq_stride=196), "fut_seq_stride"),
])
def test_grad_create_refuses_bad_options(kw, needle):
    lib = cconv.load_cconv_library()
    h = ctypes.c_void_p()
    _refused(lib.tfft_cconv_grad_create(4, 2, 8192, 130, 0, ctypes.byref(_gopts(**kw)), ctypes.byref(h)), needle, h)


def test_a_context_at_halo_0_is_refused():
    lib = cconv.load_cconv_library()
    h = ctypes.c_void_p()
    _refused(lib.tfft_cconv_plan_create(1, 1, 8, 1, 0, ctypes.byref(_opts(history=8)), ctypes.byref(h)), "history must not exceed the halo", h)
    _refused(lib.tfft_cconv_grad_create(1, 1, 8, 1, 0, ctypes.byref(_gopts(future=8)), ctypes.byref(h)), "future must not exceed the halo", h)


def test_null_arguments_are_refused():
    lib = cconv.load_cconv_library()
    assert lib.tfft_cconv_plan_create(1, 1, 8, 1, 0, None, None) == ERR_ARG
    assert lib.tfft_cconv_grad_create(1, 1, 8, 1, 0, None, None) == ERR_ARG
    assert lib.tfft_cconv_describe(8, 1, 1, 1, 0, None, 0) == ERR_ARG
    assert lib.tfft_cconv_grad_describe(8, 1, 1, 1, 0, 0, None, 0) == ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert lib.tfft_cconv_describe(8, 1, 1, 1, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_cconv_grad_describe(8, 1, 1, 1, 0, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_cconv_exec(None, None, None, None, None) == ERR_ARG
    assert lib.tfft_cconv_plan_set_taps(None, None, None) == ERR_ARG
    assert lib.tfft_cconv_plan_spectrum(None, None, None) == ERR_ARG
    assert lib.tfft_cconv_plan_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_cconv_plan_num_launches(None) == 0
    lib.tfft_cconv_plan_destroy(None)
    assert lib.tfft_cconv_grad_exec_input_grad(None, None, None, None, None) == ERR_ARG
    assert lib.tfft_cconv_grad_exec_tap_grad(None, None, None, None, None, None) == ERR_ARG
    assert lib.tfft_cconv_grad_set_taps(None, None, None) == ERR_ARG
    assert lib.tfft_cconv_grad_spectrum(None, None, None) == ERR_ARG
    assert lib.tfft_cconv_grad_set_workspace(None, None, 0) == ERR_ARG
    assert lib.tfft_cconv_grad_prepare(None) == ERR_ARG
    assert lib.tfft_cconv_grad_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_cconv_grad_workspace_bytes(None) == 0 and lib.tfft_cconv_grad_num_launches(None) == 0
    lib.tfft_cconv_grad_destroy(None)
    assert lib.tfft_cconv_last_error().decode()


def test_no_gpu_means_errors_not_fallbacks():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(tf.TfftError):
        tf.TfftChunkedConvPlan(4, 2, 16384, 2049, 0, history=2048)
    with pytest.raises(tf.TfftError):
        tf.TfftChunkedConvGradPlan(1, 1, 8, 9, 0, history=8, future=8)
    with pytest.raises(tf.TfftError):
        tf.chunked_causal_conv(torch.zeros((2, 2, 4096), dtype=torch.float16), torch.zeros((2, 7), dtype=torch.float16))


def test_next_history_is_a_view_when_the_chunk_is_long_enough():
    import torch

    x = torch.arange(2 * 3 * 32, dtype=torch.float32).reshape(2, 3, 32).to(torch.float16)
    v = tf.next_history(x, None, 16)
    assert v.data_ptr() == x.data_ptr() + 2 * 16 and torch.equal(v, x[..., 16:]) and v.stride() == x.stride()
    assert tf.next_history(x, None, 0) is None
    short = x[..., :8]
    hist = -x[..., :16]
    assert torch.equal(tf.next_history(short, hist, 16), torch.cat([hist[..., 8:], short], -1))
    assert torch.equal(tf.next_history(short, hist, 32), torch.cat([torch.zeros(2, 3, 8, dtype=torch.float16), hist, short], -1))
    assert torch.equal(tf.next_history(short, None, 16), torch.cat([torch.zeros(2, 3, 8, dtype=torch.float16), short], -1))


def _data(length, taps, rows, channels, ctx, seed=1):
    rng = np.random.default_rng([seed, length, taps, rows, channels, ctx])
    x = rng.uniform(-1, 1, (rows, channels, length))
    g = rng.uniform(-1, 1, (rows, channels, length))
    hist = rng.uniform(-1, 1, (rows, channels, ctx)) if ctx else None
    fut = rng.uniform(-1, 1, (rows, channels, ctx)) if ctx else None
    h = rng.standard_normal((channels, taps))
    h /= np.abs(h).sum(axis=1, keepdims=True)
    return x, g, hist, fut, h


@pytest.mark.parametrize("length,taps,rows,channels,ctx,_iters", cr.CASES)
def test_windows_against_numpy_convolve_and_direct_sums(length, taps, rows, channels, ctx, _iters):
    """pure numpy, fp64: the windows with a history / a future, convolved circularly and un-windowed with the helpers of
    tests/sconv_ref.py and tests/bconv_ref.py, are the definitions of include/tfft_cconv.h to 1e-13"""
    x, g, hist, fut, h = _data(length, taps, rows, channels, ctx)
    halo, hop, segs = sr.geometry(length, taps)
    idx = np.arange((rows + 1) // 2 * segs * channels) % channels
    spec = np.fft.fft(h, 4096, axis=-1)
    # forward
    re, im = cr.windows(x, taps, hist)
    assert np.array_equal(sr.unwindow(re, im, rows, channels, length, taps), x)
    if ctx:
        first = re.reshape(-1, segs, channels, 4096)[:, 0]
        assert not first[:, :, :halo - ctx].any() and np.array_equal(first[0, 0, halo - ctx:halo], hist[0, 0])
    y = np.fft.ifft(np.fft.fft(re + 1j * im, axis=-1) * spec[idx], axis=-1)
    got = sr.unwindow(y.real, y.imag, rows, channels, length, taps)
    want = cr.y_direct(x, h, hist)
    assert np.abs(got - want).max() <= 1e-13
    for b in range(rows):
        for c in range(channels):
            xe = x[b, c] if hist is None else np.concatenate([hist[b, c], x[b, c]])
            assert np.abs(got[b, c] - np.convolve(xe, h[c])[ctx:ctx + length]).max() <= 1e-13
    # input gradient
    re, im = cr.dx_windows(g, taps, fut)
    d = np.fft.ifft(np.fft.fft(re + 1j * im, axis=-1) * np.conj(spec)[idx], axis=-1)
    got = br.dx_unwindow(d.real, d.imag, rows, channels, length, taps)
    assert np.abs(got - cr.dx_direct(g, h, fut)).max() <= 1e-13
    ge = g if fut is None else np.concatenate([g, fut], axis=-1)
    brute = np.zeros_like(g)
    for j in range(taps):
        n = max(0, min(length, ge.shape[2] - j))
        brute[:, :, :n] += h[None, :, j, None] * ge[:, :, j:j + n]
    assert np.abs(got - brute).max() <= 1e-13
    # tap gradient: direct sums over 0 <= t < L of g[t] xe[t - j]. y and dx stay below 1 in magnitude; dh is a sum of up to B L
    # products and reaches several hundred, where one fp64 ulp is 5.7e-14: its 1e-13 is relative to the largest tap gradient
    items = cr.dh_items(x, g, taps, hist)
    dh = br.dh_from_items(items, channels, taps)
    dh_tol = 1e-13 * max(1.0, np.abs(dh).max())
    assert np.abs(dh - cr.dh_direct(x, g, taps, hist)).max() <= dh_tol
    xe = x if hist is None else np.concatenate([hist, x], axis=-1)
    for j in sorted({0, 1, taps // 2, taps - 1} & set(range(taps))):
        lo = max(0, j - ctx)                                                   # xe[t - j] exists for t - j >= -Hn
        want_j = np.einsum("bct,bct->c", g[:, :, lo:], xe[:, :, ctx + lo - j:ctx + length - j])
        assert np.abs(dh[:, j] - want_j).max() <= dh_tol, j
    # the history's gradient as the autograd hook composes it: the input gradient at length Hn on zeros with future g[:carry_min]
    if ctx:
        fn = min(length, cr.carry_min(taps))
        composed = cr.dx_direct(np.zeros_like(hist), h, g[:, :, :fn])
        assert np.abs(composed - cr.dhist_direct(g, h, ctx)).max() <= 1e-13
        # and it is the gradient: <dhist, e> = d/d eps of sum(g * y(hist + eps e)), y linear in hist
        e = np.random.default_rng(5).uniform(-1, 1, hist.shape)
        lin = (g * (cr.y_direct(x, h, hist + e) - cr.y_direct(x, h, hist))).sum()
        assert abs((composed * e).sum() - lin) <= 1e-10 * max(1.0, abs(lin))


@pytest.mark.parametrize("length,taps,rows,channels,ctx,_iters", cr.CASES)
def test_concatenation_identities(length, taps, rows, channels, ctx, _iters):
    """what tests/test_gpu_cconv.py runs through the shipped plans: the windows of the concatenated sequences equal the carried
    plan's own windows element for element"""
    x, g, hist, fut, h = _data(length, taps, rows, channels, ctx, seed=2)
    halo, hop, segs = sr.geometry(length, taps)
    pairs = (rows + 1) // 2
    # forward: segment s + 1 of [zeros(hop - Hn) | hist | x] at length hop + L is window s
    cat = cr.front_padded(x, hist, taps)
    assert cat.shape[2] == hop + length and sr.geometry(hop + length, taps) == (halo, hop, segs + 1)
    for mine, theirs in zip(cr.windows(x, taps, hist), sr.windows(cat, taps)):
        assert np.array_equal(mine.reshape(pairs, segs, channels, 4096), theirs.reshape(pairs, segs + 1, channels, 4096)[:, 1:])
    # input gradient: segment s of [g | fut] at length L + Fn is window s (any further segment there lies behind L)
    cat_g = cr.extend(g, fut=fut)
    segs_g = sr.geometry(length + ctx, taps)[2]
    assert segs_g >= segs
    for mine, theirs in zip(cr.dx_windows(g, taps, fut), br.dx_windows(cat_g, taps)):
        assert np.array_equal(mine.reshape(pairs, segs, channels, 4096), theirs.reshape(pairs, segs_g, channels, 4096)[:, :segs])
    # tap gradient: item (p, s + 1) of ([zeros(hop - Hn) | hist | x], [zeros(hop) | g]) is item (p, s); item (p, 0) there has Zg = 0
    cat_gz = cr.extend(g, np.zeros(g.shape[:2] + (hop,)))
    zx, zg = cr.dh_windows(x, g, taps, hist)
    zx2, zg2 = br.dh_windows(cat, cat_gz, taps)
    assert np.array_equal(zx.reshape(pairs, segs, channels, 4096), zx2.reshape(pairs, segs + 1, channels, 4096)[:, 1:])
    assert np.array_equal(zg.reshape(pairs, segs, channels, 4096), zg2.reshape(pairs, segs + 1, channels, 4096)[:, 1:])
    assert not zg2.reshape(pairs, segs + 1, channels, 4096)[:, 0].any()
    # with partials = 1 both sides add their items in increasing i = p * S + s, and the extra items add +0 to a sum that starts at +0
    assert br.partials_of(rows, channels, length, taps, 1) == br.partials_of(rows, channels, hop + length, taps, 1) == 1


def test_chunk_invariance_in_numpy():
    """three hop-aligned chunks with context = halo transform exactly the whole sequence's windows (forward and input gradient)"""
    taps, rows, channels, total = 65, 3, 2, 12096
    halo, hop, segs = sr.geometry(total, taps)
    assert (halo, hop, segs) == (64, 4032, 3)
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (rows, channels, total))
    whole_f, whole_b = sr.windows(x, taps), br.dx_windows(x, taps)
    pairs = (rows + 1) // 2
    for k in range(3):
        chunk = x[:, :, k * hop:(k + 1) * hop]
        hist = x[:, :, k * hop - halo:k * hop] if k else None
        fut = x[:, :, (k + 1) * hop:(k + 1) * hop + halo] if k < 2 else None
        for mine, theirs in zip(cr.windows(chunk, taps, hist), whole_f):
            assert np.array_equal(mine.reshape(pairs, channels, 4096), theirs.reshape(pairs, segs, channels, 4096)[:, k])
        for mine, theirs in zip(cr.dx_windows(chunk, taps, fut), whole_b):
            assert np.array_equal(mine.reshape(pairs, channels, 4096), theirs.reshape(pairs, segs, channels, 4096)[:, k])
