"""STFT add-on (include/tfft_stft.h, libtfft_stft.so) on the host: the exported symbols, the one kernel and the gfx950 ISA of its code
object (tools/isa_lint.py, the rules tests/test_sconv_host.py holds libtfft_sconv.so to), the geometry and the description, every
refusal that needs no device, the framing of tests/stft_ref.py against torch.stft in float64, and what the binary16 rounding of
the products w * x costs."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import stft_ref as st
import tensor_fft_amd as tf

stft = importlib.import_module("tensor_fft_amd.stft")      # the module: tensor_fft_amd.stft is the function of the same name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_ARG = 5


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def test_header_library_and_binding_name_the_same_symbols():
    header = open(os.path.join(ROOT, "include", "tfft_stft.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                # declarations only: the comments name calls too
    declared = set(re.findall(r"\b(tfft_stft_[a-z0-9_]+)\s*\(", code))
    assert declared == set(stft.SYMBOLS), declared ^ set(stft.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", stft.stft_lib_path()], capture_output=True, text=True, check=True).stdout
    text_syms = {line.split()[2] for line in nm.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    # -fvisibility=hidden: nothing but the entry points is exported as code
    assert text_syms == declared, text_syms ^ declared
    lib = stft.load_stft_library()
    for name in declared:
        assert hasattr(lib, name), name
    names = {"StftOpts", "TfftStftPlan", "load_stft_library", "stft", "stft_cache_clear", "stft_describe", "stft_geometry"}
    assert set(tf.__all__) >= names and all(hasattr(tf, n) for n in names)
    assert tf.stft is stft.stft and tf.TfftStftPlan is stft.TfftStftPlan


def test_library_links_the_other_two_and_no_sibling():
    import __graft_entry__ as g

    dyn = subprocess.run(["readelf", "-d", stft.stft_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "libtfft_conv.so" in dyn and "libtfft.so" in dyn and "$ORIGIN" in dyn
    assert g.ADDONS == ("conv", "lconv", "gconv", "sconv", "bconv", "gsconv", "gbconv", "cconv", "gcconv", "stft", "istft", "stftn", "istftn")
    for other in g.ADDONS:
        if other not in ("conv", "stft"):
            assert "libtfft_" + other + ".so" not in dyn, other


def test_opts_struct_size_is_the_headers():
    """sizeof(tfft_stft_opts) as the C compiler lays the header's struct out"""
    tmp = tempfile.mkdtemp(prefix="tfft_stft_size_")
    try:
        src = os.path.join(tmp, "size.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include "tfft_stft.h"\nint main(void) { tfft_stft_opts o = TFFT_STFT_OPTS_INIT; '
                    'printf("%u %u %d %d %d\\n", (unsigned)sizeof(o), o.struct_size, TFFT_STFT_N, TFFT_STFT_BINS, TFFT_STFT_PITCH); return 0; }\n')
        exe = os.path.join(tmp, "size")
        subprocess.check_call([shutil.which("cc") or "gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        out = subprocess.check_output([exe], text=True).split()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert [int(v) for v in out] == [ctypes.sizeof(stft.StftOpts), ctypes.sizeof(stft.StftOpts), stft.STFT_N, stft.STFT_BINS, stft.STFT_PITCH]
    assert ctypes.sizeof(stft.StftOpts) == 32 and (st.N, st.BINS, st.PITCH) == (stft.STFT_N, stft.STFT_BINS, stft.STFT_PITCH)
    assert tf.rplan_spectrum_pitch(4096) == stft.STFT_PITCH


@pytest.fixture(scope="module")
def report():
    import isa_lint

    return isa_lint.lint_text(isa_lint.disassemble(stft.stft_lib_path()))


def test_code_object_holds_exactly_the_one_kernel(report):
    assert len(report) == 1, list(report)
    names = subprocess.run(["c++filt"], input="\n".join(report), capture_output=True, text=True, check=True).stdout.split("\n")
    assert {n.strip().split("(")[0] for n in names if n.strip()} == {"stft4096::stft4096_kernel"}
    kernel = next(iter(report.values()))
    # one transform of 16 stage-1 tiles and 16 stage-2/3 tiles, two MFMAs per complex product: fft4096_kernel's count
    assert kernel["mfma"] == 16 * 2 + 16 * 4 == 96
    # everything comes in through registers: no LDS-DMA at all
    assert kernel["lds_dma"] == 0


def test_no_packed_fp32_and_no_lint_finding(report):
    kernel = next(iter(report.values()))
    assert kernel["pk_f32"] == 0
    assert not kernel["findings"], kernel["findings"]


def test_kernel_resources():
    """no scratch, no spills and at most 256 VGPRs (the window's 32 registers included), from the kernel metadata notes"""
    import isa_lint

    tmp = tempfile.mkdtemp(prefix="tfft_stft_isa_")
    try:
        local = os.path.join(tmp, "libtfft_stft.so")
        shutil.copy(stft.stft_lib_path(), local)
        subprocess.check_call([os.path.join(isa_lint.LLVM_BIN, "llvm-objdump"), "--offloading", local], cwd=tmp,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f][0]
        notes = subprocess.check_output([os.path.join(isa_lint.LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(tmp, co)], text=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    blocks = [b for b in notes.split("- .agpr_count") if "stft4096_kernel" in b]
    assert len(blocks) == 1
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", blocks[0]).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blocks[0]).group(1))
    spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blocks[0]).group(1))
    sgpr_spills = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blocks[0]).group(1))
    print(f"stft4096_kernel: {vgprs} VGPRs, scratch {scratch}, spills {spills} / {sgpr_spills}")
    assert scratch == 0 and spills == 0 and sgpr_spills == 0 and vgprs <= 256, (vgprs, scratch, spills, sgpr_spills)


@pytest.mark.parametrize("length,hop,pad,frames", st.GEOMETRY)
def test_geometry_and_describe(length, hop, pad, frames):
    assert tf.stft_geometry(length, hop, pad) == frames == st.geometry(length, hop, pad)
    assert tf.stft_describe(length, hop, pad, 3) == f"stft4096:4096 x {frames}"
    # the last frame ends inside the padded signal, and one more would not
    assert (frames - 1) * hop + 4096 <= length + 2 * pad < frames * hop + 4096
    # the pointer of tfft_stft_geometry may be NULL
    assert stft.load_stft_library().tfft_stft_geometry(length, hop, pad, None) == 0


def test_geometry_table_holds_what_the_gpu_cases_need():
    table = {g[:3]: g[3] for g in st.GEOMETRY}
    assert table[(8, 8, 2048)] == 2 and table[(4096, 8, 0)] == 1 and table[(4104, 8, 0)] == 2 and table[(8192, 2048, 2048)] == 5
    assert table[(4096, 512, 4088)] == 16 and table[(12288, 8192, 0)] == 2 and table[(1 << 26, 1024, 0)] == 65533
    for rows, length, hop, pad, _ in st.CASES:
        assert st.windows(np.zeros((rows, length), np.float16), hop, pad).shape == (rows * st.geometry(length, hop, pad), 4096)
    assert 4 * st.geometry(4416, 8, 0) == 164 and 3 * st.geometry(6144, 1024, 0) == 9


def _opts(**kw):
    o = stft.StftOpts(ctypes.sizeof(stft.StftOpts), 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("rows,length,hop,pad,flags,needle", [
    (1, 0, 8, 0, 0, "length must be a multiple of 8"), (1, 4, 8, 2048, 0, "length must be a multiple of 8"),
    (1, 4100, 8, 0, 0, "length must be a multiple of 8"), (1, (1 << 26) + 8, 1024, 0, 0, "2^26"),
    (1, 8192, 0, 0, 0, "hop must be"), (1, 8192, 4, 0, 0, "hop must be"), (1, 8192, 1028, 0, 0, "hop must be"),
    (1, 8192, 1024, 4, 0, "pad must be"), (1, 8192, 1024, 4096, 0, "pad must be"), (1, 8192, 1024, 1 << 20, 0, "pad must be"),
    (1, 4088, 8, 0, 0, "length + 2 * pad"), (1, 8, 8, 2040, 0, "length + 2 * pad"),
    (0, 8192, 1024, 0, 0, "rows"), (1 << 32, 8192, 1024, 0, 0, "rows"),
    (1 << 20, 1 << 26, 8, 0, 0, "frame count"), ((1 << 32) - 1, 4104, 8, 0, 0, "frame count"),
    (1, 8192, 1024, 0, 1, "flag"), (1, 8192, 1024, 0, -1, "flag"),
])
def test_describe_and_create_refuse_with_a_message(rows, length, hop, pad, flags, needle):
    lib = stft.load_stft_library()
    buf = ctypes.create_string_buffer(256)
    assert lib.tfft_stft_describe(length, hop, pad, rows, flags, buf, len(buf)) == ERR_ARG
    assert needle in lib.tfft_stft_last_error().decode()
    h = ctypes.c_void_p()
    o = _opts(flags=flags)
    assert lib.tfft_stft_plan_create(rows, length, hop, pad, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG    # before any device call
    assert needle in lib.tfft_stft_last_error().decode() and not h.value


@pytest.mark.parametrize("length,hop,pad,needle", [(0, 8, 0, "length"), (12, 8, 2048, "length"), (8192, 12, 0, "hop"), (8192, 8, 4096, "pad"),
                                                   (8, 8, 0, "length + 2 * pad"), ((1 << 26) + 8, 8, 0, "2^26")])
def test_geometry_refuses_what_create_refuses(length, hop, pad, needle):
    lib = stft.load_stft_library()
    frames = ctypes.c_uint64(77)
    assert lib.tfft_stft_geometry(length, hop, pad, ctypes.byref(frames)) == ERR_ARG and frames.value == 77
    assert needle in lib.tfft_stft_last_error().decode()
    with pytest.raises(tf.TfftError):
        tf.stft_geometry(length, hop, pad)


@pytest.mark.parametrize("rows,kw,needle", [
    (4, dict(in_sig_stride=8184), "in_sig_stride"), (4, dict(in_sig_stride=8196), "in_sig_stride"),
    (4, dict(out_frame_stride=2048), "out_frame_stride"), (4, dict(out_frame_stride=2060), "out_frame_stride"), (4, dict(out_frame_stride=8), "out_frame_stride"),
    # 32-bit item arithmetic carries the frame index; the byte extents must fit 64 bits
    (1 << 29, dict(in_sig_stride=1 << 40), "input extent"), (1 << 28, dict(out_frame_stride=1 << 40), "output extent"),
    (4, dict(struct_size=0), "struct_size"), (4, dict(struct_size=24), "struct_size"), (4, dict(struct_size=40), "struct_size"),
    (4, dict(reserved_=1), "reserved_"), (4, dict(launch_iters=65536), "launch_iters"),
    (4, dict(flags=1), "flags must be 0"), (4, dict(flags=1 << 30), "flags must be 0"),
])
def test_create_refuses_bad_options(rows, kw, needle):
    lib = stft.load_stft_library()
    h = ctypes.c_void_p()
    o = _opts(**kw)
    assert lib.tfft_stft_plan_create(rows, 8192, 1024, 0, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG
    assert needle in lib.tfft_stft_last_error().decode() and not h.value


def test_null_arguments_are_refused():
    lib = stft.load_stft_library()
    assert lib.tfft_stft_plan_create(1, 4096, 8, 0, 0, None, None) == ERR_ARG
    assert lib.tfft_stft_describe(4096, 8, 0, 1, 0, None, 0) == ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert lib.tfft_stft_describe(4096, 8, 0, 1, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_stft_exec(None, None, None, None, None) == ERR_ARG
    assert lib.tfft_stft_plan_set_window(None, None, None) == ERR_ARG
    assert lib.tfft_stft_plan_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_stft_plan_num_launches(None) == 0
    lib.tfft_stft_plan_destroy(None)
    assert lib.tfft_stft_last_error().decode()


def test_no_gpu_means_errors_not_fallbacks():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(tf.TfftError):
        tf.TfftStftPlan(2, 8192, 1024, 0)
    with pytest.raises(tf.TfftError):
        tf.stft(torch.zeros((2, 8192), dtype=torch.float16), torch.zeros(4096, dtype=torch.float16), 1024)


@pytest.mark.parametrize("length,hop,pad", [(6144, 1024, 0), (11264, 1024, 0), (8192, 2048, 2048), (4096, 512, 2048), (12288, 8192, 0), (4104, 8, 0)])
def test_framing_against_torch_stft(length, hop, pad):
    """stft_ref.windows against torch.stft in float64 on the CPU: pad 0 is center=False, pad 2048 is center=True with constant
    padding. A random window: a symmetric one hides a reversed frame."""
    import torch

    rows = 3
    rng = np.random.default_rng([length, hop, pad])
    x = rng.uniform(-1, 1, (rows, length))
    w = rng.uniform(0, 1, 4096)
    got = np.fft.rfft(st.windows(x, hop, pad) * w[None, :], axis=-1).reshape(rows, -1, st.BINS) / 4096
    kw = dict(center=False) if pad == 0 else dict(center=True, pad_mode="constant")
    want = torch.stft(torch.from_numpy(x), 4096, hop_length=hop, window=torch.from_numpy(w), return_complex=True, **kw).numpy() / 4096
    assert want.shape == (rows, st.BINS, st.geometry(length, hop, pad))           # bin-major; the plans are frame-major
    worst = np.abs(got - want.transpose(0, 2, 1)).max()
    print(f"framing L={length} hop={hop} pad={pad}: max |difference| = {worst:.2e}")
    assert worst <= 1e-12


def test_frames_round_each_product_once():
    """stft_ref.frames is the binary16 product, correctly rounded, subnormals kept; zeros outside the signal"""
    x, w = st.case_data(2, 8192, window="random")
    x[0, :64] = np.float16(6e-5) * x[0, :64]                      # products in the subnormal range
    u = st.frames(x, w, 2048, 2048)
    exact = st.windows(x.astype(np.float64), 2048, 2048) * w.astype(np.float64)[None, :]
    assert np.array_equal(u.view(np.uint16), exact.astype(np.float16).view(np.uint16))      # fp64 -> fp16 of an exact product: one rounding
    assert (u[0, 2048:2112] != 0).any() and (np.abs(u[0, 2048:2112]) < 6.2e-5).all()
    assert not u[0, :2048].any() and not u[4, 2048:].any() and u[4, :2048].any()


def test_product_rounding_stays_inside_the_allowance():
    """What tests/test_gpu_stft.py grants the comparison with fp64 of the UNROUNDED products on top of the transform's own bound:
    rounding the products to binary16 moves a frame's half spectrum by at most 2^-10 in rel-L2. Parseval: each normal product is
    off by at most 2^-11 relative, so the full spectrum moves by at most 2^-11 in rel-L2; a factor sqrt(2) covers the half spectrum,
    which counts its two edge bins once and every other bin of a conjugate pair once instead of twice. Measured on uniform(-1, 1)
    samples under the binary16 Hann window: 2.0e-4."""
    worst = 0.0
    for rows, length, hop, pad in ((3, 6144, 1024, 0), (4, 11264, 1024, 0)):
        x, w = st.case_data(rows, length)
        rounded = np.fft.rfft(st.frames(x, w, hop, pad).astype(np.float64), axis=-1)
        exact = np.fft.rfft(st.windows(x.astype(np.float64), hop, pad) * w.astype(np.float64)[None, :], axis=-1)
        worst = max(worst, st.rel_l2(rounded, exact).max())
    print(f"rounding of the products alone: rel-L2 {worst:.2e} of a frame's half spectrum")
    assert worst <= 2.0 ** -10
