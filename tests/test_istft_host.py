"""ISTFT add-on (include/tfft_istft.h, libtfft_istft.so) on the host: the exported symbols, the two kernels of its code object and
the resources of the frames kernel, the geometry and the description, every refusal that needs no device, the overlap-add of
tests/istft_ref.py against torch.istft in float64, and the numpy round trip x -> STFT -> binary16 -> ISTFT -> x on every case of
tests/test_gpu_istft.py."""
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

import istft_ref as ir
import stft_ref as st
import tensor_fft_amd as tf

istft = importlib.import_module("tensor_fft_amd.istft")      # the module: tensor_fft_amd.istft is the function of the same name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_ARG = 5


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def test_header_library_and_binding_name_the_same_symbols():
    header = open(os.path.join(ROOT, "include", "tfft_istft.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                # declarations only: the comments name calls too
    declared = set(re.findall(r"\b(tfft_istft_[a-z0-9_]+)\s*\(", code))
    assert declared == set(istft.SYMBOLS), declared ^ set(istft.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", istft.istft_lib_path()], capture_output=True, text=True, check=True).stdout
    text_syms = {line.split()[2] for line in nm.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    # -fvisibility=hidden: nothing but the entry points is exported as code
    assert text_syms == declared, text_syms ^ declared
    lib = istft.load_istft_library()
    for name in declared:
        assert hasattr(lib, name), name
    names = {"IstftOpts", "TfftIstftPlan", "load_istft_library", "istft", "istft_cache_clear", "istft_describe", "istft_geometry"}
    assert set(tf.__all__) >= names and all(hasattr(tf, n) for n in names)
    assert tf.istft is istft.istft and tf.TfftIstftPlan is istft.TfftIstftPlan


def test_library_links_the_other_two_and_no_sibling():
    import __graft_entry__ as g

    dyn = subprocess.run(["readelf", "-d", istft.istft_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "libtfft_conv.so" in dyn and "libtfft.so" in dyn and "$ORIGIN" in dyn
    assert g.ADDONS == ("conv", "lconv", "gconv", "sconv", "bconv", "gsconv", "gbconv", "cconv", "gcconv", "stft", "istft", "stftn", "istftn")
    for other in g.ADDONS:
        if other not in ("conv", "istft"):
            assert "libtfft_" + other + ".so" not in dyn, other
    # the build table: the library is checked and built with the others, and the example links it
    assert dict(g.EXAMPLES)["example_istft"] == ("-ltfft_istft", "-ltfft_stft", "-ltfft_conv")
    assert os.path.join(ROOT, "include", "tfft_istft.h") in g._addon_sources("istft")
    assert os.path.exists(os.path.join(ROOT, "examples", "example_istft"))


def test_opts_struct_size_is_the_headers():
    """sizeof(tfft_istft_opts) as the C compiler lays the header's struct out"""
    tmp = tempfile.mkdtemp(prefix="tfft_istft_size_")
    try:
        src = os.path.join(tmp, "size.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include "tfft_istft.h"\nint main(void) { tfft_istft_opts o = TFFT_ISTFT_OPTS_INIT; '
                    'printf("%u %u %d %d %d %d\\n", (unsigned)sizeof(o), o.struct_size, TFFT_ISTFT_N, TFFT_ISTFT_BINS, TFFT_ISTFT_PITCH, '
                    'TFFT_ISTFT_RAW_SUM); return 0; }\n')
        exe = os.path.join(tmp, "size")
        subprocess.check_call([shutil.which("cc") or "gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        out = subprocess.check_output([exe], text=True).split()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    size = ctypes.sizeof(istft.IstftOpts)
    assert [int(v) for v in out] == [size, size, istft.ISTFT_N, istft.ISTFT_BINS, istft.ISTFT_PITCH, istft.ISTFT_RAW_SUM]
    assert size == 32 and (ir.N, ir.BINS, ir.PITCH) == (istft.ISTFT_N, istft.ISTFT_BINS, istft.ISTFT_PITCH)
    assert tf.rplan_spectrum_pitch(4096) == istft.ISTFT_PITCH


@pytest.fixture(scope="module")
def notes():
    """the metadata notes and the symbol table of the library's gfx950 code object"""
    from isa_lint import LLVM_BIN

    tmp = tempfile.mkdtemp(prefix="tfft_istft_co_")
    try:
        local = os.path.join(tmp, "libtfft_istft.so")
        shutil.copy(istft.istft_lib_path(), local)
        subprocess.check_call([os.path.join(LLVM_BIN, "llvm-objdump"), "--offloading", local], cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f]
        assert len(co) == 1, co
        text = subprocess.check_output([os.path.join(LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(tmp, co[0])], text=True)
        syms = subprocess.check_output([os.path.join(LLVM_BIN, "llvm-readelf"), "--symbols", "--wide", os.path.join(tmp, co[0])], text=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return text, syms


def test_code_object_holds_exactly_the_two_kernels(notes):
    _, syms = notes
    funcs = [line.split()[-1] for line in syms.splitlines() if " FUNC " in line]
    names = subprocess.run(["c++filt"], input="\n".join(funcs), capture_output=True, text=True, check=True).stdout.split("\n")
    # (the dynamic and the full symbol table both list them)
    assert {n.strip().split("(")[0] for n in names if n.strip()} == {"istft4096::frames_kernel", "istft4096::ola_kernel"}, names


def test_frames_kernel_resources(notes):
    """no scratch, no spills and at most 256 VGPRs, from the kernel metadata notes"""
    text, _ = notes
    blocks = [b for b in text.split("- .agpr_count") if "frames_kernel" in b]
    assert len(blocks) == 1
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", blocks[0]).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blocks[0]).group(1))
    spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blocks[0]).group(1))
    sgpr_spills = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blocks[0]).group(1))
    print(f"frames_kernel: {vgprs} VGPRs, scratch {scratch}, spills {spills} / {sgpr_spills}")
    assert scratch == 0 and spills == 0 and sgpr_spills == 0 and vgprs <= 256, (vgprs, scratch, spills, sgpr_spills)


@pytest.mark.parametrize("length,hop,pad,frames", st.GEOMETRY + [(6152, 1024, 0, 3)])
def test_geometry_and_describe(length, hop, pad, frames):
    assert tf.istft_geometry(length, hop, pad) == frames == st.geometry(length, hop, pad)
    assert tf.istft_describe(length, hop, pad, 3) == f"istft4096:4096 x {frames} + ola" == tf.istft_describe(length, hop, pad, 3, raw_sum=True)
    # the pointer of tfft_istft_geometry may be NULL
    assert istft.load_istft_library().tfft_istft_geometry(length, hop, pad, None) == 0


@pytest.mark.parametrize("rows,length,hop,pad,iters,window", ir.HUGE_HOP_CASES)
def test_one_frame_plans_take_any_hop(rows, length, hop, pad, iters, window):
    """hop is 64 bits wide and bounded only by its type where there is one frame per signal; the reference gives +0 behind the frame"""
    assert tf.istft_geometry(length, hop, pad) == 1 == st.geometry(length, hop, pad)
    assert tf.istft_describe(length, hop, pad, rows) == "istft4096:4096 x 1 + ola"
    w = st.case_data(rows, length, window=window)[1]
    v = np.ones((rows, ir.N), np.float16)
    y = ir.ola(v, w, rows, length, hop, pad)
    assert (y.view(np.uint16)[:, ir.N - pad:] == 0).all() and (y[:, :ir.N - pad] != 0).any()
    assert np.array_equal(y, ir.ola(v, w, rows, length, length + 2 * pad, pad))


def test_case_table_extends_the_stfts():
    table = {g[:3]: g[3] for g in st.GEOMETRY}
    for rows, length, hop, pad, _, _ in ir.CASES:
        if (length, hop, pad) in table:
            assert table[(length, hop, pad)] == st.geometry(length, hop, pad)
    # the STFT's cases and one more, the tail the last frame does not reach
    assert [c[:5] for c in ir.CASES if c[1] != 6152] == st.CASES and len(ir.CASES) == len(st.CASES) + 1
    assert 4 * st.geometry(4416, 8, 0) == 164 and 3 * st.geometry(6144, 1024, 0) == 9 and st.geometry(6152, 1024, 0) == 3


def _opts(**kw):
    o = istft.IstftOpts(ctypes.sizeof(istft.IstftOpts), 0, 0, 0, 0, 0)
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
    (1, 8192, 1024, 0, 2, "flag"), (1, 8192, 1024, 0, 3, "flag"), (1, 8192, 1024, 0, -1, "flag"),
])
def test_describe_and_create_refuse_with_a_message(rows, length, hop, pad, flags, needle):
    lib = istft.load_istft_library()
    buf = ctypes.create_string_buffer(256)
    assert lib.tfft_istft_describe(length, hop, pad, rows, flags, buf, len(buf)) == ERR_ARG
    assert needle in lib.tfft_istft_last_error().decode()
    h = ctypes.c_void_p()
    o = _opts(flags=flags)
    assert lib.tfft_istft_plan_create(rows, length, hop, pad, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG    # before any device call
    assert needle in lib.tfft_istft_last_error().decode() and not h.value


@pytest.mark.parametrize("length,hop,pad,needle", [(0, 8, 0, "length"), (12, 8, 2048, "length"), (8192, 12, 0, "hop"), (8192, 8, 4096, "pad"),
                                                   (8, 8, 0, "length + 2 * pad"), ((1 << 26) + 8, 8, 0, "2^26")])
def test_geometry_refuses_what_create_refuses(length, hop, pad, needle):
    lib = istft.load_istft_library()
    frames = ctypes.c_uint64(77)
    assert lib.tfft_istft_geometry(length, hop, pad, ctypes.byref(frames)) == ERR_ARG and frames.value == 77
    assert needle in lib.tfft_istft_last_error().decode()
    with pytest.raises(tf.TfftError):
        tf.istft_geometry(length, hop, pad)


@pytest.mark.parametrize("rows,kw,needle", [
    (4, dict(out_sig_stride=8184), "out_sig_stride"), (4, dict(out_sig_stride=8196), "out_sig_stride"),
    (4, dict(in_frame_stride=2048), "in_frame_stride"), (4, dict(in_frame_stride=2060), "in_frame_stride"), (4, dict(in_frame_stride=8), "in_frame_stride"),
    # 32-bit item arithmetic carries the frame index; the byte extents must fit 64 bits
    (1 << 28, dict(in_frame_stride=1 << 40), "input extent"), (1 << 29, dict(out_sig_stride=1 << 40), "output extent"),
    (4, dict(struct_size=0), "struct_size"), (4, dict(struct_size=24), "struct_size"), (4, dict(struct_size=40), "struct_size"),
    (4, dict(reserved_=1), "reserved_"), (4, dict(launch_iters=65536), "launch_iters"),
    (4, dict(flags=2), "TFFT_ISTFT_RAW_SUM"), (4, dict(flags=1 << 30), "TFFT_ISTFT_RAW_SUM"),
])
def test_create_refuses_bad_options(rows, kw, needle):
    lib = istft.load_istft_library()
    h = ctypes.c_void_p()
    o = _opts(**kw)
    assert lib.tfft_istft_plan_create(rows, 8192, 1024, 0, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG
    assert needle in lib.tfft_istft_last_error().decode() and not h.value


def test_null_arguments_are_refused():
    lib = istft.load_istft_library()
    assert lib.tfft_istft_plan_create(1, 4096, 8, 0, 0, None, None) == ERR_ARG
    assert lib.tfft_istft_describe(4096, 8, 0, 1, 0, None, 0) == ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert lib.tfft_istft_describe(4096, 8, 0, 1, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_istft_exec(None, None, None, None, None) == ERR_ARG
    assert lib.tfft_istft_plan_set_window(None, None, None) == ERR_ARG
    assert lib.tfft_istft_plan_set_workspace(None, None, 0) == ERR_ARG
    assert lib.tfft_istft_plan_prepare(None) == ERR_ARG
    assert lib.tfft_istft_plan_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_istft_plan_num_launches(None) == 0 and lib.tfft_istft_plan_workspace_bytes(None) == 0
    lib.tfft_istft_plan_destroy(None)
    assert lib.tfft_istft_last_error().decode()


def test_no_gpu_means_errors_not_fallbacks():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(tf.TfftError):
        tf.TfftIstftPlan(2, 8192, 1024, 0)
    with pytest.raises(tf.TfftError):
        z = torch.zeros((2, 5, 2049), dtype=torch.float16)
        tf.istft(z, z, torch.zeros(4096, dtype=torch.float16), 1024, 8192)


def test_merge_gain_is_merge_times_4096_with_one_rounding():
    """where 4096 * merge stays a normal binary16 value the gain commutes with the rounding; near the subnormals it does not, which is
    why the factor sits in front of the rounding. Bin 0 and bin 2048 take A.re and B.re alone."""
    rng = np.random.default_rng(3)
    ar, ai, br, bi = (rng.uniform(-1, 1, (4, ir.BINS)).astype(np.float16) * np.float16(2.0 ** -8) for _ in range(4))
    zr, zi = ir.merge_gain(ar, ai, br, bi)
    import rfft_ref

    pr, pi = rfft_ref.merge(ar, ai, br, bi, ir.N)
    big = np.abs(pr.astype(np.float32)) >= 2.0 ** -14
    assert np.array_equal(zr[big], (pr.astype(np.float32) * 4096).astype(np.float16)[big]) and big.mean() > 0.9
    assert np.array_equal(zr[:, 0], (ar[:, 0].astype(np.float32) * 4096).astype(np.float16))
    assert np.array_equal(zi[:, 2048], (br[:, 2048].astype(np.float32) * 4096).astype(np.float16))
    assert np.array_equal(zr[:, 4095], (4096 * (ar[:, 1].astype(np.float32) + bi[:, 1].astype(np.float32))).astype(np.float16))
    tiny = np.float16(2.0 ** -20)                   # a subnormal difference survives the gain exactly
    z, _ = ir.merge_gain(np.full((1, ir.BINS), 3 * tiny, np.float16), np.zeros((1, ir.BINS), np.float16), np.zeros((1, ir.BINS), np.float16),
                         np.full((1, ir.BINS), tiny, np.float16))
    assert z[0, 5] == np.float16(4096 * 2.0 ** -19) and z[0, 4000] == np.float16(4096 * 2.0 ** -18)


@pytest.mark.parametrize("rows,length,hop", [(3, 8192, 1024), (2, 12288, 1024), (1, 8192, 2048)])
def test_ola_against_torch_istft(rows, length, hop):
    """istft_ref.ola on fp64 frames against torch.istft in float64 (Hann, center=True, length=L)"""
    import torch

    rng = np.random.default_rng([rows, length, hop])
    x = rng.uniform(-1, 1, (rows, length))
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(ir.N) / ir.N)
    spec = np.fft.rfft(st.windows(x, hop, 2048) * w[None, :], axis=-1).reshape(rows, -1, ir.BINS)
    got = ir.ola(np.fft.irfft(spec.reshape(-1, ir.BINS), n=ir.N, axis=-1), w, rows, length, hop, 2048)
    want = torch.istft(torch.from_numpy(spec.transpose(0, 2, 1).copy()), 4096, hop_length=hop, window=torch.from_numpy(w), center=True,
                       length=length).numpy()
    worst = np.abs(got - want).max()
    print(f"ola R={rows} L={length} hop={hop}: max |difference| to torch.istft = {worst:.2e}; to x = {np.abs(got - x).max():.2e}")
    assert got.dtype == np.float64 and worst <= 1e-12


def _round_trip(rows, length, hop, pad, window):
    x, w = st.case_data(rows, length, window=window)
    re, im = ir.spectra16(x, w, hop, pad)
    s = re.astype(np.float64) + 1j * im.astype(np.float64)
    v = (np.fft.irfft(s, n=ir.N, axis=-1) * ir.N).astype(np.float16)
    return x, w, v, ir.ola(v, w, rows, length, hop, pad)


@pytest.mark.parametrize("rows,length,hop,pad,iters,window", ir.CASES)
def test_numpy_round_trip_on_every_case(rows, length, hop, pad, iters, window):
    """x -> stft_ref.frames -> rfft / 4096 -> binary16 -> * 4096 -> irfft -> binary16 -> ola -> x: finite everywhere (a random window
    leaves single samples with den near 1e-8 in the self-paired cases, and the quotient still stays finite), +0 exactly where nothing
    covers a sample, and the figures the case table states."""
    x, w, v, y = _round_trip(rows, length, hop, pad, window)
    env = ir.envelope(w, length, hop, pad)
    assert y.dtype == np.float16 and y.shape == x.shape and np.isfinite(y).all()
    bare = env == 0
    assert (y.view(np.uint16)[:, bare] == 0).all()                         # +0, not -0
    want_bare = {(12288, 8192): 4096, (6152, 1024): 8}.get((length, hop), None)
    if want_bare is not None:
        assert bare.sum() == want_bare
    if window == "hann":
        # [0.5, 1] for the exact Hann window; the binary16 one is off by 2^-11 relative per value, its square by 2^-10
        assert bare.sum() == 0 and 0.5 * (1 - 2.0 ** -10) <= env.min() and env.max() <= 1.0 + 2.0 ** -10
    raw = ir.ola(v, w, rows, length, hop, pad, raw=True)
    assert np.isfinite(raw).all() and (raw.view(np.uint16)[:, bare] == 0).all()
    print(f"round trip R={rows} L={length} hop={hop} pad={pad} {window}: den in [{env[~bare].min():.2e}, {env.max():.2e}], {bare.sum()} uncovered, "
          f"max |y - x| = {np.abs(y.astype(np.float64) - x)[:, ~bare].max():.2e}")


@pytest.mark.parametrize("rows,length,hop,pad", [(3, 8192, 1024, 2048), (4, 12288, 1024, 2048)])
def test_round_trip_accuracy_on_the_accuracy_shapes(rows, length, hop, pad):
    """The shapes of the GPU accuracy test, Hann: every sample's envelope lies in [1.25, 1.5] and none is uncovered. With only the
    spectra and the frames rounded to binary16 the round trip stays inside what those roundings allow: each is 2^-11 relative per
    value (the products w x, the spectra: sqrt(2) for the half spectrum, tests/test_stft_host.py; the frames), carried through the
    overlap-add by at most sqrt(env_max / env_min) (Cauchy-Schwarz on e_y = sum w e_f / sum w^2 with sum_f |u_f|^2 <= env_max |x|^2),
    plus 2^-11 for the output. Measured: 1.1e-4."""
    x, w, v, y = _round_trip(rows, length, hop, pad, "hann")
    env = ir.envelope(w, length, hop, pad)
    assert 1.25 * (1 - 2.0 ** -10) <= env.min() and env.max() <= 1.5 * (1 + 2.0 ** -10)         # (the window is the binary16 Hann)
    bound = (2.0 ** -11 * (2 + np.sqrt(2))) * np.sqrt(env.max() / env.min()) + 2.0 ** -11
    worst = ir.rel_l2(y, x).max()
    print(f"round trip R={rows} L={length}: rel-L2 {worst:.2e} (bound {bound:.2e}), envelope in [{env.min():.4f}, {env.max():.4f}]")
    assert worst <= bound
