"""Short-frame STFT add-on (include/tfft_stftn.h, libtfft_stftn.so) on the host: the exported symbols, what it links, the three
kernels of its gfx950 code object and their resources (from the metadata notes alone), the geometry and the description, every
refusal that needs no device, the framing of tests/stftn_ref.py against torch.stft in float64, and what the binary16 rounding of
the products w * x costs."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import stftn_ref as sn
import tensor_fft_amd as tf
from tensor_fft_amd import stftn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_ARG = 5


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def test_header_library_and_binding_name_the_same_symbols():
    header = open(os.path.join(ROOT, "include", "tfft_stftn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                # declarations only: the comments name calls too
    declared = set(re.findall(r"\b(tfft_stftn_[a-z0-9_]+)\s*\(", code))
    assert declared == set(stftn.SYMBOLS), declared ^ set(stftn.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", stftn.stftn_lib_path()], capture_output=True, text=True, check=True).stdout
    text_syms = {line.split()[2] for line in nm.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    # -fvisibility=hidden: nothing but the entry points is exported as code
    assert text_syms == declared, text_syms ^ declared
    lib = stftn.load_stftn_library()
    for name in declared:
        assert hasattr(lib, name), name
    names = {"StftNOpts", "TfftShortStftPlan", "load_stftn_library", "short_stft", "stftn_cache_clear", "stftn_describe", "stftn_geometry",
             "stftn_lib_path"}
    assert set(tf.__all__) >= names and all(hasattr(tf, n) for n in names)
    assert tf.short_stft is stftn.short_stft and tf.TfftShortStftPlan is stftn.TfftShortStftPlan


def test_library_links_the_other_two_and_no_sibling():
    import __graft_entry__ as g

    dyn = subprocess.run(["readelf", "-d", stftn.stftn_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "libtfft_conv.so" in dyn and "libtfft.so" in dyn and "$ORIGIN" in dyn
    assert g.ADDONS == ("conv", "lconv", "gconv", "sconv", "bconv", "gsconv", "gbconv", "cconv", "gcconv", "stft", "istft", "stftn", "istftn")
    for other in g.ADDONS:
        if other not in ("conv", "stftn"):
            assert "libtfft_" + other + ".so" not in dyn, other
    assert ("example_stftn", ("-ltfft_stftn", "-ltfft_conv")) in g.EXAMPLES


def test_opts_struct_size_is_the_headers():
    """sizeof(tfft_stftn_opts) as the C compiler lays the header's struct out"""
    tmp = tempfile.mkdtemp(prefix="tfft_stftn_size_")
    try:
        src = os.path.join(tmp, "size.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include "tfft_stftn.h"\nint main(void) { tfft_stftn_opts o = TFFT_STFTN_OPTS_INIT; '
                    'printf("%u %u\\n", (unsigned)sizeof(o), o.struct_size); return 0; }\n')
        exe = os.path.join(tmp, "size")
        subprocess.check_call([shutil.which("cc") or "gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        out = subprocess.check_output([exe], text=True).split()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert [int(v) for v in out] == [32, 32] and ctypes.sizeof(stftn.StftNOpts) == 32
    for n, h in zip(sn.LENGTHS, (264, 520, 1032)):
        assert tf.rplan_spectrum_pitch(n) == stftn.stftn_pitch(n) == sn.pitch(n) == h and stftn.stftn_bins(n) == sn.bins(n) == n // 2 + 1
    assert stftn.STFTN_LENGTHS == sn.LENGTHS


def test_code_object_holds_the_three_kernels_and_their_resources():
    """From the metadata notes of the gfx950 code object: exactly the three instantiations of stft256r_kernel and nothing else, each
    without scratch, without VGPR or SGPR spills and within 256 VGPRs (the window's 4, 8 and 16 registers included)."""
    import isa_lint

    tmp = tempfile.mkdtemp(prefix="tfft_stftn_isa_")
    try:
        local = os.path.join(tmp, "libtfft_stftn.so")
        shutil.copy(stftn.stftn_lib_path(), local)
        subprocess.check_call([os.path.join(isa_lint.LLVM_BIN, "llvm-objdump"), "--offloading", local], cwd=tmp,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f][0]
        notes = subprocess.check_output([os.path.join(isa_lint.LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(tmp, co)], text=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    blocks = notes.split("- .agpr_count")[1:]
    seen = {}
    for block in blocks:
        mangled = re.search(r"\.name:\s+(\S+)", block).group(1)
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True, check=True).stdout.strip()
        name = name[5:] if name.startswith("void ") else name
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1))
        sgprs = int(re.search(r"\.sgpr_count:\s+(\d+)", block).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        sgpr_spills = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1))
        print(f"{name.split('(')[0]}: {vgprs} VGPRs, {sgprs} SGPRs, scratch {scratch}, spills {spills} / {sgpr_spills}")
        seen[name.split("(")[0]] = (vgprs, scratch, spills, sgpr_spills)
    assert len(blocks) == 3 and set(seen) == {f"stft256r::stft256r_kernel<{r}>" for r in (2, 4, 8)}, list(seen)
    for name, (vgprs, scratch, spills, sgpr_spills) in seen.items():
        assert scratch == 0 and spills == 0 and sgpr_spills == 0 and vgprs <= 256, (name, vgprs, scratch, spills, sgpr_spills)


@pytest.mark.parametrize("n", sn.LENGTHS)
def test_geometry_and_describe(n):
    lib = stftn.load_stftn_library()
    for length, hop, pad, frames in sn.geometry_table(n):
        assert tf.stftn_geometry(n, length, hop, pad) == frames == sn.geometry(n, length, hop, pad), (length, hop, pad)
        assert tf.stftn_describe(n, length, hop, pad, 3) == f"stft256r{n // 256}:{n} x {frames}"
        # the last frame ends inside the padded signal, and one more would not
        assert (frames - 1) * hop + n <= length + 2 * pad < frames * hop + n
        # the pointer of tfft_stftn_geometry may be NULL
        assert lib.tfft_stftn_geometry(n, length, hop, pad, None) == 0


@pytest.mark.parametrize("n", sn.LENGTHS)
def test_geometry_table_holds_what_the_gpu_cases_need(n):
    table = {g[:3]: g[3] for g in sn.geometry_table(n)}
    want = [1, 2, 3, 5, 2, 4, 2, (sn.LOOP_GROUPS * sn.per_group(n) - 3) // 3]
    for (rows, length, hop, pad, _), frames in zip(sn.cases(n), want):
        assert table[(length, hop, pad)] == frames
        assert sn.windows(n, np.zeros((rows, length), np.float16), hop, pad).shape == (rows * frames, n)
    for rows, length, hop, pad in sn.accuracy_shapes(n):
        assert (length, hop, pad) in table and (length - n) % hop == 0 and pad == 0            # every frame is full
    assert [rows * table[(length, hop, pad)] for rows, length, hop, pad in sn.accuracy_shapes(n)] == [9, 32]
    # the looping case: 93, 45, 21 frames in six groups, three per live wave, on any chip of six compute units or more
    rows, length, hop, pad, iters = sn.cases(n)[7]
    total = rows * table[(length, hop, pad)]
    assert total == {512: 93, 1024: 45, 2048: 21}[n] and iters == 3
    groups = -(-((total + 1) // 2) // (sn.per_group(n) // 2))
    for cus in (6, 64, 256, 304):
        assert sn.groups_per_wave(groups, cus, iters) == [3, 3]


def _opts(**kw):
    o = stftn.StftNOpts(ctypes.sizeof(stftn.StftNOpts), 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _refusals(n):
    return [
        (1, 0, 8, 0, 0, "length must be a multiple of 8"), (1, 4, 8, n // 2, 0, "length must be a multiple of 8"),
        (1, n + 4, 8, 0, 0, "length must be a multiple of 8"), (1, (1 << 26) + 8, 1024, 0, 0, "2^26"),
        (1, 2 * n, 0, 0, 0, "hop must be"), (1, 2 * n, 4, 0, 0, "hop must be"), (1, 2 * n, n + 4, 0, 0, "hop must be"),
        (1, 2 * n, 64, 4, 0, "pad must be"), (1, 2 * n, 64, n, 0, f"below {n}"), (1, 2 * n, 64, 1 << 20, 0, "pad must be"),
        (1, n - 8, 8, 0, 0, f"length + 2 * pad must be at least {n}"), (1, 8, 8, n // 2 - 8, 0, "length + 2 * pad"),
        (0, 2 * n, 64, 0, 0, "rows"), (1 << 32, 2 * n, 64, 0, 0, "rows"),
        (1 << 20, 1 << 26, 8, 0, 0, "frame count"), ((1 << 32) - 1, n + 8, 8, 0, 0, "frame count"),
        (1, 2 * n, 64, 0, 1, "flag"), (1, 2 * n, 64, 0, -1, "flag"),
    ]


@pytest.mark.parametrize("n", sn.LENGTHS)
def test_describe_and_create_refuse_with_a_message(n):
    lib = stftn.load_stftn_library()
    buf = ctypes.create_string_buffer(256)
    for rows, length, hop, pad, flags, needle in _refusals(n):
        assert lib.tfft_stftn_describe(n, length, hop, pad, rows, flags, buf, len(buf)) == ERR_ARG, (rows, length, hop, pad, flags)
        assert needle in lib.tfft_stftn_last_error().decode(), (needle, lib.tfft_stftn_last_error().decode())
        h = ctypes.c_void_p()
        o = _opts(flags=flags)
        assert lib.tfft_stftn_plan_create(n, rows, length, hop, pad, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG    # before any device call
        assert needle in lib.tfft_stftn_last_error().decode() and not h.value


@pytest.mark.parametrize("n,needle", [(4096, "tfft_stft_plan_create"), (0, "n must be 512, 1024 or 2048"), (256, "n must be"), (768, "n must be"),
                                      (8192, "n must be"), (1000, "n must be"), (2 ** 32 - 1, "n must be")])
def test_other_frame_lengths_are_refused(n, needle):
    lib = stftn.load_stftn_library()
    buf = ctypes.create_string_buffer(256)
    frames = ctypes.c_uint64(77)
    assert lib.tfft_stftn_geometry(n, 16384, 256, 0, ctypes.byref(frames)) == ERR_ARG and frames.value == 77
    assert needle in lib.tfft_stftn_last_error().decode()
    assert lib.tfft_stftn_describe(n, 16384, 256, 0, 1, 0, buf, len(buf)) == ERR_ARG and needle in lib.tfft_stftn_last_error().decode()
    h = ctypes.c_void_p()
    assert lib.tfft_stftn_plan_create(n, 1, 16384, 256, 0, 0, None, ctypes.byref(h)) == ERR_ARG and not h.value
    assert needle in lib.tfft_stftn_last_error().decode()
    with pytest.raises(tf.TfftError):
        tf.stftn_geometry(n, 16384, 256)
    with pytest.raises(tf.TfftError):
        tf.TfftShortStftPlan(n, 1, 16384, 256)


@pytest.mark.parametrize("n", sn.LENGTHS)
def test_geometry_refuses_what_create_refuses(n):
    lib = stftn.load_stftn_library()
    for length, hop, pad, needle in [(0, 8, 0, "length"), (12, 8, n // 2, "length"), (2 * n, 12, 0, "hop"), (2 * n, 8, n, "pad"),
                                     (8, 8, 0, "length + 2 * pad"), ((1 << 26) + 8, 8, 0, "2^26")]:
        frames = ctypes.c_uint64(77)
        assert lib.tfft_stftn_geometry(n, length, hop, pad, ctypes.byref(frames)) == ERR_ARG and frames.value == 77
        assert needle in lib.tfft_stftn_last_error().decode()
        with pytest.raises(tf.TfftError):
            tf.stftn_geometry(n, length, hop, pad)


@pytest.mark.parametrize("n", sn.LENGTHS)
def test_create_refuses_bad_options(n):
    lib = stftn.load_stftn_library()
    b = sn.bins(n)
    for rows, kw, needle in [
        (4, dict(in_sig_stride=2 * n - 8), "in_sig_stride"), (4, dict(in_sig_stride=2 * n + 4), "in_sig_stride"),
        (4, dict(out_frame_stride=b - 1), f"out_frame_stride must be 0 or a multiple of 8 that is >= {b}"),
        (4, dict(out_frame_stride=b + 3), "out_frame_stride"), (4, dict(out_frame_stride=8), "out_frame_stride"),
        # 32-bit arithmetic carries the frame index; the byte extents must fit 64 bits
        (1 << 29, dict(in_sig_stride=1 << 40), "input extent"), (1 << 26, dict(out_frame_stride=1 << 40), "output extent"),
        (4, dict(struct_size=0), "struct_size"), (4, dict(struct_size=24), "struct_size"), (4, dict(struct_size=40), "struct_size"),
        (4, dict(reserved_=1), "reserved_"), (4, dict(launch_iters=65536), "launch_iters"),
        (4, dict(flags=1), "flags must be 0"), (4, dict(flags=1 << 30), "flags must be 0"),
    ]:
        h = ctypes.c_void_p()
        o = _opts(**kw)
        assert lib.tfft_stftn_plan_create(n, rows, 2 * n, n // 4, 0, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG, (rows, kw)
        assert needle in lib.tfft_stftn_last_error().decode() and not h.value, (needle, lib.tfft_stftn_last_error().decode())


def test_null_arguments_are_refused():
    lib = stftn.load_stftn_library()
    assert lib.tfft_stftn_plan_create(1024, 1, 1024, 8, 0, 0, None, None) == ERR_ARG
    assert lib.tfft_stftn_describe(1024, 1024, 8, 0, 1, 0, None, 0) == ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert lib.tfft_stftn_describe(1024, 1024, 8, 0, 1, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_stftn_exec(None, None, None, None, None) == ERR_ARG
    assert lib.tfft_stftn_plan_set_window(None, None, None) == ERR_ARG
    assert lib.tfft_stftn_plan_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_stftn_plan_num_launches(None) == 0
    lib.tfft_stftn_plan_destroy(None)
    assert lib.tfft_stftn_last_error().decode()


def test_no_gpu_means_errors_not_fallbacks():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(tf.TfftError):
        tf.TfftShortStftPlan(1024, 2, 8192, 256, 0)
    for call in (lambda: tf.short_stft(torch.zeros((2, 8192), dtype=torch.float16), torch.zeros(1024, dtype=torch.float16), 256, 1024),
                 lambda: tf.stft(torch.zeros((2, 8192), dtype=torch.float16), torch.zeros(512, dtype=torch.float16), 128, n_fft=512),
                 lambda: tf.stft(torch.zeros((2, 8192), dtype=torch.float16), torch.zeros(768, dtype=torch.float16), 128, n_fft=768)):
        with pytest.raises(tf.TfftError):
            call()


@pytest.mark.parametrize("n", sn.LENGTHS)
def test_framing_against_torch_stft(n):
    """stftn_ref.windows against torch.stft in float64 on the CPU: pad 0 is center=False, pad n / 2 is center=True with constant
    padding. A random window: a symmetric one hides a reversed frame."""
    import torch

    rows = 3
    for length, hop, pad in [(3 * n // 2, n // 4, 0), (n + 7 * (n // 4), n // 4, 0), (2 * n, n // 2, n // 2), (n, n // 8, n // 2), (3 * n, 2 * n, 0),
                             (n + 8, 8, 0)]:
        rng = np.random.default_rng([n, length, hop, pad])
        x = rng.uniform(-1, 1, (rows, length))
        w = rng.uniform(0, 1, n)
        got = np.fft.rfft(sn.windows(n, x, hop, pad) * w[None, :], axis=-1).reshape(rows, -1, sn.bins(n)) / n
        kw = dict(center=False) if pad == 0 else dict(center=True, pad_mode="constant")
        want = torch.stft(torch.from_numpy(x), n, hop_length=hop, window=torch.from_numpy(w), return_complex=True, **kw).numpy() / n
        assert want.shape == (rows, sn.bins(n), sn.geometry(n, length, hop, pad))           # bin-major; the plans are frame-major
        worst = np.abs(got - want.transpose(0, 2, 1)).max()
        print(f"framing n={n} L={length} hop={hop} pad={pad}: max |difference| = {worst:.2e}")
        assert worst <= 1e-12


@pytest.mark.parametrize("n", sn.LENGTHS)
def test_frames_round_each_product_once(n):
    """stftn_ref.frames is the binary16 product, correctly rounded, subnormals kept; zeros outside the signal"""
    x, w = sn.case_data(n, 2, 2 * n, window="random")
    x[0, :64] = np.float16(6e-5) * x[0, :64]                      # products in the subnormal range
    h = n // 2
    u = sn.frames(x, w, h, h)                                     # F = 5: frames 0 .. 4 of signal 0, 5 .. 9 of signal 1
    exact = sn.windows(n, x.astype(np.float64), h, h) * w.astype(np.float64)[None, :]
    assert np.array_equal(u.view(np.uint16), exact.astype(np.float16).view(np.uint16))      # fp64 -> fp16 of an exact product: one rounding
    assert (u[0, h:h + 64] != 0).any() and (np.abs(u[0, h:h + 64]) < 6.2e-5).all()
    assert not u[0, :h].any() and not u[4, h:].any() and u[4, :h].any()


def test_product_rounding_stays_inside_the_allowance():
    """What tests/test_gpu_stftn.py grants the comparison with fp64 of the UNROUNDED products on top of the transform's own bound:
    rounding the products to binary16 moves a frame's half spectrum by at most 2^-10 in rel-L2. Parseval, whatever the frame
    length: each normal product is off by at most 2^-11 relative, so the full spectrum moves by at most 2^-11 in rel-L2; a factor
    sqrt(2) covers the half spectrum, which counts its two edge bins once and every other bin of a conjugate pair once instead of
    twice."""
    worst = 0.0
    for n in sn.LENGTHS:
        for rows, length, hop, pad in sn.accuracy_shapes(n):
            x, w = sn.case_data(n, rows, length)
            rounded = np.fft.rfft(sn.frames(x, w, hop, pad).astype(np.float64), axis=-1)
            exact = np.fft.rfft(sn.windows(n, x.astype(np.float64), hop, pad) * w.astype(np.float64)[None, :], axis=-1)
            worst = max(worst, sn.rel_l2(rounded, exact).max())
    print(f"rounding of the products alone: rel-L2 {worst:.2e} of a frame's half spectrum")
    assert worst <= 2.0 ** -10
