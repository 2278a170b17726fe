"""Short-frame ISTFT add-on (include/tfft_istftn.h, libtfft_istftn.so) on the host: the exported symbols, what it links, the four
kernels of its gfx950 code object and their resources (from the metadata notes alone), the geometry and the description, every
refusal that needs no device, per frame length, and the overlap-add of tests/istftn_ref.py against torch.istft in float64."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import istftn_ref as inr
import stftn_ref as sn
import tensor_fft_amd as tf
from tensor_fft_amd import istftn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_ARG = 5


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def test_header_library_and_binding_name_the_same_symbols():
    header = open(os.path.join(ROOT, "include", "tfft_istftn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                # declarations only: the comments name calls too
    declared = set(re.findall(r"\b(tfft_istftn_[a-z0-9_]+)\s*\(", code))
    assert declared == set(istftn.SYMBOLS) and len(declared) == 12, declared ^ set(istftn.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", istftn.istftn_lib_path()], capture_output=True, text=True, check=True).stdout
    text_syms = {line.split()[2] for line in nm.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    # -fvisibility=hidden: nothing but the entry points is exported as code
    assert text_syms == declared, text_syms ^ declared
    lib = istftn.load_istftn_library()
    for name in declared:
        assert hasattr(lib, name), name
    names = {"IstftNOpts", "TfftShortIstftPlan", "load_istftn_library", "short_istft", "istftn_cache_clear", "istftn_describe",
             "istftn_geometry", "istftn_lib_path"}
    assert set(tf.__all__) >= names and all(hasattr(tf, n) for n in names)
    assert tf.short_istft is istftn.short_istft and tf.TfftShortIstftPlan is istftn.TfftShortIstftPlan


def test_library_links_the_other_two_and_no_sibling():
    import __graft_entry__ as g

    dyn = subprocess.run(["readelf", "-d", istftn.istftn_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "libtfft_conv.so" in dyn and "libtfft.so" in dyn and "$ORIGIN" in dyn
    assert g.ADDONS == ("conv", "lconv", "gconv", "sconv", "bconv", "gsconv", "gbconv", "cconv", "gcconv", "stft", "istft", "stftn", "istftn")
    for other in g.ADDONS:
        if other not in ("conv", "istftn"):
            assert "libtfft_" + other + ".so" not in dyn, other
    # the build table: the library is checked and built with the others, and the example links it
    assert ("example_istftn", ("-ltfft_istftn", "-ltfft_stftn", "-ltfft_conv")) in g.EXAMPLES
    assert os.path.join(ROOT, "include", "tfft_istftn.h") in g._addon_sources("istftn")
    assert os.path.exists(os.path.join(ROOT, "examples", "example_istftn")) and g._example_current("example_istftn") and g._up_to_date()


def test_opts_struct_size_is_the_headers():
    """sizeof(tfft_istftn_opts) as the C compiler lays the header's struct out"""
    tmp = tempfile.mkdtemp(prefix="tfft_istftn_size_")
    try:
        src = os.path.join(tmp, "size.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include "tfft_istftn.h"\nint main(void) { tfft_istftn_opts o = TFFT_ISTFTN_OPTS_INIT; '
                    'printf("%u %u %d\\n", (unsigned)sizeof(o), o.struct_size, TFFT_ISTFTN_RAW_SUM); return 0; }\n')
        exe = os.path.join(tmp, "size")
        subprocess.check_call([shutil.which("cc") or "gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        out = subprocess.check_output([exe], text=True).split()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert [int(v) for v in out] == [32, 32, istftn.ISTFTN_RAW_SUM] and ctypes.sizeof(istftn.IstftNOpts) == 32
    for n, h in zip(inr.LENGTHS, (264, 520, 1032)):
        assert tf.rplan_spectrum_pitch(n) == istftn.istftn_pitch(n) == sn.pitch(n) == h and istftn.istftn_bins(n) == sn.bins(n) == n // 2 + 1
    assert istftn.ISTFTN_LENGTHS == inr.LENGTHS


def test_code_object_holds_the_four_kernels_and_their_resources():
    """From the metadata notes of the gfx950 code object: exactly the three instantiations of frames_kernel and the overlap-add and
    nothing else, each without scratch, without VGPR or SGPR spills and within 256 VGPRs."""
    import isa_lint

    tmp = tempfile.mkdtemp(prefix="tfft_istftn_isa_")
    try:
        local = os.path.join(tmp, "libtfft_istftn.so")
        shutil.copy(istftn.istftn_lib_path(), local)
        subprocess.check_call([os.path.join(isa_lint.LLVM_BIN, "llvm-objdump"), "--offloading", local], cwd=tmp,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f]
        assert len(co) == 1, co
        notes = subprocess.check_output([os.path.join(isa_lint.LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(tmp, co[0])], text=True)
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
    assert len(blocks) == 4 and set(seen) == {f"istft256r::frames_kernel<{r}>" for r in (2, 4, 8)} | {"olan::ola_kernel"}, list(seen)
    for name, (vgprs, scratch, spills, sgpr_spills) in seen.items():
        assert scratch == 0 and spills == 0 and sgpr_spills == 0 and vgprs <= 256, (name, vgprs, scratch, spills, sgpr_spills)


def _geometry_table(n):
    """(length, hop, pad) -> frames: every GPU case, and the ends of the range"""
    shapes = {c[1:4]: None for c in inr.cases(n) + inr.huge_hop_cases(n)}
    shapes.update({s[1:4]: None for s in inr.accuracy_shapes(n)})
    table = [(length, hop, pad, 1 + (length + 2 * pad - n) // hop) for length, hop, pad in shapes]
    return table + [(1 << 26, n // 4, 0, 1 + ((1 << 26) - n) // (n // 4)), (n, 1 << 40, 0, 1), (1 << 26, 8, n - 8, 1 + ((1 << 26) + 2 * (n - 8) - n) // 8)]


@pytest.mark.parametrize("n", inr.LENGTHS)
def test_geometry_and_describe(n):
    lib = istftn.load_istftn_library()
    for length, hop, pad, frames in _geometry_table(n):
        assert tf.istftn_geometry(n, length, hop, pad) == frames == inr.geometry(n, length, hop, pad) == tf.stftn_geometry(n, length, hop, pad)
        text = f"istft256r{n // 256}:{n} x {frames} + ola"
        assert tf.istftn_describe(n, length, hop, pad, 3) == text == tf.istftn_describe(n, length, hop, pad, 3, raw_sum=True)
        # the last frame ends inside the padded signal, and one more would not
        assert (frames - 1) * hop + n <= length + 2 * pad < frames * hop + n
        # the pointer of tfft_istftn_geometry may be NULL
        assert lib.tfft_istftn_geometry(n, length, hop, pad, None) == 0


@pytest.mark.parametrize("n", inr.LENGTHS)
def test_case_table_holds_the_frame_counts_it_states(n):
    per_wave = 16 // (n // 256)
    for (rows, length, hop, pad, iters, window), frames in zip(inr.cases(n), inr.FRAMES_PER_SIGNAL):
        f = inr.geometry(n, length, hop, pad)
        assert frames is None or f == frames, (length, hop, pad, f)
    totals = [c[0] * inr.geometry(n, *c[1:4]) for c in inr.cases(n)]
    assert totals[:9] == [1, 2, 9, 10, 32, 2, 2, 3, 164] and totals[9] == {512: 93, 1024: 45, 2048: 21}[n]
    # case 9: more groups than a launch of launch_iters = 3 has live waves on any chip, so waves loop; case 10: three groups per wave
    groups = -(-((164 + 1) // 2) // per_wave)
    for cus in (6, 64, 256, 304):
        assert max(sn.groups_per_wave(groups, cus, 3)) >= 2
        assert sn.groups_per_wave(-(-((totals[9] + 1) // 2) // per_wave), cus, 3) == [3, 3]
    # uncovered samples: n between the two frames of case 7, 8 behind the last frame of case 8, none under the Hann case
    for index, bare in ((6, n), (7, 8), (3, 0)):
        rows, length, hop, pad, _, window = inr.cases(n)[index]
        w = sn.case_data(n, rows, length, window=window)[1]
        assert (inr.envelope(w, n, length, hop, pad) == 0).sum() == bare
    for rows, length, hop, pad, _, _ in inr.huge_hop_cases(n):
        assert inr.geometry(n, length, hop, pad) == 1 and hop + length + pad >= 1 << 63


@pytest.mark.parametrize("n", inr.LENGTHS)
def test_one_frame_plans_take_any_hop(n):
    """hop is 64 bits wide and bounded only by its type where there is one frame per signal; the reference gives +0 behind the frame"""
    for rows, length, hop, pad, iters, window in inr.huge_hop_cases(n):
        assert tf.istftn_geometry(n, length, hop, pad) == 1
        assert tf.istftn_describe(n, length, hop, pad, rows) == f"istft256r{n // 256}:{n} x 1 + ola"
        w = sn.case_data(n, rows, length, window=window)[1]
        v = np.ones((rows, n), np.float16)
        y = inr.ola(v, w, n, rows, length, hop, pad)
        assert (y.view(np.uint16)[:, n - pad:] == 0).all() and (y[:, :n - pad] != 0).any()
        assert np.array_equal(y, inr.ola(v, w, n, rows, length, length + 2 * pad, pad))


def _opts(**kw):
    o = istftn.IstftNOpts(ctypes.sizeof(istftn.IstftNOpts), 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _refusals(n):
    return [
        (1, 0, 8, 0, 0, "length must be a multiple of 8"), (1, 4, 8, n // 2, 0, "length must be a multiple of 8"),
        (1, n + 4, 8, 0, 0, "length must be a multiple of 8"), (1, (1 << 26) + 8, 1024, 0, 0, "2^26"),
        (1, 2 * n, 0, 0, 0, "hop must be"), (1, 2 * n, 4, 0, 0, "hop must be"), (1, 2 * n, n + 4, 0, 0, "hop must be"),
        (1, 2 * n, 64, 4, 0, "pad must be"), (1, 2 * n, 64, n, 0, f"pad must be a multiple of 8 and below {n}"), (1, 2 * n, 64, 1 << 20, 0, "pad must be"),
        (1, n - 8, 8, 0, 0, f"length + 2 * pad must be at least {n}"), (1, 8, 8, n // 2 - 8, 0, "length + 2 * pad"),
        (0, 2 * n, 64, 0, 0, "rows"), (1 << 32, 2 * n, 64, 0, 0, "rows"),
        (1 << 20, 1 << 26, 8, 0, 0, "frame count"), ((1 << 32) - 1, n + 8, 8, 0, 0, "frame count"),
        (1, 2 * n, 64, 0, 2, "flag"), (1, 2 * n, 64, 0, 3, "flag"), (1, 2 * n, 64, 0, -1, "flag"),
    ]


@pytest.mark.parametrize("n", inr.LENGTHS)
def test_describe_and_create_refuse_with_a_message(n):
    lib = istftn.load_istftn_library()
    buf = ctypes.create_string_buffer(256)
    for rows, length, hop, pad, flags, needle in _refusals(n):
        assert lib.tfft_istftn_describe(n, length, hop, pad, rows, flags, buf, len(buf)) == ERR_ARG, (rows, length, hop, pad, flags)
        assert needle in lib.tfft_istftn_last_error().decode(), (needle, lib.tfft_istftn_last_error().decode())
        h = ctypes.c_void_p()
        o = _opts(flags=flags)
        assert lib.tfft_istftn_plan_create(n, rows, length, hop, pad, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG    # before any device call
        assert needle in lib.tfft_istftn_last_error().decode() and not h.value


@pytest.mark.parametrize("n,needle", [(4096, "tfft_istft_plan_create"), (0, "n must be 512, 1024 or 2048"), (256, "n must be 512, 1024 or 2048"),
                                      (768, "n must be 512, 1024 or 2048"), (8192, "n must be"), (1000, "n must be"), (2 ** 32 - 1, "n must be")])
def test_other_frame_lengths_are_refused(n, needle):
    lib = istftn.load_istftn_library()
    buf = ctypes.create_string_buffer(256)
    frames = ctypes.c_uint64(77)
    assert lib.tfft_istftn_geometry(n, 16384, 256, 0, ctypes.byref(frames)) == ERR_ARG and frames.value == 77
    assert needle in lib.tfft_istftn_last_error().decode()
    assert lib.tfft_istftn_describe(n, 16384, 256, 0, 1, 0, buf, len(buf)) == ERR_ARG and needle in lib.tfft_istftn_last_error().decode()
    h = ctypes.c_void_p()
    assert lib.tfft_istftn_plan_create(n, 1, 16384, 256, 0, 0, None, ctypes.byref(h)) == ERR_ARG and not h.value
    assert needle in lib.tfft_istftn_last_error().decode()
    with pytest.raises(tf.TfftError):
        tf.istftn_geometry(n, 16384, 256)
    with pytest.raises(tf.TfftError):
        tf.TfftShortIstftPlan(n, 1, 16384, 256)


@pytest.mark.parametrize("n", inr.LENGTHS)
def test_geometry_refuses_what_create_refuses(n):
    lib = istftn.load_istftn_library()
    for length, hop, pad, needle in [(0, 8, 0, "length"), (12, 8, n // 2, "length"), (2 * n, 12, 0, "hop"), (2 * n, 8, n, "pad"),
                                     (8, 8, 0, "length + 2 * pad"), ((1 << 26) + 8, 8, 0, "2^26")]:
        frames = ctypes.c_uint64(77)
        assert lib.tfft_istftn_geometry(n, length, hop, pad, ctypes.byref(frames)) == ERR_ARG and frames.value == 77
        assert needle in lib.tfft_istftn_last_error().decode()
        with pytest.raises(tf.TfftError):
            tf.istftn_geometry(n, length, hop, pad)


@pytest.mark.parametrize("n", inr.LENGTHS)
def test_create_refuses_bad_options(n):
    lib = istftn.load_istftn_library()
    b = sn.bins(n)
    for rows, kw, needle in [
        (4, dict(out_sig_stride=2 * n - 8), "out_sig_stride"), (4, dict(out_sig_stride=2 * n + 4), "out_sig_stride"),
        (4, dict(in_frame_stride=b - 1), f"in_frame_stride must be 0 or a multiple of 8 that is >= {b}"),
        (4, dict(in_frame_stride=b + 3), "in_frame_stride"), (4, dict(in_frame_stride=8), "in_frame_stride"),
        # 32-bit arithmetic carries the frame index; the byte extents must fit 64 bits
        (1 << 26, dict(in_frame_stride=1 << 40), "input extent"), (1 << 29, dict(out_sig_stride=1 << 40), "output extent"),
        (4, dict(struct_size=0), "struct_size"), (4, dict(struct_size=24), "struct_size"), (4, dict(struct_size=40), "struct_size"),
        (4, dict(reserved_=1), "reserved_"), (4, dict(launch_iters=65536), "launch_iters"),
        (4, dict(flags=2), "TFFT_ISTFTN_RAW_SUM"), (4, dict(flags=1 << 30), "TFFT_ISTFTN_RAW_SUM"),
    ]:
        h = ctypes.c_void_p()
        o = _opts(**kw)
        assert lib.tfft_istftn_plan_create(n, rows, 2 * n, n // 4, 0, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG, (rows, kw)
        assert needle in lib.tfft_istftn_last_error().decode() and not h.value, (needle, lib.tfft_istftn_last_error().decode())


def test_null_arguments_are_refused():
    lib = istftn.load_istftn_library()
    assert lib.tfft_istftn_plan_create(1024, 1, 1024, 8, 0, 0, None, None) == ERR_ARG
    assert lib.tfft_istftn_describe(1024, 1024, 8, 0, 1, 0, None, 0) == ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert lib.tfft_istftn_describe(1024, 1024, 8, 0, 1, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_istftn_exec(None, None, None, None, None) == ERR_ARG
    assert lib.tfft_istftn_plan_set_window(None, None, None) == ERR_ARG
    assert lib.tfft_istftn_plan_set_workspace(None, None, 0) == ERR_ARG
    assert lib.tfft_istftn_plan_prepare(None) == ERR_ARG
    assert lib.tfft_istftn_plan_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_istftn_plan_num_launches(None) == 0 and lib.tfft_istftn_plan_workspace_bytes(None) == 0
    lib.tfft_istftn_plan_destroy(None)
    assert lib.tfft_istftn_last_error().decode()


def test_no_gpu_means_errors_not_fallbacks():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(tf.TfftError):
        tf.TfftShortIstftPlan(1024, 2, 8192, 256, 0)
    z = torch.zeros((2, 29, 513), dtype=torch.float16)
    for call in (lambda: tf.short_istft(z, z, torch.zeros(1024, dtype=torch.float16), 256, 8192, 1024),
                 lambda: tf.istft(z, z, torch.zeros(1024, dtype=torch.float16), 256, 8192, n_fft=1024)):
        with pytest.raises(tf.TfftError):
            call()


def test_istft_refuses_other_frame_lengths():
    """istft(n_fft=768) is refused before anything is looked at, with the four lengths in the message; short_istft points to istft"""
    with pytest.raises(tf.TfftError) as e:
        tf.istft(None, None, None, 192, 8192, n_fft=768)
    assert "512, 1024, 2048 or 4096" in str(e.value)
    with pytest.raises(tf.TfftError) as e:
        tf.short_istft(None, None, None, 1024, 8192, 4096)
    assert "istft" in str(e.value)


@pytest.mark.parametrize("n", inr.LENGTHS)
def test_merge_gain_is_merge_times_n_with_one_rounding(n):
    """where n * merge stays a normal binary16 value the gain commutes with the rounding; near the subnormals it does not, which is
    why the factor sits in front of the rounding. Bin 0 and bin n / 2 take A.re and B.re alone."""
    import rfft_ref

    k = sn.bins(n)
    rng = np.random.default_rng([3, n])
    ar, ai, br, bi = (rng.uniform(-1, 1, (4, k)).astype(np.float16) * np.float16(2.0 ** -8) for _ in range(4))
    zr, zi = inr.merge_gain(ar, ai, br, bi, n)
    pr, pi = rfft_ref.merge(ar, ai, br, bi, n)
    big = np.abs(pr.astype(np.float32)) >= 2.0 ** -14
    assert zr.shape == zi.shape == (4, n) and zr.dtype == np.float16
    assert np.array_equal(zr[big], (pr.astype(np.float32) * n).astype(np.float16)[big]) and big.mean() > 0.9
    assert np.array_equal(zr[:, 0], (ar[:, 0].astype(np.float32) * n).astype(np.float16))
    assert np.array_equal(zi[:, n // 2], (br[:, n // 2].astype(np.float32) * n).astype(np.float16))
    assert np.array_equal(zr[:, n - 1], (n * (ar[:, 1].astype(np.float32) + bi[:, 1].astype(np.float32))).astype(np.float16))
    tiny = np.float16(2.0 ** -20)                   # a subnormal difference survives the gain exactly
    z, _ = inr.merge_gain(np.full((1, k), 3 * tiny, np.float16), np.zeros((1, k), np.float16), np.zeros((1, k), np.float16),
                          np.full((1, k), tiny, np.float16), n)
    assert z[0, 5] == np.float16(n * 2.0 ** -19) and z[0, n - 5] == np.float16(n * 2.0 ** -18)
    # merge_items: an odd total pairs its last frame with itself
    re, im = ar[:3], ai[:3]
    mr, mi = inr.merge_items(re, im, n)
    sr, si = inr.merge_gain(re[2:3], im[2:3], re[2:3], im[2:3], n)
    assert mr.shape == (2, n) and np.array_equal(mr[1:], sr) and np.array_equal(mi[1:], si)


@pytest.mark.parametrize("n", inr.LENGTHS)
def test_istft64_against_torch_istft(n):
    """istftn_ref.istft64 against torch.istft in float64 on the CPU, on shapes torch accepts: center=True with the Hann window, and
    center=False with a window drawn from uniform(0.25, 1) (no symmetry to hide a reversed frame, and an envelope torch does not
    refuse). Difference at most 1e-12 relative to the largest sample."""
    import torch

    k = sn.bins(n)
    for rows, length, hop, pad, window in [(3, 2 * n, n // 4, n // 2, "hann"), (2, 3 * n, n // 2, n // 2, "hann"), (1, 2 * n, n // 8, n // 2, "hann"),
                                           (3, n + 6 * (n // 4), n // 4, 0, "random"), (2, 3 * n, n // 2, 0, "random"), (1, n + 8 * 9, 8, 0, "random")]:
        rng = np.random.default_rng([n, rows, length, hop, pad])
        x = rng.uniform(-1, 1, (rows, length))
        w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n) if window == "hann" else rng.uniform(0.25, 1, n)
        frames = inr.geometry(n, length, hop, pad)
        spec = np.fft.rfft(sn.windows(n, x, hop, pad) * w[None, :], axis=-1) / n
        # istft64 takes what the plans take: rfft / n; torch takes rfft, bin-major
        got = inr.istft64(spec.real, spec.imag, w, rows, length, hop, pad)
        want = torch.istft(torch.from_numpy((spec * n).reshape(rows, frames, k).transpose(0, 2, 1).copy()), n, hop_length=hop,
                           window=torch.from_numpy(w), center=pad > 0, length=length).numpy()
        worst = np.abs(got - want).max() / np.abs(want).max()
        print(f"istft64 n={n} R={rows} L={length} hop={hop} pad={pad} {window}: max |difference| to torch.istft = {worst:.2e} of the largest "
              f"sample; to x = {np.abs(got - x).max():.2e}")
        assert got.dtype == np.float64 and got.shape == (rows, length) and worst <= 1e-12


@pytest.mark.parametrize("n", inr.LENGTHS)
def test_envelope_of_the_accuracy_shapes(n):
    """The shapes of the GPU accuracy test, binary16 Hann at hop n / 4 and pad n / 2: every sample's envelope lies in
    [1.25 (1 - 2^-10), 1.5 (1 + 2^-10)] and none is uncovered (the exact Hann window gives [1.25, 1.5]: 1.5 where four frames
    overlap, 1.25 at the trimmed ends)."""
    for rows, length, hop, pad in inr.accuracy_shapes(n):
        env = inr.envelope(sn.hann(n), n, length, hop, pad)
        print(f"envelope n={n} L={length}: [{env.min():.6f}, {env.max():.6f}]")
        assert 1.25 * (1 - 2.0 ** -10) <= env.min() and env.max() <= 1.5 * (1 + 2.0 ** -10)
