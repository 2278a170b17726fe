"""Masked short-frame ISTFT add-on (include/tfft_mistftn.h, libtfft_mistftn.so) on the host: the exported symbols, what it links,
the options struct as the C compiler lays it out, the four kernels of its gfx950 code object and their resources (from the metadata
notes alone), every refusal that needs no device, and the restatement of tests/mistftn_ref.py against tests/istftn_ref.py, against
correctly rounded float64 sums and, for the adjoint, against the inner-product identity."""
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
import mistftn_ref as mr
import stftn_ref as sn
import tensor_fft_amd as tf
from tensor_fft_amd import mistftn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_ARG = 5


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def _err(lib):
    return lib.tfft_mistftn_last_error().decode()


def test_header_library_and_binding_name_the_same_symbols():
    header = open(os.path.join(ROOT, "include", "tfft_mistftn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                # declarations only: the comments name calls too
    declared = set(re.findall(r"\b(tfft_mistftn_[a-z0-9_]+)\s*\(", code))
    assert declared == set(mistftn.SYMBOLS) and len(mistftn.SYMBOLS) == 12, declared ^ set(mistftn.SYMBOLS)
    # call for call tfft_istftn.h
    assert {s.replace("tfft_mistftn_", "tfft_istftn_") for s in declared} == set(tf.istftn.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", mistftn.mistftn_lib_path()], capture_output=True, text=True, check=True).stdout
    text_syms = {line.split()[2] for line in nm.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    # -fvisibility=hidden: nothing but the entry points is exported as code
    assert text_syms == declared, text_syms ^ declared
    lib = mistftn.load_mistftn_library()
    for name in declared:
        assert getattr(lib, name).argtypes is not None, name          # every prototype is set, none left to ctypes' defaults
    assert lib.tfft_mistftn_last_error.restype is ctypes.c_char_p and lib.tfft_mistftn_plan_destroy.restype is None
    assert len(lib.tfft_mistftn_exec.argtypes) == 6 and lib.tfft_mistftn_plan_workspace_bytes.restype is ctypes.c_size_t
    names = {"MaskedIstftNOpts", "TfftMaskedIstftPlan", "load_mistftn_library", "mask_buffer", "masked_istft", "mistftn_cache_clear",
             "mistftn_describe", "mistftn_geometry", "mistftn_lib_path", "differentiable_short_stft", "differentiable_power_spectrogram"}
    assert set(tf.__all__) >= names and all(hasattr(tf, n) for n in names)
    assert tf.masked_istft is mistftn.masked_istft and tf.TfftMaskedIstftPlan is mistftn.TfftMaskedIstftPlan


def test_library_links_the_other_two_and_no_sibling():
    import __graft_entry__ as g

    dyn = subprocess.run(["readelf", "-d", mistftn.mistftn_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "libtfft_conv.so" in dyn and "libtfft.so" in dyn and "$ORIGIN" in dyn
    assert g.ADDONS_MASKED == ("mistftn",) and "mistftn" not in g.ADDONS + g.ADDONS_SPECTRAL
    for other in g.ADDONS + g.ADDONS_SPECTRAL:
        if other != "conv":
            assert "libtfft_" + other + ".so" not in dyn, other
    assert ("example_masked_istft", ("-ltfft_mistftn", "-ltfft_stftn", "-ltfft_conv")) in g.EXAMPLES
    # the masked table is built, and watched, like the others; the overlap-add is istftn's header, watched too
    sources = g._addon_sources("mistftn")
    assert os.path.join(ROOT, "tensor-fft_amd", "mistftn", "mistft256r.hpp") in sources
    assert os.path.join(ROOT, "include", "tfft_mistftn.h") in sources
    assert os.path.join(ROOT, "tensor-fft_amd", "istftn", "olan.hpp") in sources
    assert os.path.exists(os.path.join(ROOT, "examples", "example_masked_istft")) and g._example_current("example_masked_istft") and g._up_to_date()


def test_opts_struct_size_and_offsets_are_the_headers():
    """sizeof(tfft_mistftn_opts), its offsets and the flag values as the C compiler lays the header out"""
    tmp = tempfile.mkdtemp(prefix="tfft_mistftn_size_")
    fields = ("struct_size", "reserved_", "in_frame_stride", "out_sig_stride", "launch_iters", "flags", "mask_frame_stride")
    try:
        src = os.path.join(tmp, "size.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include <stddef.h>\n#include "tfft_mistftn.h"\nint main(void) { tfft_mistftn_opts o = TFFT_MISTFTN_OPTS_INIT; '
                    'printf("%u %u %d %d %llu", (unsigned)sizeof(o), o.struct_size, TFFT_MISTFTN_RAW_SUM, TFFT_MISTFTN_MASK_PER_BIN, '
                    '(unsigned long long)o.mask_frame_stride);\n'
                    + "".join(f'printf(" %u", (unsigned)offsetof(tfft_mistftn_opts, {name}));\n' for name in fields) + "return 0; }\n")
        exe = os.path.join(tmp, "size")
        subprocess.check_call([shutil.which("cc") or "gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        out = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert out[:5] == [40, 40, mistftn.MISTFTN_RAW_SUM, mistftn.MISTFTN_MASK_PER_BIN, 0] and ctypes.sizeof(mistftn.MaskedIstftNOpts) == 40
    assert out[5:] == [0, 4, 8, 16, 24, 28, 32] == [getattr(mistftn.MaskedIstftNOpts, name).offset for name in fields]
    # the fields of tfft_istftn_opts, in place, and one more
    assert [f[0] for f in mistftn.MaskedIstftNOpts._fields_][:6] == [f[0] for f in tf.IstftNOpts._fields_]
    assert mistftn.MISTFTN_LENGTHS == mr.LENGTHS == inr.LENGTHS


def test_code_object_holds_the_four_kernels_and_their_resources():
    """From the metadata notes of the gfx950 code object: exactly the three instantiations of mistft256r::frames_kernel and the
    overlap-add and nothing else, each without scratch, without VGPR or SGPR spills and within 256 VGPRs. Printed: the counts
    (frames_kernel<2>, <4>, <8>: 166, 162 and 182 VGPRs as built for DESIGN.md 3.22; istft256r's are 123 .. 167)."""
    import isa_lint

    tmp = tempfile.mkdtemp(prefix="tfft_mistftn_isa_")
    try:
        local = os.path.join(tmp, "libtfft_mistftn.so")
        shutil.copy(mistftn.mistftn_lib_path(), local)
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
        name = (name[5:] if name.startswith("void ") else name).split("(")[0]
        field = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))      # noqa: E731
        seen[name] = dict(vgprs=field("vgpr_count"), sgprs=field("sgpr_count"), scratch=field("private_segment_fixed_size"),
                          spills=field("vgpr_spill_count"), sgpr_spills=field("sgpr_spill_count"))
        print(name, seen[name])
    assert len(blocks) == 4 and set(seen) == {f"mistft256r::frames_kernel<{r}>" for r in (2, 4, 8)} | {"olan::ola_kernel"}, list(seen)
    for name, res in seen.items():
        assert res["scratch"] == 0 and res["spills"] == 0 and res["sgpr_spills"] == 0 and res["vgprs"] <= 256, (name, res)


@pytest.mark.parametrize("n", mr.LENGTHS)
def test_geometry_and_describe_are_istftns(n):
    lib = mistftn.load_mistftn_library()
    shapes = {c[1:4]: None for c in inr.cases(n) + inr.huge_hop_cases(n)}
    shapes.update({s[1:4]: None for s in inr.accuracy_shapes(n)})
    for length, hop, pad in list(shapes) + [(1 << 26, n // 4, 0), (n, 1 << 40, 0), (1 << 26, 8, n - 8)]:
        frames = inr.geometry(n, length, hop, pad)
        assert tf.mistftn_geometry(n, length, hop, pad) == frames == tf.istftn_geometry(n, length, hop, pad)
        text = f"mistft256r{n // 256}:{n} x {frames} + ola"
        assert tf.mistftn_describe(n, length, hop, pad, 3) == text == tf.mistftn_describe(n, length, hop, pad, 3, raw_sum=True, per_bin=True)
        assert text == "m" + tf.istftn_describe(n, length, hop, pad, 3)
        assert lib.tfft_mistftn_geometry(n, length, hop, pad, None) == 0


def _opts(**kw):
    o = mistftn.MaskedIstftNOpts(ctypes.sizeof(mistftn.MaskedIstftNOpts), 0, 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("n", mr.LENGTHS)
def test_describe_and_create_refuse_the_shapes_istftn_refuses(n):
    """the table of tests/test_istftn_host.py, message for message, but for the flag bits: 2 is TFFT_MISTFTN_MASK_PER_BIN here"""
    import test_istftn_host as th

    lib, ilib = mistftn.load_mistftn_library(), tf.load_istftn_library()
    buf = ctypes.create_string_buffer(256)
    table = [r for r in th._refusals(n) if r[4] not in (2, 3)] + [(1, 2 * n, 64, 0, 4, "TFFT_MISTFTN_MASK_PER_BIN"), (1, 2 * n, 64, 0, 8, "flag"),
                                                                   (1, 2 * n, 64, 0, 7, "unknown flag bits")]
    assert len(table) >= 18
    for rows, length, hop, pad, flags, needle in table:
        assert lib.tfft_mistftn_describe(n, length, hop, pad, rows, flags, buf, len(buf)) == ERR_ARG, (rows, length, hop, pad, flags)
        assert needle in _err(lib), (needle, _err(lib))
        if flags == 0:           # word for word
            assert ilib.tfft_istftn_describe(n, length, hop, pad, rows, flags, buf, len(buf)) == ERR_ARG
            assert ilib.tfft_istftn_last_error().decode() == _err(lib)
        h = ctypes.c_void_p()
        o = _opts(flags=flags)
        assert lib.tfft_mistftn_plan_create(n, rows, length, hop, pad, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG    # before any device call
        assert needle in _err(lib) and not h.value


@pytest.mark.parametrize("n,needles", [(4096, ("tfft_istft_plan_create", "n = 4096")), (0, ("n must be 512, 1024 or 2048",)), (256, ("n must be",)),
                                       (768, ("n must be",)), (8192, ("n must be",)), (2 ** 32 - 1, ("n must be",))])
def test_other_frame_lengths_are_refused(n, needles):
    lib = mistftn.load_mistftn_library()
    buf = ctypes.create_string_buffer(256)
    frames = ctypes.c_uint64(77)
    h = ctypes.c_void_p()
    for rc in (lib.tfft_mistftn_geometry(n, 16384, 256, 0, ctypes.byref(frames)), lib.tfft_mistftn_describe(n, 16384, 256, 0, 1, 0, buf, len(buf)),
               lib.tfft_mistftn_plan_create(n, 1, 16384, 256, 0, 0, None, ctypes.byref(h))):
        assert rc == ERR_ARG and all(needle in _err(lib) for needle in needles), _err(lib)
    assert frames.value == 77 and not h.value
    with pytest.raises(tf.TfftError):
        tf.mistftn_geometry(n, 16384, 256)
    with pytest.raises(tf.TfftError):
        tf.TfftMaskedIstftPlan(n, 1, 16384, 256)


@pytest.mark.parametrize("n", mr.LENGTHS)
def test_create_refuses_bad_options(n):
    lib = mistftn.load_mistftn_library()
    b = sn.bins(n)
    per_bin = mistftn.MISTFTN_MASK_PER_BIN
    for rows, kw, needle in [
        # the mask's stride: 0, or a multiple of 8 that holds bins 0 .. n / 2
        (4, dict(mask_frame_stride=b - 1), f"mask_frame_stride must be 0 or a multiple of 8 that is >= {b}"),
        (4, dict(mask_frame_stride=b), "mask_frame_stride must be 0 or a multiple of 8"), (4, dict(mask_frame_stride=8), "mask_frame_stride"),
        (4, dict(mask_frame_stride=sn.pitch(n) + 4), "mask_frame_stride"),
        (4, dict(flags=per_bin, mask_frame_stride=sn.pitch(n)), "mask_frame_stride must be 0 with TFFT_MISTFTN_MASK_PER_BIN"),
        (4, dict(flags=per_bin | 1, mask_frame_stride=8), "mask_frame_stride must be 0 with TFFT_MISTFTN_MASK_PER_BIN"),
        (1 << 26, dict(mask_frame_stride=1 << 40), "the mask extent"),
        # tfft_istftn_opts' own
        (4, dict(in_frame_stride=b - 1), f"in_frame_stride must be 0 or a multiple of 8 that is >= {b}"), (4, dict(in_frame_stride=b), "in_frame_stride"),
        (4, dict(out_sig_stride=2 * n - 8), "out_sig_stride must be 0 or a multiple of 8 that is >= length"), (4, dict(out_sig_stride=2 * n + 4), "out_sig_stride"),
        (1 << 26, dict(in_frame_stride=1 << 40), "input extent"), (1 << 29, dict(out_sig_stride=1 << 40), "output extent"),
        (4, dict(struct_size=0), "struct_size"), (4, dict(struct_size=32), "struct_size"), (4, dict(struct_size=48), "struct_size"),
        (4, dict(reserved_=1), "reserved_"), (4, dict(launch_iters=65536), "launch_iters"),
        (4, dict(flags=4), "flags must be 0 or a combination"), (4, dict(flags=1 << 30), "unknown flag bits"),
    ]:
        h = ctypes.c_void_p()
        o = _opts(**kw)
        assert lib.tfft_mistftn_plan_create(n, rows, 2 * n, n // 4, 0, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG, (rows, kw)
        assert needle in _err(lib) and not h.value, (needle, _err(lib))
    # a per-bin plan's mask has no extent to refuse: rows * frames does not enter
    with pytest.raises(tf.TfftError) as e:
        tf.TfftMaskedIstftPlan(n, 4, 2 * n, n // 4, per_bin=True, mask_frame_stride=sn.pitch(n))
    assert "TFFT_MISTFTN_MASK_PER_BIN" in str(e.value)


def test_null_arguments_are_refused():
    lib = mistftn.load_mistftn_library()
    assert lib.tfft_mistftn_plan_create(1024, 1, 1024, 8, 0, 0, None, None) == ERR_ARG and "null plan pointer" in _err(lib)
    assert lib.tfft_mistftn_describe(1024, 1024, 8, 0, 1, 0, None, 0) == ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert lib.tfft_mistftn_describe(1024, 1024, 8, 0, 1, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_mistftn_exec(None, None, None, None, None, None) == ERR_ARG and "null plan" in _err(lib)
    assert lib.tfft_mistftn_plan_set_window(None, None, None) == ERR_ARG
    assert lib.tfft_mistftn_plan_set_workspace(None, None, 0) == ERR_ARG and lib.tfft_mistftn_plan_prepare(None) == ERR_ARG
    assert lib.tfft_mistftn_plan_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_mistftn_plan_num_launches(None) == 0 and lib.tfft_mistftn_plan_workspace_bytes(None) == 0
    lib.tfft_mistftn_plan_destroy(None)


def test_no_gpu_means_errors_not_fallbacks():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(tf.TfftError):
        tf.TfftMaskedIstftPlan(1024, 2, 8192, 256, 0)
    re = torch.zeros((2, 29, 513), dtype=torch.float16)
    w = torch.zeros(1024, dtype=torch.float16)
    for call in (lambda: tf.masked_istft(re, re, re, w, 256, 8192, 1024), lambda: tf.masked_istft(re, re, re[0, 0], w, 256, 8192, 1024),
                 lambda: tf.differentiable_short_stft(torch.zeros((2, 8192), dtype=torch.float16), w, 256, 1024),
                 lambda: tf.differentiable_power_spectrogram(torch.zeros((2, 8192), dtype=torch.float16), w, 256, 1024)):
        with pytest.raises(tf.TfftError):
            call()
    for call in (lambda: tf.differentiable_short_stft(None, w, 256, 4096), lambda: tf.mask_buffer(1, 1, 4096, "cpu")):
        with pytest.raises(tf.TfftError):
            call()


# ---- the restatement itself
def _spectra(n, rows, length, hop, pad, window):
    x, w = sn.case_data(n, rows, length, window=window)
    return (x, w) + inr.spectra16(x, w, hop, pad)


@pytest.mark.parametrize("n", mr.LENGTHS)
def test_a_mask_of_ones_is_the_unmasked_merge_in_every_bit(n):
    for rows, length, hop, pad, _, window in inr.cases(n)[2:5]:          # 9, 10 and 32 frames: an odd total among them
        _, _, re, im = _spectra(n, rows, length, hop, pad, window)
        want = inr.merge_items(re, im, n)
        for ones in (np.ones(sn.bins(n), np.float16), np.ones(re.shape, np.float16)):
            got = mr.merge_items_masked(re, im, ones, n)
            assert np.array_equal(got[0].view(np.int16), want[0].view(np.int16)) and np.array_equal(got[1].view(np.int16), want[1].view(np.int16))
        # {0, +-1, +-2}: the unmasked merge of the premultiplied planes
        m = mr.sign_mask(re.shape, n)
        pre_re, pre_im = (m.astype(np.float32) * re).astype(np.float16), (m.astype(np.float32) * im).astype(np.float16)
        got, want = mr.merge_items_masked(re, im, m, n), inr.merge_items(pre_re, pre_im, n)
        assert np.isfinite(pre_re).all() and np.array_equal(got[0].view(np.int16), want[0].view(np.int16))
        assert np.array_equal(got[1].view(np.int16), want[1].view(np.int16))
        # per bin is per frame with the one mask repeated, and an odd total's last frame uses its own mask for both
        mb = mr.random_mask(sn.bins(n), n)
        a, b = mr.merge_items_masked(re, im, mb, n), mr.merge_items_masked(re, im, np.broadcast_to(mb, re.shape).copy(), n)
        assert np.array_equal(a[0].view(np.int16), b[0].view(np.int16)) and np.array_equal(a[1].view(np.int16), b[1].view(np.int16))


@pytest.mark.parametrize("n", mr.LENGTHS)
def test_float32_sums_are_the_correctly_rounded_sums(n):
    """Independence from contraction: a product of two binary16 values has at most 22 significant bits and is exact in float32 and in
    float64, so a float32 sum of two of them, formed as mul, mul, add or as mul, fma, is the exact sum rounded ONCE. Here: the float32
    sums of the restatement equal, in every bit, the exact sums rounded to float32. The exact sum is formed in float64, where it is
    exact whenever the exponents of the two products lie within 53 - 22 = 31 bits of each other; beyond that the smaller product is
    below a quarter of a float32 ulp of the larger and far from a tie, so the float64 sum rounds to float32 as the exact sum does.
    Planted subnormal masks and a signal of 2^-24 stretch the exponents."""
    rows, length, hop, pad, _, window = inr.cases(n)[2]
    _, _, re, im = _spectra(n, rows, length, hop, pad, window)
    re, im = re.copy(), im.copy()
    re[0, 7], im[1, 7], re[2, 11] = np.float16(2.0 ** -24), np.float16(-(2.0 ** -24)), np.float16(60000.0)
    m = mr.random_mask(re.shape, n + 1)
    a, b = mr.rfft_ref.pair_rows(re.shape[0])
    k = sn.bins(n)
    args = (m[a, :k], m[b, :k], re[a, :k], im[a, :k], re[b, :k], im[b, :k], n)
    z32, z64 = mr._sums(*args, np.float32), mr._sums(*args, np.float64)
    for got, exact in zip(z32, z64):
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), exact.astype(np.float32).view(np.int32))
    # the exactness claimed for float64, against rational arithmetic on a sample of ordinary bins (bins 5 .. 11 hold the planted values)
    from fractions import Fraction

    rng = np.random.default_rng(5)
    for t, kk in zip(rng.integers(0, a.size, 64), rng.integers(16, n // 2, 64)):
        f = lambda arr: Fraction(float(arr[t, kk]))                               # noqa: E731
        assert Fraction(float(z64[0][t, kk])) == f(args[0]) * f(args[2]) - f(args[1]) * f(args[5])
        assert Fraction(float(z64[1][t, kk])) == f(args[0]) * f(args[3]) + f(args[1]) * f(args[4])


@pytest.mark.parametrize("n", mr.LENGTHS)
def test_fp64_adjoint_satisfies_the_inner_product_identity(n):
    """<stft64(x), G> = <x, adjoint64(G)> to 1e-12 relative, over random x and G, pad 0 and centred, with and without trimmed frames"""
    rng = np.random.default_rng([23, n])
    for rows, length, hop, pad in [(3, 3 * n // 2, n // 4, 0), (2, 2 * n, n // 2, n // 2), (2, n, n // 8, n - 8), (1, 3 * n, 2 * n, 0)]:
        frames = inr.geometry(n, length, hop, pad)
        x = rng.uniform(-1, 1, (rows, length))
        w = rng.uniform(0, 1, n)
        g_re, g_im = rng.normal(size=(rows * frames, sn.bins(n))), rng.normal(size=(rows * frames, sn.bins(n)))
        lhs = mr.inner_spectra(mr.stft64(x, w, hop, pad), g_re, g_im)
        dx = mr.adjoint64(g_re, g_im, w, rows, length, hop, pad)
        rhs = float((x * dx).sum())
        scale = np.sqrt((x ** 2).sum() * (dx ** 2).sum())
        assert dx.shape == x.shape and abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs, scale)
        # the IM of bins 0 and n / 2 carries no gradient
        g2 = g_im.copy()
        g2[:, 0], g2[:, n // 2] = 7.0, -3.0
        assert np.array_equal(mr.adjoint64(g_re, g2, w, rows, length, hop, pad), dx)
