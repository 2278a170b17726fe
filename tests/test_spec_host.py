"""Spectrogram add-on (include/tfft_spec.h, libtfft_spec.so) on the host: the exported symbols, what it links, the six kernels of its
gfx950 code object and their resources (from the metadata notes alone), every refusal that needs no device, the band helpers
against the restatement of tests/spec_ref.py, and what the restatement itself costs against fp64."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import spec_ref as sr
import stftn_ref as sn
import tensor_fft_amd as tf
from tensor_fft_amd import spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_ARG = 5


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def _err(lib):
    return lib.tfft_spec_last_error().decode()


def test_header_library_and_binding_name_the_same_symbols():
    header = open(os.path.join(ROOT, "include", "tfft_spec.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                # declarations only: the comments name calls too
    declared = set(re.findall(r"\b(tfft_spec_[a-z0-9_]+)\s*\(", code))
    assert declared == set(spec.SYMBOLS) and len(spec.SYMBOLS) == 10, declared ^ set(spec.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", spec.spec_lib_path()], capture_output=True, text=True, check=True).stdout
    text_syms = {line.split()[2] for line in nm.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    # -fvisibility=hidden: nothing but the entry points is exported as code
    assert text_syms == declared, text_syms ^ declared
    lib = spec.load_spec_library()
    for name in declared:
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name                          # every prototype is set, none left to ctypes' defaults
    assert lib.tfft_spec_last_error.restype is ctypes.c_char_p and lib.tfft_spec_plan_destroy.restype is None
    assert len(lib.tfft_spec_exec.argtypes) == 4 and len(lib.tfft_spec_plan_set_bands.argtypes) == 6
    names = {"Bands", "SpecOpts", "TfftSpectrogramPlan", "band_spectrogram", "bands_from_dense", "load_spec_library", "mel_bands",
             "power_spectrogram", "spec_cache_clear", "spec_describe", "spec_geometry", "spec_lib_path"}
    assert set(tf.__all__) >= names and all(hasattr(tf, n) for n in names)
    assert tf.power_spectrogram is spec.power_spectrogram and tf.TfftSpectrogramPlan is spec.TfftSpectrogramPlan


def test_library_links_the_other_two_and_no_sibling():
    import __graft_entry__ as g

    dyn = subprocess.run(["readelf", "-d", spec.spec_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "libtfft_conv.so" in dyn and "libtfft.so" in dyn and "$ORIGIN" in dyn
    assert g.ADDONS_SPECTRAL == ("spec",) and "spec" not in g.ADDONS
    for other in g.ADDONS:
        if other != "conv":
            assert "libtfft_" + other + ".so" not in dyn, other
    assert ("example_spec", ("-ltfft_spec", "-ltfft_conv")) in g.EXAMPLES
    # the spectral table is built, and watched, like the thirteen
    assert os.path.join(ROOT, "tensor-fft_amd", "spec", "spec256r.hpp") in g._addon_sources("spec")
    assert os.path.join(ROOT, "include", "tfft_spec.h") in g._addon_sources("spec")


def test_opts_struct_size_is_the_headers():
    """sizeof(tfft_spec_opts) and the defaults as the C compiler lays the header's struct out"""
    tmp = tempfile.mkdtemp(prefix="tfft_spec_size_")
    try:
        src = os.path.join(tmp, "size.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include <stddef.h>\n#include "tfft_spec.h"\nint main(void) { tfft_spec_opts o = TFFT_SPEC_OPTS_INIT; '
                    'printf("%u %u %u %u %u %g\\n", (unsigned)sizeof(o), o.struct_size, (unsigned)offsetof(tfft_spec_opts, bands), '
                    '(unsigned)offsetof(tfft_spec_opts, gain), o.bands, (double)o.gain); return 0; }\n')
        exe = os.path.join(tmp, "size")
        subprocess.check_call([shutil.which("cc") or "gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        out = subprocess.check_output([exe], text=True).split()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert [float(v) for v in out] == [40, 40, 32, 36, 0, 1.0] and ctypes.sizeof(spec.SpecOpts) == 40
    assert spec.SpecOpts.bands.offset == 32 and spec.SpecOpts.gain.offset == 36
    assert spec.SPEC_LENGTHS == sr.LENGTHS and spec.SPEC_MAX_BANDS == 1024


def test_code_object_holds_the_six_kernels_and_their_resources():
    """From the metadata notes of the gfx950 code object: exactly the six instantiations of spec_kernel and nothing else, each without
    scratch, without VGPR or SGPR spills, within 256 VGPRs and within the 160 KiB of LDS of a compute unit (the dynamic LDS a launch
    asks for is spec256r::spec_lds_bytes, held to 159 KiB at R = 8 by a static_assert; the notes hold the static part)."""
    import isa_lint

    tmp = tempfile.mkdtemp(prefix="tfft_spec_isa_")
    try:
        local = os.path.join(tmp, "libtfft_spec.so")
        shutil.copy(spec.spec_lib_path(), local)
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
        name = (name[5:] if name.startswith("void ") else name).split("(")[0]
        field = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))      # noqa: E731
        seen[name] = dict(vgprs=field("vgpr_count"), sgprs=field("sgpr_count"), scratch=field("private_segment_fixed_size"),
                          spills=field("vgpr_spill_count"), sgpr_spills=field("sgpr_spill_count"), lds=field("group_segment_fixed_size"))
        print(name, seen[name])
    assert len(blocks) == 6 and set(seen) == {f"spec256r::spec_kernel<{r}, {b}>" for r in (2, 4, 8) for b in ("false", "true")}, list(seen)
    for name, res in seen.items():
        assert res["scratch"] == 0 and res["spills"] == 0 and res["sgpr_spills"] == 0 and res["vgprs"] <= 256, (name, res)
        r = int(name.split("<")[1].split(",")[0])
        dynamic = 128 * 1024 + 2048 * r + 2048 * (r - 1) + (1024 if "true" in name else 0)
        assert res["lds"] + dynamic <= 160 * 1024, (name, res, dynamic)


@pytest.mark.parametrize("n", sr.LENGTHS)
def test_geometry_and_describe_are_stftns(n):
    lib = spec.load_spec_library()
    for length, hop, pad, frames in sn.geometry_table(n):
        assert tf.spec_geometry(n, length, hop, pad) == tf.stftn_geometry(n, length, hop, pad) == frames, (length, hop, pad)
        assert tf.spec_describe(n, length, hop, pad, 3) == f"spec256r{n // 256}:{n} x {frames}"
        assert lib.tfft_spec_geometry(n, length, hop, pad, None) == 0
    for rows, length, hop, pad, _ in sr.shapes(n):
        assert tf.spec_geometry(n, length, hop, pad) == sn.geometry(n, length, hop, pad)
    for length, hop, pad, needle in [(0, 8, 0, "length"), (12, 8, n // 2, "length"), (2 * n, 12, 0, "hop"), (2 * n, 8, n, "pad"),
                                     (8, 8, 0, "length + 2 * pad"), ((1 << 26) + 8, 8, 0, "2^26")]:
        frames = ctypes.c_uint64(77)
        assert lib.tfft_spec_geometry(n, length, hop, pad, ctypes.byref(frames)) == ERR_ARG and frames.value == 77
        assert needle in _err(lib)


def _opts(**kw):
    o = spec.SpecOpts(ctypes.sizeof(spec.SpecOpts), 0, 0, 0, 0, 0, 0, 1.0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("n", sr.LENGTHS)
def test_describe_and_create_refuse_a_shape_with_a_message(n):
    lib = spec.load_spec_library()
    buf = ctypes.create_string_buffer(256)
    for rows, length, hop, pad, flags, needle in [
        (1, 0, 8, 0, 0, "length must be a multiple of 8"), (1, n + 4, 8, 0, 0, "length must be a multiple of 8"),
        (1, (1 << 26) + 8, 1024, 0, 0, "2^26"), (1, 2 * n, 0, 0, 0, "hop must be"), (1, 2 * n, 4, 0, 0, "hop must be"),
        (1, 2 * n, 64, 4, 0, "pad must be"), (1, 2 * n, 64, n, 0, f"below {n}"),
        (1, n - 8, 8, 0, 0, f"length + 2 * pad must be at least {n}"),
        (0, 2 * n, 64, 0, 0, "rows"), (1 << 32, 2 * n, 64, 0, 0, "rows"), (1 << 20, 1 << 26, 8, 0, 0, "frame count"),
        (1, 2 * n, 64, 0, 1, "tfft_spec_opts.flags must be 0"), (1, 2 * n, 64, 0, -1, "flag"),
    ]:
        assert lib.tfft_spec_describe(n, length, hop, pad, rows, flags, buf, len(buf)) == ERR_ARG, (rows, length, hop, pad, flags)
        assert needle in _err(lib), (needle, _err(lib))
        h = ctypes.c_void_p()
        o = _opts(flags=flags)
        assert lib.tfft_spec_plan_create(n, rows, length, hop, pad, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG    # before any device call
        assert needle in _err(lib) and not h.value


@pytest.mark.parametrize("n,needles", [(4096, ("stop at 2048", "tfft_stft_plan_create")), (0, ("n must be 512, 1024 or 2048",)), (256, ("n must be",)),
                                       (768, ("n must be",)), (8192, ("n must be",)), (2 ** 32 - 1, ("n must be",))])
def test_other_frame_lengths_are_refused(n, needles):
    lib = spec.load_spec_library()
    buf = ctypes.create_string_buffer(256)
    frames = ctypes.c_uint64(77)
    h = ctypes.c_void_p()
    for rc in (lib.tfft_spec_geometry(n, 16384, 256, 0, ctypes.byref(frames)), lib.tfft_spec_describe(n, 16384, 256, 0, 1, 0, buf, len(buf)),
               lib.tfft_spec_plan_create(n, 1, 16384, 256, 0, 0, None, ctypes.byref(h))):
        assert rc == ERR_ARG and all(needle in _err(lib) for needle in needles), _err(lib)
    assert frames.value == 77 and not h.value
    with pytest.raises(tf.TfftError):
        tf.spec_geometry(n, 16384, 256)
    with pytest.raises(tf.TfftError):
        tf.TfftSpectrogramPlan(n, 1, 16384, 256)


@pytest.mark.parametrize("n", sr.LENGTHS)
def test_create_refuses_bad_options(n):
    lib = spec.load_spec_library()
    b = sn.bins(n)
    for rows, kw, needle in [
        (4, dict(in_sig_stride=2 * n - 8), "in_sig_stride must be 0 or a multiple of 8 that is >= length"), (4, dict(in_sig_stride=2 * n + 4), "in_sig_stride"),
        # power mode: floats, a multiple of 4 (the 16-byte stores), at least n / 2 + 1
        (4, dict(out_frame_stride=b - 1), f"out_frame_stride must be 0 or a multiple of 4 that is >= {b}"),
        (4, dict(out_frame_stride=b + 1), f"out_frame_stride must be 0 or a multiple of 4 that is >= {b}"), (4, dict(out_frame_stride=8), "out_frame_stride"),
        # band mode: anything that holds the bands
        (4, dict(bands=80, out_frame_stride=79), "out_frame_stride must be 0 or >= 80"), (4, dict(bands=3, out_frame_stride=2), "out_frame_stride must be 0 or >= 3"),
        (1 << 29, dict(in_sig_stride=1 << 40), "input extent"), (1 << 26, dict(out_frame_stride=1 << 40), "output extent"),
        (1 << 26, dict(bands=5, out_frame_stride=(1 << 40) + 1), "must be below 2^61 floats"),
        (4, dict(struct_size=0), "struct_size"), (4, dict(struct_size=32), "struct_size"), (4, dict(struct_size=48), "struct_size"),
        (4, dict(reserved_=1), "reserved_"), (4, dict(launch_iters=65536), "launch_iters"),
        (4, dict(flags=1), "flags must be 0"), (4, dict(flags=1 << 30), "flags must be 0"),
        (4, dict(bands=1025), "bands must be 0 (power mode) or 1 .. 1024"), (4, dict(bands=2 ** 32 - 1), "bands must be"),
        (4, dict(gain=0.0), "gain must be finite and > 0"), (4, dict(gain=-1.0), "gain must be"), (4, dict(gain=float("inf")), "gain must be"),
        (4, dict(gain=float("nan")), "gain must be"),
    ]:
        h = ctypes.c_void_p()
        o = _opts(**kw)
        assert lib.tfft_spec_plan_create(n, rows, 2 * n, n // 4, 0, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG, (rows, kw)
        assert needle in _err(lib) and not h.value, (needle, _err(lib))


def test_null_arguments_are_refused():
    lib = spec.load_spec_library()
    assert lib.tfft_spec_plan_create(1024, 1, 1024, 8, 0, 0, None, None) == ERR_ARG
    assert lib.tfft_spec_describe(1024, 1024, 8, 0, 1, 0, None, 0) == ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert lib.tfft_spec_describe(1024, 1024, 8, 0, 1, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_spec_exec(None, None, None, None) == ERR_ARG and "null plan" in _err(lib)
    assert lib.tfft_spec_plan_set_window(None, None, None) == ERR_ARG
    assert lib.tfft_spec_plan_set_bands(None, 1, None, None, None, None) == ERR_ARG and "null plan" in _err(lib)
    assert lib.tfft_spec_plan_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_spec_plan_num_launches(None) == 0
    lib.tfft_spec_plan_destroy(None)


def test_no_gpu_means_errors_not_fallbacks():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(tf.TfftError):
        tf.TfftSpectrogramPlan(1024, 2, 8192, 256, 0)
    with pytest.raises(tf.TfftError):
        tf.TfftSpectrogramPlan(1024, 2, 8192, 256, 0, bands=80)
    x, w = torch.zeros((2, 8192), dtype=torch.float16), torch.zeros(1024, dtype=torch.float16)
    for call in (lambda: tf.power_spectrogram(x, w, 256, 1024), lambda: tf.band_spectrogram(x, w, 256, 1024, tf.mel_bands(1024, 16000, 80))):
        with pytest.raises(tf.TfftError):
            call()


# ---- the band helpers
def test_bands_container_and_dense_round_trip():
    rng = np.random.default_rng(3)
    for n in sr.LENGTHS:
        nbins = sn.bins(n)
        for name, bands in sr.band_sets(n).items():
            dense = sr.dense_of(bands, nbins)
            got = tf.bands_from_dense(dense)
            starts, counts, weights = sr.arrays_of(bands)
            # (a random weight is never zero at the ends of its band, so the spans come back as given)
            assert np.array_equal(got.starts, starts) and np.array_equal(got.counts, counts) and np.array_equal(got.weights, weights), (n, name)
            assert got.starts.dtype == got.counts.dtype == np.uint32 and got.weights.dtype == np.float32 and len(got) == len(bands)
            assert np.array_equal(got.dense(nbins), dense)
    # zeros inside a span are kept, zeros outside dropped; a gain scales the weights
    w = np.zeros((2, 257), np.float32)
    w[0, [5, 9]] = [1.0, 2.0]
    w[1, 256] = 3.0
    b = tf.bands_from_dense(w)
    assert b.starts.tolist() == [5, 256] and b.counts.tolist() == [5, 1] and b.weights.tolist() == [1, 0, 0, 0, 2, 3]
    assert tf.bands_from_dense(w, gain=0.5).weights.tolist() == [0.5, 0, 0, 0, 1, 1.5]
    w[1] = 0
    with pytest.raises(tf.TfftError) as e:
        tf.bands_from_dense(w)
    assert "row 1" in str(e.value)
    with pytest.raises(tf.TfftError):
        tf.Bands([0, 1], [2], rng.uniform(0, 1, 2))
    with pytest.raises(tf.TfftError):
        tf.Bands([0, 1], [2, 2], rng.uniform(0, 1, 3))


@pytest.mark.parametrize("n,rate,mels,scale,norm", sr.MEL_CASES)
def test_mel_bands_are_the_formulas_rounded_once(n, rate, mels, scale, norm):
    dense64 = sr.mel_dense(n, rate, mels, scale=scale, norm=norm)
    assert dense64.shape == (mels, sn.bins(n)) and (dense64 >= 0).all()
    assert (dense64.astype(np.float32) != 0).any(1).all(), "a band without a bin: choose another case"
    bands = tf.mel_bands(n, rate, mels, scale=scale, norm=norm)
    assert len(bands) == mels and (bands.counts >= 1).all()
    assert np.array_equal(bands.dense(sn.bins(n)), dense64.astype(np.float32))
    assert np.array_equal(tf.mel_filterbank(n, rate, mels, scale=scale, norm=norm), dense64)
    # triangles: every filter rises to one peak and falls; unnormalised neighbours add up to at most 1 in every bin
    peaks = dense64.argmax(1)
    assert (np.diff(peaks) >= 0).all()
    if norm is None:
        assert dense64.max() <= 1.0 and dense64.sum(0).max() <= 1.0 + 1e-12
    with pytest.raises(tf.TfftError):
        tf.mel_bands(n, rate, mels, scale="bark")
    with pytest.raises(tf.TfftError):
        tf.mel_bands(n, rate, mels, f_max=rate)
    with pytest.raises(tf.TfftError):
        tf.mel_bands(512, 16000, 400)                                 # triangles narrower than a bin


def test_mel_scales_at_their_published_points():
    assert abs(sr.hz_to_mel(1000.0, "htk") - 999.9855) < 1e-3                       # 2595 log10(1 + 1000 / 700)
    assert sr.hz_to_mel(1000.0, "slaney") == 15.0 and abs(sr.hz_to_mel(6400.0, "slaney") - 42.0) < 1e-12
    for scale in ("htk", "slaney"):
        f = np.array([0.0, 50.0, 999.0, 1000.0, 1001.0, 4000.0, 22050.0])
        assert np.allclose(sr.mel_to_hz(sr.hz_to_mel(f, scale), scale), f, rtol=1e-12, atol=1e-9)


# ---- the restatement against fp64
@pytest.mark.parametrize("n", sr.LENGTHS)
def test_restatement_stays_inside_the_bound_on_fp64_derived_spectra(n):
    """tests/spec_ref.power and band_energies on half spectra that ARE within K_RFFT of fp64 (fp64 rounded to binary16, far inside
    it): per frame sum |P - P64| <= POWER_BOUND * sum P64, and the bands within band_bound."""
    nbins = sn.bins(n)
    for idx in sr.ACCURACY_SHAPES:
        rows, length, hop, pad, _ = sr.shapes(n)[idx]
        x, w = sn.case_data(n, rows, length)
        z = np.fft.rfft(sn.frames(x, w, hop, pad).astype(np.float64), axis=-1) / n
        re, im = z.real.astype(np.float16), z.imag.astype(np.float16)
        assert sn.rel_l2(re.astype(np.float64) + 1j * im.astype(np.float64), z).max() <= sr.K_RFFT
        for gain in (1.0, float(n) ** 2):
            want = sr.p64(n, x, w, hop, pad, gain)
            got = sr.power(re, im, gain)
            ratio = (np.abs(got.astype(np.float64) - want).sum(-1) / want.sum(-1)).max()
            print(f"n={n} shape {idx} gain {gain:g}: worst frame sum|P - P64| / sum P64 = {ratio:.2e} (bound {sr.POWER_BOUND:.2e})")
            assert ratio <= sr.POWER_BOUND
            for name, bands in sr.band_sets(n).items():
                bound, e64 = sr.band_bound(want, bands, nbins)
                err = np.abs(sr.band_energies(got, bands).astype(np.float64) - e64).sum(-1)
                assert (err <= bound).all(), (n, idx, name, (err / bound).max())


def test_restatement_rounds_where_it_says():
    """one rounding for the sum, one for the gain, one per product and per addition of a band: against exact rational arithmetic"""
    from fractions import Fraction

    rng = np.random.default_rng(11)
    # magnitudes in [1 / 4, 1): the squares lie in [2^-4, 1) with 22 bits each, so a double holds their sum exactly
    re = (rng.choice([-1, 1], (1, 9)) * rng.uniform(0.25, 1, (1, 9))).astype(np.float16)
    im = (rng.choice([-1, 1], (1, 9)) * rng.uniform(0.25, 1, (1, 9))).astype(np.float16)
    gain = 3.0
    p = sr.power(re, im, gain)
    for k in range(9):
        s = Fraction(float(re[0, k])) ** 2 + Fraction(float(im[0, k])) ** 2
        assert Fraction(float(s)) == s
        assert p[0, k] == np.float32(np.float64(gain) * np.float64(np.float32(float(s))))     # float32 x float32 is exact in a double
    w = rng.uniform(0, 1, 4).astype(np.float32)
    got = sr.band_energies(p, [(2, w)])[0, 0]
    acc = np.float32(np.float64(w[0]) * np.float64(p[0, 2]))                          # a product of two float32 is exact in a double
    for i in range(1, 4):
        acc = np.float32(np.float64(acc) + np.float64(np.float32(np.float64(w[i]) * np.float64(p[0, 2 + i]))))
    assert got == acc
