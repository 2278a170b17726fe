"""Gated gradient add-on (include/tfft_gbconv.h, libtfft_gbconv.so) on the host, as tests/test_bconv_host.py and
tests/test_gsconv_host.py check its two parents: the exported symbols, the nine kernels and the gfx950 ISA of its code object
(tools/isa_lint.py), the geometry with the partial sums P, the description, every refusal that needs no device, the numpy model of
the kernels' route (tests/gbconv_ref.py) against torch.autograd through an fp64 conv1d, the two wrong gate indexings, and the derived
tolerances of the GPU test's autograd comparison on the model alone."""
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
import gbconv_ref as gb
import gsconv_ref as gs
import sconv_ref as sr
import tensor_fft_amd as tf
from tensor_fft_amd import gbconv, gsconv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_ARG = 5
INSTANCES = [f"<{p}, {q}>" for p in ("true", "false") for q in ("true", "false")]
KERNELS = {f"gbconv4096::{k}{i}" for k in ("dgrad_kernel", "wgrad_kernel") for i in INSTANCES} | {"gbconv4096::wreduce_kernel"}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def test_header_library_and_binding_name_the_same_symbols():
    header = open(os.path.join(ROOT, "include", "tfft_gbconv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                # declarations only: the comments name calls too
    declared = set(re.findall(r"\b(tfft_gbconv_[a-z0-9_]+)\s*\(", code))
    assert declared == set(gbconv.SYMBOLS), declared ^ set(gbconv.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", gbconv.gbconv_lib_path()], capture_output=True, text=True, check=True).stdout
    text_syms = {line.split()[2] for line in nm.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    # -fvisibility=hidden: nothing but the entry points is exported as code
    assert text_syms == declared, text_syms ^ declared
    lib = gbconv.load_gbconv_library()
    for name in declared:
        assert hasattr(lib, name), name
    for name in ("TfftGatedLongConvGradPlan", "differentiable_gated_long_causal_conv", "gated_long_causal_conv_input_grad",
                 "gated_long_causal_conv_tap_grad", "gbconv_cache_clear", "gbconv_describe", "gbconv_geometry", "gbconv_lib_path",
                 "load_gbconv_library"):
        assert getattr(tf, name) is getattr(gbconv, name) and name in tf.__all__
    # the header's comment carries the sections of its siblings'
    for section in ("Shapes", "Method", "Summation order", "Data contract", "Aliasing", "Pairing", "Life cycle", "Range contract"):
        assert re.search(r"^ \* " + section + r"\b", header, flags=re.M), section


def test_library_links_the_two_below_and_none_of_the_other_five():
    dyn = subprocess.run(["readelf", "-d", gbconv.gbconv_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "libtfft_conv.so" in dyn and "libtfft.so" in dyn and "$ORIGIN" in dyn
    for other in ("libtfft_lconv.so", "libtfft_gconv.so", "libtfft_sconv.so", "libtfft_bconv.so", "libtfft_gsconv.so"):
        assert other not in dyn, other
    # tfft_gbconv_opts as the header lays it out: two uint32, six uint64 strides, launch_iters, partials and flags
    assert ctypes.sizeof(gbconv.GbconvOpts) == 72 and gbconv.GbconvOpts.dpre_seq_stride.offset == 48
    assert gbconv.GbconvOpts.partials.offset == 60 and gbconv.GbconvOpts.flags.offset == 64
    assert (gbconv.GBCONV_PRE_GATE, gbconv.GBCONV_POST_GATE) == (gsconv.GSCONV_PRE_GATE, gsconv.GSCONV_POST_GATE) == (1, 2)
    header = open(os.path.join(ROOT, "include", "tfft_gbconv.h")).read()
    assert re.search(r"TFFT_GBCONV_PRE_GATE = 1,", header) and re.search(r"TFFT_GBCONV_POST_GATE = 2\b", header)


@pytest.fixture(scope="module")
def report():
    import isa_lint

    rep = isa_lint.lint_text(isa_lint.disassemble(gbconv.gbconv_lib_path()))
    names = subprocess.run(["c++filt"], input="\n".join(rep), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n.strip().removeprefix("void ").split("(")[0]: rep[k] for n, k in zip(names, rep)}


def test_code_object_holds_exactly_the_nine_kernels(report):
    assert set(report) == KERNELS and len(report) == 9, sorted(report)
    for name in KERNELS - {"gbconv4096::wreduce_kernel"}:
        pre, post = name.endswith(("<true, true>", "<true, false>")), name.endswith(", true>")
        if "dgrad" in name:
            # two transforms of 16 stage-1 tiles and 16 stage-2/3 tiles, two MFMAs per complex product: bconv4096::dgrad_kernel's
            # count. Without a post gate the load is its LDS-DMA load; with one the window comes in through registers
            assert report[name]["mfma"] == 2 * (16 * 2 + 16 * 4) == 192, name
            assert report[name]["lds_dma"] == (0 if post else 16), name
        else:
            # three transforms, two windows: the x window by DMA without a pre gate, the g window by DMA without a post gate
            assert report[name]["mfma"] == 3 * (16 * 2 + 16 * 4) == 288, name
            assert report[name]["lds_dma"] == 16 * (not pre) + 16 * (not post), name
    assert report["gbconv4096::wreduce_kernel"]["mfma"] == 0 and report["gbconv4096::wreduce_kernel"]["lds_dma"] == 0


def test_no_packed_fp32_wait_states_and_dma_drain(report):
    for name, kernel in report.items():
        assert kernel["pk_f32"] == 0, name
        assert not kernel["findings"], (name, kernel["findings"])


def test_kernel_resources():
    """no scratch and no spills in any kernel, from the kernel metadata notes. The four dgrad_kernel instantiations and
    wreduce_kernel stay within the 256 registers of two waves per SIMD; the four wgrad_kernel instantiations run in workgroups of
    four waves, one per SIMD, as bconv4096::wgrad_kernel does: at most 256 architectural VGPRs of the 512 registers of a lane."""
    import isa_lint

    tmp = tempfile.mkdtemp(prefix="tfft_gbconv_isa_")
    try:
        local = os.path.join(tmp, "libtfft_gbconv.so")
        shutil.copy(gbconv.gbconv_lib_path(), local)
        subprocess.check_call([os.path.join(isa_lint.LLVM_BIN, "llvm-objdump"), "--offloading", local], cwd=tmp,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f][0]
        notes = subprocess.check_output([os.path.join(isa_lint.LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(tmp, co)], text=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    blocks = [b for b in notes.split("- .agpr_count") if "gbconv4096" in b]
    assert len(blocks) == 9
    for b in blocks:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        agprs = int(re.match(r":\s+(\d+)", b).group(1))
        total = int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1))                    # VGPRs and AGPRs of the unified file
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1))
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1))
        sgpr_spills = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", b).group(1))
        wg = int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", b).group(1))
        print(f"{name}: {total} registers ({total - agprs} VGPRs + {agprs} AGPRs), workgroup {wg}, scratch {scratch}, spills {spills} / {sgpr_spills}")
        assert scratch == 0 and spills == 0 and sgpr_spills == 0, (name, scratch, spills, sgpr_spills)
        if "wgrad_kernel" in name:
            assert wg == 256 and total - agprs <= 256 and total <= 512, (name, total, agprs, wg)
        else:
            assert agprs == 0 and total <= 256, (name, total, agprs)
            assert wg == (512 if "dgrad_kernel" in name else 256), (name, wg)       # no instantiation took the four-wave fallback


@pytest.mark.parametrize("length,taps", sr.INDEX_CASES)
def test_geometry_and_describe(length, taps):
    lib = gbconv.load_gbconv_library()
    halo, hop, segments = sr.geometry(length, taps)
    for rows, channels in ((3, 2), (1, 1), (5, 3), (64, 256), (2, 4096)):
        default = br.partials_of(rows, channels, length, taps)
        assert tf.gbconv_geometry(length, taps, rows, channels) == (halo, hop, segments, default) == tf.bconv_geometry(length, taps, rows, channels)
        for cap in (1, 2):
            assert tf.gbconv_geometry(length, taps, rows, channels, cap)[3] == br.partials_of(rows, channels, length, taps, cap)
        for pre, post, text in ((False, False, ""), (True, False, ":pre"), (False, True, ":post"), (True, True, ":pre+post")):
            assert tf.gbconv_describe(length, taps, rows, channels, pre_gate=pre, post_gate=post) == f"gbconv4096:4096{text} x {segments} | partials {default}"
        assert tf.gbconv_describe(length, taps, rows, channels, 2, pre_gate=True, post_gate=True) == f"gbconv4096:4096:pre+post x {segments} | partials {min(default, 2)}"
    assert tf.gbconv_geometry(length, taps)[:3] == tf.sconv_geometry(length, taps) == tf.gsconv_geometry(length, taps)
    # each pointer of tfft_gbconv_geometry may be NULL
    one = ctypes.c_uint64()
    assert lib.tfft_gbconv_geometry(length, taps, 3, 2, 0, None, None, ctypes.byref(one), None) == 0 and one.value == segments
    assert lib.tfft_gbconv_geometry(length, taps, 3, 2, 0, None, None, None, None) == 0


def _opts(**kw):
    o = gbconv.GbconvOpts(ctypes.sizeof(gbconv.GbconvOpts), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _gs_opts(flags):
    return gsconv.GsconvOpts(ctypes.sizeof(gsconv.GsconvOpts), 0, 0, 0, 0, 0, 0, flags)


@pytest.mark.parametrize("rows,channels,length,taps,flags,needle", [
    (1, 1, 0, 1, 0, "multiple of 8"), (1, 1, 4, 1, 3, "multiple of 8"), (1, 1, 4100, 1, 0, "multiple of 8"),
    (1, 1, 8, 0, 0, "taps must be at least 1"), (1, 1, 8, 2050, 3, "tfft_gconv_plan_create"), (1, 1, 16384, 1 << 20, 0, "tfft_gconv_plan_create"),
    (0, 1, 8, 1, 0, "rows"), (1 << 32, 1, 8, 1, 0, "rows"), (1, 0, 8, 1, 0, "channels"),
    (1 << 16, 1 << 16, 8, 1, 0, "rows * channels"), (1, 1, 8, 1, 4, "flag"), (1, 1, 8, 1, 8 | 3, "flag"), (1, 1, 8, 1, -1, "flag"),
    (1, 1, (1 << 26) + 8, 2, 0, "2^26"), (1 << 20, 1 << 10, 1 << 20, 2049, 0, "item count"),
])
def test_describe_and_create_refuse_with_the_messages_of_gsconv(rows, channels, length, taps, flags, needle):
    lib = gbconv.load_gbconv_library()
    buf = ctypes.create_string_buffer(256)
    assert lib.tfft_gbconv_describe(length, taps, rows, channels, 0, flags, buf, len(buf)) == ERR_ARG
    message = lib.tfft_gbconv_last_error().decode()
    assert needle in message
    h = ctypes.c_void_p()
    o = _opts(flags=flags)
    assert lib.tfft_gbconv_plan_create(rows, channels, length, taps, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG    # before any device call
    assert lib.tfft_gbconv_last_error().decode() == message and not h.value
    # the same refusal, word for word, as the forward plan's (its own names apart)
    g_lib = gsconv.load_gsconv_library()
    g_o = _gs_opts(flags)
    assert g_lib.tfft_gsconv_plan_create(rows, channels, length, taps, 0, ctypes.byref(g_o), ctypes.byref(h)) == ERR_ARG
    assert g_lib.tfft_gsconv_last_error().decode().replace("tfft_gsconv", "tfft_gbconv").replace("TFFT_GSCONV", "TFFT_GBCONV") == message
    if not flags & ~3:
        assert lib.tfft_gbconv_geometry(length, taps, rows, channels, 0, None, None, None, None) == ERR_ARG
        assert lib.tfft_gbconv_last_error().decode() == message


def test_geometry_leaves_its_outputs_alone_when_it_refuses():
    lib = gbconv.load_gbconv_library()
    halo = ctypes.c_uint64(77)
    assert lib.tfft_gbconv_geometry(12, 1, 1, 1, 0, ctypes.byref(halo), None, None, None) == ERR_ARG and halo.value == 77
    with pytest.raises(tf.TfftError):
        tf.gbconv_geometry(8, 2050)


@pytest.mark.parametrize("kw,needle", [
    (dict(x_seq_stride=8184), "x_seq_stride"), (dict(x_seq_stride=8196), "x_seq_stride"), (dict(pre_seq_stride=8), "pre_seq_stride"),
    (dict(pre_seq_stride=8193), "pre_seq_stride"), (dict(gy_seq_stride=8184), "gy_seq_stride"), (dict(gy_seq_stride=8201), "gy_seq_stride"),
    (dict(post_seq_stride=8), "post_seq_stride"), (dict(post_seq_stride=8196), "post_seq_stride"), (dict(dx_seq_stride=8184), "dx_seq_stride"),
    (dict(dx_seq_stride=8193), "dx_seq_stride"), (dict(dpre_seq_stride=8), "dpre_seq_stride"), (dict(dpre_seq_stride=8201), "dpre_seq_stride"),
    (dict(struct_size=0), "struct_size"), (dict(struct_size=48), "struct_size"), (dict(struct_size=64), "struct_size"),
    (dict(struct_size=80), "struct_size"), (dict(reserved_=1), "reserved_"), (dict(launch_iters=65536), "launch_iters"),
    (dict(flags=4), "TFFT_GBCONV_PRE_GATE and TFFT_GBCONV_POST_GATE only"), (dict(flags=1 << 30), "unknown flag bits"),
])
def test_create_refuses_bad_options(kw, needle):
    lib = gbconv.load_gbconv_library()
    h = ctypes.c_void_p()
    o = _opts(**kw)
    assert lib.tfft_gbconv_plan_create(4, 2, 8192, 64, 0, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG
    assert needle in lib.tfft_gbconv_last_error().decode() and not h.value


def test_null_arguments_are_refused():
    lib = gbconv.load_gbconv_library()
    assert lib.tfft_gbconv_plan_create(1, 1, 8, 1, 0, None, None) == ERR_ARG
    assert lib.tfft_gbconv_describe(8, 1, 1, 1, 0, 0, None, 0) == ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert lib.tfft_gbconv_describe(8, 1, 1, 1, 0, 3, small, len(small)) == ERR_ARG
    assert lib.tfft_gbconv_exec_input_grad(None, None, None, None, None, None, None, None) == ERR_ARG
    assert lib.tfft_gbconv_exec_tap_grad(None, None, None, None, None, None, None, None) == ERR_ARG
    assert lib.tfft_gbconv_plan_set_taps(None, None, None, None) == ERR_ARG
    assert lib.tfft_gbconv_plan_spectrum(None, None, None) == ERR_ARG
    assert lib.tfft_gbconv_plan_set_workspace(None, None, 0) == ERR_ARG
    assert lib.tfft_gbconv_plan_prepare(None) == ERR_ARG
    assert lib.tfft_gbconv_plan_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_gbconv_plan_num_launches(None) == 0 and lib.tfft_gbconv_plan_workspace_bytes(None) == 0
    lib.tfft_gbconv_plan_destroy(None)
    assert lib.tfft_gbconv_last_error().decode()


def test_no_gpu_means_errors_not_fallbacks():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(tf.TfftError):
        tf.TfftGatedLongConvGradPlan(4, 2, 16384, 2049, 0, pre_gate=True, post_gate=True)
    with pytest.raises(tf.TfftError):
        tf.TfftGatedLongConvGradPlan(1, 1, 8, 1, 0)
    x, h = torch.zeros((2, 2, 4096), dtype=torch.float16), torch.zeros((2, 7), dtype=torch.float16)
    with pytest.raises(tf.TfftError):
        tf.gated_long_causal_conv_input_grad(x, h, x=x, pre=x, post=x)
    with pytest.raises(tf.TfftError):
        tf.gated_long_causal_conv_tap_grad(x, x, 7, pre=x, post=x)
    with pytest.raises(tf.TfftError):
        tf.differentiable_gated_long_causal_conv(x.requires_grad_(), h, pre=x.detach(), post=x.detach())


def test_cases_are_the_issue_s():
    assert gb.DX_CASE_MODES is gs.CASE_MODES and gb.TAP_KINDS == ("delay", "noise")
    assert [c[:5] for c in gb.DH_CASE_MODES[:len(br.DH_CASES)]] == br.DH_CASES and all(c[5] == "pre+post" for c in gb.DH_CASE_MODES[:len(br.DH_CASES)])
    assert gb.SINGLE_GATE_CASES == [(8, 1, 1, 1, 0), (2056, 1, 2, 2, 0), (2048, 2049, 3, 3, 0), (4104, 7, 3, 3, 0)]
    assert [gb.items_per_channel(c) for c in gb.SINGLE_GATE_CASES] == [1, 1, 2, 4] == sorted(gb.items_per_channel(c) for c in br.DH_CASES)[:4]
    assert len(gb.DH_CASE_MODES) == len(br.DH_CASES) + 8
    assert gb.AUTOGRAD_CASES == [(4104, 7, 3, 3), (2048, 2049, 3, 3)] and gb.AUTOGRAD_MODE == "pre+post+skip"


def _rel(got, want):
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)


@pytest.mark.parametrize("mode", list(gb.GATE_MODES))
@pytest.mark.parametrize("length,taps", sr.INDEX_CASES)
def test_model_against_autograd_and_the_two_wrong_routes(length, taps, mode):
    """pure numpy fp64 by the kernels' route (gate -> windows -> circular correlation -> kept samples -> gate; for dh the forward
    windows with the halo of the gz window zeroed) against torch.autograd through an fp64 conv1d of the forward operator: all five
    gradients to 1e-12 relative; rows 3 (odd: a zero partner) x channels 2. Then the two wrong routes, a gate taken at the forward
    pass's window origin: each must differ wherever the halo is not zero."""
    rows, channels = 3, 2
    has_pre, has_post, has_skip = gb.GATE_MODES[mode]
    rng = np.random.default_rng([length, taps, 11])
    x, gy = rng.uniform(-1, 1, (rows, channels, length)), rng.uniform(-1, 1, (rows, channels, length))
    pre = rng.uniform(-1, 1, x.shape) if has_pre else None
    post = rng.uniform(-1, 1, x.shape) if has_post else None
    skip = rng.uniform(-0.5, 0.5, channels) if has_skip else None
    h = rng.standard_normal((channels, taps))
    h /= np.abs(h).sum(axis=1, keepdims=True)
    want = gb.autograd_reference(x, h, pre, post, skip, gy)
    dx, dpre = gb.model_input_grad(x, h, pre, post, skip, gy)
    dh, dskip = gb.model_tap_grad(x, pre, gy, post, taps)
    assert _rel(dx, want["dx"]) <= 1e-12 and _rel(dh, want["dh"]) <= 1e-12
    if has_pre:
        assert _rel(dpre, want["dpre"]) <= 1e-12
    else:
        assert dpre is None and "dpre" not in want
    if has_skip:
        assert _rel(dskip, want["dskip"]) <= 1e-12
    assert np.array_equal(dskip, dh[:, 0])
    if has_post:
        assert _rel(gb.model_dpost(x, h, pre, skip, gy), want["dpost"]) <= 1e-12
    halo = sr.geometry(length, taps)[0]
    if has_post and halo and length > halo:
        wrong, _ = gb.model_input_grad(x, h, pre, post, skip, gy, post_origin=-halo)
        assert np.abs(wrong - dx).max() > 1e-3
    if has_pre and halo and length > halo:
        wrong, wrong_pre = gb.model_input_grad(x, h, pre, post, skip, gy, pre_origin=halo)
        assert np.abs(wrong - dx).max() > 1e-3 and np.abs(wrong_pre - dpre).max() > 1e-3


@pytest.mark.parametrize("length,taps,rows,channels", gb.AUTOGRAD_CASES)
def test_model_with_rounded_products_stays_inside_the_derived_tolerances(length, taps, rows, channels):
    """the GPU test's autograd inputs; the model with gz, u and the output products in binary16 and fp64 everywhere else, against the
    fp64 autograd reference: inside the propagated-rounding terms ALONE (K = 0 for the middle), plus the gate's half ulp. The model's
    own fp64 transforms get the 1e-12 of the largest value that the test above holds them to (tap 2048 of L = 2048 is an empty sum)."""
    x, h, pre, post, skip, gy = gb.case_data(length, taps, rows, channels, "noise", 1, gb.AUTOGRAD_MODE)
    want = gb.autograd_reference(x, h, pre, post, skip, gy)
    dx, dpre = gb.model_input_grad(x, h, pre, post, skip, gy, rounded=True)
    peak = gb.du_peak(gb.gated(gy, post), h, skip)
    moved = gb.du_input_rounding(gy, h, post, skip)
    for got, gate, name in ((dx, pre, "dx"), (dpre, x, "dpre")):
        tol = gb.dx_tolerance(got, gate, 0.0, peak, rows, channels, length, taps, moved) + 1e-12 * np.abs(want[name]).max()
        ratio = np.abs(got - want[name]) / tol
        print(f"{name}: model / (input rounding + 1/2 ulp) = {ratio.max():.3f}")
        assert ratio.max() <= 1.0, name
        # ... and the whole tolerance of the GPU test is no tighter
        assert (gb.dx_tolerance(got, gate, gb.K_SCONV + 1.0, peak, rows, channels, length, taps, moved) >= tol - 1e-12 * np.abs(want[name]).max()).all()
    dh, _ = gb.model_tap_grad(x, pre, gy, post, taps, rounded=True)
    ratio = np.abs(dh - want["dh"]) / (gb.dh_input_rounding(x, pre, gy, post, taps) + 1e-12 * np.abs(want["dh"]).max())
    print(f"dh: model / input rounding = {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    assert np.abs(dh[:, 0] - want["dskip"]).max() <= gb.dh_input_rounding(x, pre, gy, post, taps)[:, 0].max()
    dpost = gb.model_dpost(x, h, pre, skip, gy, rounded=True).astype(np.float16)
    ratio = np.abs(dpost.astype(np.float64) - want["dpost"]) / gb.dpost_tolerance(dpost, x, h, pre, skip, gy)
    print(f"dpost: model / gsconv's tolerance = {ratio.max():.3f}")
    assert ratio.max() <= 1.0
