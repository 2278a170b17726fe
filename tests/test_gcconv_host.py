"""Gated carried convolution add-on (include/tfft_gcconv.h, libtfft_gcconv.so) on the host: the exported symbols, what the library
links, the option structs, the register budgets of its thirteen kernels (the code object's notes, tools/kernel_resources.py), what
build() compiles, the geometry and the descriptions, every refusal that needs no device with its message, and the identities that
tests/test_gpu_gcconv.py runs through the shipped gated plans, proved here in numpy: a carried window is a window of the shipped
plans on the concatenated sequences and gates, and the -0 trap of a negative gate padding."""
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
import gbconv_ref as gb
import gcconv_ref as gc
import gsconv_ref as gs
import sconv_ref as sr
import tensor_fft_amd as tf
from tensor_fft_amd import gcconv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ERR_ARG = 5
PRE, POST = gcconv.GCCONV_PRE_GATE, gcconv.GCCONV_POST_GATE


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


def test_header_library_and_binding_name_the_same_symbols():
    header = open(os.path.join(ROOT, "include", "tfft_gcconv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                # declarations only: the comments name calls too
    declared = set(re.findall(r"\b(tfft_gcconv_[a-z0-9_]+)\s*\(", code))
    assert declared == set(gcconv.SYMBOLS), declared ^ set(gcconv.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", gcconv.gcconv_lib_path()], capture_output=True, text=True, check=True).stdout
    text_syms = {line.split()[2] for line in nm.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    # -fvisibility=hidden: nothing but the entry points is exported as code
    assert text_syms == declared, text_syms ^ declared
    lib = gcconv.load_gcconv_library()
    for name in declared:
        assert hasattr(lib, name), name
    for name in ("TfftGatedChunkedConvPlan", "TfftGatedChunkedConvGradPlan", "gated_chunked_causal_conv", "gated_chunked_causal_conv_input_grad",
                 "gated_chunked_causal_conv_tap_grad", "differentiable_gated_chunked_causal_conv", "gcconv_cache_clear", "gcconv_describe",
                 "gcconv_geometry", "gcconv_lib_path", "load_gcconv_library"):
        assert getattr(tf, name) is getattr(gcconv, name) and name in tf.__all__
    # one next_history serves x and the pre gate alike
    assert gcconv.next_history is tf.next_history and not hasattr(tf, "next_pre_history")


def test_library_links_the_other_two_only():
    dyn = subprocess.run(["readelf", "-d", gcconv.gcconv_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "$ORIGIN" in dyn
    ours = set(re.findall(r"\[(libtfft[a-z_]*\.so)\]", dyn))
    assert ours == {"libtfft_conv.so", "libtfft.so"}, ours


def test_option_structs_match_the_header():
    """tfft_gsconv_opts (48 bytes) + three uint64; tfft_gbconv_opts (72 bytes, its int padded to 8) + six uint64. The compiler that
    builds the library lays the header out the same way."""
    o, g = gcconv.GcconvOpts, gcconv.GcconvGradOpts
    assert ctypes.sizeof(o) == 72 and [getattr(o, f).offset for f in ("launch_iters", "flags", "history", "hist_seq_stride", "pre_hist_seq_stride")] == [40, 44, 48, 56, 64]
    assert ctypes.sizeof(g) == 120 and (g.partials.offset, g.flags.offset) == (60, 64)
    assert [getattr(g, f).offset for f in ("history", "hist_seq_stride", "pre_hist_seq_stride", "future", "fut_seq_stride", "post_fut_seq_stride")] == [72, 80, 88, 96, 104, 112]
    # the fields in front of the contexts are tfft_gsconv_opts' and tfft_gbconv_opts', name by name
    assert [f for f, _ in o._fields_][:8] == [f for f, _ in tf.gsconv.GsconvOpts._fields_]
    assert [f for f, _ in g._fields_][:11] == [f for f, _ in tf.gbconv.GbconvOpts._fields_]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:
        tmp = tempfile.mkdtemp(prefix="tfft_gcconv_sizeof_")
        try:
            src = os.path.join(tmp, "s.c")
            with open(src, "w") as f:
                f.write('#include <stdio.h>\n#include "tfft_gcconv.h"\nint main(void) { printf("%zu %zu\\n", sizeof(tfft_gcconv_opts), '
                        'sizeof(tfft_gcconv_grad_opts)); return 0; }\n')
            subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", os.path.join(tmp, "s"), src])
            out = subprocess.check_output([os.path.join(tmp, "s")], text=True).split()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        assert [int(v) for v in out] == [ctypes.sizeof(o), ctypes.sizeof(g)]


def test_kernel_resources():
    """the code object's notes: thirteen kernels for gfx950, no scratch in any, fwd_kernel and dgrad_kernel within the 256 registers
    of two waves per SIMD and without AGPRs, wgrad_kernel within the unified file of its one-wave-per-SIMD shape"""
    import kernel_resources

    res = kernel_resources.resources(gcconv.gcconv_lib_path())
    names = subprocess.run(["c++filt"], input="\n".join(res), capture_output=True, text=True, check=True).stdout.split("\n")
    by = {re.sub(r"^void ", "", n.strip()).split("(")[0]: r for n, r in zip(names, res.values())}
    inst = [f"<{a}, {b}>" for a in ("false", "true") for b in ("false", "true")]
    want = {f"gcconv4096::{k}{i}" for k in ("fwd_kernel", "dgrad_kernel", "wgrad_kernel") for i in inst} | {"gcconv4096::wreduce_kernel"}
    assert set(by) == want, set(by) ^ want
    for name, r in sorted(by.items()):
        print(f"{name}: vgpr {r['vgpr']} agpr {r['agpr']} sgpr {r['sgpr']} scratch {r['scratch']}")
        assert r["scratch"] == 0, (name, r)
        if "wgrad_kernel" in name:
            assert r["vgpr"] - r["agpr"] <= 256 and r["vgpr"] <= 512, (name, r)
        else:
            assert r["agpr"] == 0 and r["vgpr"] <= 256, (name, r)


def test_build_compiles_the_library_and_the_example_for_gfx950(monkeypatch):
    """what build() runs when only this add-on and its example are missing, and that what it left behind is what it says"""
    import __graft_entry__ as g

    exe = os.path.join(ROOT, "examples", "example_gated_chunked_conv")
    assert os.path.exists(g.LIB_GCCONV) and os.path.exists(exe) and g._up_to_date()
    assert dict(g.EXAMPLES)["example_gated_chunked_conv"] == ("-ltfft_gcconv", "-ltfft_gsconv", "-ltfft_conv")
    sources = g._gcconv_sources()
    for f in ("tfft_gcconv.hip", "gcconv4096.hpp", "tfft_gcconv.h", "k4096.hpp", "libtfft_conv.so"):
        assert any(s.endswith(os.sep + f) for s in sources), f
    real_newer, calls = g._newer, []
    monkeypatch.setattr(g, "_newer", lambda target, deps: target not in (g.LIB_GCCONV, exe) and real_newer(target, deps))
    monkeypatch.setattr(g.subprocess, "check_call", lambda cmd, **kw: calls.append(cmd))
    assert not g._up_to_date()
    g._build_locked(False)
    assert len(calls) == 2, calls
    lib_cmd, ex_cmd = calls
    assert "--offload-arch=gfx950" in lib_cmd and "-fvisibility=hidden" in lib_cmd and "-fno-slp-vectorize" in lib_cmd and "-O3" in lib_cmd
    assert lib_cmd[lib_cmd.index("-o") + 1] == g.LIB_GCCONV and os.path.join(g.GCCONV_SRC, "tfft_gcconv.hip") in lib_cmd
    assert [a for a in lib_cmd if a.startswith("-ltfft")] == ["-ltfft_conv", "-ltfft"]
    # the flags of the ninth library, word for word
    monkeypatch.setattr(g, "_newer", lambda target, deps: target != g.LIB_CCONV and real_newer(target, deps))
    calls.clear()
    g._build_locked(False)
    swap = lambda a: a.replace("gcconv", "cconv")                                   # noqa: E731
    assert [swap(a) for a in lib_cmd] == calls[0]
    assert "--offload-arch=gfx950" in ex_cmd and ex_cmd[ex_cmd.index("-o") + 1] == exe and "-ltfft_gcconv" in ex_cmd
    monkeypatch.undo()
    dyn = subprocess.run(["readelf", "-d", exe], capture_output=True, text=True, check=True).stdout
    assert "libtfft_gcconv.so" in dyn and "libtfft_gsconv.so" in dyn
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split("\n")
    assert "examples/example_gated_chunked_conv" in ignored and "*.so" in ignored


GEOMETRY = [(c[0], c[1]) for c in gc.CASES] + [(4032, 2), (16384, 2049), (16384, 128), (1 << 26, 2049)]


@pytest.mark.parametrize("length,taps", GEOMETRY)
def test_geometry_and_describe(length, taps):
    lib = gcconv.load_gcconv_library()
    halo, hop, segments = sr.geometry(length, taps)
    out = [ctypes.c_uint64() for _ in range(4)]
    assert lib.tfft_gcconv_geometry(length, taps, *[ctypes.byref(o) for o in out]) == 0
    assert tuple(o.value for o in out) == (halo, hop, segments, gc.carry_min(taps))
    assert lib.tfft_gcconv_geometry(length, taps, None, None, None, None) == 0
    for rows, channels, cap in ((3, 2, 0), (1, 1, 0), (5, 3, 2), (64, 256, 0)):
        p = br.partials_of(rows, channels, length, taps, cap)
        assert tf.gcconv_geometry(length, taps, rows, channels, cap) == tf.cconv_geometry(length, taps, rows, channels, cap) == (halo, hop, segments, p, gc.carry_min(taps))
        for pre, post, text in ((False, False, ""), (True, False, ":pre"), (False, True, ":post"), (True, True, ":pre+post")):
            assert tf.gcconv_describe(length, taps, rows, channels, cap, pre, post) == (f"gcconv4096:4096{text} x {segments}",
                                                                                      f"gcconv4096:4096{text} x {segments} | partials {p}")
            # the shipped gated plans' descriptions but for the library's name
            assert tf.gcconv_describe(length, taps, rows, channels, cap, pre, post)[0].replace("gcconv", "gsconv") == tf.gsconv_describe(length, taps, rows, channels, pre, post)
    one = ctypes.c_uint64()
    assert lib.tfft_gcconv_grad_geometry(length, taps, 3, 2, 0, None, None, None, None, ctypes.byref(one)) == 0 and one.value == gc.carry_min(taps)


def test_cases_and_modes_cover_what_they_say():
    assert gc.CASES is cr.CASES and all(c[4] for c in gc.WITH_CONTEXT) and len(gc.WITH_CONTEXT) == len(cr.CASES) - 1
    assert [c[:2] for c in gc.SINGLE_GATE_CASES] == [(8, 9), (2048, 2049), (8064, 65)]
    modes = {}
    for c in gc.CASE_MODES:
        modes.setdefault(c[:6], set()).add(c[6])
    assert all(gc.EVERY_CASE_MODE in modes[tuple(c)] for c in gc.WITH_CONTEXT)
    assert all(modes[tuple(c)] == {gc.EVERY_CASE_MODE, "pre", "post"} for c in gc.SINGLE_GATE_CASES)
    d = gc.case_data(4104, 7, 3, 3, 8, "noise", 1, "pre")
    assert d["pre_hist"].shape == d["hist"].shape == (3, 3, 8) and d["post"] is None and d["post_fut"] is None and d["skip"] is None


def _opts(**kw):
    o = gcconv.GcconvOpts(ctypes.sizeof(gcconv.GcconvOpts))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _gopts(**kw):
    o = gcconv.GcconvGradOpts(ctypes.sizeof(gcconv.GcconvGradOpts))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _refused(rc, needle, handle=None):
    msg = gcconv.load_gcconv_library().tfft_gcconv_last_error().decode()
    assert rc == ERR_ARG and needle in msg and msg, (rc, needle, msg)
    assert handle is None or not handle.value


# everything tfft_gsconv_plan_create and tfft_gbconv_plan_create refuse (tests/test_gsconv_host.py), with their messages
@pytest.mark.parametrize("rows,channels,length,taps,flags,needle", [
    (1, 1, 0, 1, 0, "multiple of 8"), (1, 1, 4, 1, 0, "multiple of 8"), (1, 1, 4100, 1, 0, "multiple of 8"),
    (1, 1, 8, 0, 0, "taps must be at least 1"), (1, 1, 8, 2050, 0, "tfft_gconv_plan_create"), (1, 1, 16384, 1 << 20, 0, "tfft_gconv_plan_create"),
    (0, 1, 8, 1, 0, "rows"), (1 << 32, 1, 8, 1, 0, "rows"), (1, 0, 8, 1, 0, "channels"),
    (1 << 16, 1 << 16, 8, 1, 0, "rows * channels"), (1, 1, 8, 1, 4, "TFFT_GCCONV_PRE_GATE and TFFT_GCCONV_POST_GATE only"), (1, 1, 8, 1, -1, "unknown flag bits"),
    (1, 1, (1 << 26) + 8, 2, 0, "2^26"), (1 << 20, 1 << 10, 1 << 20, 2049, 0, "item count"),
])
def test_describe_and_create_refuse_with_a_message(rows, channels, length, taps, flags, needle):
    lib = gcconv.load_gcconv_library()
    buf = ctypes.create_string_buffer(256)
    _refused(lib.tfft_gcconv_describe(length, taps, rows, channels, flags, buf, len(buf)), needle)
    _refused(lib.tfft_gcconv_grad_describe(length, taps, rows, channels, 0, flags, buf, len(buf)), needle)
    h = ctypes.c_void_p()
    _refused(lib.tfft_gcconv_plan_create(rows, channels, length, taps, 0, ctypes.byref(_opts(flags=flags)), ctypes.byref(h)), needle, h)
    _refused(lib.tfft_gcconv_grad_create(rows, channels, length, taps, 0, ctypes.byref(_gopts(flags=flags)), ctypes.byref(h)), needle, h)
    # the shipped gated plans refuse the same shape (their messages name their own flags)
    assert tf.gsconv.load_gsconv_library().tfft_gsconv_describe(length, taps, rows, channels, flags, buf, len(buf)) == ERR_ARG


@pytest.mark.parametrize("length,taps,needle", [(0, 1, "multiple of 8"), (12, 1, "multiple of 8"), (8, 0, "taps"), (8, 2050, "tfft_gconv_plan_create"),
                                                ((1 << 26) + 8, 1, "2^26")])
def test_geometry_refuses_what_create_refuses(length, taps, needle):
    lib = gcconv.load_gcconv_library()
    halo = ctypes.c_uint64(77)
    _refused(lib.tfft_gcconv_geometry(length, taps, ctypes.byref(halo), None, None, None), needle)
    _refused(lib.tfft_gcconv_grad_geometry(length, taps, 1, 1, 0, ctypes.byref(halo), None, None, None, None), needle)
    assert halo.value == 77
    with pytest.raises(tf.TfftError):
        tf.gcconv_geometry(length, taps)


# (4, 2, 8192, 130): halo 192
@pytest.mark.parametrize("kw,needle", [
    (dict(in_seq_stride=8184), "in_seq_stride"), (dict(in_seq_stride=8196), "in_seq_stride"), (dict(out_seq_stride=8), "out_seq_stride"),
    (dict(pre_seq_stride=8184), "pre_seq_stride"), (dict(post_seq_stride=8196), "post_seq_stride"),
    (dict(struct_size=0), "struct_size"), (dict(struct_size=48), "struct_size"), (dict(struct_size=80), "struct_size"),
    (dict(reserved_=1), "reserved_"), (dict(launch_iters=65536), "launch_iters"), (dict(flags=8), "unknown flag bits"),
    (dict(history=4), "history must be a multiple of 8"), (dict(history=129), "history must be a multiple of 8"),
    (dict(history=200), "history must not exceed the halo"), (dict(history=1 << 40), "history must not exceed the halo"),
    (dict(history=136, hist_seq_stride=128), "hist_seq_stride"), (dict(history=136, hist_seq_stride=140), "hist_seq_stride"),
    (dict(history=136, pre_hist_seq_stride=128), "pre_hist_seq_stride"), (dict(flags=PRE, history=136, pre_hist_seq_stride=140), "pre_hist_seq_stride"),
    (dict(history=0, hist_seq_stride=4), "hist_seq_stride"),
])
def test_forward_create_refuses_bad_options(kw, needle):
    lib = gcconv.load_gcconv_library()
    h = ctypes.c_void_p()
    _refused(lib.tfft_gcconv_plan_create(4, 2, 8192, 130, 0, ctypes.byref(_opts(**kw)), ctypes.byref(h)), needle, h)


@pytest.mark.parametrize("kw,needle", [
    (dict(x_seq_stride=8184), "x_seq_stride"), (dict(pre_seq_stride=8196), "pre_seq_stride"), (dict(gy_seq_stride=8196), "gy_seq_stride"),
    (dict(post_seq_stride=8), "post_seq_stride"), (dict(dx_seq_stride=8), "dx_seq_stride"), (dict(dpre_seq_stride=12), "dpre_seq_stride"),
    (dict(struct_size=0), "struct_size"), (dict(struct_size=72), "struct_size"), (dict(struct_size=128), "struct_size"),
    (dict(reserved_=1), "reserved_"), (dict(launch_iters=65536), "launch_iters"), (dict(flags=1 << 30), "unknown flag bits"),
    (dict(history=4), "history must be a multiple of 8"), (dict(history=200), "history must not exceed the halo"),
    (dict(history=136, hist_seq_stride=128), "hist_seq_stride"), (dict(history=136, pre_hist_seq_stride=140), "pre_hist_seq_stride"),
    (dict(future=12), "future must be a multiple of 8"), (dict(future=256), "future must not exceed the halo"),
    (dict(future=136, fut_seq_stride=128), "fut_seq_stride"), (dict(future=192, post_fut_seq_stride=196), "post_fut_seq_stride"),
])
def test_grad_create_refuses_bad_options(kw, needle):
    lib = gcconv.load_gcconv_library()
    h = ctypes.c_void_p()
    _refused(lib.tfft_gcconv_grad_create(4, 2, 8192, 130, 0, ctypes.byref(_gopts(**kw)), ctypes.byref(h)), needle, h)


def test_a_context_at_halo_0_is_refused():
    lib = gcconv.load_gcconv_library()
    h = ctypes.c_void_p()
    _refused(lib.tfft_gcconv_plan_create(1, 1, 8, 1, 0, ctypes.byref(_opts(history=8)), ctypes.byref(h)), "history must not exceed the halo", h)
    _refused(lib.tfft_gcconv_grad_create(1, 1, 8, 1, 0, ctypes.byref(_gopts(future=8)), ctypes.byref(h)), "future must not exceed the halo", h)


def test_null_arguments_are_refused():
    lib = gcconv.load_gcconv_library()
    assert lib.tfft_gcconv_plan_create(1, 1, 8, 1, 0, None, None) == ERR_ARG
    assert lib.tfft_gcconv_grad_create(1, 1, 8, 1, 0, None, None) == ERR_ARG
    assert lib.tfft_gcconv_describe(8, 1, 1, 1, 0, None, 0) == ERR_ARG
    assert lib.tfft_gcconv_grad_describe(8, 1, 1, 1, 0, 0, None, 0) == ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert lib.tfft_gcconv_describe(8, 1, 1, 1, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_gcconv_grad_describe(8, 1, 1, 1, 0, 0, small, len(small)) == ERR_ARG
    assert lib.tfft_gcconv_exec(None, None, None, None, None, None, None, None) == ERR_ARG
    assert lib.tfft_gcconv_plan_set_taps(None, None, None, None) == ERR_ARG
    assert lib.tfft_gcconv_plan_spectrum(None, None, None) == ERR_ARG
    assert lib.tfft_gcconv_plan_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_gcconv_plan_num_launches(None) == 0
    lib.tfft_gcconv_plan_destroy(None)
    assert lib.tfft_gcconv_grad_exec_input_grad(*([None] * 10)) == ERR_ARG
    assert lib.tfft_gcconv_grad_exec_tap_grad(*([None] * 10)) == ERR_ARG
    assert lib.tfft_gcconv_grad_set_taps(None, None, None, None) == ERR_ARG
    assert lib.tfft_gcconv_grad_spectrum(None, None, None) == ERR_ARG
    assert lib.tfft_gcconv_grad_set_workspace(None, None, 0) == ERR_ARG
    assert lib.tfft_gcconv_grad_prepare(None) == ERR_ARG
    assert lib.tfft_gcconv_grad_kernels(None, None, 0) == ERR_ARG
    assert lib.tfft_gcconv_grad_workspace_bytes(None) == 0 and lib.tfft_gcconv_grad_num_launches(None) == 0
    lib.tfft_gcconv_grad_destroy(None)
    assert lib.tfft_gcconv_last_error().decode()


def test_no_gpu_means_errors_not_fallbacks():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(tf.TfftError):
        tf.TfftGatedChunkedConvPlan(4, 2, 16384, 2049, 0, pre_gate=True, post_gate=True, history=2048)
    with pytest.raises(tf.TfftError):
        tf.TfftGatedChunkedConvGradPlan(1, 1, 8, 9, 0, pre_gate=True, history=8, future=8)
    with pytest.raises(tf.TfftError):
        tf.gated_chunked_causal_conv(torch.zeros((2, 2, 4096), dtype=torch.float16), torch.zeros((2, 7), dtype=torch.float16))


# ---- the identities of tests/test_gpu_gcconv.py in numpy

def _planes16(planes):
    return [np.ascontiguousarray(p).astype(np.float16).view(np.uint16) for p in planes]


@pytest.mark.parametrize("length,taps,rows,channels,ctx,_iters,mode", gc.CASE_MODES)
def test_carried_windows_are_windows_of_the_shipped_plans_on_the_concatenated_sequences(length, taps, rows, channels, ctx, _iters, mode):
    """bit for bit, binary16 product by binary16 product: what the three carried kernels put into LDS is what the shipped gated
    kernels put there for segments 1 .. of (forward, tap gradient) and segments 0 .. S - 1 of (input gradient) the concatenations"""
    d = gc.case_data(length, taps, rows, channels, ctx, "noise", 1, mode)
    halo, hop, segs = sr.geometry(length, taps)
    pairs = (rows + 1) // 2

    def later_segments(plane, total_segs, first):
        return plane.reshape(pairs, total_segs, channels, gc.N)[:, first:first + segs].reshape(-1, gc.N)

    # forward and pass (a) of the tap gradient
    cx, cpre, _ = gc.forward_concat(d, taps)
    assert cx.shape[2] == hop + length and sr.geometry(hop + length, taps)[2] == segs + 1
    ours = _planes16(gc.windows(d, taps))
    theirs = _planes16(later_segments(p, segs + 1, 1) for p in sr.windows(gb.gated(cx, cpre), taps))
    assert all(np.array_equal(a, b) for a, b in zip(ours, theirs))
    # input gradient: segments s of the plan at L + Fn; it may have one segment more, whose output lies beyond L
    cgy, cpost, cxx, cpp = gc.input_grad_concat(d)
    segs_long = sr.geometry(length + ctx, taps)[2]
    assert segs_long in (segs, segs + 1)
    ours = _planes16(gc.dx_windows(d, taps))
    theirs = _planes16(later_segments(p, segs_long, 0) for p in br.dx_windows(gb.gated(cgy, cpost), taps))
    assert all(np.array_equal(a, b) for a, b in zip(ours, theirs))
    if cpp is not None:                                                            # the store side's gates of the first L samples are the chunk's
        assert np.array_equal(cpp[:, :, :length], d["pre"]) and np.array_equal(cxx[:, :, :length], d["x"])
    # pass (b) of the tap gradient: the gz windows of segments 1 .., the extra items (p, 0) hold only zeros of gz
    tx, tpre, tgy, tpost = gc.tap_grad_concat(d, taps)
    zu, zg = br.dh_windows(gb.gated(tx, tpre), gb.gated(tgy, tpost), taps)
    mine_u, mine_g = cr.dh_windows(*[a for a in (gc.ue(d)[0], gc.gze(d)[0])], taps, gc.ue(d)[1])
    assert np.array_equal(later_segments(zu, segs + 1, 1), mine_u) and np.array_equal(later_segments(zg, segs + 1, 1), mine_g)
    assert not later_segments(zg, segs + 1, 0)[:, :1].any() and not zg.reshape(pairs, segs + 1, channels, gc.N)[:, 0].any()


def test_a_negative_gate_padding_is_the_minus_zero_trap():
    """0 * (-1) = -0: the same value, another bit pattern. The shipped kernel writes that product into its window where the carried
    kernel writes +0, so the concatenations pad the gates with +1"""
    d = gc.case_data(4104, 7, 3, 3, 8, "noise", 1, gc.EVERY_CASE_MODE)
    cx, cpre, _ = gc.forward_concat(d, 7)
    bad = gc.front_padded_gate(d["pre"], d["pre_hist"], 7, pad=-1.0)
    good, trap = gb.gated(cx, cpre), gb.gated(cx, bad)
    assert np.array_equal(good, trap) and not np.array_equal(good.view(np.uint16), trap.view(np.uint16))
    assert (trap.view(np.uint16)[:, :, :100] == 0x8000).all() and not good.view(np.uint16)[:, :, :100].any()


@pytest.mark.parametrize("length,taps,rows,channels,ctx,_iters", gc.WITH_CONTEXT)
def test_concatenation_identities_in_fp64(length, taps, rows, channels, ctx, _iters):
    """the definitions of include/tfft_gcconv.h (direct fp64 sums of the extended sequences) against the shipped operators' numpy
    models (tests/gsconv_ref.py, tests/gbconv_ref.py) on the concatenations"""
    d = gc.case_data(length, taps, rows, channels, ctx, "noise", 2, gc.EVERY_CASE_MODE)
    hop = sr.geometry(length, taps)[1]
    f = gb.f64
    cx, cpre, cpost = gc.forward_concat(d, taps)
    y = gs.model(f(cx), f(d["h"]), f(cpre), f(cpost), f(d["skip"]))[:, :, hop:]
    assert np.abs(y - gc.y_direct(d)).max() <= 1e-12
    cgy, cpost, cxx, cpp = gc.input_grad_concat(d)
    dx, dpre = gb.model_input_grad(cxx, d["h"], cpp, cpost, d["skip"], cgy)
    want_dx, want_dpre = gc.input_grad_direct(d)
    assert np.abs(dx[:, :, :length] - want_dx).max() <= 1e-12 and np.abs(dpre[:, :, :length] - want_dpre).max() <= 1e-12
    tx, tpre, tgy, tpost = gc.tap_grad_concat(d, taps)
    dh, dskip = gb.model_tap_grad(tx, tpre, tgy, tpost, taps)
    want_dh = gc.dh_direct(d, taps)
    assert np.abs(dh - want_dh).max() <= 1e-11 * max(1.0, np.abs(want_dh).max()) and np.array_equal(dskip, dh[:, 0])
    # the fp64 sum over the plan's own items (what the GPU test holds partials 0 and 2 to) is the direct sum of the rounded products
    u, uh = gc.ue(d)
    rounded = cr.dh_direct(u, gc.gze(d)[0], taps, uh)
    assert np.abs(br.dh_from_items(gc.dh_items(d, taps), channels, taps) - rounded).max() <= 1e-11 * max(1.0, np.abs(rounded).max())


def test_history_gradients_are_one_input_gradient_at_length_hn():
    """d loss / d history = pre_history (.) du_h and d loss / d pre_history = history (.) du_h with du_h[u] = sum_j h'[j] gz[u + j - Hn]:
    the input gradient at length Hn with x = history, pre = pre_history, a zero gy and future = gy[:carry_min], against torch.autograd
    through the fp64 operator on [history | x]"""
    length, taps, rows, channels = 4104, 7, 3, 3
    halo = sr.geometry(length, taps)[0]
    d = gc.case_data(length, taps, rows, channels, halo, "noise", 7, gc.EVERY_CASE_MODE)
    n = min(length, gc.carry_min(taps))
    ch = dict(gy=np.zeros((rows, channels, halo), np.float16), post=np.ones((rows, channels, halo), np.float16), fut=d["gy"][:, :, :n],
              post_fut=d["post"][:, :, :n], h=d["h"], skip=d["skip"], x=d["hist"], pre=d["pre_hist"])
    dhist, dphist = gc.input_grad_direct(ch)
    zeros, ones = np.zeros((rows, channels, halo), np.float16), np.ones((rows, channels, halo), np.float16)
    want = gb.autograd_reference(gc.extend(d["x"], d["hist"]), d["h"], gc.extend(d["pre"], d["pre_hist"]), gc.extend(d["post"], ones), d["skip"],
                                 gc.extend(d["gy"], zeros))
    assert np.abs(dhist - want["dx"][:, :, :halo]).max() <= 1e-12 and np.abs(dphist - want["dpre"][:, :, :halo]).max() <= 1e-12
