"""Every transform kernel of the gfx950 code object, run by at least one plan and checked element by element against fp64.

CASES lists plans, each with the instantiations it exists for (reaches=). test_every_transform_kernel_is_reached compares the union
of what the plans launch (TfftPlan.kernels, tfft_plan_kernels & co.) with the kernels in the code object; test_case_against_fp64
runs each plan on seeded uniform(-1, 1) binary16 input, different for every transform, and checks every bin of every transform
with tests/elementwise_bound.py. Output buffers sit between guard zones of sentinel halves, and batch strides are padded (unequal
in / out) where the plan takes strides; guards and padding must come back bit for bit, and so must the input (preserve_input).
Flags of a case add an in-place run (bit-equal to out of place), an in-place run through stockham::copy_kernel (a caller's
workspace too small for a second block) and an inverse run against the fp64 inverse. tools/accuracy_per_kernel.py runs the same
CASES over three seeds and writes profiles/per_kernel_ulps.txt, where the K values of elementwise_bound.py come from."""
import os
import subprocess
import sys

import numpy as np
import pytest

import elementwise_bound as eb
from dist_emulate import GUARD, SENTINEL, _guarded, _untouched      # guard zones: shared with the distributed plans' emulator
from tensor_fft_amd import capi as _capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PREF, STAGE, NT, PLAIN = (_capi.VARIANT_K4096_PREFETCH, _capi.VARIANT_K4096_STAGE_OUT, _capi.VARIANT_K4096_NONTEMPORAL,
                          _capi.VARIANT_K4096_PLAIN)
AUTOSORT, COLPLAN, UNSTAGED, PACKED = (_capi.VARIANT_AUTOSORT_ONLY, _capi.VARIANT_COLUMN_PLAN, _capi.VARIANT_UNSTAGED_STORES,
                                       _capi.VARIANT_PACKED)
W_STAGED, W_SINCOS, PER_WAVE = _capi.VARIANT_COL_WAVE_STAGED, _capi.VARIANT_COL_WAVE_SINCOS, _capi.VARIANT_COL_PER_WAVE
CACHED, STREAMING, WG4 = _capi.VARIANT_COL_CACHED, _capi.VARIANT_COL_STREAMING, _capi.VARIANT_COL_WG4
NO512, NO1024, NO_FUSED, WIDEST = _capi.VARIANT_NO_RADIX512, _capi.VARIANT_NO_RADIX1024, _capi.VARIANT_NO_FUSED_TAIL, _capi.VARIANT_WIDEST_SPLIT
FLIP512, NO_LAT = _capi.VARIANT_FLIP_RADIX512_KERNEL, _capi.VARIANT_NO_LATENCY_KERNEL


def case(cid, reaches, kind="c", pad=(8, 24), inplace=False, copy=False, inverse=False, **kw):
    return dict(id=cid, reaches=reaches, kind=kind, pad=pad, inplace=inplace, copy=copy, inverse=inverse, kw=kw)


K4096 = "k4096::fft4096_kernel<{}, {}, {}>"
K256R = "k256r::fft256r_kernel<{}, {}, {}>"
K4096R = "k4096r::fft4096r_kernel<{}, {}, {}>"
WAVE = "colfft::colfft256_kernel<{}, {}, {}, {}>"
WG = "colfft::colfft256_wg_kernel<{}, {}, {}, {}, {}>"
C512 = "colfft::colfft512_wg_kernel<{}, {}, {}, {}>"
C512R = "colfft::colfft512r_wg_kernel<{}, {}, {}, {}>"
C1024 = "colfft::colfft1024_wg_kernel<{}, {}, {}, {}>"
LAT = "colfft::collat256_kernel<{}, {}, {}, {}, {}>"
F, T = "false", "true"
TR = "transposed"

CASES = [
    # ---- single-kernel plans; ragged batches against 2 transforms per wave (4096), 16 / R per wave (256 x R), 8 waves per workgroup
    case("k4096-default", [K4096.format(10, F, F)], n=4096, batch=37, inplace=True, inverse=True),
    case("k4096-plain", [K4096.format(0, F, F)], n=4096, batch=37, variant=PLAIN),
    case("k4096-prefetch", [K4096.format(1, F, F)], n=4096, batch=37, variant=PREF),
    case("k4096-stage", [K4096.format(2, F, F)], n=4096, batch=37, variant=STAGE),
    case("k4096-nt", [K4096.format(8, F, F)], n=4096, batch=37, variant=NT),
    case("k4096-prefetch-nt", [K4096.format(9, F, F)], n=4096, batch=1029, variant=PREF | NT),
    case("k256", ["k256::fft256_kernel<false>"], n=256, batch=1031, inplace=True, inverse=True),
    case("k256r-2", [K256R.format(2, T, F)], n=512, batch=517, inplace=True, inverse=True),
    case("k256r-2-direct", [K256R.format(2, F, F)], n=512, batch=517, variant=UNSTAGED),
    case("k256r-4", [K256R.format(4, T, F)], n=1024, batch=259),
    case("k256r-4-direct", [K256R.format(4, F, F)], n=1024, batch=259, variant=UNSTAGED),
    case("k256r-8", [K256R.format(8, T, F)], n=2048, batch=131, inverse=True),
    case("k256r-8-direct", [K256R.format(8, F, F)], n=2048, batch=131, variant=UNSTAGED),
    case("k4096r-2", [K4096R.format(2, F, F)], n=8192, batch=259, inplace=True, inverse=True),
    case("k4096r-4", [K4096R.format(4, F, F)], n=16384, batch=3, variant=PREF),
    case("k4096r-8", [K4096R.format(8, F, F)], n=32768, batch=129),
    # ---- Stockham passes: autosort chains, the fused radix-32 / 64 tails, two butterflies per thread, cooperative tails, the copy
    case("stockham-16", ["stockham::pass_kernel<16>"], n=256, batch=5, variant=AUTOSORT, inverse=True),
    case("stockham-2", ["stockham::pass_kernel<2>"], n=512, batch=5, variant=AUTOSORT, copy=True),
    case("stockham-4", ["stockham::pass_kernel<4>"], n=1024, batch=5, variant=AUTOSORT),
    case("stockham-8", ["stockham::pass_kernel<8>"], n=2048, batch=5, variant=AUTOSORT, inplace=True),
    case("stockham-32", ["stockham::pass_kernel<32>"], n=8192, batch=3, variant=COLPLAN | PACKED),
    case("stockham-64", ["stockham::pass_kernel<64>"], n=16384, batch=3, variant=COLPLAN | PACKED),
    case("coop-32", ["stockham::tail_coop_kernel<32>", LAT.format(0, 1, 1, 4, 2)], n=8192, batch=1, inplace=True, inverse=True),
    case("coop-64", ["stockham::tail_coop_kernel<64>"], n=16384, batch=2),
    case("coop-128", ["stockham::tail_coop_kernel<128>"], n=32768, batch=1),
    case("pair-2", ["stockham::pass_pair_kernel<2>", WAVE.format(1, 1, F, T)], n=512, batch=3, inner=16),
    case("pair-4", ["stockham::pass_pair_kernel<4>"], n=1024, batch=3, inner=16),
    case("pair-8", ["stockham::pass_pair_kernel<8>"], n=2048, batch=1, inner=16),
    case("copy-in-place", ["stockham::copy_kernel"], n=1 << 17, batch=2, variant=NO512 | NO1024, copy=True),
    # ---- per-wave radix-256 kernel (COL_PER_WAVE / COL_WAVE_STAGED / COL_WAVE_SINCOS, or a pitch of 16): 16-column tiles
    case("wave-lanes", [WAVE.format(0, 1, F, T)], n=8192, batch=5, variant=COLPLAN | PER_WAVE),
    case("wave-lanes-staged", [WAVE.format(0, 1, T, T)], n=8192, batch=5, variant=COLPLAN | W_STAGED, inplace=True),
    case("wave-lanes-sincos", [WAVE.format(0, 1, F, F)], n=8192, batch=5, variant=COLPLAN | W_SINCOS),
    case("wave-sincos-2^16", [WAVE.format(1, 0, F, F)], n=1 << 16, batch=3, variant=W_SINCOS, inverse=True),
    case("wave-staged-sincos-2^16", [WAVE.format(0, 1, T, F), WAVE.format(1, 0, T, F)], n=1 << 16, batch=3, variant=W_STAGED | W_SINCOS),
    case("wave-regs", [WAVE.format(1, 0, F, F)], n=256, batch=3, inner=16),
    case("wave-regs-staged", [WAVE.format(1, 0, T, F)], n=256, batch=3, inner=16, variant=W_STAGED),
    case("wave-regs-tw-staged", [WAVE.format(1, 1, T, T)], n=512, batch=3, inner=16, variant=W_STAGED),
    case("wave-regs-tw-sincos", [WAVE.format(1, 1, F, F)], n=512, batch=3, inner=16, variant=W_SINCOS),
    case("wave-regs-tw-staged-sincos", [WAVE.format(1, 1, T, F)], n=512, batch=3, inner=16, variant=W_STAGED | W_SINCOS),
    # ---- workgroup-cooperative radix-256 kernel: W = 4 / 8 waves, non-temporal or plain, staged or direct stores
    case("wg4-lanes-nt-stg", [WG.format(0, 1, T, 4, T)], n=1 << 14, batch=1, variant=COLPLAN | NO_LAT),
    case("wg8-lanes-nt-stg", [WG.format(0, 1, T, 8, T)], n=1 << 14, batch=2, variant=COLPLAN | NO_LAT),
    case("wg4-lanes-nt", [WG.format(0, 1, T, 4, F), WG.format(1, 0, T, 4, F)], n=1 << 16, batch=3, variant=UNSTAGED | NO_LAT, inplace=True),
    case("wg4-lanes-plain-stg", [WG.format(0, 1, F, 4, T), WG.format(1, 0, F, 4, F)], n=1 << 16, batch=3, variant=CACHED | NO_LAT),
    case("wg4-lanes-plain", [WG.format(0, 1, F, 4, F)], n=1 << 16, batch=17, variant=CACHED | UNSTAGED),
    case("wg8-lanes-plain-stg", [WG.format(0, 1, F, 8, T)], n=8192, batch=129, variant=COLPLAN | CACHED),
    case("wg8-lanes-nt", [WG.format(0, 1, T, 8, F)], n=8192, batch=129, variant=COLPLAN | UNSTAGED),
    case("wg8-lanes-plain", [WG.format(0, 1, F, 8, F), WG.format(1, 1, F, 8, F)], n=1 << 19, batch=17, variant=NO512 | UNSTAGED),
    case("wg4-regs-tw-nt", [WG.format(1, 1, T, 4, F)], n=1 << 17, batch=1, variant=NO512 | NO_LAT, inverse=True),
    case("wg4-regs-tw-plain", [WG.format(1, 1, F, 4, F)], n=1 << 19, batch=1, variant=NO512 | NO_LAT),
    case("wg8-regs-tw-nt", [WG.format(1, 1, T, 8, F)], n=2048, batch=1, inner=4096),
    case("wg8-regs-tw-plain", [WG.format(1, 1, F, 8, F)], n=2048, batch=1, inner=4096, variant=CACHED),
    case("wg8-regs-plain", [WG.format(1, 0, F, 8, F)], n=1 << 18, batch=33, variant=NO512),
    case("wg8-regs-input-transposed", [WG.format(1, 0, T, 8, F), K4096R.format(8, F, T)], n=1 << 23, batch=1, input_order=TR, pad=None),
    case("wg4-fourstep-nt", [WG.format(1, 2, T, 4, F), "k256::fft256_kernel<false>"], n=1 << 16, batch=3, output_order=TR, pad=None),
    case("wg8-fourstep-nt", [WG.format(1, 2, T, 8, F)], n=1 << 23, batch=1, output_order=TR, pad=None),
    case("wg4-fourstep-plain", [WG.format(1, 2, F, 4, F)], n=1 << 22, batch=3, output_order=TR, pad=None),
    case("wg8-fourstep-plain", [WG.format(1, 2, F, 8, F)], n=1 << 23, batch=3, output_order=TR, pad=None),
    # ---- radix-512 / radix-1024 column kernels, the two-round radix-512 kernel, the scale-once read-outs (SC)
    case("c512-lanes", [C512.format(0, 1, F, F), "stockham::pass_kernel<16>"], n=1 << 15, batch=1, variant=COLPLAN | NO_FUSED),
    case("c512-lanes-plain", [C512.format(0, 1, F, T)], n=1 << 15, batch=1, variant=COLPLAN | CACHED),
    case("c512-regs", [C512.format(1, 0, F, F)], n=1 << 18, batch=1, variant=FLIP512 | STREAMING),
    case("c512-regs-plain", [C512.format(1, 0, F, T)], n=1 << 18, batch=1, variant=FLIP512),
    case("c512-regs-once", [C512.format(1, 0, T, F)], n=1 << 18, batch=3, variant=FLIP512, scale="once"),
    case("c512-regs-tw", [C512.format(1, 1, F, F)], n=1 << 21, batch=1, variant=PREF),
    case("c512-regs-tw-plain", [C512.format(1, 1, F, T)], n=1 << 19, batch=1, variant=WIDEST | NO1024),
    case("c512-fourstep", [C512.format(1, 2, F, F)], n=1 << 21, batch=1, output_order=TR, pad=None),
    case("c512-fourstep-plain", [C512.format(1, 2, F, T)], n=1 << 24, batch=1, output_order=TR, pad=None),
    case("c512r-8-plain", [C512R.format(8, F, T, T)], n=1 << 18, batch=1, variant=PREF, inplace=True),
    case("c512r-8", [C512R.format(8, F, T, F)], n=1 << 18, batch=1, variant=STREAMING),
    case("c512r-4-plain", [C512R.format(4, F, F, T)], n=1 << 18, batch=1, variant=WG4),
    case("c512r-4", [C512R.format(4, F, F, F)], n=1 << 18, batch=1, variant=WG4 | STREAMING),
    case("c512r-8-once", [C512R.format(8, T, T, F)], n=1 << 18, batch=3, variant=PREF, scale="once", inverse=True),
    case("c512r-4-once", [C512R.format(4, T, F, F)], n=1 << 18, batch=3, variant=WG4, scale="once"),
    case("c1024-lanes", [C1024.format(0, 1, F, F)], n=1 << 16, batch=1, variant=WIDEST),
    case("c1024-lanes-plain", [C1024.format(0, 1, F, T)], n=1 << 16, batch=1, variant=WIDEST | CACHED),
    case("c1024-regs-plain", [C1024.format(1, 0, F, T)], n=1 << 19, batch=1, variant=PREF, inplace=True, inverse=True),
    case("c1024-regs", [C1024.format(1, 0, F, F)], n=1 << 19, batch=1, variant=STREAMING),
    case("c1024-regs-once", [C1024.format(1, 0, T, F)], n=1 << 19, batch=3, variant=PREF, scale="once"),
    case("c1024-regs-tw", [C1024.format(1, 1, F, F)], n=1 << 21, batch=1, variant=WIDEST),
    case("c1024-regs-tw-plain", [C1024.format(1, 1, F, T)], n=1 << 21, batch=1, variant=WIDEST | CACHED),
    case("scale-none", [], n=1 << 16, batch=3, scale="none", inverse=True),
    # ---- latency kernel (work that does not fill the chip): CG x HH shapes, two workgroups per block (PP = 2) or one
    case("lat-1x4-regs", [LAT.format(1, 0, 1, 4, 2)], n=256, batch=1, inner=64),
    case("lat-1x4-regs-tw", [LAT.format(1, 1, 1, 4, 2)], n=512, batch=1, inner=64),
    case("lat-2x2-lanes", [LAT.format(0, 1, 2, 2, 2)], n=8192, batch=33, variant=COLPLAN),
    case("lat-2x2-regs", [LAT.format(1, 0, 2, 2, 2)], n=1 << 16, batch=5, inplace=True, inverse=True),
    case("lat-2x2-regs-tw", [LAT.format(1, 1, 2, 2, 2)], n=512, batch=3, inner=256),
    case("lat-2x2-pp1", [LAT.format(0, 1, 2, 2, 1), LAT.format(1, 1, 2, 2, 1)], n=1 << 18, batch=5, variant=NO512 | NO1024),
    case("lat-2x2-pp1-last", [LAT.format(1, 0, 2, 2, 1)], n=1 << 18, batch=5, variant=NO512),
    # ---- transposed-input plans: row passes with the output twiddle in their epilogue (OTW), then one column pass
    case("k256-otw", ["k256::fft256_kernel<true>", LAT.format(1, 0, 1, 4, 2)], n=1 << 16, batch=1, input_order=TR, pad=None),
    case("k256r-2-otw", [K256R.format(2, T, T), LAT.format(1, 0, 2, 2, 2)], n=1 << 17, batch=3, input_order=TR, pad=None),
    case("k256r-4-otw", [K256R.format(4, T, T)], n=1 << 18, batch=1, input_order=TR, pad=None),
    case("k256r-8-otw", [K256R.format(8, T, T)], n=1 << 19, batch=1, input_order=TR, pad=None),
    case("k4096-otw", [K4096.format(10, T, F)], n=1 << 20, batch=1, input_order=TR, pad=None),
    case("k4096r-4-otw", [K4096R.format(4, F, T)], n=1 << 22, batch=1, input_order=TR, pad=None),
    # ---- real-input plans: fused N = 4096 R2C, split / merge passes (non-temporal and plain); odd batches pair the last with itself
    case("real-4096-fused", [K4096.format(10, F, T), "rfft::merge_kernel<true>"], kind="r", n=4096, batch=37),
    case("real-2^18", ["rfft::merge_kernel<false>", "rfft::split_kernel<false>"], kind="r", n=1 << 18, batch=3),
    case("real-2^13-two-pass", ["rfft::split_kernel<true>"], kind="r", n=8192, batch=5, two_pass=True),
    # ---- 2D: the fused 4096 x 4096 plan (radix-8 column butterfly in front of the 4096-point rows), and a row + column plan
    case("2d-4096x4096", [K4096R.format(8, T, F)], kind="2d", rows=4096, cols=4096, batch=1),
    case("2d-512x1024", [], kind="2d", rows=512, cols=1024, batch=3),
]

# Kernels that are not transforms of a plan, by name, with the test that covers each
EXCLUDED = {
    "synth::uniform_kernel": "input generator (the tests that compare device-generated input with orc.synth_uniform: test_gpu_round4.py)",
    "permute::permute_twiddle_kernel": "distributed pack / unpack step (test_gpu_distributed.py::test_permute_twiddle_kernel)",
    "permute::interleave_kernel": "layout adapter (test_gpu_parity.py::test_layout_adapters_roundtrip)",
    "permute::deinterleave_kernel": "layout adapter (test_gpu_parity.py::test_layout_adapters_roundtrip)",
}
# Rows of the column dispatch table that only the debug build selects:
#  - columns on lanes without the next pass's twiddles (MODE 0, TW 0) is a column pass that is both the first and the last of a
#    contiguous axis. No plan has one: N = 256 .. 2048 are single kernels, and a longer contiguous transform has a second pass.
#    The debug build's no-twiddle bit plans it.
#  - the latency kernel's CG = 4 shapes: only the debug build's TFFT_LAT_SHAPE knob picks them.
DEBUG_ONLY = sorted(
    [WAVE.format(0, 0, s, F) for s in (F, T)]
    + [WG.format(0, 0, nt, w, st) for nt in (F, T) for w in (4, 8) for st in (F, T)]
    + [C512.format(0, 0, F, p) for p in (F, T)] + [C1024.format(0, 0, F, p) for p in (F, T)]
    + [LAT.format(m, t, 4, 2, 1) for m in (0, 1) for t in (0, 1)]
    + [LAT.format(0, 0, cg, hh, pp) for cg, hh in ((2, 2), (1, 4)) for pp in (1, 2)]
)
# Shipped rows a whole MI355X never selects, so no test on one can run them (a finding, not a debug path): the latency kernel's
# CG = 1 shape with one workgroup per block (PP = 1). A pass of at most 64 such workgroups falls back to PP = 1 only where that is
# more than half the device's CUs, i.e. on a device of fewer than 128 CUs (a partition of the chip).
PARTITION_ONLY = sorted(LAT.format(m, t, 1, 4, 1) for m, t in ((0, 1), (1, 0), (1, 1)))


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd as t

    t.device_check(0)
    return t


def make_plan(tf, c, default_strides=False, **extra):
    kw = dict(c["kw"])
    if c["kind"] == "2d":
        return tf.TfftPlan2D(kw["rows"], kw["cols"], kw["batch"], 0)
    if c["kind"] == "r":
        return tf.TfftRealPlan(kw.pop("n"), kw.pop("batch"), 0, **kw, **extra)
    n, batch = kw.pop("n"), kw.pop("batch")
    inner = kw.get("inner", 1)
    if c["pad"] and not default_strides:
        kw["in_batch_stride"] = 2 * n * inner + c["pad"][0]
        kw["out_batch_stride"] = 2 * n * inner + c["pad"][1]
    kw.update(extra)
    return tf.TfftPlan(n, batch, 0, **kw)


def small_workspace(torch, plan):
    """one workspace block, not two: an odd chain in place then starts from a copy of the input (stockham::copy_kernel)"""
    return torch.empty(max(8, plan.workspace_bytes // 2), dtype=torch.float16, device="cuda")


def in_place_plan(tf, torch, c):
    p = make_plan(tf, c, default_strides=True)
    if c["copy"]:
        p.set_workspace(small_workspace(torch, p))
    return p


def case_kernels(tf, torch, c):
    plan = make_plan(tf, c)
    if c["kind"] == "r":
        return set(plan.kernels(False)) | set(plan.kernels(True))
    ks = set(plan.kernels)
    if c["inplace"] or c["copy"]:
        ks |= set(in_place_plan(tf, torch, c).kernels_in_place)
    return ks


def shipped_kernels():
    """the kernels of the gfx950 code object, as c++filt names them without their parameter lists (as test_isa_lint.py)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint

    mangled = list(isa_lint.split_kernels(isa_lint.disassemble(os.path.join(ROOT, "tensor-fft_amd", "libtfft.so"))))
    out = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    return {(d[5:] if d.startswith("void ") else d).split("(")[0] for d in (x.strip() for x in out) if d}


def test_every_transform_kernel_is_reached(tf):
    import torch

    shipped = shipped_kernels()
    named = set(EXCLUDED) | set(DEBUG_ONLY) | set(PARTITION_ONLY)
    assert named <= shipped, sorted(named - shipped)
    reached, lost = set(), []
    for c in CASES:
        ks = case_kernels(tf, torch, c)
        lost += [(c["id"], k) for k in c["reaches"] if k not in ks]
        reached |= ks
    assert not lost, f"cases that no longer launch what they exist for: {lost}"
    assert reached <= shipped, sorted(reached - shipped)
    assert not reached & named, f"excluded kernels a case launches after all: {sorted(reached & named)}"
    missing = shipped - reached - named
    assert not missing, f"transform kernels no case launches: {sorted(missing)}"


def arithmetic_class(kernels, c):
    """real-input plans; hardware v_sin / v_cos twiddles anywhere in the plan (collat256_kernel, colfft256_kernel<.., false>);
    table twiddles"""
    if c["kind"] == "r":
        return "real"
    if any("collat256" in k or (k.startswith("colfft::colfft256_kernel<") and k.endswith(", false>")) for k in kernels):
        return "sincos"
    return "table"


def k_of(kernels, c):
    return {"real": eb.K_REAL, "sincos": eb.K_SINCOS, "table": eb.K_TABLE}[arithmetic_class(kernels, c)]


def _bits(torch, dev):
    return dev.view(torch.int16).cpu().numpy()


def _ends(a):
    return np.concatenate([a[:GUARD], a[-GUARD:]])


def run_complex(tf, orc, torch, c, seed):
    """{kernel: worst ulps} over the runs of one case (forward, in place, inverse)"""
    kw = c["kw"]
    n, batch, inner = kw["n"], kw["batch"], kw.get("inner", 1)
    nf = n * inner                       # halves per plane of one transform
    scale = kw.get("scale", "sequential")
    plan = make_plan(tf, c, preserve_input=True)
    ins, outs = plan.in_batch_stride, plan.out_batch_stride
    rng = np.random.default_rng([seed, n, batch, inner])
    x = rng.uniform(-1, 1, (batch, 2, nf)).astype(np.float16)
    if scale == "none":                  # unscaled output: keep it inside binary16
        x = (x * np.float16(min(1.0, 4096.0 / n))).astype(np.float16)
    n2 = tf.transposed_n2(n) if TR in (kw.get("input_order"), kw.get("output_order")) else 0
    xin = x
    if kw.get("input_order") == TR:      # x[p + N1 q] at q + N2 p
        xin = np.ascontiguousarray(x.reshape(batch, 2, n2, n // n2).transpose(0, 1, 3, 2)).reshape(batch, 2, n)
    host_in = np.full(GUARD + (batch - 1) * ins + 2 * nf + GUARD, SENTINEL, dtype=np.int16)
    for b in range(batch):
        host_in[GUARD + b * ins:GUARD + b * ins + 2 * nf] = xin[b].reshape(-1).view(np.int16)
    len_out = (batch - 1) * outs + 2 * nf
    d_in = torch.from_numpy(host_in).cuda().view(torch.float16)
    d_out = _guarded(torch, len_out)
    before = _bits(torch, d_out)
    a_in, a_out = d_in[GUARD:GUARD + (batch - 1) * ins + 2 * nf], d_out[GUARD:GUARD + len_out]
    outside = np.ones(before.size, dtype=bool)
    for b in range(batch):
        outside[GUARD + b * outs:GUARD + b * outs + 2 * nf] = False

    def gather(o):
        return np.stack([o[GUARD + b * outs:GUARD + b * outs + 2 * nf] for b in range(batch)]).reshape(batch, 2, nf)

    plan.exec(a_in, a_in[nf:], a_out, a_out[nf:])
    torch.cuda.synchronize()
    _untouched(_bits(torch, d_in), host_in, f"{c['id']}: input (preserve_input)")
    o = _bits(torch, d_out)
    _untouched(o[outside], before[outside], f"{c['id']}: guard zones and stride padding")
    fwd = gather(o)
    got = fwd.view(np.float16).astype(np.float64)
    xc = (x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)).reshape(batch, n, inner)
    if inner == 1:
        e_re, e_im = orc.dft64(x[:, 0], x[:, 1])
        ref = (e_re + 1j * e_im).reshape(batch, n, 1)
    else:
        ref = np.fft.fft(xc, axis=1) / n
    if scale == "none":
        ref = ref * n
    if kw.get("output_order") == TR:     # X[k1 + N1 k2] at k1 N2 + k2
        ref = ref.reshape(batch, n2, n // n2).transpose(0, 2, 1)
    ref = ref.reshape(batch, nf)
    kernels = plan.kernels
    k = k_of(kernels, c)
    launched = set(kernels)
    worst = eb.check(got[:, 0], got[:, 1], ref.real, ref.imag, k, what=f"{c['id']} seed {seed}")
    res = {kk: worst for kk in kernels}
    if c["inplace"] or c["copy"]:
        p2 = in_place_plan(tf, torch, c)
        ran = p2.kernels_in_place
        assert ("stockham::copy_kernel" in ran) == c["copy"], ran
        launched |= set(ran)
        buf = _guarded(torch, batch * 2 * nf, xin)
        b0 = _bits(torch, buf)
        a = buf[GUARD:GUARD + batch * 2 * nf]
        p2.exec(a, a[nf:], a, a[nf:])
        torch.cuda.synchronize()
        o2 = _bits(torch, buf)
        _untouched(_ends(o2), _ends(b0), f"{c['id']}: in place, guard zones")
        assert np.array_equal(o2[GUARD:GUARD + batch * 2 * nf].reshape(batch, 2, nf), fwd), f"{c['id']}: in place differs from out of place"
        for kk in ran:
            res[kk] = max(res.get(kk, 0.0), worst)
    if c["inverse"]:
        plan.exec_inverse(a_in, a_in[nf:], a_out, a_out[nf:])
        torch.cuda.synchronize()
        o = _bits(torch, d_out)
        _untouched(o[outside], before[outside], f"{c['id']}: inverse, guard zones and stride padding")
        gi = gather(o).view(np.float16).astype(np.float64)
        inv = (np.fft.ifft(xc, axis=1) * (n if scale == "none" else 1)).reshape(batch, nf)
        w = eb.check(gi[:, 0], gi[:, 1], inv.real, inv.imag, k, what=f"{c['id']} inverse seed {seed}")
        for kk in kernels:
            res[kk] = max(res[kk], w)
    assert set(c["reaches"]) <= launched, sorted(set(c["reaches"]) - launched)
    return res


def run_real(tf, torch, c, seed):
    kw = c["kw"]
    n, batch = kw["n"], kw["batch"]
    plan = make_plan(tf, c)
    h, pitch, ss = n // 2 + 1, plan.pitch, plan.out_batch_stride
    rng = np.random.default_rng([seed, n, batch, 2])
    x = rng.uniform(-1, 1, (batch, n)).astype(np.float16)
    d_x = _guarded(torch, batch * n, x)
    x_bits = _bits(torch, d_x)
    len_s = (batch - 1) * ss + 2 * pitch
    d_s = _guarded(torch, len_s)
    before = _bits(torch, d_s)
    s = d_s[GUARD:GUARD + len_s]
    plan.r2c(d_x[GUARD:GUARD + batch * n], s, s[pitch:])
    torch.cuda.synchronize()
    _untouched(_bits(torch, d_x), x_bits, f"{c['id']}: r2c input")
    o = _bits(torch, d_s)
    outside = np.ones(o.size, dtype=bool)
    for b in range(batch):
        outside[GUARD + b * ss:GUARD + b * ss + h] = False
        outside[GUARD + b * ss + pitch:GUARD + b * ss + pitch + h] = False
    _untouched(o[outside], before[outside], f"{c['id']}: r2c guard zones and pitch padding")
    of = o.view(np.float16).astype(np.float64)
    g_re = np.stack([of[GUARD + b * ss:GUARD + b * ss + h] for b in range(batch)])
    g_im = np.stack([of[GUARD + b * ss + pitch:GUARD + b * ss + pitch + h] for b in range(batch)])
    ref = np.fft.rfft(x.astype(np.float64), axis=1) / n
    w = eb.check(g_re, g_im, ref.real, ref.imag, eb.K_REAL, pairs=True, what=f"{c['id']} r2c seed {seed}")
    res = {kk: w for kk in plan.kernels(False)}
    # C2R of half spectra of binary16 size: X = fp16(rfft(x) / sqrt(n)); irfft(X, n) is about x / sqrt(n)
    spec = np.fft.rfft(x.astype(np.float64), axis=1) / np.sqrt(n)
    s_host = np.zeros(len_s, dtype=np.float16)
    for b in range(batch):
        s_host[b * ss:b * ss + h] = spec[b].real.astype(np.float16)
        s_host[b * ss + pitch:b * ss + pitch + h] = spec[b].imag.astype(np.float16)
    d_in = torch.from_numpy(s_host).cuda()
    d_y = _guarded(torch, batch * n)
    y0 = _bits(torch, d_y)
    plan.c2r(d_in, d_in[pitch:], d_y[GUARD:GUARD + batch * n])
    torch.cuda.synchronize()
    _untouched(_bits(torch, d_in), s_host.view(np.int16), f"{c['id']}: c2r input")
    y = _bits(torch, d_y)
    _untouched(_ends(y), _ends(y0), f"{c['id']}: c2r guard zones")
    got = y[GUARD:GUARD + batch * n].view(np.float16).astype(np.float64).reshape(batch, n)
    sf = s_host.astype(np.float64)
    xs = np.stack([sf[b * ss:b * ss + h] + 1j * sf[b * ss + pitch:b * ss + pitch + h] for b in range(batch)])
    want = np.fft.irfft(xs, n, axis=1)
    w2 = eb.check(got, np.zeros_like(got), want, np.zeros_like(want), eb.K_REAL, pairs=True, what=f"{c['id']} c2r seed {seed}")
    for kk in plan.kernels(True):
        res[kk] = max(res.get(kk, 0.0), w2)
    assert set(c["reaches"]) <= set(res), sorted(set(c["reaches"]) - set(res))
    return res


def run_2d(tf, torch, c, seed):
    kw = c["kw"]
    rows, cols, batch = kw["rows"], kw["cols"], kw["batch"]
    plan = make_plan(tf, c)
    m = batch * rows * cols
    rng = np.random.default_rng([seed, rows, cols, batch])
    x = rng.uniform(-1, 1, (2, m)).astype(np.float16)
    d_re, d_im = _guarded(torch, m, x[0]), _guarded(torch, m, x[1])
    o_re, o_im = _guarded(torch, m), _guarded(torch, m)
    g0 = _bits(torch, o_re)
    plan.exec(d_re[GUARD:GUARD + m], d_im[GUARD:GUARD + m], o_re[GUARD:GUARD + m], o_im[GUARD:GUARD + m])
    torch.cuda.synchronize()
    out = []
    for buf in (o_re, o_im):
        hb = _bits(torch, buf)
        _untouched(_ends(hb), _ends(g0), f"{c['id']}: guard zones")
        out.append(hb[GUARD:GUARD + m].view(np.float16).astype(np.float64).reshape(batch, rows * cols))
    xc = x[0].astype(np.float64) + 1j * x[1].astype(np.float64)
    ref = (np.fft.fft2(xc.reshape(batch, rows, cols)) / (rows * cols)).reshape(batch, rows * cols)
    kernels = plan.kernels
    w = eb.check(out[0], out[1], ref.real, ref.imag, k_of(kernels, c), what=f"{c['id']} seed {seed}")
    assert set(c["reaches"]) <= set(kernels), sorted(set(c["reaches"]) - set(kernels))
    return {kk: w for kk in kernels}


def run_case(tf, orc, torch, c, seed):
    if c["kind"] == "r":
        return run_real(tf, torch, c, seed)
    if c["kind"] == "2d":
        return run_2d(tf, torch, c, seed)
    return run_complex(tf, orc, torch, c, seed)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["id"])
def test_case_against_fp64(tf, orc, c):
    import torch

    run_case(tf, orc, torch, c, 1)
