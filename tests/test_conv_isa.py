"""CPU-side checks of the gfx950 ISA inside libtfft_conv.so (tools/isa_lint.py), the rules tests/test_isa_lint.py holds libtfft.so to:
no packed fp32 arithmetic in the MFMA kernel (the filter multiply sits right behind stage 3's MFMAs), every MFMA -> consumer wait
state present, and no program end reachable behind an LDS-DMA without an s_waitcnt vmcnt(0)."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def text():
    import __graft_entry__ as g
    import isa_lint

    g.build()
    return isa_lint.disassemble(os.path.join(ROOT, "tensor-fft_amd", "libtfft_conv.so"))


@pytest.fixture(scope="module")
def report(text):
    import isa_lint

    return isa_lint.lint_text(text)


def _one(report, needle):
    names = [k for k in report if needle in k]
    assert len(names) == 1, names
    return report[names[0]]


def test_code_object_holds_exactly_the_two_kernels(report):
    assert len(report) == 2, list(report)
    fused, cmul = _one(report, "conv4096_kernel"), _one(report, "cmul_kernel")
    # two transforms of 16 stage-1 tiles and 16 stage-2/3 tiles, two MFMAs per complex product
    assert fused["mfma"] == 2 * (16 * 2 + 16 * 4)
    assert cmul["mfma"] == 0 and not cmul["lds_dma"]


def test_no_packed_fp32_next_to_the_mfmas(report):
    assert _one(report, "conv4096_kernel")["pk_f32"] == 0


def test_wait_states_and_dma_drain(report):
    fused = _one(report, "conv4096_kernel")
    assert fused["lds_dma"], "the fused kernel loads through LDS-DMA"
    assert not fused["findings"], fused["findings"]
    assert not _one(report, "cmul_kernel")["findings"]


def test_fused_kernel_resources():
    """no scratch, and at most 256 VGPRs: two waves per SIMD, the eight waves of a workgroup that owns the CU's 160 KiB of LDS (read
    from the kernel metadata notes of the code object)"""
    import __graft_entry__ as g
    import isa_lint

    g.build()
    tmp = tempfile.mkdtemp(prefix="tfft_conv_isa_")
    try:
        local = os.path.join(tmp, "libtfft_conv.so")
        shutil.copy(os.path.join(ROOT, "tensor-fft_amd", "libtfft_conv.so"), local)
        subprocess.check_call([os.path.join(isa_lint.LLVM_BIN, "llvm-objdump"), "--offloading", local], cwd=tmp,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f][0]
        notes = subprocess.check_output([os.path.join(isa_lint.LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(tmp, co)], text=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    blocks = [b for b in notes.split("- .agpr_count") if "conv4096_kernel" in b]
    assert len(blocks) == 1
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", blocks[0]).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blocks[0]).group(1))
    spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blocks[0]).group(1))
    assert scratch == 0 and spills == 0 and vgprs <= 256, (vgprs, scratch, spills)
