"""The masked short-frame ISTFT plan with its mask frames placed beyond 4 and 8 GiB of one device allocation (tests/far_layout.py):
include/tfft_mistftn.h promises a 64-bit mask_frame_stride, and the frames kernel keeps that promise only where g * mask_frame is
formed in 64 bits. One case at n = 512: three frames (three signals of one frame each: a pair and a self-paired last frame) whose
masks lie 2^31 + 8 halves apart, so that the last mask frame starts beyond 8 GiB. The result equals the dense execution (the default
mask stride) bit for bit, the mask arena's gaps still hold the sentinel afterwards and its blocks are unchanged. Skipped, as
tests/test_gpu_far_addresses.py skips, only when the device has less free memory than the arena and far_layout.Pool.HEADROOM."""
import numpy as np
import pytest

import far_layout as fl
import istftn_ref as inr
import mistftn_ref as mr
import stftn_ref as sn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
N, ROWS, LENGTH, HOP = 512, 3, 512, 512
MASK_STRIDE = (1 << 31) + 8


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    return tensor_fft_amd


@pytest.fixture(scope="module")
def pool():
    p = fl.Pool(torch, DEV)
    yield p
    p.release()


def test_mask_frames_beyond_8_gib(tf, pool):
    bins, pitch = sn.bins(N), sn.pitch(N)
    assert inr.geometry(N, LENGTH, HOP, 0) == 1
    x, w = sn.case_data(N, ROWS, LENGTH, window="random")
    re, im = inr.spectra16(x, w, HOP, 0)
    mask = mr.random_mask((ROWS, bins), 3)
    block = fl.Block(1 << 14, ROWS, MASK_STRIDE, bins)
    assert [2 * s >> 32 for s in block.starts()] == [0, 1, 2], "the mask frames start below 4 GiB, beyond 4 GiB and beyond 8 GiB"
    sizes = {"mask": (ROWS - 1) * MASK_STRIDE + fl.ROOM}
    short = pool.missing(sizes)
    if short:
        pytest.skip(f"needs {sizes['mask'] * 2 >> 30} GiB of HBM and {fl.Pool.HEADROOM >> 30} GiB of headroom: {short >> 20} MiB short")
    arena = pool.get(sizes)["mask"]
    arena.scatter(block, mask)
    # the spectra in the layout short_stft writes, sentinels beyond bin n / 2
    buf = np.full((ROWS, 2, pitch), fl.SENTINEL, np.int16)
    buf[:, 0, :bins], buf[:, 1, :bins] = re.view(np.int16), im.view(np.int16)
    d_in = torch.from_numpy(buf.reshape(-1)).to(DEV).view(torch.float16)
    d_w = torch.from_numpy(w.copy()).to(DEV)

    def run(mask_tensor, stride):
        plan = tf.TfftMaskedIstftPlan(N, ROWS, LENGTH, HOP, 0, 0, mask_frame_stride=stride)
        plan.set_window(d_w)
        out = torch.from_numpy(np.full(ROWS * LENGTH, fl.SENTINEL, np.int16)).to(DEV).view(torch.float16)
        plan.exec(d_in, d_in[pitch:], mask_tensor, out)
        torch.cuda.synchronize()
        plan.close()
        return out.cpu().numpy().view(np.int16).reshape(ROWS, LENGTH)

    far = run(arena.view(block).view(torch.float16), MASK_STRIDE)
    arena.check_gaps("mask arena")
    arena.check_block(block, mask, "mask arena")
    dense_mask = np.full((ROWS, pitch), fl.SENTINEL, np.int16)
    dense_mask[:, :bins] = mask.view(np.int16)
    dense = run(torch.from_numpy(dense_mask.reshape(-1)).to(DEV).view(torch.float16), 0)
    bad = np.argwhere(far != dense)
    assert bad.size == 0, f"the result at the far mask stride differs from the dense execution in {len(bad)} halves, first {bad[:3].tolist()}"
    assert np.isfinite(far.view(np.float16)).all() and far.any()
    # and both are the restatement's: the shipped inverse plan on the masked merge, then the numpy overlap-add
    import test_gpu_istftn as tn

    frames = tn.via_inverse_plan(tf, N, *mr.merge_items_masked(re, im, mask, N), ROWS)
    want = inr.ola(frames.view(np.float16), w, N, ROWS, LENGTH, HOP, 0).view(np.int16)
    tn._assert_bits("the far execution against merge_items_masked -> TfftPlan.exec_inverse -> istftn_ref.ola", far, want, ("signal", "sample"))
