"""tests/far_layout.py without a GPU: the two layouts reach the address bands they are there for (exact Python integers), and the
scatter, gather and gap code the GPU tests trust is held to a dense numpy restatement at a shrunken stride, where a dense mask is
affordable. A deliberately wrong offset (a 32-bit product in place of the 64-bit one, restated at the shrunken stride as a
product taken modulo a small power of two) is caught by the gap check, the block check or the gather: what
tests/test_gpu_far_addresses.py relies on to notice a truncated `row * stride` in a kernel."""
import numpy as np
import pytest

import far_layout as fl

LENGTH = 4104                        # the overlap-save families' L in tests/test_gpu_far_addresses.py


def test_the_layouts_are_the_ones_documented():
    w, c = fl.LAYOUTS["wide"], fl.LAYOUTS["channels"]
    assert (w.rows, w.channels, w.in_stride, w.out_stride) == (3, 1, 2 ** 31 + 8, 2 ** 31 + 24)
    assert (c.rows, c.channels, c.in_stride, c.out_stride) == (2, 2, 2 ** 30 + 8, 2 ** 30 + 24)
    for lay in (w, c):
        assert lay.in_stride % 8 == 0 and lay.out_stride % 8 == 0 and lay.in_stride != lay.out_stride
    assert (fl.FRAME_ROWS, fl.FRAMES_PER_ROW) == (3, 2)


@pytest.mark.parametrize("side", fl.SIDES)
def test_block_starts_reach_every_band(side):
    starts = [b for lay in fl.LAYOUTS.values() for b in fl.bands(lay, side, LENGTH)]
    assert any(2 ** 31 < b < 2 ** 32 for b in starts)
    assert any(2 ** 32 < b < 2 ** 33 for b in starts)
    assert any(b > 2 ** 33 for b in starts)
    assert any(b // 2 > 2 ** 32 for b in starts)              # a start INDEX in halves that no uint32_t holds
    # each layout on its own crosses 2^32 bytes; `wide` has the base beyond 2^33, `channels` a +c term and a pair distance
    # (channels * stride) that each cross a line
    w = fl.bands(fl.LAYOUTS["wide"], side, LENGTH)
    assert w[0] == 0 and 2 ** 32 < w[1] < 2 ** 33 < w[2]
    c = fl.bands(fl.LAYOUTS["channels"], side, LENGTH)
    assert c[0] == 0 and 2 ** 31 < c[1] < 2 ** 32 < c[2] < c[3] < 2 ** 33
    assert c[1] - c[0] > 2 ** 31 and c[2] - c[0] > 2 ** 32    # + c; the IM row of a pair, channels * stride on


@pytest.mark.parametrize("side", fl.SIDES)
@pytest.mark.parametrize("name", list(fl.LAYOUTS))
def test_frame_strided_sides_reach_the_same_bands(name, side):
    """g = r F + f over FRAME_ROWS x FRAMES_PER_ROW frames at the layout's stride: no fewer bands than the sequence side"""
    lay = fl.LAYOUTS[name]
    frames = fl.bands(lay, side, 4098, count=fl.FRAME_ROWS * fl.FRAMES_PER_ROW)
    seqs = fl.bands(lay, side, LENGTH)
    assert len(frames) == 6 and frames[:len(seqs)] == seqs
    if name == "wide":
        assert sum(b > 2 ** 33 for b in frames) == 4 and frames[-1] // 2 > 2 ** 33
    else:
        assert frames[4] > 2 ** 33 and 2 ** 32 < frames[3] < 2 ** 33


def test_arenas_fit_the_memory_budget():
    """the largest pair of arenas one test holds, a frame-strided side and a sequence-strided one, stays below 36 GiB"""
    for lay in fl.LAYOUTS.values():
        six = fl.FRAME_ROWS * fl.FRAMES_PER_ROW
        for frames, seqs in (("in", "out"), ("out", "in")):
            assert 2 * (fl.arena_halves(lay, frames, six) + fl.arena_halves(lay, seqs, fl.FRAME_ROWS)) <= 36 << 30, lay.name
        for side in fl.SIDES:
            b = fl.Block(fl.ROOM - LENGTH, lay.rows * lay.channels, fl.stride_of(lay, side), LENGTH)
            assert b.extent == fl.arena_halves(lay, side)


def _dense(blocks, datas, size):
    """the restatement: one flat array and one mask, by fancy indexing"""
    flat = np.full(size, fl.SENTINEL, np.int16)
    mask = np.ones(size, bool)
    for b, d in zip(blocks, datas):
        idx = b.base + (np.arange(b.count) * b.stride)[:, None] + np.arange(b.length)[None, :]
        flat[idx] = d.view(np.int16)
        mask[idx.reshape(-1)] = False
    return flat, mask


def _small(name, side):
    lay = fl.shrunken(fl.LAYOUTS[name], LENGTH)
    count, stride = lay.rows * lay.channels, fl.stride_of(lay, side)
    rng = np.random.default_rng(7)
    # two tensors at small distinct bases with equal strides, as the inputs and gates of one execution: the second in the first's gaps
    blocks = [fl.Block(16, count, stride, LENGTH - 8), fl.Block(16 + LENGTH - 8, count, stride, 8)]
    datas = [rng.standard_normal((b.count, b.length)).astype(np.float16) for b in blocks]
    size = max(b.extent for b in blocks) + 40
    return lay, blocks, datas, size


@pytest.mark.parametrize("side", fl.SIDES)
@pytest.mark.parametrize("name", list(fl.LAYOUTS))
def test_scatter_gather_and_gaps_against_a_dense_restatement(name, side, monkeypatch):
    monkeypatch.setattr(fl, "CHUNK", 1000)                    # several chunks per gap, a ragged last one
    lay, blocks, datas, size = _small(name, side)
    arena = fl.Arena(np.zeros(size, np.int16))
    assert (arena.buf == fl.SENTINEL).all()
    for b, d in zip(blocks, datas):
        arena.scatter(b, d)
    flat, mask = _dense(blocks, datas, size)
    assert np.array_equal(arena.buf, flat)
    got_mask = np.zeros(size, bool)
    for lo, hi in fl.gaps(arena.blocks, size):
        assert lo < hi and not got_mask[lo:hi].any()
        got_mask[lo:hi] = True
    assert np.array_equal(got_mask, mask)
    arena.check_gaps()
    for b, d in zip(blocks, datas):
        assert np.array_equal(arena.gather(b), d.view(np.int16))
        arena.check_block(b, d)
        assert np.array_equal(fl.to_bcl(arena.gather(b), lay.rows, lay.channels), d.reshape(lay.rows, lay.channels, -1))
        v = arena.view(b)
        assert v.shape[0] == (b.count - 1) * b.stride + b.length and v[0] == d.view(np.int16)[0, 0]
    # every single half of the gaps is seen, the first and the last of the arena included
    for at in np.nonzero(mask)[0][[0, 1, -1]].tolist() + [int(np.nonzero(mask)[0][len(np.nonzero(mask)[0]) // 2])]:
        arena.buf[at] = 0
        with pytest.raises(AssertionError, match=f"first at half {at} "):
            arena.check_gaps()
        arena.buf[at] = fl.SENTINEL
    arena.check_gaps()
    arena.fill()
    assert (arena.buf == fl.SENTINEL).all() and arena.blocks == []


@pytest.mark.parametrize("name", list(fl.LAYOUTS))
def test_a_truncated_offset_is_caught(name):
    """A kernel with `row * stride` in too few bits, restated at the shrunken stride: the product modulo 2^13 (the shrunken
    strides lie between 2^12 and 2^13, as the far ones between 2^30 and 2^32). A store through it lands in a gap or in another
    run: the gap check or the comparison of the gathered runs fails. A load through it reads the sentinel or another run's data."""
    lay, blocks, datas, size = _small(name, "out")
    b, d = blocks[0], datas[0]
    wrong = [b.base + (q * b.stride) % (1 << 13) for q in range(b.count)]
    assert wrong != b.starts() and all(w + b.length <= size for w in wrong)
    # the store
    arena = fl.Arena(np.zeros(size, np.int16))
    arena.place(b)
    for q, s in enumerate(wrong):
        arena.buf[s:s + b.length] = d.view(np.int16)[q]
    caught = 0
    try:
        arena.check_gaps()
    except AssertionError:
        caught += 1
    try:
        arena.check_block(b, d)
    except AssertionError:
        caught += 1
    assert caught >= 1
    assert not np.array_equal(arena.gather(b), d.view(np.int16))
    # the load: what the kernel would have read differs from what was placed, and holds NaNs wherever it touched a gap
    arena = fl.Arena(np.zeros(size, np.int16))
    arena.scatter(b, d)
    read = np.stack([arena.buf[s:s + b.length] for s in wrong])
    assert not np.array_equal(read, d.view(np.int16))


def test_blocks_may_not_overlap_or_leave_the_arena():
    arena = fl.Arena(np.zeros(10000, np.int16))
    arena.place(fl.Block(0, 2, 4112, 4104))
    with pytest.raises(AssertionError, match="overlap"):
        arena.place(fl.Block(4100, 1, 0, 8))
    with pytest.raises(AssertionError):
        fl.Arena(np.zeros(100, np.int16)).place(fl.Block(96, 1, 0, 8))
