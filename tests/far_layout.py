"""Far layouts: sequences of one execution placed beyond 2, 4 and 8 GiB of one device allocation.

Every public header promises 64-bit strides; a kernel keeps that promise only where `row * stride` is formed in 64 bits, and a
binding only where the stride travels as a 64-bit integer. A stride of L + 8 cannot tell. The two layouts here can:

  layout     shape                  input stride   output stride   sequences start near
  wide       3 rows x 1 channel     2^31 + 8       2^31 + 24       0, 4 GiB, 8 GiB
  channels   2 rows x 2 channels    2^30 + 8       2^30 + 24       0, 2, 4, 6 GiB

(strides in halves). `wide` has one full RE/IM pair and a zero partner whose base lies beyond 2^33 bytes; in `channels` the `+ c`
term and the `channels * stride` distance of a pair's IM row each cross a 2^32-byte line. A frame-strided side (STFT output, ISTFT
input) takes FRAME_ROWS rows of FRAMES_PER_ROW frames, so that the frame index g = r F + f reaches the same bands.

An Arena is one flat int16 buffer filled with the suite's NaN sentinel (dist_emulate.SENTINEL). Blocks, small host arrays, are
scattered into it at base + q * stride; gather reads them back; check_gaps asserts that every half outside the blocks still holds
the sentinel, in chunks of at most CHUNK halves, so that no large temporary appears. The buffer is a torch tensor on the device in
the GPU tests and a numpy array in the host tests (tests/test_far_layout_host.py runs this very code at a shrunken stride against a
dense restatement): nothing here needs a GPU, or torch, at import.

Tensors that a plan's overlap rule lets share memory (the inputs, gates and contexts of one execution, the RE and IM planes of a
spectrum) live in ONE arena at small distinct base offsets with equal strides, where seqs_overlap of conv/host_math.hpp is exact;
outputs have an arena of their own with the output stride."""
import collections

import numpy as np

import dist_emulate as de

SENTINEL = de.SENTINEL
CHUNK = 1 << 28                      # halves per step of a fill or a scan (512 MiB)
ROOM = 1 << 20                       # halves of base offsets an arena has room for beyond (count - 1) * stride
FRAME_ROWS, FRAMES_PER_ROW = 3, 2    # the smallest frame-strided side whose g = r F + f reaches the bands of both layouts' counts

Layout = collections.namedtuple("Layout", "name rows channels in_stride out_stride")
LAYOUTS = {
    "wide": Layout("wide", 3, 1, (1 << 31) + 8, (1 << 31) + 24),
    "channels": Layout("channels", 2, 2, (1 << 30) + 8, (1 << 30) + 24),
}
SIDES = ("in", "out")


def stride_of(layout, side):
    return layout.in_stride if side == "in" else layout.out_stride


def shrunken(layout, length):
    """the same layout at the strides the other tests use: the helper's code is the same, only the numbers are small"""
    return layout._replace(in_stride=length + 8, out_stride=length + 24)


class Block(collections.namedtuple("Block", "base count stride length")):
    """`count` runs of `length` halves, run q at base + q * stride (all in halves, exact Python integers)"""

    def starts(self):
        return [self.base + q * self.stride for q in range(self.count)]

    @property
    def extent(self):
        """halves from the arena's start to the end of the last run"""
        return self.base + self.span

    @property
    def span(self):
        """what a plan asks of the tensor it is handed: (count - 1) * stride + length"""
        return (self.count - 1) * self.stride + self.length


def arena_halves(layout, side, count=None):
    """halves of an arena that holds `count` (default: the layout's rows * channels) runs and ROOM halves of base offsets"""
    count = layout.rows * layout.channels if count is None else count
    return (count - 1) * stride_of(layout, side) + ROOM


def gaps(blocks, size):
    """the intervals [lo, hi) of [0, size) that no block covers, in order"""
    runs = sorted((s, s + b.length) for b in blocks for s in b.starts())
    out, at = [], 0
    for lo, hi in runs:
        assert lo >= at, f"blocks overlap at half {lo}"
        if lo > at:
            out.append((at, lo))
        at = hi
    assert at <= size, f"a block ends at half {at}, beyond the arena's {size}"
    if at < size:
        out.append((at, size))
    return out


class Arena:
    """One flat int16 buffer (a torch tensor on any device, or a numpy array) of sentinel halves with blocks scattered into it."""

    def __init__(self, buf):
        assert len(buf.shape) == 1 and "int16" in str(buf.dtype)
        self.buf = buf
        self.size = int(buf.shape[0])
        self.is_numpy = isinstance(buf, np.ndarray)
        self.blocks = []
        self.fill()

    def fill(self):
        """every half back to the sentinel, no block placed"""
        for lo in range(0, self.size, CHUNK):
            self.buf[lo:lo + CHUNK] = np.int16(SENTINEL) if self.is_numpy else SENTINEL
        self.blocks = []

    def _to_buf(self, host):
        if self.is_numpy:
            return host
        import torch

        return torch.from_numpy(np.array(host)).to(self.buf.device)        # a copy: the host data may be read-only

    def _to_host(self, part):
        return np.array(part) if self.is_numpy else part.cpu().numpy()

    def place(self, block):
        """registers a block without writing it (an output: its halves may change, every other half may not)"""
        assert block.base >= 0 and block.extent <= self.size, (block, self.size)
        gaps(self.blocks + [block], self.size)       # asserts that no two blocks share a half
        self.blocks.append(block)
        return block

    def scatter(self, block, host):
        """host: [count][length] binary16 (or int16 bit patterns); run q lands at base + q * stride"""
        host = np.ascontiguousarray(host).reshape(block.count, block.length)
        bits = host.view(np.int16) if host.dtype != np.int16 else host
        self.place(block)
        for q, s in enumerate(block.starts()):
            self.buf[s:s + block.length] = self._to_buf(bits[q])
        return block

    def gather(self, block):
        """[count][length] int16 bit patterns of the block's runs"""
        return np.stack([self._to_host(self.buf[s:s + block.length]) for s in block.starts()])

    def view(self, block):
        """the flat slice a plan is handed for this block: span halves from base (int16; the caller views it as float16)"""
        return self.buf[block.base:block.base + block.span]

    def check_gaps(self, what="arena"):
        """asserts that every half outside the placed blocks holds the sentinel; one pass, CHUNK halves at a time"""
        bad, first = 0, None
        for lo, hi in gaps(self.blocks, self.size):
            for a in range(lo, hi, CHUNK):
                b = min(hi, a + CHUNK)
                n = int((self.buf[a:b] != (np.int16(SENTINEL) if self.is_numpy else SENTINEL)).sum())
                if n and first is None:
                    part = self._to_host(self.buf[a:b])
                    first = a + int(np.nonzero(part != np.int16(SENTINEL))[0][0])
                bad += n
        assert bad == 0, f"{what}: {bad} halves outside the written blocks changed, first at half {first} (byte {2 * first:#x})"

    def check_block(self, block, host, what="arena"):
        """asserts that the block's runs hold `host` bit for bit"""
        host = np.ascontiguousarray(host).reshape(block.count, block.length)
        bits = host.view(np.int16) if host.dtype != np.int16 else host
        got = self.gather(block)
        ne = np.argwhere(got != bits)
        assert ne.size == 0, f"{what}: {len(ne)} halves of a placed block changed, first (run, half) = {ne[0].tolist()}"


class Pool:
    """The device arenas of one test module: at most one per side, re-used (and refilled) while the size asked for stays the same,
    released and allocated anew when it changes, so that a module never holds more than one test needs. need() is what the next
    test would hold; a test skips only when the device has less than that plus HEADROOM free (tests/test_gpu_full_size.py)."""
    HEADROOM = 4 << 30

    def __init__(self, torch, device="cuda:0"):
        self.torch, self.device, self.arenas = torch, device, {}

    def held(self):
        return sum(2 * a.size for a in self.arenas.values())

    def missing(self, sizes):
        """bytes the arenas of `sizes` ({side: halves}) need beyond what the pool can re-use or release; the pool's own memory
        is in torch's cache or in use, so it counts as available"""
        need = sum(2 * h for h in sizes.values())
        self.torch.cuda.empty_cache()
        free, _ = self.torch.cuda.mem_get_info()
        return max(0, need + self.HEADROOM - (free + self.held()))

    def get(self, sizes):
        """{side: Arena} of exactly sizes[side] halves each, every half the sentinel"""
        for side in list(self.arenas):
            if sizes.get(side) != self.arenas[side].size:
                del self.arenas[side]
        if len(self.arenas) < len(sizes):
            self.torch.cuda.empty_cache()
        for side, halves in sizes.items():
            if side in self.arenas:
                self.arenas[side].fill()
            else:
                self.arenas[side] = Arena(self.torch.empty(halves, dtype=self.torch.int16, device=self.device))
        return {side: self.arenas[side] for side in sizes}

    def release(self):
        self.arenas.clear()
        self.torch.cuda.empty_cache()


def to_bcl(runs, rows, channels):
    """gathered runs [rows * channels][L] -> [B][C][L] binary16"""
    runs = np.asarray(runs)
    return runs.view(np.float16).reshape(rows, channels, runs.shape[-1])


def bands(layout, side, length=8, base=0, count=None):
    """byte offsets at which the layout's runs start on that side (exact integers)"""
    count = layout.rows * layout.channels if count is None else count
    return [2 * s for s in Block(base, count, stride_of(layout, side), length).starts()]
