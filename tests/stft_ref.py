"""numpy restatement of the framing of the STFT plans (include/tfft_stft.h): the geometry, the binary16 products of every frame in
the flat order g = r * F + f, and the cases of tests/test_gpu_stft.py. No library, no GPU."""
import numpy as np

N = 4096
BINS = N // 2 + 1
PITCH = 2056

# (rows, length, hop, pad, launch_iters): the smallest shapes at which each index of the kernel can go wrong
CASES = [
    (1, 4096, 8, 0, 0),            # one frame, paired with itself
    (1, 4104, 8, 0, 0),            # two frames one chunk apart
    (3, 6144, 1024, 0, 0),         # 9 frames: pairs straddle signals, the last one is paired with itself
    (2, 8192, 2048, 2048, 0),      # zeros at both ends, F = 5 odd
    (2, 4096, 512, 4088, 0),       # frame 0 holds 8 real samples
    (1, 8, 8, 2048, 0),            # both ends zero inside one frame
    (1, 12288, 8192, 0, 0),        # hop beyond a frame
    (4, 4416, 8, 0, 3),            # 164 frames, every wave takes three items
    (5, 8192, 2048, 2048, 3),      # padding and looping together
]

# (length, hop, pad) -> frames
GEOMETRY = [
    (8, 8, 2048, 2), (4096, 8, 0, 1), (4104, 8, 0, 2), (8192, 2048, 2048, 5), (4096, 512, 4088, 16), (12288, 8192, 0, 2),
    (1 << 26, 1024, 0, 1 + ((1 << 26) - 4096) // 1024), (6144, 1024, 0, 3), (4416, 8, 0, 41), (4096, 1 << 40, 0, 1),
    (1 << 26, 8, 4088, 1 + ((1 << 26) + 8176 - 4096) // 8),
]


def geometry(length, hop, pad=0):
    """F, the frames per signal"""
    assert length % 8 == 0 and length >= 8 and hop % 8 == 0 and hop >= 8 and pad % 8 == 0 and 0 <= pad < N and length + 2 * pad >= N
    return 1 + (length + 2 * pad - N) // hop


def windows(x, hop, pad=0):
    """x [R, L] of any dtype -> the frames [R * F, 4096] in the order g, zeros outside [0, L), same dtype"""
    x = np.asarray(x)
    rows, length = x.shape
    f = geometry(length, hop, pad)
    tail = max(0, (f - 1) * hop + N - pad - length)
    padded = np.concatenate([np.zeros((rows, pad), x.dtype), x, np.zeros((rows, tail), x.dtype)], axis=1)
    idx = (np.arange(f) * hop)[:, None] + np.arange(N)[None, :]
    return padded[:, idx].reshape(rows * f, N)


def frames(x, w, hop, pad=0):
    """x [R, L] float16, w [4096] float16 -> u [R * F, 4096] float16: u = fp16(w * x), one rounding to nearest even, subnormals
    kept (a product of two binary16 values is exact in float32), in the order g; zeros outside the signal"""
    x, w = np.asarray(x), np.asarray(w)
    assert x.dtype == np.float16 and w.dtype == np.float16 and w.shape == (N,)
    return (windows(x, hop, pad).astype(np.float32) * w.astype(np.float32)[None, :]).astype(np.float16)


def hann():
    """the periodic Hann window of 4096 samples (torch.hann_window), rounded to binary16"""
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)).astype(np.float16)


def case_data(rows, length, seed=1, window="hann"):
    """uniform(-1, 1) binary16 signals [R, L] and the window: "hann" or "random" (uniform(0, 1), no symmetry to hide an index error)"""
    rng = np.random.default_rng([rows, length, seed])
    x = rng.uniform(-1, 1, (rows, length)).astype(np.float16)
    w = hann() if window == "hann" else rng.uniform(0, 1, N).astype(np.float16)
    return x, w


def rel_l2(got, want):
    """per row: |got - want|_2 / |want|_2 over complex rows"""
    return np.sqrt((np.abs(got - want) ** 2).sum(-1) / (np.abs(want) ** 2).sum(-1))
