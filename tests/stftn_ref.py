"""numpy restatement of the framing of the short-frame STFT plans (include/tfft_stftn.h, frame lengths 512, 1024 and 2048): the
geometry, the binary16 products of every frame in the flat order g = r * F + f, the launch shape, and the cases of
tests/test_gpu_stftn.py. No library, no GPU."""
import numpy as np

LENGTHS = (512, 1024, 2048)


def bins(n):
    return n // 2 + 1


def pitch(n):
    """tfft_rplan_spectrum_pitch(n): 264, 520, 1032"""
    return (bins(n) + 7) // 8 * 8


def per_group(n):
    """frames a wave takes per iteration: 16 / R transforms of two frames each, R = n / 256"""
    return 2 * (16 // (n // 256))


def geometry(n, length, hop, pad=0):
    """F, the frames per signal"""
    assert n in LENGTHS and length % 8 == 0 and length >= 8 and hop % 8 == 0 and hop >= 8 and pad % 8 == 0 and 0 <= pad < n and length + 2 * pad >= n
    return 1 + (length + 2 * pad - n) // hop


def conv_shape(items, cus, launch_iters):
    """conv_shape of tensor-fft_amd/conv/host_plumbing.hpp: (live waves per workgroup, workgroups) for `items` work items"""
    live = 8
    for l in (1, 2, 4):
        if items <= cus * l:
            live = l
            break
    blocks = (items + live - 1) // live
    if launch_iters >= 65535:
        return live, min(blocks, cus)
    if launch_iters:
        return live, (blocks + launch_iters - 1) // launch_iters
    iters = 2 if blocks >= 4 * cus else 1
    return live, max(min(blocks, cus), (blocks + iters - 1) // iters)


def groups_per_wave(items, cus, launch_iters):
    """how many work items each live wave of the launch takes: wave w of workgroup b starts at b * live + w and strides by grid * live"""
    live, grid = conv_shape(items, cus, launch_iters)
    return [len(range(b * live + w, items, grid * live)) for b in range(grid) for w in range(live)]


LOOP_GROUPS, LOOP_ITERS = 6, 3


def looping_case(n, cus=256):
    """(rows, length, hop, pad) of the case in which, at launch_iters = 3, EVERY live wave takes three groups, the total is odd and
    the last group ragged. Six groups on `cus` >= 6 compute units are one live wave per workgroup and ceil(6 / 3) = 2 workgroups:
    wave 0 takes groups 0, 2, 4 and wave 1 groups 1, 3, 5. Six groups whose last lacks one transform are 6 * (16 / R) - 1
    transforms, and with the last one self-paired 12 * (16 / R) - 3 frames: 93, 45 and 21 at n = 512, 1024, 2048, each 3 signals of
    31, 15 and 7 frames. pad = n / 2 and hop = n / 8: F = 1 + L / hop, so L = (F - 1) * n / 8."""
    assert conv_shape(LOOP_GROUPS, cus, LOOP_ITERS) == (1, 2) and groups_per_wave(LOOP_GROUPS, cus, LOOP_ITERS) == [3, 3]
    total = LOOP_GROUPS * per_group(n) - 3
    rows, hop, pad = 3, n // 8, n // 2
    assert total % rows == 0 and total % 2 == 1
    length = (total // rows - 1) * hop
    assert rows * geometry(n, length, hop, pad) == total
    # odd, and the last of the six groups holds fewer transforms than a full one
    transforms = (total + 1) // 2
    assert -(-transforms // (per_group(n) // 2)) == LOOP_GROUPS and transforms % (per_group(n) // 2)
    return rows, length, hop, pad


def cases(n):
    """(rows, length, hop, pad, launch_iters): the smallest shapes at which each index of the kernel can go wrong"""
    return [
        (1, n, 8, 0, 0),                         # one self-paired frame in a ragged group
        (1, n + 8, 8, 0, 0),                     # two frames one chunk apart
        (3, 3 * n // 2, n // 4, 0, 0),           # 9 frames: pairs straddle signals, the last self-paired, a ragged last group at n = 2048
        (1, 2 * n, n // 2, n // 2, 0),           # F = 5, zeros at both ends
        (1, 8, 8, n // 2, 0),                    # both ends zero inside each of two frames
        (1, n, n // 2, n - 8, 0),                # the first frame holds 8 real samples
        (2, 3 * n, 2 * n, 0, 0),                 # hop beyond a frame
        looping_case(n) + (LOOP_ITERS,),         # every live wave takes three groups; odd total, ragged last group
    ]


RANDOM_WINDOW_CASES = (2, 3, 5)                  # indices into cases(n) that run again with a uniform(0, 1) window


def accuracy_shapes(n):
    """pad-0 shapes where every frame is full"""
    return [(3, n + 2 * (n // 4), n // 4, 0), (4, n + 7 * (n // 4), n // 4, 0)]


def geometry_table(n):
    """(length, hop, pad) -> frames: every GPU case, and the ends of the range"""
    rows = {(length, hop, pad): None for _, length, hop, pad, _ in cases(n)}
    rows.update({(length, hop, pad): None for _, length, hop, pad in accuracy_shapes(n)})
    table = [(length, hop, pad, geometry(n, length, hop, pad)) for length, hop, pad in rows]
    table += [(1 << 26, n // 4, 0, 1 + ((1 << 26) - n) // (n // 4)), (n, 1 << 40, 0, 1),
              (1 << 26, 8, n - 8, 1 + ((1 << 26) + 2 * (n - 8) - n) // 8)]
    return table


def windows(n, x, hop, pad=0):
    """x [R, L] of any dtype -> the frames [R * F, n] in the order g, zeros outside [0, L), same dtype"""
    x = np.asarray(x)
    rows, length = x.shape
    f = geometry(n, length, hop, pad)
    tail = max(0, (f - 1) * hop + n - pad - length)
    padded = np.concatenate([np.zeros((rows, pad), x.dtype), x, np.zeros((rows, tail), x.dtype)], axis=1)
    idx = (np.arange(f) * hop)[:, None] + np.arange(n)[None, :]
    return padded[:, idx].reshape(rows * f, n)


def frames(x, w, hop, pad=0):
    """x [R, L] float16, w [n] float16 -> u [R * F, n] float16: u = fp16(w * x), one rounding to nearest even, subnormals kept (a
    product of two binary16 values is exact in float32), in the order g; zeros outside the signal"""
    x, w = np.asarray(x), np.asarray(w)
    n = w.shape[0]
    assert x.dtype == np.float16 and w.dtype == np.float16 and w.shape == (n,)
    return (windows(n, x, hop, pad).astype(np.float32) * w.astype(np.float32)[None, :]).astype(np.float16)


def hann(n):
    """the periodic Hann window of n samples (torch.hann_window), rounded to binary16"""
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float16)


def case_data(n, rows, length, seed=1, window="hann"):
    """uniform(-1, 1) binary16 signals [R, L] and the window: "hann" or "random" (uniform(0, 1), no symmetry to hide an index error)"""
    rng = np.random.default_rng([n, rows, length, seed])
    x = rng.uniform(-1, 1, (rows, length)).astype(np.float16)
    w = hann(n) if window == "hann" else rng.uniform(0, 1, n).astype(np.float16)
    return x, w


def rel_l2(got, want):
    """per row: |got - want|_2 / |want|_2 over complex rows"""
    return np.sqrt((np.abs(got - want) ** 2).sum(-1) / (np.abs(want) ** 2).sum(-1))
