"""The distributed transform (tfft_dist_*) checked bin by bin and phase by phase against fp64, all ranks in one process.

tests/dist_emulate.py runs every rank of a case between guard zones. Per case and rank:
  1. guard zones of input, send, receive and output planes come back bit for bit, the input is untouched, no half of the send
     planes (after pre) or of the output (after post) is left unwritten;
  2. the send buffer after tfft_dist_exec_pre against dist_emulate.send_reference, column by column (eb.K_PRE): the row
     transforms dilute a fault of the column pass (a wrong four-step twiddle of one rank's column block) below binary16 rounding
     noise, so only this check can see one (tests/test_dist_check_host.py shows it);
  3. the output after tfft_dist_exec_post against the fp64 spectrum, every row transform on its own for the rel-L2 bounds, every
     element in ulps of the largest bin of the whole N-point spectrum (eb.K_DIST, or eb.K_SINCOS by arithmetic class), and the
     rel-L2 of the rank's whole share as the older tests assert it;
  4. with column slabs: the output bit-equal to one slab, and check 2 on the [q][s][k][c_s] layout;
  5. every rank launches the same kernels, and a plan that reads the received segments in place starts its row transforms
     with a kernel that can.
Input: seeded uniform(-1, 1) binary16; the cases of one length share one signal and its fp64 spectrum (the host FFT is the
expensive part). From 2^28 on the full spectrum does not fit the host in fp64: the output is checked on each rank's first and
last row and two seeded ones against dist_emulate.spectrum_rows, in ulps of the largest bin of the sampled rows (at most the
largest of the whole spectrum, so the unit is never larger than the rule's); the send buffer is still checked in full.
tools/accuracy_dist.py runs the same cases over three seeds and writes profiles/dist_ulps.txt, where eb.K_PRE and eb.K_DIST come from."""
import ctypes

import numpy as np
import pytest

import dist_emulate as de
import elementwise_bound as eb

pytestmark = pytest.mark.gpu

REL_L2 = 1.5e-3
FULL_SPECTRUM_MAX_LG = 27

# (log2 N, world, slabs)
CASES = [
    (15, 2, 1),                 # smallest geometry: C = 64, autosort rows, re-order
    (16, 4, 1),                 # C = 64, k256 rows, re-order
    (20, 2, 1), (20, 16, 1),    # k4096 rows, re-order; 16 ranks, K = 16
    (21, 4, 1),                 # N1 = 512 column pass with col0 != 0, re-order
    (24, 8, 1),                 # N1 = 512, k4096r:8 rows
    (25, 2, 1), (25, 16, 1),    # segments, N2 = 2^17 (final radix-256 pass)
    (25, 1, 2),                 # slabs without an exchange: receive = send, segments of C / S inside one rank
    (26, 1, 1), (26, 2, 1), (26, 8, 1), (26, 16, 1),    # BASELINE configs[4b]; one rank = no exchange; 16 = the default-variant corner
    (26, 8, 2), (26, 8, 4),     # the slab layout of the send buffer, checked directly
    (27, 4, 1),                 # segments, radix-1024 final pass
    (28, 4, 1),                 # re-order in front of col:1024; sampled rows
    (29, 8, 1),                 # four local passes; sampled rows
]

# the column kernels that read segmented input rows (colfft::Args::in_seg_shift / in_seg_gap)
SEGMENT_READERS = ("colfft::colfft256_wg_kernel<", "colfft::colfft512_wg_kernel<", "colfft::colfft512r_wg_kernel<", "colfft::collat256_kernel<")
# Coverage statement (test_which_kernels_read_segments): the first row-pass kernels over every geometry that reads segments in
# place, log2 N = 14 .. 30, 1 .. 16 ranks, and column slabs where the plan takes them. FINDING: only the single-round radix-512
# cooperative kernel is ever reached, with non-temporal or plain accesses by the footprint of the rank's share. The segmented
# reads of colfft256_wg_kernel (colfft.hpp), colfft512r_wg_kernel (colfft512r.hpp, two places) and collat256_kernel (collat.hpp)
# are reached by no geometry: segments are read in place only at log2 N = 25, 26, 27, 29, 30, where N2 >= 2^17 and the row plan
# starts with col:512+tw, and the segmented sub-plan takes no planner variant (not 2^26 over 16 ranks either, where a caller's
# plan of N2 x K would flip the radix-512 kernel). No test can run that code through the public entry points; whether it stays
# is a later decision.
SEGMENTED_FIRST_KERNELS = {"colfft::colfft512_wg_kernel<0, 1, false, false>", "colfft::colfft512_wg_kernel<0, 1, false, true>"}


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd as t

    t.device_check(0)
    return t


def make_signal(lg, seed):
    """(xr, xi, exact): the signal of length 2^lg for `seed` and, up to 2^27, its fp64 spectrum DFT(x) / N"""
    n = 1 << lg
    rng = np.random.default_rng([seed, lg, 4711])
    xr = rng.uniform(-1, 1, n).astype(np.float16)
    xi = rng.uniform(-1, 1, n).astype(np.float16)
    exact = None
    if lg <= FULL_SPECTRUM_MAX_LG:
        exact = np.fft.fft(xr.astype(np.float64) + 1j * xi.astype(np.float64))
        exact /= n
    return xr, xi, exact


@pytest.fixture(scope="module")
def signals():
    """the signal of the latest length asked for: the cases are ordered by length, one length is held at a time"""
    held = {}

    def get(lg, seed=1):
        if (lg, seed) not in held:
            held.clear()
            held[(lg, seed)] = make_signal(lg, seed)
        return held[(lg, seed)]

    return get


def sampled_rows(g, rank, seed):
    rng = np.random.default_rng([seed, g.n, g.world, rank])
    return sorted({0, g.rows - 1, *(int(v) for v in rng.integers(1, g.rows - 1, 2))})


def run_case(torch, capi, lg, world, slabs, signal, seed=1, k_pre=None, k_out=None):
    """Runs one case with every assertion of this module; returns [(rank, send ulps, output ulps, rel-L2, arithmetic K)] and
    the kernels of the two phases. k_pre / k_out replace the committed constants (tools/accuracy_dist.py measures with the
    ceiling 4)."""
    xr, xi, exact = signal
    what = f"2^{lg} over {world} ranks, {slabs} slab(s), seed {seed}"
    res = de.run(torch, capi, xr, xi, world, slabs)
    g = res[0].g
    faults = [f for r in res for f in r.faults]
    assert not faults, f"{what}: {faults}"
    # 5. the same kernels on every rank; segments are read by a kernel that can
    for r in res:
        assert (r.kernels_pre, r.kernels_post) == (res[0].kernels_pre, res[0].kernels_post), f"{what}: rank {r.g.rank} launches other kernels"
    pre, post = res[0].kernels_pre, res[0].kernels_post
    assert len(pre) == slabs and (post[0] == "permute::permute_twiddle_kernel") == bool(g.reorder), (pre, post)
    if not g.reorder and (world > 1 or slabs > 1):
        assert post[0].startswith(SEGMENT_READERS), post
    k = de.k_of(pre + post) if k_out is None else k_out
    rows_of, want_of = {}, {}
    if exact is None:
        for r in res:
            rows_of[r.g.rank] = sampled_rows(g, r.g.rank, seed)
        k1s = [r * g.rows + k_ for r in range(world) for k_ in rows_of[r]]
        ref = de.spectrum_rows((xr, xi), g, k1s)
        peak, at = float(np.abs(ref).max()), 0
        for r in range(world):
            want_of[r] = ref[at:at + len(rows_of[r])]
            at += len(rows_of[r])
    else:
        peak = float(np.abs(exact).max())
    out = []
    for r in res:
        rank = r.g.rank
        # 2. the send buffer, column by column
        w_send = de.check_send(r.send_re, r.send_im, de.send_reference((xr, xi), g, rank), g, eb.K_PRE if k_pre is None else k_pre,
                               f"{what}, rank {rank}")
        # 3. the output, row by row, in ulps of the whole spectrum's largest bin
        want = want_of[rank] if exact is None else de.rank_rows(exact, g, rank)
        w_out, rel = de.check_output(r.out_re, r.out_im, want, peak, k, f"{what}, rank {rank}", rows=rows_of.get(rank))
        assert rel < REL_L2, f"{what}, rank {rank}: rel-L2 of the rank's share {rel:.3e}"
        print(f"{what}, rank {rank}: send {w_send:.3f} ulp, output {w_out:.3f} ulp, rel-L2 {rel:.2e}", flush=True)
        out.append((rank, w_send, w_out, rel, k))
        r.send_re = r.send_im = None
    if slabs > 1:
        # 4. the same bits as one slab
        base = de.run(torch, capi, xr, xi, world, 1, keep_send=False)
        for r, b in zip(res, base):
            assert np.array_equal(r.out_re.view(np.int16), b.out_re.view(np.int16)) and np.array_equal(r.out_im.view(np.int16), b.out_im.view(np.int16)), \
                f"{what}, rank {r.g.rank}: output differs from one slab"
    return out, (pre, post)


@pytest.mark.parametrize("lg,world,slabs", CASES, ids=lambda v: str(v))
def test_case_phase_by_phase(tf, signals, lg, world, slabs):
    import torch
    from tensor_fft_amd import capi

    run_case(torch, capi, lg, world, slabs, signals(lg))


def test_which_kernels_read_segments(tf):
    """Every geometry tfft_dist_geometry_query accepts, log2 N = 14 .. 30, 1 .. 16 ranks, first and last rank: the plan is created
    (caller's buffers, none handed in: only the re-order and row scratch is allocated), its geometry is the query's, and the
    kernels of its post phase agree with `reorder`. The first row-pass kernels of the plans that read segments are the literal set
    SEGMENTED_FIRST_KERNELS."""
    from tensor_fft_amd import capi

    lib = capi.load_library()
    firsts, seen = set(), 0
    for lg in range(14, 31):
        for world in (1, 2, 4, 8, 16):
            for rank in sorted({0, world - 1}):
                q = capi.DistGeometry()
                q.struct_size = ctypes.sizeof(q)
                if lib.tfft_dist_geometry_query(1 << lg, world, rank, ctypes.byref(q)) != 0:
                    continue
                q = de.geometry(q)
                one_slab_first = None
                for slabs in (1, 2, 4):
                    # column slabs: N1 = 256, whole 128-column blocks, and row transforms that read the slabs' segments in place
                    # (several ranks: no re-order pass; one rank has none in any case: its row plan must start with such a kernel)
                    takes = slabs == 1 or (q.n1 == 256 and not q.reorder and (q.cols // slabs) % 128 == 0
                                           and one_slab_first.startswith(SEGMENT_READERS))
                    if not takes:
                        with pytest.raises(capi.TfftError, match="TFFT_DIST_SLABS") as e:
                            capi.DistPlan(1 << lg, world, rank, 0, slabs=slabs, caller_buffers=True)
                        assert e.value.code == 5
                        continue
                    p = capi.DistPlan(1 << lg, world, rank, 0, slabs=slabs, caller_buffers=True)
                    g, pre, post = de.geometry(p.geometry), p.kernels(0), p.kernels(1)
                    p.close()
                    seen += 1
                    q.slabs = slabs
                    assert vars(g) == vars(q), (lg, world, rank, slabs)
                    assert len(pre) == slabs and len(set(pre)) == 1, pre
                    assert (post[0] == "permute::permute_twiddle_kernel") == bool(g.reorder), (lg, world, post)
                    assert "permute::permute_twiddle_kernel" not in post[1:], post
                    if slabs == 1:
                        one_slab_first = post[0]
                    if not g.reorder and (world > 1 or slabs > 1):
                        assert post[0].startswith(SEGMENT_READERS), (lg, world, post)
                        firsts.add(post[0])
    assert seen > 100, seen
    assert firsts == SEGMENTED_FIRST_KERNELS, sorted(firsts)
