"""Round 4 on the GPU: ABI versioning against real plans, the copy / compute ordering of the C++ shim, the top of the
reference's benchmark range (2^29; 2^30: VERDICT r3 item 5), the 2^20 -> 2^21 planner boundary, and bench.py's distributed entry
rehearsed with one rank under torch.distributed.run (VERDICT r3 item 1 iii)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import elementwise_bound as eb
from tensor_fft_amd import capi

K_ANY = max(eb.K_TABLE, eb.K_SINCOS)        # per-element bound of a plan that may take either twiddle source

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_L2_TOL = 1.5e-3


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd as t

    t.device_check(0)
    return t


def test_truncated_option_struct_gives_the_default_plan(tf, orc):
    """A caller compiled against an older header (48- or 64-byte tfft_plan_opts, garbage behind it) gets exactly the plan a
    current caller gets from zeroed options: same spectrum, bit for bit, and correct against the CPU oracle."""
    import torch
    from tensor_fft_amd import capi

    L = capi.load_library()
    n, batch = 1 << 16, 5
    x = torch.empty(batch * 2 * n, dtype=torch.float16, device="cuda")
    tf.synth_uniform(x, x[n:], n, batch, seed=4)
    outs = []
    for size in (72, 64, 48):
        blob = size.to_bytes(4, "little") + bytes(size - 4) + b"\xff" * (136 - size)
        buf = ctypes.create_string_buffer(blob, len(blob))
        h = ctypes.c_void_p()
        assert L.tfft_plan_create(n, batch, 0, ctypes.cast(buf, ctypes.POINTER(capi.PlanOpts)), ctypes.byref(h)) == 0, capi.last_error()
        y = torch.full_like(x, float("nan"))
        assert L.tfft_plan_num_launches(h) == 2
        assert L.tfft_exec(h, x.data_ptr(), x[n:].data_ptr(), y.data_ptr(), y[n:].data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        L.tfft_plan_destroy(h)
        outs.append(y)
    assert all(bool((o.view(torch.int16) == outs[0].view(torch.int16)).all()) for o in outs[1:])
    re, im = orc.synth_uniform(n, 1, batch - 1, 4)
    e_re, e_im = orc.dft64(re, im)
    o = outs[0][(batch - 1) * 2 * n:].cpu().numpy().astype(np.float64)
    got, exact = o[:n] + 1j * o[n:], e_re[0] + 1j * e_im[0]
    assert np.linalg.norm(got - exact) / np.linalg.norm(exact) <= REL_L2_TOL


def test_copy_after_async_compute_does_not_overwrite_the_running_input(tf):
    """examples/copy_order_check.cpp over include/tensor_fft.hpp: 2000 queued ComputeFFT calls, then CopyDataHostToDevice with no
    synchronisation in between, for the plain hipMemcpy path and for the pinned ring (tfft_copy_h2d)."""
    exe = os.path.join(ROOT, "examples", "copy_order_check")
    r = subprocess.run(["timeout", "-k", "10", "300", exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert r.stdout.count("signal A (ordered)") == 2 and r.stdout.count("arrived") == 2


def _tone_and_bins(torch, tf, lg, bins_to_check=8):
    """One transform of length 2^lg: (a) a plane wave at an arbitrary bin lands in that bin alone, (b) a uniform(-1, 1) signal
    obeys Parseval and matches direct fp64 DFT sums at sampled bins (tests/accuracy_protocol.direct_bins)."""
    import math

    import accuracy_protocol as ap

    n = 1 << lg
    plan = tf.TfftPlan(n, 1, 0, preserve_input=True)
    f0 = 123456789 % n
    x = torch.empty(2 * n, dtype=torch.float16, device="cuda")
    step = 1 << 26
    for lo in range(0, n, step):                                     # (in blocks: fp64 temporaries of 2^26 elements)
        idx = torch.arange(lo, min(n, lo + step), device="cuda", dtype=torch.int64)
        ph = ((idx * f0) % n).double() * (2 * math.pi / n)
        x[lo:lo + idx.numel()] = torch.cos(ph).half()
        x[n + lo:n + lo + idx.numel()] = torch.sin(ph).half()
        del idx, ph
    y = torch.empty_like(x)
    plan.exec(x, x[n:], y, y[n:])
    torch.cuda.synchronize()
    peak_re, peak_im = float(y[f0]), float(y[n + f0])
    assert abs(peak_re - 1.0) < 4e-3 and abs(peak_im) < 4e-3, (lg, peak_re, peak_im)
    y[f0] = 0
    y[n + f0] = 0
    others = 0.0
    for lo in range(0, 2 * n, step):
        others = max(others, float(y[lo:lo + step].float().abs().max()))
    assert others < 2e-3, (lg, others)                               # fp16 rounding of the input spreads ~1e-4 per bin at most
    # white signal: Parseval + sampled bins
    tf.synth_uniform(x, x[n:], n, 1, seed=lg)
    plan.exec(x, x[n:], y, y[n:])
    torch.cuda.synchronize()
    e_in = e_out = 0.0
    for lo in range(0, 2 * n, step):
        e_in += float((x[lo:lo + step].double() ** 2).sum())
        e_out += float((y[lo:lo + step].double() ** 2).sum())
    assert abs(e_out - e_in / n) / (e_in / n) < 5e-3, (lg, e_out, e_in / n)
    rng = np.random.default_rng(lg)
    bins = [1, n - 1, n // 2 + 1] + [int(b) for b in rng.integers(0, n, bins_to_check - 3)]
    d_re, d_im = x[:n].double(), x[n:].double()
    want = ap.direct_bins(torch, d_re, d_im, bins)
    del d_re, d_im
    got = np.array([complex(float(y[k]), float(y[n + k])) for k in bins])
    rms = (e_in / n / n / 2) ** 0.5
    assert np.abs(got - want).max() < 8 * 2.0 ** -11 * max(rms, 2.0 ** -14), (lg, np.abs(got - want).max(), rms)
    return plan.num_launches


@pytest.mark.parametrize("lg", [29, 30])
def test_top_of_the_reference_bench_range(tf, lg):
    """The reference benches single transforms to 2^29 (FFTBenchSinlge.cu:11-12); the planner has hand-picked three-pass splits
    for 2^29 and 2^30 (tfft.hip kColSplit). 2^30: 4 GiB of planes + 4 GiB of output + 4 GiB of workspace."""
    import torch

    free, _ = torch.cuda.mem_get_info()
    if free < 5 * (1 << lg) * 4:
        pytest.skip("not enough free HBM")
    assert _tone_and_bins(torch, tf, lg) == 3
    torch.cuda.empty_cache()


@pytest.mark.parametrize("lg,passes", [(20, 2), (21, 3)])
def test_planner_boundary_between_two_and_three_passes(tf, orc, lg, passes):
    """2^20 is the last length with two passes in natural order, 2^21 the first with three: batch 512 of each against the oracle
    (first, middle and last transform), replicas bit-identical."""
    import torch

    n, batch = 1 << lg, 512
    assert tf.plan_describe(n).count(":") == passes
    x = torch.empty(batch * 2 * n, dtype=torch.float16, device="cuda")
    tf.synth_uniform(x, x[n:], n, batch, seed=lg)
    x[(batch - 2) * 2 * n:(batch - 1) * 2 * n] = x[: 2 * n]           # a replica of transform 0 near the end of the batch
    y = torch.empty_like(x)
    plan = tf.TfftPlan(n, batch, 0, preserve_input=True)
    assert plan.num_launches == passes
    plan.exec(x, x[n:], y, y[n:])
    torch.cuda.synchronize()
    assert bool((y[: 2 * n].view(torch.int16) == y[(batch - 2) * 2 * n:(batch - 1) * 2 * n].view(torch.int16)).all())
    for b in (0, batch // 2, batch - 1):
        re, im = orc.synth_uniform(n, 1, b, lg)
        e_re, e_im = orc.dft64(re, im)
        o = y[b * 2 * n:(b + 1) * 2 * n].cpu().numpy().astype(np.float64)
        got, exact = o[:n] + 1j * o[n:], e_re[0] + 1j * e_im[0]
        assert np.linalg.norm(got - exact) / np.linalg.norm(exact) <= REL_L2_TOL, (lg, b)


def test_bench_distributed_entry_rehearsal_with_one_rank():
    """bench.py's configs[4b] entry exactly as an 8-GPU run takes it, with one rank: under torch.distributed.run (so the torch
    process group has its own RCCL communicator), the library's communicator next to it, the own chunk through ncclSend / ncclRecv.
    A fresh child with a time limit; the ONE JSON line is parsed."""
    cmd = ["timeout", "-k", "10", "900", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
           "--master-addr", "127.0.0.1", "--master-port", "29517", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full", "--with-dist",
           "--dist-self-via-comm", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--only-dist-entry"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["value"] > 100 and d["roofline"]["kernel_ms_per_rank"]["all"] and d["runtime"]["backend"] == "nccl"
    e = d["other_configs"]["configs[4b]_n2^26_distributed"]
    assert "error" not in e, e
    assert e["transport"] == "rccl" and e["transport_fallback_taken"] is False
    assert e["communicator"] == {"ncclCommCount": 1, "ncclCommUserRank_of_rank0": 0}
    assert isinstance(e["rccl_version"], int) and e["rccl_version"] > 20000
    ph = e["phases"]
    assert all(ph[k]["max_over_ranks"] > 0 for k in ("pre_ms", "exchange_ms", "post_ms"))
    assert e["bytes_through_the_collective_per_rank"] == 2 * (1 << 26) * 2            # both planes of the own chunk
    assert "Parseval" in e["check"]


# ---- transposed-order INPUT (tfft_plan_opts.input_order): in[k1 N2 + k2] = x[k1 + N1 k2] -> natural-order X
def _transposed_layout(x, n1, n2):
    """natural-order samples -> the [N1][N2] matrix in[k1 N2 + k2] = x[k1 + N1 k2]"""
    return np.ascontiguousarray(x.reshape(n2, n1).T).reshape(-1)


@pytest.mark.parametrize("lg", list(range(16, 25)))
@pytest.mark.parametrize("scale", ["sequential", "none"])
def test_transposed_input_against_the_oracle(tf, orc, lg, scale):
    """Two passes (contiguous N2-point transforms with the four-step twiddle in their fp32 epilogue, one radix-N1 column pass)
    from the transposed layout to the natural-order spectrum, for every length that has the layout, against the fp64 oracle."""
    import torch

    n = 1 << lg
    n2 = tf.transposed_n2(n)
    n1 = n // n2
    batch = max(2, min(8, (1 << 22) // n))
    amp = 1.0 if scale == "sequential" else 40000.0 / n          # unscaled: keep N * max|x| inside binary16
    re, im = orc.synth_uniform(n, batch, 0, lg)
    re, im = (re * amp).astype(np.float16), (im * amp).astype(np.float16)
    host = np.empty((batch, 2, n), dtype=np.float16)
    for b in range(batch):
        host[b, 0] = _transposed_layout(re[b], n1, n2)
        host[b, 1] = _transposed_layout(im[b], n1, n2)
    x = torch.from_numpy(host.reshape(-1)).cuda()
    y = torch.full_like(x, float("nan"))
    plan = tf.TfftPlan(n, batch, 0, input_order="transposed", scale=scale, preserve_input=True)
    assert plan.num_launches == 2
    keep = x.clone()
    plan.exec(x, x[n:], y, y[n:])
    torch.cuda.synchronize()
    assert bool((x.view(torch.int16) == keep.view(torch.int16)).all())            # preserve_input
    e_re, e_im = orc.dft64(re, im)
    got = y.cpu().numpy().reshape(batch, 2, n).astype(np.float64)
    f = 1.0 if scale == "sequential" else float(n)
    for b in range(batch):
        g, ex = got[b, 0] + 1j * got[b, 1], (e_re[b] + 1j * e_im[b]) * f
        assert np.linalg.norm(g - ex) / np.linalg.norm(ex) <= REL_L2_TOL, (lg, scale, b)
        eb.check(g.real, g.imag, ex.real, ex.imag, K_ANY, what=f"2^{lg} {scale}, transform {b}")
    # in place too (the input is consumed completely by the first pass before the second writes)
    plan2 = tf.TfftPlan(n, batch, 0, input_order="transposed", scale=scale)
    plan2.exec(x, x[n:], x, x[n:])
    torch.cuda.synchronize()
    assert bool((x.view(torch.int16) == y.view(torch.int16)).all())


@pytest.mark.parametrize("lg", [16, 20, 21, 24])
def test_spectrum_multiply_and_back_in_two_plus_two_passes(tf, orc, lg):
    """What the transposed orders are for: forward (natural -> transposed spectrum, 2 passes), pointwise work on the spectrum in
    that layout, inverse from it (transposed input -> natural samples, 2 passes): a circular shift by one sample done in the
    frequency domain, checked against numpy's roll of the input."""
    import torch

    n = 1 << lg
    n2 = tf.transposed_n2(n)
    n1 = n // n2
    rng = np.random.default_rng(lg)
    xr, xi = rng.uniform(-1, 1, n).astype(np.float16), rng.uniform(-1, 1, n).astype(np.float16)
    x = torch.from_numpy(np.concatenate([xr, xi])).cuda()
    spec = torch.empty_like(x)
    # forward unscaled (white noise of rms 0.58: |X| ~ 0.8 sqrt(N) <= 3300, inside binary16), inverse with the 1/N: x comes back
    fwd = tf.TfftPlan(n, 1, 0, output_order="transposed", scale="none", preserve_input=True)       # X in the [N1][N2] layout
    inv = tf.TfftPlan(n, 1, 0, input_order="transposed", preserve_input=True)                      # (1/N) sum X e^{+...}
    assert fwd.num_launches == 2 and inv.num_launches == 2
    fwd.exec(x, x[n:], spec, spec[n:])
    # multiply bin k by exp(-2 pi i k / N) (a delay of one sample); bin k = k1 + N1 k2 sits at [k1][k2]
    k = (torch.arange(n1, device="cuda", dtype=torch.float64)[:, None] + n1 * torch.arange(n2, device="cuda", dtype=torch.float64)[None, :]).reshape(-1)
    ph = -2.0 * np.pi * k / n
    c, s = torch.cos(ph), torch.sin(ph)
    sr, si = spec[:n].double(), spec[n:].double()
    prod = torch.cat([(sr * c - si * s), (sr * s + si * c)]).half()
    back = torch.empty_like(x)
    inv.exec_inverse(prod, prod[n:], back, back[n:])
    torch.cuda.synchronize()
    got = back.cpu().numpy().astype(np.float64)
    want = np.concatenate([np.roll(xr.astype(np.float64), 1), np.roll(xi.astype(np.float64), 1)])
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert err < 3e-3, (lg, err)                                  # two transforms + one extra rounding of the product


def test_transposed_input_refusals(tf):
    with pytest.raises(tf.TfftError) as e:
        tf.TfftPlan(1 << 15, 4, 0, input_order="transposed")
    assert e.value.code == 5 and "no [N1][N2] layout" in e.value.message
    with pytest.raises(tf.TfftError) as e:
        tf.TfftPlan(1 << 20, 4, 0, input_order="transposed", output_order="transposed")
    assert "cannot both" in e.value.message
    with pytest.raises(tf.TfftError) as e:
        tf.TfftPlan(1 << 20, 4, 0, input_order="transposed", scale="once")
    assert "TFFT_SCALE_ONCE" in e.value.message
    with pytest.raises(tf.TfftError):
        tf.TfftPlan(1 << 20, 4, 0, input_order="transposed", variant=capi.VARIANT_AUTOSORT_ONLY)
    with pytest.raises(tf.TfftError):
        tf.TfftPlan(1 << 12, 4, 0, inner=64, input_order="transposed")


# ---- chunked execution (round 4): the transposed-order plans and the fused 2D plan run the batch chunk by chunk through one
# chunk-sized workspace; a batch that is not a whole number of chunks ends with a shorter chunk on sub-plans of its own
@pytest.mark.parametrize("order", ["transposed_out", "transposed_in"])
def test_chunked_transposed_plans_with_a_tail_chunk(tf, orc, order):
    import torch

    n = 1 << 16
    n2 = tf.transposed_n2(n)
    n1 = n // n2
    chunk = (1 << (26 if order == "transposed_out" else 27)) // n      # tfft.hip transposed_chunk: 256 / 512 MiB of intermediate
    batch = chunk + 3
    x = torch.empty(batch * 2 * n, dtype=torch.float16, device="cuda")
    tf.synth_uniform(x, x[n:], n, batch, seed=77)
    y = torch.full_like(x, float("nan"))
    kw = {"output_order": "transposed"} if order == "transposed_out" else {"input_order": "transposed"}
    plan = tf.TfftPlan(n, batch, 0, preserve_input=True, **kw)
    assert plan.workspace_bytes == chunk * n * 4                 # ONE chunk of intermediate, whatever the batch
    plan.exec(x, x[n:], y, y[n:])
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y).any())
    for b in (0, chunk - 1, chunk, batch - 1):                   # last of the full chunk, first and last of the tail
        re, im = orc.synth_uniform(n, 1, b, 77)
        if order == "transposed_in":                             # the generated block IS the [N1][N2] matrix: x[k1 + N1 k2] = in[k1 N2 + k2]
            perm = np.arange(n).reshape(n1, n2).T.reshape(-1)
            re, im = np.ascontiguousarray(re[:, perm]), np.ascontiguousarray(im[:, perm])
        e_re, e_im = orc.dft64(re, im)
        exact = e_re[0] + 1j * e_im[0]
        if order == "transposed_out":
            exact = exact[np.arange(n).reshape(n2, n1).T.reshape(-1)]     # out[k1 N2 + k2] = X[k1 + N1 k2]
        o = y[b * 2 * n:(b + 1) * 2 * n].cpu().numpy().astype(np.float64)
        got = o[:n] + 1j * o[n:]
        assert np.linalg.norm(got - exact) / np.linalg.norm(exact) <= REL_L2_TOL, (order, b)


def test_chunked_2d_plan_with_a_tail_chunk_and_in_place(tf, orc):
    """4096 x 4096 x 6: one chunk of 4 images and a tail of 2; the workspace is one chunk; results equal the batch-1 plan's bit for
    bit, image by image, also when the plan runs in place."""
    import torch

    n, images = 4096, 6
    half = images * n * n
    x = torch.empty(2 * half, dtype=torch.float16, device="cuda")
    tf.synth_uniform(x[:half], x[half:], n * n, images, batch_stride=n * n, seed=5)
    y = torch.full_like(x, float("nan"))
    plan = tf.TfftPlan2D(n, n, images, 0)
    assert plan.workspace_bytes == 4 * n * n * 4
    plan.exec(x[:half], x[half:], y[:half], y[half:])
    one = tf.TfftPlan2D(n, n, 1, 0)
    z = torch.empty(2 * n * n, dtype=torch.float16, device="cuda")
    for i in range(images):
        one.exec(x[i * n * n:(i + 1) * n * n], x[half + i * n * n:half + (i + 1) * n * n], z[:n * n], z[n * n:])
        torch.cuda.synchronize()
        assert bool((z[:n * n].view(torch.int16) == y[i * n * n:(i + 1) * n * n].view(torch.int16)).all()), i
        assert bool((z[n * n:].view(torch.int16) == y[half + i * n * n:half + (i + 1) * n * n].view(torch.int16)).all()), i
    plan.exec(x[:half], x[half:], x[:half], x[half:])            # in place
    torch.cuda.synchronize()
    assert bool((x.view(torch.int16) == y.view(torch.int16)).all())


def test_dist_set_buffers_validates_ranges_before_it_commits(tf):
    """tfft_dist_plan_set_buffers used to assign first and check pointer equality only. Now: range overlap over
    N / world halves, and a refused call leaves the plan on its previous buffers."""
    import torch
    from tensor_fft_amd import capi

    n, world = 1 << 20, 2
    loc = n // world
    big = torch.zeros(5 * loc, dtype=torch.float16, device="cuda")
    good = [big[i * loc:(i + 1) * loc] for i in range(4)]
    p = capi.DistPlan(n, world, 0, 0, buffers=tuple(good))
    before = [ctypes.c_void_p() for _ in range(4)]
    capi.load_library().tfft_dist_plan_buffers(p._h, *[ctypes.byref(b) for b in before])
    assert [b.value for b in before] == [t.data_ptr() for t in good]
    shifted = big[loc // 2:loc // 2 + loc]                       # overlaps send_re and send_im partially
    for bad in ((good[0], good[1], shifted, good[3]), (good[0], shifted, good[2], good[3]), (good[0], good[1], good[2], good[2])):
        with pytest.raises(tf.TfftError) as e:
            p.set_buffers(*bad)
        assert e.value.code == 5
        after = [ctypes.c_void_p() for _ in range(4)]
        capi.load_library().tfft_dist_plan_buffers(p._h, *[ctypes.byref(b) for b in after])
        assert [b.value for b in after] == [b.value for b in before]          # nothing changed
    # a plan created for caller buffers refuses to run before it has them
    L = capi.load_library()
    h = ctypes.c_void_p()
    assert L.tfft_dist_plan_create(n, world, 0, 0, None, capi.DIST_CALLER_BUFFERS, ctypes.byref(h)) == 0
    assert L.tfft_dist_exec_pre(h, good[0].data_ptr(), good[1].data_ptr(), None) == 5 and "set_buffers" in capi.last_error()
    L.tfft_dist_plan_destroy(h)


def test_transposed_input_is_as_accurate_as_natural_order(tf, orc):
    """The four-step twiddle of a transposed-input plan is applied to fp32 accumulators (one rounding, like every other stage):
    its error against the fp64 oracle stays within 10 % of the natural-order plan's on the same signal (and far below the
    restatement of the reference kernels)."""
    import torch

    for lg in (16, 20):
        n = 1 << lg
        n2 = tf.transposed_n2(n)
        n1 = n // n2
        re, im = orc.synth_uniform(n, 1, 0, lg + 100)
        e_re, e_im = orc.dft64(re, im)
        exact = e_re[0] + 1j * e_im[0]
        errs = {}
        for order in ("natural", "transposed_in"):
            a, b = re[0], im[0]
            if order == "transposed_in":
                a, b = _transposed_layout(a, n1, n2), _transposed_layout(b, n1, n2)
            x = torch.from_numpy(np.concatenate([a, b])).cuda()
            y = torch.empty_like(x)
            tf.TfftPlan(n, 1, 0, preserve_input=True, input_order="transposed" if order == "transposed_in" else "natural").exec(x, x[n:], y, y[n:])
            torch.cuda.synchronize()
            o = y.cpu().numpy().astype(np.float64)
            errs[order] = float(np.linalg.norm(o[:n] + 1j * o[n:] - exact) / np.linalg.norm(exact))
        assert errs["transposed_in"] <= 1.1 * errs["natural"] + 1e-5, (lg, errs)
        assert errs["transposed_in"] < 6e-4, (lg, errs)


def test_c_abi_spectral_filter_example():
    """examples/example_spectral_filter.cpp: forward (transposed output, unscaled) -> pointwise delay filter -> inverse (transposed
    input) through the plain C ABI, 2 + 2 passes; the program checks the delayed signal itself."""
    exe = os.path.join(ROOT, "examples", "example_spectral_filter")
    for args in (["22", "8", "5"], ["16", "40", "1"], ["24", "3", "12345"]):
        r = subprocess.run(["timeout", "-k", "10", "300", exe] + args, capture_output=True, text=True)
        print(r.stdout, r.stderr)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
        assert "forward 2 passes, inverse 2 passes" in r.stdout


@pytest.mark.parametrize("lg,batch,order", [(18, 32, "natural"), (19, 12, "natural"), (20, 16, "natural"), (21, 8, "natural"),
                                            (22, 4, "natural"), (24, 1, "natural"), (17, 32, "natural"),
                                            (20, 16, "transposed"), (22, 4, "transposed"), (24, 1, "transposed"),
                                            (20, 16, "transposed_in")])
def test_cache_policy_changes_the_time_never_the_result(tf, lg, batch, order):
    """The column passes exist with plain and with non-temporal global accesses (COL_CACHED / COL_STREAMING; neither = the
    library picks by the plan's footprint, tfft_plan_cache_policy): same arithmetic, so the three plans must agree to the bit."""
    import torch

    n = 1 << lg
    x = torch.empty(batch * 2 * n, dtype=torch.float16, device="cuda")
    tf.synth_uniform(x, x[n:], n, batch)
    kw = {"natural": {}, "transposed": {"output_order": "transposed"}, "transposed_in": {"input_order": "transposed"}}[order]
    if order == "natural" and tf.plan_default_variant(n, 1, batch):
        pytest.skip("variant 0 of this shape is another split (tfft_plan_default_variant), not another cache policy of the same plan")
    outs = []
    for v in (0, capi.VARIANT_COL_CACHED, capi.VARIANT_COL_STREAMING):
        plan = tf.TfftPlan(n, batch, 0, variant=v, preserve_input=True, **kw)
        ws = torch.empty(max(1, plan.workspace_bytes // 2), dtype=torch.float16, device="cuda")
        if plan.workspace_bytes:
            plan.set_workspace(ws)
        y = torch.full_like(x, float("nan"))
        plan.exec(x, x[n:], y, y[n:])
        torch.cuda.synchronize()
        outs.append(y.view(torch.int16))
        plan.close()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert not torch.isnan(outs[0].view(torch.float16)).any()


@pytest.mark.parametrize("lg,batch", [(18, 1), (18, 16), (18, 32), (18, 64), (18, 128), (19, 1), (19, 4), (19, 8), (19, 16), (20, 1), (20, 8), (20, 16), (21, 1), (21, 2), (21, 4), (25, 1), (17, 64), (17, 256), (24, 2)])
def test_small_work_default_split_against_the_oracle_and_the_large_batch_split(tf, orc, lg, batch):
    """A variant-0 plan that does not fill the chip takes the split with more workgroups (tfft_plan_default_variant). Either split
    must be within the stated tolerance of the fp64 oracle, and the default plan must BE the variant it reports."""
    import torch

    n = 1 << lg
    x = torch.empty(batch * 2 * n, dtype=torch.float16, device="cuda")
    tf.synth_uniform(x, x[n:], n, batch)
    dv = tf.plan_default_variant(n, 1, batch)
    outs = {}
    for name, v in (("default", 0), ("reported", dv), ("large-batch split", capi.VARIANT_COL_STREAMING)):
        plan = tf.TfftPlan(n, batch, 0, variant=v, preserve_input=True)
        ws = torch.empty(max(1, plan.workspace_bytes // 2), dtype=torch.float16, device="cuda")
        if plan.workspace_bytes:
            plan.set_workspace(ws)
        y = torch.full_like(x, float("nan"))
        plan.exec(x, x[n:], y, y[n:])
        torch.cuda.synchronize()
        outs[name] = y.cpu().numpy().reshape(batch, 2, n)
        if name == "default":
            assert plan.num_launches == len(tf.plan_describe(n, 1, dv).split())
        plan.close()
    if dv:
        assert np.array_equal(outs["default"].view(np.uint16), outs["reported"].view(np.uint16))
    xin = x.cpu().numpy().reshape(batch, 2, n)
    for b in range(batch):                  # every transform of the batch
        er, ei = orc.dft64(xin[b:b + 1, 0], xin[b:b + 1, 1])                   # fp64 DFT(x) / N, the plan's scaling
        exact = er[0] + 1j * ei[0]
        for name in ("default", "large-batch split"):
            got = outs[name][b, 0].astype(np.float64) + 1j * outs[name][b, 1].astype(np.float64)
            rel = np.linalg.norm(got - exact) / np.linalg.norm(exact)
            assert rel <= 1.5e-3, (name, lg, batch, b, rel)
            eb.check(got.real, got.imag, exact.real, exact.imag, K_ANY, what=f"{name} 2^{lg} x {batch}, transform {b}")


@pytest.mark.parametrize("n,inner,batch", [(1 << 16, 1, 129), (1 << 16, 1, 513), (1 << 16, 1, 2049), (1 << 16, 1, 4100),
                                           (256, 64, 8191), (256, 4096, 131), (1 << 17, 1, 1027)])
def test_rounds_per_workgroup_launch_shape_at_ragged_block_counts(tf, n, inner, batch):
    """The radix-256 workgroup kernel is launched with about four rounds per workgroup in whole multiples of the resident
    capacity (tfft.hip rounds_grid): block counts just off those multiples, against the static partition (launch_iters =
    persistent) and one round per workgroup, bit for bit."""
    import torch

    nf = n * inner
    x = torch.empty(batch * 2 * nf, dtype=torch.float16, device="cuda")
    tf.synth_uniform(x, x[nf:], nf, batch)
    outs = []
    for it in (0, 65535, 1):
        plan = tf.TfftPlan(n, batch, 0, inner=inner, preserve_input=True, launch_iters=it)
        ws = torch.empty(max(1, plan.workspace_bytes // 2), dtype=torch.float16, device="cuda")
        if plan.workspace_bytes:
            plan.set_workspace(ws)
        y = torch.full_like(x, float("nan"))
        plan.exec(x, x[nf:], y, y[nf:])
        torch.cuda.synchronize()
        outs.append(y.view(torch.int16))
        plan.close()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert not torch.isnan(outs[0].view(torch.float16)).any()
