"""bench.py --gpus N without a launcher starts its ranks itself: the spawn logic on CPU, two ranks
over gloo with the numpy engine from tests/; and the failure modes: a rank that dies, a box with too few GPUs."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCRIPT = os.path.join(ROOT, "tests", "helpers", "launch_rank.py")


def test_self_launch_runs_two_ranks_and_relays_rank_zero(capfd):
    import bench

    rc = bench.self_launch(2, SCRIPT, ["--gpus", "2"])
    out = capfd.readouterr().out
    assert rc == 0, out
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1                         # ONE JSON line, rank 0's
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rel_l2"] < 1.5e-3


def test_self_launch_reports_a_failed_rank(capfd):
    import bench

    rc = bench.self_launch(2, SCRIPT, ["--gpus", "2", "--fail-rank", "1"])
    captured = capfd.readouterr()
    assert rc != 0
    assert "2-rank run failed" in captured.err


def test_self_launch_refuses_more_ranks_than_gpus(capfd):
    import bench

    assert bench.self_launch(2, SCRIPT, ["--gpus", "2"], nproc_visible=1) == 2
    captured = capfd.readouterr()
    assert "needs 2 GPUs" in captured.err and "{" not in captured.out          # nothing was started


def test_bench_gpus_2_on_a_box_without_two_gpus_fails_clearly():
    """The driver's own command line, no launcher: on this box (no GPU, or one) it must fail with a clear message and a
    non-zero exit code before any rank starts."""
    import torch

    if torch.cuda.device_count() >= 2:
        import pytest

        pytest.skip("two GPUs present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "needs 2 GPUs" in r.stderr and not r.stdout.strip().startswith("{")


@pytest.mark.parametrize("flag", ["--with-dist", "--dist-self-via-comm", "--only-dist-entry"])
def test_bench_dist_options_need_full(flag):
    """The configs[4b] options belong to --full: without it the command is refused before anything is built or started."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", flag], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2
    assert f"{flag} is part of --full" in r.stderr and not r.stdout.strip()


@pytest.mark.gpu
def test_bench_plain_run_posts_only_the_headline():
    """bench.py without --full: the self-checked headline line, and none of what --full adds (single launches, CPU baseline,
    other_configs)."""
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1"], capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert d["unit"] == "Gsamples/s" and d["dtype"] == "f16" and "rel-L2" in d["config"]["self_check"]
    assert d["roofline"]["kernel_ms"] > 0 and "kernel_ms_single_launches" not in d["roofline"]
    assert "cpu_baseline" not in d and "other_configs" not in d


def test_dump_outputs_writes_a_fixed_float32_sample(tmp_path):
    """--dump-outputs on a host tensor in the output layout ([fft_i RE | fft_i IM] fp16 blocks): float32 .npy files, the same
    seeded sample of transforms in every run, the values of those transforms exactly, at most 64 MB in all."""
    import numpy as np
    import torch

    import bench

    n, batch = bench.N, bench.DUMP_TRANSFORMS + 333
    y = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, batch * 2 * n).astype(np.float16))
    a, b = tmp_path / "a", tmp_path / "b"
    rep = bench.dump_outputs(torch, y, n, batch, str(a))
    bench.dump_outputs(torch, y, n, batch, str(b))
    assert rep["transforms"] == bench.DUMP_TRANSFORMS
    total = 0
    for name in ("out_re", "out_im", "transform_index"):
        u, v = np.load(a / (name + ".npy")), np.load(b / (name + ".npy"))
        assert u.dtype in (np.float32, np.float64) and np.array_equal(u, v)
        total += (a / (name + ".npy")).stat().st_size
    assert total <= 64 << 20
    ids = np.load(a / "transform_index.npy").astype(np.int64)
    assert len(set(ids.tolist())) == bench.DUMP_TRANSFORMS and ids.min() >= 0 and ids.max() < batch
    blocks = y.numpy().reshape(batch, 2, n)[ids].astype(np.float32)
    assert np.array_equal(np.load(a / "out_re.npy"), blocks[:, 0]) and np.array_equal(np.load(a / "out_im.npy"), blocks[:, 1])
    small = bench.dump_outputs(torch, y[: 5 * 2 * n], n, 5, str(tmp_path / "c"))      # a small batch is written whole
    assert small["transforms"] == 5 and np.array_equal(np.load(tmp_path / "c" / "transform_index.npy"), np.arange(5.0))


@pytest.mark.gpu
def test_bench_dump_outputs_holds_what_the_timed_step_computed(tmp_path, orc):
    """bench.py --steps 1 --dump-outputs end to end: the result line counts one timed step and describes the dump, and sampled
    rows of the dump are the oracle's fp64 DFT/N of the transforms that transform_index.npy names."""
    import numpy as np

    import bench

    out = tmp_path / "dump"
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1",
                        "--warmup", "1", "--no-other-configs", "--no-cpu-baseline", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 1 and d["ms_per_step"] > 0
    assert d["dump_outputs"]["dir"] == str(out) and d["dump_outputs"]["transforms"] == bench.DUMP_TRANSFORMS
    got_re, got_im = np.load(out / "out_re.npy"), np.load(out / "out_im.npy")
    ids = np.load(out / "transform_index.npy").astype(np.int64)
    assert got_re.dtype == got_im.dtype == np.float32 and got_re.shape == got_im.shape == (bench.DUMP_TRANSFORMS, bench.N)
    for k in (0, len(ids) // 2, len(ids) - 1):
        x_re, x_im = orc.synth_uniform(bench.N, 1, int(ids[k]), bench.SEED)
        e_re, e_im = orc.dft64(x_re, x_im)
        exact = e_re[0] + 1j * e_im[0]
        got = got_re[k].astype(np.float64) + 1j * got_im[k]
        assert np.linalg.norm(got - exact) / np.linalg.norm(exact) < bench.REL_L2_TOL, (k, int(ids[k]))
