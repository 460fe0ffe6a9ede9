"""GPU: bench.py on one GPU.  A plain run is the headline and nothing else, --steps sets the timed steps, --dump-outputs
writes what the last timed step computed (held against the CPU oracle), and --full still carries every other figure."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import datagen
import parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("kernel_ms", "roofline", "cpu_baseline", "direct_cotangent", "no_skip", "pipelined_walk", "clocks")


def _bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BENCH_FORCE_DIST", "BENCH_SHARE_GPU", "BENCH_BACKEND")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args,
                       capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    B, N, M = 8, 64, 64
    out = tmp_path / "out"
    d = _bench(["--steps", "5", "--warmup", "2", "--B", str(B), "--N", str(N), "--M", str(M), "--dump-outputs", str(out)])
    assert d["steps"] == 5 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["unit"] == "cell-updates/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["metric"] == "DP cell-updates/sec (fwd+bwd)"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 2 * B * N * M / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert not [k for k in FULL_ONLY if k in d], d
    assert sorted(os.listdir(out)) == ["E.npy", "Vt.npy"]
    got = {k: np.load(out / f"{k}.npy") for k in ("Vt", "E")}
    assert got["E"].dtype == np.float32 and got["E"].shape == (B, N, M) and got["Vt"].shape == (B,)
    theta, A = datagen.theta_A(1, B, N, M)    # bench.py's inputs on rank 0
    errs = parity.compare(got, parity.oracle_all(theta, A, None, None, 0, omp=False))
    assert max(errs.values()) <= parity.TOL, errs


@pytest.mark.gpu
def test_dump_of_the_headline_shape_is_a_fixed_sample(tmp_path):
    """B=256, N=M=512: E (256 MB) is cut to the same seeded pairs on every run, all files together within 64 MB."""
    sys.path.insert(0, ROOT)
    import bench
    runs = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        _bench(["--steps", "2", "--warmup", "1", "--dump-outputs", str(out)])
        runs.append({k: np.load(out / f"{k}.npy") for k in ("Vt", "E")})
        assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20
    k = runs[0]["E"].shape[0]
    assert 1 <= k < 256 and runs[0]["E"].shape == (k, 512, 512) and runs[0]["Vt"].shape == (k,)
    for name in ("Vt", "E"):
        assert np.array_equal(runs[0][name], runs[1][name]), name
    pairs = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(256, size=k, replace=False))
    theta, A = datagen.theta_A(1, 256, 512, 512)
    ref = parity.oracle_all(np.ascontiguousarray(theta[pairs[:4]]), np.ascontiguousarray(A[pairs[:4]]), None, None, 0)
    errs = parity.compare({"Vt": runs[0]["Vt"][:4], "E": runs[0]["E"][:4]}, ref)
    assert max(errs.values()) <= parity.TOL, errs


@pytest.mark.gpu
def test_traceback_mode_dumps_the_walks(tmp_path):
    out = tmp_path / "out"
    d = _bench(["--steps", "3", "--warmup", "1", "--B", "6", "--N", "40", "--M", "50", "--mode", "align+traceback",
                "--dump-outputs", str(out)])
    assert d["steps"] == 3 and "pipelined_walk" not in d
    states, counts = np.load(out / "path_states.npy"), np.load(out / "path_counts.npy")
    assert states.dtype == np.float64 and states.shape[0] == 6 and states.shape[2] == 3 and counts.shape == (6,)
    assert np.array_equal(states, np.round(states)) and np.array_equal(counts, np.round(counts)) and (counts != 0).all()


@pytest.mark.gpu
def test_full_run_keeps_every_figure():
    d = _bench(["--steps", "3", "--warmup", "1", "--B", "8", "--N", "64", "--M", "64", "--cpu-pairs", "8", "--full"])
    assert d["steps"] == 3 and d["value"] > 0
    for k in ("kernel_ms", "roofline", "cpu_baseline", "direct_cotangent", "no_skip"):
        assert k in d, k
    assert d["roofline"]["kernel"].startswith("sdp_") and d["cpu_baseline"]["value"] > 0 and d["no_skip"]["value"] > 0
