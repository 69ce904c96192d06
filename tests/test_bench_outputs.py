"""bench.py's plain run and its --full / --dump-outputs options: a plain run times exactly --steps steps and reports them,
--full adds the repeated windows and the CPU baseline, and --dump-outputs writes the factors of the timed path's last step
(the same ones with the same arguments, the ones the oracle computes from the same seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_full_and_dump_outputs_options():
    import bench
    a = bench.parse_args([])
    assert not a.full and a.dump_outputs is None
    a = bench.parse_args(["--full", "--api-path", "--dump-outputs", "out"])
    assert a.full and a.api_path and a.dump_outputs == "out"
    for argv in (["--api-path"], ["--gpus", "2", "--dump-outputs", "out"]):
        with pytest.raises(SystemExit):
            bench.parse_args(argv)


def test_written_outputs_are_capped_and_sampled_the_same_way(tmp_path):
    from bench_launch import DUMP_BYTES_PER_ARRAY, write_outputs
    rng = np.random.default_rng(5)
    W, H = rng.random((262144, 64)), rng.random((64, 65536))           # C4's factors: 134 MB + 34 MB in fp64
    for d in ("a", "b"):
        write_outputs(str(tmp_path / d), W, H)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in ("W.npy", "H.npy"))
    assert total <= 64 * 10**6
    Wa, Ha = np.load(tmp_path / "a" / "W.npy"), np.load(tmp_path / "a" / "H.npy")
    assert Wa.dtype == np.float64 and Wa.shape[1] == 64 and Wa.nbytes <= DUMP_BYTES_PER_ARRAY
    assert Ha.dtype == np.float64 and Ha.shape[0] == 64 and Ha.nbytes <= DUMP_BYTES_PER_ARRAY
    assert (Wa == np.load(tmp_path / "b" / "W.npy")).all() and (Ha == np.load(tmp_path / "b" / "H.npy")).all()
    rows = [int(np.flatnonzero((W == r).all(axis=1))[0]) for r in Wa[:50]]   # whole rows of W, in order
    assert rows == sorted(rows)
    write_outputs(str(tmp_path / "small"), W[:512, :8], H[:8, :256])     # small factors are written whole
    assert (np.load(tmp_path / "small" / "W.npy") == W[:512, :8]).all()
    assert (np.load(tmp_path / "small" / "H.npy") == H[:8, :256]).all()


def _bench(*args):
    r = subprocess.run([sys.executable, "bench.py", "--workload", "c1", "--steps", "4", "--warmup", "2", *args], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1, r.stdout[-1500:]
    return json.loads(line[0])


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_factors(tmp_path):
    import oracle
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    assert plain["steps"] == 4 and plain["windows"] == 1 and "cpu_baseline" not in plain
    assert abs(plain["ms_per_step"] - plain["windows_ms"][0] / 4) <= 1e-3 * plain["ms_per_step"]
    assert abs(plain["value"] * plain["ms_per_step"] - 1e3) <= 1e-6 * 1e3
    full = _bench("--full", "--dump-outputs", str(tmp_path / "full"))
    assert full["windows"] >= 5 and "cpu_baseline" in full
    assert abs(full["ms_per_step"] - full["windows_ms"][0] / 4) <= 1e-3 * full["ms_per_step"]
    W, H = np.load(tmp_path / "plain" / "W.npy"), np.load(tmp_path / "plain" / "H.npy")
    assert (W == np.load(tmp_path / "full" / "W.npy")).all() and (H == np.load(tmp_path / "full" / "H.npy")).all()
    # C1: 512 x 256, k = 8, MU, A in fp32 on the device; warm-up + timed steps = 6 iterations from bench.py's seeded start
    m, n, k = 512, 256, 8
    ref = oracle.nmf(oracle.fill_uniform(m, n, 42), oracle.fill_uniform(m, k, 43), oracle.fill_uniform(k, n, 44) * (2.0 / k), "MU",
                     min_iter=6, max_iter=6)
    assert W.shape == (m, k) and H.shape == (k, n)
    scale = np.linalg.norm(W, axis=0)                   # the dump is unnormalised; the oracle returns unit columns of W
    assert np.linalg.norm(W / scale - ref.W) / np.linalg.norm(ref.W) < 1e-4
    assert np.linalg.norm(H * scale[:, None] - ref.H) / np.linalg.norm(ref.H) < 1e-4
