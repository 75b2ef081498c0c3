"""bench.py's `--gpus N` contract, on CPU: under a launcher N must
equal WORLD_SIZE; without one, a single process drives N devices and refuses when
fewer are visible -- never a mislabeled line."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_resolve_topology_cases():
    from bench import resolve_topology
    assert resolve_topology(1, {}, 1) == ("process", 1, 0, 0)
    assert resolve_topology(8, {}, 8) == ("process", 8, 0, 0)
    assert resolve_topology(2, {"WORLD_SIZE": "2", "RANK": "1", "LOCAL_RANK": "1"}, 8) == ("ranks", 2, 1, 1)
    assert resolve_topology(1, {"WORLD_SIZE": "1"}, 1) == ("ranks", 1, 0, 0)
    with pytest.raises(SystemExit, match="only 1 HIP device"):
        resolve_topology(2, {}, 1)
    with pytest.raises(SystemExit, match="WORLD_SIZE=1"):
        resolve_topology(8, {"WORLD_SIZE": "1"}, 8)
    with pytest.raises(SystemExit, match="WORLD_SIZE=4"):
        resolve_topology(8, {"WORLD_SIZE": "4", "RANK": "0"}, 8)
    with pytest.raises(SystemExit, match=">= 1"):
        resolve_topology(0, {}, 8)


def test_bench_refuses_more_gpus_than_visible():
    """`python bench.py --gpus 2` on a machine with fewer devices exits non-zero with a
    message before touching a GPU (here: none visible)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0
    assert "--gpus 2 but only" in r.stderr
    assert r.stdout.strip() == ""


class _FakeLane:
    """What dump_outputs needs of a bench.Lane: its sizes, its sets and the last step's arrays."""

    def __init__(self, B, M, sets, seed):
        self.B, self.M, self.bufs = B, M, [None] * sets
        self.C = np.random.default_rng(seed).standard_normal((B, M, 3, 8))

    def last_step_outputs(self, K, index):
        return self.C[index], np.zeros(self.B, dtype=np.int32)


def test_dump_outputs_is_a_fixed_sample_under_the_size_limit(tmp_path):
    """--dump-outputs: float64 .npy files, the same seeded sample of trajectories in every
    run, every GPU's share of it, under 64 MB in all at the headline's size."""
    import bench
    B, M = 65536, 10
    lanes = [_FakeLane(B, M, 4, 1), _FakeLane(B, M, 4, 2)]
    infos = [bench.dump_outputs(str(tmp_path / d), lanes, [0, 1], 2, 7) for d in ("a", "b")]
    assert infos[0]["step"] == 6 and infos[0]["set"] == 2
    assert sorted(infos[0]["files"]) == ["coeffs.npy", "coeffs_gpu1.npy", "sample_index.npy", "status.npy",
                                         "status_gpu1.npy"]
    total = 0
    for fn in infos[0]["files"]:
        a, b = np.load(tmp_path / "a" / fn), np.load(tmp_path / "b" / fn)
        assert a.dtype == np.float64 and np.array_equal(a, b)
        total += os.path.getsize(tmp_path / "a" / fn)
    assert total == sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 10 ** 6
    idx = np.load(tmp_path / "a" / "sample_index.npy").astype(np.int64)
    n = bench.DUMP_SAMPLE_BYTES // (M * 3 * 8 * 8 * 2)
    assert idx.shape == (n,) and (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < B
    assert np.array_equal(np.load(tmp_path / "a" / "coeffs.npy"), lanes[0].C[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "coeffs_gpu1.npy"), lanes[1].C[idx])
    assert np.load(tmp_path / "a" / "status.npy").shape == (B,)
    # a batch that fits is written whole
    small = _FakeLane(300, 3, 4, 3)
    bench.dump_outputs(str(tmp_path / "c"), [small], [0], 1, 1)
    assert np.array_equal(np.load(tmp_path / "c" / "coeffs.npy"), small.C)


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_the_last_step(tmp_path, solver):
    """A plain `bench.py --steps K` run prints the headline line without the side
    measurements that --full adds, and --dump-outputs holds what step K - 1 (batch
    (K - 1) % sets, seeded) computed: bit for bit what the library solves for that batch."""
    import json

    import torch

    from trajectory_generator_ros2_amd import METHOD_REDUCED
    from trajectory_generator_ros2_amd import synthetic as S
    B, M, K, sets = 1536, 10, 7, 4
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K),
                        "--warmup", "2", "--batch", str(B), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == K and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["full"] is False
    assert d["unit"] == "trajectories/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert abs(d["value"] - B / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    for side in ("cpu_baseline", "verification", "per_launch", "config2", "config4", "config5", "sampler",
                 "dense_kkt", "band_kkt", "host_path", "node_config1"):
        assert side not in d, side
    assert sorted(os.listdir(tmp_path)) == ["coeffs.npy", "sample_index.npy", "status.npy"]
    C, st = np.load(tmp_path / "coeffs.npy"), np.load(tmp_path / "status.npy")
    assert C.dtype == np.float64 and C.shape == (B, M, 3, 8) and st.shape == (B,) and (st == 0).all()
    assert np.array_equal(np.load(tmp_path / "sample_index.npy"), np.arange(B))
    _, W, T = S.uniform_batch(B, M, seed=S.SEED + 7919 * ((K - 1) % sets))
    ref = torch.empty((B, M, 3, 8), dtype=torch.float64, device="cuda:0")
    solver.set_method(METHOD_REDUCED)
    solver.solve_uniform_device(B, M, torch.from_numpy(W).cuda(0), torch.from_numpy(T).cuda(0), ref)
    torch.cuda.synchronize()
    assert np.array_equal(C, ref.cpu().numpy())


def test_bench_refuses_streams_that_would_share_a_batch():
    """With --streams S the timed steps alternate over S streams and step k solves batch
    k % sets: unless S divides sets, two steps in flight at once could write one batch.
    bench.py refuses before touching a GPU."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--streams", "3", "--sets", "4",
                        "--steps", "1"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0
    assert "must be a multiple of --streams 3" in r.stderr
    assert r.stdout.strip() == ""
