"""bench.py's own launcher (no GPU): `bench.py --gpus N` without WORLD_SIZE
starts N ranks itself; under a launcher WORLD_SIZE must equal --gpus."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [2, 4, 8])
def test_bench_starts_its_own_ranks(n):
    """`bench.py --gpus N` (the driver's N = 2, 4, 8 scaling runs) starts N
    ranks, and each rehearses config 5's exchange schedule over gloo: 8 / N
    views per rank, the pipelined view-record gather (at N = 8 one view per
    rank: only the chunked last-view path) and the flat gradient all-reduce,
    bit-identical on every rank."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--launcher-dry-run"],
                       capture_output=True, text=True, env=_env(), timeout=280)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1  # rank 0 only
    L = lines[0]
    assert L["n_gpus"] == n and L["allreduce_ok"] and L["views_per_rank"] == 8 // n
    assert L["view_exchange_ok"] and L["grad_allreduce_ok"] and L["ranks_identical"]


@pytest.mark.timeout(120)
def test_bench_rejects_world_size_mismatch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launcher-dry-run"],
                       capture_output=True, text=True, env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"),
                       timeout=100)
    assert r.returncode == 2
    assert "WORLD_SIZE=1" in r.stderr


@pytest.mark.timeout(120)
def test_bench_single_rank_dry_run():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--launcher-dry-run"],
                       capture_output=True, text=True, env=_env(), timeout=100)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1])["n_gpus"] == 1


def test_plain_run_drops_everything_but_the_headline():
    """Without --full every extra leg is off; --full turns them on, and each
    --no-* option takes its leg out again."""
    import bench
    legs = ("no_cpu_baseline", "no_sub", "no_profile", "no_ext")
    plain = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not plain.full and plain.steps == 7 and plain.warmup == 2 and plain.dump_outputs is None
    assert all(getattr(plain, k) for k in legs)
    full = bench.parse_args(["--full"])
    assert full.full and not any(getattr(full, k) for k in legs)
    part = bench.parse_args(["--full", "--no-sub"])
    assert part.no_sub and not part.no_profile


def test_dump_outputs_is_repeatable_and_within_budget(tmp_path, monkeypatch):
    """--dump-outputs: float32 .npy files; arrays within their share of the
    budget whole, larger ones as the same seeded sample on every call."""
    import numpy as np
    import torch

    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 300)
    g = torch.Generator().manual_seed(1)
    arrays = {"color": torch.rand(3, 20, 30, generator=g), "radii": torch.arange(50, dtype=torch.int32),
              "grad_shs": torch.rand(100, 16, 3, generator=g), "unset": None}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, seed=0)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("color", "radii", "grad_shs")}
    assert not (tmp_path / "a" / "unset.npy").exists()
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 4 * 300
    np.testing.assert_array_equal(got["radii"], np.arange(50, dtype=np.float32))  # within its share: whole
    assert got["color"].shape == (125,) and got["grad_shs"].shape == (125,)       # (300 - 50) / 2 each
    for n, a in got.items():
        np.testing.assert_array_equal(a, np.load(tmp_path / "b" / f"{n}.npy"))
    man = json.load(open(tmp_path / "a" / "manifest.json"))["arrays"]
    assert man["grad_shs"] == {"shape": [100, 16, 3], "dtype": "float32", "kept": 125, "sampled": True}
    # the sample holds elements of the array at the recorded seed's indices
    idx = np.sort(np.random.default_rng([0, sorted(got).index("grad_shs")]).integers(0, 4800, 125))
    np.testing.assert_array_equal(got["grad_shs"], arrays["grad_shs"].reshape(-1).numpy()[idx])
