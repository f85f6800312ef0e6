"""bench.py's launcher contract, host-only: `--gpus N` without a launcher
starts N ranks itself, a launcher world that differs from --gpus is refused
before anything touches torch or a GPU, and configs[3]'s strong-scaling shard
sizes."""
import os
import subprocess
import sys

import pytest

import bench
from conftest import REPO


def test_world_check():
    assert bench.world_check(1, {}) is None
    assert bench.world_check(8, {}) == "spawn"
    assert bench.world_check(8, {"WORLD_SIZE": "8"}) is None
    assert bench.world_check(1, {"WORLD_SIZE": "1"}) is None
    assert "WORLD_SIZE=2" in bench.world_check(8, {"WORLD_SIZE": "2"})


def test_world_mismatch_refused_before_torch():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    # -X importtime would show torch; simpler: the refusal exits 2 within a
    # second, long before `import torch` could have finished
    p = subprocess.run([sys.executable, "-c",
                        "import sys; sys.argv = ['bench.py', '--gpus', '8']; import bench; bench.main()"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=60)
    assert p.returncode == 2, p.stderr
    assert "WORLD_SIZE=2 but --gpus 8" in p.stderr


def test_plain_run_is_the_default_and_full_is_an_option():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(["--full", "--verify-single", "--dump-outputs", "d"])
    assert a.full and a.verify_single and a.dump_outputs == "d"
    # a check beyond the headline without --full, or no timed step: refused
    for argv in (["--verify-single"], ["--steps", "0"]):
        with pytest.raises(SystemExit) as ei:
            bench.parse(argv)
        assert ei.value.code == 2


def test_dump_windows_are_fixed_and_bounded():
    assert bench.dump_windows(0, 1 << 22, 1 << 22) == [(0, 1 << 22)]           # k = 11: the whole table
    assert bench.dump_windows(1 << 21, 1 << 22, 1 << 24) == [(1 << 21, 1 << 21)]  # a rank's small slice
    for lo, hi in ((0, 1 << 24), (0, 1 << 40), (3 << 30, 1 << 32), (1 << 22, 1 << 23)):
        w = bench.dump_windows(lo, hi, 1 << 40)
        assert w == bench.dump_windows(lo, hi, 1 << 40) == sorted(w)     # the same sample every run
        assert len(w) == bench.DUMP_WINDOWS
        assert all(lo <= s and s + n <= hi and n == bench.DUMP_WINDOW for s, n in w)
    # table.npy + table_index.npy as float64, with counters.npy: under 64 MB
    assert 2 * 8 * bench.DUMP_WINDOWS * bench.DUMP_WINDOW + 8 * 32 < 64_000_000
    assert 8 * bench.DUMP_WHOLE + 8 * 32 < 64_000_000


def test_launcher_command():
    cmd = bench.launcher_cmd(8, ["--gpus", "8", "--steps", "5"], 29511)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    i = cmd.index("--nproc-per-node")
    assert cmd[i + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--master-port") + 1] == "29511"
    assert cmd[-5:] == [os.path.join(REPO, "bench.py"), "--gpus", "8", "--steps", "5"]


def test_strong_scaling_shards():
    # configs[3]: the 10 G-base genome split N ways, whole FASTA lines and words
    for n in (1, 2, 4, 8):
        s = bench.shard_bases(10_000_000_000, n, 80)
        assert s * n == 10_000_000_000 and s % 80 == 0 and s % 32 == 0
    s = bench.shard_bases(10_000_000_000, 3, 80)
    assert s % 160 == 0 and 3 * s <= 10_000_000_000
    assert bench.shard_bases(25_600_000, 2, 0) == 12_800_000
