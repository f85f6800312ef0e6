"""bench.py's plain run on the GPU: the line carries the headline only, and
--dump-outputs writes what the last timed step computed -- checked against
the CPU oracle over the same seeded stream, for each form of table: whole
(k <= 11), sampled windows of the dense table, sampled windows of the sparse
one, and (two gloo ranks on cuda:0) rank 0's slice of a merged dense and of
a merged sparse table."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import oracle
from conftest import REPO

BASES = 6_400_000


@pytest.mark.gpu
@pytest.mark.parametrize("k,world", [(11, 1), (13, 1), (17, 1), (12, 2), (17, 2)])
def test_plain_run_dumps_the_last_steps_outputs(k, world, tmp_path):
    out_dir = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", str(world), "--steps", "2", "--warmup", "1",
           "--k", str(k), "--bases", str(BASES), "--dump-outputs", out_dir]
    if world > 1:
        cmd += ["--dist-backend", "gloo"]
    env = {k_: v for k_, v in os.environ.items() if k_ not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == world and line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["value"] == pytest.approx(BASES / (line["ms_per_step"] * 1e-3))
    # a plain run: none of what --full adds
    assert not {"north_star", "weak_scaling", "cpu_baseline", "cpu_baseline_multicore", "verify"} & set(line)

    files = sorted(os.listdir(out_dir))
    assert files == (["counters.npy", "table.npy"] if k <= 11 else ["counters.npy", "table.npy", "table_index.npy"])
    arrays = {f: np.load(os.path.join(out_dir, f)) for f in files}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64_000_000

    data = oracle.synth(BASES, 2, 80)       # the bench's default seed and framing
    nb = 1 << (2 * k)
    wins = bench.dump_windows(0, (nb + world - 1) // world, nb)   # rank 0's slice of a sharded table
    assert len(wins) == bench.DUMP_WINDOWS or k <= 11
    if k <= 16:
        t_o, r_o, _ = oracle.count_dense(data, k, threads=oracle.host_threads())
        want = np.concatenate([t_o[s:s + n] for s, n in wins])
        index = np.concatenate([np.arange(s, s + n) for s, n in wins])
        distinct = int((t_o != 0).sum())
    else:
        keys, cnts, r_o = oracle.count_sparse(data, k, cap=1 << 23)
        sel = [(keys >= s) & (keys < s + n) for s, n in wins]
        want = np.concatenate([cnts[m] for m in sel])
        index = np.concatenate([keys[m] for m in sel])
        distinct = len(keys)
    assert np.array_equal(arrays["table.npy"], want.astype(np.float64))
    assert want.sum() > 0
    if k > 11:
        assert np.array_equal(arrays["table_index.npy"], index.astype(np.float64))
    assert arrays["counters.npy"].tolist() == [float(x) for x in (
        [r_o.windows, r_o.valid_bases] + list(r_o.base_count) + list(r_o.depth1)
        + [distinct, r_o.unknown_chars, r_o.scanned_bytes, r_o.hit_eof_byte, r_o.unterminated_header])]
