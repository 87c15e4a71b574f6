"""GPU: a plain bench.py run and --dump-outputs.

A plain run (no --full) times its steps and prints the line with the side
legs' fields null; --dump-outputs DIR leaves the last timed step's digest
table (here a seeded sample of its rows: the table has more than
bench.DUMP_ROWS) as float32 .npy files, equal to the oracle's digests of the
same seeded input, and identical from run to run by construction (the rows
depend on the table's size alone)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_last_step_digests(gpu, tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    bs = 4096
    nblk = bench.DUMP_ROWS + 4097  # more rows than a dump keeps: the sampled form
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--ramp-s", "0", "--shard-gib", repr(nblk * bs / (1 << 30)), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=110, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0 and line["full"] is False
    assert line["config"]["blocks"] == nblk
    for leg in ("cpu_baseline", "config1", "e2e_host_buffer", "content_defined_list", "default_mode_files",
                "blocks_hash_host_ms"):
        assert line[leg] is None, leg
    assert sorted(os.listdir(out)) == ["digest_rows.npy", "digests.npy"]
    dig, rows = np.load(out / "digests.npy"), np.load(out / "digest_rows.npy")
    assert dig.dtype == np.float32 and rows.dtype == np.float64
    assert dig.nbytes + rows.nbytes <= bench.DUMP_MAX_BYTES
    keep = bench.dump_rows(nblk)
    assert np.array_equal(rows, keep) and dig.shape == (keep.size, 20)
    want = oracle.index_fixed_mt(oracle.splitmix_bytes(nblk * bs, bench.SEED), bs, 8)
    assert np.array_equal(dig, want[keep].astype(np.float32))
