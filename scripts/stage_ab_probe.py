#!/usr/bin/env python3
"""A/B of the host routes between two built trees of this repository (the
figures of profiles/stage_driver/ab.md).

  stage_ab_probe.py routes TREE
      One JSON line: GB/s of each host entry point bench.py --full has no leg
      for, on TREE's library (a 1 GiB file, 512 files of 2 MiB, a 256 MiB
      pipe; best of 5 calls).  Run it once per tree, alternately.

  stage_ab_probe.py leg ROUNDS NAME=TREE [NAME=TREE ...]
      bench.py's config1.default_mode_e2e.hash_call_GB/s, as bench.py takes it
      (TREE/examples/build/sf_index -Z -T over the 64 MiB file three times in
      one process; of passes 2 and 3 the one with the smaller chunker + hash
      time; 64 MiB / its hash_s), one process per tree per round, the order of
      the trees rotated every round.  Naming one tree twice (parent=T
      control=T) gives the A/A control.  One JSON line: every figure per name,
      and per name against the first, the issue's rule over consecutive sets
      of three rounds (median >= first's median - (first's max - min)).
"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))  # oracle: input bytes only


def routes(tree):
    import threading

    import numpy as np
    import oracle
    root = os.path.abspath(tree)
    sys.path.insert(0, root)
    import torch
    from syncfast_amd import _lib, device, host, wire
    assert os.path.abspath(_lib.LIB_PATH).startswith(root), _lib.LIB_PATH
    d = tempfile.mkdtemp(prefix="sf_ab_")
    n = 1 << 30
    big = os.path.join(d, "big")
    oracle.splitmix_bytes(n, 0xAB).tofile(big)
    small = [os.path.join(d, f"s{i:04d}") for i in range(512)]
    for i, p in enumerate(small):
        oracle.splitmix_bytes(2 << 20, 0xAB00 + i).tofile(p)
    rng = np.random.default_rng(5)
    cuts = np.cumsum(np.minimum(rng.geometric(1 / 8192, n // 4096), 32768).astype(np.uint64))
    b = np.concatenate([[0], cuts[cuts < n], [n]]).astype(np.uint64)
    offs, sizes = b[:-1].copy(), np.diff(b).astype(np.uint32)
    buf = np.fromfile(big, np.uint8)

    def best(fn, nbytes, reps=5):
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return round(nbytes / min(t) / 1e9, 3)

    res = {"tree": tree}
    res["sf_index_file"] = best(lambda: host.index_file(big, 4096), n)
    res["sf_index_files"] = best(lambda: host.index_files(small, 4096), 512 * (2 << 20))
    with open(big, "rb") as f:
        st = host.file_stamp(f.fileno())
        res["sf_index_fd_fixed"] = best(lambda: host.index_fd_fixed(f.fileno(), 4096, st), n)
        res["sf_index_fd_blocks"] = best(lambda: host.index_fd_blocks(f.fileno(), offs, sizes, st), n)
        res["sf_index_fd_zpaq"] = best(lambda: host.index_fd_zpaq(f.fileno(), stamp=st), n, reps=3)
    fs = [open(p, "rb") for p in small]
    lists = [(np.arange(0, 2 << 20, 8192, dtype=np.uint64), np.full(256, 8192, np.uint32)) for _ in small]
    stamps = [host.file_stamp(f.fileno()) for f in fs]
    res["sf_index_fds_blocks"] = best(lambda: host.index_fds_blocks([f.fileno() for f in fs], lists, stamps),
                                      512 * (2 << 20))
    for f in fs:
        f.close()
    res["sf_index_buffer_blocks"] = best(lambda: host.index_buffer_blocks(buf, offs, sizes), n)

    def pipe_run():
        r, w = os.pipe()

        def wr():
            with os.fdopen(w, "wb") as o:
                o.write(memoryview(buf[:256 << 20]))
        th = threading.Thread(target=wr)
        th.start()
        host.index_fd(r, 4096)
        th.join()
        os.close(r)

    res["sf_index_fd_pipe"] = best(pipe_run, 256 << 20, reps=3)
    dev = torch.device("cuda:0")
    dig = device.index_device(torch.from_numpy(buf).to(dev), 4096)
    torch.cuda.synchronize()
    fd = os.open("/dev/null", os.O_WRONLY)
    nmsg = wire.file_blocks_to_fd(dig, 4096, n, fd)
    res["sf_wire_file_blocks_fd"] = best(lambda: wire.file_blocks_to_fd(dig, 4096, n, fd), nmsg)
    dsz = torch.from_numpy(sizes.view(np.int32)).to(dev)
    dig2 = dig[:1].repeat(len(sizes), 1).contiguous()
    nmsg2 = wire.blocks_to_fd(dig2, dsz, fd)
    res["sf_wire_blocks_fd"] = best(lambda: wire.blocks_to_fd(dig2, dsz, fd), nmsg2)
    os.close(fd)
    for p in small + [big]:
        os.unlink(p)
    os.rmdir(d)
    print(json.dumps(res), flush=True)


def leg(rounds, sides):
    import oracle
    n = 64 << 20
    d = tempfile.mkdtemp(prefix="sf_cfg1_")
    path = os.path.join(d, "file64m")
    oracle.splitmix_bytes(n, 0x5EED0000).tofile(path)
    names = [s.split("=", 1)[0] for s in sides]
    trees = dict(s.split("=", 1) for s in sides)
    got = {k: [] for k in names}
    try:
        for r in range(rounds):
            for k in names[r % len(names):] + names[:r % len(names)]:
                exe = os.path.join(trees[k], "examples", "build", "sf_index")
                p = subprocess.run([exe, "-Z", "-T", path, path, path], capture_output=True, text=True, timeout=120)
                if p.returncode != 0:
                    sys.exit(f"{k}: sf_index failed ({p.returncode}): {p.stderr[-300:]}")
                times = [json.loads(ln) for ln in p.stderr.splitlines() if ln.startswith("{")]
                best = min(times[1:], key=lambda t: t["chunk_s"] + t["hash_s"])
                got[k].append(round(n / best["hash_s"] / 1e9, 3))
    finally:
        os.unlink(path)
        os.rmdir(d)
    ref = names[0]
    out = {"rounds": rounds, "order": "rotated every round", "hash_call_GB/s": got, "median": {}, "rule": {}}
    for k in names:
        out["median"][k] = round(statistics.median(got[k]), 3)
        if k == ref:
            continue
        sets = []
        for i in range(0, rounds - rounds % 3, 3):
            p, q = got[ref][i:i + 3], got[k][i:i + 3]
            sets.append(statistics.median(q) >= statistics.median(p) - (max(p) - min(p)))
        out["rule"][k] = {"sets": len(sets), "missed": sets.count(False)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "routes":
        routes(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "leg":
        leg(int(sys.argv[2]), sys.argv[3:])
    else:
        sys.exit(__doc__)
