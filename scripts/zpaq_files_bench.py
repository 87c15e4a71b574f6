#!/usr/bin/env python3
"""sf_index_fds_zpaq (every file read once, cut on the device a stage at a
time) against the route index_path takes today for the reference's default
mode: the files cut by sf_zpaq_chunker_ops on 16 host threads, then
sf_index_fds_blocks, batch by batch.

Sets: the two file shapes of scripts/recv_files_bench.py -- 1,024 files of
8 MiB and 42,111 files of 0-200 KiB -- filled from a seed, written to a
temporary directory and read once before timing (page cache).  Real parameters
13 / 32768.  Per set and batch size (--stage-mib, default 256 1024 2048): the
two routes alternate in one process after a warm-up pass each; median, min and
max of --reps passes; rows and blocks_hash values compared for equality.

A batch is what Index._index_batched_fds makes: about `stage` bytes and at
most a quarter of the descriptor limit (this process raises its soft limit to
the hard one first) or 4096 files.  In the host route the 16-thread pool cuts
batch k + 1 while batch k is hashed, as there.

Also: the join launches per call on every set and on a text-like tree (this
checkout); one mixed set with a 32 MiB file of zeros, with max_rounds 8 and 0;
one 64 MiB file alone; one pass per set with SF_TRACE on (phase times on
stderr).  One JSON line per measurement on stdout.

usage: python scripts/zpaq_files_bench.py [--reps 5] [--sets large small] [--stage-mib 256 1024 2048]
                                          [--extras text mixed one] [--scale 1.0]"""
import argparse
import json
import os
import resource
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from syncfast_amd import _lib, device, host  # noqa: E402
from syncfast_amd.index import ZpaqChunker, _cut_stamped, _offsets  # noqa: E402

MIB = 1 << 20
SHAPES = {"small": (42111, None), "large": (1024, 8 << 20)}  # scripts/recv_files_bench.py's
THREADS = 16


def emit(**kw):
    print(json.dumps(kw), flush=True)


def write_set(root, n_files, fixed, seed):
    rng = np.random.default_rng(seed)
    sizes = np.full(n_files, fixed) if fixed else rng.integers(0, 200 * 1024 + 1, n_files)
    paths = []
    for k, size in enumerate(sizes.tolist()):
        d = os.path.join(root, f"d{k // 1000}")
        os.makedirs(d, exist_ok=True)
        p = os.path.join(d, f"f{k}")
        with open(p, "wb") as f:
            f.write(rng.bytes(int(size)))
        paths.append(p)
    return paths, int(sizes.sum())


def batches(paths, stage, max_files):
    out, cur, nbytes = [], [], 0
    for p in paths:
        cur.append(p)
        nbytes += os.path.getsize(p)
        if nbytes >= stage or len(cur) >= max_files:
            out.append(cur)
            cur, nbytes = [], 0
    if cur:
        out.append(cur)
    return out


def device_route(bs, stage, max_rounds):
    """Every batch through one sf_index_fds_zpaq call.  Returns the per-batch
    results and (join launches, files finished on the host, calls)."""
    res, launches, on_host = [], 0, 0
    for b in bs:
        fs = [open(p, "rb") for p in b]
        try:
            stamps = [host.file_stamp(f.fileno()) for f in fs]
            r = host.index_fds_zpaq([f.fileno() for f in fs], 13, 32768, stamps, max_rounds, stage)
        finally:
            for f in fs:
                f.close()
        st = device.zpaq_files_stats()
        launches, on_host = max(launches, st[2]), on_host + st[5]
        assert not r[3].any()
        res.append(r)
    return res, (launches, on_host, len(bs))


def host_route(bs, stage, ch, pool):
    """Today's route: the files of a batch cut on the pool, then one
    sf_index_fds_blocks call; batch k + 1 is cut while batch k is hashed."""
    def start(b):
        fs = [open(p, "rb") for p in b]
        stamps = [host.file_stamp(f.fileno()) for f in fs]
        return fs, stamps, [pool.submit(_cut_stamped, ch.fn, f, s) for f, s in zip(fs, stamps)]
    res = []
    nxt = start(bs[0])
    for k in range(len(bs)):
        fs, stamps, futs = nxt
        nxt = start(bs[k + 1]) if k + 1 < len(bs) else None
        try:
            cuts = [x.result() for x in futs]
            lists = [(_offsets(c), np.asarray(c, np.uint32)) for c in cuts]
            r = host.index_fds_blocks([f.fileno() for f in fs], lists, stamps, stage_bytes=stage)
        finally:
            for f in fs:
                f.close()
        assert not r[3].any()
        res.append(r)
    return res


def same(a, b):
    return len(a) == len(b) and all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
                                    and x[2].tobytes() == y[2].tobytes() for x, y in zip(a, b))


def spread(ts):
    return dict(ms=round(statistics.median(ts) * 1e3, 1), min_ms=round(min(ts) * 1e3, 1), max_ms=round(max(ts) * 1e3, 1))


def compare(name, paths, nbytes, stage, max_files, reps, ch, pool):
    bs = batches(paths, stage, max_files)
    a, info = device_route(bs, stage, host.ZPAQ_MAX_ROUNDS)  # warm-up passes, and the comparison
    b = host_route(bs, stage, ch, pool)
    equal = same(a, b)
    del a, b
    td, th = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        device_route(bs, stage, host.ZPAQ_MAX_ROUNDS)
        td.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        host_route(bs, stage, ch, pool)
        th.append(time.perf_counter() - t0)
    emit(what="sf_index_fds_zpaq", set=name, files=len(paths), bytes=nbytes, stage_mib=stage // MIB, calls=len(bs),
         GBps=round(nbytes / statistics.median(td) / 1e9, 2), **spread(td), join_launches_max=info[0],
         finished_on_host=info[1], same_rows_and_hashes=equal)
    emit(what="host cut on 16 threads + sf_index_fds_blocks", set=name, files=len(paths), bytes=nbytes,
         stage_mib=stage // MIB, calls=len(bs), GBps=round(nbytes / statistics.median(th) / 1e9, 2), **spread(th))


def launches_of(name, paths, max_files):
    """The join launches of the set with no cap: the largest of any call, each
    call one stage (batches of 256 MiB in stages of 1 GiB)."""
    bs = batches(paths, 256 * MIB, max_files)
    _r, info = device_route(bs, 1024 * MIB, 0)
    emit(what="join launches, no cap", set=name, files=len(paths), calls=info[2], join_launches_max=info[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sets", nargs="*", default=["large", "small"])
    ap.add_argument("--stage-mib", type=int, nargs="*", default=[256, 1024, 2048])
    ap.add_argument("--extras", nargs="*", default=["text", "mixed", "one"], help="text mixed one (none: --extras)")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each set's files (a short run)")
    a = ap.parse_args()
    soft, hard = resource.getrlimit(resource.RLIMIT_NOFILE)
    want = hard if hard != resource.RLIM_INFINITY else 65536
    if soft < want:
        resource.setrlimit(resource.RLIMIT_NOFILE, (min(want, 65536), hard))
    soft = resource.getrlimit(resource.RLIMIT_NOFILE)[0]
    max_files = max(16, min(4096, soft // 4))
    import torch
    emit(what="setup", device=torch.cuda.get_device_name(0), reps=a.reps, nofile=soft, max_files=max_files,
         max_rounds=host.ZPAQ_MAX_ROUNDS, scale=a.scale)
    ch = ZpaqChunker()
    with tempfile.TemporaryDirectory(prefix="sf_zpaq_files_") as tmp, ThreadPoolExecutor(max_workers=THREADS) as pool:
        for name in a.sets:
            n_files, fixed = SHAPES[name]
            root = os.path.join(tmp, name)
            paths, nbytes = write_set(root, max(1, int(n_files * a.scale)), fixed, 42)
            for stage in a.stage_mib:
                compare(name, paths, nbytes, stage * MIB, max_files, a.reps, ch, pool)
            launches_of(name, paths, max_files)
            _lib.set_knob("SF_TRACE", 1)  # one pass with the phase times on stderr
            try:
                for stage in a.stage_mib:
                    device_route(batches(paths, stage * MIB, max_files), stage * MIB, host.ZPAQ_MAX_ROUNDS)
            finally:
                _lib.set_knob("SF_TRACE", 0)
            for p in paths:
                os.unlink(p)
        if "text" in a.extras:  # a text-like tree: this checkout's own files
            tops = ("include", "syncfast_amd", "tests", "scripts", "oracle", "examples", "profiles")
            text = [os.path.join(ROOT, f) for f in sorted(os.listdir(ROOT)) if os.path.isfile(os.path.join(ROOT, f))]
            for top in tops:
                text += [os.path.join(d, f) for d, _s, fs in os.walk(os.path.join(ROOT, top)) for f in sorted(fs)
                         if "/." not in d[len(ROOT):] and "/build" not in d[len(ROOT):] and "/lib" not in d[len(ROOT):]]
            text = [p for p in text if not os.path.islink(p) and not p.endswith((".so", ".o", ".pyc"))]
            emit(what="text-like tree", files=len(text), bytes=sum(os.path.getsize(p) for p in text))
            launches_of("this checkout (text-like)", text, max_files)
        if "mixed" in a.extras:
            mixed(tmp, max_files, a.reps)
        if "one" in a.extras:
            one_file(tmp, a.reps, ch)


def mixed(tmp, max_files, reps):
    # what the cap buys: 256 files of 1 MiB and one 32 MiB file of zeros in one call
    root = os.path.join(tmp, "mixed")
    paths, nbytes = write_set(root, 256, MIB, 43)
    z = os.path.join(root, "zeros")
    with open(z, "wb") as f:
        f.write(bytes(32 * MIB))
    paths.insert(100, z)
    nbytes += 32 * MIB
    ref = None
    for cap in (host.ZPAQ_MAX_ROUNDS, 0):
        ts = []
        for _ in range(2 if cap == 0 else reps + 1):
            t0 = time.perf_counter()
            r, info = device_route([paths], 512 * MIB, cap)
            ts.append(time.perf_counter() - t0)
        ref = ref or r
        emit(what="mixed set: 256 x 1 MiB random and 32 MiB of zeros, one call", max_rounds=cap, bytes=nbytes,
             join_launches=info[0], finished_on_host=info[1], same_rows_and_hashes=same(r, ref),
             **spread(ts[1:]))


def one_file(tmp, reps, ch):
    # one 64 MiB file alone: the batch route has one file's lanes only
    one = os.path.join(tmp, "one64")
    with open(one, "wb") as f:
        f.write(np.random.default_rng(44).bytes(64 * MIB))
    td, th = [], []
    with open(one, "rb") as f:
        for k in range(reps + 1):
            t0 = time.perf_counter()
            rd = host.index_fds_zpaq([f.fileno()], stage_bytes=256 * MIB)
            td.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            rh = host.index_fd_cut(f.fileno(), ch.ops, THREADS)
            th.append(time.perf_counter() - t0)
    emit(what="one 64 MiB file: sf_index_fds_zpaq", bytes=64 * MIB, GBps=round(64 * MIB / statistics.median(td[1:]) / 1e9, 2),
         **spread(td[1:]), same_rows=bool(rd[0].tobytes() == rh[0].tobytes() and bytes(rd[2][0]) == rh[1]))
    emit(what="one 64 MiB file: sf_index_fd_cut, 16 threads", bytes=64 * MIB,
         GBps=round(64 * MIB / statistics.median(th[1:]) / 1e9, 2), **spread(th[1:]))


if __name__ == "__main__":
    main()
