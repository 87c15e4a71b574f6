#!/usr/bin/env python3
"""The device ZPAQ cutter against the host routes.

Inputs generated in HBM (fill_splitmix), as bench.py does: 64 MiB
(configs[0]'s size) and 4 GiB of splitmix data, and 64 MiB of zeros (the
serial-in-rounds case).  Per input, after warm-up calls, the median wall time
of REPS blocking calls (the stream is idle before and after each):

  cut          sf_cut_device_zpaq alone, with its join rounds and re-cut bytes
  cut+hash     sf_index_device_zpaq (with and without blocks_hash)
  hash floor   sf_index_device_blocks alone over the same list
  host cut     sf_cut_fd with sf_zpaq_chunker_ops on 16 threads and on 1, over
               the same bytes in a page-cache file (64 MiB inputs)
  fd routes    sf_index_fd_zpaq against sf_index_fd_cut with the ops on 16
               threads, same file (64 MiB and 1 GiB)

One JSON line per measurement on stdout.

usage: python scripts/zpaq_device_bench.py [--reps 5] [--warmup 2] [--big-gib 4] [--zeros-mib 64]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from syncfast_amd import device, host  # noqa: E402

MIB = 1 << 20


def timed(fn, reps, warmup):
    out = None
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), out


def emit(**kw):
    print(json.dumps(kw), flush=True)


def rate(n, t):
    return round(n / t / 1e9, 2)


def device_side(name, data, reps, warmup):
    n = data.numel()
    med, best, (offs, sizes) = timed(lambda: device.cut_device_zpaq(data), reps, warmup)
    seg_len, segs, rounds, recut = device.zpaq_device_stats()
    emit(what="cut", input=name, bytes=n, blocks=offs.numel(), ms=round(med * 1e3, 3), best_ms=round(best * 1e3, 3),
         GBps=rate(n, med), segment=seg_len, segments=segs, join_rounds=rounds, recut_bytes=recut)
    for bh in (False, True):
        med, best, _ = timed(lambda: device.index_device_zpaq(data, blocks_hash=bh), reps, warmup)
        emit(what="cut+hash" + ("+blocks_hash" if bh else ""), input=name, bytes=n, ms=round(med * 1e3, 3),
             best_ms=round(best * 1e3, 3), GBps=rate(n, med))
    out = torch.empty((offs.numel(), 20), dtype=torch.uint8, device=data.device)
    med, best, _ = timed(lambda: device.index_device_blocks(data, offs, sizes, out=out, check_range=False), reps,
                         warmup)
    emit(what="hash floor (sf_index_device_blocks)", input=name, bytes=n, ms=round(med * 1e3, 3),
         best_ms=round(best * 1e3, 3), GBps=rate(n, med))
    return offs, sizes


def file_side(name, data, tmp, reps, warmup, cut_too):
    p = os.path.join(tmp, name)
    with open(p, "wb") as f:
        f.write(memoryview(data.cpu().numpy()))
    n = data.numel()
    ops = host.ZpaqOps()
    with open(p, "rb") as f:
        fd = f.fileno()
        if cut_too:
            for threads in (16, 1):
                med, best, (o, _z) = timed(lambda: host.cut_fd(fd, ops.address, threads), reps if threads > 1 else 1,
                                           warmup if threads > 1 else 0)
                emit(what=f"host cut, sf_cut_fd + zpaq ops, {threads} threads", input=name, bytes=n, blocks=int(o.size),
                     ms=round(med * 1e3, 3), best_ms=round(best * 1e3, 3), GBps=rate(n, med))
        med, best, (rows_h, bh_h) = timed(lambda: host.index_fd_cut(fd, ops.address, 16), reps, warmup)
        emit(what="sf_index_fd_cut + zpaq ops, 16 threads", input=name, bytes=n, ms=round(med * 1e3, 3),
             best_ms=round(best * 1e3, 3), GBps=rate(n, med))
        med, best, (rows_d, bh_d) = timed(lambda: host.index_fd_zpaq(fd), reps, warmup)
        emit(what="sf_index_fd_zpaq", input=name, bytes=n, ms=round(med * 1e3, 3), best_ms=round(best * 1e3, 3),
             GBps=rate(n, med), same_rows=bool(rows_d.tobytes() == rows_h.tobytes() and bh_d == bh_h))
    os.unlink(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--big-gib", type=int, default=4)
    ap.add_argument("--zeros-mib", type=int, default=64)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    emit(what="setup", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup)
    with tempfile.TemporaryDirectory(prefix="sf_zpaq_") as tmp:
        d64 = device.splitmix_tensor(64 * MIB, 0x5EED0000, dev)
        device_side("splitmix 64 MiB", d64, a.reps, a.warmup)
        file_side("splitmix 64 MiB", d64, tmp, a.reps, a.warmup, cut_too=True)
        del d64
        d1g = device.splitmix_tensor(1024 * MIB, 0x5EED0001, dev)
        file_side("splitmix 1 GiB", d1g, tmp, 3, 1, cut_too=False)
        del d1g
        if a.big_gib:
            big = device.splitmix_tensor(a.big_gib * 1024 * MIB, 0x5EED0002, dev)
            device_side(f"splitmix {a.big_gib} GiB", big, a.reps, a.warmup)
            del big
        if a.zeros_mib:
            z = torch.zeros(a.zeros_mib * MIB, dtype=torch.uint8, device=dev)
            t0 = time.perf_counter()
            offs, _s = device.cut_device_zpaq(z)
            dt = time.perf_counter() - t0
            seg_len, segs, rounds, recut = device.zpaq_device_stats()
            emit(what="cut", input=f"zeros {a.zeros_mib} MiB", bytes=z.numel(), blocks=offs.numel(),
                 ms=round(dt * 1e3, 3), GBps=rate(z.numel(), dt), segment=seg_len, segments=segs, join_rounds=rounds,
                 recut_bytes=recut)
            zh = bytes(z.numel())
            t0 = time.perf_counter()
            ho, _hz = host.zpaq_cut_buffer(zh)
            dt = time.perf_counter() - t0
            emit(what="host cut, sf_zpaq_cut_buffer, 1 thread", input=f"zeros {a.zeros_mib} MiB", bytes=len(zh),
                 blocks=int(ho.size), ms=round(dt * 1e3, 3), GBps=rate(len(zh), dt),
                 same_cuts=bool(ho.size == offs.numel() and (ho.astype("int64") == offs.cpu().numpy()).all()))


if __name__ == "__main__":
    main()
