"""A received BLOCK_DATA run parsed and verified on the device, timed
(not part of bench.py).

Input: a CDC-like block list (geometric sizes, mean 8 KiB, capped at 32 KiB)
of seeded random payloads, --mib of them (256 and 4096 for the table in
DESIGN.md), each sent as the source sends it: wire.write_message("BlockData",
sha1(payload), payload), built on the host and uploaded.

Each figure is the median of --runs calls after --warmup calls, a host clock
around a call that ends in a stream synchronisation (every entry point timed
here is blocking, or is followed by one):
  parse        sf_receive_block_data_device with d_ok = NULL: nothing hashed
  verify       the same with d_ok: parse, hash every payload in place, compare
  floor        sf_index_device_blocks alone over the same offsets and sizes:
               what the verify pass cannot beat
  buffer       sf_receive_block_data_buffer from the run in host memory
               (upload through the pinned stages included)
  host         parse_data_run + sf_sha1_host per payload on one thread
               (scripts/block_data_host.cpp, built here with g++)

    python scripts/block_data_bench.py --mib 256 [--log profiles/block_data/block_data_256.log]
"""
import argparse
import ctypes
import hashlib
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from syncfast_amd import _lib, host, wire  # noqa: E402


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def build_run(total_bytes, seed):
    """(run as a pinned uint8 tensor, payload sizes) of messages whose
    payloads add up to total_bytes."""
    rng = np.random.default_rng(seed)
    sizes = []
    left = total_bytes
    while left:
        batch = np.minimum(rng.geometric(1.0 / 8192, 4096), 32768)
        for s in batch:
            s = int(min(s, left))
            sizes.append(s)
            left -= s
            if not left:
                break
    sizes = np.array(sizes, np.uint32)
    room = int(sizes.sum(dtype=np.uint64)) + 48 * len(sizes)
    run = torch.empty(room, dtype=torch.uint8, pin_memory=True)
    view = run.numpy()
    at, i = 0, 0
    while i < len(sizes):  # payload bytes 64 MiB or so at a time
        j, piece = i, 0
        while j < len(sizes) and piece < (64 << 20):
            piece += int(sizes[j])
            j += 1
        data = rng.integers(0, 256, piece, dtype=np.uint8).tobytes()
        p = 0
        for s in sizes[i:j]:
            payload = data[p:p + int(s)]
            m = wire.write_message("BlockData", hashlib.sha1(payload).digest(), payload)
            view[at:at + len(m)] = np.frombuffer(m, np.uint8)
            at += len(m)
            p += int(s)
        i = j
    return run[:at], sizes


def host_baseline():
    """block_data_host(run, n, &n_msgs, &n_bad) of scripts/block_data_host.cpp."""
    tmp = tempfile.mkdtemp(prefix="block_data_host_")
    so = os.path.join(tmp, "block_data_host.so")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "scripts", "block_data_host.cpp"),
                    "-o", so, "-L" + libdir, "-lsyncfast_amd", "-Wl,-rpath," + libdir], check=True)
    fn = ctypes.CDLL(so).block_data_host
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("block_data_bench.py needs a ROCm device: there is no CPU path to time")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t0 = time.perf_counter()
    pin_run, sizes_h = build_run(args.mib << 20, 9)
    n, nb = len(sizes_h), pin_run.numel()
    payload = int(sizes_h.sum(dtype=np.uint64))
    run = pin_run.to(dev)
    say(f"run: {n} messages, {nb} bytes, {payload} payload bytes ({payload / n:.0f} B mean), built in "
        f"{time.perf_counter() - t0:.1f} s, {torch.cuda.get_device_name(0)}")

    cap = n
    d_dig = torch.empty((cap, 20), dtype=torch.uint8, device=dev)
    d_sz = torch.empty(cap, dtype=torch.int32, device=dev)
    d_off = torch.empty(cap, dtype=torch.int64, device=dev)
    d_ok = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_comp = torch.empty((cap, 20), dtype=torch.uint8, device=dev)
    cnt, consumed, stop = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
    need, bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    refs = tuple(ctypes.byref(v) for v in (cnt, consumed, stop, need, bad))
    s = torch.cuda.current_stream(dev).cuda_stream

    def receive(ok):
        _lib.check(L.sf_receive_block_data_device(run.data_ptr(), nb, d_dig.data_ptr(), d_sz.data_ptr(),
                                                  d_off.data_ptr(), ok, cap, *refs, s))

    def report(name, t, extra=""):
        say(f"{name:7s} median {t[0]:10.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f})  {nb / t[0] / 1e6:9.2f} GB/s of run"
            f"{extra}")

    t_parse = timed(lambda: receive(None), args.runs, args.warmup)
    stats = wire.block_data_stats()
    assert (cnt.value, consumed.value, stop.value, bad.value) == (n, nb, 0, 0) and stats[2] == 0
    assert np.array_equal(d_sz.cpu().numpy().view(np.uint32), sizes_h)
    report("parse", t_parse, f"  candidates {stats[0]}, walk {stats[2]}")

    t_verify = timed(lambda: receive(d_ok.data_ptr()), args.runs, args.warmup)
    assert (cnt.value, bad.value) == (n, 0) and int(d_ok.sum()) == n
    report("verify", t_verify)

    def floor():
        _lib.check(L.sf_index_device_blocks(run.data_ptr(), nb, d_off.data_ptr(), d_sz.data_ptr(), n,
                                            d_comp.data_ptr(), None, s))
    t_floor = timed(floor, args.runs, args.warmup)
    assert torch.equal(d_comp, d_dig)
    report("floor", t_floor, f"  verify - floor - parse = {t_verify[0] - t_floor[0] - t_parse[0]:+.3f} ms")

    rows, p_rows = host._rows(n)
    ok_h = np.zeros(n, np.uint8)
    wire_ptr = pin_run.data_ptr()

    def buffer():
        _lib.check(L.sf_receive_block_data_buffer(wire_ptr, nb, p_rows, ok_h.ctypes.data, n, *refs))
    t_buf = timed(buffer, args.runs, args.warmup)
    assert (cnt.value, bad.value) == (n, 0) and int(ok_h.sum()) == n
    assert np.array_equal(rows["size"][:n], sizes_h)
    report("buffer", t_buf)

    fn = host_baseline()
    hn, hbad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    t_host = timed(lambda: fn(wire_ptr, nb, ctypes.byref(hn), ctypes.byref(hbad)), args.runs, args.warmup)
    assert (hn.value, hbad.value) == (n, 0)
    report("host", t_host, f"  one thread; verify is {t_host[0] / t_verify[0]:.0f}x, buffer {t_host[0] / t_buf[0]:.1f}x")

    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
