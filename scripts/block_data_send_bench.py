"""The BLOCK_DATA writer and the GET_BLOCK answer, timed (not
part of bench.py).

The workload is copy_blocks_bench.py's list B: geometric block sizes, mean
8 KiB, cap 32 KiB, --mib of payload (535,012 blocks at 4 GiB), the blocks back
to back at byte offsets of one source file in HBM.  In one process, each figure
the median of --runs blocking calls after --warmup (a host clock around call +
synchronize), the five calls alternating inside one loop whose order rotates:

  build      sf_wire_block_data_device over the list (+ freeing the run)
  copy       sf_copy_blocks_device of the same jobs to the payload offsets of
             that run, in a buffer of the run's size: the call the build makes
             for its payloads, alone -- unchanged by this writer, the yardstick
  torch      dst.copy_(src) of the payload bytes, contiguous
  serve      sf_serve_get_blocks_device over the GET_BLOCK run of the same
             blocks, in order: parse, lookup, jobs and the build
  serve0     the same run with its first digest unknown: parse, lookup and
             jobs over every request, and an empty run

    python scripts/block_data_send_bench.py [--log profiles/block_data_send/block_data_send.log]
    ... --trace    three builds and nothing else (for a kernel trace)
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from copy_blocks_bench import cdc_sizes  # noqa: E402
from syncfast_amd import _lib, device, wire  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--mib", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("block_data_send_bench.py needs a ROCm device: there is no CPU path to time")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sz = cdc_sizes(args.mib << 20, 9)
    n, payload = len(sz), int(sz.sum())
    so = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint64)
    head = 33 + np.char.str_len(sz.astype(str)).astype(np.uint64)
    msg = head + sz + 1
    do = (np.concatenate([[0], np.cumsum(msg)[:-1]]).astype(np.uint64) + head)  # payload offsets in the run
    run_len = int(msg.sum())
    labels = np.random.default_rng(3).integers(0, 256, (n, 20), dtype=np.uint8)
    say(f"{torch.cuda.get_device_name(0)}: {n} blocks, payload {payload} B, run {run_len} B "
        f"(headers and end bytes {100.0 * (run_len - payload) / run_len:.2f} %)")

    src = device.splitmix_tensor(payload, 6, dev)
    so_t = torch.from_numpy(so.view(np.int64)).to(dev)
    do_t = torch.from_numpy(do.view(np.int64)).to(dev)
    sz_t = torch.from_numpy(sz.astype(np.uint32).view(np.int32)).to(dev)
    dig_t = torch.from_numpy(labels).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def build():
        h = ctypes.c_void_p()
        _lib.check(L.sf_wire_block_data_device(src.data_ptr(), payload, dig_t.data_ptr(), so_t.data_ptr(),
                                               sz_t.data_ptr(), n, ctypes.byref(h), stream))
        return h

    def free(h):
        _lib.check(L.sf_wire_run_free(h, stream))

    if args.trace:
        for _ in range(3):
            free(build())
        torch.cuda.synchronize()
        return

    # exact, before anything is timed: the ends of the run and a sample of its messages
    run = wire.BlockDataRun(build(), dev)
    assert (run.nbytes, run.n_messages) == (run_len, n)
    start = do - head
    for i in np.unique(np.concatenate([np.arange(16), np.arange(n - 16, n), np.random.default_rng(1).integers(0, n, 96)])):
        want = wire.write_message("BlockData", labels[i].tobytes(), bytes(src[int(so[i]):int(so[i] + sz[i])].cpu().numpy()))
        assert run.bytes(int(start[i]), len(want)) == want, i
    run.close()

    dst = torch.empty(run_len, dtype=torch.uint8, device=dev)
    ysrc, ydst = src, dst[:payload]
    bset = device.BlockSet(dig_t)
    tag = np.frombuffer(b"GET_BLOCK\n", np.uint8)
    req = np.concatenate([np.tile(tag, (n, 1)), labels, np.full((n, 1), 10, np.uint8)], axis=1).reshape(-1)
    req_t = torch.from_numpy(req).to(dev)
    req0 = req.copy()
    req0[10:30] ^= 0xFF  # request 0 names a block nobody holds
    req0_t = torch.from_numpy(req0).to(dev)
    outs = [ctypes.c_uint64(0) for _ in range(3)] + [ctypes.c_int(0)]
    seen = {}

    def serve(r, name):
        h = ctypes.c_void_p()
        _lib.check(L.sf_serve_get_blocks_device(bset._h, so_t.data_ptr(), sz_t.data_ptr(), src.data_ptr(), payload,
                                                r.data_ptr(), r.numel(), ctypes.byref(h),
                                                *(ctypes.byref(v) for v in outs), stream))
        seen[name] = tuple(v.value for v in outs)
        free(h)

    calls = {
        "torch": lambda: ydst.copy_(ysrc),
        "copy": lambda: _lib.check(L.sf_copy_blocks_device(src.data_ptr(), payload, dst.data_ptr(), run_len,
                                                           so_t.data_ptr(), do_t.data_ptr(), sz_t.data_ptr(), None, n,
                                                           None, stream)),
        "build": lambda: free(build()),
        "serve": lambda: serve(req_t, "serve"),
        "serve0": lambda: serve(req0_t, "serve0"),
    }
    times = {k: [] for k in calls}
    names = list(calls)
    for k in range(args.warmup + args.runs):
        # what ran just before a call, and into which buffer, moves its time by
        # a tenth: the order rotates, so every call follows every other one
        for name in names[k % len(names):] + names[:k % len(names)]:
            f = calls[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if k >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    assert seen["serve"] == (n, n, 31 * n, 0) and seen["serve0"] == (n, 0, 31 * n, 0), seen
    med = {k: statistics.median(v) for k, v in times.items()}
    for name, what, nbytes in (("torch", "contiguous copy of the payload", payload),
                               ("copy", "sf_copy_blocks_device, the payloads alone", payload),
                               ("build", "sf_wire_block_data_device", run_len),
                               ("serve", "sf_serve_get_blocks_device", run_len),
                               ("serve0", "the same, first digest unknown: no build", 31 * n)):
        v = times[name]
        say(f"{name:6s} {med[name]:8.3f} ms (min {min(v):.3f}, max {max(v):.3f}) = {nbytes / med[name] / 1e6:8.1f} GB/s "
            f"of {nbytes} B  [{what}]")
    say(f"build / copy {med['build'] / med['copy']:.3f}x the bare copy's time (+{med['build'] - med['copy']:.3f} ms); "
        f"copy / torch {med['copy'] / med['torch']:.3f}; serve - build {med['serve'] - med['build']:.3f} ms; "
        f"request side alone {med['serve0']:.3f} ms = {n / med['serve0'] / 1e3:.1f} M requests/s")
    bset.close()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
