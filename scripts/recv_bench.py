"""The receiving side's FILE_BLOCK run, timed (not part of bench.py).

Input: config 2's signature table -- the 2^21 digests of an 8 GiB splitmix
file at 4 KiB blocks, hashed here 1 GiB at a time -- sent as the default
mode would send it: one FILE_BLOCK message per block with a CDC-like size
(geometric, mean 8 KiB, capped at 32 KiB), the run built in HBM by
sf_wire_blocks_device.

Each figure is the median of --runs calls after --warmup calls, a host clock
around a call that ends in a stream synchronisation (every entry point timed
here is blocking):
  parse        sf_wire_parse_blocks_device alone, outputs allocated before
  receive      sf_receive_blocks_device against a set of the same 2^21 rows
  host         the same parse with SF_TEST_WIRE_PARSE_HOST=1: the run copied
               back through a pinned stage, parsed serially in C++, digests
               and sizes uploaded
  d2h, h2d     plain pinned copies of the run and of the parse's result, to
               take the copies out of `host`
  parser       wire.Parser (Python) on the first 2^16 messages

    python scripts/recv_bench.py [--log profiles/recv/recv_bench.log]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from syncfast_amd import _lib, device, wire  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--log2-messages", type=int, default=21)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("recv_bench.py needs a ROCm device: there is no CPU path to time")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = 1 << args.log2_messages
    per = min(n, 1 << 18)  # blocks of 4 KiB per 1 GiB piece
    table = torch.cat([device.index_device(device.splitmix_tensor(per * 4096, 0x5EED0000 + k, dev), 4096)
                       for k in range(n // per)])
    rng = np.random.default_rng(8)
    sizes_h = np.minimum(rng.geometric(1.0 / 8192, n), 32768).astype(np.uint32)
    sizes = torch.from_numpy(sizes_h.view(np.int32)).to(dev)
    run = wire.blocks_device(table, sizes)
    nb = run.numel()
    say(f"run: {n} messages, {nb} bytes ({nb / n:.2f} B per message), {torch.cuda.get_device_name(0)}")

    cap = n
    d_dig = torch.empty((cap, 20), dtype=torch.uint8, device=dev)
    d_sz = torch.empty(cap, dtype=torch.int32, device=dev)
    d_off = torch.empty(cap, dtype=torch.int64, device=dev)
    d_rows = torch.empty(cap, dtype=torch.int64, device=dev)
    cnt, consumed, end, stop = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
    s = torch.cuda.current_stream(dev).cuda_stream

    def parse():
        _lib.check(L.sf_wire_parse_blocks_device(run.data_ptr(), nb, d_dig.data_ptr(), d_sz.data_ptr(), cap,
                                                 ctypes.byref(cnt), ctypes.byref(consumed), ctypes.byref(stop), s))

    def report(name, t, extra=""):
        say(f"{name:8s} median {t[0]:9.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f})  {n / t[0] / 1e6:8.2f} G msg/s"
            f"  {nb / t[0] / 1e6:7.2f} GB/s of run{extra}")

    t_parse = timed(parse, args.runs, args.warmup)
    assert (cnt.value, consumed.value, stop.value) == (n, nb, 0) and wire.parse_stats()[2] == 0
    assert torch.equal(d_dig, table) and torch.equal(d_sz, sizes)
    report("parse", t_parse, f"  candidates {wire.parse_stats()[0]}")

    with device.BlockSet(table) as bset:
        def receive():
            _lib.check(L.sf_receive_blocks_device(bset._h, run.data_ptr(), nb, 0, d_dig.data_ptr(), d_sz.data_ptr(),
                                                  d_off.data_ptr(), d_rows.data_ptr(), cap, ctypes.byref(cnt),
                                                  ctypes.byref(consumed), ctypes.byref(stop), ctypes.byref(end), s))
        t_recv = timed(receive, args.runs, args.warmup)
        assert end.value == int(sizes_h.sum(dtype=np.uint64)) and int((d_rows < 0).sum()) == 0
        report("receive", t_recv)

    old = _lib.set_knob("SF_TEST_WIRE_PARSE_HOST", 1)
    try:
        t_host = timed(parse, args.runs, args.warmup)
        assert wire.parse_stats()[2] == 1 and torch.equal(d_dig, table) and torch.equal(d_sz, sizes)
    finally:
        _lib.set_knob("SF_TEST_WIRE_PARSE_HOST", old)
    report("host", t_host)

    pin_run = torch.empty(nb, dtype=torch.uint8, pin_memory=True)
    pin_res = torch.empty(n * 24, dtype=torch.uint8, pin_memory=True)
    d_res = torch.empty(n * 24, dtype=torch.uint8, device=dev)
    t_d2h = timed(lambda: pin_run.copy_(run, non_blocking=True), args.runs, args.warmup)
    t_h2d = timed(lambda: d_res.copy_(pin_res, non_blocking=True), args.runs, args.warmup)
    t_up = timed(lambda: run.copy_(pin_run, non_blocking=True), args.runs, args.warmup)
    say(f"d2h of the run {t_d2h[0]:.3f} ms, h2d of the run {t_up[0]:.3f} ms, h2d of digests + sizes ({n * 24} B) "
        f"{t_h2d[0]:.3f} ms")
    host_parse = t_host[0] - t_d2h[0] - t_h2d[0]
    say(f"host parse alone (host - d2h - h2d): {host_parse:.3f} ms = {n / host_parse / 1e3:.1f} M msg/s")
    say(f"bytes in host memory: h2d of the run + device parse {t_up[0] + t_parse[0]:.3f} ms  vs  host parse + h2d "
        f"of its result {host_parse + t_h2d[0]:.3f} ms")

    m = min(n, 1 << 16)
    head = bytes(pin_run[:int((33 + np.char.str_len(sizes_h[:m].astype(str))).sum())].numpy())
    t0 = time.perf_counter()
    msgs = wire.Parser().receive(head)
    t_py = (time.perf_counter() - t0) * 1e3
    assert len(msgs) == m
    say(f"parser   wire.Parser on {m} messages: {t_py:.1f} ms = {m / t_py / 1e3:.3f} M msg/s")

    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
