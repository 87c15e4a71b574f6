"""The block copy kernel and the image's way to a descriptor, timed
(not part of bench.py).

Each figure is the median of --runs blocking calls after --warmup, a host
clock around call + synchronize, one process.  The yardstick, a contiguous
device-to-device copy of the same total bytes (dst.copy_(src) in torch), is
timed in the same loop, alternating with the call under test.

  A        2^20 jobs of 4 KiB, everything 16-byte aligned, destinations back to
           back: the kernel with its shifts and edges idle
  B        block_data_bench.py's CDC-like list (geometric sizes, mean 8 KiB,
           cap 32 KiB, --mib of payload); the source offsets are the payload
           offsets of the honest BLOCK_DATA run of that list (a header of 34 to
           38 bytes and an end byte between two payloads: arbitrary alignment),
           destinations back to back
  B x2     the same list with each job fanned out to two destinations
  write    sf_write_device_fd of --write-mib to a file in --dir, beside a
           plain pinned device-to-host copy of the same bytes

    python scripts/copy_blocks_bench.py [--log profiles/copy_blocks/copy_blocks.log]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from syncfast_amd import _lib, device  # noqa: E402


def timed_pair(fn, yard, runs, warmup):
    """Medians (ms) of fn and of yard, alternating, each call blocking."""
    a, b = [], []
    for k in range(warmup + runs):
        for f, out in ((yard, b), (fn, a)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if k >= warmup:
                out.append((time.perf_counter() - t0) * 1e3)
    return (statistics.median(a), min(a), max(a)), (statistics.median(b), min(b), max(b))


def cdc_sizes(total_bytes, seed):
    """block_data_bench.py's list."""
    rng = np.random.default_rng(seed)
    sizes, left = [], total_bytes
    while left:
        for s in np.minimum(rng.geometric(1.0 / 8192, 4096), 32768):
            s = int(min(s, left))
            sizes.append(s)
            left -= s
            if not left:
                break
    return np.array(sizes, np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--mib", type=int, default=4096)
    ap.add_argument("--write-mib", type=int, default=4096)
    ap.add_argument("--dir", default=None, help="where the written file goes (default: the temp directory)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("copy_blocks_bench.py needs a ROCm device: there is no CPU path to time")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name(0)}, T = {device.copy_stats()[0]}")
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run_shape(name, src, dst, so, do, sz, base=None):
        so_t, do_t = (torch.from_numpy(v.view(np.int64)).to(dev) for v in (so, do))
        sz_t = torch.from_numpy(sz.astype(np.uint32).view(np.int32)).to(dev)
        total = int(sz.sum(dtype=np.uint64))
        ysrc, ydst = src[:total], dst[:total]
        status = torch.zeros(1, dtype=torch.int32, device=dev)

        def call():
            _lib.check(L.sf_copy_blocks_device(src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel(),
                                               so_t.data_ptr(), do_t.data_ptr(), sz_t.data_ptr(), None, len(sz),
                                               status.data_ptr(), stream))
        t, y = timed_pair(call, lambda: ydst.copy_(ysrc), args.runs, args.warmup)
        assert int(status.item()) == 0
        stats = device.copy_stats()
        # exact: a sample of the jobs, and the ends
        pick = np.unique(np.concatenate([np.arange(min(len(sz), 64)), np.arange(max(len(sz) - 64, 0), len(sz)),
                                         np.random.default_rng(1).integers(0, len(sz), 512)]))
        for i in pick:
            s, d, n = int(so[i]), int(do[i]), int(sz[i])
            assert torch.equal(dst[d:d + n], src[s:s + n]), (name, i)
        gbs = total / t[0] / 1e6
        say(f"{name:5s} {len(sz):8d} jobs {total:11d} B  copy {t[0]:8.3f} ms (min {t[1]:.3f}, max {t[2]:.3f}) = "
            f"{gbs:8.1f} GB/s copied | torch copy_ {y[0]:8.3f} ms (min {y[1]:.3f}, max {y[2]:.3f}) = "
            f"{total / y[0] / 1e6:8.1f} GB/s | ratio {y[0] / t[0]:.3f} | tiles {stats[2]}"
            + (f" | vs {base[0]}: {gbs / base[1]:.3f}" if base else ""))
        return gbs, t[0]

    # A
    nA = 1 << 20
    szA = np.full(nA, 4096, np.uint64)
    offA = np.arange(nA, dtype=np.uint64) * 4096
    src = device.splitmix_tensor(nA * 4096, 5, dev)
    dst = torch.zeros(nA * 4096, dtype=torch.uint8, device=dev)
    gA, _ = run_shape("A", src, dst, offA, offA, szA)
    del src, dst

    # B
    sz = cdc_sizes(args.mib << 20, 9)
    digits = np.char.str_len(sz.astype(str)).astype(np.uint64)
    head = 33 + digits  # "BLOCK_DATA\n" + 20 + "\n" + the length field + "\n"
    msg = head + sz + 1
    start = np.concatenate([[0], np.cumsum(msg)[:-1]]).astype(np.uint64)
    so = start + head
    do = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint64)
    run_len, payload = int(msg.sum()), int(sz.sum())
    src = device.splitmix_tensor(max(run_len, 2 * payload), 6, dev)  # (the x2 yardstick reads 2 x payload)
    dst = torch.zeros(2 * payload, dtype=torch.uint8, device=dev)
    say(f"B: {len(sz)} messages, run {run_len} B, payload {payload} B, source offsets mod 16 spread "
        f"{np.bincount((so % 16).astype(np.int64), minlength=16).min()}..{np.bincount((so % 16).astype(np.int64), minlength=16).max()}")
    gB, tB = run_shape("B", src, dst[:payload], so, do, sz, ("A", gA))
    say(f"B against parse + verify of the same run (4.04 ms on record for 4 GiB): {tB / 4.04:.2f}x its time")
    so2 = np.concatenate([so, so])
    do2 = np.concatenate([do, do + np.uint64(payload)])
    sz2 = np.concatenate([sz, sz])
    run_shape("B x2", src, dst, so2, do2, sz2, ("B", gB))
    del src, dst

    # write
    n = args.write_mib << 20
    t = device.splitmix_tensor(n, 7, dev)
    pin = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    with tempfile.NamedTemporaryFile(dir=args.dir) as f:
        fd = f.fileno()

        def write():
            assert device.write_to_fd(t, fd, 0) == n
        tw, td = timed_pair(write, lambda: pin.copy_(t, non_blocking=True), args.runs, args.warmup)
        os.lseek(fd, 0, os.SEEK_SET)
        tail = os.pread(fd, 1 << 20, n - (1 << 20))
        assert tail == bytes(t[n - (1 << 20):].cpu().numpy()) and os.fstat(fd).st_size == n
    say(f"write {n} B to {args.dir or tempfile.gettempdir()}: {tw[0]:.1f} ms (min {tw[1]:.1f}, max {tw[2]:.1f}) = "
        f"{n / tw[0] / 1e6:.2f} GB/s | pinned D2H alone {td[0]:.1f} ms = {n / td[0] / 1e6:.2f} GB/s")

    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
