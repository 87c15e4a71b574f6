"""A whole GetFiles stream received in one call, timed against one call per
file (not part of bench.py).

Input: a seeded session stream as the source answers a destination that asked
for every file at once -- FILE_START, the file's FILE_BLOCKs, FILE_END, back
to back.  Two shapes:
  small   42,111 files (names d<k>/f<j>), sizes uniform in 0-200 KiB
  large   1,024 files of 8 MiB (config 3's shape)
Block sizes are CDC-like (geometric, mean 8 KiB, capped at 32 KiB), digests
random; half of them are rows of the block set.  The stream is built once on
the host and kept in HBM.

Each figure is a host clock around blocking calls, the two routes alternating
in one process, the median of --runs after --warmup:
  files     ONE sf_receive_files_device over the whole buffer
  per-file  the route that existed before it: one sf_receive_blocks_device
            per file on the same set, into the same preallocated outputs.
            The host must first find every FILE_START and FILE_END (the
            Python parser's work); that search is done before the clock
            starts and is NOT in the figure.
  host      `files` with SF_TEST_WIRE_PARSE_HOST=1: the cost of the fallback
            (the buffer copied back, parsed serially in C++, the rows
            uploaded), one run.
`files` and `per-file` must give the same digests, sizes, offsets and rows.

    python scripts/recv_files_bench.py [--shape small|large|both] [--only files]
                                       [--log profiles/recv_files/recv_files_bench.log]
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

SHAPES = {"small": (42111, None), "large": (1024, 8 << 20)}


def session(n_files, fixed_size, seed):
    """(stream bytes, digests uint8[n, 20], per file (run offset, run length,
    blocks)): the run of a file is its FILE_BLOCKs and its FILE_END."""
    rng = np.random.default_rng(seed)
    sizes = np.full(n_files, fixed_size) if fixed_size else rng.integers(0, 200 * 1024 + 1, n_files)
    parts, runs, at, counts = [], [], 0, []
    for f, size in enumerate(sizes.tolist()):
        head = b"FILE_START\nd%d/f%d\n" % (f // 100, f % 100)
        blocks, left = [], size
        while left:
            b = min(int(rng.geometric(1.0 / 8192)), 32768, left)
            blocks.append(b)
            left -= b
        counts.append(len(blocks))
        parts.append((head, blocks))
    digests = rng.integers(0, 256, (sum(counts), 20), dtype=np.uint8)
    raw, out, k = digests.tobytes(), [], 0
    for head, blocks in parts:
        body = b"".join(b"FILE_BLOCK\n" + raw[20 * (k + i):20 * (k + i) + 20] + b"\n%d\n" % b for i, b in enumerate(blocks))
        body += b"FILE_END\n"
        out += [head, body]
        runs.append((at + len(head), len(body), len(blocks)))
        at += len(head) + len(body)
        k += len(blocks)
    return b"".join(out), digests, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--shape", default="both", choices=("small", "large", "both"))
    ap.add_argument("--only", default=None, choices=("files",), help="time the one call alone (for a profiler)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("recv_files_bench.py needs a ROCm device: there is no CPU path to time")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(torch.cuda.get_device_name(0))
    for shape in (("small", "large") if args.shape == "both" else (args.shape,)):
        n_files, fixed = SHAPES[shape]
        data, digests, runs = session(n_files, fixed, 42)
        nb, n = len(data), digests.shape[0]
        run = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
        say(f"{shape}: {n_files} files, {n} blocks, {nb} bytes of stream ({nb / max(n, 1):.2f} B per block)")
        rng = np.random.default_rng(7)
        table = np.concatenate([digests[::2], rng.integers(0, 256, (n // 2, 20), dtype=np.uint8)])
        rng.shuffle(table)
        e = lambda m, t: torch.empty(m, dtype=t, device=dev)  # noqa: E731
        out = {r: (e((n, 20), torch.uint8), e(n, torch.int32), e(n, torch.int64), e(n, torch.int64)) for r in "ab"}
        bfile, name_at, name_len = e(n, torch.int32), e(n_files, torch.int64), e(n_files, torch.int32)
        first, fsize = e(n_files + 1, torch.int64), e(n_files, torch.int64)
        c_nb, c_nf, used, end = (ctypes.c_uint64(0) for _ in range(4))
        stop, still = ctypes.c_int(0), ctypes.c_int(0)
        s = torch.cuda.current_stream(dev).cuda_stream

        with device.BlockSet(torch.from_numpy(table).to(dev)) as bset:
            def files():
                d, z, o, r = out["a"]
                _lib.check(L.sf_receive_files_device(
                    bset._h, run.data_ptr(), nb, 0, 0, d.data_ptr(), z.data_ptr(), o.data_ptr(), r.data_ptr(),
                    bfile.data_ptr(), n, name_at.data_ptr(), name_len.data_ptr(), first.data_ptr(), fsize.data_ptr(),
                    n_files, ctypes.byref(c_nb), ctypes.byref(c_nf), ctypes.byref(used), ctypes.byref(stop),
                    ctypes.byref(still), ctypes.byref(end), s))

            def per_file():
                d, z, o, r = (t.data_ptr() for t in out["b"])
                base, k = run.data_ptr(), 0
                cnt, c, st, en = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0), ctypes.c_uint64(0)
                for at, length, blocks in runs:
                    _lib.check(L.sf_receive_blocks_device(bset._h, base + at, length, 0, d + 20 * k, z + 4 * k, o + 8 * k,
                                                          r + 8 * k, blocks, ctypes.byref(cnt), ctypes.byref(c),
                                                          ctypes.byref(st), ctypes.byref(en), s))
                    k += blocks

            def clock(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            t = {"files": [], "per-file": []}
            for _ in range(args.warmup + args.runs):  # the two routes alternate
                t["files"].append(clock(files))
                if not args.only:
                    t["per-file"].append(clock(per_file))
            assert (c_nb.value, c_nf.value, used.value, stop.value, still.value) == (n, n_files, nb, 0, 0)
            assert wire.recv_files_stats()[2] == 0
            assert torch.equal(out["a"][0].cpu(), torch.from_numpy(digests))
            for name, ms in t.items():
                ms = ms[args.warmup:]
                if ms:
                    med = statistics.median(ms)
                    say(f"  {name:9s} median {med:10.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f})  "
                        f"{n_files / med:9.2f} files/ms  {n / med / 1e3:8.3f} M blocks/s  {nb / med / 1e6:7.3f} GB/s of stream")
            if not args.only:
                for x, y in zip(out["a"], out["b"]):
                    assert torch.equal(x, y)
                say(f"  per-file / files = {statistics.median(t['per-file'][args.warmup:]) / statistics.median(t['files'][args.warmup:]):.1f}"
                    "  (finding the file boundaries on the host is not in per-file's time)")
            old = _lib.set_knob("SF_TEST_WIRE_PARSE_HOST", 1)
            try:
                ms = clock(files)
                assert wire.recv_files_stats()[2] == 1
            finally:
                _lib.set_knob("SF_TEST_WIRE_PARSE_HOST", old)
            say(f"  host      one run  {ms:10.3f} ms  (the fallback: copy back, serial parse, upload)")

    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
