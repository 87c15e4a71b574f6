"""A whole GetFiles answer built in one call, timed against one call per file
and against the Python loop (not part of bench.py).

Input: the session of scripts/recv_files_bench.py seen from the source -- a
destination asked for every file at once, and the source holds every file's
rows in HBM: digests, sizes, the CSR of the files into them and the packed
names.  Two shapes, generated exactly as there (same seed, same draws):
  small   42,111 files (names d<k>/f<j>), sizes uniform in 0-200 KiB
  large   1,024 files of 8 MiB (config 3's shape)
Block sizes are CDC-like (geometric, mean 8 KiB, capped at 32 KiB), digests
random.

Each figure is a host clock around blocking calls that ends in a device
synchronise, the median of --runs after --warmup, legs (a) and (b)
alternating in one process:
  a  files      ONE sf_wire_files_device over all files (and the run's free)
  a+ files+read the same, and the run copied to the host (sf_wire_run_read)
  b  per-file   what the library offered before: one sf_wire_blocks_device per
                file, each blocking on its read-back, into one device buffer;
                then that buffer copied to the host and FILE_START / FILE_END
                joined around each file's run there.  Compare with a+: both
                end with the stream in host memory.
  c  python     the write_message loop over host copies of the same rows
  d  one-list   ONE sf_wire_blocks_device over all blocks as a single list:
                the FILE_BLOCK bytes alone, no file frames -- what the binary
                search and the frames cost on top of it
All of a+, b and c must give the same bytes.

    python scripts/send_files_bench.py [--shape small|large|both] [--only files]
                                       [--log profiles/send_files/send_files_bench.log]
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

from syncfast_amd import _lib, wire  # noqa: E402

SHAPES = {"small": (42111, None), "large": (1024, 8 << 20)}


def session(n_files, fixed_size, seed):
    """(names, per-file block counts, sizes uint32[n], digests uint8[n, 20]):
    the draws of recv_files_bench.session, in its order."""
    rng = np.random.default_rng(seed)
    file_sizes = np.full(n_files, fixed_size) if fixed_size else rng.integers(0, 200 * 1024 + 1, n_files)
    names, counts, sizes = [], [], []
    for f, size in enumerate(file_sizes.tolist()):
        names.append(b"d%d/f%d" % (f // 100, f % 100))
        left, k = size, 0
        while left:
            b = min(int(rng.geometric(1.0 / 8192)), 32768, left)
            sizes.append(b)
            left -= b
            k += 1
        counts.append(k)
    digests = rng.integers(0, 256, (len(sizes), 20), dtype=np.uint8)
    return names, counts, np.array(sizes, np.uint32), digests


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--shape", default="both", choices=("small", "large", "both"))
    ap.add_argument("--only", default=None, choices=("files",), help="time the one call alone (for a profiler)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-runs", type=int, default=3, help="runs of the per-file and python legs (seconds each)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("send_files_bench.py needs a ROCm device: there is no CPU path to time")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    say(torch.cuda.get_device_name(0))
    for shape in (("small", "large") if args.shape == "both" else (args.shape,)):
        n_files, fixed = SHAPES[shape]
        names, counts, sizes, digests = session(n_files, fixed, 42)
        n = len(sizes)
        first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        name_at = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.int64)
        d_dig, d_sizes = torch.from_numpy(digests).to(dev), torch.from_numpy(sizes.view(np.int32)).to(dev)
        d_first, d_name_at = torch.from_numpy(first).to(dev), torch.from_numpy(name_at).to(dev)
        d_names = torch.frombuffer(bytearray(b"".join(names)), dtype=torch.uint8).to(dev)
        block_bytes = int(sum(33 + len(str(int(s))) for s in sizes.tolist()))
        total = block_bytes + int(name_at[-1]) + 21 * n_files
        say(f"{shape}: {n_files} files, {n} blocks, {total} bytes of answer, {block_bytes} of them FILE_BLOCKs")
        s = torch.cuda.current_stream(dev).cuda_stream
        d_out = torch.empty(block_bytes, dtype=torch.uint8, device=dev)
        host = np.empty(total, np.uint8)
        h_out = np.empty(block_bytes, np.uint8)
        need = ctypes.c_uint64(0)

        def build():
            h, bad = ctypes.c_void_p(), ctypes.c_uint64(0)
            _lib.check(L.sf_wire_files_device(d_dig.data_ptr(), d_sizes.data_ptr(), n, d_first.data_ptr(),
                                              d_names.data_ptr(), d_name_at.data_ptr(), n_files, ctypes.byref(h),
                                              ctypes.byref(bad), s), "sf_wire_files_device")
            return h

        def files():
            _lib.check(L.sf_wire_run_free(build(), s))

        def files_read():
            h = build()
            _lib.check(L.sf_wire_run_read(h, 0, host.ctypes.data, total))
            _lib.check(L.sf_wire_run_free(h, s))
            return host.tobytes()

        def per_file():
            dig, siz, out, at = d_dig.data_ptr(), d_sizes.data_ptr(), d_out.data_ptr(), 0
            ends = []
            for f in range(n_files):
                k, c = int(first[f]), counts[f]
                if c:
                    _lib.check(L.sf_wire_blocks_device(dig + 20 * k, siz + 4 * k, c, out + at, block_bytes - at,
                                                       ctypes.byref(need), s), "sf_wire_blocks_device")
                    at += need.value
                ends.append(at)
            h_out[:] = d_out.cpu().numpy()
            raw, parts, a = h_out.tobytes(), [], 0
            for name, b in zip(names, ends):
                parts += [b"FILE_START\n", name, b"\n", raw[a:b], b"FILE_END\n"]
                a = b
            return b"".join(parts)

        def python():
            dig, out, k = digests.tobytes(), [], 0
            for name, c in zip(names, counts):
                out.append(wire.write_message("FileStart", name))
                for i in range(k, k + c):
                    out.append(wire.write_message("FileBlock", dig[20 * i:20 * i + 20], int(sizes[i])))
                out.append(wire.write_message("FileEnd"))
                k += c
            return b"".join(out)

        def one_list():
            _lib.check(L.sf_wire_blocks_device(d_dig.data_ptr(), d_sizes.data_ptr(), n, d_out.data_ptr(), block_bytes,
                                               ctypes.byref(need), s), "sf_wire_blocks_device")

        t = {"files": [], "files+read": [], "one-list": [], "per-file": [], "python": []}
        got = {}
        for k in range(args.warmup + args.runs):  # the legs alternate
            t["files"].append(clock(files)[0])
            if args.only:
                continue
            ms, got["files+read"] = clock(files_read)
            t["files+read"].append(ms)
            t["one-list"].append(clock(one_list)[0])
            if k >= args.warmup + args.runs - args.host_runs - 1:  # one warm-up run of its own, then host_runs
                ms, got["per-file"] = clock(per_file)
                t["per-file"].append(ms)
                ms, got["python"] = clock(python)
                t["python"].append(ms)
        med = {}
        for name, ms in t.items():
            ms = ms[args.warmup:] if name in ("files", "files+read", "one-list") else ms[1:]
            if ms:
                med[name] = statistics.median(ms)
                wrote = block_bytes if name == "one-list" else total
                say(f"  {name:10s} median {med[name]:10.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} runs)  "
                    f"{n / med[name] / 1e3:9.3f} M blocks/s  {wrote} bytes written")
        if not args.only:
            assert len(got["files+read"]) == total
            assert got["files+read"] == got["python"] == got["per-file"]
            say(f"  per-file / files+read = {med['per-file'] / med['files+read']:.1f}   python / files+read = "
                f"{med['python'] / med['files+read']:.1f}   files / one-list = {med['files'] / med['one-list']:.2f}")

    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
