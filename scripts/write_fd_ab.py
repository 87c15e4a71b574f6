"""sf_write_device_fd of two builds in ONE process: both libraries loaded,
alternating calls on the same tensor and the same file, so that where a
process's pinned buffers, page-cache pages and pool threads land is common to
both (profiles/host_split/README.md: between processes that placement moves
the figure by tens of per cent).

usage: python scripts/write_fd_ab.py NAME=LIB NAME=LIB   (loaded in that order)"""
import ctypes
import statistics
import sys
import tempfile
import time

import torch


def main():
    libs = {}
    for arg in sys.argv[1:]:
        name, path = arg.split("=", 1)
        lib = ctypes.CDLL(path)
        lib.sf_write_device_fd.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64,
                                           ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
        lib.sf_write_device_fd.restype = ctypes.c_int
        libs[name] = lib
    n, warmup, runs = 4 << 30, 3, 15
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    t.random_(0, 256)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    times = {k: [] for k in libs}
    with tempfile.NamedTemporaryFile() as f:
        for rep in range(warmup + runs):
            for k, lib in libs.items():
                nw = ctypes.c_uint64(0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = lib.sf_write_device_fd(t.data_ptr(), n, f.fileno(), 0, ctypes.byref(nw), stream)
                dt = (time.perf_counter() - t0) * 1e3
                assert rc == 0 and nw.value == n, (k, rc, nw.value)
                if rep >= warmup:
                    times[k].append(dt)
    for k, v in times.items():
        print(f"{k}: median {statistics.median(v):.1f} ms, mean {statistics.mean(v):.1f}, min {min(v):.1f}, "
              f"max {max(v):.1f}  " + " ".join(f"{x:.0f}" for x in v), flush=True)


if __name__ == "__main__":
    main()
