"""A received GET_FILE run answered in one call, timed against the route the
library offered before and against the build alone (not part of
bench.py).

Input: the two seeded sources of scripts/send_files_bench.py (same seed, same
draws), each held by an Index in memory, every file requested once in list
order:
  small   42,111 files (names d<k>/f<j>), sizes uniform in 0-200 KiB
  large   1,024 files of 8 MiB

Each figure is a host clock around blocking calls that ends in a device
synchronise, the median of --runs after --warmup (min-max beside it), all legs
alternating in one process:
  a  serve      ONE sf_serve_get_files_device: the request run and the source's
                tables (Index.source_tables) in HBM; the run is freed again
  b  before     wire.Parser over the request run, then what
                Index.serve_get_files(names, device) does, step by step: one
                get_file and one list_file_blocks per name (SQLite), the rows
                packed and uploaded, ONE sf_wire_files_device
  c  build      sf_wire_files_device alone on inputs gathered beforehand, for
                the same answer: the floor the parse, the lookup and the
                indirection of (a) are priced against
  d  tables     Index.source_tables, once per sync: the database read, the
                pack and upload, sf_name_set_build
(a) and (b) must give the same bytes.

    python scripts/serve_files_bench.py [--shape small|large|both] [--only serve]
                                        [--log profiles/serve_files/serve_files_bench.log]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time
from pathlib import PurePath

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from send_files_bench import SHAPES, session  # noqa: E402
from syncfast_amd import _lib, wire  # noqa: E402
from syncfast_amd.device import upload  # noqa: E402
from syncfast_amd.index import Index  # noqa: E402
from syncfast_amd.timestamp import DateTimeUtc  # noqa: E402


def source(names, counts, sizes, digests) -> Index:
    idx = Index.open_in_memory()
    k = 0
    for f, (name, c) in enumerate(zip(names, counts)):
        fid, _new = idx.add_file(PurePath(name.decode()), DateTimeUtc.from_ns(f + 1))
        offsets = np.concatenate([[0], np.cumsum(sizes[k:k + c], dtype=np.int64)])
        idx.add_blocks(fid, [(int(offsets[i]), int(sizes[k + i]), digests[k + i].tobytes()) for i in range(c)])
        k += c
    idx.commit()
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--shape", default="both", choices=("small", "large", "both"))
    ap.add_argument("--only", default=None, choices=("serve",), help="time the one call alone (for a profiler)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("serve_files_bench.py needs a ROCm device: there is no CPU path to time")
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
        t0 = time.perf_counter()
        idx = source(names, counts, sizes, digests)
        say(f"{shape}: {n_files} files, {len(sizes)} blocks (the index took {time.perf_counter() - t0:.1f} s to fill)")
        requests = b"".join(wire.write_message("GetFile", n) for n in names)
        s = torch.cuda.current_stream(dev).cuda_stream

        # (d) once, then kept for every run of (a)
        tables = idx.source_tables(dev)
        d = {k: v * 1e3 for k, v in tables.seconds.items()}
        d_req = upload(requests, dev)
        torch.cuda.synchronize()

        def serve(read=False):
            got = tables.name_set.serve_files(d_req, tables.file_first, tables.digests, tables.sizes)
            assert (got.n_answered, got.why) == (n_files, 0)
            data = got.run.bytes() if read else None
            got.run.close()
            return data

        parts = {"parse": [], "sqlite": [], "upload": [], "build": []}
        pre = {}

        def before(read=False):
            t = [time.perf_counter()]
            asked = [m[1] for m in wire.Parser().receive(requests)]
            t.append(time.perf_counter())
            files = []
            for name in asked:  # Index.serve_get_files, step by step
                found = idx.get_file(PurePath(name.decode("utf-8")))
                files.append((name, idx.list_file_blocks(found[0])))
            rows = [b for _raw, blocks in files for b in blocks]
            packed = [np.cumsum([0] + [len(blocks) for _raw, blocks in files], dtype=np.int64).tobytes(),
                      np.cumsum([0] + [len(raw) for raw, _blocks in files], dtype=np.int64).tobytes(),
                      np.fromiter((size for _h, _offset, size in rows), np.uint32, len(rows)).tobytes(),
                      b"".join(h.bytes for h, _offset, _size in rows), b"".join(raw for raw, _blocks in files)]
            t.append(time.perf_counter())
            buf = upload(b"".join(packed), dev)
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            at = np.cumsum([0] + [len(p) for p in packed]).tolist()
            first, name_at, sz, dig, nm = (buf[a:b] for a, b in zip(at, at[1:]))
            pre.update(dig=dig.reshape(len(rows), 20), sz=sz.view(torch.int32), first=first.view(torch.int64), nm=nm,
                       name_at=name_at.view(torch.int64), buf=buf)
            run = wire.files_device(pre["dig"], pre["sz"], pre["first"], nm, pre["name_at"])
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            for k, a, b in zip(parts, t, t[1:]):
                parts[k].append((b - a) * 1e3)
            data = run.bytes() if read else None
            run.close()
            return data

        def build():
            h, bad = ctypes.c_void_p(), ctypes.c_uint64(0)
            _lib.check(L.sf_wire_files_device(pre["dig"].data_ptr(), pre["sz"].data_ptr(), pre["dig"].shape[0],
                                              pre["first"].data_ptr(), pre["nm"].data_ptr(), pre["name_at"].data_ptr(),
                                              n_files, ctypes.byref(h), ctypes.byref(bad), s), "sf_wire_files_device")
            _lib.check(L.sf_wire_run_free(h, s))

        if args.only:
            for _ in range(args.warmup + args.runs):
                say(f"  serve {clock(serve)[0]:.3f} ms")
            tables.close()
            continue
        same = serve(read=True) == before(read=True)
        say(f"  (a) and (b) give the same {len(requests)} request bytes' answer: {same}")
        assert same
        for v in parts.values():
            v.clear()
        t = {"a serve": [], "b before": [], "c build": []}
        for _ in range(args.warmup + args.runs):  # the legs alternate
            t["a serve"].append(clock(serve)[0])
            t["b before"].append(clock(before)[0])
            t["c build"].append(clock(build)[0])
        med = {}
        for name, ms in list(t.items()) + [("b   " + k, v) for k, v in parts.items()]:
            ms = ms[args.warmup:]
            med[name] = statistics.median(ms)
            say(f"  {name:12s} median {med[name]:10.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} runs)")
        say(f"  d tables     once: database {d['database']:.3f} ms, pack and upload {d['pack_upload']:.3f} ms, "
            f"sf_name_set_build {d['name_set']:.3f} ms")
        a, b, c = med["a serve"], med["b before"], med["c build"]
        d_all, d_dev = sum(d.values()), d["pack_upload"] + d["name_set"]
        say(f"  a / c = {a / c:.2f}   b / a = {b / a:.1f}   with (d) once: (a + d) / c = {(a + d_all) / c:.1f}, "
            f"b / (a + d) = {b / (a + d_all):.2f}; with (d)'s pack, upload and set alone: b / (a + d) = {b / (a + d_dev):.2f}")
        tables.close()

    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
