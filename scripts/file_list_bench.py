"""The files-list phase on the device, timed against the per-message host
loops it stands beside (not part of bench.py).

Input: a seeded destination index of N files and the list a source announces
for it -- names of realistic length (d<k>/sub<j>/file_<i>_<word>.<ext>, 20 to
60 bytes), half of the files unchanged, a quarter with another blocks_hash, a
quarter unknown to the destination.  Two sets: 42,111 files (README's set) and
1,024.

Each figure is a host clock around blocking calls, the routes alternating in
one process, the median of --runs after --warmup, with min and max:
  receive   host    what existed before: wire.Parser over the list, one
                    Index.get_file (a SQLite query) per entry and the compare
            device  ONE sf_receive_file_entries_device over the list in HBM
                    against a name set (parse, lookup, compare, need list)
            upload  the list's bytes to HBM (what a caller whose bytes arrive
                    in host memory pays on top)
            build   the name set alone: sf_name_set_build over names already
                    in HBM (once per sync), and the upload of those names
  entries   host    the write_message loop over the source's files
            device  ONE sf_wire_file_entries_device (inputs in HBM)
  requests  host    the write_message loop over the needed names
            device  ONE sf_wire_get_files_device from the receive call's list
The device routes must give the host routes' bytes and the host loop's needed
entries.  add_temp_file (SQLite) is the same work on both routes and is not
timed.

    python scripts/file_list_bench.py [--files 42111,1024] [--only receive]
                                      [--log profiles/file_list/file_list_bench.log]
"""
import argparse
import os
import statistics
import sys
import time
from pathlib import PurePath

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from syncfast_amd import device, wire  # noqa: E402
from syncfast_amd.digest import HashDigest  # noqa: E402
from syncfast_amd.index import Index  # noqa: E402
from syncfast_amd.timestamp import DateTimeUtc  # noqa: E402

WORDS = ("report", "image", "notes", "backup", "thumbnail_large", "index", "a", "configuration_final_v2")
EXTS = ("txt", "jpeg", "tar.gz", "c", "parquet")


def data_set(n, seed):
    """(destination Index, [(name, size, announced hash)], expected need flags)."""
    rng = np.random.default_rng(seed)
    names = [b"d%d/sub%d/file_%d_%s.%s" % (i % 97, i % 13, i, WORDS[i % len(WORDS)].encode(), EXTS[i % len(EXTS)].encode())
             for i in range(n)]
    hashes = rng.integers(0, 256, (n, 20), dtype=np.uint8)
    kind = rng.permutation(n) % 4  # 0, 1: unchanged; 2: changed; 3: unknown
    idx = Index.open_in_memory()
    idx.begin()
    stamp = DateTimeUtc.from_ns(0).to_sql()
    idx.db.executemany("INSERT INTO files(name, modified, size, blocks_hash, temporary) VALUES(?, ?, ?, ?, 0);",
                       ((names[i].decode(), stamp, 1000 + i, HashDigest(hashes[i].tobytes()).to_sql())
                        for i in range(n) if kind[i] != 3))
    idx.commit()
    announced = hashes.copy()
    announced[kind == 2, 0] ^= 0xFF
    files = [(names[i], 1000 + i, HashDigest(announced[i].tobytes())) for i in range(n)]
    return idx, files, (kind >= 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--files", default="42111,1024")
    ap.add_argument("--only", default=None, choices=("receive",), help="the device receive alone (for a profiler)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("file_list_bench.py needs a ROCm device: there is no CPU path to time")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    say(torch.cuda.get_device_name(0))
    for n in (int(v) for v in args.files.split(",")):
        idx, files, need = data_set(n, 42)
        listing = b"".join(wire.write_message("FileEntry", *f) for f in files) + wire.write_message("EndFiles")
        name_len = statistics.mean(len(f[0]) for f in files)
        say(f"{n} files: {len(listing)} bytes of list ({len(listing) / n:.1f} B per entry, names of {name_len:.1f} B), "
            f"{int(need.sum())} needed")
        rows = idx.db.execute("SELECT name, blocks_hash FROM files WHERE temporary = 0 ORDER BY file_id;").fetchall()
        dest_names = [r[0].encode() for r in rows]
        have = torch.from_numpy(np.frombuffer(b"".join(bytes.fromhex(r[1]) for r in rows), np.uint8).reshape(-1, 20).copy()).to(dev)
        result = {}

        def receive_host():
            needed = []
            for k, (_kind, name, _size, blocks_hash) in enumerate(wire.Parser().receive(listing)[:-1]):
                found = idx.get_file(PurePath(name.decode("utf-8")))
                if found is None or found[2] != blocks_hash:
                    needed.append(k)
            result["host"] = needed

        packed, at = device.pack_names(dest_names, dev)
        run = device.upload(listing, dev)
        sets = []

        def build():
            sets.append(device.NameSet(packed, at))

        def build_upload():
            device.pack_names(dest_names, dev)

        def upload():
            device.upload(listing, dev)

        def receive_device():
            result["device"] = sets[-1].receive_entries(run, have)

        # the two writers' inputs, in HBM
        e_names, e_at = device.pack_names([f[0] for f in files], dev)
        e_sizes = torch.tensor([f[1] for f in files], dtype=torch.int64, device=dev)
        e_hashes = torch.from_numpy(np.frombuffer(b"".join(f[2].bytes for f in files), np.uint8).reshape(-1, 20).copy()).to(dev)

        def entries_host():
            result["entries_host"] = b"".join(wire.write_message("FileEntry", *f) for f in files) + wire.write_message("EndFiles")

        def entries_device():
            result["entries_device"] = wire.file_entries_device(e_names, e_at, e_sizes, e_hashes)

        def requests_host():
            result["requests_host"] = b"".join(wire.write_message("GetFile", files[k][0]) for k in result["host"])

        def requests_device():
            got = result["device"]
            result["requests_device"] = wire.get_files_device(run, got.name_at, got.name_len, got.need_list)

        order = [("build", build), ("receive device", receive_device)] if args.only else [
            ("build", build), ("build: names upload", build_upload), ("receive host", receive_host),
            ("receive device", receive_device), ("receive: list upload", upload), ("entries host", entries_host),
            ("entries device", entries_device), ("requests host", requests_host), ("requests device", requests_device)]
        t = {name: [] for name, _fn in order}
        for _ in range(args.warmup + args.runs):  # the routes alternate
            for name, fn in order:
                t[name].append(clock(fn))
            for s in sets[:-1]:
                s.close()
            del sets[:-1]
        got = result["device"]
        assert (int(got.name_at.numel()), got.stop, got.bad_name) == (n, wire.SF_WIRE_END_FILES, None)
        assert device.file_entries_stats()[0] == 0 and got.need.cpu().numpy().astype(bool).tolist() == need.tolist()
        if not args.only:
            assert got.need_list.cpu().tolist() == result["host"]
            assert result["entries_device"].bytes() == result["entries_host"] == listing
            assert result["requests_device"].bytes() == result["requests_host"]
        for name, ms in t.items():
            ms = ms[args.warmup:]
            med = statistics.median(ms)
            say(f"  {name:22s} median {med:10.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f})  "
                f"{n / med:10.1f} files/ms")
        if not args.only:
            med = {k: statistics.median(v[args.warmup:]) for k, v in t.items()}
            for what in ("receive", "entries", "requests"):
                say(f"  {what}: host / device = {med[what + ' host'] / med[what + ' device']:.1f}")
            say(f"  receive: host / (build + names upload + list upload + device) = "
                f"{med['receive host'] / (med['build'] + med['build: names upload'] + med['receive: list upload'] + med['receive device']):.1f}")
        sets[-1].close()

    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
