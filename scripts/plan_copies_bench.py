"""The destination's copy plan and its local-file loader, timed beside the host
route they replace (not part of bench.py).

The workload is block_data_send_bench.py's list: geometric block sizes, mean
8 KiB, cap 32 KiB, --mib of payload (535,012 blocks at 4 GiB), as ONE GetFiles
stream of --files incoming files that the blocks tile.  Every second block is
held locally: its row lies, in shuffled order, in one of --local local files
that sit back to back (256-byte aligned) in one HBM arena, and its announced
digest is the explicit-list kernel's over those bytes, so verification passes.
The other blocks are missing.

In one process, after the plan has been compared with a numpy restatement:

  host-loop    the parent commit's Index._store_received tuple loop over the
               blocks (the executemany is the same on both routes and is left
               out) plus FileImages.apply_copies per incoming file, with the
               local files already in HBM (source=): --host-runs times, a wall
               clock around it
  query        sf_plan_copies_device with d_local_base NULL
  plan         the plan with d_src NULL: every candidate a job
  plan-verify  the plan with the arena: every candidate hashed first
  hash         sf_index_device_blocks over the candidates' list alone: the
               explicit-list kernel's rate on the bytes the verified plan reads
  copy         sf_copy_blocks_device over the plan's lists

the device figures the median of --runs blocking calls after --warmup (a host
clock around call + synchronize), alternating inside one loop whose order
rotates.  Then a --file-mib file in the page cache is brought to HBM by
device.read_fd and by np.fromfile + device.upload, alternating.

    python scripts/plan_copies_bench.py [--log profiles/plan_copies/plan_copies.log]
"""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile
import time
from pathlib import PurePath

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from copy_blocks_bench import cdc_sizes  # noqa: E402
from syncfast_amd import _lib, device  # noqa: E402
from syncfast_amd.assemble import FileImages  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--mib", type=int, default=4096)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--local", type=int, default=32)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-runs", type=int, default=2)
    ap.add_argument("--file-mib", type=int, default=1024)
    ap.add_argument("--file-runs", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plan_copies_bench.py needs a ROCm device: there is no CPU path to time")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- the stream's blocks: --files sections of equal block counts
    sz = cdc_sizes(args.mib << 20, 9).astype(np.int64)
    n = len(sz)
    block_file = np.minimum(np.arange(n) * args.files // n, args.files - 1).astype(np.int32)
    first = np.searchsorted(block_file, np.arange(args.files + 1))
    ends = np.cumsum(sz)
    start_of_file = np.concatenate([[0], ends])[first[:-1]]
    offsets = np.concatenate([[0], ends[:-1]]) - start_of_file[block_file]
    file_size = np.concatenate([[0], ends])[first[1:]] - start_of_file
    names = [PurePath(f".syncfast_tmp_new{f:03d}.bin") for f in range(args.files)]
    images = FileImages(dict(zip(names, file_size.tolist())), dev)
    file_base = images.bases(names)
    # ---- the table: the even blocks, shuffled, over --local files of one arena
    held = np.arange(0, n, 2)
    t = len(held)
    rng = np.random.default_rng(4)
    order = rng.permutation(t)  # row r holds block held[order[r]]
    t_size = sz[held[order]]
    t_file = np.minimum(np.arange(t) * args.local // t, args.local - 1).astype(np.int32)
    t_first = np.searchsorted(t_file, np.arange(args.local + 1))
    t_ends = np.cumsum(t_size)
    l_start = np.concatenate([[0], t_ends])[t_first[:-1]]
    t_off = np.concatenate([[0], t_ends[:-1]]) - l_start[t_file]
    l_size = np.concatenate([[0], t_ends])[t_first[1:]] - l_start
    l_base = np.concatenate([[0], np.cumsum((l_size + 255) // 256 * 256)[:-1]])
    arena_len = int(l_base[-1] + l_size[-1])
    rows = np.full(n, -1, np.int64)
    rows[held[order]] = np.arange(t)
    held_bytes = int(t_size.sum())
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(dev)  # noqa: E731
    arena = device.splitmix_tensor(arena_len, 6, dev)
    cand_off = up(l_base[t_file] + t_off, np.int64)
    cand_sz = up(t_size, np.int32)
    row_dig = device.index_device_blocks(arena, cand_off, cand_sz)  # what each row's bytes hash to
    dig_t = torch.from_numpy(rng.integers(0, 256, (n, 20), dtype=np.uint8)).to(dev)
    dig_t[up(held[order], np.int64)] = row_dig
    x = dict(sizes=up(sz, np.int32), offsets=up(offsets, np.int64), rows=up(rows, np.int64),
             block_file=up(block_file, np.int32), table_file=up(t_file, np.int32), table_offset=up(t_off, np.int64),
             table_size=up(t_size, np.int32), local_base=up(l_base, np.int64), local_size=up(l_size, np.int64))
    say(f"{torch.cuda.get_device_name(0)}: {n} blocks in {args.files} incoming files, payload {int(sz.sum())} B; "
        f"{t} of them held in {args.local} local files, {held_bytes} B, arena {arena_len} B")

    # ---- the parent's route, on the host: the tuple loop and apply_copies
    found, offs_h, sz_h, bf_h = rows.tolist(), offsets.tolist(), sz.tolist(), block_file.tolist()
    local_names = [f"old{j:03d}.bin" for j in range(args.local)]
    table_rows = [(None, True, local_names[j], int(o), int(s)) for j, o, s in zip(t_file, t_off, t_size)]
    local_t = {local_names[j]: arena[int(l_base[j]): int(l_base[j] + l_size[j])] for j in range(args.local)}
    t_loop, t_apply = [], []
    for _ in range(args.host_runs):
        host_images = FileImages(dict(zip(names, file_size.tolist())), dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        copies = [[] for _ in names]
        for f, o, s, q in zip(bf_h, offs_h, sz_h, found):
            if q >= 0:
                copies[f].append((PurePath(table_rows[q][2]), int(table_rows[q][3]), int(o), int(s)))
        t1 = time.perf_counter()
        calls = sum(host_images.apply_copies(name, c, source=lambda k: local_t[str(k)]) for name, c in zip(names, copies))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_loop.append((t1 - t0) * 1e3)
        t_apply.append((t2 - t1) * 1e3)
    host_ms = statistics.median(a + b for a, b in zip(t_loop, t_apply))
    say(f"host-loop     {host_ms:10.1f} ms = tuple loop {statistics.median(t_loop):.1f} + apply_copies "
        f"{statistics.median(t_apply):.1f} ({calls} copy_blocks calls; {args.host_runs} runs, local files in HBM already)")

    # ---- the device route
    present, ask = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2))
    dst, j_src, j_dst, j_blk = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4))
    j_sz = torch.empty(n, dtype=torch.int32, device=dev)
    local_jobs = torch.empty(args.local, dtype=torch.int32, device=dev)
    counts = (ctypes.c_uint64 * 8)()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def plan(query, verify):
        rc = L.sf_plan_copies_device(
            dig_t.data_ptr(), x["sizes"].data_ptr(), x["offsets"].data_ptr(), x["rows"].data_ptr(),
            x["block_file"].data_ptr(), n, file_base.data_ptr(), args.files, x["table_file"].data_ptr(),
            x["table_offset"].data_ptr(), x["table_size"].data_ptr(), t, None if query else x["local_base"].data_ptr(),
            x["local_size"].data_ptr(), args.local, arena.data_ptr() if verify else None, arena_len,
            present.data_ptr(), ask.data_ptr(), dst.data_ptr(), j_src.data_ptr(), j_dst.data_ptr(), j_sz.data_ptr(),
            j_blk.data_ptr(), n, local_jobs.data_ptr(), counts, stream)
        if rc != (_lib.SF_ENOSPC if query else 0):
            raise _lib.SfError(rc, "sf_plan_copies_device")

    def copy():
        _lib.check(L.sf_copy_blocks_device(arena.data_ptr(), arena_len, images.buffer.data_ptr(),
                                           images.buffer.numel(), j_src.data_ptr(), j_dst.data_ptr(), j_sz.data_ptr(),
                                           None, t, None, stream))

    def hash_candidates():
        device.index_device_blocks(arena, cand_off, cand_sz, out=row_dig, check_range=False)

    # exact, before anything is timed: the plan against numpy, with and without verification, and the images
    base_h = file_base.cpu().numpy()
    for verify in (False, True):
        plan(False, verify)
        torch.cuda.synchronize()
        assert list(counts) == [t, held_bytes, n - t, 0, 0, 0, 0, 0], list(counts)
        assert np.array_equal(j_blk[:t].cpu().numpy(), held)
        assert np.array_equal(j_src[:t].cpu().numpy(), (l_base[t_file] + t_off)[rows[held]])
        assert np.array_equal(j_dst[:t].cpu().numpy(), (base_h[block_file] + offsets)[held])
        assert np.array_equal(j_sz[:t].cpu().numpy(), sz[held])
        assert np.array_equal(present.cpu().numpy(), (rows >= 0).astype(np.uint8))
        assert np.array_equal(local_jobs.cpu().numpy(), np.bincount(t_file, minlength=args.local))
    copy()
    torch.cuda.synchronize()
    assert torch.equal(images.buffer, host_images.buffer)  # the parent's route filled the same bytes
    plan(True, False)
    assert counts[0] == t

    calls_d = {"query": lambda: plan(True, False), "plan": lambda: plan(False, False),
               "plan-verify": lambda: plan(False, True), "hash": hash_candidates, "copy": copy}
    times = {k: [] for k in calls_d}
    order_d = list(calls_d)
    for k in range(args.warmup + args.runs):
        for name in order_d[k % len(order_d):] + order_d[:k % len(order_d)]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls_d[name]()
            torch.cuda.synchronize()
            if k >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    for name, what in (("query", f"sf_plan_copies_device, d_local_base NULL, {n} blocks"),
                       ("plan", f"the plan, no verification -> {t} jobs"),
                       ("plan-verify", f"the plan, {t} candidates hashed first, {held_bytes} B"),
                       ("hash", "sf_index_device_blocks over the candidates' list alone"),
                       ("copy", f"sf_copy_blocks_device over the plan's lists, {held_bytes} B")):
        v = times[name]
        say(f"{name:13s} {med[name]:10.3f} ms (min {min(v):.3f}, max {max(v):.3f}; {args.runs} runs after "
            f"{args.warmup})  [{what}]")
    say(f"plan {n / med['plan'] / 1e6:.2f} G blocks/s; plan-verify {held_bytes / med['plan-verify'] / 1e6:.1f} GB/s of "
        f"local bytes (hash alone {held_bytes / med['hash'] / 1e6:.1f} GB/s, copy {held_bytes / med['copy'] / 1e6:.1f} "
        f"GB/s); plan-verify / copy {med['plan-verify'] / med['copy']:.2f}, plan / copy {med['plan'] / med['copy']:.3f}; "
        f"host-loop / (plan + copy) {host_ms / (med['plan'] + med['copy']):.0f}x, / (plan-verify + copy) "
        f"{host_ms / (med['plan-verify'] + med['copy']):.0f}x")

    # ---- the loader against np.fromfile + upload, on a file in the page cache
    size = args.file_mib << 20
    with tempfile.NamedTemporaryFile(dir=os.environ.get("TMPDIR")) as f:
        block = np.random.default_rng(1).integers(0, 256, 64 << 20, dtype=np.uint8).tobytes()
        for at in range(0, size, len(block)):
            f.write(block[:size - at])
        f.flush()
        out = torch.empty(size, dtype=torch.uint8, device=dev)
        t_lib, t_np = [], []
        for k in range(1 + args.file_runs):  # the first round warms the page cache and the pinned stages
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            device.read_fd(f.fileno(), size, out=out)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            other = device.upload(np.fromfile(f.name, dtype=np.uint8).tobytes(), dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if k == 0:
                assert torch.equal(out, other)
            else:
                t_lib.append((t1 - t0) * 1e3)
                t_np.append((t2 - t1) * 1e3)
            del other
    a, b = statistics.median(t_lib), statistics.median(t_np)
    say(f"read_fd       {a:10.1f} ms (min {min(t_lib):.1f}, max {max(t_lib):.1f}) = {size / a / 1e6:.1f} GB/s; "
        f"np.fromfile + upload {b:.1f} ms (min {min(t_np):.1f}, max {max(t_np):.1f}) = {size / b / 1e6:.1f} GB/s; "
        f"{b / a:.1f}x  [{size} B from the page cache, {args.file_runs} runs]")
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
