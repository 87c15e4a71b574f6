"""The destination's request run and its BLOCK_DATA join, timed beside the host
loops they replace (not part of bench.py).

The workload is block_data_send_bench.py's list: geometric block sizes, mean
8 KiB, cap 32 KiB, --mib of payload (535,012 blocks at 4 GiB), as the missing
rows of one incoming file that tile it.  Duplicates are injected: every 50th
row takes the digest and the size of the row 37 before it, so one digest in 50
is missing in two places.  The source answers the reference's requests, one
BLOCK_DATA per row in row order, so the parsed run has as many messages as
rows, duplicates included.

In one process:

  host-requests  b"".join(write_message("GetBlock", h) for h in
                 idx.list_missing_blocks()) on an in-memory index
  host-apply     Index.apply_block_data over the parsed arrays: one
                 list_block_locations and one mark_block_present per message
                 and location -- the parent commit's route, --host-runs times,
                 each on a fresh index (a wall clock around the call)
  requests       sf_wire_get_blocks_device over the rows (+ freeing the run)
  requests-d     the same with distinct = 1
  join           sf_place_block_data_device (the rows' present flags cleared
                 before each call, outside the clock)
  copy           sf_copy_blocks_device over the join's lists: the one launch

the device figures the median of --runs blocking calls after --warmup (a host
clock around call + synchronize), alternating inside one loop whose order
rotates.

    python scripts/want_bench.py [--log profiles/want/want.log]
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
from syncfast_amd.index import INSERT_BLOCK, Index  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--mib", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("want_bench.py needs a ROCm device: there is no CPU path to time")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sz = cdc_sizes(args.mib << 20, 9)
    n = len(sz)
    labels = np.random.default_rng(3).integers(0, 256, (n, 20), dtype=np.uint8)
    dup = np.arange(49, n, 50)
    sz[dup], labels[dup] = sz[dup - 37], labels[dup - 37]
    payload = int(sz.sum())
    row_off = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint64)  # the rows tile the file
    head = 33 + np.char.str_len(sz.astype(str)).astype(np.uint64)
    msg = head + sz + 1
    msg_off = np.concatenate([[0], np.cumsum(msg)[:-1]]).astype(np.uint64) + head  # payload offsets in the run
    run_len = int(msg.sum())
    say(f"{torch.cuda.get_device_name(0)}: {n} rows, {len(dup)} of them a second place of an earlier digest, "
        f"{n} messages, payload {payload} B, run {run_len} B")

    # ---- the parent's route, on the host
    hexes = [d.tobytes().hex() for d in labels]

    def index():
        idx = Index.open_in_memory()
        fid = idx.add_temp_file("new.bin")
        idx.begin()
        idx.db.executemany(INSERT_BLOCK, ((h, fid, int(o), int(s), 0) for h, o, s in zip(hexes, row_off, sz)))
        idx.commit()
        return idx
    t_req, t_apply, n_writes = [], [], 0
    want_requests = b""
    for _ in range(args.host_runs):
        idx = index()
        t0 = time.perf_counter()
        want_requests = b"".join(wire.write_message("GetBlock", h) for h in idx.list_missing_blocks())
        t_req.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        writes, rejected = idx.apply_block_data(labels, sz, msg_off, None)
        idx.commit()
        t_apply.append((time.perf_counter() - t0) * 1e3)
        n_writes = len(writes)
        assert not rejected and idx.list_missing_blocks() == []
        del idx, writes
    say(f"host-requests {statistics.median(t_req):10.1f} ms (min {min(t_req):.1f}, max {max(t_req):.1f}; "
        f"{args.host_runs} runs)  [write_message over list_missing_blocks, {len(want_requests)} B]")
    say(f"host-apply    {statistics.median(t_apply):10.1f} ms (min {min(t_apply):.1f}, max {max(t_apply):.1f}; "
        f"{args.host_runs} runs)  [Index.apply_block_data, {n} messages -> {n_writes} writes, commit included]")

    # ---- the device route
    src = device.splitmix_tensor(run_len, 6, dev)
    image = torch.zeros(payload, dtype=torch.uint8, device=dev)
    dig_t = torch.from_numpy(labels).to(dev)
    sz_t = torch.from_numpy(sz.astype(np.uint32).view(np.int32)).to(dev)
    dst_t = torch.from_numpy(row_off.view(np.int64)).to(dev)
    off_t = torch.from_numpy(msg_off.view(np.int64)).to(dev)
    present = torch.zeros(n, dtype=torch.uint8, device=dev)
    j_src, j_dst, j_rows, j_msgs = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4))
    j_sz = torch.empty(n, dtype=torch.int32, device=dev)
    uses = torch.empty(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    counts = [ctypes.c_uint64(0) for _ in range(3)]
    seen = {}

    def requests(distinct):
        h, k = ctypes.c_void_p(), ctypes.c_uint64(0)
        _lib.check(L.sf_wire_get_blocks_device(dig_t.data_ptr(), None, None, n, distinct, ctypes.byref(h),
                                               ctypes.byref(k), stream))
        seen[distinct] = k.value
        return h

    def free(h):
        _lib.check(L.sf_wire_run_free(h, stream))

    def join():
        _lib.check(L.sf_place_block_data_device(
            dig_t.data_ptr(), sz_t.data_ptr(), dst_t.data_ptr(), present.data_ptr(), n, dig_t.data_ptr(),
            sz_t.data_ptr(), off_t.data_ptr(), None, n, j_src.data_ptr(), j_dst.data_ptr(), j_sz.data_ptr(),
            j_rows.data_ptr(), j_msgs.data_ptr(), n, uses.data_ptr(), *(ctypes.byref(c) for c in counts), stream))

    def copy():
        _lib.check(L.sf_copy_blocks_device(src.data_ptr(), run_len, image.data_ptr(), payload, j_src.data_ptr(),
                                           j_dst.data_ptr(), j_sz.data_ptr(), None, n, None, stream))

    # exact, before anything is timed: the request bytes, the join's lists, the image
    run = wire.BlockDataRun(requests(0), dev)
    assert run.bytes() == want_requests and seen[0] == n
    run.close()
    free(requests(1))
    assert seen[1] == n - len(dup)
    join()
    torch.cuda.synchronize()
    assert [c.value for c in counts] == [n, 0, 0]
    first = np.arange(n)
    first[dup] = dup - 37  # the lowest-numbered message with the row's digest
    assert np.array_equal(j_rows.cpu().numpy(), np.arange(n)) and np.array_equal(j_msgs.cpu().numpy(), first)
    assert np.array_equal(j_src.cpu().numpy().view(np.uint64), msg_off[first])
    assert np.array_equal(j_dst.cpu().numpy().view(np.uint64), row_off)
    assert np.array_equal(j_sz.cpu().numpy().view(np.uint32), sz.astype(np.uint32))
    assert np.array_equal(uses.cpu().numpy(), np.bincount(first, minlength=n)) and bool(present.all())
    copy()
    for i in np.unique(np.concatenate([np.arange(8), dup[:8], dup[-8:], np.arange(n - 8, n)])):
        a, b, s = int(row_off[i]), int(msg_off[first[i]]), int(sz[i])
        assert torch.equal(image[a:a + s], src[b:b + s]), i

    calls = {"requests": lambda: free(requests(0)), "requests-d": lambda: free(requests(1)), "join": join, "copy": copy}
    times = {k: [] for k in calls}
    names = list(calls)
    for k in range(args.warmup + args.runs):
        for name in names[k % len(names):] + names[:k % len(names)]:
            present.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls[name]()
            torch.cuda.synchronize()
            if k >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    for name, what in (("requests", f"sf_wire_get_blocks_device, {31 * n} B"),
                       ("requests-d", f"the same, distinct: {31 * (n - len(dup))} B"),
                       ("join", f"sf_place_block_data_device, {n} rows x {n} messages -> {n} jobs"),
                       ("copy", f"sf_copy_blocks_device over the join's lists, {payload} B")):
        v = times[name]
        say(f"{name:13s} {med[name]:10.3f} ms (min {min(v):.3f}, max {max(v):.3f}; {args.runs} runs after "
            f"{args.warmup})  [{what}]")
    say(f"join / copy {med['join'] / med['copy']:.3f}; host-apply / join {statistics.median(t_apply) / med['join']:.0f}x; "
        f"host-requests / requests {statistics.median(t_req) / med['requests']:.0f}x; "
        f"join {n / med['join'] / 1e3:.1f} M rows/s, requests {31 * n / med['requests'] / 1e6:.1f} GB/s")
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
