#!/usr/bin/env python3
"""Headline benchmark: device-resident block-signature indexing on MI355X.

Metric (BASELINE.json): "GiB/s indexed (device-resident), 4 KiB blocks;
%HBM peak at 1/2/4/8 GPU".

Workload (BASELINE.json configs[1]): index one 8 GiB synthetic file in 4 KiB
blocks on one MI355X.  A step = one pass of the hot path over the whole
buffer: the SHA-1 kernel over every block (input already resident in HBM) ->
20-byte digest table.  With --gpus N (torchrun, one rank per GPU) the logical
file is N x 8 GiB, each rank holds its contiguous 8 GiB shard (weak scaling,
the shard layout of configs[3]) and a step also gathers every shard's digest
table to rank 0 over RCCL (the exchange the single-file blocks_hash needs).

Also: --config 3 (1024 x 8 MiB files, per-file blocks_hash on device),
--config 4 (32 GiB shard per GPU of one 256 GiB file at 8 GPUs, RCCL gather
of the 1.25 GiB table) and --config 5 (32 GiB, 64 KiB blocks).

A plain run does only what the headline needs: it generates the input in
HBM, warms up, times --steps steps, writes --dump-outputs DIR if asked (what
the last timed step computed, as DIR/<name>.npy; the input is seeded, so two
builds can be compared output for output) and prints the line.  --full adds,
after the timed steps, the self-checks (digests and blocks_hash against the
product's host SHA-1) and every side leg below from cpu_baseline on; in a
plain line those fields are null.

Rank 0 prints ONE JSON line (contract in the task statement), with:
  roofline      -- the SHA-1 kernel's algorithmic bytes / its average launch
                   time (HIP events on the launch stream) vs 8.0 TB/s HBM peak;
                   traffic = HBM bytes per launch from rocprofv3 PMC counters
                   (profiles/traffic.json, measured separately on the SAME
                   kernel -- keyed by the SHA-256 of the headline kernel's
                   machine code in the library's gfx950 code object -- else
                   null);
  cpu_baseline  -- the C oracle (single-threaded SHA-1 port of the
                   reference loop) on a bounded sample of the same bytes, rank 0
                   at N=1 only; cpu_baseline_shani the same tiling with the
                   product's SHA-NI host SHA-1, on 1 core and on all cores;
  e2e_host_buffer -- not `value`: the same bytes from a host buffer through
                   sf_index_buffer (H2D + kernel + D2H rows), beside the raw
                   pinned H2D rate (north_star asks for the end-to-end rate);
  content_defined_list -- not `value`: the reference's default block shape
                   (content-defined, mean 8 KiB, max 32 KiB) as an explicit
                   4 GiB list through sf_index_device_blocks, beside the same
                   bytes as a 4 KiB list (config 2 at N=1);
  config1       -- BASELINE configs[0] (the unmodified Rust CPU path): probed
                   live (cargo / rustc on this host) and reported as not
                   runnable when they are absent.

Launch: --gpus N > 1 without torchrun (no WORLD_SIZE in the environment)
starts the N rank processes itself -- torch.distributed.run as a CHILD
process, before anything here touches the GPU -- and exits with its status;
rank 0 asserts that the process group holds N ranks.  The process group has
a timeout (--dist-timeout, 300 s): a gather that never completes ends the run
with an error instead of hanging.  At N > 1 the line carries a `multi` block:
every rank's kernel time, how long each rank's stream waited for the gathers
(as receiving rank and as sender), and the world size the backend reports.
"""
import ctypes
import datetime
import argparse
import hashlib
import json
import os
import shutil
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

GiB = 1 << 30
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec, MI355X_MICROARCH.md
# SHA-1 is VALU-issue bound: 613 VALU per 64-B
# compression, 400 half-rate (4 SIMD-cycles per wave64 op) + 213 full-rate
# (2 cycles); the uniform padding chunk of a 64-B-multiple block ~1120 cycles.
SIMDS, MAX_CLOCK_HZ = 1024, 2.4e9  # 256 CUs x 4 SIMD-32, MI355X_MICROARCH.md


def valu_ceiling_gbs(bs):
    """Input bytes/s the SIMDs can hash at the max clock under the op-cost
    model above (one lane per block, 64 blocks per wave)."""
    full, rem = divmod(bs, 64)
    per_block = full * (400 * 4 + 213 * 2) + (1120 if rem == 0 else (400 * 4 + 213 * 2) * (1 + (rem >= 56)))
    return SIMDS * MAX_CLOCK_HZ * 64 * bs / per_block / 1e9
SEED = 0x5EED0000

DUMP_MAX_BYTES = 64 * 1000 * 1000  # --dump-outputs: all .npy files of one run together
DUMP_ROWS = 1 << 18  # rows kept of a table with more rows than this


def dump_rows(n):
    """The row numbers --dump-outputs keeps of an n-row table: every row, or a
    fixed sample (seed SEED, ascending) that holds the first and the last row.
    Depends on n alone, so two builds dump the same rows."""
    import numpy as np
    if n <= DUMP_ROWS:
        return np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(SEED)
    return np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, DUMP_ROWS - 2)])).astype(np.int64)


def dump_outputs(torch, out_dir, digests, file_hashes=None, weak=None):
    """--dump-outputs: the arrays a caller of the timed path receives, as the
    last timed step left them.  digests.npy: rows dump_rows() of the (blocks,
    20) digest table, float32, one digest byte per element; digest_rows.npy:
    those row numbers (float64); file_hashes.npy: config 3's per-file
    blocks_hash, whole; weak.npy: --weak's Adler-32 sums of the same rows
    (float64, exact)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    rows = dump_rows(digests.shape[0])
    idx = torch.from_numpy(rows).to(digests.device)
    arrays = {"digests": digests.index_select(0, idx).cpu().numpy().astype(np.float32),
              "digest_rows": rows.astype(np.float64)}
    if file_hashes is not None:
        arrays["file_hashes"] = file_hashes.cpu().numpy().astype(np.float32)
    if weak is not None:
        arrays["weak"] = weak.index_select(0, idx).cpu().numpy().astype(np.uint32).astype(np.float64)
    assert sum(v.nbytes for v in arrays.values()) <= DUMP_MAX_BYTES, "--dump-outputs: more than 64 MB"
    for name, v in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), v)


CONFIGS = {
    2: dict(workload="index one 8 GiB synthetic file, 4 KiB blocks (BASELINE configs[1])",
            bytes=8 * GiB, block=4096, files=1),
    3: dict(workload="index 1024 x 8 MiB synthetic files, 4 KiB blocks (BASELINE configs[2])",
            bytes=1024 * 8 * (1 << 20), block=4096, files=1024),
    4: dict(workload="index one 256 GiB synthetic file, 4 KiB blocks, 32 GiB contiguous shard per GPU "
                     "(BASELINE configs[3] at --gpus 8; N x 32 GiB at --gpus N)",
            bytes=32 * GiB, block=4096, files=1),
    5: dict(workload="index one 32 GiB synthetic file, 64 KiB blocks (BASELINE configs[4])",
            bytes=32 * GiB, block=65536, files=1),
}


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--config", type=int, default=None, choices=sorted(CONFIGS),
                   help="default: 2 (configs[1]) at --gpus 1, 4 (configs[3], 32 GiB per GPU) at --gpus N > 1")
    p.add_argument("--shard-gib", type=float, default=None, help="override bytes per rank (GiB)")
    p.add_argument("--full", action="store_true",
                   help="after the timed steps also run every side leg and self-check (digest and blocks_hash "
                        "self-checks, CPU baselines, config1, the end-to-end, content-defined-list and default-mode "
                        "legs, e2e_file_multi on the library path; each still subject to its --no-* switch).  Off "
                        "by default: a plain run sets up, warms up, times the steps and prints the line")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps write what the last timed step computed as DIR/<name>.npy (float32 "
                        "or float64, at most 64 MB in all): digests.npy, the digest table's rows (one byte per "
                        "element; a fixed seeded sample of the rows when the table is larger) and "
                        "digest_rows.npy, their row numbers; config 3 also file_hashes.npy, --weak also weak.npy")
    p.add_argument("--cpu-seconds", type=float, default=12.0, help="CPU baseline time budget (--full)")
    p.add_argument("--ramp-s", type=float, default=0.5,
                   help="setup: keep the kernel busy this long before the warmup steps (the chip takes "
                        "~6 launches to ramp its clock from ~1.6 GHz; see DESIGN.md section 4)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-e2e", action="store_true",
                   help="skip the end-to-end leg (the same bytes from a host buffer through sf_index_buffer)")
    p.add_argument("--no-cdc-list", action="store_true",
                   help="skip the content-defined-like list leg (config 2 at N=1: the reference's default block "
                        "shape through the explicit-list kernel, not `value`)")
    p.add_argument("--no-default-mode", action="store_true",
                   help="skip the default-mode leg (config 2 at N=1: the reference's content-defined mode over "
                        "many files on disk through sf_index_fds_blocks, with the stand-in chunker; not `value`)")
    p.add_argument("--no-gather", action="store_true")
    p.add_argument("--gather-root", default="rotate", choices=("rotate", "fixed"),
                   help="rank that receives each step's tables: rotates over the ranks, the last step's being "
                        "rank 0 (files owned round-robin, as a multi-file indexer spreads them), or always 0")
    p.add_argument("--c3-mode", default="stream", choices=("stream", "staged"),
                   help="config 3: 'stream' = batch after batch, each launch also finishing the previous batch's "
                        "blocks_hash (sf_index_device_batch_chained); 'staged' = each batch self-contained "
                        "(sf_index_device_batch: two column halves, the chains' second half alone)")
    p.add_argument("--weak", action="store_true",
                   help="also compute the opt-in fused Adler-32 weak sum per block (not in the reference; "
                        "configs 2 and 5 only); not the headline")
    p.add_argument("--multi-path", default="auto", choices=("auto", "library", "torch"),
                   help="N > 1: 'library' = ONE process drives the N devices through the C-ABI "
                        "(sf_index_device_multi_ex: every shard hashed on its device, the tables gathered to a "
                        "rotating root by RCCL inside the library, as the Rust host would call it); 'torch' = one "
                        "process per GPU over torch.distributed (RCCL).  auto = library at N > 1 (torch for "
                        "--check-launch and gloo rehearsals), the single-GPU path at N = 1; --multi-path library "
                        "at N = 1 runs the library path on one device (SF_TEST_MULTI_SELF_GATHER=1 sends its table "
                        "through RCCL)")
    p.add_argument("--check-plan", action="store_true",
                   help="print the library path's launch plan for --gpus N as JSON and exit (no GPU)")
    p.add_argument("--e2e-multi-gib", type=float, default=1.0,
                   help="library path: GiB per device of the e2e_file_multi leg (a file on disk through "
                        "sf_index_file_multi; 0 = skip)")
    p.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL) or gloo (rehearsal only)")
    p.add_argument("--library-timeout", type=float, default=900.0,
                   help="library path: seconds before a call that never returns (a stuck RCCL exchange) ends "
                        "the process with an error instead of hanging the run")
    p.add_argument("--dist-timeout", type=float, default=300.0,
                   help="seconds before a stuck collective fails the run (init_process_group timeout)")
    p.add_argument("--traffic-file", default=os.path.join(ROOT, "profiles", "traffic.json"))
    p.add_argument("--events", default="auto", choices=("auto", "step", "region"),
                   help="kernel time from HIP events around every step's launch (step) or once around the timed "
                        "steps (region: no event between consecutive launches).  auto = region on one rank "
                        "(a timing event between two launches costs a batch stream's chain loads ~1.5 %%, "
                        "profiles/r03/c3/seq), step with several ranks (the multi block splits kernel time "
                        "from gather waits)")
    p.add_argument("--check-launch", action="store_true",
                   help="launcher check only (no GPU): every rank joins the process group (gloo), rank 0 "
                        "prints the world size it saw and exits")
    return p.parse_args()


def self_launch(a, extra_args=()) -> int:
    """--gpus N without a launcher: run this script under torch.distributed.run
    as a child process (never an exec: the parent only waits), one rank per
    GPU, on a free local port."""
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + sys.argv[1:] + \
        list(extra_args)
    print(f"bench.py: --gpus {a.gpus} without WORLD_SIZE: launching {a.gpus} ranks", file=sys.stderr, flush=True)
    return subprocess.call(cmd)


def multi_block(dist, torch, dev, a, rank, world, kern_ms, waits, roots, backend):
    """The `multi` block of an N > 1 line: every rank's kernel time and how
    long its stream stood waiting for gathers, split by whether the rank was
    the gather's receiving rank (waits[j] is the wait before step j's table
    could be reused, roots[j] that gather's destination).  One all_gather of
    4 numbers per rank."""
    recv = [w for w, r in zip(waits, roots) if r == rank]
    send = [w for w, r in zip(waits, roots) if r != rank]
    mine = torch.tensor([kern_ms, sum(recv) / max(1, len(recv)), sum(send) / max(1, len(send)),
                         float(len(recv))], dtype=torch.float64, device=dev)
    allv = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(allv, mine)
    rows = [v.cpu().tolist() for v in allv]
    k = [r[0] for r in rows]
    return {"world": dist.get_world_size(), "backend": backend,
            "kernel_ms": {"max": round(max(k), 4), "min": round(min(k), 4), "per_rank": [round(x, 4) for x in k]},
            "gather_wait_ms_as_root": [round(r[1], 4) for r in rows],
            "gather_wait_ms_as_sender": [round(r[2], 4) for r in rows],
            "steps_as_root": [int(r[3]) for r in rows],
            "note": "wait = time the rank's stream stood still before reusing a table its gather was still "
                    "reading (HIP events around work.wait()), per gather, averaged"}


def config_block(a, world):
    """The line's `config` object: the workload string of BASELINE.json's
    config, the per-GPU shard and the parallelism (one shard per rank, the
    pipelined gather of the digest tables)."""
    from syncfast_amd.shard import shard_range
    cfg = CONFIGS[a.config]
    bs = cfg["block"]
    per_rank = int(a.shard_gib * GiB) if a.shard_gib else cfg["bytes"]
    per_rank -= per_rank % bs
    total = per_rank * world
    shard = shard_range(total, bs, world, 0)[1]
    gather = world > 1 and not a.no_gather
    backend = "rccl" if a.dist_backend == "nccl" else a.dist_backend
    return {"workload": cfg["workload"], "bytes_per_gpu": shard, "block_size": bs, "total_bytes": total,
            "files": cfg["files"], "blocks": total // bs,
            **({"c3_mode": a.c3_mode} if cfg["files"] > 1 else {}),
            "parallelism": f"shard{world}" + (f"+{backend}_gather(pipelined, root %s)" % (
                "rotating" if a.gather_root == "rotate" else "0") if gather else "")}


def check_launch(a, world, rank, fallback_note=None) -> None:
    """CPU-only rehearsal of the N-rank launch (gloo): every rank joins, the
    world size is checked, and rank 0 prints the `multi` block built from
    stand-in per-rank numbers (the kernel is not run without a GPU) and, after
    a failed library path, the `multi_fallback` note a real line would carry."""
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=a.dist_timeout))
    seen = torch.ones(1)
    dist.all_reduce(seen)
    assert dist.get_world_size() == world == a.gpus and int(seen.item()) == a.gpus, (world, a.gpus, seen)
    roots = [i % world for i in range(a.steps)]
    multi = multi_block(dist, torch, torch.device("cpu"), a, rank, world, float(rank + 1), [0.0] * a.steps, roots,
                        "gloo")
    if rank == 0:
        line = {"launch_check": True, "n_gpus": dist.get_world_size(), "ranks_seen": int(seen.item()),
                "config": config_block(a, world), "multi": multi}
        if fallback_note:
            line["multi_fallback"] = fallback_note
        print(json.dumps(line), flush=True)
    dist.destroy_process_group()


def lib_sha256() -> str:
    """SHA-256 of the HIP library this process runs."""
    from syncfast_amd._lib import LIB_PATH
    h = hashlib.sha256()
    with open(LIB_PATH, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    return h.hexdigest()


def config1_probe():
    """BASELINE configs[0] needs the unmodified Rust indexer (cargo build of
    /root/reference): probe for the toolchain on this host."""
    tools = {t: shutil.which(t) for t in ("cargo", "rustc")}
    cargo_home = os.path.isdir(os.path.expanduser("~/.cargo"))
    runnable = all(tools.values())
    return {"workload": "index a folder with one 64 MiB file, default CDC, unmodified Rust CPU path (BASELINE configs[0])",
            "status": "runnable (not timed here)" if runnable else "reference CPU path not runnable",
            "probe": {**{k: (v or "absent") for k, v in tools.items()}, "~/.cargo": cargo_home},
            "note": None if runnable else "no Rust toolchain on this host; cpu_baseline times the C restatement "
                                          "(scalar, stands in for the sha1 0.6 crate) and cpu_baseline_shani the "
                                          "SHA-NI host code on the same fixed tiling instead; standin_cpu adds the "
                                          "boundary finding with a stand-in chunker (same per-byte work, not the "
                                          "crate's boundaries), default_mode_e2e the drop-in's default splice "
                                          "with that chunker feeding sf_index_fd_blocks"}


CONFIG1_BYTES = 64 << 20  # BASELINE configs[0]: one 64 MiB file (seed 0x5EED0000)


def config1_standin(budget_s):
    """configs[0]'s CPU cost with a STAND-IN chunker (no Rust toolchain, and
    the crate's recurrence is unpinned): the ZPAQ-form
    fragmenter of examples/zpaq_standin.h (13 bits, 32 KiB cap: the crate's
    per-byte table lookup, compare, add and multiply -- NOT its boundaries)
    over the 64 MiB file's bytes, alone and with every block SHA-1'd as it is
    cut (the reference's single pass, src/index.rs:629-647; scalar SHA-1
    standing in for the pure-Rust sha1 0.6 crate, and SHA-NI), one core, in
    memory (SQLite and the file read excluded)."""
    import oracle  # CPU baseline leg: the stand-in chunker + SHA-1 timed on the host
    buf = oracle.splitmix_bytes(CONFIG1_BYTES, SEED)
    res = {}
    for name, fn in (("chunker", lambda: oracle.zpaq_standin_sizes(buf)),
                     ("chunker_sha1_scalar", lambda: oracle.zpaq_standin_index(buf, False)),
                     ("chunker_sha1_shani", lambda: oracle.zpaq_standin_index(buf, True))):
        best, spent, reps = None, 0.0, 0
        while reps < 2 or (spent < budget_s / 3 and reps < 20):
            t0 = time.perf_counter()
            n = len(fn())
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
            spent += dt
            reps += 1
        res[name] = {"GB/s": round(CONFIG1_BYTES / best / 1e9, 4), "ms": round(best * 1e3, 2), "reps": reps}
        res["blocks"] = n
    res.update({"bytes": CONFIG1_BYTES, "cores": 1, "kind": "stand-in",
                "label": "stand-in: same per-byte work as cdchunking's ZPAQ (zpaq's fragmenter form, 13 bits, "
                         "32 KiB cap), not the crate's boundaries; SHA-1 per block in the same pass",
                "source": "examples/zpaq_standin.h via oracle/sf_baseline.cpp (sfb_zpaq_cut, sfb_zpaq_index)"})
    return res


def config1_default_mode_e2e():
    """The drop-in's default mode end to end on configs[0]'s file (not
    `value`): the 64 MiB file written to disk, then the plain-C consumer's -Z
    splice (examples/build/sf_index: ONE open, the stand-in chunker streams the
    open file in 64 KiB reads keeping the (offset, size) list, then
    sf_index_fd_blocks hashes the list from the same descriptor on the GPU),
    three passes in one process (the first pays the library's stage
    allocations), each timed inside the consumer: chunker seconds + hashing
    call seconds.  16 rows re-hashed with the product's host SHA-1."""
    import random
    import tempfile
    from syncfast_amd import host
    exe = os.path.join(ROOT, "examples", "build", "sf_index")
    if not os.access(exe, os.X_OK):
        return {"status": "examples/build/sf_index not built"}
    import numpy as np
    d = tempfile.mkdtemp(prefix="sf_cfg1_")
    path = os.path.join(d, "file64m")
    try:
        import oracle  # input generation only (the same splitmix64 bytes as configs[0])
        raw = oracle.splitmix_bytes(CONFIG1_BYTES, SEED).tobytes()
        with open(path, "wb") as f:
            f.write(raw)
        def run(extra):
            r = subprocess.run([exe, "-Z", "-T"] + extra + [path, path, path], capture_output=True, text=True,
                               timeout=300)
            if r.returncode != 0:
                raise RuntimeError(f"sf_index -Z {' '.join(extra)} failed ({r.returncode}): {r.stderr.strip()[-300:]}")
            times = [json.loads(ln) for ln in r.stderr.splitlines() if ln.startswith("{")]
            rows = []
            for ln in r.stdout.splitlines():
                parts = ln.split()
                if len(parts) == 3 and parts[0].isdigit():
                    rows.append((int(parts[0]), int(parts[1]), parts[2]))
            last = rows[-times[-1]["blocks"]:]
            assert sum(s for _o, s, _h in last) == CONFIG1_BYTES, "e2e rows do not tile the file"
            for o, s, h in random.Random(7).sample(last, min(16, len(last))):
                assert host.sha1(np.frombuffer(raw[o:o + s], np.uint8)).hex() == h, "e2e row self-check failed"
            return times, last
        try:
            times, last = run([])
            ptimes, plast = run(["-p", str(CONFIG1_CUT_THREADS), "-W"])
            ftimes, flast = run(["-p", str(CONFIG1_CUT_THREADS)])
        except RuntimeError as e:
            return {"status": str(e)}
        # the parallel cut is the one-stream cut: same rows, row for row
        assert plast == last, "sf_cut_fd's boundaries differ from the one-stream cut"
        assert flast == last, "sf_index_fd_cut's rows differ from the one-stream route's"
        nb = len(last)
    finally:
        try:
            os.unlink(path)
        except OSError:
            pass
        os.rmdir(d)
    best = min(times[1:] or times, key=lambda t: t["chunk_s"] + t["hash_s"])
    c, h = best["chunk_s"], best["hash_s"]
    pbest = min(ptimes[1:] or ptimes, key=lambda t: t["chunk_s"] + t["hash_s"])
    fbest = min(ftimes[1:] or ftimes, key=lambda t: t["hash_s"])
    pc, ph = pbest["chunk_s"], pbest["hash_s"]
    return {"bytes": CONFIG1_BYTES, "blocks": nb, "passes": len(times),
            "chunker_GB/s": round(CONFIG1_BYTES / c / 1e9, 4), "hash_call_GB/s": round(CONFIG1_BYTES / h / 1e9, 3),
            "e2e_GB/s": round(CONFIG1_BYTES / (c + h) / 1e9, 4), "chunker_share": round(c / (c + h), 4),
            "route": "file (page cache) -> stand-in chunker over the open fd (1 host core, 64 KiB reads) -> "
                     "sf_index_fd_blocks on the same fd (pread windows, H2D, sha1_table_kernel, D2H rows + "
                     "blocks_hash)",
            "parallel_cut": {"threads": CONFIG1_CUT_THREADS, "chunker_GB/s": round(CONFIG1_BYTES / pc / 1e9, 4),
                             "hash_call_GB/s": round(CONFIG1_BYTES / ph / 1e9, 3),
                             "e2e_GB/s": round(CONFIG1_BYTES / (pc + ph) / 1e9, 4),
                             "chunker_share": round(pc / (pc + ph), 4), "rows_equal_one_stream": True,
                             "route": "the same file cut by sf_cut_fd (the stand-in chunker on "
                                      f"{CONFIG1_CUT_THREADS} threads, segments joined to the one-stream "
                                      "boundaries) -> sf_index_fd_blocks on the same fd"},
            "fused_cut": {"threads": CONFIG1_CUT_THREADS, "e2e_GB/s": round(CONFIG1_BYTES / fbest["hash_s"] / 1e9, 4),
                          "rows_equal_one_stream": True,
                          "route": "sf_index_fd_cut: the file read once into pinned memory by the cutting threads, "
                                   "copied to HBM while the segments are cut and joined, the list hashed from HBM"},
            "label": "stand-in chunker: the crate's per-byte work, not its boundaries"}


def config1_index_path_folder(raw_bytes, fused_gbs):
    """configs[0] through the reference's own entry point (not `value`): a
    folder holding the one 64 MiB file, Index.index_path with a NativeChunker
    (the stand-in's sf_chunker_ops on CONFIG1_CUT_THREADS threads): the file
    is at least LARGE_FILE_BYTES, so the walk indexes it through
    sf_index_fd_cut (cut in parallel, read once, hashed on the GPU) and then
    stores its rows (the reference's SQLite schema, one executemany).  Three
    passes, each on a fresh in-memory index; the best is reported, split into
    the native call (host.index_fd_cut, timed by wrapping it) and the rest
    (walk, mtime gate, the SQLite rows).  Rows checked against the one-thread
    cut, 16 of them re-hashed, blocks_hash recomputed."""
    import ctypes as C
    import random
    import tempfile
    import numpy as np
    from syncfast_amd import host
    from syncfast_amd import index as sfindex
    so = os.path.join(ROOT, "examples", "build", "libzpaq_standin.so")
    if not os.path.exists(so):
        return {"status": "examples/build/libzpaq_standin.so not built"}
    zl = C.CDLL(so)
    zl.sf_zpaq_standin_ops.restype = C.c_void_p
    zl.sf_zpaq_standin_ops.argtypes = [C.c_uint, C.c_uint32]
    zl.sf_zpaq_standin_ops_free.argtypes = [C.c_void_p]
    ops = zl.sf_zpaq_standin_ops(13, 32768)
    d = tempfile.mkdtemp(prefix="sf_cfg1_folder_")
    real = host.index_fd_cut
    spent = []

    def timed_cut(*args, **kw):
        t0 = time.perf_counter()
        try:
            return real(*args, **kw)
        finally:
            spent.append(time.perf_counter() - t0)

    try:
        path = os.path.join(d, "file64m")
        with open(path, "wb") as f:
            f.write(raw_bytes)
        host.index_fd_cut = timed_cut
        passes = []
        for _ in range(3):
            idx = sfindex.Index.open_in_memory(chunker=sfindex.NativeChunker(ops, threads=CONFIG1_CUT_THREADS))
            spent.clear()
            t0 = time.perf_counter()
            idx.index_path(d)
            idx.commit()
            wall = time.perf_counter() - t0
            assert len(spent) == 1, "the 64 MiB file did not take sf_index_fd_cut"
            passes.append((wall, spent[0], idx))
        host.index_fd_cut = real
        wall, call, idx = min(passes, key=lambda x: x[0])
        fid, _m, bh = idx.get_file("file64m")
        rows = idx.list_file_blocks(fid)
        with open(path, "rb") as f:
            offs, sizes = host.cut_fd(f.fileno(), ops, 1)
        assert [(o, s) for _h, o, s in rows] == list(zip(offs.tolist(), sizes.tolist())), "rows != one-stream cut"
        raw = np.frombuffer(raw_bytes, np.uint8)
        for h, o, s in random.Random(3).sample(rows, min(16, len(rows))):
            assert host.sha1(raw[o:o + s]) == h.bytes, "index_path row self-check failed"
        assert host.blocks_hash(b"".join(h.bytes for h, _o, _s in rows)) == bh.bytes, "blocks_hash self-check"
        n = len(raw_bytes)
        return {"bytes": n, "blocks": len(rows), "passes": len(passes),
                "e2e_GB/s": round(n / wall / 1e9, 4), "wall_ms": round(wall * 1e3, 2),
                "native_call_GB/s": round(n / call / 1e9, 4), "native_call_ms": round(call * 1e3, 2),
                "rest_ms": round((wall - call) * 1e3, 2),
                "native_call_of_fused_cut": round(n / call / 1e9 / fused_gbs, 4) if fused_gbs else None,
                "rows_equal_one_stream": True,
                "route": "Index.index_path(folder) -> walk + mtime gate -> the file (>= 64 MiB) through "
                         "sf_index_fd_cut on the chunker's threads (read once, cut in parallel, hashed on the GPU) "
                         "-> its rows into the reference's SQLite schema (rest_ms: walk, gate, row inserts)"}
    finally:
        host.index_fd_cut = real
        zl.sf_zpaq_standin_ops_free(ops)
        shutil.rmtree(d, ignore_errors=True)


CONFIG1_CUT_THREADS = 16  # the box's CPU share per GPU

DEFAULT_MODE_TREES = {
    # config 3's shape: 1024 files of 8 MiB (BASELINE configs[2]); a tree of 0-200 KiB files
    "c3_1024x8MiB": [8 << 20] * 1024,
    "small_0_200KiB": "small",
}
SMALL_TREE_BYTES = 1 << 30
PER_FILE_SAMPLE_BYTES = 512 << 20  # the per-file loop is timed on the tree's first ~512 MiB


def _sf_index_run(exe, args, paths, timeout=600):
    r = subprocess.run([exe] + args + paths, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(f"sf_index {' '.join(args)} failed ({r.returncode}): {r.stderr.strip()[-300:]}")
    return r


def _parse_files(out):
    """sf_index's stdout -> {path: (rows or None, blocks_hash hex)}."""
    res, cur, rows = {}, None, None
    for ln in out.splitlines():
        if ln.startswith("file "):
            cur, rows = ln.split()[1], []
        elif ln.startswith("blocks_hash "):
            res[cur] = (rows if rows else None, ln.split()[1])
        elif rows is not None and ln and ln[0].isdigit():
            o, s, h = ln.split()
            rows.append((int(o), int(s), h))
    return res


def default_mode_files(data, budget_threads):
    """Not `value`: the reference's DEFAULT mode over many files on disk
    (index_path -> index_file per file, src/index.rs:685-715 -> 610-659),
    end to end: files in the page cache -> the stand-in chunker (the crate's
    per-byte work, not its boundaries) on 1 and on N host threads, each file
    opened once and cut over its descriptor -> every batch of ~256 MiB of cut
    files through ONE sf_index_fds_blocks call (pread windows into packed
    pinned stages, one sort + one sha1_table_kernel launch per stage, rows +
    blocks_hash) while the threads cut the next batch (examples/build/sf_index
    -Z -M; at N threads the second of two passes in one process is timed, the
    first pays the library's allocations).  Beside it today's per-file loop (sf_index -Z: chunk, then one
    sf_index_fd_blocks call per file), timed on the tree's first ~512 MiB.
    Self-checks: every file's blocks_hash equal across the routes; the first
    and last file's rows re-hashed with the product's host SHA-1."""
    import numpy as np
    import random
    import tempfile
    from syncfast_amd import host
    exe = os.path.join(ROOT, "examples", "build", "sf_index")
    if not os.access(exe, os.X_OK):
        return {"status": "examples/build/sf_index not built"}
    out = {"label": "stand-in chunker: the crate's per-byte work, not its boundaries",
           "route": "files (page cache) -> chunker threads over the open fds -> sf_index_fds_blocks per ~256 MiB "
                    "batch (overlapped with cutting the next) -> rows + blocks_hash",
           "threads_max": budget_threads}
    host_bytes = data.cpu() if data.numel() <= (8 << 30) else data[: 8 << 30].cpu()
    hb = host_bytes.numpy()
    rng = np.random.default_rng(11)
    for name, spec in DEFAULT_MODE_TREES.items():
        d = tempfile.mkdtemp(prefix="sf_dm_")
        try:
            if spec == "small":
                lens, tot = [], 0
                while tot < SMALL_TREE_BYTES:
                    n = int(rng.integers(0, 200 << 10))
                    lens.append(n)
                    tot += n
            else:
                lens = spec
            paths, pos = [], 0
            for k, n in enumerate(lens):
                p = os.path.join(d, f"f{k:05d}")
                a0 = pos % (hb.size - n) if hb.size > n else 0
                hb[a0: a0 + n].tofile(p)
                pos += n + 4099
                paths.append(p)
            total = sum(lens)
            leg = {"files": len(lens), "bytes": total}
            print(f"bench.py: default mode {name}: {len(lens)} files written", file=sys.stderr, flush=True)
            hashes = {}
            for j in (budget_threads, 1):
                # -P 2: the whole run twice in one process, the second timed (the
                # first pays the library's stage allocations and first launches,
                # as a long-lived indexer does once); one pass at one thread
                r = _sf_index_run(exe, ["-Z", "-M", "-q", "-T", "-P", "2" if j > 1 else "1", "-j", str(j)], paths)
                t = [json.loads(ln) for ln in r.stderr.splitlines() if ln.startswith("{")][-1]
                print(f"bench.py: default mode {name}, {j} chunker threads: {t['wall_s']:.3f} s", file=sys.stderr,
                      flush=True)
                res = _parse_files(r.stdout)
                if not hashes:
                    hashes = {p: h for p, (_rows, h) in res.items()}
                    for p in (paths[0], paths[-1]):  # full rows: re-hash them
                        rows = res[p][0] or []
                        raw = np.fromfile(p, np.uint8)
                        assert sum(s for _o, s, _h in rows) == raw.size, "rows do not tile the file"
                        for o, s, h in random.Random(5).sample(rows, min(32, len(rows))):
                            assert host.sha1(raw[o:o + s]).hex() == h, "row self-check failed"
                        dig = np.frombuffer(b"".join(bytes.fromhex(h) for _o, _s, h in rows), np.uint8)
                        assert host.blocks_hash(dig).hex() == res[p][1], "blocks_hash self-check failed"
                assert {p: h for p, (_rows, h) in res.items()} == hashes, "routes disagree on a blocks_hash"
                leg[f"threads_{j}"] = {"e2e_GB/s": round(total / t["wall_s"] / 1e9, 3), "wall_s": round(t["wall_s"], 4),
                                       "hash_call_s": round(t["hash_call_s"], 4),
                                       "chunk_cpu_s": round(t["chunk_cpu_s"], 4),
                                       "wait_for_cut_s": round(t["wait_cut_s"], 4), "batches": t["batches"],
                                       "blocks": t["blocks"], "timed_pass": 2 if j > 1 else 1}
            # today's per-file loop on a sample
            sample, sb = [], 0
            for p, n in zip(paths, lens):
                if sb >= PER_FILE_SAMPLE_BYTES:
                    break
                sample.append(p)
                sb += n
            r = _sf_index_run(exe, ["-Z", "-T"], sample)
            ts = [json.loads(ln) for ln in r.stderr.splitlines() if ln.startswith("{")]
            res = _parse_files(r.stdout)
            assert all(res[p][1] == hashes[p] for p in sample), "per-file loop disagrees on a blocks_hash"
            c = sum(x["chunk_s"] for x in ts)
            h = sum(x["hash_s"] for x in ts)
            leg["per_file_loop"] = {"e2e_GB/s": round(sb / (c + h) / 1e9, 3), "files": len(sample), "bytes": sb,
                                    "chunk_s": round(c, 4), "hash_calls_s": round(h, 4),
                                    "note": "one thread: chunk a file, then one sf_index_fd_blocks call for it"}
            j16 = leg[f"threads_{budget_threads}"]
            leg["chunker_share"] = round(min(1.0, j16["chunk_cpu_s"] / budget_threads / j16["wall_s"]), 4)
            out[name] = leg
        finally:
            shutil.rmtree(d, ignore_errors=True)
    return out


def cpu_baseline(nbytes_total, bs, budget_s):
    """Time the oracle (C, 1 thread) on the leading bytes of the same
    synthetic stream, in 64 MiB pieces, until the time budget is used."""
    import numpy as np
    import oracle  # test infrastructure: used here only as the timed CPU baseline
    piece = 64 << 20
    piece -= piece % bs
    done = 0
    t_hash = 0.0
    while done < nbytes_total and t_hash < budget_s:
        n = min(piece, nbytes_total - done)
        buf = oracle.splitmix_bytes(n, SEED, done)  # generation not timed
        t0 = time.perf_counter()
        _, _, dig = oracle.index_fixed(buf, bs)
        t_hash += time.perf_counter() - t0
        done += n
        del buf, dig
    return {"value": round(done / GiB / t_hash, 4), "unit": "GiB/s", "cores": 1, "kind": "port",
            "sample": f"first {done / GiB:.3f} GiB of the same splitmix64 stream, {bs}-B blocks, "
                      f"oracle/sf_oracle.c SHA-1 (scalar C, no SHA-NI), 1 thread, SQLite excluded"}


def cpu_model() -> str:
    """The host CPU the baselines ran on (/proc/cpuinfo model name, x count)."""
    try:
        names = [ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")]
    except OSError:
        return "unknown"
    return f"{names[0]} (x{len(names)} logical CPUs visible)" if names else "unknown"


E2E_MAX = 8 * GiB  # host RAM bound of the end-to-end leg (config 4 at 256 GiB per GPU would not fit)
CDC_LIST_BYTES = 4 * GiB  # the content-defined-like list leg: scripts/cdc_ab.py's list


def content_defined_list(torch, data, stream, rounds=7, reps=3):
    """Not `value`: the reference's DEFAULT block shape, content-defined
    blocks (cdchunking ZPAQ 13 bits, max 32 KiB, src/index.rs:40-41; the
    boundaries themselves are the host crate's), as an
    explicit list over the shard's first 4 GiB: geometric sizes (mean 8 KiB,
    capped at 32 KiB, byte offsets; scripts/cdc_ab.py's list, seed 7) through
    sf_index_device_blocks (length-class sort + sha1_table_kernel), against
    the same bytes as a 4 KiB list through the same entry point, interleaved,
    HIP events on the launch stream around each round of calls.  64 random
    blocks checked with the product's host SHA-1."""
    import statistics
    import numpy as np
    from syncfast_amd import device, host
    total = min(CDC_LIST_BYTES, data.numel())
    rng = np.random.default_rng(7)
    sz = np.minimum(32768, np.maximum(1, rng.geometric(1 / 8192, size=total // 4096 + 64))).astype(np.int64)
    c = np.cumsum(sz)
    n = int(np.searchsorted(c, total))
    sz = sz[: n + 1]
    sz[-1] -= int(c[n] - total) if c[n] > total else 0
    sz = sz[sz > 0]
    offs = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.int64)
    o4 = np.arange(total // 4096, dtype=np.int64) * 4096
    view = data[:total]
    lists = {"cdc": (offs, sz), "list4k": (o4, np.full(o4.size, 4096, np.int64))}
    dl = {k: (torch.from_numpy(o).to(data.device), torch.from_numpy(z.astype(np.int32)).to(data.device))
          for k, (o, z) in lists.items()}
    outs = {k: torch.empty((lists[k][0].size, 20), dtype=torch.uint8, device=data.device) for k in lists}

    def run(k):
        device.index_device_blocks(view, dl[k][0], dl[k][1], out=outs[k], check_range=False, stream=stream)

    for k in lists:
        run(k)
    t_ramp = time.perf_counter()  # the GPU idled through the self-checks: clock back up first
    while time.perf_counter() - t_ramp < 0.3:
        run("list4k")
        torch.cuda.synchronize()
    torch.cuda.synchronize()
    times = {k: [] for k in lists}
    for r in range(rounds):
        for k in (lists if r % 2 == 0 else reversed(list(lists))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                run(k)
            e1.record(stream)
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / reps)
    d = outs["cdc"].cpu().numpy()
    for j in list(rng.integers(0, offs.size, 64)) + [0, offs.size - 1]:
        b = view[int(offs[j]): int(offs[j]) + int(sz[j])].cpu().numpy()
        assert bytes(d[j]) == host.sha1(b), "content-defined list digest self-check failed"
    med = {k: statistics.median(v) for k, v in times.items()}
    gibs = {k: total / GiB / (med[k] * 1e-3) for k in med}
    alg = total + 20 * int(offs.size)  # every byte read once, 20 B written per block (per call)
    return {"bytes": total, "blocks": int(offs.size), "mean_block": round(total / offs.size, 1),
            "ms_per_call": round(med["cdc"], 4), "GiB/s": round(gibs["cdc"], 1),
            "hbm_frac": round(alg / (med["cdc"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "list4k_GiB/s": round(gibs["list4k"], 1), "of_list4k": round(gibs["cdc"] / gibs["list4k"], 4),
            "entry": "sf_index_device_blocks (sort + sha1_table_kernel per call)",
            "rounds": rounds, "reps": reps}


def e2e_host_buffer(torch, data, dig_host, bs):
    """End to end on the same bytes (not `value`): the shard's first
    E2E_MAX bytes (all of configs 2) copied to a host buffer, then
    sf_index_buffer -- page-locked in place, pipelined H2D + kernel + D2H of
    the rows -- best of two calls, rows checked against the device-resident
    table.  Beside it the raw pinned H2D copy rate (the PCIe ceiling of the
    route)."""
    from syncfast_amd import host
    m = min(data.numel(), E2E_MAX)
    m -= m % bs if m < data.numel() else 0
    hbytes = data[:m].cpu().numpy()
    dig_host = dig_host[:(m + bs - 1) // bs]
    best = None
    for _ in range(2):
        t0 = time.perf_counter()
        rows = host.index_buffer(hbytes, bs)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    assert rows.shape[0] == dig_host.shape[0] and rows["sha1"].tobytes() == dig_host.tobytes(), "e2e rows differ"
    n = hbytes.size
    del hbytes, rows
    pin = torch.empty(1 << 30, dtype=torch.uint8, pin_memory=True)
    dev = torch.empty(1 << 30, dtype=torch.uint8, device=data.device)
    dev.copy_(pin, non_blocking=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(4):
        dev.copy_(pin, non_blocking=True)
    torch.cuda.synchronize()
    h2d = (4 << 30) / (time.perf_counter() - t0)
    return {"value": round(n / GiB / best, 3), "unit": "GiB/s", "gbs": round(n / best / 1e9, 2), "bytes": n,
            "route": "host buffer -> sf_index_buffer (page-locked in place, pipelined H2D + kernel + D2H rows)",
            "pcie_h2d_pinned_gbs": round(h2d / 1e9, 2)}


def cpu_baseline_shani(nbytes_total, bs, budget_s, threads):
    """The same fixed tiling with the product's host SHA-1 (SHA-NI): the
    strongest CPU number for this work, on `threads` cores."""
    import oracle
    piece = ((256 if threads > 1 else 64) << 20)
    piece -= piece % bs
    done, t_hash = 0, 0.0
    while done < nbytes_total and t_hash < budget_s:
        n = min(piece, nbytes_total - done)
        buf = oracle.splitmix_bytes(n, SEED, done)
        t0 = time.perf_counter()
        oracle.index_fixed_shani(buf, bs, threads)
        t_hash += time.perf_counter() - t0
        done += n
    return {"value": round(done / GiB / t_hash, 4), "unit": "GiB/s", "cores": threads, "kind": "port",
            "sample": f"first {done / GiB:.3f} GiB of the same stream, {bs}-B blocks, host SHA-1 with "
                      f"{'SHA-NI' if oracle.has_shani() else 'scalar (no SHA-NI on this CPU)'} "
                      f"(syncfast_amd/csrc/host_sha1.cpp via oracle/sf_baseline.cpp), {threads} thread(s)"}


def cpu_baseline_all_cores(nbytes_total, bs, budget_s):
    """Same port on every host core this process may use (capped at 16, the
    GPU box's CPU share), 256 MiB pieces, bounded by the time budget."""
    import oracle
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    piece = (256 << 20) - ((256 << 20) % bs)
    done, t_hash = 0, 0.0
    while done < nbytes_total and t_hash < budget_s:
        n = min(piece, nbytes_total - done)
        buf = oracle.splitmix_bytes(n, SEED, done)
        t0 = time.perf_counter()
        oracle.index_fixed_mt(buf, bs, threads)
        t_hash += time.perf_counter() - t0
        done += n
    return {"value": round(done / GiB / t_hash, 4), "unit": "GiB/s", "cores": threads, "kind": "port",
            "sample": f"first {done / GiB:.3f} GiB of the same stream, {threads} pthreads"}


def library_plan(a, n):
    """The single-process multi-GPU launch (--multi-path library), computed
    without a GPU (--check-plan; tests/test_bench_launch.py): one logical file
    of n shards (configs[3]: n x 32 GiB at 4 KiB blocks), shard r on device r
    (sf_shard_range = syncfast_amd.shard.shard_range), three rotating scratch
    tables per device, two receive tables per device, used in turn (the gather's root
    rotates: step i of the timed steps goes to device (i - (steps-1)) mod n,
    so the last timed step's table is device 0's), and the rows of each
    device's shard in the root's table (sf_test_multi_plan's offsets)."""
    from syncfast_amd.shard import shard_range
    cfg = CONFIGS[a.config]
    if cfg["files"] > 1:
        raise SystemExit("--multi-path library: configs 2, 4 and 5 (one file)")
    bs = cfg["block"]
    per = int(a.shard_gib * GiB) if a.shard_gib else cfg["bytes"]
    per -= per % bs
    total = per * n
    shards = []
    for r in range(n):
        start, ln = shard_range(total, bs, n, r)
        shards.append({"device": r, "start": start, "bytes": ln, "rows": (ln + bs - 1) // bs,
                       "first_row": start // bs})
    roots_timed = [(i - (a.steps - 1)) % n for i in range(a.steps)]
    return {"path": "library", "n_devices": n, "config": a.config, "workload": cfg["workload"], "block_size": bs,
            "bytes_per_gpu": per, "total_bytes": total, "blocks": total // bs, "shards": shards,
            "scratch_tables_per_device": 3, "receive_tables_per_device": 2, "receive_table_rows": total // bs,
            "roots_warmup": list(range(n)), "roots_timed": roots_timed,
            "entry": "sf_index_device_multi_ex (hash streams + gather streams)"}


def library_main(a, n=None):
    """--multi-path library: ONE process drives n devices through the C-ABI
    (north_star: the host calls the kernels through the C-ABI and gathers with
    RCCL over xGMI).  Per step: sf_index_device_multi_ex hashes shard r on
    device r on its hash stream (sha1_fixed_kernel) and, on the gather
    streams, sends every other shard's table to the step's root (rotating),
    inside the library; the next step's hashing overlaps the previous step's
    exchange (three scratch tables and two receive tables per device, events
    on the gather streams before a table is reused).  value = n x shard bytes x steps / wall time
    of the timed steps (every device synchronised on both sides).  Kernel time
    from HIP events on each device's hash stream around its launch."""
    import threading
    n = a.gpus if n is None else n
    plan = library_plan(a, n)

    def stuck():  # a hang inside the library (RCCL) cannot be interrupted: end the process loudly
        print(f"bench.py: library multi-GPU path still running after {a.library_timeout:.0f} s; exiting",
              file=sys.stderr, flush=True)
        os._exit(3)

    watchdog = threading.Timer(a.library_timeout, stuck)
    watchdog.daemon = True
    watchdog.start()
    try:
        return _library_run(a, n, plan)
    finally:
        watchdog.cancel()


def _library_run(a, n, plan):
    import torch
    import numpy as np
    from syncfast_amd import _lib, device, host
    ndev = torch.cuda.device_count()
    if ndev < n:
        # RuntimeError, not SystemExit: under the driver's torchrun a rank may
        # see only its own GPU, and the caller then falls back to the per-process form
        raise RuntimeError(f"--gpus {n}: only {ndev} device(s) visible to one process")
    bs, total = plan["block_size"], plan["total_bytes"]
    nb_total = plan["blocks"]
    L = _lib.lib()
    devs = [torch.device("cuda", r) for r in range(n)]
    data, digs, tables, hs, gs = [], [], [], [], []
    for r, sh in enumerate(plan["shards"]):
        with torch.cuda.device(devs[r]):
            t = torch.empty(sh["bytes"], dtype=torch.uint8, device=devs[r])
            device.fill_splitmix(t, SEED, sh["start"])
            data.append(t)
            digs.append([torch.empty((max(sh["rows"], 1), 20), dtype=torch.uint8, device=devs[r]) for _ in range(3)])
            tables.append([torch.empty((max(nb_total, 1), 20), dtype=torch.uint8, device=devs[r]) for _ in range(2)])
            hs.append(torch.cuda.Stream(devs[r]))
            gs.append(torch.cuda.Stream(devs[r]))
    for r in range(n):
        torch.cuda.synchronize(devs[r])
    vp = lambda xs: (ctypes.c_void_p * n)(*xs)  # noqa: E731
    shard_p = vp([t.data_ptr() for t in data])
    hs_p, gs_p = vp([s.cuda_stream for s in hs]), vp([s.cuda_stream for s in gs])
    scratch_p = [vp([digs[r][b].data_ptr() for r in range(n)]) for b in range(3)]
    send_ev = [[None] * 3 for _ in range(n)]  # gather stream r past the exchange that read digs[r][b]
    # gather stream r past the last exchange into tables[r][k]: a root's next
    # step hashes into its other table, so it never waits for the exchange
    # just issued (with one table, N = 1 serialised every exchange behind the
    # next step's hashing)
    table_ev = [[None, None] for _ in range(n)]
    uses = [0] * n  # steps each device has been root for (its tables in turn)
    last = [None]  # (root, table) of the last step
    self_gather = n == 1 and _lib.get_knob("SF_TEST_MULTI_SELF_GATHER") != 0
    exchange = n > 1 or self_gather  # else the library only hashes (the table is whole on hs[0])
    kern = [[] for _ in range(n)]  # (e0, e1) per timed step on each hash stream
    gather_ev = []  # (root, root's kernel end, exchange end) per timed step

    def step(i, root, timed):
        b = i % 3
        for r in range(n):
            if send_ev[r][b] is not None:
                hs[r].wait_event(send_ev[r][b])
        k = uses[root] % 2
        uses[root] += 1
        last[0] = (root, k)
        if table_ev[root][k] is not None:
            hs[root].wait_event(table_ev[root][k])
        evs = []
        if timed:
            for r in range(n):
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record(hs[r])
                evs.append(e0)
        _lib.check(L.sf_index_device_multi_ex(n, shard_p, total, bs, scratch_p[b], root, tables[root][k].data_ptr(),
                                              hs_p, gs_p), "sf_index_device_multi_ex")
        if timed:
            for r in range(n):
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record(hs[r])
                kern[r].append((evs[r], e1))
        for r in range(n):
            e = torch.cuda.Event(enable_timing=timed and r == root)
            e.record(gs[r])
            send_ev[r][b] = e
            if r == root:
                table_ev[r][k] = e
                if timed and exchange:
                    gather_ev.append((root, kern[root][-1][1], e))

    def sync_all():
        for r in range(n):
            torch.cuda.synchronize(devs[r])

    for i in range(a.warmup):
        step(i, i % n, False)
    for r in range(n):  # every device once as root (RCCL connects a pair on its first exchange)
        step(r, r, False)
    sync_all()
    # setup (not a step): clock ramp on every device, hashing only
    t_ramp = time.perf_counter()
    while time.perf_counter() - t_ramp < a.ramp_s:
        for r in range(n):
            device.index_device(data[r], bs, out=digs[r][0], stream=hs[r])
        sync_all()
    sync_all()
    roots = plan["roots_timed"]
    t0 = time.perf_counter()
    for i in range(a.steps):
        step(i, roots[i], True)
    sync_all()
    t1 = time.perf_counter()
    t = t1 - t0
    kms = [sum(e0.elapsed_time(e1) for e0, e1 in kern[r]) / a.steps for r in range(n)]
    gms = [e1.elapsed_time(e2) for _root, e1, e2 in gather_ev]

    # self-check: the last step's table (device 0's) against every shard's
    # first and last block (product host SHA-1) and, for the other devices,
    # against their scratch table of that step
    # (--full only, as the host blocks_hash stage and the e2e_file_multi leg)
    b_last = (a.steps - 1) % 3
    assert last[0][0] == roots[-1]
    tab = tables[last[0][0]][last[0][1]][:nb_total]
    for r, sh in enumerate(plan["shards"]):
        if not a.full or not sh["rows"]:
            continue
        rows = tab[sh["first_row"]: sh["first_row"] + sh["rows"]].cpu().numpy()
        first = data[r][:bs].cpu().numpy()
        lastb = data[r][(sh["rows"] - 1) * bs:].cpu().numpy()
        assert bytes(rows[0]) == host.sha1(first) and bytes(rows[-1]) == host.sha1(lastb), f"device {r} digests"
        if r != roots[-1]:
            assert np.array_equal(rows, digs[r][b_last][: sh["rows"]].cpu().numpy()), f"device {r} gather"
    if a.dump_outputs:  # the last timed step's table, as its root received it
        dump_outputs(torch, a.dump_outputs, tab)
    bh_ms = None
    if a.full:
        full = tab.cpu().numpy()
        tb = time.perf_counter()
        host.blocks_hash(full)
        bh_ms = (time.perf_counter() - tb) * 1e3
        del full

    e2e = None
    if a.full and a.e2e_multi_gib > 0 and not a.no_e2e:
        try:  # a side leg: its failure (a full /tmp) must not cost the measured line
            e2e = e2e_file_multi(data, n, bs, a.e2e_multi_gib)
        except Exception as e:  # noqa: BLE001
            e2e = {"status": f"failed: {type(e).__name__}: {e}"[:300]}
    per = plan["bytes_per_gpu"]
    kmax = max(kms)
    alg = (per // bs) * (bs + 20)  # per device: read every byte once + write 20 B per block
    achieved = alg / (kmax * 1e-3) / 1e9
    gibs = total / GiB / (t / a.steps)
    from syncfast_amd._lib import FIXED_KERNEL, code_object_sha256, kernel_code_sha256
    kcode = kernel_code_sha256(symbol=FIXED_KERNEL)
    traffic = None
    try:
        with open(a.traffic_file) as f:
            ent = json.load(f).get(f"config{a.config}", {})
        if ent.get("shard_bytes") == per and ent.get("kernel_code_sha256") == kcode:
            traffic = ent["hbm_bytes_per_launch"]
    except (OSError, ValueError):
        pass
    line = {
        "metric": "GiB/s indexed (device-resident), %d KiB blocks" % (bs // 1024),
        "value": round(gibs, 3),
        "unit": "GiB/s",
        "n_gpus": n,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": round(t / a.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic (splitmix64 bytes generated in HBM, seed 0x5EED0000)",
        "config": {"workload": plan["workload"], "bytes_per_gpu": per, "block_size": bs, "total_bytes": total,
                   "files": 1, "blocks": nb_total,
                   "parallelism": f"shard{n}+rccl_gather(one process, sf_index_device_multi_ex, root rotating)"},
        "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                     "kernel": "sha1_fixed_kernel<128>", "kernel_ms": round(kmax, 4), "alg_bytes_per_launch": alg},
        "valu_roofline": {"bound": "valu", "achieved": round(per / (kmax * 1e-3) / 1e9, 1),
                          "peak": round(valu_ceiling_gbs(bs), 1), "unit": "GB/s of input",
                          "frac": round(per / (kmax * 1e-3) / 1e9 / valu_ceiling_gbs(bs), 4)},
        "cpu_baseline": None,
        "multi": {"path": "library", "world": n, "self_gather": self_gather,
                  "kernel_ms": {"max": round(kmax, 4), "min": round(min(kms), 4),
                                "per_device": [round(x, 4) for x in kms]},
                  "gather_ms_after_root_kernel": {"mean": round(sum(gms) / max(1, len(gms)), 4),
                                                  "max": round(max(gms) if gms else 0.0, 4)},
                  "steps_as_root": [roots.count(r) for r in range(n)],
                  "note": "one process; per step sf_index_device_multi_ex: hashing on each device's hash stream, "
                          "the tables sent to the step's root on the gather streams (grouped RCCL send/recv inside "
                          "the library), overlapped with the next step's hashing; gather_ms = from the root's "
                          "kernel end to its last receive"},
        "lib_sha256": lib_sha256(),
        "code_object_sha256": code_object_sha256(),
        "kernel_code_sha256": kcode,
        "events": "step",
        "full": a.full,  # false: the self-checks, blocks_hash_host_ms and e2e_file_multi are not run (null)
        "hbm_frac_of_peak": round(per / (t / a.steps) / 1e9 / HBM_PEAK_GBS, 4),
        "blocks_hash_host_ms": round(bh_ms, 2) if bh_ms is not None else None,
        "e2e_file_multi": e2e,
    }
    print(json.dumps(line), flush=True)
    return line


def e2e_file_multi(data, n, bs, gib_per_device):
    """Not `value`: one file on disk (page cache) through sf_index_file_multi:
    shard r read with pread and hashed on device r by a host thread of its
    own (its own PCIe link), rows in file order, blocks_hash over all of them
    on the host.  The file is n x gib_per_device GiB, written from device 0's
    bytes; best of two calls; the first and last row checked."""
    import tempfile
    import numpy as np
    from syncfast_amd import host
    per = int(gib_per_device * GiB)
    per -= per % bs
    chunk = data[0][: min(per, data[0].numel())].cpu().numpy()
    d = tempfile.mkdtemp(prefix="sf_multi_")
    path = os.path.join(d, "file")
    try:
        with open(path, "wb") as f:
            left = per * n
            while left > 0:
                k = min(left, chunk.size)
                chunk[:k].tofile(f)
                left -= k
        size = os.path.getsize(path)
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            rows, bh = host.index_file_multi(path, bs, n)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        with open(path, "rb") as f:
            first = np.frombuffer(f.read(min(bs, size)), np.uint8)
            f.seek((len(rows) - 1) * bs)
            last = np.frombuffer(f.read(), np.uint8)
        assert len(rows) == (size + bs - 1) // bs
        assert bytes(rows["sha1"][0]) == host.sha1(first) and bytes(rows["sha1"][-1]) == host.sha1(last)
        del rows
    finally:
        try:
            os.unlink(path)
        except OSError:
            pass
        os.rmdir(d)
    return {"bytes": size, "devices": n, "GB/s": round(size / best / 1e9, 2), "s": round(best, 4),
            "route": "file (page cache) -> sf_index_file_multi: shard r read (pread pool) and hashed on device r by "
                     "a host thread of its own -> rows in file order + blocks_hash on the host"}


def torchrun_library(a):
    """The driver's N-rank torchrun with the library path: rank 0 drives all
    N devices in one process; the other ranks never touch a GPU and wait in a
    CPU (gloo) group.  If rank 0's library path fails, every rank runs the
    per-process torch.distributed form instead (the line says so)."""
    import torch
    import torch.distributed as dist
    world = int(os.environ["WORLD_SIZE"])
    rank = int(os.environ.get("RANK", "0"))
    if a.gpus != world:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=max(a.dist_timeout, 3600.0)))
    err = ""
    if rank == 0:
        try:
            library_main(a)
        except (Exception, SystemExit) as e:  # noqa: BLE001 -- the per-process form measures instead
            err = f"{type(e).__name__}: {e}"[:500] or "failed"
            print(f"bench.py: library multi-GPU path failed ({err}); every rank runs the per-process form",
                  file=sys.stderr, flush=True)
        if err:  # the failed path's tensors are unreferenced once its frames are gone
            import gc
            gc.collect()
            torch.cuda.empty_cache()
    box = [err]
    dist.broadcast_object_list(box, src=0)
    dist.barrier()
    dist.destroy_process_group()
    if box[0]:
        a.multi_path = "torch"
        return torch_main(a, box[0])


def resolve_args(a):
    """Defaults that depend on --gpus: the config (configs[1] on one GPU,
    configs[3]'s 32 GiB shard per GPU on N > 1) and the multi-GPU path."""
    if a.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if a.config is None:
        a.config = 2 if a.gpus == 1 else 4
    if a.multi_path == "auto":
        rehearsal = a.check_launch or a.dist_backend != "nccl"
        a.multi_path = "library" if a.gpus > 1 and not rehearsal else "torch"
    return a


def main():
    a = resolve_args(parse())
    if a.check_plan:
        print(json.dumps(library_plan(a, a.gpus)), flush=True)
        return
    if a.multi_path == "library":
        if "WORLD_SIZE" in os.environ:  # the driver's torchrun: rank 0 drives every device
            return torchrun_library(a)
        try:
            return library_main(a)
        except (Exception, SystemExit) as e:  # noqa: BLE001 -- reported, then the per-process form measures instead
            if a.gpus == 1:
                raise
            msg = f"{type(e).__name__}: {e}"
            print(f"bench.py: library multi-GPU path failed ({msg}); falling back to one process per GPU",
                  file=sys.stderr, flush=True)
            a.multi_path = "torch"
            os.environ["SF_BENCH_FALLBACK"] = msg[:500]
            sys.exit(self_launch(a, ["--multi-path", "torch"]))
    return torch_main(a, os.environ.get("SF_BENCH_FALLBACK"))


def torch_main(a, fallback_note=None):
    """One process per GPU over torch.distributed (the --multi-path torch
    form, and the single-GPU line)."""
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        sys.exit(self_launch(a))  # before any torch.cuda / HIP call in this process
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    if a.events == "auto":
        a.events = "region" if world == 1 else "step"
    if a.check_launch:
        return check_launch(a, world, rank, fallback_note)

    import torch
    import torch.distributed as dist
    from syncfast_amd import device, host
    from syncfast_amd.shard import gather_digests, shard_range

    ndev = torch.cuda.device_count()  # does not initialise the GPU
    if ndev == 0:
        raise SystemExit("bench.py needs a ROCm device (syncfast_amd has no CPU path)")
    if a.dist_backend == "nccl" and local >= ndev:
        raise SystemExit(f"rank {rank}: local rank {local} but only {ndev} GPU(s): RCCL needs one GPU per rank "
                         f"(use --dist-backend gloo for a shared-GPU rehearsal)")
    dev = torch.device("cuda", local % ndev)  # % only for gloo rehearsals on fewer GPUs than ranks
    torch.cuda.set_device(dev)
    distributed = world > 1
    if distributed:
        tmo = datetime.timedelta(seconds=a.dist_timeout)  # a stuck gather fails the run, never hangs it
        if a.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=tmo)
        else:
            dist.init_process_group(a.dist_backend, timeout=tmo)
        # every rank joined and the communicator carries data: N ranks, N ones
        ones = torch.ones(1, device=dev) if a.dist_backend == "nccl" else torch.ones(1)
        dist.all_reduce(ones)
        if dist.get_world_size() != a.gpus or int(ones.item()) != a.gpus:
            raise SystemExit(f"process group has {dist.get_world_size()} ranks ({int(ones.item())} answered), "
                             f"--gpus {a.gpus}")

    cfg = CONFIGS[a.config]
    bs = cfg["block"]
    per_rank = int(a.shard_gib * GiB) if a.shard_gib else cfg["bytes"]
    per_rank -= per_rank % bs
    total = per_rank * world  # one logical file, weak scaling: per-GPU bytes fixed
    start, shard = shard_range(total, bs, world, rank)
    nblk = shard // bs

    # Synthetic input, generated in HBM: rank r holds bytes [start,
    # start+shard) of one logical file (seed SEED).
    data = torch.empty(shard, dtype=torch.uint8, device=dev)
    device.fill_splitmix(data, SEED, start)
    # Rotating digest tables: step i writes table i%nbuf while the gathers of
    # earlier steps' tables are still in flight (RCCL runs on its own stream).
    # With a gather, three, so a gather may run into step i+2 without stalling
    # it (simulated on one GPU, scripts/gather_sim.py: 2, 3 and 4 tables all
    # cost rank 0 the same +3.7 %, the receive traffic itself).
    gather = distributed and not a.no_gather
    nbuf = 3 if (gather or (cfg["files"] > 1 and a.c3_mode == "stream")) else 2  # split chains read batch i-2's table
    digs = [torch.empty((nblk, 20), dtype=torch.uint8, device=dev) for _ in range(nbuf)]
    files = None
    if cfg["files"] > 1:
        flen = shard // cfg["files"]
        files = [(i * flen, flen) for i in range(cfg["files"])]
    fhash = torch.empty((len(files), 20), dtype=torch.uint8, device=dev) if files else None
    status = torch.zeros(1, dtype=torch.int32, device=dev)  # staged batch: never written since round 6 (no waits)
    if a.weak and files is not None:
        raise SystemExit("--weak applies to configs 2 and 5")
    weaks = [torch.empty(nblk, dtype=torch.int32, device=dev) for _ in range(nbuf)] if a.weak else None
    torch.cuda.synchronize()

    stream = torch.cuda.current_stream(dev)
    bstream = device.BatchStream(len(files), flen, bs, stream=stream) if files and a.c3_mode == "stream" else None
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
    # gather waits: events on the launch stream around work.wait() of every
    # timed step's gather (multi block), with that gather's receiving rank
    wait_ev, wait_root = [], []
    pending = [None] * nbuf
    last_table = [None]
    last_hashes = [None]  # batch stream: blocks_hash of the latest finished batch

    def root(i, timed):
        # The rank that receives step i's tables (the owner of that step's
        # logical file: it writes the rows and computes blocks_hash).  With a
        # fixed root that rank takes (N-1) tables every step and runs ~3.7 %
        # behind the others (scripts/gather_sim.py), which the max-over-ranks
        # clock charges to the whole job; rotating spreads the receive load,
        # and the last timed step's root is rank 0, which checks its table.
        if a.gather_root == "fixed":
            return 0
        return ((i - (a.steps - 1)) if timed else i) % world

    def wait_gather(b, timed):
        work, finish, j, r = pending[b]
        if timed and j >= 0:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            work.wait()
            e1.record(stream)
            wait_ev.append((e0, e1))
            wait_root.append(r)
        else:
            work.wait()
        last_table[0] = finish  # concatenated only once, after the timed loop
        pending[b] = None

    def step(i, timed):
        b = i % nbuf
        if pending[b] is not None:  # the gather that reads digs[b] must be done
            wait_gather(b, timed)
        if timed and (a.events == "step" or i == 0):
            ev[i][0].record(stream)
        if weaks is not None:
            device.index_device_weak(data, bs, out=digs[b], weak_out=weaks[b], stream=stream)
        elif files is None:
            device.index_device(data, bs, out=digs[b], stream=stream)
        elif bstream is not None and timed and i == a.steps - 1:
            # the last batch: two column halves, then its chains' second half
            # (inside the timed region)
            fin = bstream.push_last(data, digs[b])
            if fin:
                last_hashes[0] = fin[-1]
        elif bstream is not None:
            h = bstream.push(data, digs[b])
            if h is not None:
                last_hashes[0] = h
        else:
            device.index_device_batch(data, files, bs, file_hashes=True, out=digs[b], hashes_out=fhash,
                                      stream=stream, status=status)
        if timed and a.events == "step":
            ev[i][1].record(stream)
        if gather:
            r = root(i, timed)
            pending[b] = gather_digests(digs[b], total, bs, dst=r, async_op=True) + ((i if timed else -1), r)

    def drain(timed=False):
        # in step order, so last_table ends as the last step's gather (rank 0's)
        for b in sorted((b for b in range(nbuf) if pending[b] is not None), key=lambda b: pending[b][2]):
            wait_gather(b, timed)

    for i in range(a.warmup):
        step(i, False)
    if bstream is not None:
        bstream.finish()
    drain()
    if gather and a.gather_root == "rotate":
        # RCCL connects a pair of ranks on its first exchange: one gather to
        # every root here (untimed), so no timed step pays for a connection
        for r in range(world):
            gather_digests(digs[0], total, bs, dst=r)
    # Setup (not a step): clock ramp, untimed, no gather -- after the warmup,
    # so that every config's timed steps follow the same busy GPU (a batch
    # stream's warmup ends with its light finish launches).
    t_ramp = time.perf_counter()
    while time.perf_counter() - t_ramp < a.ramp_s:
        if weaks is not None:
            device.index_device_weak(data, bs, out=digs[0], weak_out=weaks[0], stream=stream)
        else:
            device.index_device(data, bs, out=digs[0], stream=stream)
        torch.cuda.synchronize()
    torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        step(i, True)
    if bstream is not None:  # the last batches' blocks_hash: inside the timed region
        fin = bstream.finish()
        if fin:
            last_hashes[0] = fin[-1]
    if a.events == "region":  # one interval over every timed launch (and the batch stream's finish)
        ev[0][1].record(stream)
    drain(True)
    torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    t1 = time.perf_counter()
    elapsed = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    if a.events == "step":
        kern_ms = sum(s.elapsed_time(e) for s, e in ev) / a.steps
    else:
        kern_ms = ev[0][0].elapsed_time(ev[0][1]) / a.steps
    kt = torch.tensor([kern_ms], dtype=torch.float64, device=dev)
    if distributed:
        if a.dist_backend == "gloo":
            elapsed, kt = elapsed.cpu(), kt.cpu()
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
        dist.all_reduce(kt, op=dist.ReduceOp.MAX)
    t = float(elapsed.item())
    multi = None
    if distributed:
        waits = [e0.elapsed_time(e1) for e0, e1 in wait_ev]
        multi = multi_block(dist, torch, dev if a.dist_backend == "nccl" else torch.device("cpu"), a, rank, world,
                            kern_ms, waits, wait_root, "rccl" if a.dist_backend == "nccl" else a.dist_backend)
    kern_ms = float(kt.item())
    dig = digs[(a.steps - 1) % nbuf]
    gathered = last_table[0]() if last_table[0] is not None else None

    d = None
    if a.full:
        if int(status.item()) != 0:
            raise SystemExit(f"staged batch status word changed to {int(status.item())} (it is never written)")
        # Self-check (product host SHA-1): first and last block of this shard.
        d = dig.cpu().numpy()
        first = data[:bs].cpu().numpy()
        lastb = data[(nblk - 1) * bs:].cpu().numpy()
        assert bytes(d[0]) == host.sha1(first) and bytes(d[-1]) == host.sha1(lastb), "digest self-check failed"
        if files is not None:  # the last batch's per-file blocks_hash (device) vs the host SHA-1 of its rows
            per_file = d.reshape(len(files), -1, 20)
            fh = (last_hashes[0] if bstream is not None else fhash).cpu().numpy()
            for f in (0, len(files) - 1):
                assert bytes(fh[f]) == host.blocks_hash(per_file[f]), "blocks_hash self-check failed"

    if rank != 0:
        if distributed:
            dist.destroy_process_group()
        return

    if gather and gathered is None:
        raise SystemExit("rank 0 received no table from the last step's gather")
    if a.full and gathered is not None:  # rank 0 owns the whole file's table, rank order
        assert gathered.shape[0] == total // bs and torch.equal(gathered[:nblk].to(dig.device), dig)

    if a.dump_outputs:  # the last timed step's table (rank 0's gathered one at N > 1) and what came with it
        dump_outputs(torch, a.dump_outputs, gathered if gathered is not None else dig,
                     file_hashes=None if files is None else (last_hashes[0] if bstream is not None else fhash),
                     weak=weaks[(a.steps - 1) % nbuf] if weaks is not None and gathered is None else None)

    # Host stage of the single-file path: blocks_hash over all digests
    # (sequential SHA-1, reported separately, not in `value`).
    bh_ms = None
    if a.full and files is None:
        full = gathered.cpu().numpy() if gathered is not None else d
        tb = time.perf_counter()
        host.blocks_hash(full)
        bh_ms = (time.perf_counter() - tb) * 1e3

    total_bytes = total
    gibs = total_bytes / GiB / (t / a.steps)
    alg_bytes = nblk * (bs + 20)  # read every byte once + write 20 B/block
    if files is not None:  # + per-file blocks_hash kernel: re-read the digests, write 20 B/file
        alg_bytes += nblk * 20 + len(files) * 20
    if weaks is not None:  # + 4 B weak sum written per block
        alg_bytes += nblk * 4
    achieved = alg_bytes / (kern_ms * 1e-3) / 1e9
    # PMC traffic of the same kernel (same machine code of the headline
    # kernel; else null: numbers from other code are stale).
    from syncfast_amd._lib import CHAINED_KERNEL, FIXED_KERNEL, code_object_sha256, kernel_code_sha256
    traffic = None
    build = lib_sha256()
    kernels = code_object_sha256()
    kcode = kernel_code_sha256(symbol=CHAINED_KERNEL if bstream is not None else FIXED_KERNEL)
    try:
        with open(a.traffic_file) as f:
            tr = json.load(f)
        key = f"config{a.config}"
        ent = tr.get(key, {})
        if ent.get("shard_bytes") == shard and ent.get("kernel_code_sha256") == kcode and not a.weak:
            traffic = ent["hbm_bytes_per_launch"]
    except (OSError, ValueError):
        pass
    # Everything below the line's own figures runs under --full only.
    cdc = None
    if a.full and not a.no_cdc_list and world == 1 and files is None and weaks is None and a.config == 2:
        cdc = content_defined_list(torch, data, stream)
    e2e = None
    if a.full and not a.no_e2e and world == 1 and files is None and weaks is None:
        e2e = e2e_host_buffer(torch, data, d, bs)
    dmode = None
    if a.full and not a.no_default_mode and world == 1 and files is None and weaks is None and a.config == 2:
        dmode = default_mode_files(data, max(1, min(16, len(os.sched_getaffinity(0)))))
    cpu = cpu_all = cpu_ni = cpu_ni_all = None
    config1 = config1_probe() if a.full and world == 1 else None
    if a.full and not a.no_cpu_baseline and world == 1:
        threads = max(1, min(16, len(os.sched_getaffinity(0))))
        cpu = cpu_baseline(shard, bs, a.cpu_seconds)
        cpu_all = cpu_baseline_all_cores(shard, bs, a.cpu_seconds / 4)
        cpu_ni = cpu_baseline_shani(shard, bs, a.cpu_seconds / 4, 1)
        cpu_ni_all = cpu_baseline_shani(shard, bs, a.cpu_seconds / 4, threads)
        config1["standin_cpu"] = config1_standin(a.cpu_seconds / 4)
        config1["default_mode_e2e"] = config1_default_mode_e2e()
        try:
            import oracle  # input generation only (configs[0]'s bytes)
            raw = oracle.splitmix_bytes(CONFIG1_BYTES, SEED).tobytes()
            fused = (config1["default_mode_e2e"].get("fused_cut") or {}).get("e2e_GB/s")
            config1["index_path_folder"] = config1_index_path_folder(raw, fused)
        except Exception as e:  # noqa: BLE001 -- a side leg: reported, the line stands
            config1["index_path_folder"] = {"status": f"failed: {type(e).__name__}: {e}"[:300]}

    line = {
        "metric": "GiB/s indexed (device-resident), %d KiB blocks" % (bs // 1024)
                  + (" + opt-in Adler-32 weak sum" if weaks is not None else ""),
        "value": round(gibs, 3),
        "unit": "GiB/s",
        "n_gpus": world,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": round(t / a.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic (splitmix64 bytes generated in HBM, seed 0x5EED0000)",
        "config": config_block(a, world),
        "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                     "kernel": ("sha1_fixed_chained_kernel<128>" if bstream is not None else
                                "sha1_fixed_chained_kernel<128> x2 + sha1_chain_helper_kernel" if files else
                                "sha1_fixed_kernel<128%s>" % (", 1, true" if weaks is not None else "")),
                     "kernel_ms": round(kern_ms, 4),
                     "alg_bytes_per_launch": alg_bytes},
        "valu_roofline": None if weaks is not None else {
            "bound": "valu", "achieved": round(total_bytes / world / (kern_ms * 1e-3) / 1e9, 1),
            "peak": round(valu_ceiling_gbs(bs), 1), "unit": "GB/s of input",
            "frac": round(total_bytes / world / (kern_ms * 1e-3) / 1e9 / valu_ceiling_gbs(bs), 4),
            "model": "613 VALU per 64-B SHA-1 compression (400 at 4 + 213 at 2 SIMD-cycles), 1024 SIMDs at 2.4 GHz; "
                     "the chip holds ~2.1 GHz under this load (DESIGN.md section 4)"},
        "cpu_baseline": cpu,
        "cpu_model": cpu_model() if cpu is not None else None,  # state the CPU model
        "cpu_baseline_all_cores": cpu_all,
        "cpu_baseline_shani": cpu_ni,
        "cpu_baseline_shani_all_cores": cpu_ni_all,
        "config1": config1,
        "lib_sha256": build,
        "code_object_sha256": kernels,
        "kernel_code_sha256": kcode,
        "events": a.events,
        "full": a.full,  # false: the fields of the side legs and self-checks are null (not run)
        "multi": multi,
        "hbm_frac_of_peak": round(total_bytes / world / (t / a.steps) / 1e9 / HBM_PEAK_GBS, 4),
        "blocks_hash_host_ms": round(bh_ms, 2) if bh_ms is not None else None,
        "e2e_host_buffer": e2e,
        "content_defined_list": cdc,
        "default_mode_files": dmode,
    }
    if fallback_note:
        line["multi_fallback"] = ("the single-process library path (sf_index_device_multi_ex) failed, this line is "
                                  "the per-process torch.distributed form: " + fallback_note)
    print(json.dumps(line), flush=True)
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
