"""A dict model of sf_plan_copies_device (include/syncfast_amd.h): the classes,
the jobs and the counts, block by block in plain Python over plain lists, and
the cases the plan's tests share.

Test helper (a plain module, imported like want_expect.py).  The model reads
the header's table of classes top to bottom; hashlib stands for the explicit-
list kernel."""
import hashlib

import numpy as np

U64 = 1 << 64
NOT_LOADED = U64 - 1
CLASSES = ("missing", "size_mismatch", "stale", "unavailable", "empty", "candidate")
COUNTS = ("jobs", "bytes", "missing", "size_mismatch", "stale", "unavailable", "unverified", "empty")
ERANGE = "erange"


def classify(r, size, t_size, t_offset, l_size, l_base):
    """The first class of the header's table that applies (r in the table,
    its file among the local files)."""
    if r < 0:
        return "missing"
    if t_size != size:
        return "size_mismatch"
    if t_offset + size > l_size:
        return "stale"
    if l_base == NOT_LOADED:
        return "unavailable"
    if size == 0:
        return "empty"
    return "candidate"


def plan_model(digests, sizes, offsets, rows, block_file, file_base, table_file, table_offset, table_size,
               local_size, local_base=None, src=None):
    """What the call computes, or ERANGE.  ``local_base`` None: a query (no
    file is unavailable, nothing is verified); ``src`` None: no verification.
    Returns a dict: cls (per block, with "job" / "unverified" in place of
    "candidate"), present, ask, dst, jobs [(src, dst, size, block)],
    local_jobs, counts (in COUNTS' order), candidates (how many were hashed)."""
    n, query = len(sizes), local_base is None
    verify = src is not None and not query
    cls, dst, jobs = [], [], []
    local_jobs = [0] * len(local_size)
    counts = dict.fromkeys(COUNTS, 0)
    hashed = 0
    for i in range(n):
        r, f = rows[i], block_file[i]
        if f >= len(file_base) or file_base[f] + offsets[i] >= U64:
            return ERANGE
        dst.append(file_base[f] + offsets[i])
        if r >= len(table_file):
            return ERANGE
        if r < 0:
            c = "missing"
        else:
            j = table_file[r]
            if j >= len(local_size):
                return ERANGE
            base = 0 if query else local_base[j]
            c = classify(r, sizes[i], table_size[r], table_offset[r], local_size[j], base)
            if c == "candidate":
                at = base + table_offset[r]
                if verify and (at >= U64 or at + sizes[i] > len(src)):
                    return ERANGE
                if verify:
                    hashed += 1
                    same = hashlib.sha1(bytes(src[at:at + sizes[i]])).digest() == bytes(digests[i])
                    c = "job" if same else "unverified"
                else:
                    c = "job"
                if c == "job":
                    jobs.append((at % U64, dst[i], sizes[i], i))
                    local_jobs[j] += 1
                    counts["bytes"] += sizes[i]
        cls.append(c)
        if c != "job":
            counts[c] += 1
    counts["jobs"] = len(jobs)
    present = [int(c in ("job", "empty")) for c in cls]
    return dict(cls=cls, present=present, ask=[1 - p for p in present], dst=dst, jobs=jobs, local_jobs=local_jobs,
                counts=[counts[k] for k in COUNTS], candidates=hashed)


KINDS = ("missing", "size_mismatch", "stale", "unavailable", "empty", "unverified", "job")


def mixed_case(seed, n, kinds=None, n_local=3):
    """n blocks over two sections, each found (or not) in a table row of its
    own; the rows lie, in shuffled order, in n_local local files of one arena,
    the last of which is not loaded when there is more than one.  ``kinds``:
    what block i is made to be (a name of KINDS, cycled; default: KINDS in
    order, so every class occurs from 7 blocks on; "unverified" is a block
    whose announced digest differs from its local bytes' in one bit -- a job
    without verification).  Returns the model's keyword arguments."""
    rng = np.random.default_rng(seed)
    kinds = kinds or KINDS
    sizes_l = [int(rng.integers(600, 900)) for _ in range(n_local)]
    base_l, at = [], 0
    for j in range(n_local):
        base_l.append(at)
        at += (sizes_l[j] + 255) // 256 * 256
    src = rng.integers(0, 256, at, dtype=np.uint8)
    loaded = n_local
    if n_local > 1:
        base_l[-1], loaded = NOT_LOADED, n_local - 1
    n_table = n + 5
    perm = rng.permutation(n_table).tolist()
    t_file = [int(rng.integers(0, loaded)) for _ in range(n_table)]
    t_size = [int(rng.integers(1, 200)) for _ in range(n_table)]
    t_off = [int(rng.integers(0, sizes_l[t_file[r]] - t_size[r] + 1)) for r in range(n_table)]
    rows, sizes, digests = [], [], []
    for i in range(n):
        kind, r = kinds[i % len(kinds)], perm[i]
        if kind == "unavailable" and n_local == 1:
            kind = "job"
        if kind == "missing":
            rows.append(-1 - int(rng.integers(0, 3)))
            sizes.append(int(rng.integers(0, 200)))
            digests.append(rng.integers(0, 256, 20, dtype=np.uint8).tobytes())
            continue
        if kind == "unavailable":
            t_file[r] = n_local - 1
            t_off[r] = int(rng.integers(0, sizes_l[-1] - t_size[r] + 1))
        elif kind == "stale":  # the row ends one byte past its file
            t_off[r] = sizes_l[t_file[r]] - t_size[r] + 1
        elif kind == "empty":
            t_size[r] = 0
        size = t_size[r] + (kind == "size_mismatch")
        j = t_file[r]
        b = 0 if base_l[j] == NOT_LOADED else base_l[j]
        digest = hashlib.sha1(src[b + t_off[r]: b + t_off[r] + size].tobytes()).digest()
        if kind == "unverified":
            digest = bytes([digest[0] ^ 1]) + digest[1:]
        rows.append(r)
        sizes.append(size)
        digests.append(digest)
    split = n // 2
    block_file = [0] * split + [1] * (n - split)
    offsets, run = [], 0
    for i in range(n):
        if i == split:
            run = 0
        offsets.append(run)
        run += sizes[i]
    file_base = [0, (sum(sizes[:split]) + 255) // 256 * 256]
    return dict(digests=digests, sizes=sizes, offsets=offsets, rows=rows, block_file=block_file, file_base=file_base,
                table_file=t_file, table_offset=t_off, table_size=t_size, local_size=sizes_l, local_base=base_l,
                src=src.tobytes())
