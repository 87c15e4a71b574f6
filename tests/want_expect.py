"""What the destination's request run and its BLOCK_DATA join must give, from
wire.write_message and a plain dict model alone (shared by test_want_capi.py
and test_gpu_want.py; no code under test), and the input of the end-to-end
test with the properties that test needs."""
import random

from syncfast_amd import wire


def expected_requests(digests, rows=None, take=None, distinct=False) -> bytes:
    """write_message("GetBlock", d) over the asking rows in row order; with
    `distinct`, over the first asking row of each digest."""
    out, seen = [], set()
    for i, d in enumerate(digests):
        if (rows is not None and rows[i] >= 0) or (take is not None and not take[i]):
            continue
        if distinct and d in seen:
            continue
        seen.add(d)
        out.append(wire.write_message("GetBlock", d))
    return b"".join(out)


def place_model(row_digests, row_sizes, row_dst, row_present, msg_digests, msg_sizes, msg_offsets, msg_ok=None):
    """The join as the header states it: every waiting row takes the
    lowest-numbered ok message with its digest; equal sizes make a job, in row
    order.  Returns (jobs [(src, dst, size, row, msg)], present, uses, n_left,
    n_size_mismatch)."""
    first = {}
    for m, d in enumerate(msg_digests):
        if (msg_ok is None or msg_ok[m]) and d not in first:
            first[d] = m
    jobs, present, uses, mismatch = [], [int(bool(p)) for p in row_present], [0] * len(msg_digests), 0
    for r, d in enumerate(row_digests):
        m = first.get(d)
        if present[r] or m is None:
            continue
        if msg_sizes[m] != row_sizes[r]:
            mismatch += 1
            continue
        jobs.append((msg_offsets[m], row_dst[r], row_sizes[r], r, m))
        present[r] = 1
        uses[m] += 1
    return jobs, present, uses, present.count(0), mismatch


def join_case(seed, many_rows=300):
    """Rows and messages as Python lists (place_model's arguments).  Digests
    held once, twice, three times and `many_rows` times; rows already present;
    messages shuffled, repeated and unsolicited; a repeated message whose
    first copy did not verify; a size mismatch; a digest no message carries."""
    rng = random.Random(seed)
    d = [rng.randbytes(20) for _ in range(40)]
    many, bad_first, wrong_size, unanswered = d[30], d[31], d[32], d[33]
    row_digests = d[:10] + d[10:20] * 2 + d[20:30] * 3 + [many] * many_rows + [bad_first] * 2 + [wrong_size, unanswered]
    rng.shuffle(row_digests)
    size = {x: rng.randrange(1, 40_000) for x in d}
    size[d[0]] = 0  # a block of no bytes
    n = len(row_digests)
    row_sizes = [size[x] for x in row_digests]
    row_dst, at = [], 7
    for s in row_sizes:
        row_dst.append(at)
        at += s
    present = [int(rng.random() < 0.15) for _ in range(n)]
    for x in (many, bad_first, wrong_size, unanswered, d[25]):  # their first rows wait
        present[row_digests.index(x)] = 0
    msgs = [x for x in d if x != unanswered] + [d[3], d[12], many, many] + [rng.randbytes(20) for _ in range(6)]
    rng.shuffle(msgs)
    msgs = [bad_first] + msgs  # message 0 does not verify; a later copy does
    msg_sizes = [size.get(x, 123) for x in msgs]
    msg_sizes = [s + 1 if x == wrong_size else s for s, x in zip(msg_sizes, msgs)]
    msg_offsets, at = [], 40
    for s in msg_sizes:
        msg_offsets.append(at)
        at += s + 40
    ok = [1] * len(msgs)
    ok[0] = 0
    ok[msgs.index(d[5])] = 0  # a digest whose only message did not verify
    return dict(row_digests=row_digests, row_sizes=row_sizes, row_dst=row_dst, row_present=present,
                msg_digests=msgs, msg_sizes=msg_sizes, msg_offsets=msg_offsets, msg_ok=ok)


E2E_SEED = 311


def e2e_files():
    """(source, old): a source file that holds one region three times and
    200 KB of zeros, and the file the destination already has, which holds the
    source's first 60 KB and none of the repeated content."""
    rng = random.Random(E2E_SEED)
    region = rng.randbytes(90_000)
    source = (rng.randbytes(70_000) + region + rng.randbytes(50_000) + region + bytes(200_000) + rng.randbytes(40_000)
              + region + rng.randbytes(30_000))
    old = rng.randbytes(30_000) + source[:60_000] + rng.randbytes(20_000)
    return source, old


def missing_of(source_digests, old_digests):
    """The digests the destination lacks, one per row, in row order: a block
    of the incoming file is looked up among the rows the index held before the
    file's own were added."""
    held = set(old_digests)
    return [d for d in source_digests if d not in held]
