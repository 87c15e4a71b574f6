"""GPU: the many-file device ZPAQ cut (sf_cut_device_zpaq_files,
sf_index_device_zpaq_files, sf_index_fds_zpaq) against the host cutter per
file, hashlib, and the restatement of its join (tests/zpaq_files_join.py,
pinned by test_zpaq_files_join.py without the code under test).

The batch of most tests is zpaq_files_join.table_files() at (6, 256),
L = 256: zeros of 40 L and 12 L + 5, period 7 of 20 L, random bytes of 9.5 L, L
and L + 1, and islands -- 39, 12, 18, 1, 0, 1 and 5 rounds -- with two empty
files among them, packed at odd bases with gaps into an allocation full of a
pattern that must come back bit-identical.  A test that relies on which files
settle asserts it from the restatement first."""
import ctypes
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

import stream_order as so
import zpaq_files_join as zfj
import zpaq_join as zj
from syncfast_amd import _lib, device, host

pytestmark = pytest.mark.gpu

BITS, MAX_SIZE, L = 6, 256, 256
PATTERN = 0xC3
EMPTY_SHA1 = hashlib.sha1(b"").digest()


def pack(files, lead=1):
    """(buffer, [(offset, length)]): the files at bases of every byte phase,
    3 to 15 pattern bytes between them and around them."""
    spans, at = [], lead
    for k, d in enumerate(files):
        at += 3 + (5 * k) % 13
        spans.append((at, len(d)))
        at += len(d)
    buf = np.full(at + 7, PATTERN, np.uint8)
    for (o, n), d in zip(spans, files):
        buf[o:o + n] = np.frombuffer(d, np.uint8)
    return buf, spans


def host_rows(files, spans, bits, max_size, skip=()):
    """The rows the call must give: (offsets, sizes, first_row) from the host
    cutter per file; files in `skip` have none."""
    offs, sizes, first = [], [], [0]
    for f, (d, (base, _n)) in enumerate(zip(files, spans)):
        if f not in skip:
            o, z = host.zpaq_cut_buffer(np.frombuffer(d, np.uint8), bits, max_size)
            offs.append(o.astype(np.int64) + base)
            sizes.append(z.astype(np.int32))
        first.append(first[-1] + (0 if f in skip else len(offs[-1])))
    cat = (lambda a, t: np.concatenate(a).astype(t) if a else np.zeros(0, t))
    return cat(offs, np.int64), cat(sizes, np.int32), np.array(first, np.int64)


@functools.lru_cache(None)
def batch():
    """The table's files, an empty file first, in the middle and last."""
    t = [d for _n, d, _r in zfj.table_files()]
    files = [b""] + t[:3] + [b""] + t[3:] + [b""]
    buf, spans = pack(files)
    return files, buf, spans


def check(res, want, gpu):
    offs, sizes, first = want
    torch.cuda.synchronize(gpu)
    assert np.array_equal(res.first_row.cpu().numpy(), first)
    assert np.array_equal(res.offsets.cpu().numpy(), offs) and np.array_equal(res.sizes.cpu().numpy(), sizes)


def test_no_cap_every_file_exact_and_the_statistics_are_the_restatements(gpu):
    files, buf, spans = batch()
    j = zfj.restate_files(files, BITS, MAX_SIZE)
    assert j.launches == 40 and not any(j.unsettled)
    x = torch.from_numpy(buf).to(gpu)
    res = device.cut_zpaq_files(x, spans, BITS, MAX_SIZE)
    check(res, host_rows(files, spans, BITS, MAX_SIZE), gpu)
    assert not res.unsettled.any() and res.unsettled.shape == (len(files),)
    assert device.zpaq_files_stats() == (L, j.segments, j.launches, j.recut, 0, 0)
    assert np.array_equal(x.cpu().numpy(), buf)  # the input, gaps included, is as it was


def test_a_cap_of_six_leaves_exactly_the_predicted_files_without_rows(gpu):
    files, buf, spans = batch()
    j = zfj.restate_files(files, BITS, MAX_SIZE, 6)
    left = {f for f, u in enumerate(j.unsettled) if u}
    assert left == {1, 2, 3} and j.launches == 6  # the zeros and the period 7
    x = torch.from_numpy(buf).to(gpu)
    res = device.cut_zpaq_files(x, spans, BITS, MAX_SIZE, max_rounds=6)
    assert res.unsettled.tolist() == j.unsettled
    want = host_rows(files, spans, BITS, MAX_SIZE, skip=left)
    assert want[2].tolist() == j.first_row
    check(res, want, gpu)
    st = device.zpaq_files_stats()
    assert (st[0], st[1], st[2], st[4], st[5]) == (L, j.segments, 6, 3, 0)


@pytest.mark.parametrize("cap", [1, 2, 5, 7, 13, 19, 39, 40])
def test_caps_at_and_beside_the_files_own_counts(gpu, cap):
    """Caps at a file's own round count (1, 5, 12, 18, 39), one above (2, 13,
    19, 40) and between (7): the unsettled files are those with at least `cap`
    rounds, and the launches are the restatement's."""
    files, buf, spans = batch()
    j = zfj.restate_files(files, BITS, MAX_SIZE, cap)
    assert j.unsettled == [r >= cap for r in j.rounds]
    res = device.cut_zpaq_files(torch.from_numpy(buf).to(gpu), spans, BITS, MAX_SIZE, max_rounds=cap)
    assert res.unsettled.tolist() == j.unsettled and device.zpaq_files_stats()[2] == j.launches
    check(res, host_rows(files, spans, BITS, MAX_SIZE, skip={f for f, u in enumerate(j.unsettled) if u}), gpu)


@pytest.mark.parametrize("index", [False, True])
def test_capacity_exact_and_one_short(gpu, index):
    files, buf, spans = batch()
    offs, sizes, first = host_rows(files, spans, BITS, MAX_SIZE)
    n, nf = offs.size, len(files)
    x = torch.from_numpy(buf).to(gpu)
    fo = np.array([s[0] for s in spans], np.uint64)
    fl = np.array([s[1] for s in spans], np.uint64)
    for cap in (n, n - 1):
        o = torch.full((n,), -1, dtype=torch.int64, device=gpu)
        z = torch.full((n,), -1, dtype=torch.int32, device=gpu)
        fr = torch.full((nf + 1,), -1, dtype=torch.int64, device=gpu)
        d = torch.full((n, 20), 0xEE, dtype=torch.uint8, device=gpu)
        nb, nu, bad = ctypes.c_uint64(7), ctypes.c_uint32(7), ctypes.c_uint32(7)
        head = (x.data_ptr(), x.numel(), fo.ctypes.data, fl.ctypes.data, nf, BITS, MAX_SIZE, 0, o.data_ptr(), z.data_ptr())
        tail = (None, ctypes.byref(nu), ctypes.byref(bad), torch.cuda.current_stream(gpu).cuda_stream)
        if index:
            rc = _lib.lib().sf_index_device_zpaq_files(*head, d.data_ptr(), cap, fr.data_ptr(), ctypes.byref(nb), None,
                                                       *tail)
        else:
            rc = _lib.lib().sf_cut_device_zpaq_files(*head, cap, fr.data_ptr(), ctypes.byref(nb), *tail)
        torch.cuda.synchronize(gpu)
        assert (nb.value, nu.value) == (n, 0)  # the need is reported either way
        if cap == n:
            assert rc == 0
            assert np.array_equal(o.cpu().numpy(), offs) and np.array_equal(z.cpu().numpy(), sizes)
            assert np.array_equal(fr.cpu().numpy(), first)
        else:  # nothing written
            assert rc == _lib.SF_ENOSPC
            assert (o == -1).all() and (z == -1).all() and (fr == -1).all()
        if index and cap != n:
            assert (d == 0xEE).all()


def test_three_thousand_small_files(gpu):
    """0 to 600 bytes each: many files per wave, most with one segment, some
    with two or three."""
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 601, 3000)
    lens[[0, 1, 2, 1500, 2999]] = 0
    files = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]
    buf, spans = pack(files, lead=0)
    assert max(zfj.restate_files(files, BITS, MAX_SIZE).rounds) < 8  # at most three segments each
    res = device.cut_zpaq_files(torch.from_numpy(buf).to(gpu), spans, BITS, MAX_SIZE, max_rounds=8)
    assert not res.unsettled.any()
    check(res, host_rows(files, spans, BITS, MAX_SIZE), gpu)
    assert device.zpaq_files_stats()[1] == sum(-(-int(n) // L) for n in lens)


def test_one_file_is_the_single_buffer_cut(gpu):
    """300 L of islands-like bytes as one file at base 0: the rows and the
    join's counters are cut_device_zpaq's (one launch more than its rounds:
    the one that finds nothing changed)."""
    raw = (zj.islands(L, 5, pairs=30) * 8)[:300 * L]
    assert len(raw) == 300 * L
    x = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(gpu)
    o1, z1 = device.cut_device_zpaq(x, BITS, MAX_SIZE)
    s1 = device.zpaq_device_stats()
    res = device.cut_zpaq_files(x, [(0, len(raw))], BITS, MAX_SIZE)
    torch.cuda.synchronize(gpu)
    assert torch.equal(res.offsets, o1) and torch.equal(res.sizes, z1)
    assert res.first_row.tolist() == [0, o1.numel()]
    assert device.zpaq_files_stats() == (s1[0], s1[1], s1[2] + 1, s1[3], 0, 0)


def test_default_parameters(gpu):
    """(13, 32768), L = 32768: twelve files, about 1 MiB in all, of 0 bytes to
    several segments."""
    rng = np.random.default_rng(5)
    lens = [0, 1, 32767, 32768, 32769, 100_000, 200_001, 65536, 5, 300_000, 250_000, 70_000]
    files = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    buf, spans = pack(files)
    res = device.cut_zpaq_files(torch.from_numpy(buf).to(gpu), spans)
    assert not res.unsettled.any()
    check(res, host_rows(files, spans, 13, 32768), gpu)


def test_overlapping_and_abutting_files(gpu):
    """Files are read only: two files over the same bytes, one inside
    another, two that abut."""
    raw = np.random.default_rng(3).integers(0, 256, 20 * L, dtype=np.uint8)
    spans = [(0, 20 * L), (0, 20 * L), (L + 3, 5 * L), (6 * L + 3, 2 * L + 1), (0, 0)]
    files = [raw[o:o + n].tobytes() for o, n in spans]
    res = device.cut_zpaq_files(torch.from_numpy(raw).to(gpu), spans, BITS, MAX_SIZE)
    check(res, host_rows(files, spans, BITS, MAX_SIZE), gpu)


def _index_want(files, spans, skip):
    offs, sizes, first = host_rows(files, spans, BITS, MAX_SIZE, skip=skip)
    digs, hashes = [], []
    for f, (d, (base, _n)) in enumerate(zip(files, spans)):
        if f in skip:
            hashes.append(bytes(20))
            continue
        mine = [hashlib.sha1(d[o - base:o - base + z]).digest()
                for o, z in zip(offs[first[f]:first[f + 1]].tolist(), sizes[first[f]:first[f + 1]].tolist())]
        digs += mine
        hashes.append(hashlib.sha1(b"".join(mine)).digest())
    return offs, sizes, first, np.frombuffer(b"".join(digs), np.uint8).reshape(-1, 20), hashes


@pytest.mark.parametrize("cap", [0, 6])
def test_index_digests_and_blocks_hashes_against_hashlib(gpu, cap):
    files, buf, spans = batch()
    skip = {1, 2, 3} if cap else set()
    assert [f for f, u in enumerate(zfj.restate_files(files, BITS, MAX_SIZE, cap).unsettled) if u] == sorted(skip)
    offs, sizes, first, digs, hashes = _index_want(files, spans, skip)
    res = device.index_zpaq_files(torch.from_numpy(buf).to(gpu), spans, BITS, MAX_SIZE, max_rounds=cap)
    check(res, (offs, sizes, first), gpu)
    assert np.array_equal(res.digests.cpu().numpy(), digs)
    assert [bytes(h) for h in res.blocks_hashes] == hashes
    assert hashes[0] == hashes[4] == hashes[-1] == EMPTY_SHA1  # the empty files
    if cap:
        assert hashes[1] == bytes(20) and res.unsettled.tolist() == [f in skip for f in range(len(files))]
    no = device.index_zpaq_files(torch.from_numpy(buf).to(gpu), spans, BITS, MAX_SIZE, max_rounds=cap,
                                 blocks_hashes=False)
    assert no.blocks_hashes is None and np.array_equal(no.digests.cpu().numpy(), digs)


def test_empty_batches(gpu):
    x = torch.from_numpy(np.full(64, PATTERN, np.uint8)).to(gpu)
    res = device.index_zpaq_files(x, [(0, 0), (64, 0), (7, 0)], BITS, MAX_SIZE)
    torch.cuda.synchronize(gpu)
    assert res.offsets.numel() == 0 and res.first_row.tolist() == [0, 0, 0, 0]
    assert [bytes(h) for h in res.blocks_hashes] == [EMPTY_SHA1] * 3
    res = device.cut_zpaq_files(x, [], BITS, MAX_SIZE)
    torch.cuda.synchronize(gpu)
    assert res.offsets.numel() == 0 and res.first_row.tolist() == [0] and res.unsettled.shape == (0,)


@pytest.mark.parametrize("index", [False, True])
def test_behind_a_hold_on_a_fresh_stream(gpu, index):
    """The inputs are still in production on the caller's stream when the call
    is made (tests/stream_order.py): a launch, an upload or a read-back on
    another stream sees the decoy or the 0xEE fill."""
    t = [d for _n, d, _r in zfj.table_files()]
    files = [t[6], b"", t[3], t[5]]
    assert zfj.restate_files(files, BITS, MAX_SIZE).launches >= 3  # a host read per join launch
    buf, spans = pack(files)
    other = np.random.default_rng(77).integers(0, 256, buf.size, dtype=np.uint8)

    def call(data, s):
        if index:
            r = device.index_zpaq_files(data, spans, BITS, MAX_SIZE, stream=s)
            return (r.offsets, r.sizes, r.first_row, r.digests, r.blocks_hashes.tobytes())
        r = device.cut_zpaq_files(data, spans, BITS, MAX_SIZE, stream=s)
        return (r.offsets, r.sizes, r.first_row)
    real, decoy = {"data": torch.from_numpy(buf).to(gpu)}, {"data": torch.from_numpy(other).to(gpu)}
    torch.cuda.synchronize(gpu)
    S = so.fresh_stream(gpu)
    H = so.hold_ms(so.timed_ms(lambda: call(real["data"], None), gpu))
    x, _o = so.pending(S, real, decoy, H)
    got = so.settle(S, x, decoy, call(x["data"], S))
    offs, sizes, first, digs, hashes = _index_want(files, spans, set())
    want = (offs, sizes, first) + ((digs, b"".join(hashes)) if index else ())
    assert so.same(got, want), so.first_difference(got, want)


# ------------------------------------------------------------ sf_index_fds_zpaq

import oracle  # noqa: E402
from syncfast_amd.index import Index, ZpaqChunker  # noqa: E402

BIG = 100_000


@functools.lru_cache(None)
def tree_contents():
    """Files of 0 B and 1 B, random bytes, zeros that need 19 rounds (finished
    on the host under the default cap), islands that need 5 (settled on the
    device), and one file larger than every stage the tests use."""
    t = {n: d for n, d, _r in zfj.table_files()}
    rng = np.random.default_rng(21)
    rnd = (lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    files = [("e0", b""), ("one", b"\x07"), ("r3000", rnd(3000)), ("zeros", bytes(20 * L)), ("r700", rnd(700)),
             ("islands", t["islands"]), ("r2500", rnd(2500)), ("e1", b""), ("big", rnd(BIG))]
    rounds = zfj.restate_files([d for _n, d in files[:-1]], BITS, MAX_SIZE).rounds
    assert rounds[3] == 19 >= host.ZPAQ_MAX_ROUNDS > rounds[5] == 5  # which is finished where
    return files


def stages_of(lens, target):
    """The stages sf_index_fds_zpaq packs files of `lens` into (each file at a
    64-byte boundary; empty files take no room), as include/syncfast_amd.h
    states it: the number of stages."""
    stages, used, any_file = 0, 0, False
    for n in lens:
        if n == 0:
            continue
        at = -(-used // 64) * 64
        if any_file and at + n > target:
            stages, at = stages + 1, 0
        used, any_file = at + n, True
    return stages + (1 if any_file else 0)


def write_tree(root, files):
    root.mkdir()
    paths = []
    for name, d in files:
        (root / name).write_bytes(d)
        paths.append(root / name)
    return paths


def check_file(name, data, rows, bh):
    a = np.frombuffer(data, np.uint8)
    offs, sizes = host.zpaq_cut_buffer(a, BITS, MAX_SIZE)
    assert np.array_equal(rows["offset"], offs) and np.array_equal(rows["size"], sizes), name
    dig = oracle.index_blocks(a, offs, sizes) if offs.size else np.zeros((0, 20), np.uint8)
    assert np.array_equal(rows["sha1"], dig), name
    assert bytes(bh) == oracle.blocks_hash(dig), name


@pytest.mark.parametrize("with_stamps", [False, True])
@pytest.mark.parametrize("stage_bytes,stages", [(1 << 16, 1), (8192, 2), (5120, 5)])
def test_index_fds_zpaq_against_the_oracle_per_file(gpu, tmp_path, stage_bytes, stages, with_stamps):
    files = tree_contents()
    assert stages_of([len(d) for _n, d in files[:-1]], stage_bytes) == stages and BIG > stage_bytes
    paths = write_tree(tmp_path / "t", files)
    reads = []
    fs = [open(p, "rb") for p in paths]
    _lib.set_read_hook(reads.append)
    try:
        stamps = [host.file_stamp(f.fileno()) for f in fs] if with_stamps else None
        rows, first, hashes, status = host.index_fds_zpaq([f.fileno() for f in fs], BITS, MAX_SIZE, stamps,
                                                          stage_bytes=stage_bytes)
    finally:
        _lib.set_read_hook(None)
        for f in fs:
            f.close()
    assert status.tolist() == [0] * len(files) and int(first[-1]) == rows.size
    assert len(reads) == stages + 1  # every stage read once, and the large file's one window
    for k, (name, d) in enumerate(files):
        check_file(name, d, rows[int(first[k]):int(first[k + 1])], hashes[k])
    st = device.zpaq_files_stats()
    assert (st[0], st[4], st[5]) == (L, 1, 1)  # the zeros did not settle and were finished on the host
    assert st[1] == sum(-(-len(d) // L) for _n, d in files[:-1])


@pytest.mark.parametrize("max_rounds,on_host", [(0, 0), (1, 5), (6, 1), (20, 0)])
def test_the_result_is_exact_whatever_the_cap(gpu, tmp_path, max_rounds, on_host):
    """No cap: the device joins the zeros' 19 rounds itself.  A cap of 1:
    every file that needs a round at all is finished on the host."""
    files = tree_contents()[:-1]
    rounds = zfj.restate_files([d for _n, d in files], BITS, MAX_SIZE).rounds
    assert sum(1 for r in rounds if max_rounds and r >= max_rounds) == on_host
    paths = write_tree(tmp_path / "t", files)
    fs = [open(p, "rb") for p in paths]
    try:
        rows, first, hashes, status = host.index_fds_zpaq([f.fileno() for f in fs], BITS, MAX_SIZE,
                                                          max_rounds=max_rounds, stage_bytes=1 << 16)
    finally:
        for f in fs:
            f.close()
    assert not status.any()
    for k, (name, d) in enumerate(files):
        check_file(name, d, rows[int(first[k]):int(first[k + 1])], hashes[k])
    assert device.zpaq_files_stats()[4:] == (on_host, on_host)


def test_a_large_file_in_the_middle_keeps_the_file_order(gpu, tmp_path):
    files = tree_contents()
    files = files[:3] + [files[-1]] + files[3:-1]
    paths = write_tree(tmp_path / "t", files)
    fs = [open(p, "rb") for p in paths]
    try:
        rows, first, hashes, status = host.index_fds_zpaq([f.fileno() for f in fs], BITS, MAX_SIZE, stage_bytes=8192)
    finally:
        for f in fs:
            f.close()
    assert not status.any() and int(first[-1]) == rows.size
    for k, (name, d) in enumerate(files):
        check_file(name, d, rows[int(first[k]):int(first[k + 1])], hashes[k])


def test_files_fail_alone(gpu, tmp_path):
    """Five stages; after the first is read a file of a later stage grows by a
    byte (its size moves, so its stamp does): SF_EAGAIN for it alone.  A stale
    stamp and a pipe fail alone too; every other file equals the oracle."""
    files = tree_contents()[:-1]
    paths = write_tree(tmp_path / "t", files)
    victim, stale, pipe_at = 5, 2, 4  # islands (stage 4 of 5), r3000, r700
    fired = []

    def hook(stage):
        if stage == 0 and not fired:
            fired.append(stage)
            with open(paths[victim], "ab") as g:
                g.write(b"!")
    r, w = os.pipe()
    fs = [open(p, "rb") for p in paths]
    _lib.set_read_hook(hook)
    try:
        stamps = [host.file_stamp(f.fileno()) for f in fs]
        stamps[stale].mtime_nsec += 1
        fds = [f.fileno() for f in fs]
        fds[pipe_at] = r
        rows, first, hashes, status = host.index_fds_zpaq(fds, BITS, MAX_SIZE, stamps, stage_bytes=5120)
    finally:
        _lib.set_read_hook(None)
        for f in fs:
            f.close()
        os.close(r)
        os.close(w)
    assert fired
    want = [0] * len(files)
    want[victim], want[stale], want[pipe_at] = _lib.SF_EAGAIN, _lib.SF_EAGAIN, _lib.SF_EINVAL
    assert status.tolist() == want
    for k, (name, d) in enumerate(files):
        if want[k]:
            assert first[k] == first[k + 1] and not hashes[k].any(), name
        else:
            check_file(name, d, rows[int(first[k]):int(first[k + 1])], hashes[k])


def test_index_path_on_the_device_route_fills_the_same_tables(gpu, tmp_path, monkeypatch):
    """Index.index_path with ZpaqChunker(device=True) against ZpaqChunker():
    the `files` and `blocks` tables are equal row for row.  Batches of 8 KiB
    (several sf_index_fds_zpaq calls) and large_file_bytes below the big file
    (it goes alone, through sf_index_fd_zpaq)."""
    files = tree_contents()
    root = tmp_path / "t"
    write_tree(root, files)
    (root / "sub").mkdir()
    (root / "sub" / "deep").write_bytes(files[2][1][:1234])
    calls, real = [], host.index_fds_zpaq

    def counted(fds, *a, **kw):  # the hook's statistics are the most recent call's: keep every call's
        res = real(fds, *a, **kw)
        calls.append((len(fds), device.zpaq_files_stats()[5]))
        return res
    monkeypatch.setattr(host, "index_fds_zpaq", counted)
    tables = []
    for name, chunker in (("a.idx", ZpaqChunker(BITS, MAX_SIZE)), ("b.idx", ZpaqChunker(BITS, MAX_SIZE, device=True))):
        idx = Index.open(tmp_path / name, chunker=chunker)
        idx.index_path(root, batch_bytes=8192, large_file_bytes=50_000)
        idx.commit()
        tables.append((idx.db.execute("SELECT file_id, name, modified, size, blocks_hash, temporary FROM files "
                                      "ORDER BY file_id").fetchall(),
                       idx.db.execute("SELECT file_id, hash, offset, size, present FROM blocks "
                                      "ORDER BY file_id, offset").fetchall()))
    assert tables[0][0] == tables[1][0] and len(tables[0][0]) == len(files) + 1
    assert tables[0][1] == tables[1][1] and len(tables[0][1]) > 100
    # every file but the large one went through the new call, in several batches, and the zeros were
    # finished on the host inside it
    assert len(calls) >= 2 and sum(n for n, _h in calls) == len(files) and sum(h for _n, h in calls) == 1
