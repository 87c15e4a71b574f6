"""GPU: a whole GetFiles stream -- many files' FILE_START / FILE_BLOCK /
FILE_END in one buffer -- received in one device call
(sf_receive_files_device, BlockSet.receive_files) and as the sink's GetFiles
state over an index (Index.receive_files).  Every result is compared with
files_expect's model, which is wire.Parser and the sink's rule."""
import ctypes
import hashlib
import random
from pathlib import PurePath

import numpy as np
import pytest
import torch

import oracle
import stream_order as so
from files_expect import (END, FILE_END, INCOMPLETE, MALFORMED, NO_NAME, OTHER, UNEXPECTED, block, expected,
                          needs_fallback, start)
from syncfast_amd import _lib, wire
from syncfast_amd.device import BlockSet
from syncfast_amd.digest import HashDigest
from syncfast_amd.index import Index, SyncfastError
from syncfast_amd.timestamp import DateTimeUtc
from test_wire_files import table as fixed_table

pytestmark = pytest.mark.gpu

GUARD, EXTRA = 0xEE, 3
D1, D2 = bytes(range(1, 21)), b"\n\n\n\n\n" + b"B" * 15
BIG = 1 << 40
OUTS = (("digests", np.uint8, 20), ("sizes", np.uint32, 1), ("offsets", np.uint64, 1), ("rows", np.int64, 1),
        ("block_file", np.uint32, 1), ("name_at", np.uint64, 1), ("name_len", np.uint32, 1), ("first", np.uint64, 1),
        ("file_size", np.uint64, 1))


def _digest(i) -> bytes:
    return hashlib.sha1(b"block %d" % i).digest()


class Got:
    pass


def receive(gpu, data: bytes, is_open=False, base=0, bset=None, align=0, bcap=None, fcap=None, query=False) -> Got:
    """sf_receive_files_device over ``data`` at ``align`` bytes past a 16-byte
    boundary, every output with EXTRA rows beyond its capacity (default: the
    model's need) and full of GUARD.  Returns the outputs as they are after
    the call, whole, and the results."""
    e = expected(data, is_open, base)
    bcap = len(e.sizes) if bcap is None else bcap
    fcap = len(e.name_at) if fcap is None else fcap
    raw = torch.empty(len(data) + 32, dtype=torch.uint8, device=gpu)
    lead = (align - raw.data_ptr()) % 16
    x = raw[lead:lead + len(data)]
    x.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8)) if data else None
    t = {}
    for name, dtype, width in OUTS:
        rows = (fcap + 1 if name == "first" else fcap if name in ("name_at", "name_len", "file_size") else bcap) + EXTRA
        t[name] = torch.full((rows * width * np.dtype(dtype).itemsize,), GUARD, dtype=torch.uint8, device=gpu)
    p = {k: None if query else v.data_ptr() for k, v in t.items()}
    nb, nf, used, end = (ctypes.c_uint64(77) for _ in range(4))
    why, still = ctypes.c_int(77), ctypes.c_int(77)
    g = Got()
    g.rc = _lib.lib().sf_receive_files_device(
        bset._h if bset is not None else None, x.data_ptr() if data else None, len(data), int(is_open), base,
        p["digests"], p["sizes"], p["offsets"], p["rows"], p["block_file"],
        bcap, p["name_at"], p["name_len"], p["first"], p["file_size"], fcap, ctypes.byref(nb), ctypes.byref(nf),
        ctypes.byref(used), ctypes.byref(why), ctypes.byref(still), ctypes.byref(end),
        torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize(gpu)
    assert x.cpu().numpy().tobytes() == data  # the input is as it was
    g.n_blocks, g.n_files, g.consumed, g.stop, g.open, g.end_offset = (nb.value, nf.value, used.value, why.value,
                                                                     still.value, end.value)
    for name, dtype, width in OUTS:
        a = t[name].cpu().numpy().view(dtype)
        setattr(g, name, a.reshape(-1, width) if width > 1 else a)
    g.stats, g.bcap, g.fcap, g.e, g.nothing = wire.recv_files_stats(), bcap, fcap, e, not data
    return g


def guard(dtype):
    """An element of ``dtype`` as the fill left it."""
    return np.frombuffer(bytes([GUARD]) * np.dtype(dtype).itemsize, dtype)[0]


def hold(g: Got, what="", rows=None):
    """A complete result against the model: every row the call must write,
    GUARD in every row after them."""
    e = g.e
    assert g.rc == 0, (what, g.rc)
    assert (g.n_blocks, g.n_files, g.consumed, g.stop, bool(g.open), g.end_offset) == \
        (len(e.sizes), len(e.name_at), e.consumed, e.stop, e.open, e.end_offset), what
    assert g.stats[1] == e.messages, what
    b, f = len(e.sizes), len(e.name_at)
    if g.nothing:  # no bytes: the state is handed back and no row is written, not even the carried section's
        f = -1
    want = {"digests": np.frombuffer(b"".join(e.digests), np.uint8).reshape(-1, 20), "sizes": e.sizes,
            "offsets": e.offsets, "block_file": e.block_file, "name_at": e.name_at, "name_len": e.name_len,
            "first": e.first, "file_size": e.file_size, "rows": rows}
    for name, dtype, _w in OUTS:
        got = getattr(g, name)
        n = max(f + 1 if name == "first" else f if name in ("name_at", "name_len", "file_size") else b, 0)
        if want[name] is None:  # no set: d_rows is not written
            n = 0
        else:
            assert np.array_equal(got[:n], np.array(want[name], dtype).reshape((-1,) + got.shape[1:])[:n]), (what, name)
        assert (got[n:].view(np.uint8) == GUARD).all(), (what, name, "written past its rows")


# ------------------------------------------------------------------ geometry

def test_every_phase_of_the_bitmap_word_and_of_the_base_pointer(gpu):
    """The messages after a FILE_START whose name has 0..100 bytes start at
    every phase of a bitmap word and of a lane; among them a 112-byte
    FILE_START (its link check reads three words) and a 9-byte FILE_END, at
    every phase.  The base pointer at alignments 0..3."""
    long_name = b"n" * 100
    for k in range(101):
        data = (start(b"a" * k) + block(D1, 5) + FILE_END + start(long_name) + block(D2, 0) + block(D1, 4096) + FILE_END
                + start(b"") + FILE_END)
        g = receive(gpu, data, align=k % 4)
        hold(g, k)
        assert g.stats[2] == 0 and g.stop == END
    # the 112-byte message begins at position 63 and at 62 (mod 64), and the buffer ends with it
    for at in (62, 63, 126, 127):
        lead = start(b"") + FILE_END if at > 64 else b""
        data = lead + start(b"a" * (at - len(lead) - 21)) + FILE_END + start(long_name)
        assert len(data) == at + 112
        g = receive(gpu, data)
        hold(g, at)
        assert g.stats[2] == 0 and g.open and g.name_at[g.n_files - 1] == at + 11


def test_a_buffer_that_ends_anywhere_in_a_lane(gpu):
    """Streams cut 0..40 bytes short, at base alignments 0..3: the lanes that
    cannot read five whole dwords read bytes, and nothing past the end."""
    data = start(b"dir/file") + b"".join(block(_digest(i), 1000 + i) for i in range(6)) + FILE_END + start(b"x") + FILE_END
    for cut in range(41):
        for align in range(4):
            g = receive(gpu, data[:len(data) - cut], align=align)
            hold(g, (cut, align))
            assert g.stats[2] == 0


# ------------------------------------------------------------------- content

def test_empty_files_one_block_files_and_empty_blocks(gpu):
    e, b1, b0 = start(b"e") + FILE_END, start(b"one") + block(D1, 7) + FILE_END, start(b"z") + block(D2, 0) * 3 + FILE_END
    for name, data in (("first", e + b1), ("last", b1 + e), ("adjacent", b1 + e + e + e + b0), ("only", e * 70),
                       ("zero", b0 + b1 + b0), ("carried_empty", FILE_END + e + b1)):
        g = receive(gpu, data, is_open=name == "carried_empty", base=BIG)
        hold(g, name)
        assert g.stats[2] == 0 and g.stop == END and not g.open


@pytest.fixture(scope="module")
def big():
    """About 300 files with about 20,000 blocks: names from [a-z0-9/._-],
    digests from hashlib."""
    rng = random.Random(5)
    parts, k = [], 0
    for f in range(300):
        name = "".join(rng.choice("abcdefghijklmnopqrstuvwxyz0123456789/._-") for _ in range(rng.randrange(1, 60)))
        parts.append(start(name.encode()))
        for _ in range(rng.choice((0, 1, 2, 40, 120, 240))):
            parts.append(block(_digest(k % 9000), rng.choice((0, 1, 8191, 8192, 65536, rng.randrange(1 << 20)))))
            k += 1
        parts.append(FILE_END)
    data = b"".join(parts)
    assert k > 15000
    return data


def test_three_hundred_files_on_the_device_route(gpu, big):
    assert not needs_fallback(big)  # on the CPU, before the GPU call: no case is left to the fallback silently
    rng = np.random.default_rng(8)
    table = np.frombuffer(b"".join(_digest(int(i)) for i in rng.integers(0, 12000, 5000)), np.uint8).reshape(-1, 20).copy()
    present = rng.random(5000) < 0.7
    with BlockSet(torch.from_numpy(table).to(gpu), torch.from_numpy(present).to(gpu)) as bset:
        g = receive(gpu, big, bset=bset)
        want = oracle.block_lookup(table, present, g.digests[:g.n_blocks])
        hold(g, "big", rows=want)
        assert g.stats[2] == 0 and g.stats[0] == g.stats[1] == g.e.messages  # the device route, every candidate a message
        assert g.n_files == 300 and (want >= 0).any() and (want < 0).any()
        # the wrapper: the same arrays, sized by its guess
        r = bset.receive_files(torch.frombuffer(bytearray(big), dtype=torch.uint8).to(gpu))
        assert (r.consumed, r.stop, r.open, r.end_offset) == (len(big), END, False, g.e.end_offset)
        assert np.array_equal(r.rows.cpu().numpy(), want)
        assert r.offsets.cpu().numpy().tolist() == g.e.offsets and r.file_first.cpu().numpy().tolist() == g.e.first
        assert r.file_size.cpu().numpy().tolist() == g.e.file_size
        assert r.name_at.cpu().numpy().tolist() == g.e.name_at
        # ... also when the guess is short (files of no block at all)
        many = (start(b"e") + FILE_END) * 200
        r = bset.receive_files(torch.frombuffer(bytearray(many), dtype=torch.uint8).to(gpu))
        assert (r.name_at.shape[0], r.digests.shape[0], r.consumed, r.stop) == (200, 0, len(many), END)
        # ... and with nothing to read
        r = bset.receive_files(torch.empty(0, dtype=torch.uint8, device=gpu), open=True, base_offset=9)
        assert (r.name_at.tolist(), r.file_first.tolist(), r.file_size.tolist(), r.open, r.end_offset) == \
            ([-1], [0, 0], [9], True, 9)


# --------------------------------------------------------------------- carry

def test_a_stream_cut_at_every_byte_continues_through_the_carry(gpu):
    data = (start(b"dir/a") + b"".join(block(_digest(i), 100 * i) for i in range(14)) + FILE_END + start(b"empty")
            + FILE_END + start(b"n" * 100) + b"".join(block(_digest(i), 4294967295) for i in range(12)) + FILE_END
            + start(b"last") + b"".join(block(_digest(i), i) for i in range(5)))
    whole = expected(data)
    assert whole.messages >= 38 and whole.open and whole.stop == END
    for cut in range(len(data) + 1):
        g1 = receive(gpu, data[:cut])
        hold(g1, cut)
        g2 = receive(gpu, data[g1.consumed:], is_open=bool(g1.open), base=g1.end_offset)
        hold(g2, cut)
        assert g1.stats[2] == g2.stats[2] == 0
        e1, e2 = g1.e, g2.e
        shift = len(e1.name_at) - int(e1.open)  # section 0 of the second call is the open file
        assert (e1.consumed + e2.consumed, e2.stop, e2.open, e2.end_offset) == \
            (whole.consumed, whole.stop, whole.open, whole.end_offset), cut
        assert e1.digests + e2.digests == whole.digests and e1.sizes + e2.sizes == whole.sizes, cut
        assert e1.offsets + e2.offsets == whole.offsets, cut
        assert e1.block_file + [f + shift for f in e2.block_file] == whole.block_file, cut
        sizes = e1.file_size[:shift] + e2.file_size
        assert sizes == whole.file_size, cut
        if e1.open:
            assert e2.name_at[0] == NO_NAME
            # (the last cut leaves the second call no bytes: it launches nothing and writes no row)
            assert g2.n_files >= 1 and (g2.nothing or g2.name_at[0] == NO_NAME)
        at = e1.name_at + [a + e1.consumed for a in e2.name_at if a != NO_NAME]  # the open file's name came first
        assert at == whole.name_at, cut


# --------------------------------------------------------------------- stops

def test_every_stop_class_after_a_valid_prefix(gpu):
    """The fixed table of test_wire_files.py on the device: every stop class,
    every proper prefix, the filename quirk, all pairs, every first message
    for open 0 and 1."""
    stops = set()
    for name, data, is_open, base in fixed_table():
        g = receive(gpu, data, is_open=is_open, base=base)
        hold(g, name)
        assert g.stats[2] == int(needs_fallback(data, is_open)) or not data, name
        stops.add((g.stop, name.split("_")[0]))
    assert {s for s, _ in stops} == {END, INCOMPLETE, OTHER, MALFORMED, UNEXPECTED}
    assert (UNEXPECTED, "pair") in stops and (UNEXPECTED, "first") in stops


# ------------------------------------------------------------------ fallback

FORGED = {
    "digest": start(b"t") + block(b"FILE_END\n" + b"z" * 11, 1) + block(D1, 2) + FILE_END + start(b"u") + FILE_END,
    "name_end": start(b"x/FILE_END") + block(D1, 7) + FILE_END + start(b"y") + FILE_END,
    "name_start": start(b"x/FILE_START") + block(D1, 7) + FILE_END + start(b"y") + block(D2, 1) + FILE_END,
    "name_start_twice": start(b"a") + FILE_END + start(b"FILE_START") + block(D1, 7) + FILE_END,
}


@pytest.mark.parametrize("case", list(FORGED))
def test_a_start_inside_a_message_goes_to_the_host(gpu, knobs, case):
    data = FORGED[case]
    assert needs_fallback(data)
    rng = np.random.default_rng(3)
    table = np.concatenate([np.frombuffer(D1 + D2, np.uint8).reshape(2, 20), rng.integers(0, 256, (30, 20), dtype=np.uint8)])
    present = np.ones(32, bool)
    with BlockSet(torch.from_numpy(table).to(gpu), torch.from_numpy(present).to(gpu)) as bset:
        g = receive(gpu, data, bset=bset)
        want = oracle.block_lookup(table, present, g.digests[:g.n_blocks])
        hold(g, case, rows=want)
        assert g.stats[2] == 1 and g.stats[0] > g.e.messages and (want >= 0).any()
        # cut short after the forged start, and with capacities one short
        g = receive(gpu, data[:-3], bset=bset)
        hold(g, case, rows=oracle.block_lookup(table, present, g.digests[:g.n_blocks]))
        assert g.stats[2] == 1
        g = receive(gpu, data, bset=bset, bcap=len(g.e.sizes) - 1, fcap=len(g.e.name_at) - 1)
        assert (g.rc, g.n_blocks, g.n_files, g.stats[2]) == (_lib.SF_ENOSPC, len(g.e.sizes), len(g.e.name_at), 1)
        assert (g.digests[g.bcap:] == GUARD).all() and (g.name_at[g.fcap:] == guard(np.uint64)).all()
        assert (g.first[g.fcap:] == guard(np.uint64)).all() and (g.offsets == guard(np.uint64)).all()


def test_the_forced_host_route_gives_the_same_arrays(gpu, knobs, big):
    honest = big[:expected(big[:40000]).consumed] + b"FILE_BLO"
    a = receive(gpu, honest)
    hold(a, "device")
    assert a.stats[2] == 0
    knobs.set("SF_TEST_WIRE_PARSE_HOST", 1)
    b = receive(gpu, honest)
    hold(b, "host")
    assert b.stats == (0, a.stats[1], 1, 0) and b.stop == INCOMPLETE
    for name, _d, _w in OUTS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    hold(receive(gpu, FILE_END + honest, is_open=True, base=BIG), "host, carried")


# ------------------------------------------------------------------ capacity

@pytest.mark.parametrize("short", ["blocks", "files", "both", "query"])
def test_a_capacity_one_short_and_the_query(gpu, short):
    data = start(b"a") + block(D1, 5) + block(D2, 6) + FILE_END + start(b"b") + block(D1, 7) + FILE_END + b"COMPLETE\n"
    e = expected(data)
    nb, nf = len(e.sizes), len(e.name_at)
    g = receive(gpu, data, bcap=nb - (short in ("blocks", "both")), fcap=nf - (short in ("files", "both")),
                query=short == "query")
    assert (g.rc, g.n_blocks, g.n_files, g.consumed, g.stop, g.open) == (_lib.SF_ENOSPC, nb, nf, e.consumed, OTHER, 0)
    assert g.stats[2] == 0
    b, f = (0, 0) if short == "query" else (g.bcap, g.fcap)
    # the parse's rows that fit; no offset, no file size, no last entry of first; nothing past a capacity
    assert g.digests[:b].tobytes() == b"".join(e.digests[:b]) and (g.digests[b:] == GUARD).all()
    assert g.sizes[:b].tolist() == e.sizes[:b] and (g.sizes[b:] == guard(np.uint32)).all()
    assert g.block_file[:b].tolist() == e.block_file[:b] and (g.block_file[b:] == guard(np.uint32)).all()
    assert g.name_at[:f].tolist() == e.name_at[:f] and (g.name_at[f:] == guard(np.uint64)).all()
    assert g.name_len[:f].tolist() == e.name_len[:f] and (g.name_len[f:] == guard(np.uint32)).all()
    assert g.first[:f].tolist() == e.first[:f] and (g.first[f:] == guard(np.uint64)).all()
    for untouched in (g.offsets, g.file_size):
        assert (untouched == guard(np.uint64)).all()
    assert (g.rows == guard(np.int64)).all()


def test_a_size_above_32_bits_is_out_of_range(gpu, knobs):
    data = start(b"a") + block(D1, 4294967295) + block(D2, 4294967296) + FILE_END
    for host in (0, 1):
        knobs.set("SF_TEST_WIRE_PARSE_HOST", host)
        assert receive(gpu, data, bcap=2, fcap=1).rc == _lib.SF_ERANGE
        g = receive(gpu, data[:60])  # up to the size that fits
        hold(g, host)
        assert g.sizes[0] == 4294967295 and g.end_offset == 4294967295


# -------------------------------------------------------------------- lookup

def test_one_lookup_of_all_files_and_none_without_a_set(gpu):
    rng = np.random.default_rng(21)
    pool = rng.integers(0, 256, (40, 20), dtype=np.uint8)
    table = pool[rng.integers(0, 30, 200)]  # repeated digests; rows 30..39 of the pool are in no row
    present = rng.random(200) < 0.5
    picks = rng.integers(0, 40, 120)
    data, k = b"", 0
    for f in range(6):
        data += start(b"f%d" % f) + b"".join(block(pool[i].tobytes(), 10 + int(i)) for i in picks[k:k + 20]) + FILE_END
        k += 20
    with BlockSet(torch.from_numpy(table).to(gpu), torch.from_numpy(present).to(gpu)) as bset:
        g = receive(gpu, data, bset=bset)
        want = oracle.block_lookup(table, present, pool[picks])
        hold(g, "set", rows=want)
        assert (want >= 0).sum() > 20 and (want < 0).sum() > 20
    hold(receive(gpu, data), "no set")  # d_rows keeps its fill


# -------------------------------------------------------------- stream order

def test_inputs_pending_on_the_callers_stream(gpu):
    """The run holds a decoy until a hold on a fresh stream ends; the call,
    given that stream, must parse the real run."""
    def stream_of(seed):
        rng = random.Random(seed)
        return b"".join(start(b"f%02d" % f) + b"".join(block(rng.randbytes(20), rng.randrange(1000, 10000))
                                                       for _ in range(30)) + FILE_END for f in range(20))
    real, decoy = stream_of(1), stream_of(2)
    assert len(real) == len(decoy) and not needs_fallback(real) and not needs_fallback(decoy)
    e = expected(real)
    table = np.frombuffer(b"".join(e.digests[::3] + expected(decoy).digests[::3]), np.uint8).reshape(-1, 20).copy()
    present = np.ones(table.shape[0], bool)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(gpu)  # noqa: E731
    real_t, decoy_t = dev(real), dev(decoy)
    torch.cuda.synchronize(gpu)
    S = so.fresh_stream(gpu)
    with torch.cuda.stream(S):
        bset = BlockSet(torch.from_numpy(table).to(gpu), torch.from_numpy(present).to(gpu), stream=S)
        bset.receive_files(real_t)
    S.synchronize()
    H = so.hold_ms(so.timed_ms(lambda: bset.receive_files(real_t), gpu))
    x, _o = so.pending(S, {"run": real_t}, {"run": decoy_t}, H)
    r = bset.receive_files(x["run"])
    got = so.settle(S, x, {"run": decoy_t}, tuple(r))
    bset.close()
    want_rows = oracle.block_lookup(table, present, np.frombuffer(b"".join(e.digests), np.uint8).reshape(-1, 20))
    assert (want_rows < 0).any()
    want = (np.frombuffer(b"".join(e.digests), np.uint8).reshape(-1, 20), np.array(e.sizes, np.uint32),
            np.array(e.offsets, np.int64), want_rows, np.array(e.block_file, np.int32), np.array(e.name_at, np.int64),
            np.array(e.name_len, np.int32), np.array(e.first, np.int64), np.array(e.file_size, np.int64), e.consumed,
            e.stop, e.open, e.end_offset)
    assert so.same(got, want), so.first_difference(got, want)


# ------------------------------------------------ Index.receive_files: the sink

NAMES = [PurePath("dir/n%d" % f) for f in range(5)]


def _indexes(seed, copies):
    """Equal in-memory indexes: files with blocks from a small pool (repeated
    hashes), rows recorded as missing, and five temporary files the incoming
    blocks go to."""
    rng = np.random.default_rng(seed)
    pool = [HashDigest(rng.integers(0, 256, 20, dtype=np.uint8).tobytes()) for _ in range(50)]
    plan = [(f, [(int(rng.integers(0, len(pool))), bool(rng.random() < 0.3)) for _ in range(40)]) for f in range(5)]
    out = []
    for _ in range(copies):
        idx = Index.open_in_memory()
        for f, blocks in plan:
            fid, _ = idx.add_file(PurePath(f"dir/f{f}"), DateTimeUtc.from_ns(f))
            for b, (h, missing) in enumerate(blocks):
                (idx.add_missing_block if missing else idx.add_block)(pool[h], fid, b * 4096, 4096)
        for name in NAMES:
            idx.add_temp_file(name)
        out.append(idx)
    return out, pool, rng


def _dump(idx):
    return (idx.db.execute("SELECT rowid, hash, file_id, offset, size, present FROM blocks ORDER BY rowid;").fetchall(),
            idx.db.execute("SELECT file_id, name, size, blocks_hash, temporary FROM files ORDER BY file_id;").fetchall())


def _sink_loop(idx, data):
    """The reference's loop (src/sync/fs.rs:449-500), message by message."""
    state, copies = None, {}
    for msg in wire.Parser().receive(data):
        if msg[0] == "FileStart":
            assert state is None
            fid = idx.get_temp_file(PurePath(msg[1].decode()))[0]
            state = (fid, 0)
            copies.setdefault(idx.get_file_name(fid), [])
        elif msg[0] == "FileBlock":
            fid, offset = state
            found = idx.get_block(msg[1])
            if found is not None:
                copies[idx.get_file_name(fid)].append((found[0], found[1], offset, msg[2]))
                idx.add_block(msg[1], fid, offset, msg[2])
            else:
                idx.add_missing_block(msg[1], fid, offset, msg[2])
            state = (fid, offset + msg[2])
        else:
            assert msg == ("FileEnd",)
            idx.set_file_size_and_compute_blocks_hash(*state)
            state = None
    return copies, state


def test_index_receive_files_is_the_sink_loop(gpu):
    (loop, once, per_file), pool, rng = _indexes(70, 3)
    fresh = [HashDigest(rng.integers(0, 256, 20, dtype=np.uint8).tobytes()) for _ in range(30)]
    known = next(h for h in pool if loop.get_block(h) is not None)
    files = []
    for f in range(5):
        n = 0 if f == 2 else 60  # one empty file
        picks = [(pool + fresh)[int(rng.integers(0, 80))] for _ in range(n)]
        if f in (1, 3):  # one hash in two incoming files that the index holds, and one that it does not
            picks[5], picks[6] = known, fresh[0]
        sizes = [int(s) for s in rng.integers(1, 70000, n)]  # (file_id, offset) is unique in the index: no empty block
        files.append(b"".join(wire.write_message("FileBlock", h, s) for h, s in zip(picks, sizes)) + FILE_END)
    data = b"".join(start(str(name).encode()) + body for name, body in zip(NAMES, files))
    copies, state = _sink_loop(loop, data)
    assert state is None and 0 < sum(map(len, copies.values())) < 240
    # one call
    got, consumed, carry = once.receive_files(data, device=gpu)
    assert (got, consumed, carry) == (copies, len(data), None)
    assert wire.recv_files_stats()[2] == 0
    assert _dump(once) == _dump(loop) and once.list_missing_blocks() == loop.list_missing_blocks()
    rows = dict(((r[1], r[2]), r[5]) for r in _dump(once)[0][200:])
    ids = [once.get_temp_file(n)[0] for n in NAMES]
    assert {rows[(known.to_sql(), ids[f])] for f in (1, 3)} == {1} and {rows[(fresh[0].to_sql(), ids[f])] for f in (1, 3)} == {0}
    # the loop of receive_file_blocks, one file per call
    for name, body in zip(NAMES, files):
        assert per_file.receive_file_blocks(per_file.get_temp_file(name)[0], body, device=gpu) == \
            copies[per_file.get_file_name(per_file.get_temp_file(name)[0])]
    assert _dump(per_file) == _dump(loop)
    # the same buffer in two pieces through the carry
    for cut in (len(files[0]) // 2, len(data) - 9):
        (idx,), _, _ = _indexes(70, 1)
        c1, used, carry = idx.receive_files(data[:cut], device=gpu)
        assert carry is not None and carry[0] == idx.get_temp_file(NAMES[0 if cut < len(files[0]) else 4])[0]
        c2, used2, carry2 = idx.receive_files(data[used:], device=gpu, open_file=carry)
        assert (used + used2, carry2) == (len(data), None)
        assert {k: c1.get(k, []) + c2.get(k, []) for k in copies} == copies
        assert _dump(idx) == _dump(loop)
    # what the sink refuses is refused, and nothing is written
    before = _dump(once)
    one = start(b"dir/n0") + wire.write_message("FileBlock", fresh[1], 5)
    for bad, error in ((start(b"dir/unknown") + FILE_END, SyncfastError),
                       (one + FILE_END + start(b"dir/\xff\xfe") + FILE_END, wire.ProtocolError),
                       (one + start(b"dir/n1"), wire.ProtocolError),          # an unexpected message
                       (one + FILE_END + FILE_END, wire.ProtocolError),
                       (one + b"COMPLETE\n", wire.ProtocolError),
                       (one + FILE_END + b"BOGUS\n", wire.ProtocolError)):  # a malformed tail
        with pytest.raises(error):
            once.receive_files(bad, device=gpu)
        assert _dump(once) == before
