"""GPU: a received FILE_BLOCK run parsed on the device
(sf_wire_parse_blocks_device), with offsets and block lookup
(sf_receive_blocks_device / _buffer, BlockSet.receive) and as the rows of the
sink's GetFiles state (Index.receive_file_blocks).  What a run must parse to
always comes from wire.Parser / wire.write_message (recv_expect.py), never
from the code under test."""
import ctypes
from pathlib import PurePath

import numpy as np
import pytest
import torch

import data_expect
import oracle
import recv_forge
import syncfast_amd
from recv_expect import END, INCOMPLETE, MALFORMED, OTHER, expected, message
from syncfast_amd import _lib, host, wire
from syncfast_amd.device import BlockSet
from syncfast_amd.digest import HashDigest
from syncfast_amd.index import Index
from syncfast_amd.timestamp import DateTimeUtc

pytestmark = pytest.mark.gpu


def _sizes(n, rng):
    """1 to 10 digits in turn, with 0 and 2^32 - 1 among them."""
    out = []
    for i in range(n):
        d = i % 10 + 1
        out.append(int(rng.integers(10 ** (d - 1), min(10 ** d, 1 << 32))))
    if n > 0:
        out[0] = 0
    if n > 1:
        out[1] = 4294967295
    return out


def _honest(n, seed=1):
    rng = np.random.default_rng(seed + n)
    digests = rng.integers(0, 256, (n, 20), dtype=np.uint8)
    sizes = _sizes(n, rng)
    return b"".join(message(digests[i].tobytes(), sizes[i]) for i in range(n)), digests, sizes


def _dev(run: bytes, gpu, lead=0):
    """`run` in HBM, `lead` bytes into an allocation that ends with it."""
    t = torch.empty(lead + len(run), dtype=torch.uint8, device=gpu)
    if run:
        t[lead:] = torch.frombuffer(bytearray(run), dtype=torch.uint8).to(gpu)
    return t[lead:]


def _check(run: bytes, gpu, lead=0):
    """parse_blocks_device(run) is what the parser reads; returns the stats."""
    want_d, want_s, want_c, want_stop = expected(run)
    d, s, consumed, stop = wire.parse_blocks_device(_dev(run, gpu, lead))
    assert (d.shape[0], consumed, stop) == (len(want_d), want_c, want_stop)
    assert d.cpu().numpy().tobytes() == b"".join(want_d)
    assert s.cpu().numpy().tolist() == want_s
    stats = wire.parse_stats()
    assert stats[1] == len(want_d)
    return stats


@pytest.mark.parametrize("n", [0, 1, 2, 64, 65, 257, 5000])
def test_honest_runs(gpu, n):
    run, digests, sizes = _honest(n)
    want_d, want_s, want_c, want_stop = expected(run)
    assert (len(want_d), want_s, want_c, want_stop) == (n, sizes, len(run), END)  # the parser reads the run back
    stats = _check(run, gpu)
    assert stats[0] >= n and stats[2] == 0


def test_round_trip_with_the_device_writer(gpu):
    rng = np.random.default_rng(5)
    digests = torch.from_numpy(rng.integers(0, 256, (5000, 20), dtype=np.uint8)).to(gpu)
    sizes = torch.from_numpy(np.array(_sizes(5000, rng), np.uint32).view(np.int32)).to(gpu)
    run = wire.blocks_device(digests, sizes)
    d, s, consumed, stop = wire.parse_blocks_device(run)
    assert (consumed, stop) == (run.numel(), END)
    assert torch.equal(d, digests) and torch.equal(s.view(torch.int32), sizes)
    assert wire.parse_stats()[2] == 0


def test_size_field_forms(gpu):
    d = bytes(range(20))
    run = message(d, b"+12") + message(d, b"0012") + message(d, b"000000000000007") + message(d, 5)
    assert expected(run)[1] == [12, 12, 7, 5]
    assert _check(run, gpu)[2] == 0
    big = message(d, 1) + message(d, 4294967296)
    assert expected(big)[1] == [1, 4294967296]  # the reference's usize takes it; sizes are uint32 here
    with pytest.raises(_lib.SfError) as e:
        wire.parse_blocks_device(_dev(big, gpu))
    assert e.value.code == _lib.SF_ERANGE
    # ... but only inside the parsed prefix: after FILE_END it is not this run's business
    assert _check(message(d, 1) + b"FILE_END\n" + message(d, 4294967296), gpu)[1] == 1


def _tails():
    d4 = bytes(range(100, 120))
    fourth = message(d4, 1234567)
    cases = [(b"", END), (b"FILE_END\n", OTHER), (b"FILE_START\nname", OTHER), (b"BOGUS\n", MALFORMED),
             (b"X" * 20, MALFORMED), (b"X" * 19, INCOMPLETE), (b"FILE_BLOCK\n" + d4 + b"x", MALFORMED),
             (message(d4, b"12a"), MALFORMED), (message(d4, b""), MALFORMED),
             (message(d4, b"1234567890123456"), MALFORMED)]
    cases += [(fourth[:k], INCOMPLETE) for k in range(1, len(fourth))]
    return cases


def test_tails_after_three_messages(gpu):
    three = b"".join(message(bytes([40 + i]) * 20, 10 ** (3 * i)) for i in range(3))
    for tail, want in _tails():
        run = three + tail
        digests, _, consumed, stop = expected(run)
        assert (len(digests), consumed, stop) == (3, len(three), want), tail  # the written-out class is the parser's
        assert _check(run, gpu)[2] == 0, tail
        # and with nothing before it
        assert expected(tail)[3] == want and _check(tail, gpu)[1] == 0, tail


def test_two_files_in_one_buffer(gpu):
    run_a, _, _ = _honest(70, seed=11)
    run_b, _, _ = _honest(33, seed=12)
    buf = run_a + b"FILE_END\n" + b"FILE_START\nb\n" + run_b
    d, s, consumed, stop = wire.parse_blocks_device(_dev(buf, gpu))
    assert (d.shape[0], consumed, stop) == (70, len(run_a), OTHER) and wire.parse_stats()[2] == 0
    assert d.cpu().numpy().tobytes() == b"".join(expected(run_a)[0])
    # the caller's parser reads the two messages that stand there and hands the rest back
    p = wire.Parser()
    skip = len(b"FILE_END\n" + b"FILE_START\nb\n")
    msgs = p.receive(buf[consumed:consumed + skip])
    assert msgs == [("FileEnd",), ("FileStart", b"b")]
    rest = buf[consumed + skip:]
    assert rest == run_b
    assert _check(rest, gpu, lead=1)[2] == 0


@pytest.mark.parametrize("fill", ["newlines", "digits", "tags"])
def test_hostile_digests(gpu, fill):
    if fill == "newlines":
        digests = [b"\n" * 20] * 40
    elif fill == "digits":
        digests = [bytes([0x30 + (i + k) % 10 for k in range(20)]) for i in range(40)]
    else:  # the tag at every digest offset at which it fits or is cut by the digest's end
        digests = [(bytes(j) + b"FILE_BLOCK\n" + bytes(20))[:20] for j in range(10)] * 4
    rng = np.random.default_rng(3)
    run = b"".join(message(d, s) for d, s in zip(digests, _sizes(len(digests), rng)))
    assert len(expected(run)[0]) == len(digests) and expected(run)[3] == END
    _check(run, gpu)
    _check(run + b"FILE_END\n", gpu)


@pytest.mark.parametrize("lead", [0, 3])
def test_block_data_messages_in_the_digests_and_after_the_run(gpu, lead):
    """The other receive parser's message kind as the hostile content: every
    digest holds the BLOCK_DATA tag and goes on like a data header, the second
    and third so that a whole BLOCK_DATA message stands inside the run, and
    one follows it.  None of that is a FILE_BLOCK candidate."""
    fill = b"\xaa"
    # the data header in the second digest reaches over the third message's tag, whose newline ends its
    # digest; its length field, its payload and its end byte are the third digest's first bytes
    digests = [b"BLOCK_DATA\n" + bytes(8) + b"\n",
               fill * 4 + b"BLOCK_DATA\n" + fill * 5,
               b"4\nabcd\n" + b"BLOCK_DATA\n" + fill * 2]
    three = b"".join(message(d, s) for d, s in zip(digests, (5, 123, 4294967295)))
    run = three + data_expect.message(b"BLOCK_DATA\n" + b"FILE_BLOC" + fill * 30)
    inside = [p for p, _ in data_expect.candidates(run) if p < len(three)]
    assert inside == [len(message(digests[0], 5)) + 11 + 4]  # a whole message to the parser, started there
    assert 100 < len(run) < 400
    want_d, _, want_c, want_stop = expected(run)
    assert (want_d, want_c, want_stop) == (digests, len(three), OTHER)
    stats = _check(run, gpu, lead)
    assert stats[0] == len(recv_forge.candidates(run)) == 3 and stats[2] == 0


def _forged():
    """Message A's digest ends with the tag, and message B's digest goes on
    like a digest's end, a newline, a size and a newline: byte 20 starts a
    whole message that no parser reading from byte 0 sees."""
    a = message(bytes(9) + b"FILE_BLOCK\n", 1234)
    b = message(b"\xaa\xaa\xaa\n777\n" + b"\xaa" * 12, 99)
    return a + b


@pytest.mark.parametrize("around", [0, 300])
def test_forged_message_start_takes_the_host_fallback(gpu, around):
    before, _, _ = _honest(around, seed=21)
    after, _, _ = _honest(around, seed=22)
    run = before + _forged() + after
    digests, sizes, consumed, stop = expected(run)
    assert len(digests) == 2 * around + 2 and sizes[around:around + 2] == [1234, 99] and stop == END
    stats = _check(run, gpu)
    assert stats[0] == 2 * around + 3 and stats[2] == 1  # candidates [0, 20, 37] when alone
    assert _check(run + b"FILE_END\n", gpu)[2] == 1


def test_forced_fallback_gives_the_same(gpu, knobs):
    run, _, _ = _honest(5000)
    fast = wire.parse_blocks_device(_dev(run + b"FILE_END\n", gpu))
    assert wire.parse_stats()[2] == 0
    knobs.set("SF_TEST_WIRE_PARSE_HOST", 1)
    assert _check(run + b"FILE_END\n", gpu)[2] == 1
    slow = wire.parse_blocks_device(_dev(run + b"FILE_END\n", gpu))
    assert torch.equal(fast[0], slow[0]) and torch.equal(fast[1].view(torch.int32), slow[1].view(torch.int32))
    assert fast[2:] == slow[2:]


@pytest.mark.parametrize("lead", [1, 2, 3])
def test_run_at_odd_offsets_ending_with_its_allocation(gpu, lead):
    run, _, _ = _honest(130, seed=30 + lead)
    assert _check(run, gpu, lead)[2] == 0
    assert _check(run[:-1], gpu, lead)[1] == 129  # the last message one byte short: nothing is read past the end
    assert _check(run[:-20], gpu, lead)[1] == 129


def _table(rng, n=1000):
    table = rng.integers(0, 256, (n, 20), dtype=np.uint8)
    table[rng.integers(0, n, 50)] = table[rng.integers(0, n, 50)]  # repeated digests
    return table, rng.random(n) < 0.7


def _receive_case(rng, table, m=3000):
    q = rng.integers(0, 256, (m, 20), dtype=np.uint8)
    q[::2] = table[rng.integers(0, table.shape[0], (m + 1) // 2)]  # half of them rows of the table
    sizes = _sizes(m, rng)
    return b"".join(message(q[i].tobytes(), sizes[i]) for i in range(m)), sizes


def test_block_set_receive(gpu):
    rng = np.random.default_rng(40)
    table, present = _table(rng)
    run, sizes = _receive_case(rng, table)
    base = 2 ** 40
    want_d, want_s, want_c, _ = expected(run + b"FILE_END\n")
    assert want_s == sizes
    with BlockSet(torch.from_numpy(table).to(gpu), torch.from_numpy(present).to(gpu)) as bset:
        d, s, offsets, rows, consumed, stop, end = bset.receive(_dev(run + b"FILE_END\n", gpu), base_offset=base)
        assert wire.parse_stats()[2] == 0
        assert (consumed, stop) == (want_c, OTHER)
        assert d.cpu().numpy().tobytes() == b"".join(want_d) and s.cpu().numpy().tolist() == want_s
        want_rows = oracle.block_lookup(table, present, np.frombuffer(b"".join(want_d), np.uint8).reshape(-1, 20))
        assert np.array_equal(rows.cpu().numpy(), want_rows) and (want_rows >= 0).any() and (want_rows < 0).any()
        cum = np.cumsum(np.array([0] + want_s, dtype=object))
        assert offsets.cpu().numpy().tolist() == [base + int(c) for c in cum[:-1]]
        assert end == base + int(cum[-1]) and end - base > 1 << 32
        # a run in two pieces: the tail that did not parse goes in front of the next bytes
        cut = len(run) // 2
        d1, s1, o1, r1, c1, stop1, end1 = bset.receive(_dev(run[:cut], gpu), base_offset=base)
        assert stop1 in (INCOMPLETE, END) and c1 <= cut
        d2, s2, o2, r2, c2, stop2, end2 = bset.receive(_dev(run[c1:] + b"FILE_END\n", gpu), base_offset=end1)
        assert (c1 + c2, stop2, end2) == (len(run), OTHER, end)
        assert torch.equal(torch.cat([o1, o2]), offsets) and torch.equal(torch.cat([r1, r2]), rows)
        # an empty run
        d0, s0, o0, r0, c0, stop0, end0 = bset.receive(_dev(b"", gpu), base_offset=7)
        assert (d0.shape[0], c0, stop0, end0) == (0, 0, END, 7)


def _receive_buffer(bset, run: bytes, base, cap):
    L = syncfast_amd.lib()
    n, consumed, end, stop = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
    out = np.zeros(max(cap, 1), host.SIG_DTYPE)
    src = np.zeros(max(cap, 1), np.int64)
    wire_bytes = np.frombuffer(run, np.uint8)
    rc = L.sf_receive_blocks_buffer(bset._h if bset is not None else None, wire_bytes.ctypes.data, wire_bytes.size, base,
                                    out.ctypes.data_as(ctypes.POINTER(_lib.BlockSig)) if cap else None,
                                    src.ctypes.data if cap else None, cap, ctypes.byref(n), ctypes.byref(consumed),
                                    ctypes.byref(stop), ctypes.byref(end))
    return rc, out[:n.value] if cap else out[:0], src[:n.value] if cap else src[:0], n.value, consumed.value, \
        stop.value, end.value


@pytest.mark.parametrize("case", ["honest", "forged"])
def test_receive_from_host_bytes_equals_the_device_route(gpu, case):
    rng = np.random.default_rng(50)
    table, present = _table(rng)
    if case == "honest":
        run, _ = _receive_case(rng, table, m=5000)
    else:
        run = message(table[3].tobytes(), 5) + _forged() + message(table[4].tobytes(), 4294967295)
    run += b"FILE_END\n"
    want_d, want_s, want_c, _ = expected(run)
    with torch.cuda.device(gpu), BlockSet(torch.from_numpy(table).to(gpu), torch.from_numpy(present).to(gpu)) as bset:
        d, s, offsets, rows, consumed, stop, end = bset.receive(_dev(run, gpu), base_offset=2 ** 40)
        fell_back = wire.parse_stats()[2]
        torch.cuda.synchronize()
        # the query form first: the need, the bytes and the stop, nothing written
        rc, _, _, n, c, st, _ = _receive_buffer(bset, run, 2 ** 40, 0)
        assert (rc, n, c, st) == (_lib.SF_ENOSPC, len(want_d), want_c, OTHER)
        rc, out, src, n, c, st, e = _receive_buffer(bset, run, 2 ** 40, len(want_d))
        assert rc == 0 and wire.parse_stats()[2] == fell_back == (case == "forged")
    assert (n, c, st, e) == (len(want_d), consumed, stop, end) == (len(want_d), want_c, OTHER, e)
    assert out["sha1"].tobytes() == b"".join(want_d) == d.cpu().numpy().tobytes()
    assert out["size"].tolist() == want_s == s.cpu().numpy().tolist()
    assert out["offset"].tolist() == offsets.cpu().numpy().tolist()
    assert np.array_equal(src, rows.cpu().numpy())
    assert np.array_equal(src, oracle.block_lookup(table, present, out["sha1"].reshape(-1, 20)))
    # without a set: the rows alone
    with torch.cuda.device(gpu):
        rc, out2, src2, n2, _, _, e2 = _receive_buffer(None, run, 2 ** 40, len(want_d))
    assert rc == 0 and n2 == n and e2 == e and np.array_equal(out2, out) and (src2 == -1).all()


def _two_indexes(seed):
    """Two in-memory indexes with the same contents: files with blocks from a
    small pool (repeated hashes), rows recorded as missing, and the temporary
    file the incoming blocks go to."""
    rng = np.random.default_rng(seed)
    pool = [HashDigest(rng.integers(0, 256, 20, dtype=np.uint8).tobytes()) for _ in range(50)]
    plan = [(f, [(int(rng.integers(0, len(pool))), bool(rng.random() < 0.3)) for _ in range(40)]) for f in range(5)]
    out = []
    for _ in range(2):
        idx = Index.open_in_memory()
        for f, blocks in plan:
            fid, _ = idx.add_file(PurePath(f"dir/f{f}"), DateTimeUtc.from_ns(f))
            for b, (h, missing) in enumerate(blocks):
                (idx.add_missing_block if missing else idx.add_block)(pool[h], fid, b * 4096, 4096)
        out.append((idx, idx.add_temp_file(PurePath("dir/new"))))
    return out, pool, rng


def _dump(idx):
    return (idx.db.execute("SELECT rowid, hash, file_id, offset, size, present FROM blocks ORDER BY rowid;").fetchall(),
            idx.db.execute("SELECT file_id, name, size, blocks_hash, temporary FROM files ORDER BY file_id;").fetchall())


def test_index_receive_file_blocks_is_the_sink_loop(gpu):
    (loop, new), pool, rng = _two_indexes(60)
    fresh = [HashDigest(rng.integers(0, 256, 20, dtype=np.uint8).tobytes()) for _ in range(30)]
    picks = [(pool + fresh)[int(rng.integers(0, 80))] for _ in range(400)]
    sizes = [max(s, 1) for s in _sizes(len(picks), rng)]  # (file_id, offset) is unique in the index: no empty block
    data = b"".join(wire.write_message("FileBlock", h, s) for h, s in zip(picks, sizes)) + wire.write_message("FileEnd")
    # the reference's loop (src/sync/fs.rs:461-480) on one index
    idx, fid = loop
    offset, copies = 0, []
    for msg in wire.Parser().receive(data):
        if msg[0] == "FileBlock":
            found = idx.get_block(msg[1])
            if found is not None:
                copies.append((found[0], found[1], offset, msg[2]))
                idx.add_block(msg[1], fid, offset, msg[2])
            else:
                idx.add_missing_block(msg[1], fid, offset, msg[2])
            offset += msg[2]
        else:
            assert msg == ("FileEnd",)
            idx.set_file_size_and_compute_blocks_hash(fid, offset)
    # the one call on the other
    idx2, fid2 = new
    assert idx2.receive_file_blocks(fid2, data, device=gpu) == copies
    assert 0 < len(copies) < len(picks)
    assert _dump(idx2) == _dump(idx)
    assert idx2.list_missing_blocks() == idx.list_missing_blocks()
    # a run that does not end with FILE_END is refused, and nothing is written
    before = _dump(idx2)
    for bad in (data[:-9], data[:-1], data[:-9] + b"BOGUS\n", data + b"FILE_END\n", data[:-9] + b"COMPLETE\n"):
        with pytest.raises(wire.ProtocolError):
            idx2.receive_file_blocks(fid2, bad, device=gpu)
    assert _dump(idx2) == before
