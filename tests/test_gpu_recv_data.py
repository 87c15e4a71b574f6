"""GPU: a received BLOCK_DATA run parsed and verified on the device
(sf_receive_block_data_device / _buffer) and as the sink's GetBlocks state
(Index.receive_block_data).  What a run must parse to always comes from
wire.Parser / wire.write_message and hashlib (data_expect.py), never from the
code under test."""
import ctypes
import hashlib
import random

import numpy as np
import pytest
import torch

import recv_expect
import syncfast_amd
from data_expect import (END, INCOMPLETE, MALFORMED, OTHER, OTHERS, TAG, candidates, dense_run, expected, header,
                         honest_run, message, needs_walk)
from syncfast_amd import _lib, host, wire
from syncfast_amd.digest import HashDigest
from syncfast_amd.index import Index, temp_name

pytestmark = pytest.mark.gpu


def _dev(run: bytes, gpu, lead=0):
    """`run` in HBM, `lead` bytes into an allocation that ends with it."""
    t = torch.empty(lead + len(run), dtype=torch.uint8, device=gpu)
    if run:
        t[lead:] = torch.frombuffer(bytearray(run), dtype=torch.uint8).to(gpu)
    return t[lead:]


def _want_ok(run, digests, sizes, offsets):
    return [int(hashlib.sha1(run[o:o + s]).digest() == d) for d, s, o in zip(digests, sizes, offsets)]


def _check(run: bytes, gpu, lead=0, verify=True):
    """receive_block_data_device(run) is what the parser reads and hashlib
    verifies; returns (outputs, stats)."""
    want_d, want_s, want_o, want_c, want_stop, want_need = expected(run)
    got = wire.receive_block_data_device(_dev(run, gpu, lead), verify=verify)
    d, s, o, ok, consumed, stop, need = got
    assert (d.shape[0], consumed, stop, need) == (len(want_d), want_c, want_stop, want_need)
    assert d.cpu().numpy().tobytes() == b"".join(want_d)
    assert s.cpu().numpy().tolist() == want_s and o.cpu().numpy().tolist() == want_o
    if verify:
        assert ok.cpu().numpy().tolist() == _want_ok(run, want_d, want_s, want_o)
    else:
        assert ok is None
    stats = wire.block_data_stats()
    assert stats[1] == len(want_d) and stats[0] >= stats[1] and stats[3] == (16 * stats[0] if stats[2] else 0)
    return got, stats


def _same(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y


@pytest.mark.parametrize("n", [0, 1, 2, 64, 65, 257])
def test_honest_runs(gpu, knobs, n):
    run = honest_run(random.Random(100 + n), n)
    want = expected(run)
    assert (len(want[0]), want[3], want[4]) == (n, len(run), END) and not needs_walk(run)
    got, stats = _check(run, gpu)
    assert got[3].cpu().numpy().tolist() == [1] * n
    assert stats[2] == 0  # no walk: the chain was found on the device
    knobs.set("SF_TEST_BLOCK_DATA_WALK", 1)
    forced, stats = _check(run, gpu)
    assert stats[2] == (1 if n else 0)
    _same(got, forced)


def test_n_bad_is_reported_through_the_c_abi(gpu):
    run = honest_run(random.Random(3), 5)
    run = _flip(run, expected(run)[2][1])  # the second payload's one byte (the first is empty)
    L = syncfast_amd.lib()
    t = _dev(run, gpu)
    d = torch.empty((5, 20), dtype=torch.uint8, device=gpu)
    s = torch.empty(5, dtype=torch.int32, device=gpu)
    o = torch.empty(5, dtype=torch.int64, device=gpu)
    ok = torch.empty(5, dtype=torch.uint8, device=gpu)
    n, consumed, stop, need, bad = (ctypes.c_uint64(9), ctypes.c_uint64(9), ctypes.c_int(9), ctypes.c_uint64(9),
                                    ctypes.c_uint64(9))
    refs = tuple(ctypes.byref(v) for v in (n, consumed, stop, need, bad))
    stream = torch.cuda.current_stream(gpu).cuda_stream
    args = (t.data_ptr(), t.numel(), d.data_ptr(), s.data_ptr(), o.data_ptr())
    assert L.sf_receive_block_data_device(*args, ok.data_ptr(), 5, *refs, stream) == 0
    assert (n.value, consumed.value, stop.value, need.value, bad.value) == (5, len(run), END, 0, 1)
    assert ok.cpu().numpy().tolist() == [1, 0, 1, 1, 1]
    # capacity: the query form, one short, and parse only
    assert L.sf_receive_block_data_device(t.data_ptr(), t.numel(), None, None, None, None, 0, *refs,
                                          stream) == _lib.SF_ENOSPC
    assert (n.value, consumed.value, bad.value) == (5, len(run), 0)
    d.zero_()
    ok.fill_(7)
    assert L.sf_receive_block_data_device(*args, ok.data_ptr(), 4, *refs, stream) == _lib.SF_ENOSPC
    assert n.value == 5 and bad.value == 0
    assert d[:4].cpu().numpy().tobytes() == b"".join(expected(run)[0][:4]) and int(d[4].sum()) == 0
    assert ok.cpu().numpy().tolist() == [7] * 5  # nothing hashed
    assert L.sf_receive_block_data_device(*args, None, 5, *refs, stream) == 0
    assert (n.value, bad.value) == (5, 0) and ok.cpu().numpy().tolist() == [7] * 5
    _check(run, gpu, verify=False)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_placement_in_the_allocation(gpu, lead):
    """The run starts 0 to 3 bytes into its allocation and ends with it; the
    last message's end byte is the buffer's last byte."""
    run = honest_run(random.Random(11), 14)
    _, stats = _check(run, gpu, lead)
    assert stats[2] == 0


@pytest.mark.parametrize("lead", [0, 3])
def test_file_block_messages_as_payloads_and_after_the_run(gpu, lead):
    """The other receive parser's message kind as the hostile content: every
    payload is a whole FILE_BLOCK message (the shortest, the longest and one
    between), and one follows the run.  None of that is a BLOCK_DATA
    candidate."""
    rng = random.Random(13)
    payloads = [recv_expect.message(rng.randbytes(20), size) for size in (b"7", b"4294967295", b"+00000000000012")]
    assert [len(p) for p in payloads] == [34, 43, 48]
    three = b"".join(message(p) for p in payloads)
    run = three + recv_expect.message(rng.randbytes(20), 99)
    assert len(recv_expect.expected(run[len(three):])[0]) == 1 and 100 < len(run) < 400
    want = expected(run)
    assert (want[1], want[3], want[4]) == ([34, 43, 48], len(three), OTHER)
    got, stats = _check(run, gpu, lead)
    assert got[3].cpu().numpy().tolist() == [1, 1, 1]
    assert stats[0] == len(candidates(run)) == 3 and stats[2] == 0


@pytest.mark.parametrize("at", [15, 16, 63, 64])
def test_message_start_at_each_lane_and_word_edge(gpu, at):
    """The second and third message start at `at` mod 64 (a lane's last and
    first position, a bitmap word's last and first)."""
    first = (at - 36) % 64  # a two-digit payload length that ends the first message (35 + length + 1) at `at` mod 64
    first += 64 if first < 10 else 0
    rng = random.Random(at)
    second = message(rng.randbytes(64 - 36))  # 64 bytes: the third starts at the same residue
    run = message(rng.randbytes(first)) + second + message(rng.randbytes(300)) + message(b"")
    want = expected(run)
    assert (want[2][1] - 35) % 64 == at % 64 and (want[2][2] - 36) % 64 == at % 64
    _, stats = _check(run, gpu)
    assert stats[2] == 0


def test_a_b_in_each_of_the_last_bytes(gpu):
    """A 'B' k bytes before the end, k = 1 .. 11, as payload and as a cut tail:
    the candidate test reads nothing past the run."""
    base = honest_run(random.Random(12), 3)
    for k in range(1, 12):
        payload = bytes(20 - k) + b"B" + b"L" * (k - 1)
        _check(base + message(payload)[:-1], gpu)  # the 'B' k bytes before the end, the end byte missing
        _check(base + TAG[:k], gpu)
        for lead in (1, 3):
            _check(base + message(bytes(7)) + TAG[:k], gpu, lead)


def _nested_cases():
    rng = random.Random(21)
    inner = message(rng.randbytes(50))
    deep = message(b"x" + message(b"yy" + message(rng.randbytes(10)) + b"z") + b"w")
    later = message(rng.randbytes(70))
    # a header in the first payload whose length lands on `later`'s end byte
    crossing_payload = header(len(later) + 2) + b"qq"
    return {
        "whole_message": message(inner) + later,
        "three_deep": message(deep) + later,
        "nested_cut_short": message(inner[:-7]) + later + message(inner[:40]),
        "overshoot_onto_later_end_byte": message(crossing_payload) + later + message(b"tail"),
        "run_of_B": message(b"B" * 4096) + later,
        "run_of_tags": message(TAG * 40) + later,
        "newlines": message(b"\n" * 300) + later,
    }


@pytest.mark.parametrize("name", sorted(_nested_cases()))
def test_nested_and_crossing_payloads(gpu, name):
    """The stats report the walk exactly where the reference model's link
    test needs one: a whole message in a payload, three deep, a header that
    overshoots onto a later end byte.  A nested message cut short, 4096 'B's,
    repeated tags and newlines hold no whole message -- no candidate lies
    inside -- so the device chain must take them without a walk."""
    run = _nested_cases()[name]
    want = expected(run)
    assert want[3:5] == (len(run), END)
    (_, _, _, ok, *_), stats = _check(run, gpu)
    assert ok.cpu().numpy().tolist() == [1] * len(want[0])
    walks = name in ("whole_message", "three_deep", "overshoot_onto_later_end_byte")
    assert needs_walk(run) == walks  # the reference model: which of these a parallel parser must walk
    assert stats[2] == int(walks)
    if walks:
        assert stats[0] > stats[1] and stats[3] == 16 * stats[0]


def test_walk_prefix_then_stop(gpu):
    """A nested message in the first payload and a malformed tail: the walk's
    chain ends where the parser stops."""
    inner = message(b"inner")
    run = message(inner + inner) + message(b"after") + message(b"x", end=b"X") + message(b"never")
    want = expected(run)
    assert len(want[0]) == 2 and want[4] == MALFORMED and needs_walk(run)
    _, stats = _check(run, gpu)
    assert stats[2] == 1


def test_more_candidates_than_messages_fit(gpu):
    """A hostile run with a candidate every 21 bytes -- more candidates than
    n / 35 + 1, the most messages a run can hold: the list is sized by the
    candidates, the outputs by the messages.  One message, the whole run."""
    run = dense_run(200)
    want = expected(run)
    assert len(want[0]) == 1 and want[3:5] == (len(run), END)
    assert len(candidates(run)) > len(run) // 35 + 1 and needs_walk(run)
    (_, _, _, ok, *_), stats = _check(run, gpu)
    assert stats[0] == len(candidates(run)) and stats[2] == 1
    assert ok.cpu().numpy().tolist() == [0]  # its digest is not its payload's


def _flip(run: bytes, at: int) -> bytes:
    return run[:at] + bytes([run[at] ^ 0x10]) + run[at + 1:]


def test_corruption(gpu):
    run = honest_run(random.Random(31), 65)
    _, sizes, offsets, *_ = expected(run)
    # one flipped bit in one payload
    bad = _flip(run, offsets[40] + sizes[40] // 2)
    (_, _, _, ok, *_), _ = _check(bad, gpu)
    assert ok.cpu().numpy().tolist() == [int(i != 40) for i in range(65)]
    # one flipped bit in a claimed digest (a 35-byte header: its digest is bytes -24 .. -5 from the payload)
    bad = _flip(run, offsets[7] - 20)
    assert expected(bad)[1:3] == (sizes, offsets)
    (_, _, _, ok, *_), _ = _check(bad, gpu)
    assert ok.cpu().numpy().tolist() == [int(i != 7) for i in range(65)]
    # a wrong end byte: malformed at that message, the prefix parsed and verified
    at = offsets[20] + sizes[20]
    bad = run[:at] + b"X" + run[at + 1:]
    want = expected(bad)
    assert len(want[0]) == 20 and want[4] == MALFORMED
    (_, _, _, ok, *_), _ = _check(bad, gpu)
    assert ok.cpu().numpy().tolist() == [1] * 20


def test_tails(gpu):
    three = honest_run(random.Random(41), 3)
    d = bytes(range(100, 120))
    cases = [(cmd + b"\n" + b"rest", OTHER) for cmd in OTHERS]
    cases += [(b"BOGUS\n", MALFORMED), (b"X" * 20, MALFORMED), (b"X" * 19, INCOMPLETE),
              (TAG + d + b"x5\nhello\n", MALFORMED), (TAG + d + b"\n1a\nx\n", MALFORMED),
              (TAG + d + b"\n\n\n", MALFORMED), (TAG + d + b"\n" + b"1" * 16 + b"\n", MALFORMED),
              (TAG + d + b"\n999999999999999\n", INCOMPLETE), (TAG + d + b"\n000000000000005\nabc", INCOMPLETE)]
    last = message(random.Random(42).randbytes(300))
    cuts = list(range(1, 37)) + [36 + 150, 36 + 299, len(last) - 1]  # header bytes, payload first/middle/last, no end byte
    cases += [(last[:k], INCOMPLETE) for k in cuts]
    for tail, want_stop in cases:
        run = three + tail
        want = expected(run)
        assert (len(want[0]), want[3], want[4]) == (3, len(three), want_stop), tail
        _, stats = _check(run, gpu)
        assert stats[2] == 0, tail
        assert expected(tail)[4] == want_stop and _check(tail, gpu)[1][1] == 0, tail
    assert expected(three + last[:36])[5] == len(last) and expected(three + last[:35])[5] == 0
    assert expected(three + TAG + d + b"\n999999999999999\n")[5] == 48 + 999999999999999 + 1


def test_a_length_above_uint32_in_the_chain(gpu):
    """Only a chained message can be too large, and it cannot fit a test; the
    incomplete one is reported with its need."""
    run = message(b"abc") + header(1 << 32) + b"xyz"
    want = expected(run)
    assert want[4] == INCOMPLETE and want[5] == 43 + (1 << 32) + 1
    _check(run, gpu)


def _buffer(run: bytes, verify=True):
    """sf_receive_block_data_buffer through the C-ABI, with n_bad; the ok
    bytes start out as 7s, so an entry the call does not write shows."""
    a = np.frombuffer(run, np.uint8)
    cap = len(run) // 35 + 1
    rows = np.zeros(cap, host.SIG_DTYPE)
    ok = np.full(cap, 7, np.uint8)
    n, c, st, nd, nb = (ctypes.c_uint64(9), ctypes.c_uint64(9), ctypes.c_int(9), ctypes.c_uint64(9), ctypes.c_uint64(9))
    _lib.check(syncfast_amd.lib().sf_receive_block_data_buffer(
        a.ctypes.data if a.size else None, a.size, rows.ctypes.data_as(ctypes.POINTER(_lib.BlockSig)),
        ok.ctypes.data if verify else None, cap, ctypes.byref(n), ctypes.byref(c), ctypes.byref(st), ctypes.byref(nd),
        ctypes.byref(nb)), "sf_receive_block_data_buffer")
    return rows[:n.value], ok[:n.value], c.value, st.value, nd.value, nb.value


def _check_buffer(run: bytes):
    """The buffer route's outputs are what the parser reads and hashlib
    verifies -- held against the reference model, not against another call."""
    want_d, want_s, want_o, want_c, want_stop, want_need = expected(run)
    want_ok = _want_ok(run, want_d, want_s, want_o)
    rows, ok, consumed, stop, need, n_bad = _buffer(run)
    assert (len(rows), consumed, stop, need) == (len(want_d), want_c, want_stop, want_need)
    assert rows["sha1"].tobytes() == b"".join(want_d)
    assert rows["size"].tolist() == want_s and rows["offset"].tolist() == want_o
    assert ok.tolist() == want_ok and n_bad == want_ok.count(0)
    return rows, ok


def test_buffer_route_equals_the_device_route(gpu, knobs):
    rng = random.Random(51)
    honest = honest_run(rng, 65)
    _, sizes, offsets, *_ = expected(honest)
    two_bad = _flip(_flip(honest, offsets[9] + 1), offsets[50] + 1)
    runs = [b"", honest, honest + TAG + bytes(20) + b"\n77\nabc", _flip(honest, offsets[9] + 1), two_bad,
            honest[:offsets[30] + sizes[30]] + b"X", honest + b"FILE_END\n"] + list(_nested_cases().values())
    # a run of another length whose bad payloads are others: run before every
    # call under test, so nothing a call leaves behind on the device can pass
    # for the next call's verdict
    other = honest_run(rng, 40)
    other_offsets = expected(other)[2]
    for i in (1, 2, 5, 9, 10, 30):
        other = _flip(other, other_offsets[i])
    for run in runs:
        (d, s, o, ok, consumed, stop, need), dstats = _check(run, gpu)
        for mode in (2, 0):  # the serial host parse of the caller's bytes, and the device parse
            knobs.set("SF_TEST_BLOCK_DATA_WALK", 0)
            _check_buffer(other)
            knobs.set("SF_TEST_BLOCK_DATA_WALK", mode)
            rows, bok = _check_buffer(run)
            assert rows["sha1"].tobytes() == d.cpu().numpy().tobytes()
            assert bok.tolist() == ok.cpu().numpy().tolist()
            if mode == 0:
                assert wire.block_data_stats() == dstats
        knobs.set("SF_TEST_BLOCK_DATA_WALK", 0)
    # the Python wrapper, with and without verification
    rows, bok, consumed, stop, need = host.receive_block_data(two_bad)
    assert bok.tolist() == [int(i not in (9, 50)) for i in range(65)] and (consumed, stop, need) == (len(two_bad), END, 0)
    rows, bok, *_ = host.receive_block_data(honest, verify=False)
    assert bok is None and rows["size"].tolist() == sizes
    rows, bok, *_, n_bad = _buffer(two_bad, verify=False)
    assert bok.tolist() == [7] * 65 and n_bad == 0  # parse only: nothing hashed, nothing written
    # capacity one short through the C-ABI: the need, nothing else
    L = syncfast_amd.lib()
    a = np.frombuffer(honest, np.uint8)
    out = np.zeros(64, host.SIG_DTYPE)
    n, c, st, nd, nb = (ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0), ctypes.c_uint64(0), ctypes.c_uint64(0))
    rc = L.sf_receive_block_data_buffer(a.ctypes.data, a.size, out.ctypes.data_as(ctypes.POINTER(_lib.BlockSig)), None,
                                        64, ctypes.byref(n), ctypes.byref(c), ctypes.byref(st), ctypes.byref(nd),
                                        ctypes.byref(nb))
    assert rc == _lib.SF_ENOSPC and n.value == 65 and int(out["size"].sum()) == 0


def test_index_receive_block_data_end_to_end(gpu, tmp_path):
    """A destination index with missing blocks receives a run: verified
    blocks are marked and listed for writing, applying the write list to the
    temp files reproduces the source bytes, a corrupted block is rejected and
    still missing."""
    rng = random.Random(61)
    blocks = [rng.randbytes(s) for s in (5000, 1, 32768, 0, 777, 4096)]
    files = {"a.bin": [0, 1, 2, 0, 3], "sub/b.bin": [4, 2, 5]}  # block 0 twice in a.bin, block 2 in both
    idx = Index.open_in_memory()
    source = {}
    for name, order in files.items():
        file_id, at = idx.add_temp_file(name), 0
        for b in order:
            idx.add_missing_block(HashDigest(hashlib.sha1(blocks[b]).digest()), file_id, at, len(blocks[b]))
            at += len(blocks[b])
        source[name] = b"".join(blocks[b] for b in order)
    idx.commit()
    run = b"".join(message(b) for b in blocks)
    offsets = expected(run)[2]
    run = _flip(run, offsets[4] + 100)  # block 4 arrives corrupted
    data = run + message(rng.randbytes(50))[:60]  # and the next message has not arrived whole
    writes, rejected, consumed = idx.receive_block_data(data, device=gpu)
    assert consumed == len(run)
    assert rejected == [HashDigest(hashlib.sha1(blocks[4]).digest())]
    assert idx.list_missing_blocks() == rejected
    (tmp_path / "sub").mkdir()
    for name in files:  # the temp files, at their full size
        (tmp_path / temp_name(name)).write_bytes(bytes(len(source[name])))
    for name, offset, start, size in writes:  # write_block (src/sync/fs.rs:42-51) per entry
        with open(tmp_path / name, "r+b") as f:
            f.seek(offset)
            f.write(data[start:start + size])
    assert (tmp_path / temp_name("a.bin")).read_bytes() == source["a.bin"]
    want_b = bytearray(source["sub/b.bin"])
    want_b[:777] = bytes(777)  # the rejected block was not written
    assert (tmp_path / temp_name("sub/b.bin")).read_bytes() == bytes(want_b)
    assert len(writes) == 7
    # the source sends the block again, intact: nothing is missing any more
    writes, rejected, consumed = idx.receive_block_data(message(blocks[4]), device=gpu)
    assert rejected == [] and idx.list_missing_blocks() == []
    assert [(str(w[0]), w[1], w[3]) for w in writes] == [("sub/.syncfast_tmp_b.bin", 0, 777)]
    # another command, or bytes the parser raises on, after the messages: an error, nothing marked
    idx2 = Index.open_in_memory()
    fid = idx2.add_temp_file("c")
    idx2.add_missing_block(HashDigest(hashlib.sha1(blocks[1]).digest()), fid, 0, 1)
    for tail in (b"COMPLETE\n", b"BOGUS\n"):
        with pytest.raises(wire.ProtocolError):
            idx2.receive_block_data(message(blocks[1]) + tail, device=gpu)
        assert len(idx2.list_missing_blocks()) == 1
    # without verification a corrupted payload is taken, as the reference takes it
    writes, rejected, _ = idx2.receive_block_data(message(b"?", hashlib.sha1(blocks[1]).digest()), device=gpu,
                                                  verify=False)
    assert rejected == [] and len(writes) == 1 and idx2.list_missing_blocks() == []
