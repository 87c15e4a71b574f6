"""CPU: the files-list entry points without a device, and the host routes of
Index.file_entries / Index.receive_file_entries.

Every argument check of sf_name_set_build / _lookup / _free,
sf_wire_file_entries_device, sf_receive_file_entries_device and
sf_wire_get_files_device comes before any device call, and a call with nothing
to do launches nothing: all of that runs here, on a machine with no GPU.  The
``device=None`` routes of the two Index methods are held against a
transcription of the reference's sink (file_list_cases.reference_sink,
src/sync/fs.rs:378-446 over wire.Parser) on copies of one index, and
``Index.get_file``'s "first row wins" is pinned on an index that holds a name
twice."""
import ctypes
from pathlib import PurePath

import numpy as np
import pytest

import syncfast_amd
from file_list_cases import H, SCENARIOS, copy, destination, put, reference_sink, run_pieces, table
from syncfast_amd import _lib, wire
from syncfast_amd.index import Index, SyncfastError

EINVAL, MAX = _lib.SF_EINVAL, (1 << 64) - 1
R = ctypes.byref


def _u64(v=7):
    return ctypes.c_uint64(v)


def _run_is_empty(L, h):
    p, nb, nm = ctypes.c_void_p(1), _u64(), _u64()
    assert L.sf_wire_run_info(h, R(p), R(nb), R(nm)) == 0
    assert (p.value, nb.value, nm.value) == (None, 0, 0)
    assert L.sf_wire_run_free(h, None) == 0


def test_constants():
    assert wire.SF_WIRE_END_FILES == _lib.SF_WIRE_END_FILES == 5
    assert _lib.get_knob("SF_TEST_NAME_HASH_MASK") == 0
    L = syncfast_amd.lib()
    assert L.sf_test_file_entries_stats(None) == EINVAL


def test_name_set_checks_arguments_before_any_device_call():
    L = syncfast_amd.lib()
    at = np.zeros(4, np.uint64)
    h, bad = ctypes.c_void_p(5), _u64()
    assert L.sf_name_set_build(None, at.ctypes.data, None, 3, None, R(bad), None) == EINVAL  # no out
    assert L.sf_name_set_build(None, at.ctypes.data, None, 3, R(h), None, None) == EINVAL and h.value is None  # no bad_row
    assert L.sf_name_set_build(None, at.ctypes.data, None, (1 << 31) + 1, R(h), R(bad), None) == EINVAL
    assert L.sf_name_set_build(None, None, None, 1, R(h), R(bad), None) == EINVAL  # rows without a CSR
    for off in range(1, 8):
        assert L.sf_name_set_build(None, 0x10000 + off, None, 1, R(h), R(bad), None) == EINVAL, off
    assert bad.value == MAX and h.value is None
    # no row: a set that needs no device
    assert L.sf_name_set_build(None, None, None, 0, R(h), R(bad), None) == 0 and h.value
    assert L.sf_name_set_lookup(h, None, 0, None, None, 0, None, None) == 0  # nothing asked
    assert L.sf_name_set_lookup(None, None, 0, None, None, 0, None, None) == EINVAL  # no set
    q = 0x10000
    assert L.sf_name_set_lookup(h, None, 0, None, q, 1, q, None) == EINVAL  # queries without their arrays
    assert L.sf_name_set_lookup(h, None, 0, q, None, 1, q, None) == EINVAL
    assert L.sf_name_set_lookup(h, None, 0, q, q, 1, None, None) == EINVAL
    assert L.sf_name_set_lookup(h, None, 5, q, q, 1, q, None) == EINVAL  # bytes announced without a buffer
    for off in range(1, 8):
        assert L.sf_name_set_lookup(h, None, 0, q + off, q, 1, q, None) == EINVAL
        assert L.sf_name_set_lookup(h, None, 0, q, q, 1, q + off, None) == EINVAL
        if off < 4:
            assert L.sf_name_set_lookup(h, None, 0, q, q + off, 1, q, None) == EINVAL
    assert L.sf_name_set_free(h, None) == 0 and L.sf_name_set_free(None, None) == 0


def test_wire_file_entries_checks_arguments_before_any_device_call():
    L = syncfast_amd.lib()
    q = 0x10000
    h, bad = ctypes.c_void_p(5), _u64()

    def call(names=q, at=q, sizes=q, hashes=q, n=1, end=1, run=R(h), badp=R(bad)):
        return L.sf_wire_file_entries_device(names, at, sizes, hashes, n, end, run, badp, None)
    assert call(run=None) == EINVAL and call(badp=None) == EINVAL
    assert call(n=(1 << 31) + 1) == EINVAL
    assert call(at=None) == EINVAL and call(sizes=None) == EINVAL and call(hashes=None) == EINVAL
    for off in range(1, 8):
        assert call(at=q + off) == EINVAL and call(sizes=q + off) == EINVAL
        if off < 4:
            assert call(hashes=q + off) == EINVAL
    assert h.value is None and bad.value == MAX
    assert call(names=None, at=None, sizes=None, hashes=None, n=0, end=0) == 0  # no file, no END_FILES: the empty run
    _run_is_empty(L, h)


def test_wire_get_files_checks_arguments_before_any_device_call():
    L = syncfast_amd.lib()
    q = 0x10000
    h, bad = ctypes.c_void_p(5), _u64()

    def call(data=q, nb=100, at=q, ln=q, n=1, pick=None, n_pick=0, run=R(h), badp=R(bad)):
        return L.sf_wire_get_files_device(data, nb, at, ln, n, pick, n_pick, run, badp, None)
    assert call(run=None) == EINVAL and call(badp=None) == EINVAL
    assert call(n=(1 << 31) + 1) == EINVAL and call(pick=q, n_pick=(1 << 31) + 1) == EINVAL
    assert call(at=None) == EINVAL and call(ln=None) == EINVAL and call(data=None) == EINVAL
    for off in range(1, 8):
        assert call(at=q + off) == EINVAL
        if off < 4:
            assert call(ln=q + off) == EINVAL and call(pick=q + off, n_pick=1) == EINVAL
    assert h.value is None and bad.value == MAX
    assert call(pick=q, n_pick=0) == 0  # an explicit pick of nothing
    _run_is_empty(L, h)
    assert call(data=None, nb=0, at=None, ln=None, n=0) == 0  # all of no span
    _run_is_empty(L, h)


def test_receive_file_entries_checks_arguments_before_any_device_call():
    L = syncfast_amd.lib()
    vals = [_u64(), _u64(), _u64(), _u64(), ctypes.c_int(7)]  # n_out, n_need, bad_name, consumed, stop
    refs = [R(v) for v in vals]
    q = 0x10000

    def call(set_=None, wire_=q, nb=50, have=None, ok=None, outs=(None,) * 7, cap=0, results=refs):
        return L.sf_receive_file_entries_device(set_, wire_, nb, have, ok, *outs, cap, *results, None)

    def state():
        return [v.value for v in vals]
    assert call(wire_=None, nb=0) == 0 and state() == [0, 0, MAX, 0, 0]  # no bytes: nothing launched, no device
    assert call(wire_=None) == EINVAL  # bytes announced without a buffer
    assert call(nb=(1 << 35) + 1) == EINVAL
    for k in range(5):
        assert call(results=refs[:k] + [None] + refs[k + 1:]) == EINVAL, k
    # name_at, name_len, sizes, hashes | rows, need, need_list
    for j, align in enumerate((8, 4, 8, 4, 8, 1, 4)):
        for off in range(1, align):
            outs = [None] * 7
            outs[j] = q + off
            assert call(set_=0x1000 if j >= 4 else None, have=q if j >= 4 else None, outs=outs) == EINVAL, (j, off)
    for j in (4, 5, 6):  # a lookup output and no set
        outs = [None] * 7
        outs[j] = q
        assert call(outs=outs) == EINVAL
    assert call(set_=0x1000) == EINVAL  # a set and no recorded hashes
    for off in (1, 2, 3):
        assert call(set_=0x1000, have=q + off) == EINVAL
    assert state() == [0, 0, MAX, 0, 0]
    out = (ctypes.c_uint64 * 4)(9, 9, 9, 9)
    assert L.sf_test_file_entries_stats(out) == 0 and list(out) == [0, 0, 0, 0]  # reset by the calls above
    assert wire.file_entries_stats() == (0, 0, 0, 0)


def test_get_file_takes_the_first_row_of_a_repeated_name():
    """The schema has no UNIQUE on name: get_file answers the lowest row
    (idx_files_name is in (name, rowid) order), whatever was inserted when --
    what sf_name_set_lookup is defined by."""
    idx = Index.open_in_memory()
    put(idx, "other", H(1))
    first = put(idx, "twice", H(2))
    put(idx, "between", H(3))
    second = put(idx, "twice", H(4))
    assert first < second
    assert idx.get_file(PurePath("twice"))[::2] == (first, H(2))
    idx.begin()
    idx.db.execute("UPDATE files SET temporary = 1 WHERE file_id = ?;", (first,))
    assert idx.get_file(PurePath("twice"))[::2] == (second, H(4))  # the lowest row that is not temporary
    idx.db.execute("UPDATE files SET temporary = 1 WHERE file_id = ?;", (second,))
    assert idx.get_file(PurePath("twice")) is None


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_receive_file_entries_is_the_references_sink(name):
    kwargs, pieces, expect = SCENARIOS[name]
    base = destination(**kwargs)
    ref, got = copy(base), copy(base)
    if isinstance(expect, str):  # the reference returns Err there, with the earlier entries applied
        with pytest.raises(SyncfastError, match=expect):
            reference_sink(ref, pieces)
        with pytest.raises(SyncfastError, match=expect):
            run_pieces(got, pieces)
        assert table(got) == table(ref) != table(base)
        return
    n, needed, requests = reference_sink(ref, pieces)
    k, names, req, calls = run_pieces(got, pieces)
    assert (k, names, req) == (n, needed, requests) and names == expect
    assert table(got) == table(ref)
    assert (table(got) != table(base)) == bool(expect)
    ended = b"END_FILES\n" in pieces[-1]
    carried = len(pieces[0]) - calls[0][0] if len(pieces) > 1 else 0  # the first piece's unconsumed tail
    assert calls[-1] == (carried + len(pieces[-1]), wire.SF_WIRE_END_FILES if ended else wire.SF_WIRE_END)
    assert (req is not None) == ended
    if len(pieces) > 1:
        assert calls[0][1] == wire.SF_WIRE_INCOMPLETE and 0 < calls[0][0] < len(pieces[0])
    if ended:  # the requests parse back to the temp rows, in list_temp_files' order
        assert [m[1] for m in wire.Parser().receive(req)] == [
            str(syncfast_amd.index.untemp_name(t)).encode() for t in got.list_temp_files()]


def test_receive_file_entries_stops_where_the_parser_does():
    base = destination()
    e = wire.write_message("FileEntry", b"unknown", 1, H(9))
    for tail, stop in ((b"COMPLETE\n", wire.SF_WIRE_OTHER), (b"FILE_BLOCK\nxx", wire.SF_WIRE_OTHER),
                       (b"BOGUS\n", wire.SF_WIRE_MALFORMED), (b"FILE_ENTRY\nn\n1x\n", wire.SF_WIRE_MALFORMED),
                       (b"FILE_ENTRY\nn\n1", wire.SF_WIRE_INCOMPLETE), (b"", wire.SF_WIRE_END)):
        got = copy(base).receive_file_entries(e + tail)
        assert got == (1, len(e), stop, [b"unknown"], None), tail


def _source():
    idx = Index.open_in_memory()
    put(idx, "a", H(1), size=0)
    put(idx, "dir/b", H(2), size=9)
    put(idx, "n" * 100, H(3), size=10 ** 15 - 1)
    put(idx, "tmp/.syncfast_tmp_t", H(4), temporary=1)  # not listed
    put(idx, "dir/é", H(5), size=10)
    return idx


def test_file_entries_is_the_write_message_loop():
    idx = _source()
    want = b"".join(wire.write_message("FileEntry", str(p).encode(), size, bh)
                    for _id, p, _m, size, bh in idx.list_files()) + wire.write_message("EndFiles")
    got = idx.file_entries()
    assert got == want and got.count(b"FILE_ENTRY\n") == 4
    msgs = wire.Parser().receive(got)
    assert [m[0] for m in msgs] == ["FileEntry"] * 4 + ["EndFiles"] and msgs[2][1:3] == (b"n" * 100, 10 ** 15 - 1)
    assert Index.open_in_memory().file_entries() == b"END_FILES\n"


@pytest.mark.parametrize("name, size, blocks_hash", [("n" * 101, 1, H(1)), ("a\nb", 1, H(1)), ("big", 10 ** 15, H(1)),
                                                     ("nohash", 1, None)])
def test_file_entries_refuses_what_the_protocol_cannot_carry(name, size, blocks_hash):
    idx = _source()
    put(idx, name, blocks_hash, size=size)
    put(idx, "after", H(9))
    with pytest.raises(SyncfastError, match="cannot carry"):
        idx.file_entries()
