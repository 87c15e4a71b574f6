"""CPU: sf_wire_parse_get_files_device and sf_serve_get_files_device without a
device, and the host route of Index.serve_get_file_requests.

Every argument check of the two entry points comes before any device call, and
a call with no bytes launches nothing: all of that runs here, on a machine with
no GPU.  ``Index.serve_get_file_requests(device=None)`` is held against a
transcription of the reference's source (src/sync/fs.rs:177-231 over
wire.Parser) on copies of one index."""
import ctypes
import random
from pathlib import PurePath

import pytest

import syncfast_amd
from entries_expect import get_files_run, utf8_ok
from get_files_expect import ALL, BAD_NAME, END, FULL, INCOMPLETE, MALFORMED, OTHER, UNKNOWN, expected
from send_files_expect import parse_back, reference_loop, source_index
from syncfast_amd import _lib, wire

EINVAL, MAX = _lib.SF_EINVAL, (1 << 64) - 1
R = ctypes.byref
Q = 0x10000  # an address nothing reads: every call here returns before any device call


def _u64(v=7):
    return ctypes.c_uint64(v)


def test_constants_and_the_stats_hook():
    assert (wire.SF_SERVE_ALL, wire.SF_SERVE_BAD_NAME, wire.SF_SERVE_UNKNOWN, wire.SF_SERVE_FULL) == (0, 1, 2, 3)
    assert (ALL, BAD_NAME, UNKNOWN, FULL) == (0, 1, 2, 3)
    L = syncfast_amd.lib()
    assert L.sf_test_serve_files_stats(None) == EINVAL
    assert "sf_test_serve_files_stats" in _lib.EXPORTED_TEST
    assert {"sf_wire_parse_get_files_device", "sf_serve_get_files_device"} <= set(_lib.EXPORTED)


def test_parse_checks_arguments_before_any_device_call():
    L = syncfast_amd.lib()
    n, bad, used, stop = _u64(), _u64(), _u64(), ctypes.c_int(7)

    def call(wire_=Q, nb=100, at=Q, ln=Q, cap=10, n_out=R(n), badp=R(bad), usedp=R(used), stopp=R(stop)):
        return L.sf_wire_parse_get_files_device(wire_, nb, at, ln, cap, n_out, badp, usedp, stopp, None)
    assert call(n_out=None) == EINVAL and call(badp=None) == EINVAL and call(usedp=None) == EINVAL and call(stopp=None) == EINVAL
    assert call(wire_=None) == EINVAL  # bytes announced without a buffer
    assert call(nb=(1 << 35) + 1) == EINVAL
    for off in range(1, 8):
        assert call(at=Q + off) == EINVAL, off
        if off < 4:
            assert call(ln=Q + off) == EINVAL, off
    assert (n.value, bad.value, used.value, stop.value) == (0, MAX, 0, END)
    # no bytes: nothing is launched, no device is needed, outputs or not
    for at, ln in ((Q, Q), (None, None), (Q, None)):
        n.value, bad.value, used.value, stop.value = 7, 7, 7, 7
        assert call(wire_=None, nb=0, at=at, ln=ln) == 0
        assert (n.value, bad.value, used.value, stop.value) == (0, MAX, 0, END)


def test_serve_checks_arguments_before_any_device_call():
    L = syncfast_amd.lib()
    h = ctypes.c_void_p(5)
    nreq, nans, ab, bad, used = (_u64() for _ in range(5))
    why, stop = ctypes.c_int(7), ctypes.c_int(7)
    results = dict(run=R(h), nreq=R(nreq), nans=R(nans), ab=R(ab), why=R(why), bad=R(bad), used=R(used), stop=R(stop))

    def call(set_=Q, first=Q, digests=Q, sizes=Q, n_blocks=5, req=Q, nb=100, max_run=0, **kw):
        p = dict(results, **kw)
        return L.sf_serve_get_files_device(set_, first, digests, sizes, n_blocks, req, nb, max_run, p["run"], p["nreq"],
                                           p["nans"], p["ab"], p["why"], p["bad"], p["used"], p["stop"], None)
    for k in results:
        assert call(**{k: None}) == EINVAL, k
    assert call(set_=None) == EINVAL and call(req=None) == EINVAL and call(first=None) == EINVAL
    assert call(digests=None) == EINVAL and call(sizes=None) == EINVAL  # blocks without their table
    assert call(nb=(1 << 35) + 1) == EINVAL and call(n_blocks=(1 << 32) + 1) == EINVAL
    for off in range(1, 8):
        assert call(first=Q + off) == EINVAL, off
        if off < 4:
            assert call(digests=Q + off) == EINVAL and call(sizes=Q + off) == EINVAL, off
    assert h.value is None and bad.value == MAX
    assert (nreq.value, nans.value, ab.value, why.value, used.value, stop.value) == (0, 0, 0, ALL, 0, END)
    # no bytes: the empty run and SF_WIRE_END, nothing launched, no device, no set
    for kw in ({}, dict(set_=None, first=None, digests=None, sizes=None, n_blocks=0), dict(max_run=1)):
        h.value, why.value, stop.value, nreq.value = 5, 7, 7, 7
        assert call(req=None, nb=0, **kw) == 0
        assert (nreq.value, nans.value, ab.value, why.value, bad.value, used.value, stop.value) == (0, 0, 0, ALL, MAX, 0, END)
        p, nbytes, nm = ctypes.c_void_p(1), _u64(), _u64()
        assert L.sf_wire_run_info(h, R(p), R(nbytes), R(nm)) == 0 and (p.value, nbytes.value, nm.value) == (None, 0, 0)
        assert L.sf_wire_run_free(h, None) == 0
    out = (ctypes.c_uint64 * 4)(9, 9, 9, 9)
    assert L.sf_test_serve_files_stats(out) == 0 and list(out) == [0, 0, 0, 0]


# ------------------------------------ Index.serve_get_file_requests(device=None)

def respond(idx, data: bytes, max_run_bytes: int = 0):
    """FsSource's Respond and ListBlocks states over what wire.Parser reads
    from ``data`` (src/sync/fs.rs:177-231): String::from_utf8, get_file,
    FILE_START, list_file_blocks, FILE_END, name by name."""
    e = expected(data)
    out, answered, why = b"", 0, ALL
    for name in e.names:
        if not utf8_ok(name):
            why = BAD_NAME  # Error::BadFilenameEncoding
            break
        found = idx.get_file(PurePath(name.decode()))
        if found is None:
            why = UNKNOWN  # "Requested file is unknown"
            break
        answer = wire.write_message("FileStart", name) + b"".join(
            wire.write_message("FileBlock", h, size) for h, _o, size in idx.list_file_blocks(found[0])) + wire.write_message("FileEnd")
        if max_run_bytes and len(out) + len(answer) > max_run_bytes:
            why = FULL
            break
        out += answer
        answered += 1
    used = e.name_at[answered - 1] + e.name_len[answered - 1] + 1 if answered else 0
    return out, len(e.names), answered, used, why, e.consumed, e.stop


@pytest.fixture(scope="module")
def source():
    return source_index(random.Random(61))


CASES = {
    "all": ([b"a.bin", b"dir/empty", b"dir/b.bin", b"x/FILE_END", b"z"], b"", ALL, 5),
    "unknown_in_the_middle": ([b"a.bin", b"nope", b"z"], b"", UNKNOWN, 1),
    "a_temporary_files_name": ([b"z", b".syncfast_tmp_incoming.bin", b"a.bin"], b"", UNKNOWN, 1),
    "the_temp_files_own_name": ([b"z", b"incoming.bin"], b"", UNKNOWN, 1),
    "a_repeated_request": ([b"dir/b.bin", b"z", b"dir/b.bin", b"dir/empty", b"dir/empty"], b"", ALL, 5),
    "a_bad_encoding": ([b"a.bin", b"z", b"\xff\xfe", b"a.bin"], b"", BAD_NAME, 2),
    "bad_encoding_before_unknown": ([b"\xc0\x80", b"nope"], b"", BAD_NAME, 0),
    "then_complete": ([b"a.bin"], b"COMPLETE\n", ALL, 1),
    "then_half_a_request": ([b"a.bin", b"z"], b"GET_FILE\ndir/b", ALL, 2),
    "then_garbage": ([b"z"], b"BOGUS\n", ALL, 1),
    "nothing": ([], b"", ALL, 0),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_host_route_is_the_reference_loop(source, case):
    idx, _added = source
    names, tail, why, answered = CASES[case]
    data = get_files_run(names) + tail
    got = idx.serve_get_file_requests(data)
    assert got == respond(idx, data)
    run, n_requests, n_answered, used, got_why, consumed, stop = got
    assert (n_requests, n_answered, got_why) == (len(names), answered, why)
    assert stop == {b"": END, b"COMPLETE\n": OTHER, b"GET_FILE\ndir/b": INCOMPLETE, b"BOGUS\n": MALFORMED}[tail]
    assert consumed == len(data) - len(tail) and used == len(get_files_run(names[:answered]))
    # what the reference's loop over the decodable, answered names writes; and it parses back
    assert (run, n_answered) == reference_loop(idx, names[:answered])
    assert [n for n, _rows in parse_back(run)] == names[:answered]
    assert isinstance(run, bytes)


def test_host_route_bounds_the_run_and_continues(source):
    idx, _added = source
    names = [b"a.bin", b"dir/b.bin", b"dir/b.bin", b"dir/empty", b"z"]
    data = get_files_run(names)
    whole = idx.serve_get_file_requests(data)
    assert whole[4] == ALL and whole[2] == 5
    first = len(idx.serve_get_file_requests(get_files_run(names[:1]))[0])
    for bound in (len(whole[0]), len(whole[0]) - 1, first, first - 1, 1, len(whole[0]) // 2):
        got = idx.serve_get_file_requests(data, max_run_bytes=bound)
        assert got == respond(idx, data, bound), bound
        assert len(got[0]) <= bound
    assert idx.serve_get_file_requests(data, max_run_bytes=len(whole[0]))[4] == ALL
    assert idx.serve_get_file_requests(data, max_run_bytes=first - 1)[2:5] == (0, 0, FULL)
    # the continuation loop: every piece within the bound, together the one-call answer
    bound = max(len(idx.serve_get_file_requests(get_files_run([n]))[0]) for n in names)
    rest, pieces = data, []
    while True:
        run, _n, n_answered, used, why, _c, _s = idx.serve_get_file_requests(rest, max_run_bytes=bound)
        pieces.append(run)
        assert len(run) <= bound
        if why != FULL:
            break
        assert n_answered > 0
        rest = rest[used:]
    assert b"".join(pieces) == whole[0] and len(pieces) > 2 and why == ALL


def test_host_route_continues_a_run_in_two_pieces(source):
    """A request run that arrives in two buffers: the second call gets the
    unconsumed tail and the new bytes."""
    idx, _added = source
    names = [b"a.bin", b"dir/empty", b"x/FILE_END", b"z"]
    data = get_files_run(names)
    whole = idx.serve_get_file_requests(data)[0]
    for cut in (1, 9, 10, 15, 16, 20, len(data) - 1):
        a = idx.serve_get_file_requests(data[:cut])
        assert a[6] in (INCOMPLETE, END) and a[4] == ALL and a[3] == a[5]  # all parsed requests answered
        b = idx.serve_get_file_requests(data[a[5]:cut] + data[cut:])
        assert a[0] + b[0] == whole and a[1] + b[1] == len(names) and b[6] == END, cut
