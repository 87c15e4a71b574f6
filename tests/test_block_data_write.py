"""CPU: the sending side's framing rules (syncfast_amd/csrc/sf_wire_data.hpp)
-- the BLOCK_DATA message length and header writer, and the serial definition
of a GET_BLOCK run -- alone, in tests/native/block_data_write.cpp: a
stand-alone program with its own main, built with ASan + UBSan and run
directly (nothing is loaded into Python under a sanitizer).  Every expected
value is wire.write_message's or wire.Parser's.  And the argument checks of
the run entry points, which need no device."""
import ctypes
import os
import random
import subprocess

import pytest

import syncfast_amd
from send_expect import END, INCOMPLETE, MALFORMED, OTHER, OTHERS, expected_requests, hostile_requests
from syncfast_amd import _lib, wire

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
ENV = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("block_data_write")
    probe = tmp / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode or \
            subprocess.run([str(tmp / "probe")], capture_output=True).returncode:
        pytest.skip("g++ -fsanitize=address,undefined unavailable")
    exe = tmp / "block_data_write"
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "native", "block_data_write.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _run(program, *args):
    r = subprocess.run([program, *args], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_rules_under_asan_ubsan(program):
    """The program's own checks: headers in buffers of their exact length, no
    payload byte written, what is written reads back through data_message, the
    one-lane slot test agrees with the serial rule, the stop decided from 128
    bytes equals the one decided from the whole run."""
    assert _run(program).strip() == "ok"


def test_the_writer_writes_what_write_message_writes(program):
    sizes = [0] + [v for e in range(1, 10) for v in (10 ** e - 1, 10 ** e)] + [2 ** 32 - 1]
    lines = _run(program, "--writer").strip().split("\n")
    assert [int(ln.split()[0]) for ln in lines] == sizes
    for ln in lines:
        size, length, head = ln.split()
        size = int(size)
        digest = bytearray((size * 31 + k * 13 + 1) & 0xFF for k in range(20))
        digest[5:7] = b"\nB"
        # write_message's header is the message of an empty payload up to its size field, with this size in it
        want = wire.write_message("BlockData", bytes(digest), b"")[:32] + b"%d\n" % size
        assert bytes.fromhex(head) == want, size
        assert int(length) == len(want) + size + 1 == 34 + len(str(size)) + size
        if size <= 100000:
            assert len(wire.write_message("BlockData", bytes(digest), bytes(size))) == int(length)


def test_the_get_block_table_holds_what_wire_parser_gives(program):
    lines = _run(program, "--table").strip().split("\n")
    stops, prefixes, others = set(), 0, set()
    for ln in lines:
        name, run_hex, count, consumed, stop = ln.split(" ")
        run = b"" if run_hex == "-" else bytes.fromhex(run_hex)
        digests, want_consumed, want_stop = expected_requests(run)
        assert (int(count), int(consumed), int(stop)) == (len(digests), want_consumed, want_stop), (name, run)
        stops.add(want_stop)
        if name == "prefix":
            prefixes += 1
            assert want_stop == INCOMPLETE and len(digests) == 2
        if name == "other":
            assert want_stop == OTHER and len(digests) == 3
            others.add(run[want_consumed:-1])
        if name.startswith("end-byte"):
            assert want_stop == MALFORMED
    assert stops == {END, INCOMPLETE, OTHER, MALFORMED}
    assert prefixes == 30 and others == set(OTHERS)


def test_hostile_get_block_runs_equal_wire_parser(program, tmp_path):
    rng = random.Random(11)
    path = tmp_path / "run.bin"
    classes, spoilt = set(), 0
    for _ in range(100):
        run = hostile_requests(rng)
        path.write_bytes(run)
        digests, consumed, stop = expected_requests(run)
        assert [int(v) for v in _run(program, str(path)).split()] == [len(digests), consumed, stop], run
        classes.add(stop)
        spoilt += consumed + 31 < len(run)
    assert classes == {END, INCOMPLETE, OTHER, MALFORMED} and spoilt >= 5


def _run_outs():
    return ctypes.c_void_p(7), ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_int(7)


def _empty_run_works(L, h):
    p, nb, nm = ctypes.c_void_p(5), ctypes.c_uint64(5), ctypes.c_uint64(5)
    assert L.sf_wire_run_info(h, ctypes.byref(p), ctypes.byref(nb), ctypes.byref(nm)) == 0
    assert (p.value, nb.value, nm.value) == (None, 0, 0)
    assert L.sf_wire_run_info(h, None, None, None) == 0
    buf = ctypes.create_string_buffer(4)
    assert L.sf_wire_run_read(h, 0, buf, 0) == 0 and L.sf_wire_run_read(h, 0, None, 0) == 0
    assert L.sf_wire_run_read(h, 0, buf, 1) == _lib.SF_ERANGE and L.sf_wire_run_read(h, 1, buf, 0) == _lib.SF_ERANGE
    r, w = os.pipe()
    try:
        nw = ctypes.c_uint64(9)
        assert L.sf_wire_run_to_fd(h, w, ctypes.byref(nw)) == 0 and nw.value == 0
        assert L.sf_wire_run_to_fd(h, -1, ctypes.byref(nw)) == _lib.SF_EINVAL
    finally:
        os.close(r)
        os.close(w)
    assert L.sf_wire_run_free(h, None) == 0


def test_run_entry_points_check_arguments_before_any_device_call():
    L = syncfast_amd.lib()
    h = ctypes.c_void_p(7)
    lists = (ctypes.c_uint64 * 4)()
    a = ctypes.addressof(lists)
    # no jobs: an empty run, whatever the other arguments hold, and it needs no device
    assert L.sf_wire_block_data_device(None, 0, None, None, None, 0, ctypes.byref(h), None) == 0 and h.value
    _empty_run_works(L, h)
    # no place for the handle; too many jobs; a missing buffer, table or list; a list off its element's grid
    assert L.sf_wire_block_data_device(a, 8, a, a, a, 1, None, None) == _lib.SF_EINVAL
    assert L.sf_wire_block_data_device(None, 0, None, None, None, 0, None, None) == _lib.SF_EINVAL
    for args in ((a, 8, a, a, a, (1 << 32) + 1), (None, 8, a, a, a, 1), (a, 8, None, a, a, 1), (a, 8, a, None, a, 1),
                 (a, 8, a, a, None, 1), (a, 8, a + 2, a, a, 1), (a, 8, a, a + 4, a, 1), (a, 8, a, a, a + 2, 1)):
        h.value = 7
        assert L.sf_wire_block_data_device(*args, ctypes.byref(h), None) == _lib.SF_EINVAL, args
        assert h.value is None
    assert L.sf_wire_run_info(None, None, None, None) == _lib.SF_EINVAL
    assert L.sf_wire_run_read(None, 0, None, 0) == _lib.SF_EINVAL
    assert L.sf_wire_run_to_fd(None, 1, None) == _lib.SF_EINVAL
    assert L.sf_wire_run_free(None, None) == 0


def test_serve_checks_arguments_before_any_device_call():
    L = syncfast_amd.lib()
    req = (ctypes.c_uint8 * 64)()
    a = ctypes.addressof(req)
    h, nreq, nans, consumed, stop = outs = _run_outs()
    refs = tuple(ctypes.byref(v) for v in outs)
    # no bytes: an empty run and SF_WIRE_END, without a set and without a device
    assert L.sf_serve_get_blocks_device(None, None, None, None, 0, None, 0, *refs, None) == 0
    assert (nreq.value, nans.value, consumed.value, stop.value) == (0, 0, 0, END) and h.value
    _empty_run_works(L, h)
    fake_set = a  # never read: every call below fails before the set is used
    for k in range(5):
        short = refs[:k] + (None,) + refs[k + 1:]
        assert L.sf_serve_get_blocks_device(fake_set, a, a, a, 8, a, 31, *short, None) == _lib.SF_EINVAL
        assert L.sf_serve_get_blocks_device(None, None, None, None, 0, None, 0, *short, None) == _lib.SF_EINVAL
    for v in outs:
        v.value = 7
    assert L.sf_serve_get_blocks_device(fake_set, a, a, a, 8, a, (1 << 38) + 1, *refs, None) == _lib.SF_EINVAL
    assert L.sf_serve_get_blocks_device(fake_set, a, a, a, 8, None, 31, *refs, None) == _lib.SF_EINVAL
    assert L.sf_serve_get_blocks_device(None, a, a, a, 8, a, 31, *refs, None) == _lib.SF_EINVAL
    assert h.value is None and (nreq.value, nans.value, consumed.value, stop.value) == (0, 0, 0, END)


def test_python_names():
    assert {"sf_wire_block_data_device", "sf_serve_get_blocks_device", "sf_wire_run_info", "sf_wire_run_read",
            "sf_wire_run_to_fd", "sf_wire_run_free"} <= set(_lib.EXPORTED)
    assert callable(wire.block_data_device) and hasattr(wire.BlockDataRun, "to_fd")
