"""CPU: the host FILE_BLOCK parser (syncfast_amd/csrc/sf_wire_parse.hpp) -- the
fallback of sf_wire_parse_blocks_device and the rules its kernels share --
alone, in tests/native/wire_parse.cpp: a stand-alone program with its own
main, built with ASan + UBSan and run directly (nothing is loaded into Python
under a sanitizer).  And the argument checks of the three receive entry
points, which need no device."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import syncfast_amd
from recv_expect import END, expected, message
from syncfast_amd import _lib, host

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
ENV = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wire_parse")
    probe = tmp / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode or \
            subprocess.run([str(tmp / "probe")], capture_output=True).returncode:
        pytest.skip("g++ -fsanitize=address,undefined unavailable")
    exe = tmp / "wire_parse"
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "wire_parse.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def test_host_parser_table_under_asan_ubsan(program):
    """parse_run, classify and block_message over the program's fixed table:
    every stop class, every proper prefix of a message, the size-field forms,
    digests full of newlines, digits and tags, the forged-start recipe; each
    input parsed from a heap copy of its exact length, also in the query form
    and with a capacity one short."""
    r = subprocess.run([program], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and not r.stderr, (r.stdout[-2000:], r.stderr[-4000:])


def _random_run(rng):
    """Messages whose digests are built from the protocol's own bytes, cut or
    followed by something else: the inputs most likely to split the parsers."""
    pieces = [b"FILE_BLOCK\n", b"\n", b"FILE_END\n", b"0", b"12", b"+", b"\n7\n", bytes(3), b"\xaa" * 5, b"FILE_"]
    run = b""
    for _ in range(rng.randrange(0, 6)):
        d = b""
        while len(d) < 20:
            d += rng.choice(pieces)
        size = rng.choice([0, 7, 99, 1234, 4294967295, 4294967296, 10 ** 14, b"+5", b"007", b"", b"1a", b"1" * 16])
        run += message(d[:20], size)
    run += rng.choice([b"", b"FILE_END\n", b"FILE_START\nab", b"XYZ\n", b"FILE_BLOCK\n" + bytes(20), b"Z" * 25])
    return run[:rng.randrange(0, len(run) + 1)] if rng.random() < 0.5 else run


def test_host_parser_equals_wire_parser_on_random_runs(program, tmp_path):
    rng = random.Random(20)
    path = tmp_path / "run.bin"
    classes = set()
    for _ in range(150):
        run = _random_run(rng)
        path.write_bytes(run)
        r = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=60, env=ENV)
        assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
        lines = r.stdout.split("\n")
        digests, sizes, consumed, stop = expected(run)
        count, got_consumed, got_stop, too_large = (int(v) for v in lines[0].split())
        assert (count, got_consumed, got_stop) == (len(digests), consumed, stop), run
        assert too_large == int(any(s > 0xFFFFFFFF for s in sizes)), run
        assert [ln.split()[0] for ln in lines[1:1 + count]] == [d.hex() for d in digests], run
        assert [int(ln.split()[1]) for ln in lines[1:1 + count]] == [s & 0xFFFFFFFF for s in sizes], run
        classes.add(stop)
    assert classes == {0, 1, 2, 3}


def _outs():
    return ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_int(7), ctypes.c_uint64(7)


def test_receive_entry_points_check_arguments_before_any_device_call():
    L = syncfast_amd.lib()
    n, consumed, stop, end = _outs()
    refs = (ctypes.byref(n), ctypes.byref(consumed), ctypes.byref(stop))
    wire = np.frombuffer(message(bytes(20), 1), np.uint8)
    # an empty run: no messages, the offset stays at the base, nothing launched
    assert L.sf_wire_parse_blocks_device(None, 0, None, None, 0, *refs, None) == 0
    assert (n.value, consumed.value, stop.value) == (0, 0, END)
    assert L.sf_receive_blocks_device(None, None, 0, 1 << 40, None, None, None, None, 0, *refs, ctypes.byref(end),
                                      None) == 0
    assert (n.value, end.value) == (0, 1 << 40)
    assert L.sf_receive_blocks_buffer(None, None, 0, 5, None, None, 0, *refs, ctypes.byref(end)) == 0
    assert (n.value, end.value) == (0, 5)
    # bytes announced without a buffer, a missing result pointer, a digest table off the dword grid, too long a run
    assert L.sf_wire_parse_blocks_device(None, 34, None, None, 0, *refs, None) == _lib.SF_EINVAL
    assert L.sf_wire_parse_blocks_device(wire.ctypes.data, 34, None, None, 0, None, refs[1], refs[2], None) == _lib.SF_EINVAL
    assert L.sf_wire_parse_blocks_device(wire.ctypes.data, 34, None, None, 0, refs[0], None, refs[2], None) == _lib.SF_EINVAL
    assert L.sf_wire_parse_blocks_device(wire.ctypes.data, 34, None, None, 0, refs[0], refs[1], None, None) == _lib.SF_EINVAL
    assert L.sf_wire_parse_blocks_device(wire.ctypes.data, 34, 0x1002, None, 1, *refs, None) == _lib.SF_EINVAL
    assert L.sf_wire_parse_blocks_device(wire.ctypes.data, (1 << 38) + 1, None, None, 0, *refs, None) == _lib.SF_EINVAL
    assert L.sf_receive_blocks_device(None, None, 34, 0, None, None, None, None, 0, *refs, ctypes.byref(end),
                                      None) == _lib.SF_EINVAL
    assert L.sf_receive_blocks_device(None, wire.ctypes.data, 34, 0, None, None, None, None, 0, *refs, None,
                                      None) == _lib.SF_EINVAL
    assert L.sf_receive_blocks_device(None, wire.ctypes.data, 34, 0, 0x1001, None, None, None, 1, *refs,
                                      ctypes.byref(end), None) == _lib.SF_EINVAL
    assert L.sf_receive_blocks_buffer(None, None, 34, 0, None, None, 0, *refs, ctypes.byref(end)) == _lib.SF_EINVAL
    assert L.sf_receive_blocks_buffer(None, wire.ctypes.data, 34, 0, None, None, 0, *refs, None) == _lib.SF_EINVAL
    assert L.sf_test_wire_parse_stats(None) == _lib.SF_EINVAL
    assert _lib.get_knob("SF_TEST_WIRE_PARSE_HOST") == 0


def test_receive_buffer_without_a_device():
    """From host bytes on a machine without a device: SF_ENODEV, nothing
    reported.  (With one: test_gpu_recv.py, the buffer route.)"""
    L = syncfast_amd.lib()
    nd = ctypes.c_int(0)
    if L.sf_device_count(ctypes.byref(nd)) == 0 and nd.value > 0:
        return
    run = b"".join(message(bytes([i]) * 20, i) for i in range(3)) + b"FILE_END\n"
    wire = np.frombuffer(run, np.uint8)
    n, consumed, stop, end = _outs()
    out = np.zeros(3, host.SIG_DTYPE)
    rc = L.sf_receive_blocks_buffer(None, wire.ctypes.data, wire.size, 0, out.ctypes.data_as(ctypes.POINTER(_lib.BlockSig)),
                                    None, 3, ctypes.byref(n), ctypes.byref(consumed), ctypes.byref(stop),
                                    ctypes.byref(end))
    assert rc == _lib.SF_ENODEV and n.value == 0
