"""CPU: the BLOCK_DATA framing rules (syncfast_amd/csrc/sf_wire_data.hpp) --
data_message, classify_data, the serial parse_data_run and walk_candidates,
the exact chain the device parser falls back on -- alone, in
tests/native/wire_data.cpp: a stand-alone program with its own main, built
with ASan + UBSan and run directly (nothing is loaded into Python under a
sanitizer).  And the argument checks of the two receive_block_data entry
points and the stats hook, which need no device."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import syncfast_amd
from data_expect import END, candidates, dense_run, expected, hostile_run, message, needs_walk
from syncfast_amd import _lib, host

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
ENV = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wire_data")
    probe = tmp / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode or \
            subprocess.run([str(tmp / "probe")], capture_output=True).returncode:
        pytest.skip("g++ -fsanitize=address,undefined unavailable")
    exe = tmp / "wire_data"
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "wire_data.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def _run(program, *args):
    r = subprocess.run([program, *args], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_framing_rules_table_under_asan_ubsan(program):
    """The program's fixed table: every stop class, every proper prefix of a
    message with its need, the length-field forms (+5, 007, 15 and 16 digits,
    empty, 1a), a wrong end byte, a zero-length payload, nested and crossing
    payloads; each input parsed from a heap copy of its exact length, also in
    the query form, with a capacity one short, through walk_candidates and by
    data_message at every position."""
    assert _run(program).strip() == "ok"


def test_the_table_holds_what_wire_parser_gives(program):
    """Every expected value of that table is the reference parser's."""
    lines = _run(program, "--table").strip().split("\n")
    assert len(lines) > 80
    stops, prefixes_with_need = set(), 0
    for ln in lines:
        name, run_hex, count, consumed, stop, need, *pairs = ln.split(" ")
        run = b"" if run_hex == "-" else bytes.fromhex(run_hex)
        _digests, sizes, offsets, want_consumed, want_stop, want_need = expected(run)
        assert (int(count), int(consumed), int(stop), int(need)) == (len(sizes), want_consumed, want_stop, want_need), name
        assert pairs == ["%d:%d" % (o, s) for o, s in zip(offsets, sizes)], name
        stops.add(want_stop)
        prefixes_with_need += name == "prefix" and want_need > 0
    assert stops == {0, 1, 2, 3} and prefixes_with_need >= 10


def test_walk_and_serial_parse_equal_wire_parser_on_hostile_runs(program, tmp_path):
    """Random nested, crossing and hostile runs: parse_data_run, and
    walk_candidates over the candidates data_message finds at every position
    (the program fails if the two differ), against wire.Parser."""
    rng = random.Random(7)
    path = tmp_path / "run.bin"
    classes, walks, runs = set(), 0, 160
    for _ in range(runs):
        run = hostile_run(rng)
        path.write_bytes(run)
        lines = _run(program, str(path)).split("\n")
        digests, sizes, offsets, consumed, stop, need = expected(run)
        count, got_consumed, got_stop, got_need, too_large, walk_needed, _cand = (int(v) for v in lines[0].split())
        assert (count, got_consumed, got_stop, got_need) == (len(digests), consumed, stop, need), run
        assert too_large == 0
        assert [ln.split()[0] for ln in lines[1:1 + count]] == [d.hex() for d in digests], run
        assert [int(ln.split()[1]) for ln in lines[1:1 + count]] == sizes, run
        assert [int(ln.split()[2]) for ln in lines[1:1 + count]] == offsets, run
        assert walk_needed == int(needs_walk(run)), run
        classes.add(stop)
        walks += needs_walk(run)
    assert classes == {0, 1, 2, 3}
    assert walks * 4 >= runs, walks


def test_a_candidate_every_21_bytes(program, tmp_path):
    """More candidates than the n / 35 + 1 messages a run can hold: the walk
    passes over all but the first, as the parser reads one message."""
    run = dense_run(60)
    path = tmp_path / "dense.bin"
    path.write_bytes(run)
    count, consumed, stop, need, _large, walk_needed, cand = (int(v) for v in _run(program, str(path)).split("\n")[0].split())
    assert (count, consumed, stop, need, walk_needed) == (1, len(run), END, 0, 1)
    assert expected(run)[3:5] == (len(run), END) and len(expected(run)[0]) == 1
    assert cand == len(candidates(run)) > len(run) // 35 + 1


def _outs():
    return (ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_int(7), ctypes.c_uint64(7), ctypes.c_uint64(7))


def test_block_data_entry_points_check_arguments_before_any_device_call():
    L = syncfast_amd.lib()
    outs = _outs()
    n, consumed, stop, need, n_bad = outs
    refs = tuple(ctypes.byref(v) for v in outs)
    wire = np.frombuffer(message(b"hello"), np.uint8)
    # an empty run: no messages, nothing launched
    assert L.sf_receive_block_data_device(None, 0, None, None, None, None, 0, *refs, None) == 0
    assert (n.value, consumed.value, stop.value, need.value, n_bad.value) == (0, 0, END, 0, 0)
    for v in outs:
        v.value = 7
    assert L.sf_receive_block_data_buffer(None, 0, None, None, 0, *refs) == 0
    assert (n.value, consumed.value, stop.value, need.value, n_bad.value) == (0, 0, END, 0, 0)
    # bytes announced without a buffer, a missing result pointer, a digest table off the dword grid, too long a run
    assert L.sf_receive_block_data_device(None, 40, None, None, None, None, 0, *refs, None) == _lib.SF_EINVAL
    assert L.sf_receive_block_data_buffer(None, 40, None, None, 0, *refs) == _lib.SF_EINVAL
    for k in range(5):
        short = refs[:k] + (None,) + refs[k + 1:]
        assert L.sf_receive_block_data_device(wire.ctypes.data, 40, None, None, None, None, 0, *short,
                                              None) == _lib.SF_EINVAL
        assert L.sf_receive_block_data_buffer(wire.ctypes.data, 40, None, None, 0, *short) == _lib.SF_EINVAL
    assert L.sf_receive_block_data_device(wire.ctypes.data, 40, 0x1002, None, None, None, 1, *refs,
                                          None) == _lib.SF_EINVAL
    assert L.sf_receive_block_data_device(wire.ctypes.data, (1 << 38) + 1, None, None, None, None, 0, *refs,
                                          None) == _lib.SF_EINVAL
    assert L.sf_receive_block_data_buffer(wire.ctypes.data, (1 << 38) + 1, None, None, 0, *refs) == _lib.SF_EINVAL
    assert n.value == 0 and stop.value == END
    assert L.sf_test_block_data_stats(None) == _lib.SF_EINVAL
    out = (ctypes.c_uint64 * 4)(9, 9, 9, 9)
    assert L.sf_test_block_data_stats(out) == 0 and list(out) == [0, 0, 0, 0]  # reset by the calls above
    assert _lib.get_knob("SF_TEST_BLOCK_DATA_WALK") == 0


def test_block_data_buffer_without_a_device():
    """From host bytes on a machine without a device: SF_ENODEV, nothing
    reported.  (With one: test_gpu_recv_data.py, the buffer route.)"""
    L = syncfast_amd.lib()
    nd = ctypes.c_int(0)
    if L.sf_device_count(ctypes.byref(nd)) == 0 and nd.value > 0:
        return
    run = b"".join(message(bytes([i]) * i) for i in range(3)) + b"COMPLETE\n"
    wire = np.frombuffer(run, np.uint8)
    outs = _outs()
    out = np.zeros(3, host.SIG_DTYPE)
    ok = np.zeros(3, np.uint8)
    rc = L.sf_receive_block_data_buffer(wire.ctypes.data, wire.size, out.ctypes.data_as(ctypes.POINTER(_lib.BlockSig)),
                                        ok.ctypes.data, 3, *(ctypes.byref(v) for v in outs))
    assert rc == _lib.SF_ENODEV and outs[0].value == 0
    with pytest.raises(_lib.SfError) as e:
        host.receive_block_data(run)
    assert e.value.code == _lib.SF_ENODEV
