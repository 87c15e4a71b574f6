"""CPU: the GetFiles framing rules (syncfast_amd/csrc/sf_wire_files.hpp) --
files_message, classify_files, the sink's order and the serial
parse_files_run, which defines sf_receive_files_device and is its fallback --
alone, in tests/native/wire_files.cpp: a stand-alone program with its own
main, built with ASan + UBSan and run directly (nothing is loaded into Python
under a sanitizer).  Every expected value is files_expect's, from wire.Parser
and the sink's rule.  And the argument checks of the entry point and its
stats hook, which need no device."""
import ctypes
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import syncfast_amd
from files_expect import (END, FILE_END, INCOMPLETE, MALFORMED, OTHER, UNEXPECTED, block, candidates, expected,
                          needs_fallback, start)
from syncfast_amd import _lib, wire

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
ENV = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")

D1, D2 = bytes(range(1, 21)), b"\n\n\n\n\n" + b"B" * 15
BIG = 1 << 40


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wire_files")
    probe = tmp / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode or \
            subprocess.run([str(tmp / "probe")], capture_output=True).returncode:
        pytest.skip("g++ -fsanitize=address,undefined unavailable")
    exe = tmp / "wire_files"
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "wire_files.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def _run(program, path, cases):
    """The program over ``cases`` = [(stream, open, base)] -> per case the
    parsed output lines."""
    with open(path, "wb") as f:
        for stream, is_open, base in cases:
            f.write(struct.pack("<IQQ", int(is_open), base, len(stream)) + stream)
    r = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok %d" % len(cases)
    out = []
    for ln in lines[:-1]:
        if ln.startswith("R "):
            out.append([])
        out[-1].append(ln.split(" "))
    assert len(out) == len(cases)
    return out


def _hold(lines, stream, is_open, base, what):
    """One record of the program's output against the model."""
    e = expected(stream, is_open, base)
    head = [int(v) for v in lines[0][1:]]
    assert head == [len(e.sizes), len(e.name_at), e.messages, e.consumed, e.stop, int(e.open), e.end_offset, 0], what
    rows = {k: [ln[1:] for ln in lines if ln[0] == k] for k in "BFLC"}
    assert rows["B"] == [[d.hex(), str(s), str(o), str(f)]
                         for d, s, o, f in zip(e.digests, e.sizes, e.offsets, e.block_file)], what
    assert rows["F"] == [[str(a), str(n), str(f), str(z)]
                         for a, n, f, z in zip(e.name_at, e.name_len, e.first, e.file_size)], what
    assert rows["L"] == [[str(e.first[-1])]], what
    assert rows["C"] == [[str(p), str(n), str(k)] for p, n, k in candidates(stream)], what
    return e


def table():
    """[(name, stream, open, base)]: the fixed cases."""
    one = start(b"dir/a") + block(D1, 5) + block(D2, 0) + FILE_END
    two = one + start(b"b") + FILE_END + start(b"") + block(D1, 4096) + FILE_END
    msgs = {"start": start(b"n" * 100), "block": block(D2, b"+0000000012345"), "end": FILE_END}
    assert [len(m) for m in msgs.values()] == [112, 47, 9]
    c = [("nothing", b"", False, 0), ("nothing_open", b"", True, 7), ("one", one, False, 0), ("two", two, False, 9),
         ("empty_file", start(b"e") + FILE_END, False, 0), ("carried", block(D1, 3) + FILE_END + two, True, BIG),
         ("carried_end_only", FILE_END, True, BIG), ("carried_open_after", block(D1, 3) + block(D2, 4), True, BIG),
         ("open_after", one + start(b"z") + block(D1, 1), False, 0)]
    # every stop class at the end of a valid prefix and at byte 0
    for other in (b"FILE_ENTRY\nx", b"END_FILES\n", b"GET_FILE\n", b"GET_BLOCK\n", b"BLOCK_DATA\n", b"COMPLETE\nrest"):
        c += [("other", one + other, False, 0), ("other_first", other, True, 1), ("other_in_file", one[:-9] + other, False, 0)]
    for bad in (b"BOGUS\n", b"X" * 20, b"\n" + one, b"file_end\n", b"FILE_BLOCK\n" + D1 + b"x5\n",
                b"FILE_BLOCK\n" + D1 + b"\n\n", b"FILE_BLOCK\n" + D1 + b"\n1a\n", b"FILE_BLOCK\n" + D1 + b"\n" + b"1" * 16 + b"\n"):
        c += [("malformed", one + start(b"m") + bad, False, 0), ("malformed_first", bad, True, 0)]
    c.append(("x19", one + b"X" * 19, False, 0))
    # every proper prefix of each kind, where the state takes that kind
    for kind, m in msgs.items():
        lead = b"" if kind == "start" else start(b"lead")
        c += [("prefix_" + kind, one + lead + m[:t], False, 0) for t in range(1, len(m))]
        c += [("whole_" + kind, one + lead + m, False, 0)]
    # names of 0, 1, 99 and 100 bytes; 101 name bytes; exactly 100 available and no newline
    c += [("name%d" % n, start(b"q" * n) + block(D1, n) + FILE_END, False, 0) for n in (0, 1, 99, 100)]
    c += [("name101", b"FILE_START\n" + b"q" * 101 + b"\n", False, 0), ("name100_open", b"FILE_START\n" + b"q" * 100, False, 0),
          ("name99_open", b"FILE_START\n" + b"q" * 99, False, 0), ("name150_open", one + b"FILE_START\n" + b"q" * 150, False, 0)]
    # all nine pairs (four of them bad) and every first message in both states
    for ka, a in msgs.items():
        for kb, b in msgs.items():
            lead = {"start": one, "block": one + start(b"p"), "end": one + start(b"p")}[ka]
            c.append(("pair_%s_%s" % (ka, kb), lead + a + b + b"COMPLETE\n", False, 0))
        c += [("first_%s_closed" % ka, a + one, False, 5), ("first_%s_open" % ka, a + one, True, 5)]
    # names that end in a tag
    for tail in (b"FILE_END", b"FILE_START", b"FILE_BLOCK"):
        c.append(("name_" + tail.decode(), start(b"x/" + tail) + block(D1, 7) + FILE_END + start(b"y") + FILE_END, False, 0))
    c.append(("digest_tag", start(b"t") + block(b"FILE_END\n" + b"z" * 11, 1) + FILE_END, False, 0))
    return c


def test_fixed_table_under_asan_ubsan(program, tmp_path):
    """Every stop class, every proper prefix of each kind, the name lengths
    and the filename quirk, all pairs and first messages, an empty file, names
    that end in a tag: parse_files_run from heap copies of the exact length
    (also with capacities one short and none) and files_message at every
    position, against the model."""
    cases = table()
    assert len(cases) > 200
    stops, seen = set(), {}
    for lines, (name, stream, is_open, base) in zip(_run(program, tmp_path / "table.bin", [c[1:] for c in cases]), cases):
        e = _hold(lines, stream, is_open, base, name)
        stops.add(e.stop)
        seen.setdefault(name, []).append(e)
    assert stops == {END, INCOMPLETE, OTHER, MALFORMED, UNEXPECTED}
    # the table shows what it is meant to show
    assert all(e.stop == OTHER for k in ("other", "other_first", "other_in_file") for e in seen[k])
    assert all(e.stop == MALFORMED for k in ("malformed", "malformed_first", "name101", "name100_open", "name150_open")
               for e in seen[k])
    assert seen["name99_open"][0].stop == seen["x19"][0].stop == INCOMPLETE
    assert [e.stop for e in seen["prefix_start"]] == [INCOMPLETE] * 110 + [MALFORMED]  # 100 name bytes and no newline
    assert all(e.stop == INCOMPLETE for k in ("prefix_block", "prefix_end") for e in seen[k])
    bad = {k for k, v in seen.items() if k.startswith("pair_") and v[0].stop == UNEXPECTED}
    assert bad == {"pair_start_start", "pair_block_start", "pair_end_block", "pair_end_end"}
    assert all(seen[k][0].stop == OTHER for k in seen if k.startswith("pair_") and k not in bad)
    first_bad = {k for k, v in seen.items() if k.startswith("first_") and (v[0].stop, v[0].consumed) == (UNEXPECTED, 0)}
    assert first_bad == {"first_start_open", "first_block_closed", "first_end_closed"}
    assert seen["empty_file"][0].first == [0, 0] and seen["empty_file"][0].file_size == [0]
    assert seen["carried"][0].offsets[0] == BIG and seen["carried"][0].name_at[0] == (1 << 64) - 1
    streams = {c[0]: c[1] for c in cases}
    for k in ("name_FILE_END", "name_FILE_START", "digest_tag"):  # honest names, and a digest, that forge a start
        assert needs_fallback(streams[k]), k
    assert not needs_fallback(streams["name_FILE_BLOCK"]) and not needs_fallback(streams["two"])


def hostile(rng: random.Random) -> bytes:
    """A stream built from the protocol's own bytes: mostly the sink's order,
    with tags inside names and digests, wrong orders, other commands, broken
    fields and cuts."""
    tags = (b"FILE_END\n", b"FILE_START\n", b"FILE_BLOCK\n", b"FILE_END", b"FILE_START")

    def digest():
        d = bytearray(rng.randbytes(20))
        if rng.random() < 0.3:
            t = rng.choice(tags)
            at = rng.randrange(0, 21 - len(t))
            d[at:at + len(t)] = t
        return bytes(d)

    def name():
        n = bytes(rng.choice(b"abc/._-F") for _ in range(rng.choice((0, 1, 3, 8, 40, 99, 100))))
        if rng.random() < 0.3:
            n = n[:80] + rng.choice(tags).rstrip(b"\n")
        return n

    out = b""
    for _ in range(rng.randrange(1, 7)):
        out += start(name())
        for _ in range(rng.randrange(0, 5)):
            out += block(digest(), rng.choice((0, 1, 4096, 65536, b"+7", b"007")))
        r = rng.random()
        if r < 0.70:
            out += FILE_END
        elif r < 0.76:
            out += rng.choice((FILE_END + FILE_END, start(b"again"), b""))  # a wrong order
        elif r < 0.82:
            out += rng.choice((b"COMPLETE\n", b"GET_BLOCK\n" + bytes(20) + b"\n", b"END_FILES\n"))
            break
        elif r < 0.88:
            out += rng.choice((b"BOGUS\n", b"FILE_BLOCK\n" + bytes(20) + b"\n1x\n", b"FILE_START\n" + b"n" * 101 + b"\n"))
            break
        else:
            out = out[:len(out) - rng.randrange(1, 40)]
            break
    return out


def test_serial_parse_equals_the_model_on_hostile_streams(program, tmp_path):
    rng = random.Random(11)
    cases = []
    for k in range(200):
        stream = hostile(rng)
        is_open = k % 4 == 3
        if is_open:  # the tail of a file first
            stream = block(D1, 9) * (k % 3) + FILE_END + stream
        cases.append((stream, is_open, BIG if is_open else 0))
    stops, fallbacks = set(), 0
    for lines, (stream, is_open, base) in zip(_run(program, tmp_path / "hostile.bin", cases), cases):
        stops.add(_hold(lines, stream, is_open, base, stream).stop)
        fallbacks += needs_fallback(stream, is_open)
    assert stops == {END, INCOMPLETE, OTHER, MALFORMED, UNEXPECTED}
    assert 10 <= fallbacks < len(cases)


def _call(L, wire_ptr, n_bytes, is_open, base, outs, results, set_=None):
    return L.sf_receive_files_device(set_, wire_ptr, n_bytes, is_open, base, *outs[:5], 0, *outs[5:], 0, *results, None)


def test_receive_files_checks_arguments_before_any_device_call():
    L = syncfast_amd.lib()
    assert wire.SF_WIRE_UNEXPECTED == _lib.SF_WIRE_UNEXPECTED == UNEXPECTED
    vals = [ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_int(7), ctypes.c_int(7), ctypes.c_uint64(7)]
    refs = [ctypes.byref(v) for v in vals]
    nothing = [None] * 9
    # no bytes: nothing launched, no device needed, the state handed back
    for is_open, base in ((0, 5), (1, BIG), (2, 0)):
        assert _call(L, None, 0, is_open, base, nothing, refs) == 0
        assert [v.value for v in vals] == [0, int(is_open != 0), 0, END, int(is_open != 0), base]
    buf = np.frombuffer(start(b"a") + block(D1, 5) + FILE_END, np.uint8)
    p, n = buf.ctypes.data, buf.size
    assert _call(L, None, n, 0, 0, nothing, refs) == _lib.SF_EINVAL  # bytes announced without a buffer
    for k in range(6):  # a missing result pointer
        assert _call(L, p, n, 0, 0, nothing, refs[:k] + [None] + refs[k + 1:]) == _lib.SF_EINVAL
    assert _call(L, p, (1 << 35) + 1, 0, 0, nothing, refs) == _lib.SF_EINVAL  # too long a buffer
    # outputs off their grid: digests, sizes, offsets, rows, block_file | name_at, name_len, first, file_size
    for j, align in enumerate((4, 4, 8, 8, 4, 8, 4, 8, 8)):
        for off in range(1, align):
            outs = list(nothing)
            outs[j] = 0x10000 + off
            assert _call(L, p, n, 0, 0, outs, refs) == _lib.SF_EINVAL, (j, off)
    assert _call(L, p, n, 0, 0, nothing, refs, set_=0x1000) == _lib.SF_EINVAL  # a set and no rows
    assert [v.value for v in vals[:4]] == [0, 0, 0, END]
    assert L.sf_test_recv_files_stats(None) == _lib.SF_EINVAL
    out = (ctypes.c_uint64 * 4)(9, 9, 9, 9)
    assert L.sf_test_recv_files_stats(out) == 0 and list(out) == [0, 0, 0, 0]  # reset by the calls above
    assert wire.recv_files_stats() == (0, 0, 0, 0)
