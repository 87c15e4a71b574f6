"""CPU: a whole GetFiles answer, as far as no device is needed
(sf_wire_files_device; sf_send_files.hip).  The framing rules of
syncfast_amd/csrc/sf_wire_send_files.hpp alone, in tests/native/send_files.cpp:
a stand-alone program with its own main, built with ASan + UBSan and run
directly (nothing is loaded into Python under a sanitizer); the symbol and its
argument checks, which come before any device call; and
Index.serve_get_files(device=None) against the reference's per-name loop.
Expected bytes are wire.write_message's (send_files_expect.py)."""
import ctypes
import os
import random
import subprocess

import pytest

import syncfast_amd
from send_files_expect import (NO_FILE, csr, expected, first_bad_file, parse_back, random_files, reference_loop,
                                source_index, table)
from syncfast_amd import _lib, wire
from syncfast_amd.index import Index

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
ENV = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
EINVAL = _lib.SF_EINVAL


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("send_files")
    probe = tmp / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode or \
            subprocess.run([str(tmp / "probe")], capture_output=True).returncode:
        pytest.skip("g++ -fsanitize=address,undefined unavailable")
    exe = tmp / "send_files"
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "native", "send_files.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _run(program, *args):
    r = subprocess.run([program, *args], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def _case_text(digests, sizes, first, names, name_at):
    return (f"{len(first) - 1} {len(digests)}\n" + " ".join(map(str, first)) + "\n" + " ".join(map(str, name_at)) + "\n"
            + (names.hex() or "-") + "\n" + "".join(f"{s} {d.hex()}\n" for s, d in zip(sizes, digests)))


def _serial(program, tmp_path, cases):
    """The program's answer for each case: ("bad", F) or ("ok", total, run,
    starts, ends, blocks)."""
    path = tmp_path / "cases.txt"
    path.write_text("".join(_case_text(*c) for c in cases))
    out = []
    for line in _run(program, str(path)).strip("\n").split("\n"):
        if line.startswith("bad "):
            out.append(("bad", int(line.split()[1])))
            continue
        head, starts, ends, blocks = line.split("|")
        _ok, total, run = head.split()
        out.append(("ok", int(total), b"" if run == "-" else bytes.fromhex(run),
                    *([int(v) for v in part.split()] for part in (starts, ends, blocks))))
    assert len(out) == len(cases)
    return out


def test_rules_under_asan_ubsan(program):
    """The program's own checks: name_ok at 100 and 101 bytes and with a
    newline at the first, a middle and the last byte; the three writers in
    buffers of their exact length, read back by the receiving rules; the
    upper-bound search among empty files; file_ok reading no name it must
    not."""
    assert _run(program).strip() == "ok"


def test_the_serial_run_is_write_message_and_the_formulas_find_every_message(program, tmp_path):
    rng = random.Random(2024)
    cases = list(table().values()) + [random_files(rng) for _ in range(200)]
    assert max(len(c) for c in cases) >= 35 and max(len(r) for c in cases for _n, r in c) >= 60
    got = _serial(program, tmp_path, [csr(c) for c in cases])
    for files, g in zip(cases, got):
        want, starts, ends, blocks = expected(files)
        assert g == ("ok", len(want), want, starts, ends, blocks), files
        assert parse_back(want) == [(n, [(d, s) for d, s in rows]) for n, rows in files]
        assert len(wire.Parser().receive(want)) == len(blocks) + 2 * len(files)


def test_the_serial_rule_names_the_first_bad_file(program, tmp_path):
    rng = random.Random(7)
    good = csr([(b"a", [(rng.randbytes(20), 5)] * 2), (b"bb", []), (b"ccc", [(rng.randbytes(20), 7)]), (b"d", [])])
    digests, sizes, first, names, name_at = good

    def change(**kw):
        c = dict(first=list(first), names=names, name_at=list(name_at))
        for k, (i, v) in kw.items():
            c[k][i] = v
        return digests, sizes, c["first"], c["names"], c["name_at"]
    cases = {
        "first decreasing": (change(first=(2, 1)), 1),
        "first does not end at n_blocks": (change(first=(4, 4)), 3),
        "first[0] is not 0": (change(first=(0, 1)), 0),
        "name_at decreasing": (change(name_at=(2, 0)), 1),
        "name_at[0] is not 0": (change(name_at=(0, 1)), 0),
        "a name past the names": (change(name_at=(2, 50)), 1),
        "a newline": ((digests, sizes, first, b"abb\nccd", name_at), 2),
        "101 bytes": (csr([(b"a", []), (b"n" * 101, []), (b"n" * 100, [])]), 1),
        "two bad files": (csr([(b"a", []), (b"x\n", []), (b"n" * 101, [])]), 1),
    }
    got = _serial(program, tmp_path, [c for c, _bad in cases.values()])
    for (name, (c, bad)), g in zip(cases.items(), got):
        assert first_bad_file(c[2], c[3], c[4], len(c[0])) == bad, name  # the model agrees with the table
        assert g == ("bad", bad), name
    assert _serial(program, tmp_path, [good])[0][0] == "ok" and first_bad_file(first, names, name_at, 3) == NO_FILE


# ------------------------------------------------------------- the library

def _call(L, digests, sizes, n_blocks, first, names, name_at, n_files, run="ref", bad="ref"):
    h, b = ctypes.c_void_p(7), ctypes.c_uint64(7)
    rc = L.sf_wire_files_device(digests, sizes, n_blocks, first, names, name_at, n_files,
                                ctypes.byref(h) if run == "ref" else None, ctypes.byref(b) if bad == "ref" else None,
                                None)
    return rc, h.value, b.value


def test_symbol_and_python_names():
    assert "sf_wire_files_device" in _lib.EXPORTED and callable(syncfast_amd.lib().sf_wire_files_device)
    assert callable(wire.files_device) and issubclass(wire.FilesRun, wire.BlockDataRun)
    assert wire.FilesRun.receive is not wire.BlockDataRun.receive and callable(Index.serve_get_files)


def test_no_files_give_an_empty_run_without_a_device():
    L = syncfast_amd.lib()
    lists = (ctypes.c_uint64 * 4)()
    a = ctypes.addressof(lists)
    for args in ((None, None, 0, None, None, None, 0), (a, a, 0, a, a, a, 0)):
        rc, h, bad = _call(L, *args)
        assert (rc, bad) == (0, NO_FILE) and h
        p, nb, nm = ctypes.c_void_p(5), ctypes.c_uint64(5), ctypes.c_uint64(5)
        assert L.sf_wire_run_info(h, ctypes.byref(p), ctypes.byref(nb), ctypes.byref(nm)) == 0
        assert (p.value, nb.value, nm.value) == (None, 0, 0)
        assert L.sf_wire_run_read(h, 0, None, 0) == 0
        assert L.sf_wire_run_free(h, None) == 0


def test_arguments_are_checked_before_any_device_call():
    L = syncfast_amd.lib()
    lists = (ctypes.c_uint64 * 8)()
    a = ctypes.addressof(lists)  # 8-B aligned host memory that no failing call reads
    # no place for the handle or for the bad file, with and without files
    for args in ((a, a, 1, a, a, a, 1), (None, None, 0, None, None, None, 0)):
        assert _call(L, *args, run=None)[0] == EINVAL
        rc, h, _bad = _call(L, *args, bad=None)
        assert rc == EINVAL and h is None
    bad_args = [
        (a, a, 1, None, a, a, 1), (a, a, 1, a, a, None, 1),          # a CSR is missing
        (None, a, 1, a, a, a, 1), (a, None, 1, a, a, a, 1),          # blocks and no table, or no sizes
        (a + 2, a, 1, a, a, a, 1), (a + 1, a, 1, a, a, a, 1), (a, a + 2, 1, a, a, a, 1),   # off the dword grid
        (a, a, 1, a + 4, a, a, 1), (a, a, 1, a, a, a + 4, 1), (a, a, 1, a + 1, a, a, 1),   # off the 8-byte grid
        (a, a, 0, a + 4, a, a, 0),                                   # misaligned with nothing to read: still the caller's bug
        (a, a, (1 << 32) - 1, a, a, a, 1), (a, a, 0, a, a, a, (1 << 31) + 1), (a, a, 1 << 33, a, a, a, 1),
        (a, a, 1 << 63, a, a, a, 1 << 63),                           # a sum that wraps
        (a, a, 1, a, a, a, 0),                                       # blocks of no file
    ]
    for args in bad_args:
        assert _call(L, *args) == (EINVAL, None, NO_FILE), args


# ------------------------------------------------- Index.serve_get_files, host

def test_serve_get_files_is_thereference_loop():
    idx, added = source_index(random.Random(5))
    names = [b"dir/b.bin", b"dir/empty", b"a.bin", b"x/FILE_END", b"a.bin", b"z"]
    got, n = idx.serve_get_files(names)
    assert (got, n) == reference_loop(idx, names) and n == len(names)
    # the rows are those that were added, in list_file_blocks' order
    assert parse_back(got) == [(nm, [(h.bytes, s) for h, _o, s in idx.list_file_blocks(idx.get_file(nm.decode())[0])])
                               for nm in names]
    assert sorted(parse_back(got)[0][1]) == sorted((h.bytes, s) for h, _o, s in added["dir/b.bin"])
    assert got.count(added["a.bin"][1][0].bytes) >= 2 * 2 + 2  # the repeated digest, in every answer that holds it
    assert idx.serve_get_files([]) == (b"", 0)


def test_serve_get_files_stops_before_an_unknown_name():
    idx, _added = source_index(random.Random(6))
    names = [b"a.bin", b"dir/empty", b"nope", b"z"]
    got, n = idx.serve_get_files(names)
    assert n == 2 and (got, n) == reference_loop(idx, names) == (idx.serve_get_files(names[:2])[0], 2)
    assert idx.serve_get_files([b"nope"]) == (b"", 0)
    # a temporary file is not a file the source holds, under either of its names
    assert idx.get_temp_file("incoming.bin") is not None
    for name in (b"incoming.bin", b".syncfast_tmp_incoming.bin"):
        assert idx.serve_get_files([b"z", name, b"a.bin"])[1] == 1
    with pytest.raises(wire.ProtocolError):
        idx.serve_get_files([b"a.bin", b"\xff\xfe"])
