"""CPU: the destination's missing blocks on the device, as far as no device is
needed (sf_wire_get_blocks_device, sf_place_block_data_device; sf_want.hip).
The two symbols and their argument checks, which come before any device call;
the per-row rules of syncfast_amd/csrc/sf_want_plan.hpp alone, in
tests/native/want_plan.cpp: a stand-alone program with its own main, built
with ASan + UBSan and run directly (nothing is loaded into Python under a
sanitizer); and Index.missing_rows against list_missing_blocks.  Expected
request bytes are wire.write_message's."""
import ctypes
import os
import random
import subprocess
from pathlib import PurePath

import pytest

import syncfast_amd
from syncfast_amd import _lib, wire
from syncfast_amd.digest import HashDigest
from syncfast_amd.index import Index
from syncfast_amd.timestamp import DateTimeUtc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
ENV = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
EINVAL = _lib.SF_EINVAL


def test_symbols_and_python_names():
    L = syncfast_amd.lib()
    assert {"sf_wire_get_blocks_device", "sf_place_block_data_device"} <= set(_lib.EXPORTED)
    assert callable(L.sf_wire_get_blocks_device) and callable(L.sf_place_block_data_device)
    from syncfast_amd import device
    from syncfast_amd.assemble import FileImages
    assert callable(device.get_block_requests) and callable(device.place_block_data)
    assert callable(FileImages.base) and callable(FileImages.apply_jobs)
    assert callable(Index.missing_rows) and callable(Index.get_block_requests) and callable(Index.place_block_data)


# ------------------------------------------------ sf_wire_get_blocks_device

def test_no_rows_give_an_empty_run_without_a_device():
    L = syncfast_amd.lib()
    for distinct in (0, 1):
        h, n = ctypes.c_void_p(7), ctypes.c_uint64(7)
        assert L.sf_wire_get_blocks_device(None, None, None, 0, distinct, ctypes.byref(h), ctypes.byref(n), None) == 0
        assert h.value and n.value == 0
        p, nb, nm = ctypes.c_void_p(5), ctypes.c_uint64(5), ctypes.c_uint64(5)
        assert L.sf_wire_run_info(h, ctypes.byref(p), ctypes.byref(nb), ctypes.byref(nm)) == 0
        assert (p.value, nb.value, nm.value) == (None, 0, 0)
        assert L.sf_wire_run_read(h, 0, None, 0) == 0
        r, w = os.pipe()
        try:
            nw = ctypes.c_uint64(9)
            assert L.sf_wire_run_to_fd(h, w, ctypes.byref(nw)) == 0 and nw.value == 0
        finally:
            os.close(r)
            os.close(w)
        assert L.sf_wire_run_free(h, None) == 0
    # the count is optional
    h = ctypes.c_void_p(7)
    assert L.sf_wire_get_blocks_device(None, None, None, 0, 0, ctypes.byref(h), None, None) == 0 and h.value
    assert L.sf_wire_run_free(h, None) == 0


def test_get_blocks_checks_arguments_before_any_device_call():
    L = syncfast_amd.lib()
    buf = (ctypes.c_uint64 * 8)()
    a = ctypes.addressof(buf)
    n = ctypes.c_uint64(7)
    # no place for the handle, with and without rows
    assert L.sf_wire_get_blocks_device(a, None, None, 1, 0, None, ctypes.byref(n), None) == EINVAL
    assert L.sf_wire_get_blocks_device(None, None, None, 0, 0, None, ctypes.byref(n), None) == EINVAL
    # too many rows; no table; a table off the dword grid; a row list off its own
    for args in ((a, None, None, (1 << 31) + 1), (None, None, None, 1), (a + 1, None, None, 1), (a + 2, None, None, 1),
                 (a, a + 4, None, 1), (a, a + 1, None, 1), (None, a + 4, None, 0)):
        for distinct in (0, 1):
            h = ctypes.c_void_p(7)
            n.value = 7
            assert L.sf_wire_get_blocks_device(*args, distinct, ctypes.byref(h), ctypes.byref(n), None) == EINVAL, args
            assert h.value is None and n.value == 0


# ------------------------------------------------ sf_place_block_data_device

def _place_args(a, **change):
    """A call with one row and one message whose every list is `a` (8-B
    aligned host memory that no failing call reads), then the changes."""
    args = dict(row_digests=a, row_sizes=a, row_dst=a, row_present=a, n_rows=1, msg_digests=a, msg_sizes=a,
                msg_offsets=a, msg_ok=None, n_msgs=1, src=a, dst=a, sizes=a, job_rows=a, job_msgs=a, cap=1, uses=a)
    args.update(change)
    return tuple(args.values())


def test_place_checks_arguments_before_any_device_call():
    L = syncfast_amd.lib()
    buf = (ctypes.c_uint64 * 8)()
    a = ctypes.addressof(buf)
    outs = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    refs = tuple(ctypes.byref(v) for v in outs)
    # a result pointer is missing
    for k in range(3):
        short = refs[:k] + (None,) + refs[k + 1:]
        assert L.sf_place_block_data_device(*_place_args(a), *short, None) == EINVAL
        assert L.sf_place_block_data_device(*_place_args(None, n_rows=0, n_msgs=0, cap=0), *short, None) == EINVAL
    bad = [dict(n_rows=(1 << 31) + 1), dict(n_msgs=(1 << 31) + 1)]
    bad += [{name: None} for name in ("row_digests", "row_sizes", "row_dst", "row_present", "msg_digests", "msg_sizes",
                                      "msg_offsets")]
    bad += [{name: a + 2} for name in ("row_digests", "row_sizes", "msg_digests", "msg_sizes", "sizes", "uses")]
    bad += [{name: a + 4} for name in ("row_dst", "msg_offsets", "src", "dst", "job_rows", "job_msgs")]
    for change in bad:
        for v in outs:
            v.value = 7
        assert L.sf_place_block_data_device(*_place_args(a, **change), *refs, None) == EINVAL, change
        assert [v.value for v in outs] == [0, 0, 0]
    # a misaligned list is refused with a zero count too: nothing is read from it, but the caller's bug is there
    assert L.sf_place_block_data_device(*_place_args(a, n_rows=0, row_dst=a + 4), *refs, None) == EINVAL


def test_place_with_no_rows_and_no_messages_needs_no_device():
    L = syncfast_amd.lib()
    outs = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    refs = tuple(ctypes.byref(v) for v in outs)
    assert L.sf_place_block_data_device(*_place_args(None, n_rows=0, n_msgs=0, cap=0), *refs, None) == 0
    assert [v.value for v in outs] == [0, 0, 0]


# ------------------------------------------------ the rules, under sanitizers

@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("want_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode or \
            subprocess.run([str(tmp / "probe")], capture_output=True).returncode:
        pytest.skip("g++ -fsanitize=address,undefined unavailable")
    exe = tmp / "want_plan"
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "native", "want_plan.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _run(program, *args):
    r = subprocess.run([program, *args], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_rules_under_asan_ubsan(program):
    assert _run(program).strip() == "ok"


@pytest.mark.parametrize("n", [0, 1, 2, 5, 64, 257])
def test_the_serial_run_is_write_message_over_the_asking_rows(program, tmp_path, n):
    rng = random.Random(300 + n)
    digests = [rng.randbytes(20) for _ in range(n)]
    if n >= 2:
        digests[0], digests[1] = b"GET_BLOCK\n" * 2, b"\n" * 20
    rows = [rng.choice((-1, -1, 0, 3, 1 << 40)) for _ in range(n)]
    take = [rng.choice((0, 1, 255)) for _ in range(n)]
    path = tmp_path / "table.txt"
    for has_rows in (0, 1):
        for has_take in (0, 1):
            path.write_text(f"{has_rows} {has_take} {n}\n" +
                            "".join(f"{r} {t} {d.hex()}\n" for r, t, d in zip(rows, take, digests)))
            want = b"".join(wire.write_message("GetBlock", d) for r, t, d in zip(rows, take, digests)
                            if (not has_rows or r < 0) and (not has_take or t))
            got = _run(program, str(path)).strip()
            assert (b"" if got == "-" else bytes.fromhex(got)) == want


# ------------------------------------------------ the end-to-end test's input

def test_the_end_to_end_input_repeats_digests_under_the_host_cut():
    """test_gpu_want.py's two-route test needs a missing list with repeats and
    a digest in three or more rows; the host ZPAQ cut says the seed gives
    both, and that the destination holds some of the source's blocks."""
    import hashlib
    from collections import Counter

    from syncfast_amd import host
    from want_expect import e2e_files, missing_of

    def digests(data):
        offs, sizes = host.zpaq_cut_buffer(data)
        return [hashlib.sha1(data[int(o):int(o) + int(s)]).digest() for o, s in zip(offs, sizes)]
    source, old = e2e_files()
    src = digests(source)
    missing = missing_of(src, digests(old))
    assert 0 < len(missing) < len(src)
    assert len(missing) > len(set(missing))
    assert max(Counter(missing).values()) >= 3


# ------------------------------------------------ Index.missing_rows

def test_missing_rows_agree_with_list_missing_blocks():
    rng = random.Random(12)
    idx = Index.open_in_memory()
    a = idx.add_temp_file("a.bin")
    b = idx.add_temp_file("dir/b.bin")
    twice = HashDigest(rng.randbytes(20))
    want, at = [], {a: 0, b: 0}
    # interleaved: rows of the two files alternate, present and missing alternate irregularly, one digest is
    # missing in three rows and present in one
    for k in range(60):
        fid = (a, b)[k % 2] if k % 7 else a
        h = twice if k in (5, 6, 30, 41) else HashDigest(rng.randbytes(20))
        size = rng.randrange(1, 5000)
        if k == 30 or (k not in (5, 6, 41) and rng.random() < 0.4):
            idx.add_block(h, fid, at[fid], size)
        else:
            idx.add_missing_block(h, fid, at[fid], size)
            want.append((fid, at[fid], size, h))
        at[fid] += size
    idx.commit()
    rows = idx.missing_rows()
    assert [r[5] for r in rows] == idx.list_missing_blocks() and len(rows) == len(want) > 20
    assert [(r[1], r[3], r[4], r[5]) for r in rows] == want
    assert [r[0] for r in rows] == sorted(r[0] for r in rows) and len({r[0] for r in rows}) == len(rows)
    names = {a: PurePath(".syncfast_tmp_a.bin"), b: PurePath("dir/.syncfast_tmp_b.bin")}
    assert all(r[2] == names[r[1]] for r in rows)
    assert [r[5] for r in rows].count(twice) == 3
    # every rowid names the row it was read from
    for rowid, fid, _name, offset, size, h in rows:
        assert idx.db.execute("SELECT file_id, offset, size, hash, present FROM blocks WHERE rowid = ?;",
                              (rowid,)).fetchone() == (fid, offset, size, h.to_sql(), 0)
    # a row marked present leaves the list; the others keep their order
    idx.mark_block_present(rows[3][1], rows[3][5], rows[3][3])
    idx.commit()
    assert idx.missing_rows() == rows[:3] + rows[4:]
    assert Index.open_in_memory().missing_rows() == []
