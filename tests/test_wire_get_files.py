"""CPU: the rules of a received GET_FILE run and of its answer
(syncfast_amd/csrc/sf_wire_get_files.hpp) -- get_file_message,
classify_get_files, the serial parse_get_files_run, the same parse told by
lines (what the kernels of sf_serve_files.hip run) and build_serve_files_serial,
the definition of sf_serve_get_files_device's plan -- alone, in
tests/native/wire_get_files.cpp: a stand-alone program with its own main, built
with ASan + UBSan and run directly (nothing is loaded into Python under a
sanitizer).  Every expected value is get_files_expect's, from wire.Parser,
wire.write_message and bytes.decode."""
import os
import random
import struct
import subprocess

import pytest

from get_files_expect import (ALL, BAD_NAME, END, FULL, INCOMPLETE, MALFORMED, OTHER, THREE, UNKNOWN, by_lines, candidates,
                              expected, hostile, plan_cases, plan_source, served, table)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
ENV = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wire_get_files")
    probe = tmp / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode or \
            subprocess.run([str(tmp / "probe")], capture_output=True).returncode:
        pytest.skip("g++ -fsanitize=address,undefined unavailable")
    exe = tmp / "wire_get_files"
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "wire_get_files.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def _run(program, path, records):
    """The program over ``records`` (packed bytes each) -> its output lines
    grouped per record."""
    with open(path, "wb") as f:
        f.write(b"".join(records))
    r = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok %d" % len(records)
    out = []
    for ln in lines[:-1]:
        if ln[0] in "RS":
            out.append([])
        out[-1].append(ln.rstrip(" ").split(" "))
    assert len(out) == len(records)
    return out


def P(stream):
    return b"P" + struct.pack("<Q", len(stream)) + stream


def S(stream, source, max_run_bytes=0, broken=-1):
    return (b"S" + struct.pack("<Q", len(stream)) + stream + struct.pack("<QqI", max_run_bytes, broken, len(source))
            + b"".join(struct.pack("<I", len(n)) + n + struct.pack("<BI", int(p), len(rows))
                       + b"".join(d + struct.pack("<I", s) for d, s in rows) for n, p, rows in source))


def _hold(lines, stream, what):
    """One parse record of the program's output against the model."""
    e = expected(stream)
    assert [int(v) for v in lines[0][1:]] == [len(e.names), e.consumed, e.stop, -1 if e.bad_name is None else e.bad_name], what
    assert [ln[1:] for ln in lines if ln[0] == "E"] == [[str(a), str(n)] for a, n in zip(e.name_at, e.name_len)], what
    assert [ln[1:] for ln in lines if ln[0] == "C"] == [[str(p), str(n), str(k)] for p, n, k in candidates(stream)], what
    assert by_lines(stream) == (len(e.names), e.consumed), what  # the issue's model of the parse
    return e


def test_fixed_table_under_asan_ubsan(program, tmp_path):
    cases = table()
    assert len(cases) > 90
    seen, stops = {}, set()
    for lines, (name, stream) in zip(_run(program, tmp_path / "table.bin", [P(s) for _n, s in cases]), cases):
        e = _hold(lines, stream, name)
        stops.add(e.stop)
        seen.setdefault(name, []).append(e)
    assert stops == {END, INCOMPLETE, OTHER, MALFORMED}
    # the table shows what it is meant to show
    assert (seen["nothing"][0].names, seen["nothing"][0].stop) == ([], END)
    assert (seen["three"][0].names, seen["three"][0].consumed) == ([b"dir/a", b"", b"b" * 7], len(THREE))
    assert all(e.stop == OTHER for k in ("other", "other_first") for e in seen[k]) and len(seen["other"]) == 8
    assert all(e.stop == MALFORMED for k in ("malformed", "malformed_first") for e in seen[k])
    assert all(len(e.names) == 3 for e in seen["other"] + seen["malformed"]) and not any(
        e.names for e in seen["other_first"] + seen["malformed_first"])
    assert seen["x19"][0].stop == INCOMPLETE
    assert len(seen["prefix"]) == len(THREE) - 1 and {e.stop for e in seen["prefix"]} == {END, INCOMPLETE}
    assert [len(e.names) for k in ("name0", "name1", "name99", "name100") for e in seen[k]] == [7] * 4
    # the filename quirk: 100 name bytes with no newline raise although a 101st byte could still be one
    for k in ("name100_open", "name101_open", "name101", "name100_open_first", "name300"):
        assert seen[k][0].stop == MALFORMED, k
    assert (seen["name99_open"][0].stop, len(seen["name99_open"][0].names)) == (INCOMPLETE, 3)
    assert seen["name_ends_in_tag"][0].names[0] == b"x/GET_FILE" and len(seen["name_ends_in_tag"][0].names) == 4
    assert seen["name_is_tag"][0].names[:2] == [b"GET_FILE", b"dir/a"]
    assert (seen["name_is_tag_twice"][0].names, seen["name_is_tag_twice"][0].stop) == ([b"GET_FILE"] * 2, INCOMPLETE)
    assert (seen["tag_only"][0].stop, seen["tag_only"][0].consumed) == (INCOMPLETE, len(THREE))
    assert (seen["complete"][0].stop, seen["get_block_newlines"][0].stop) == (OTHER, OTHER)
    assert len(seen["get_block_newlines"][0].names) == 3 and seen["long_line_then_requests"][0].stop == MALFORMED
    assert [seen[k][0].bad_name for k in ("bad_name_first", "bad_name_middle", "bad_name_last", "bad_name_twice")] == [0, 1, 3, 1]
    assert len(seen["bad_name_first"][0].names) == 4  # the requests behind it are parsed all the same


def test_serial_parse_equals_the_model_on_hostile_runs(program, tmp_path):
    rng = random.Random(31)
    cases = [hostile(rng) for _ in range(200)]
    stops, bad_names, counts = set(), 0, set()
    for lines, stream in zip(_run(program, tmp_path / "hostile.bin", [P(s) for s in cases]), cases):
        e = _hold(lines, stream, stream)
        stops.add(e.stop)
        bad_names += e.bad_name is not None
        counts.add(len(e.names))
    assert stops == {END, INCOMPLETE, OTHER, MALFORMED}
    assert 10 <= bad_names < len(cases) and {0, 1, 2} <= counts and max(counts) >= 7


def _held(line, want, what):
    n_req, n_ans, used, why, bad_row, messages, consumed, stop = (int(v) for v in line[1:9])
    run = bytes.fromhex(line[9]) if len(line) > 9 else b""
    assert (run, n_req, n_ans, used, why, consumed, stop, messages) == tuple(want), what
    assert bad_row == -1, what


def test_the_plan_equals_the_reference_loop(program, tmp_path):
    source = plan_source(random.Random(40))
    cases = plan_cases(source)
    out = _run(program, tmp_path / "plan.bin", [S(stream, source, m) for _n, stream, m in cases])
    got = {}
    for lines, (name, stream, m) in zip(out, cases):
        want = served(stream, source, m)
        _held(lines[0], want, name)
        got[name] = want
    whys = {k: (v.why, v.n_answered, v.n_requests) for k, v in got.items()}
    assert whys["every_present_file"] == (ALL, 11, 11) and whys["only_empty"] == (ALL, 3, 3)
    assert len(got["only_empty"].run) == 3 * (12 + 2 + 9)  # an empty file gives two frames
    assert whys["one_file_three_times"] == (ALL, 3, 3) and got["one_file_three_times"].messages == 3 * 72
    assert got["lower_row_not_present"].messages == 2 + 2 + 5 + 2 + 2 + 2  # the present "twice" has 2 blocks, the other 4
    assert whys["unknown_before_bad_name"] == (UNKNOWN, 1, 3) and whys["bad_name_before_unknown"] == (BAD_NAME, 1, 3)
    assert whys["bad_name_is_also_unknown"] == (BAD_NAME, 1, 2)
    assert whys["unknown_first"] == (UNKNOWN, 0, 2) and whys["bad_name_first"] == (BAD_NAME, 0, 2)
    assert (got["stop_other"].stop, got["stop_incomplete"].stop, got["stop_malformed"].stop) == (OTHER, INCOMPLETE, MALFORMED)
    assert whys["full_exact"] == (ALL, 3, 3) and whys["full_one_short"] == (FULL, 2, 3)
    assert whys["full_below_first"] == (FULL, 0, 3) and whys["full_first_exact"] == (FULL, 1, 3) and whys["full_one"] == (FULL, 0, 3)
    assert got["full_one_short"].answered_bytes == len(b"GET_FILE\na.bin\nGET_FILE\ndir/b.bin\n")


def test_a_broken_row_is_refused_only_where_answering_reaches_it(program, tmp_path):
    from entries_expect import get_files_run as g
    source = plan_source(random.Random(40))
    # row 8 (x/FILE_END) broken: first[8] above first[9], which breaks row 7's end too
    reqs = [(g([b"a.bin", b"x/FILE_END"]), 0, 8), (g([b"a.bin", b"dir/b.bin"]), 0, None),
            (g([b"a.bin", b"nope", b"x/FILE_END"]), 0, None), (g([b"a.bin", b"\xff", b"x/FILE_END"]), 0, None),
            (g([b"dir/b.bin", b"x/FILE_END"]), 100, None), (g([b"x/FILE_END"]), 1, 8), (g([b"twice"]), 0, 7)]
    out = _run(program, tmp_path / "broken.bin", [S(s, source, m, broken=8) for s, m, _b in reqs])
    for lines, (stream, m, bad) in zip(out, reqs):
        if bad is None:
            _held(lines[0], served(stream, source, m), stream)
        else:
            assert int(lines[0][5]) == bad, stream
