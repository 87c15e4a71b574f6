"""CPU: the files-list rules (syncfast_amd/csrc/sf_wire_entries.hpp) --
entry_message, classify_entries, the serial parse_entries_run (which defines
sf_receive_file_entries_device and is its fallback), utf8_ok, the writers of
FILE_ENTRY / END_FILES / GET_FILE with their refusals, and the name hash --
alone, in tests/native/wire_entries.cpp: a stand-alone program with its own
main, built with ASan + UBSan and run directly (nothing is loaded into Python
under a sanitizer).  Every expected value is entries_expect's, from
wire.Parser, wire.write_message and bytes.decode."""
import os
import random
import struct
import subprocess

import pytest

from entries_expect import (END, END_FILES, END_FILES_MSG, INCOMPLETE, MALFORMED, OTHER, candidates, carries, entries_run,
                            entry, expected, get_files_run, needs_fallback, utf8_ok)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
ENV = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")

D1, D2, NL = bytes(range(1, 21)), b"\xff" * 5 + b"B" * 15, b"\n" * 20


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wire_entries")
    probe = tmp / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode or \
            subprocess.run([str(tmp / "probe")], capture_output=True).returncode:
        pytest.skip("g++ -fsanitize=address,undefined unavailable")
    exe = tmp / "wire_entries"
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "wire_entries.cpp"),
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
        if ln[0] in "RUWGH":
            out.append([])
        out[-1].append(ln.split(" "))
    assert len(out) == len(records)
    return out


def P(stream):
    return b"P" + struct.pack("<Q", len(stream)) + stream


def _hold(lines, stream, what):
    """One parse record of the program's output against the model."""
    e = expected(stream)
    assert [int(v) for v in lines[0][1:]] == [len(e.sizes), e.consumed, e.stop, -1 if e.bad_name is None else e.bad_name], what
    assert [ln[1:] for ln in lines if ln[0] == "E"] == [[str(a), str(n), str(s), h.hex()] for a, n, s, h in
                                                         zip(e.name_at, e.name_len, e.sizes, e.hashes)], what
    assert [ln[1:] for ln in lines if ln[0] == "C"] == [[str(p), str(n), str(k)] for p, n, k in candidates(stream)], what
    return e


def table():
    """[(name, stream)]: the fixed cases (test_gpu_file_entries.py runs the
    same table on the device)."""
    three = entry(b"dir/a", 5, D1) + entry(b"", 0, D2) + entry(b"b" * 7, 10 ** 15 - 1, D1)
    c = [("nothing", b""), ("three", three), ("three_end", three + END_FILES_MSG), ("end_only", END_FILES_MSG),
         ("end_then_more", three + END_FILES_MSG + three)]
    # every stop class at the end of a valid prefix and at byte 0
    for other in (b"GET_FILE\nx", b"FILE_START\n", b"FILE_END\n", b"GET_BLOCK\n", b"FILE_BLOCK\n", b"BLOCK_DATA\n",
                  b"COMPLETE\nrest"):
        c += [("other", three + other), ("other_first", other)]
    for bad in (b"BOGUS\n", b"X" * 20, b"\n" + three, b"file_entry\n", b"END_FILE\n"):
        c += [("malformed", three + bad), ("malformed_first", bad)]
    c.append(("x19", three + b"X" * 19))
    # every proper prefix of a 3-entry list with END_FILES
    whole = three + END_FILES_MSG
    c += [("prefix", whole[:t]) for t in range(1, len(whole))]
    # names of 0, 1, 99 and 100 bytes; 100 and 101 bytes without newline
    c += [("name%d" % n, entry(b"q" * n, n, D1) + END_FILES_MSG) for n in (0, 1, 99, 100)]
    c += [("name101", entry(b"q" * 101, 1, D1)), ("name100_open", b"FILE_ENTRY\n" + b"q" * 100),
          ("name99_open", b"FILE_ENTRY\n" + b"q" * 99), ("name101_open", three + b"FILE_ENTRY\n" + b"q" * 101)]
    # size fields
    for k, field in (("0", b"0"), ("plus7", b"+7"), ("007", b"007"), ("15digits", b"9" * 15), ("plus14", b"+" + b"1" * 14)):
        c.append(("size_" + k, three + entry(b"s", field, D2) + END_FILES_MSG))
    for k, field in (("16", b"1" * 16), ("minus1", b"-1"), ("empty", b""), ("1a", b"1a"), ("plus", b"+"), ("space", b" 1")):
        c += [("badsize_" + k, three + entry(b"s", field, D2)), ("badsize_early_" + k, b"FILE_ENTRY\ns\n" + field + b"\n")]
    c += [("size15_open", three + b"FILE_ENTRY\ns\n" + b"1" * 15), ("size14_open", three + b"FILE_ENTRY\ns\n" + b"1" * 14)]
    # a digest of 20 newlines; a wrong byte after the digest; the digest there and its newline not yet
    c += [("digest_newlines", entry(b"n", 3, NL) + entry(b"m", 4, NL) + END_FILES_MSG),
          ("digest_unterminated", three + b"FILE_ENTRY\nu\n5\n" + D1 + b"x"),
          ("digest_unterminated_more", three + b"FILE_ENTRY\nu\n5\n" + D1 + b"x" + three),
          ("digest_20_of_21", three + b"FILE_ENTRY\nu\n5\n" + D1)]
    # an unknown command that begins like ours
    c += [("unknown", three + b"FILE_ENTRIES\n"), ("unknown_long", three + b"FILE_ENTRY_AND_MORE_THAN_20\n")]
    # forged starts: a digest that spells a whole entry's head, a name that ends in the tag
    forged = b"FILE_ENTRY\n\n1\n" + b"z" * 6
    assert len(forged) == 20
    # (the forged entry: no name, size 1, its digest the 6 z, the true entry's newline and 13 bytes behind it -- the
    # head of an entry with a 2-byte name, whose name's newline ends the forged one -- or 13 y and a newline)
    c += [("forged_digest", entry(b"f", 1, forged) + entry(b"ab", 5, D1) + three),
          ("forged_digest_last", three + entry(b"f", 1, forged) + b"y" * 13 + b"\n"),
          ("forged_name", entry(b"x/FILE_ENTRY", 1, b"1\n" + b"h" * 18) + b"h" + b"\n"),
          ("name_tag_honest", entry(b"x/FILE_ENTRY", 12, D1) + three + END_FILES_MSG)]
    return c


def test_fixed_table_under_asan_ubsan(program, tmp_path):
    cases = table()
    assert len(cases) > 200
    seen, stops = {}, set()
    for lines, (name, stream) in zip(_run(program, tmp_path / "table.bin", [P(s) for _n, s in cases]), cases):
        e = _hold(lines, stream, name)
        stops.add(e.stop)
        seen.setdefault(name, []).append(e)
    assert stops == {END, INCOMPLETE, OTHER, MALFORMED, END_FILES}
    # the table shows what it is meant to show
    assert all(e.stop == OTHER for k in ("other", "other_first") for e in seen[k])
    assert all(e.stop == MALFORMED for k in seen if k.startswith(("malformed", "badsize_", "unknown")) for e in seen[k])
    assert all(seen[k][0].stop == MALFORMED for k in ("name101", "name100_open", "name101_open", "size15_open",
                                                      "digest_unterminated", "digest_unterminated_more"))
    assert all(seen[k][0].stop == INCOMPLETE for k in ("x19", "name99_open", "size14_open", "digest_20_of_21"))
    assert (seen["three_end"][0].stop, seen["three_end"][0].consumed) == (END_FILES, len(cases[2][1]))
    assert (seen["end_only"][0].stop, seen["end_only"][0].consumed, seen["end_only"][0].sizes) == (END_FILES, 10, [])
    assert seen["end_then_more"][0].consumed == seen["three_end"][0].consumed  # nothing is read past END_FILES
    # (one prefix raises: the third entry's 15 size digits with their newline not there yet, "Unterminated size")
    assert sorted(e.stop for e in seen["prefix"] if e.stop != INCOMPLETE) == [END, END, END, MALFORMED]
    assert len(seen["prefix"]) == len(cases[2][1]) - 1
    assert [len(e.sizes) for k in ("name0", "name1", "name99", "name100") for e in seen[k]] == [1] * 4
    assert seen["size_15digits"][0].sizes[-1] == 10 ** 15 - 1 and seen["size_plus7"][0].sizes[-1] == 7
    assert seen["size_007"][0].sizes[-1] == 7 and seen["size_plus14"][0].sizes[-1] == int("1" * 14)
    assert seen["digest_newlines"][0].hashes == [b"\n" * 20] * 2 and seen["digest_newlines"][0].stop == END_FILES
    streams = dict(cases)
    for k in ("forged_digest", "forged_digest_last", "forged_name"):
        assert needs_fallback(streams[k]), k
    assert not needs_fallback(streams["name_tag_honest"]) and not needs_fallback(streams["three_end"])
    assert len(seen["forged_digest"][0].sizes) == 5 and len(seen["forged_name"][0].sizes) == 1
    assert len(seen["forged_digest_last"][0].sizes) == 4


def hostile(rng: random.Random) -> bytes:
    """A list built from the protocol's own bytes: digests that spell a whole
    entry, names ending in FILE_ENTRY, odd size fields, other commands, broken
    fields and cuts."""
    def digest():
        r = rng.random()
        if r < 0.3:  # a whole entry's head with no name and size 1: forged when a 2-byte name follows
            return b"FILE_ENTRY\n\n1\n" + rng.randbytes(6)
        if r < 0.4:
            return b"\n" * 20
        return rng.randbytes(20)

    def name():
        if rng.random() < 0.35:
            return bytes(rng.choice(b"ab\xc3\xa9") for _ in range(2))  # 2 bytes: completes a forged digest before it
        n = bytes(rng.choice(b"abc/._-F\xc3\xa9") for _ in range(rng.choice((0, 1, 3, 8, 40, 99, 100))))
        if rng.random() < 0.3:  # the tag, the true size as a name, the digest's first bytes as a size
            n = n[:88] + b"/FILE_ENTRY"
        return n

    out = b""
    for _ in range(rng.randrange(1, 9)):
        nm = name()
        d = b"1\n" + rng.randbytes(18) if nm.endswith(b"FILE_ENTRY") and rng.random() < 0.5 else digest()
        out += entry(nm, rng.choice((0, 1, 4096, 10 ** 15 - 1, b"+7", b"007")), d)
    r = rng.random()
    if r < 0.5:
        out += END_FILES_MSG + (entry(b"late", 1, D1) if rng.random() < 0.3 else b"")
    elif r < 0.6:
        out += rng.choice((b"COMPLETE\n", b"GET_FILE\nx\n", b"FILE_START\nx\n"))
    elif r < 0.75:
        out += rng.choice((b"BOGUS\n", b"FILE_ENTRY\nn\n1x\n", b"FILE_ENTRY\n" + b"n" * 101 + b"\n", entry(b"n", 1, D1)[:-1] + b"x"))
    elif r < 0.9:
        out = out[:len(out) - rng.randrange(1, 40)]
    return out


def test_serial_parse_equals_the_model_on_hostile_lists(program, tmp_path):
    rng = random.Random(12)
    cases = [hostile(rng) for _ in range(200)]
    stops, fallbacks, bad_names = set(), 0, 0
    for lines, stream in zip(_run(program, tmp_path / "hostile.bin", [P(s) for s in cases]), cases):
        e = _hold(lines, stream, stream)
        stops.add(e.stop)
        fallbacks += needs_fallback(stream)
        bad_names += e.bad_name is not None
    assert stops == {END, INCOMPLETE, OTHER, MALFORMED, END_FILES}
    assert 10 <= fallbacks < len(cases) and 10 <= bad_names < len(cases)


UTF8 = [b"", b"plain/name.txt", "grüß/中文/\U0001f600".encode(), b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80\x80",
        b"\xe0\x9f\xbf", b"\xe0\xa0\x80", b"\xed\xa0\x80", b"\xed\x9f\xbf", b"\xed\xbf\xbf", b"\xee\x80\x80", b"\xf0\x8f\xbf\xbf",
        b"\xf0\x90\x80\x80", b"\xf4\x8f\xbf\xbf", b"\xf4\x90\x80\x80", b"\xf5", b"\xf5\x80\x80\x80", b"\xf8\x88\x80\x80\x80",
        b"\x80", b"a\x80", b"\xbf", b"\xff", b"\xfe", b"\xc2", b"\xc2\x41", b"\xe2\x82", b"\xe2\x82\x41", b"\xe2\x41\x82",
        b"\xf0\x9f", b"\xf0\x9f\x98", b"\xf0\x9f\x98\x41", b"\xc2\xa9\xc2", b"\x7f", b"\xef\xbf\xbf", b"\xef\xbb\xbf"]


def test_utf8_ok_is_rusts_from_utf8(program, tmp_path):
    """The table of the issue, every length truncated at the name's end, a
    100-byte name ending in a 4-byte character, and seeded mutations of valid
    names, against bytes.decode("utf-8")."""
    names = list(UTF8)
    for ch in ("é", "€", "\U0001f600"):
        full = ch.encode()
        names += [b"ab" + full[:k] for k in range(1, len(full) + 1)]
    smile = "\U0001f600".encode()
    names += [b"n" * 96 + smile, b"n" * 97 + smile[:3], b"n" * 96 + smile[:3] + b"n"]
    rng = random.Random(5)
    base = "déjà/中/\U0001f600x".encode()
    for _ in range(300):
        b = bytearray(base)
        for _ in range(rng.randrange(1, 3)):
            b[rng.randrange(len(b))] = rng.choice((0x80, 0xBF, 0xC0, 0xC2, 0xE0, 0xED, 0xF0, 0xF4, 0xF5, 0x41, rng.randrange(256)))
        names.append(bytes(b[:rng.randrange(1, len(b) + 1)]))
    assert all(len(n) <= 100 for n in names)
    out = _run(program, tmp_path / "utf8.bin", [b"U" + struct.pack("<Q", len(n)) + n for n in names])
    want = [utf8_ok(n) for n in names]
    assert [lines[0][1] == "1" for lines in out] == want
    assert want[:3] == [True] * 3 and not any(want[3:7]) and want[7] and not want[8] and want[9]
    assert 50 < sum(want) < len(want) - 50


def W(files, end):
    return b"W" + struct.pack("<II", len(files), int(end)) + b"".join(
        struct.pack("<IQ", len(n), s) + n + h for n, s, h in files)


def G(data, spans, pick):
    return (b"G" + struct.pack("<Q", len(data)) + data + struct.pack("<I", len(spans))
            + b"".join(struct.pack("<QI", a, n) for a, n in spans)
            + struct.pack("<II", int(pick is not None), len(pick or ())) + b"".join(struct.pack("<I", k) for k in pick or ()))


def test_writers_are_write_message_and_refuse_what_the_protocol_cannot_carry(program, tmp_path):
    good = [(b"", 0, D1), (b"a", 9, D2), (b"n" * 99, 10, NL), (b"n" * 100, 10 ** 15 - 1, D1), (b"dir/\xc3\xa9", 123456789012, D2)]
    lists = [(good, True), (good, False), ([], True), ([], False), (good[:1], True)]
    for k, bad in enumerate(((b"x", 10 ** 15, D1), (b"n" * 101, 1, D1), (b"a\nb", 1, D1), (b"\n", 1, D1), (b"x", (1 << 64) - 1, D1))):
        lists.append((good[:k] + [bad] + good, True))
    out = _run(program, tmp_path / "w.bin", [W(f, e) for f, e in lists])
    for lines, (files, end) in zip(out, lists):
        bad = [i for i, (n, s, _h) in enumerate(files) if not carries(n, s)]
        if bad:
            assert lines[0][1:] == ["bad", str(bad[0])]
        else:
            assert lines[0][1] == "ok" and bytes.fromhex(lines[0][2] if len(lines[0]) > 2 else "") == entries_run(files, end)
    assert sum(1 for f, _e in lists if all(carries(n, s) for n, s, _h in f)) == 5
    # the requests: spans of a received list, in place
    e = expected(entries_run(good))
    data, spans = entries_run(good), list(zip(e.name_at, e.name_len))
    picks = [None, [], [4, 0, 0, 2], [3], [5], [0, 1 << 31]]
    reqs = [(data, spans, p) for p in picks]
    reqs += [(data, spans + [(len(data) - 3, 4)], [5]), (data, spans + [(len(data) + 1, 0)], [5]), (data, spans + [(len(data), 0)], [5]),
             (data, [(0, 101)], None), (data, [(5, 10)], None), (data, [(11, 0), (0, 10)], [1, 0]), (b"", [], None)]
    out = _run(program, tmp_path / "g.bin", [G(*r) for r in reqs])
    results = []
    for lines, (d, sp, pick) in zip(out, reqs):
        order = list(range(len(sp))) if pick is None else pick
        bad = None
        for k, i in enumerate(order):
            if i >= len(sp) or sp[i][0] + sp[i][1] > len(d) or sp[i][0] > len(d) or sp[i][1] > 100 \
                    or b"\n" in d[sp[i][0]:sp[i][0] + sp[i][1]]:
                bad = k
                break
        results.append(bad)
        if bad is not None:
            assert lines[0][1:] == ["bad", str(bad)]
        else:
            want = get_files_run([d[sp[i][0]:sp[i][0] + sp[i][1]] for i in order])
            assert lines[0][1] == "ok" and bytes.fromhex(lines[0][2] if len(lines[0]) > 2 else "") == want
    assert results == [None, None, None, None, 0, 1, 0, 0, None, 0, 0, None, None]


def _name_hash(name: bytes, mask: int) -> int:
    """sf_wire_entries.hpp's name_hash: 64-bit FNV-1a and a 64-bit finisher."""
    m64 = (1 << 64) - 1
    h = 0xCBF29CE484222325
    for b in name:
        h = ((h ^ b) * 0x100000001B3) & m64
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & m64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & m64
    h ^= h >> 33
    return h & mask if mask else h


def test_name_hash_with_the_mask(program, tmp_path):
    names = [b"", b"a", b"b", b"a\0", b"dir/file", b"dir/filf", b"n" * 300, bytes(range(256))]
    masks = [0, 1, 1 << 63, 0xFFFF, (1 << 64) - 1]
    out = _run(program, tmp_path / "h.bin", [b"H" + struct.pack("<QQ", m, len(n)) + n for m in masks for n in names])
    got = [int(lines[0][1], 16) for lines in out]
    assert got == [_name_hash(n, m) for m in masks for n in names]
    plain = got[:len(names)]
    assert len(set(plain)) == len(names) and len({h & 1023 for h in plain}) >= 6  # the low bits spread
    assert set(got[len(names):2 * len(names)]) == {0, 1}  # mask 1: two probe sequences
    assert {h & ((1 << 63) - 1) for h in got[2 * len(names):3 * len(names)]} == {0}  # no slot bit left: one slot
