"""What a received GET_FILE run must parse to and what its answer must be, from
syncfast_amd.wire.Parser, wire.write_message and bytes.decode alone (shared by
test_wire_get_files.py, test_serve_files_capi.py and test_gpu_serve_files*.py;
no code under test).  A source is a list of rows (name, present, [(digest,
size)]) in file_id order -- the name set's rows and the CSR into the block
table."""
import random
from collections import namedtuple

from entries_expect import get_file, get_files_run, utf8_ok
from syncfast_amd import wire

END, INCOMPLETE, OTHER, MALFORMED = 0, 1, 2, 3
ALL, BAD_NAME, UNKNOWN, FULL = 0, 1, 2, 3
OTHERS = (b"FILE_ENTRY", b"END_FILES", b"FILE_START", b"FILE_END", b"GET_BLOCK", b"FILE_BLOCK", b"BLOCK_DATA",
          b"COMPLETE")
NONE = (1 << 64) - 1

Expected = namedtuple("Expected", "name_at name_len names consumed stop bad_name")
Served = namedtuple("Served", "run n_requests n_answered answered_bytes why consumed stop messages")


def _parser(stream: bytes):
    p = wire.Parser()
    p._buf = bytearray(stream)
    return p


def _at(p, pos):
    """What stands at pos: ((kind, name), end) for a whole GET_FILE, else the
    stop class."""
    if pos == len(p._buf):
        return END
    try:
        line = p._line(pos, wire.COMMAND_MAX, "Unterminated command")
        if line is None:
            return INCOMPLETE
        if line[0] in OTHERS:  # their complete command line, whatever follows it
            return OTHER
        r = p._one(pos)  # GET_FILE, or an unknown command (raises)
    except wire.ProtocolError:
        return MALFORMED
    return INCOMPLETE if r is None else r


def expected(stream: bytes) -> Expected:
    """Every output of sf_wire_parse_get_files_device's contract for
    ``stream``: the reference parser's GET_FILE messages from byte 0."""
    p = _parser(stream)
    name_at, name_len, names = [], [], []
    pos, bad = 0, None
    while True:
        r = _at(p, pos)
        if isinstance(r, int):
            return Expected(name_at, name_len, names, pos, r, bad)
        (kind, name), end = r
        assert kind == "GetFile" and stream[pos + 9:pos + 9 + len(name)] == name
        if bad is None and not utf8_ok(name):
            bad = len(names)
        name_at.append(pos + 9), name_len.append(len(name)), names.append(name)
        pos = end


def candidates(stream: bytes):
    """[(position, length, name length)] of every position where
    ``Parser._one`` reads a whole GET_FILE: every position is tried."""
    p, out = _parser(stream), []
    for pos in range(len(stream)):
        try:
            r = p._one(pos)
        except wire.ProtocolError:
            r = None
        if r is not None and r[0][0] == "GetFile":
            out.append((pos, r[1] - pos, len(r[0][1])))
    return out


def by_lines(stream: bytes):
    """(requests, consumed) by the line rule alone: request k is lines 2k and
    2k + 1, the first "GET_FILE", the second at most 100 bytes."""
    lines = stream.split(b"\n")[:-1]  # the terminated ones
    bad = next((j for j, ln in enumerate(lines) if (len(ln) > 100 if j & 1 else ln != b"GET_FILE")), len(lines))
    k = bad // 2
    return k, sum(len(ln) + 1 for ln in lines[:2 * k])


THREE = get_file(b"dir/a") + get_file(b"") + get_file(b"b" * 7)


def table():
    """[(name, stream)]: the fixed cases of the parse (test_gpu_serve_files.py
    runs the same table on the device)."""
    c = [("nothing", b""), ("three", THREE)]
    # every stop class behind a valid prefix and at byte 0
    for other in (b"FILE_ENTRY\nx", b"END_FILES\n", b"FILE_START\n", b"FILE_END\n", b"GET_BLOCK\n", b"FILE_BLOCK\n",
                  b"BLOCK_DATA\n", b"COMPLETE\nrest"):
        c += [("other", THREE + other), ("other_first", other)]
    for bad in (b"BOGUS\n", b"X" * 20, b"\n" + THREE, b"get_file\n", b"GET_FILES\n", b"GET_FIL\n", b" GET_FILE\nx\n"):
        c += [("malformed", THREE + bad), ("malformed_first", bad)]
    c.append(("x19", THREE + b"X" * 19))
    c += [("prefix", THREE[:t]) for t in range(1, len(THREE))]
    # names of 0, 1, 99 and 100 bytes; 100 and 101 name bytes unterminated; 101 terminated
    c += [("name%d" % n, THREE + get_file(b"q" * n) + THREE) for n in (0, 1, 99, 100)]
    c += [("name100_open", THREE + b"GET_FILE\n" + b"q" * 100), ("name101_open", THREE + b"GET_FILE\n" + b"q" * 101),
          ("name99_open", THREE + b"GET_FILE\n" + b"q" * 99), ("name101", THREE + b"GET_FILE\n" + b"q" * 101 + b"\n" + THREE),
          ("name100_open_first", b"GET_FILE\n" + b"q" * 100), ("name300", b"GET_FILE\n" + b"q" * 300 + b"\n" + THREE)]
    # names that spell the protocol
    c += [("name_ends_in_tag", get_file(b"x/GET_FILE") + THREE), ("name_is_tag", get_file(b"GET_FILE") + THREE),
          ("name_is_tag_twice", get_file(b"GET_FILE") + get_file(b"GET_FILE") + b"GET_FILE\n"),
          ("tag_only", THREE + b"GET_FILE\n")]
    # COMPLETE, and a GET_BLOCK whose digest is 20 newlines, behind the requests
    c += [("complete", THREE + wire.write_message("Complete")),
          ("get_block_newlines", THREE + b"GET_BLOCK\n" + b"\n" * 20 + b"\n" + THREE),
          ("long_line_then_requests", THREE + b"Z" * 500 + b"\n" + THREE)]
    # names that are no UTF-8: first, in the middle, last
    bad = b"bad\xff"
    c += [("bad_name_first", get_file(bad) + THREE), ("bad_name_middle", get_file(b"a") + get_file(b"\xc0\x80") + THREE),
          ("bad_name_last", THREE + get_file(b"\xed\xa0\x80")), ("bad_name_twice", get_file(b"ok") + get_file(bad) + get_file(bad))]
    return c


def hostile(rng: random.Random) -> bytes:
    """A run built from the protocol's own bytes: names that are or end in
    GET_FILE, names of 99 to 101 bytes, other commands, GET_BLOCK digests made
    of newlines, broken lines and cuts."""
    def name():
        r = rng.random()
        if r < 0.2:
            return rng.choice((b"GET_FILE", b"x/GET_FILE", b"GET_FILE/GET_FILE", b"END_FILES", b"COMPLETE"))
        if r < 0.35:
            return b"n" * rng.choice((99, 100))
        return bytes(rng.choice(b"ab/._-G\xc3\xa9\xff") for _ in range(rng.choice((0, 1, 3, 8, 40))))

    out = b""
    for _ in range(rng.randrange(0, 9)):
        out += get_file(name())
    r = rng.random()
    if r < 0.25:
        out += rng.choice((b"COMPLETE\n", b"GET_BLOCK\n" + b"\n" * 21, b"FILE_START\nx\n", b"END_FILES\n")) + get_file(name())
    elif r < 0.5:
        out += rng.choice((b"BOGUS\n", b"GET_FILE\n" + b"n" * 101 + b"\n", b"GET_FILE\n" + b"n" * 100, b"\n", b"GET_FILE \nx\n",
                           b"X" * rng.randrange(19, 23))) + (get_file(name()) if rng.random() < 0.5 else b"")
    elif r < 0.8 and out:
        out = out[:len(out) - rng.randrange(1, min(len(out), 40) + 1)]
    return out


# ------------------------------------------------------------- the answer

def lowest_present(source):
    first = {}
    for r, (name, present, _rows) in enumerate(source):
        if present:
            first.setdefault(name, r)
    return first


def served(stream: bytes, source, max_run_bytes: int = 0) -> Served:
    """sf_serve_get_files_device's contract for the request run ``stream``
    against ``source``: the reference's Respond loop over the parsed names with
    write_message, stopped where include/syncfast_amd.h says."""
    e = expected(stream)
    first = lowest_present(source)
    out, answered, why, messages = bytearray(), 0, ALL, 0
    for name in e.names:
        if not utf8_ok(name):
            why = BAD_NAME
            break
        r = first.get(name)
        if r is None:
            why = UNKNOWN
            break
        rows = source[r][2]
        answer = wire.write_message("FileStart", name) + b"".join(
            wire.write_message("FileBlock", d, s) for d, s in rows) + wire.write_message("FileEnd")
        if (max_run_bytes and len(out) + len(answer) > max_run_bytes) or messages + len(rows) + 2 > 1 << 32:
            why = FULL
            break
        out += answer
        answered += 1
        messages += len(rows) + 2
    used = e.name_at[answered - 1] + e.name_len[answered - 1] + 1 if answered else 0
    return Served(bytes(out), len(e.names), answered, used, why, e.consumed, e.stop, messages)


def plan_source(rng: random.Random):
    """About 12 rows of 0 to 70 blocks: empty files first, last and three in a
    row, a name in two rows whose lower one is not present, and a row that is
    not present at all."""
    def rows(n):
        return [(rng.randbytes(20), rng.choice((0, 9, 10, 99999, 4294967295, rng.randrange(1 << 20)))) for _ in range(n)]
    return [(b"empty_first", 1, []), (b"a.bin", 1, rows(5)), (b"twice", 0, rows(4)), (b"dir/b.bin", 1, rows(70)),
            (b"e1", 1, []), (b"e2", 1, []), (b"e3", 1, []), (b"twice", 1, rows(2)), (b"x/FILE_END", 1, rows(3)),
            (b"gone", 0, rows(1)), (b"", 1, rows(1)), (b"n" * 100, 1, rows(7)), (b"empty_last", 1, [])]


def plan_cases(source):
    """[(name, request stream, max_run_bytes)]: the plan table of the serve."""
    g = get_files_run
    everything = g([n for n, p, _r in source if p])
    c = [("every_present_file", everything, 0),
         ("empty_first_last_three", g([b"empty_first", b"e1", b"e2", b"e3", b"a.bin", b"empty_last"]), 0),
         ("only_empty", g([b"e1", b"e2", b"e3"]), 0),
         ("one_file_three_times", g([b"dir/b.bin"] * 3), 0),
         ("lower_row_not_present", g([b"twice", b"a.bin", b"twice"]), 0),
         ("unknown_before_bad_name", g([b"a.bin", b"nope", b"\xff"]), 0),
         ("bad_name_before_unknown", g([b"a.bin", b"\xff", b"nope"]), 0),
         ("bad_name_is_also_unknown", g([b"a.bin", b"\xc0\x80"]), 0),
         ("unknown_first", g([b"gone", b"a.bin"]), 0), ("bad_name_first", g([b"\xff", b"a.bin"]), 0),
         ("stop_other", g([b"a.bin", b""]) + b"COMPLETE\n", 0), ("stop_incomplete", g([b"a.bin", b"n" * 100]) + b"GET_FILE\nab", 0),
         ("stop_malformed", g([b"e1"]) + b"GET_FILE\n" + b"q" * 100, 0)]
    three = g([b"a.bin", b"dir/b.bin", b"x/FILE_END"])
    whole = served(three, source)
    one = served(g([b"a.bin"]), source)
    for k, m in (("exact", len(whole.run)), ("one_short", len(whole.run) - 1), ("below_first", len(one.run) - 1),
                 ("first_exact", len(one.run)), ("one", 1)):
        c.append(("full_" + k, three, m))
    return c


# ---------------------------------------------------- a source's arrays

def csr(source):
    """(names, present, first, digests, sizes): what the calls take."""
    first = [0]
    for _n, _p, rows in source:
        first.append(first[-1] + len(rows))
    return ([n for n, _p, _r in source], [p for _n, p, _r in source], first,
            b"".join(d for _n, _p, rows in source for d, _s in rows), [s for _n, _p, rows in source for _d, s in rows])
