"""What a GetFiles stream of many files must parse to, from
syncfast_amd.wire.Parser and the sink's rule (src/sync/fs.rs:449-500) alone
(shared by test_wire_files.py and the test_gpu_recv_files*.py files; no code
under test)."""
from collections import namedtuple

from syncfast_amd import wire

END, INCOMPLETE, OTHER, MALFORMED, UNEXPECTED = 0, 1, 2, 3, 4
OTHERS = (b"FILE_ENTRY", b"END_FILES", b"GET_FILE", b"GET_BLOCK", b"BLOCK_DATA", b"COMPLETE")
KINDS = {"FileStart": 1, "FileBlock": 2, "FileEnd": 3}  # as the library numbers them
NO_NAME = (1 << 64) - 1

Expected = namedtuple("Expected", "digests sizes offsets block_file name_at name_len first file_size consumed stop "
                                  "open end_offset messages")


def start(name: bytes) -> bytes:
    return wire.write_message("FileStart", name)


def block(digest: bytes, size) -> bytes:
    """One FILE_BLOCK message; size an int or the raw bytes of a size field."""
    if isinstance(size, int):
        return wire.write_message("FileBlock", digest, size)
    return b"FILE_BLOCK\n" + digest + b"\n" + size + b"\n"


FILE_END = wire.write_message("FileEnd")


def _parser(stream: bytes):
    p = wire.Parser()
    p._buf = bytearray(stream)
    return p


def _at(p, pos):
    """What stands at pos: ((kind, *fields), end) for a whole message of the
    three kinds, else the stop class."""
    if pos == len(p._buf):
        return END
    try:
        line = p._line(pos, wire.COMMAND_MAX, "Unterminated command")
        if line is None:
            return INCOMPLETE
        if line[0] in OTHERS:  # their complete command line, whatever follows it
            return OTHER
        r = p._one(pos)  # one of the three, or an unknown command (raises)
    except wire.ProtocolError:
        return MALFORMED
    return INCOMPLETE if r is None else r


def expected(stream: bytes, open: bool = False, base: int = 0) -> Expected:
    """Every output of sf_receive_files_device's contract for ``stream``
    received in state (open, base): the reference parser's messages from byte
    0, taken while the sink's state takes them."""
    p = _parser(stream)
    digests, sizes, offsets, block_file, name_at, name_len, first, file_size = ([] for _ in range(8))
    run = base if open else 0
    if open:
        name_at.append(NO_NAME), name_len.append(0), first.append(0), file_size.append(run)
    pos = messages = 0
    while True:
        r = _at(p, pos)
        if isinstance(r, int):
            stop = r
            break
        msg, end = r
        if (msg[0] == "FileStart") == open:  # FILE_START only with no file open, the others only with one
            stop = UNEXPECTED
            break
        if msg[0] == "FileStart":
            name_at.append(pos + 11), name_len.append(len(msg[1])), first.append(len(sizes)), file_size.append(0)
            assert stream[pos + 11:pos + 11 + len(msg[1])] == msg[1]
            open, run = True, 0
        elif msg[0] == "FileBlock":
            digests.append(msg[1].bytes), sizes.append(msg[2]), offsets.append(run), block_file.append(len(first) - 1)
            run += msg[2]
            file_size[-1] = run
        else:
            open = False
        pos, messages = end, messages + 1
    first.append(len(sizes))
    return Expected(digests, sizes, offsets, block_file, name_at, name_len, first, file_size, pos, stop, open,
                    run if file_size else base, messages)


def candidates(stream: bytes):
    """[(position, length, kind)] of every position where ``Parser._one``
    reads a whole message of the three kinds -- brute force over the
    positions that hold an 'F' (all three commands begin with one)."""
    p, out = _parser(stream), []
    pos = stream.find(b"F")
    while pos >= 0:
        try:
            r = p._one(pos)
        except wire.ProtocolError:
            r = None
        if r is not None and r[0][0] in KINDS:
            out.append((pos, r[1] - pos, KINDS[r[0][0]]))
        pos = stream.find(b"F", pos + 1)
    return out


def needs_fallback(stream: bytes, open: bool = False) -> bool:
    """Whether a candidate lies inside the last message that chains from
    byte 0 in the sink's order: the one case the device hands to the host."""
    cand = candidates(stream)
    at = {p: k for p, _n, k in cand}
    if 0 not in at or ((at[0] == 1) == open):
        return False
    for i, (p, n, k) in enumerate(cand):
        inside = i + 1 < len(cand) and cand[i + 1][0] < p + n
        nxt = at.get(p + n)
        good = nxt is not None and ((nxt == 1) == (k == 3))  # FILE_START exactly after FILE_END
        if inside or not good:
            return inside
    return False
