"""What a files list must parse to and what its runs must hold, from
syncfast_amd.wire.Parser and wire.write_message alone (shared by
test_wire_entries.py, test_file_list_capi.py and the test_gpu_file_*.py files;
no code under test)."""
from collections import namedtuple

from syncfast_amd import wire

END, INCOMPLETE, OTHER, MALFORMED, END_FILES = 0, 1, 2, 3, 5
OTHERS = (b"GET_FILE", b"FILE_START", b"FILE_END", b"GET_BLOCK", b"FILE_BLOCK", b"BLOCK_DATA", b"COMPLETE")
END_FILES_MSG = wire.write_message("EndFiles")

Expected = namedtuple("Expected", "name_at name_len sizes hashes names consumed stop bad_name")


def entry(name: bytes, size, digest: bytes) -> bytes:
    """One FILE_ENTRY message; size an int or the raw bytes of a size field."""
    if isinstance(size, int):
        return wire.write_message("FileEntry", name, size, digest)
    return b"FILE_ENTRY\n" + name + b"\n" + size + b"\n" + digest + b"\n"


def get_file(name: bytes) -> bytes:
    return wire.write_message("GetFile", name)


def utf8_ok(name: bytes) -> bool:
    """Rust's String::from_utf8 accepts exactly what Python's strict decoder
    does: no overlong form, no surrogate, nothing above U+10FFFF."""
    try:
        name.decode("utf-8")
    except UnicodeDecodeError:
        return False
    return True


def _parser(stream: bytes):
    p = wire.Parser()
    p._buf = bytearray(stream)
    return p


def _at(p, pos):
    """What stands at pos: ((kind, *fields), end) for a whole FILE_ENTRY or
    END_FILES, else the stop class."""
    if pos == len(p._buf):
        return END
    try:
        line = p._line(pos, wire.COMMAND_MAX, "Unterminated command")
        if line is None:
            return INCOMPLETE
        if line[0] in OTHERS:  # their complete command line, whatever follows it
            return OTHER
        r = p._one(pos)  # FILE_ENTRY, END_FILES, or an unknown command (raises)
    except wire.ProtocolError:
        return MALFORMED
    return INCOMPLETE if r is None else r


def expected(stream: bytes) -> Expected:
    """Every parse output of sf_receive_file_entries_device's contract for
    ``stream``: the reference parser's FILE_ENTRY messages from byte 0."""
    p = _parser(stream)
    name_at, name_len, sizes, hashes, names = [], [], [], [], []
    pos, bad = 0, None
    while True:
        r = _at(p, pos)
        if isinstance(r, int):
            stop = r
            break
        msg, end = r
        if msg[0] == "EndFiles":
            pos, stop = end, END_FILES
            break
        _kind, name, size, digest = msg
        assert stream[pos + 11:pos + 11 + len(name)] == name
        if bad is None and not utf8_ok(name):
            bad = len(names)
        name_at.append(pos + 11), name_len.append(len(name)), sizes.append(size), hashes.append(digest.bytes)
        names.append(name)
        pos = end
    return Expected(name_at, name_len, sizes, hashes, names, pos, stop, bad)


def candidates(stream: bytes):
    """[(position, length, name length)] of every position where
    ``Parser._one`` reads a whole FILE_ENTRY: every position is tried."""
    p, out = _parser(stream), []
    for pos in range(len(stream)):
        try:
            r = p._one(pos)
        except wire.ProtocolError:
            r = None
        if r is not None and r[0][0] == "FileEntry":
            out.append((pos, r[1] - pos, len(r[0][1])))
    return out


def needs_fallback(stream: bytes) -> bool:
    """Whether a candidate lies inside the last entry that chains from byte
    0: the one case the device hands to the host."""
    cand = candidates(stream)
    at = {p for p, _n, _l in cand}
    if 0 not in at:
        return False
    for i, (p, n, _l) in enumerate(cand):
        inside = i + 1 < len(cand) and cand[i + 1][0] < p + n
        if inside or p + n not in at:
            return inside
    return False


def entries_run(files, end_files: bool = True) -> bytes:
    """The list of ``files`` = [(name, size, hash)] as write_message gives it."""
    out = b"".join(wire.write_message("FileEntry", n, s, h) for n, s, h in files)
    return out + (END_FILES_MSG if end_files else b"")


def get_files_run(names) -> bytes:
    return b"".join(get_file(n) for n in names)


def carries(name: bytes, size: int) -> bool:
    """Whether the protocol can carry a file: the receiver reads the name with
    read_line(FILENAME_MAX) and the size with read_line(SIZE_MAX)."""
    return len(name) <= wire.FILENAME_MAX and b"\n" not in name and 0 <= size < 10 ** wire.SIZE_MAX
