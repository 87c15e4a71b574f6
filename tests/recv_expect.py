"""What a FILE_BLOCK run must parse to, from syncfast_amd.wire.Parser alone
(shared by test_wire_parse.py and test_gpu_recv.py; no code under test)."""
from syncfast_amd import wire

END, INCOMPLETE, OTHER, MALFORMED = 0, 1, 2, 3
OTHERS = (b"FILE_ENTRY", b"END_FILES", b"GET_FILE", b"FILE_START", b"FILE_END", b"GET_BLOCK", b"BLOCK_DATA",
          b"COMPLETE")


def expected(run: bytes):
    """(digests, sizes, consumed, stop): the FILE_BLOCK messages the reference
    parser reads from byte 0 until something else stands there, the bytes
    they take and the class of what stops it: the buffer's end, a message
    that more bytes could complete, another command's complete line (whatever
    follows it) or bytes the parser raises on."""
    p = wire.Parser()
    p._buf = bytearray(run)
    digests, sizes, pos = [], [], 0
    while True:
        if pos == len(run):
            return digests, sizes, pos, END
        try:
            line = p._line(pos, wire.COMMAND_MAX, "Unterminated command")
            if line is None:
                return digests, sizes, pos, INCOMPLETE
            if line[0] in OTHERS:
                return digests, sizes, pos, OTHER
            r = p._one(pos)  # FILE_BLOCK, or an unknown command (raises)
        except wire.ProtocolError:
            return digests, sizes, pos, MALFORMED
        if r is None:
            return digests, sizes, pos, INCOMPLETE
        (kind, digest, size), pos = r
        assert kind == "FileBlock"
        digests.append(digest.bytes)
        sizes.append(size)


def message(digest: bytes, size) -> bytes:
    """One FILE_BLOCK message; size an int (write_message's form) or the raw
    bytes of a size field."""
    if isinstance(size, int):
        return wire.write_message("FileBlock", digest, size)
    return b"FILE_BLOCK\n" + digest + b"\n" + size + b"\n"
