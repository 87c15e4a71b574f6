"""What the sending side must produce, from syncfast_amd.wire (write_message,
Parser) alone (shared by test_block_data_write.py and
test_gpu_block_data_send.py; no code under test): the parse of a GET_BLOCK
run, and hostile runs to feed it."""
from syncfast_amd import wire

END, INCOMPLETE, OTHER, MALFORMED = 0, 1, 2, 3
OTHERS = (b"FILE_ENTRY", b"END_FILES", b"GET_FILE", b"FILE_START", b"FILE_END", b"FILE_BLOCK", b"BLOCK_DATA",
          b"COMPLETE")
GET = 31  # bytes of a GET_BLOCK message


def get_block(digest: bytes) -> bytes:
    return wire.write_message("GetBlock", digest)


def expected_requests(run: bytes):
    """(digests, consumed, stop): the GetBlock messages the reference parser
    reads from byte 0 until something else stands there, the bytes they take
    and the class of what stops it -- the buffer's end, bytes that more could
    complete, another command's complete line, bytes the parser raises on."""
    p = wire.Parser()
    p._buf = bytearray(run)
    digests, pos = [], 0
    while True:
        if pos == len(run):
            return digests, pos, END
        try:
            line = p._line(pos, wire.COMMAND_MAX, "Unterminated command")
            if line is None:
                return digests, pos, INCOMPLETE
            if line[0] in OTHERS:
                return digests, pos, OTHER
            r = p._one(pos)  # GET_BLOCK, or an unknown command (raises)
            if r is None:
                return digests, pos, INCOMPLETE
        except wire.ProtocolError:
            return digests, pos, MALFORMED
        (kind, digest), end = r
        assert kind == "GetBlock" and end == pos + GET
        digests.append(digest.bytes)
        pos = end


def hostile_digest(rng) -> bytes:
    kind = rng.randrange(6)
    if kind == 0:
        return b"GET_BLOCK\nGET_BLOCK\n"
    if kind == 1:
        return b"\n" * 20
    if kind == 2:
        return (b"COMPLETE\n" * 3)[:20]
    if kind == 3:
        return b"\nGET_BLOCK\n" + rng.randbytes(9)
    return rng.randbytes(20)


TAILS = [b"", b"", b"COMPLETE\n", b"COMPLETE\n", b"FILE_END\nrest", b"GET_FILE\n", b"BLOCK_DATA\n" + bytes(20) + b"\n0\n\n",
         b"XYZ\n", b"Z" * 25, b"Z" * 12, b"GET_BLOCK\n" + bytes(20) + b"x", b"GET_BLOCK\n" + bytes(20), b"GET_BLOCK",
         b"GET_BLOCK \n" + bytes(30), b"get_block\n" + bytes(21), b"\n", b"GET_BLOC\n"]


def hostile_requests(rng) -> bytes:
    """Requests with hostile digests, followed by something else or cut; now
    and then one of them spoilt in the middle of the run."""
    run = b"".join(get_block(hostile_digest(rng)) for _ in range(rng.randrange(0, 9)))
    if run and rng.random() < 0.4:
        at = rng.randrange(len(run))
        run = run[:at] + bytes([rng.choice([0, 10, 71, 255])]) + run[at + 1:]
    run += rng.choice(TAILS)
    return run[:rng.randrange(0, len(run) + 1)] if rng.random() < 0.3 else run
