"""What a BLOCK_DATA run must parse to, from syncfast_amd.wire.Parser and
hashlib alone (shared by test_wire_data.py and test_gpu_recv_data.py; no code
under test), and the runs those tests feed: honest ones, and payloads that
hold messages of their own."""
import hashlib

from syncfast_amd import wire

END, INCOMPLETE, OTHER, MALFORMED = 0, 1, 2, 3
OTHERS = (b"FILE_ENTRY", b"END_FILES", b"GET_FILE", b"FILE_START", b"FILE_END", b"GET_BLOCK", b"FILE_BLOCK",
          b"COMPLETE")
TAG = b"BLOCK_DATA\n"


def _parser(run):
    p = wire.Parser()
    p._buf = bytearray(run)
    return p


def _need(p, pos):
    """The full length of the message whose whole header stands at pos (its
    payload or end byte is not all there), else 0."""
    r = p._exact(pos + len(TAG), 20, "Unterminated digest")
    if r is None:
        return 0
    r = p._line(r[1], wire.SIZE_MAX, "Unterminated length")
    if r is None:
        return 0
    return r[1] - pos + int(r[0]) + 1


def expected(run: bytes):
    """(digests, sizes, offsets, consumed, stop, need): the BLOCK_DATA
    messages the reference parser reads from byte 0 until something else
    stands there -- claimed digest, payload length, payload offset in the run
    -- the bytes they take, the class of what stops it (the buffer's end, a
    message that more bytes could complete, another command's complete line,
    bytes the parser raises on) and, for a whole header whose payload is not
    all there, that message's full length."""
    p = _parser(run)
    digests, sizes, offsets, pos = [], [], [], 0
    while True:
        if pos == len(run):
            return digests, sizes, offsets, pos, END, 0
        try:
            line = p._line(pos, wire.COMMAND_MAX, "Unterminated command")
            if line is None:
                return digests, sizes, offsets, pos, INCOMPLETE, 0
            if line[0] in OTHERS:
                return digests, sizes, offsets, pos, OTHER, 0
            r = p._one(pos)  # BLOCK_DATA, or an unknown command (raises)
            if r is None:
                return digests, sizes, offsets, pos, INCOMPLETE, _need(p, pos)
        except wire.ProtocolError:
            return digests, sizes, offsets, pos, MALFORMED, 0
        (kind, digest, data), end = r
        assert kind == "BlockData"
        digests.append(digest.bytes)
        sizes.append(len(data))
        offsets.append(end - 1 - len(data))
        pos = end


def candidates(run: bytes):
    """[(position, length)] of every position where the reference parser,
    started there, reads a whole BLOCK_DATA message, in position order."""
    p = _parser(run)
    out, at = [], run.find(TAG)
    while at >= 0:
        try:
            r = p._one(at)
        except wire.ProtocolError:
            r = None
        if r is not None:
            out.append((at, r[1] - at))
        at = run.find(TAG, at + 1)
    return out


def needs_walk(run: bytes) -> bool:
    """The link test over the candidates: a candidate lies inside the first
    one from byte 0 whose successor does not start where it ends."""
    c = candidates(run)
    if not c or c[0][0] != 0:
        return False
    for i, (pos, length) in enumerate(c):
        if i + 1 == len(c) or c[i + 1][0] != pos + length:
            return i + 1 < len(c) and c[i + 1][0] < pos + length
    return False


def message(payload: bytes, digest: bytes = None, length=None, end: bytes = b"\n") -> bytes:
    """One BLOCK_DATA message: the digest its payload hashes to unless one is
    given, the length field write_message writes unless raw bytes are given."""
    digest = hashlib.sha1(payload).digest() if digest is None else digest
    if length is None and end == b"\n":
        return wire.write_message("BlockData", digest, payload)
    field = b"%d" % len(payload) if length is None else length
    return TAG + digest + b"\n" + field + b"\n" + payload + end


def header(length: int, digest: bytes = bytes(20)) -> bytes:
    return TAG + digest + b"\n%d\n" % length


def honest_run(rng, n: int) -> bytes:
    """n messages whose payload sizes cycle through the SHA-1 padding edges,
    with one of 100,000 bytes; seeded random payloads."""
    cycle = [0, 1, 3, 55, 56, 63, 64, 65, 119, 120, 4096, 32768]
    sizes = [cycle[i % len(cycle)] for i in range(n)]
    if n > 2:
        sizes[n // 2] = 100_000
    return b"".join(message(rng.randbytes(s)) for s in sizes)


def nested_payload(rng, depth: int = 0) -> bytes:
    """A payload of the kinds that split a parallel parser from the serial
    one: whole messages (up to three deep), one cut short, a header whose
    length overshoots, tags, newlines, 'B's."""
    kind = rng.randrange(9)
    if kind == 0:
        return rng.randbytes(rng.randrange(0, 80))
    if kind == 1 and depth < 3:
        return b"".join(message(nested_payload(rng, depth + 1)) for _ in range(rng.randrange(1, 3)))
    if kind == 2 and depth < 3:
        m = message(nested_payload(rng, depth + 1))
        return m[:rng.randrange(1, len(m))]
    if kind == 3:
        return header(rng.randrange(0, 300), rng.randbytes(20)) + rng.randbytes(rng.randrange(0, 40))
    if kind == 4:
        return b"\n" * rng.randrange(1, 60)
    if kind == 5:
        return TAG * rng.randrange(1, 6)
    if kind == 6:
        return b"B" * rng.randrange(1, 100)
    if kind == 7 and depth < 3:
        return rng.randbytes(rng.randrange(0, 20)) + message(nested_payload(rng, depth + 1)) + \
            rng.randbytes(rng.randrange(0, 20))
    return rng.randbytes(rng.randrange(0, 20)).replace(b"B", b"b")


def cross(run: bytes, starts, rng) -> bytes:
    """One payload of ``run`` (message starts ``starts``, the run's end last)
    gets a header whose announced length lands exactly on a later message's
    end byte: the bytes are overwritten in place, no message moves."""
    for _ in range(8):
        i = rng.randrange(0, len(starts) - 1)
        h = run.index(b"\n", starts[i] + 32) + 1  # payload start
        room = starts[i + 1] - 1 - h
        target = starts[rng.randrange(i + 1, len(starts))] - 1  # an end byte: its own message's or a later one's
        for digits in range(1, 8):
            forged = header(0)[:-2]  # up to the length field
            length = target - (h + len(forged) + digits + 1)
            if length >= 0 and len(b"%d" % length) == digits and len(forged) + digits + 1 <= room:
                piece = forged + b"%d\n" % length
                return run[:h] + piece + run[h + len(piece):]
    return run


def dense_run(k: int) -> bytes:
    """A hostile run with a candidate every 21 bytes, more than one per 35:
    each tag's newline is the previous header's digest terminator, and every
    length is aimed at the run's last byte.  The parser reads one message,
    the whole run."""
    n = 21 * k + 60
    buf = bytearray(b"x" * (n - 1) + b"\n")
    for i in range(k):
        buf[21 * i:21 * i + 11] = TAG
    for i in range(k):
        p = 21 * i
        for digits in range(1, 10):
            size = n - 1 - p - (32 + digits + 1)
            if size >= 0 and len(b"%d" % size) == digits:
                buf[p + 32:p + 33 + digits] = b"%d\n" % size
                break
    return bytes(buf)


TAILS = [b"", b"", b"FILE_END\n", b"FILE_BLOCK\n" + bytes(20) + b"\n5\n", b"GET_BLOCK\n" + bytes(20) + b"\n",
         b"COMPLETE\n", b"XYZ\n", b"Z" * 25, TAG + bytes(20) + b"x1\n", TAG + bytes(20) + b"\n1a\n", TAG + bytes(20),
         TAG + bytes(20) + b"\n" + b"1" * 16 + b"\n", header(3) + b"abcX", header(50) + b"abc", TAG[:5]]


def hostile_run(rng) -> bytes:
    """Messages with nested, crossing and hostile payloads, the digests
    random (nothing is hashed here), followed by something else or cut."""
    msgs = []
    for _ in range(rng.randrange(0, 7)):
        payload = nested_payload(rng)
        msgs.append(message(payload, rng.randbytes(20), rng.choice([b"%d", b"%d", b"%d", b"+%d", b"00%d"]) % len(payload)))
    run, starts = b"".join(msgs), [0]
    for m in msgs:
        starts.append(starts[-1] + len(m))
    if len(msgs) >= 2 and rng.random() < 0.4:
        run = cross(run, starts, rng)
    run += rng.choice(TAILS)
    return run[:rng.randrange(0, len(run) + 1)] if rng.random() < 0.3 else run
