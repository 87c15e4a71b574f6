"""FILE_BLOCK runs in which a digest forges a message start, every way the
wire format allows, and the Python scan that says where whole messages stand.

Test helper: no GPU, no call into the library; what a run parses to comes
from recv_expect.expected (wire.Parser) alone.

A message is TAG (11 bytes, "FILE_BLOCK\\n") + 20 digest bytes + "\\n" + a size
field + "\\n".  Take message A with the tag at offset j of its digest, j in
0..9, and a size of d digits, followed by message B:

    byte  0        11       11+j      31  32    32+d  33+d     44+d      64+d
    A     TAG      digest.. TAG ..    \\n  size  \\n
    B                                                 TAG      digest..  \\n size \\n
    forged                  TAG  digest (20 bytes)   \\n size \\n
                            ^p = 11 + j              ^42 + j

The forged message at p needs a newline at byte 42 + j, then a valid size
field and its newline.  Bytes 32 .. 42 + d are A's size, its newline and the
first ten bytes of B's tag, none of which is a newline but byte 32 + d < 42 +
j.  So the forged digest's newline is

  family 1   B's own tag newline, byte 43 + d: j = d + 1 (8 forms), and the
             forged size field is the start of B's digest;
  family 2   a byte of B's digest, j >= d + 2 (28 forms): B's digest holds a
             newline at offset j - d - 2, then the forged size field.

Any other (j, d) cannot forge a start: `forge` returns None for it.
"""
from recv_expect import expected, message
from syncfast_amd import wire

TAG = b"FILE_BLOCK\n"
# the longest message, 11 + 20 + 1 + 15 + 1 = 48 (kMaxMessage in sf_wire_parse.hpp): it follows the
# parser's limit on a size field
MAX_MESSAGE = len(TAG) + 20 + 1 + wire.SIZE_MAX + 1
FILL = 0xAA  # digest bytes that are no part of any tag, digit or newline


def forge(j, d, forged_size=b"7", b_size=99):
    """(run = A + B, p, family) with a whole message at p = 11 + j inside A,
    or None when (j, d) has no such run.  A's size has d digits."""
    if not (0 <= j <= 9 and 1 <= d <= 10):
        return None
    if j == d + 1:
        family, at = 1, 0          # the forged size field opens B's digest
    elif j >= d + 2:
        family, at = 2, j - d - 1  # after a newline at offset j - d - 2 of B's digest
    else:
        return None
    digest_a = bytes([FILL]) * j + TAG + bytes([FILL]) * (9 - j)
    size_a = int("1" + "0" * (d - 1)) + 3 if d > 1 else 3
    a = message(digest_a, size_a)
    assert len(a) == 33 + d
    head = (bytes([FILL]) * (at - 1) + b"\n" if family == 2 else b"") + forged_size + b"\n"
    assert len(head) <= 20
    digest_b = head + bytes([FILL]) * (20 - len(head))
    return a + message(digest_b, b_size), 11 + j, family


def forms():
    """[(j, d, family)] of every forged form: 8 of family 1, 28 of family 2."""
    out = []
    for j in range(10):
        for d in range(1, 11):
            f = forge(j, d)
            if f is not None:
                out.append((j, d, f[2]))
    return out


def message_at(run, q):
    """The length of the whole FILE_BLOCK message the parser reads at q, or 0."""
    if run[q:q + len(TAG)] != TAG:  # the parser's first line must be the command
        return 0
    # at most one message is read: two need 2 * 34 = 68 bytes
    digests, _sizes, consumed, _stop = expected(run[q:q + MAX_MESSAGE])
    return consumed if digests else 0


def candidates(run):
    """{q: length} of every position at which a whole message stands."""
    out = {}
    q = run.find(TAG)
    while q >= 0:
        n = message_at(run, q)
        if n:
            out[q] = n
        q = run.find(TAG, q + 1)
    return out


def forged_start_in_chain(run):
    """Whether a candidate lies strictly inside the last message of the chain
    from byte 0: the chain is the candidates that follow one another with no
    candidate inside them; it ends at the first that has one inside (True) or
    is not followed by a candidate (False).  sf_recv.hip parses on the host
    exactly when this holds."""
    cand = candidates(run)
    q = 0
    while q in cand:
        n = cand[q]
        if any(q < c < q + n for c in cand):
            return True
        if q + n not in cand:
            return False
        q += n
    return False


def honest_prefix(total, rng):
    """Honest messages of 34 to 43 bytes (sizes of 1 to 10 digits, random
    digests) that take exactly `total` bytes; total = 0 or >= 136, or a sum
    of such lengths."""
    if total == 0:
        return b""
    m = -(-total // 43)
    assert 34 * m <= total <= 43 * m, total
    lens = [34] * m
    for k in range(total - 34 * m):
        lens[k % m] += 1
    out = []
    for n in lens:
        digits = n - 33
        lo = 10 ** (digits - 1) if digits > 1 else 0
        size = int(rng.integers(lo, min(10 ** digits, 1 << 32)))
        out.append(message(rng.integers(0, 256, 20, dtype="uint8").tobytes(), size))
    run = b"".join(out)
    assert len(run) == total
    return run


_FRAGMENTS = [TAG, TAG[:10], TAG[1:], b"FILE_", b"BLOCK\n", b"K\n", b"F", b"\n", b"+", b"FILE_END\n"[:6]] + \
    [bytes([0x30 + k]) for k in range(10)]


def hostile_digest(rng):
    """20 bytes, most of them newlines, 'F', digits, '+' and pieces of the tag."""
    out = bytearray()
    while len(out) < 20:
        if rng.random() < 0.85:
            out += _FRAGMENTS[int(rng.integers(0, len(_FRAGMENTS)))]
        else:
            out.append(int(rng.integers(0, 256)))
    return bytes(out[:20])


def hostile_size_field(rng):
    """A size field in one of the forms the parser accepts, 1 to 15 bytes:
    an optional '+', leading zeros, a value below 2^32."""
    value = str(int(rng.integers(0, 1 << 32)) >> int(rng.integers(0, 32))).encode()
    plus = b"+" if rng.random() < 0.3 else b""
    room = 15 - len(plus) - len(value)
    zeros = b"0" * int(rng.integers(0, room + 1)) if rng.random() < 0.5 else b""
    return plus + zeros + value


def hostile_run(n, rng):
    return b"".join(message(hostile_digest(rng), hostile_size_field(rng)) for _ in range(n))
