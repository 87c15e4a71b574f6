"""Expected values for a whole GetFiles answer (sf_wire_files_device,
syncfast_amd/csrc/sf_wire_send_files.hpp): test helper, a plain module imported
like want_expect.py.  A case is a list of files, each (name bytes, [(digest
bytes, size)]).  The expected stream is wire.write_message's, message after
message, and the places of the messages are found by walking it; nothing here
comes from the code under test."""
import random
from pathlib import PurePath

from syncfast_amd import wire
from syncfast_amd.digest import HashDigest
from syncfast_amd.index import Index
from syncfast_amd.timestamp import DateTimeUtc

NO_FILE = (1 << 64) - 1
SIZES = (0, 9, 10, 99999, 4294967295)
HOSTILE = (b"FILE_END\nFILE_START\n", b"\n" * 20, b"FILE_BLOCK\n" + b"\n" * 9)


def expected(files):
    """(stream, starts, ends, blocks): write_message over the files, and where
    each FILE_START, FILE_END and FILE_BLOCK begins in it."""
    out, starts, ends, blocks = bytearray(), [], [], []
    for name, rows in files:
        starts.append(len(out))
        out += wire.write_message("FileStart", name)
        for digest, size in rows:
            blocks.append(len(out))
            out += wire.write_message("FileBlock", digest, size)
        ends.append(len(out))
        out += wire.write_message("FileEnd")
    return bytes(out), starts, ends, blocks


def csr(files):
    """(digests, sizes, first, names, name_at): the arrays of the call."""
    digests = [d for _n, rows in files for d, _s in rows]
    sizes = [s for _n, rows in files for _d, s in rows]
    first, name_at = [0], [0]
    for name, rows in files:
        first.append(first[-1] + len(rows))
        name_at.append(name_at[-1] + len(name))
    return digests, sizes, first, b"".join(n for n, _r in files), name_at


def parse_back(stream):
    """The files wire.Parser reads from the stream, in a case's form."""
    files = []
    for msg in wire.Parser().receive(stream):
        if msg[0] == "FileStart":
            files.append((msg[1], []))
        elif msg[0] == "FileBlock":
            files[-1][1].append((msg[1].bytes, msg[2]))
        else:
            assert msg == ("FileEnd",), msg
    return files


def first_bad_file(first, names, name_at, n_blocks):
    """The rule include/syncfast_amd.h states, file by file: the first file
    whose entries do not hold, NO_FILE when all do."""
    m = len(first) - 1
    for f in range(m):
        ok = first[f] <= first[f + 1] and name_at[f] <= name_at[f + 1] <= name_at[m]
        ok = ok and (f > 0 or (first[0] == 0 and name_at[0] == 0)) and (f + 1 < m or first[m] == n_blocks)
        if ok:
            name = names[name_at[f]:name_at[f + 1]]
            ok = len(name) == name_at[f + 1] - name_at[f] <= wire.FILENAME_MAX and b"\n" not in name
        if not ok:
            return f
    return NO_FILE


def _digest(rng):
    return rng.choice(HOSTILE)[:20].ljust(20, b"\n") if rng.random() < 0.05 else rng.randbytes(20)


def _name(rng, length=None):
    length = rng.choice((0, 1, 5, 12, 40, 99, 100)) if length is None else length
    return bytes(rng.choice(b"abcxyz/._ -\r\0\xff") for _ in range(length))


def _size(rng):
    return rng.choice(SIZES) if rng.random() < 0.2 else rng.randrange(1 << rng.randrange(1, 33))


def _rows(rng, n):
    return [(_digest(rng), _size(rng)) for _ in range(n)]


def table():
    """The fixed table: {name: case}."""
    rng = random.Random(20)
    rows = lambda n: _rows(rng, n)  # noqa: E731
    return {
        "no files": [],
        "one empty file": [(b"a", [])],
        "three empty files": [(b"a", []), (b"dir/b", []), (b"c", [])],
        "empty first and last": [(b"first", []), (b"mid", rows(3)), (b"", []), (b"mid2", rows(2)), (b"last", [])],
        "name lengths": [(_name(rng, n), rows(2)) for n in (0, 1, 99, 100)],
        "sizes": [(b"sizes", [(_digest(rng), s) for s in SIZES]), (b"again", [(HOSTILE[0][:20], s) for s in SIZES])],
        "a forged end in a name": [(b"x/FILE_END", rows(2)), (b"FILE_END", []), (b"FILE_BLOCK", rows(1))],
    }


def random_files(rng, max_files=40, max_blocks=70):
    return [(_name(rng), _rows(rng, rng.choice((0, 0, 1, 2, rng.randrange(max_blocks + 1)))))
            for _ in range(rng.randrange(max_files + 1))]


def files_with_messages(rng, total):
    """A random case of exactly `total` messages (blocks + 2 per file)."""
    files = []
    while total >= 2:
        n = min(total - 2, rng.choice((0, 1, 3, rng.randrange(80))))
        if total - 2 - n == 1:  # one message cannot be a file
            n += 1
        files.append((_name(rng), _rows(rng, n)))
        total -= n + 2
    assert total == 0
    return files


# ------------------------------------------------ Index.serve_get_files

def source_index(rng):
    """An index with an empty file, a repeated digest (within a file and
    across files) and a temporary file; {name: rows as added}."""
    idx = Index.open_in_memory()
    twice = HashDigest(rng.randbytes(20))
    added = {}
    for k, (name, n) in enumerate((("a.bin", 5), ("dir/empty", 0), ("dir/b.bin", 70), ("x/FILE_END", 3), ("z", 1))):
        fid, _new = idx.add_file(PurePath(name), DateTimeUtc.from_ns(k + 1))
        at, rows = 0, []
        for j in range(n):
            h = twice if j in (1, 3) else HashDigest(rng.randbytes(20))
            size = rng.choice((1, 9, 10, 99999, rng.randrange(1, 40000)))  # (file, offset) is unique: no empty block
            idx.add_block(h, fid, at, size)
            rows.append((h, at, size))
            at += size
        added[name] = rows
    tid = idx.add_temp_file("incoming.bin")
    idx.add_missing_block(twice, tid, 0, 11)
    idx.commit()
    return idx, added


def reference_loop(idx, names):
    """FsSource's Respond and ListBlocks states, name by name."""
    out, answered = b"", 0
    for name in names:
        found = idx.get_file(PurePath(name.decode()))
        if found is None:
            break  # "Requested file is unknown"
        out += wire.write_message("FileStart", name)
        for h, _offset, size in idx.list_file_blocks(found[0]):
            out += wire.write_message("FileBlock", h, size)
        out += wire.write_message("FileEnd")
        answered += 1
    return out, answered
