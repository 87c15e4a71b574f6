"""The scenarios of the files-list phase shared by test_file_list_capi.py (CPU)
and test_gpu_file_entries.py (the same on the device route): one destination
index, copies of it, the lists a source announces, and a transcription of the
reference's sink (src/sync/fs.rs:378-446) over wire.Parser -- no code under
test but Index's long-standing queries."""
import sqlite3
from pathlib import PurePath

from syncfast_amd import wire
from syncfast_amd.digest import HashDigest
from syncfast_amd.index import Index, SyncfastError, untemp_name
from syncfast_amd.timestamp import DateTimeUtc


def H(k: int) -> HashDigest:
    return HashDigest(bytes([k]) * 19 + b"\x01")


def H_last(k: int) -> HashDigest:
    """H(k) with another last byte: a comparison that stops early misses it."""
    return HashDigest(bytes([k]) * 19 + b"\x02")


def H_first(k: int) -> HashDigest:
    return HashDigest(b"\xfe" + bytes([k]) * 18 + b"\x01")


def put(idx: Index, name: str, blocks_hash, temporary: int = 0, size: int = 7) -> int:
    idx.begin()
    fid = idx._put_file(None, PurePath(name), DateTimeUtc.from_ns(0), temporary)
    idx.db.execute("UPDATE files SET size = ?, blocks_hash = ? WHERE file_id = ?;",
                   (size, blocks_hash.to_sql() if blocks_hash is not None else None, fid))
    return fid


def destination(tmp_nontemp: bool = False, leftover: bool = True) -> Index:
    idx = Index.open_in_memory()
    put(idx, "same", H(1))
    put(idx, "changed", H(2))
    put(idx, "dup", H(3))
    put(idx, "dup", H(4))  # the same name again: the first row wins
    put(idx, "nohash", None)
    if leftover:
        put(idx, "dir/.syncfast_tmp_old", None, temporary=1)  # a leftover of an earlier sync
    put(idx, "last_byte", H(5))
    put(idx, "first_byte", H(6))
    put(idx, "dir/é.txt", H(7))
    if tmp_nontemp:
        put(idx, ".syncfast_tmp_x", H(8))  # a non-temporary file that looks like a temp file
    idx.commit()
    return idx


def copy(idx: Index) -> Index:
    idx.commit()
    db = sqlite3.connect(":memory:")
    idx.db.backup(db)
    return Index(db)


def table(idx: Index):
    """Everything of the files table but the time add_temp_file stamps."""
    return idx.db.execute("SELECT file_id, name, size, blocks_hash, temporary FROM files ORDER BY file_id;").fetchall()


def E(name, blocks_hash, size=7) -> bytes:
    return wire.write_message("FileEntry", name if isinstance(name, bytes) else name.encode(), size, blocks_hash)


END = wire.write_message("EndFiles")
BASE = (E("same", H(1)) + E("changed", H(9)) + E("unknown", H(10)) + E("twice", H(11)) + E("twice", H(11))
        + E("dup", H(3)) + E("nohash", H(12)) + E("last_byte", H_last(5)) + E("first_byte", H_first(6))
        + E("dir/é.txt", H(7)) + E("old", H(13)) + END)

NEEDED = [b"changed", b"unknown", b"twice", b"twice", b"nohash", b"last_byte", b"first_byte", b"old"]
# name -> (destination's arguments, the pieces the list arrives in, the names that must come out needed)
SCENARIOS = {
    "base": ({}, [BASE], NEEDED),  # with a leftover temp row: the requests need an explicit pick
    "no_leftover": ({"leftover": False}, [BASE], NEEDED),  # the temp rows are the needed entries in order
    "dup_second_row": ({}, [E("dup", H(4)) + E("same", H(1)) + END], [b"dup"]),
    "nothing_needed": ({"leftover": False}, [E("same", H(1)) + E("dup", H(3)) + END], []),
    "no_end": ({}, [E("same", H(1)) + E("unknown", H(9))], [b"unknown"]),
    "empty_list": ({}, [END], []),
    "spelled_otherwise": ({"leftover": False}, [E("dir//sub/./f", H(9)) + END], [b"dir//sub/./f"]),
    "two_pieces": ({}, [BASE[:len(BASE) // 2 + 3], BASE[len(BASE) // 2 + 3:]], NEEDED),
    "tmp_nontemp": ({"tmp_nontemp": True}, [E("x", H(20)) + E(".syncfast_tmp_x", H(8)) + E("same", H(1)) + END],
                    [b"x", b".syncfast_tmp_x"]),
    "bad_third": ({}, [E("unknown", H(9)) + E("same", H(1)) + E(b"bad\xff", H(10)) + E("later", H(11)) + END],
                  "Bad filename encoding"),
}


def reference_sink(idx: Index, pieces):
    """fs.rs:378-446 message by message over wire.Parser: (n_entries, needed
    names, requests or None).  Raises SyncfastError where the reference
    returns Err."""
    parser, n, needed, requests = wire.Parser(), 0, [], None
    for piece in pieces:
        for msg in parser.receive(piece):
            assert requests is None
            if msg[0] == "FileEntry":
                _kind, name, _size, blocks_hash = msg
                n += 1
                try:
                    path = PurePath(name.decode("utf-8"))
                except UnicodeDecodeError:
                    raise SyncfastError("Bad filename encoding") from None
                found = idx.get_file(path)
                if found is None or found[2] != blocks_hash:
                    idx.add_temp_file(path)
                    needed.append(name)
            else:
                assert msg[0] == "EndFiles"
                requests = b"".join(wire.write_message("GetFile", str(untemp_name(t)).encode())
                                    for t in idx.list_temp_files())
    return n, needed, requests


def run_pieces(idx: Index, pieces, device=None):
    """Index.receive_file_entries over a list that arrives in pieces, the
    unconsumed tail carried: (n_entries, needed, requests as bytes or None,
    [(consumed, stop)] per call)."""
    n, needed, requests, calls, tail = 0, [], None, [], b""
    for piece in pieces:
        data = tail + piece
        k, consumed, stop, names, req = idx.receive_file_entries(data, device=device)
        n, needed, tail = n + k, needed + names, data[consumed:]
        calls.append((consumed, stop))
        if req is not None:
            requests = req if isinstance(req, bytes) else req.bytes()
    return n, needed, requests, calls
