"""CPU: the database half of Index.receive_block_data (Index.apply_block_data,
from parsed arrays, no GPU) against the reference's per-message loop of the
sink's GetBlocks state (src/sync/fs.rs:505-510: list_block_locations ->
mark_block_present) run on a second Index, table for table."""
import hashlib
from pathlib import PurePath

from syncfast_amd.digest import HashDigest
from syncfast_amd.index import Index

NOW = 1_700_000_000_000_000_000


def _dest(blocks):
    """A destination index that waits for ``blocks``: {temp file name:
    [(payload, offset)]}, every row recorded missing."""
    idx = Index.open_in_memory()
    for name, rows in blocks.items():
        file_id = idx.add_temp_file(name)
        for payload, offset in rows:
            idx.add_missing_block(HashDigest(hashlib.sha1(payload).digest()), file_id, offset, len(payload))
    idx.commit()
    return idx


def _reference_loop(idx, messages):
    """fs.rs:505-510 per message: every location of the hash is written and
    marked present."""
    writes = []
    for digest, data_start, size in messages:
        h = HashDigest(digest)
        for file_id, name, offset, _size in idx.list_block_locations(h):
            writes.append((name, offset, data_start, size))
            idx.mark_block_present(file_id, h, offset)
    return writes


def _tables(idx):
    return (idx.db.execute("SELECT file_id, name, size, blocks_hash, temporary FROM files ORDER BY file_id;").fetchall(),
            idx.db.execute("SELECT file_id, hash, offset, size, present FROM blocks ORDER BY file_id, offset;").fetchall())


A, B, C = b"alpha" * 100, b"beta" * 7, b""
LAYOUT = {"one": [(A, 0), (B, 500), (A, 507)], "dir/two": [(B, 0), (A, 28), (C, 528)]}


def _messages(payloads):
    """(digest, data_start, size) as a parse would give them: payloads back
    to back behind 35-byte headers."""
    out, at = [], 0
    for p in payloads:
        out.append((hashlib.sha1(p).digest(), at + 35, len(p)))
        at += 35 + len(p) + 1
    return out


def _apply(idx, messages, ok=None):
    return idx.apply_block_data([m[0] for m in messages], [m[2] for m in messages], [m[1] for m in messages], ok)


def test_same_hash_wanted_at_two_locations_in_two_temp_files():
    got, ref = _dest(LAYOUT), _dest(LAYOUT)
    msgs = _messages([A, B, C])
    writes, rejected = _apply(got, msgs, [1, 1, 1])
    assert writes == _reference_loop(ref, msgs) and rejected == []
    assert _tables(got) == _tables(ref)
    # A is wanted three times in two files, B twice, the empty block once
    assert [(str(w[0]), w[1]) for w in writes if w[2] == msgs[0][1]] == \
        [(".syncfast_tmp_one", 0), (".syncfast_tmp_one", 507), ("dir/.syncfast_tmp_two", 28)]
    assert len(writes) == 6 and all(isinstance(w[0], PurePath) for w in writes)
    assert got.list_missing_blocks() == []
    # without ok every message is taken, as the reference takes it
    third = _dest(LAYOUT)
    assert _apply(third, msgs) == (writes, []) and _tables(third) == _tables(ref)


def test_a_hash_received_twice():
    got, ref = _dest(LAYOUT), _dest(LAYOUT)
    msgs = _messages([B, A, B])
    writes, rejected = _apply(got, msgs, [1, 1, 1])
    assert writes == _reference_loop(ref, msgs) and rejected == []
    assert _tables(got) == _tables(ref)
    assert sum(1 for w in writes if w[3] == len(B)) == 4  # both locations, for each of the two messages
    assert got.list_missing_blocks() == [HashDigest(hashlib.sha1(C).digest())]


def test_a_rejected_message_leaves_its_rows_missing():
    got, ref = _dest(LAYOUT), _dest(LAYOUT)
    msgs = _messages([A, B, C])
    writes, rejected = _apply(got, msgs, [1, 0, 1])
    assert rejected == [HashDigest(hashlib.sha1(B).digest())]
    assert writes == _reference_loop(ref, [msgs[0], msgs[2]])  # the loop over the verified messages alone
    assert _tables(got) == _tables(ref)
    assert not any(w[3] == len(B) for w in writes)
    assert got.list_missing_blocks() == [HashDigest(hashlib.sha1(B).digest())] * 2
    present = dict(got.db.execute("SELECT hash, SUM(present) FROM blocks GROUP BY hash;").fetchall())
    assert present[hashlib.sha1(B).hexdigest()] == 0 and present[hashlib.sha1(A).hexdigest()] == 3
    # a digest nobody asked for: nothing to write, nothing rejected
    assert _apply(got, _messages([b"unasked"]), [1]) == ([], [])
