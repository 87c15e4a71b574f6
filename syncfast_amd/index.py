"""Index -- syncfast's library index API with the signatures computed on MI355X.

Mirrors ``pub struct Index`` (/root/reference/src/index.rs:43-736): the same
SQLite schema (src/index.rs:12-38), the same methods and row semantics, so
callers written against the reference (the CLI ``index`` command,
src/main.rs:111-124, and the sync endpoints, src/sync/fs.rs:53-58, 239-248,
463) see identical data.  What changes is the hot path inside
``index_file`` (src/index.rs:610-659): instead of a per-byte CPU loop and one
SQL INSERT per block, the file's bytes go through the C-ABI to the gfx950
SHA-1 kernel and the rows are inserted in one batch.

Chunking -- an explicit choice, there is no default.  The reference cuts
blocks with the third-party cdchunking 0.2.1 ZPAQ chunker (src/index.rs:
622-625); ``ZpaqChunker()`` is that chunker, from the library (its recurrence
reproduces the reference's known-answer test).  ``index_file``
/ ``index_path`` need the chunker the caller chose when opening the index:
  * ``ZpaqChunker(bits=13, max_size=32768)`` -- the reference's blocks with
    nothing handed in: a NativeChunker over sf_zpaq_chunker_ops, on host
    threads or (``device=True``) cut on the GPU;
  * ``BoundaryChunker(fn)`` -- the reference's mode: the boundary function is
    the host chunker (in a Rust drop-in, the cdchunking crate itself), so the
    blocks are the reference's by construction; every block's SHA-1 and the
    ``blocks_hash`` come from the GPU.  ``stream=True`` hands ``fn`` the open
    file (as ``chunker.stream(file)`` reads it) and the library re-reads the
    same open file by windows (sf_index_fd_blocks), so no file is held whole;
  * ``FixedChunker(block_size)`` -- fixed tiling, the BASELINE configs' mode.
    NOT the reference's default blocks: an index built this way only works
    with peers that use the same mode and read a block as its row's
    ``(offset, size)`` bytes (``read_block`` below), never by re-chunking
    from the offset as the reference's ``read_block`` does
    (src/sync/fs.rs:26-40).
The per-block SHA-1, the rows, ``blocks_hash`` and every query are
bit-identical to the reference for the same boundaries.  An ``Index`` opened
without a chunker serves every query but refuses to index.

Timestamps.  ``files.modified`` is a ``DateTime<Utc>`` (``timestamp.DateTimeUtc``):
taken from the open file's metadata with nanosecond precision
(src/index.rs:616-619), written as chrono's RFC 3339 text and compared as a
parsed value in the mtime gate (src/index.rs:183) -- see timestamp.py (parity
with rusqlite's exact writer is unpinned).

Walk order.  ``index_path`` visits directory entries in ``os.listdir`` order,
which is readdir(3) order -- the order Rust's ``read_dir`` yields
(src/index.rs:698) -- so ``file_id``s are assigned as the reference would on
the same filesystem.

Quirks kept on purpose: ``index_file`` leaves ``files.size`` NULL (the
reference never sets it there, so ``list_files`` reports 0, src/index.rs:
376-377); ``compute_blocks_hash`` hashes the digests in the order SQLite
returns them for ``WHERE file_id = ?`` with no ORDER BY (src/index.rs:663-
669), which is insertion (= offset) order.
"""
from __future__ import annotations

import contextlib
import ctypes
import itertools
import logging
import os
import sqlite3
import stat
from pathlib import Path, PurePath
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import host
from ._lib import SF_EAGAIN, ChunkerOps, SfError, same_stamp
from .digest import HashDigest
from .timestamp import DateTimeUtc

log = logging.getLogger("syncfast_amd.index")

# index_file: times a file that keeps changing while it is indexed
# (SF_EAGAIN from the descriptor routes) is opened and indexed again.
CHANGED_RETRIES = 3
# Index.index_path with a NativeChunker: a file this large is cut on the
# chunker's threads and hashed from one read (sf_index_fd_cut), not cut on one
# pool thread among the batch's files (configs[0]'s folder is one 64 MiB file).
LARGE_FILE_BYTES = 64 << 20

SCHEMA = """
    CREATE TABLE files(
        file_id INTEGER NOT NULL PRIMARY KEY,
        name VARCHAR(512) NOT NULL,
        modified DATETIME NOT NULL,
        size INTEGER NULL,
        blocks_hash VARCHAR(40) NULL,
        temporary BOOLEAN NOT NULL
    );
    CREATE INDEX idx_files_name ON files(name);

    CREATE TABLE blocks(
        file_id INTEGER NOT NULL,
        hash VARCHAR(40) NOT NULL,
        offset INTEGER NOT NULL,
        size INTEGER NOT NULL,
        present BOOLEAN NOT NULL,
        PRIMARY KEY(file_id, offset)
    );
    CREATE INDEX idx_blocks_file_id ON blocks(file_id);
    CREATE INDEX idx_blocks_hash ON blocks(hash);
    CREATE INDEX idx_blocks_offset ON blocks(file_id, offset);
    CREATE INDEX idx_blocks_present ON blocks(file_id, present);

    PRAGMA application_id=0x51367457;
    PRAGMA user_version=0x00000000;
"""

# add_block / add_missing_block (src/index.rs:387-408, 433-451): the last
# parameter is the present flag
INSERT_BLOCK = "INSERT INTO blocks(hash, file_id, offset, size, present) VALUES(?, ?, ?, ?, ?);"

INDEX_FILE_NAME = ".syncfast.idx"  # src/index.rs:699, src/main.rs:117
TEMP_PREFIX = ".syncfast_tmp_"     # src/lib.rs:152


class SyncfastError(Exception):
    """Error (src/lib.rs:24-31): Io / Sqlite / BadFilenameEncoding."""


def temp_name(name) -> PurePath:
    """src/lib.rs:147-158: dir/file -> dir/.syncfast_tmp_file."""
    p = PurePath(name)
    if not p.name:
        raise SyncfastError("Invalid path")
    return p.with_name(TEMP_PREFIX + p.name)


def untemp_name(name) -> PurePath:
    """src/lib.rs:160-174."""
    p = PurePath(name)
    if not p.name.startswith(TEMP_PREFIX):
        raise SyncfastError("Not a temporary path")
    return p.with_name(p.name[len(TEMP_PREFIX):])


def _name_str(name) -> str:
    s = str(PurePath(name)) if str(name) != "" else ""
    try:
        s.encode("utf-8")
    except UnicodeEncodeError:
        raise SyncfastError("BadFilenameEncoding") from None
    return s


def _mtime(f) -> DateTimeUtc:
    """``file.metadata()?.modified()?.into()`` (src/index.rs:616-619): the open
    file's mtime, to the nanosecond."""
    return DateTimeUtc.from_ns(os.fstat(f.fileno()).st_mtime_ns)


def _stamp_mtime(stamp) -> DateTimeUtc:
    """``_mtime`` from a stamp (host.file_stamp) of the open file."""
    return DateTimeUtc.from_ns(stamp.mtime_sec * 10**9 + stamp.mtime_nsec)


def _stamp_moved(fd: int, stamp) -> bool:
    """Has the file open on fd changed since `stamp` (host.file_stamp)?"""
    return not same_stamp(host.file_stamp(fd), stamp)


def _now() -> DateTimeUtc:
    """``chrono::Utc::now()`` (src/index.rs:265)."""
    import time
    return DateTimeUtc.from_ns(time.time_ns())


# ----------------------------------------------------------------- chunkers

def _seekable(f) -> bool:
    """A regular file: the native routes map or pread it.  Anything else
    File::open accepts (a FIFO, a character device) is read sequentially from
    the open descriptor (sf_index_fd): a second open of a FIFO would wait for
    another writer."""
    return stat.S_ISREG(os.fstat(f.fileno()).st_mode)


class FixedChunker:
    """Blocks of `block_size` bytes (last one shorter); no empty blocks.

    Not the reference's blocks (those are content-defined, src/index.rs:
    622-625): use it only where every peer indexes the same way and reads a
    block by its row's (offset, size) -- see ``read_block``."""

    def __init__(self, block_size: int):
        if not 0 < block_size <= (32 << 20):
            raise ValueError("block_size must be in (0, 32 MiB]")
        self.block_size = block_size


class BoundaryChunker:
    """Blocks from a host chunker -- the reference's mode (src/index.rs:
    622-625).  fn(data: bytes) -> list of block sizes (positive, summing to
    len(data)); with ``stream=True``, fn(file) reads an open binary file to
    its end (as ``chunker.stream(file)`` does, src/index.rs:625) and returns
    the sizes, and the file is re-read by windows on the library side
    (sf_index_fd_blocks) instead of being held whole.  The signatures are
    computed by the GPU kernel (explicit-block-list entry points)."""

    def __init__(self, fn: Callable, stream: bool = False):
        self.fn = fn
        self.stream = stream


class NativeChunker(BoundaryChunker):
    """The reference's mode with a native chunker: ``ops`` is the address of
    an sf_chunker_ops (create / next / destroy in C: cdchunking's ZPAQ on the
    Rust side; examples/zpaq_standin_ops.c here).  The
    library runs it itself: Index.index_file cuts and hashes a file in one
    call on ``threads`` threads, the file read once (sf_index_fd_cut, the
    one-stream boundaries whatever the thread count); Index.index_path cuts
    the files on its pool (sf_cut_fd, one thread per file) and hashes them
    as batches (sf_index_fds_blocks)."""

    def __init__(self, ops: int, threads: int = 0):
        super().__init__(self._sizes, stream=True)
        self.ops = int(ops)
        self.threads = threads

    def index_fd(self, fd: int, threads: int, stamp):
        """(rows, blocks_hash) of the regular file open on fd: cut on
        ``threads`` threads and hashed from one read (sf_index_fd_cut)."""
        return host.index_fd_cut(fd, self.ops, threads, stamp)

    def _sizes(self, f) -> List[int]:
        if hasattr(f, "fileno"):
            try:
                fd = f.fileno()
            except (OSError, ValueError):  # io.BytesIO: the bytes of one read
                fd = None
            if fd is not None:
                return host.cut_fd(fd, self.ops, 1)[1].tolist()
        return self._cut_bytes(f.read())

    def _cut_bytes(self, raw: bytes) -> List[int]:
        """The chunker over bytes in memory, driven from here through its
        three functions (the one-pass fallback of index_file)."""
        ops = ChunkerOps.from_address(self.ops)
        ch = ops.create(ops.ctx)
        if not ch:
            raise MemoryError("chunker create failed")
        try:
            buf = ctypes.create_string_buffer(raw, len(raw)) if raw else None
            base = ctypes.addressof(buf) if buf is not None else 0
            sizes, start, pos = [], 0, 0
            while pos < len(raw):
                k = ops.next(ch, base + pos, len(raw) - pos)
                if k == 0:
                    break
                pos += k
                sizes.append(pos - start)
                start = pos
            if start < len(raw):
                sizes.append(len(raw) - start)
            return sizes
        finally:
            ops.destroy(ch)


class ZpaqChunker(NativeChunker):
    """The reference's own chunker (cdchunking's ZPAQ, src/index.rs:622-625:
    13 bits, 32 KiB cap), from the library: a NativeChunker over
    sf_zpaq_chunker_ops, so Index.index_file / index_path produce the
    reference's blocks with no chunker handed in.  ``device=True`` cuts on
    the GPU as well: Index.index_file, and index_path's large-file route, go
    through sf_index_fd_zpaq (the file read once, cut and hashed in HBM by
    windows) instead of sf_index_fd_cut's host threads; the rows are the
    same.  With ``device=True`` index_path's smaller files are not cut on
    the host either: each batch goes through one sf_index_fds_zpaq call (every
    file read once, a whole stage of files cut on the device at a time;
    ``max_rounds`` bounds a stage's join launches, and a file that has not
    settled by then is finished by the host cutter inside the call).  The
    default stays on the host route (DESIGN.md 3.7 and 3.17 have the
    measurements)."""

    def __init__(self, bits: int = 13, max_size: int = 32768, device: bool = False, threads: int = 0,
                 max_rounds: int = host.ZPAQ_MAX_ROUNDS):
        self._zops = host.ZpaqOps(bits, max_size)  # kept alive: ops is its address
        super().__init__(self._zops.address, threads)
        self.bits, self.max_size, self.device, self.max_rounds = bits, max_size, device, max_rounds

    def index_fd(self, fd: int, threads: int, stamp):
        """(rows, blocks_hash) of the regular file open on fd, cut and hashed
        in one call on the route this chunker was opened with."""
        if self.device:
            return host.index_fd_zpaq(fd, self.bits, self.max_size, stamp)
        return host.index_fd_cut(fd, self.ops, threads, stamp)


def _sizes_ok(sizes, n: int) -> List[int]:
    sizes = [int(x) for x in sizes]
    if any(x <= 0 for x in sizes) or sum(sizes) != n:
        raise ValueError("boundary function must return positive sizes covering the data")
    return sizes


def _offsets(sizes) -> np.ndarray:
    offs = np.zeros(len(sizes), np.uint64)
    if len(sizes) > 1:
        offs[1:] = np.cumsum(np.asarray(sizes, np.uint64), dtype=np.uint64)[:-1]
    return offs


def _cut_stamped(fn: Callable, f, stamp) -> Optional[List[int]]:
    """The stream chunker ``fn`` over the open, stamped regular file ``f``:
    its block sizes, checked against the stamp's size, or None if the file
    was written while it was cut."""
    sizes = [int(x) for x in fn(f)]
    if sum(sizes) != stamp.size and _stamp_moved(f.fileno(), stamp):
        return None
    return _sizes_ok(sizes, stamp.size)


def _stop_error(stop: int, consumed: int, what: str, refused: bool, why: str) -> None:
    """Raise the wire.ProtocolError for what stopped a device parse after
    ``consumed`` bytes: bytes the parser raises on in ``what``, or a stop the
    caller's state ``refused`` (``why``)."""
    from . import wire
    if stop == wire.SF_WIRE_MALFORMED:
        raise wire.ProtocolError("Malformed %s at byte %d" % (what, consumed))
    if refused:
        raise wire.ProtocolError("%s (byte %d)" % (why, consumed))


class _FdBatch(contextlib.ExitStack):
    """The files of one sf_index_fds_blocks call and the owner of their open
    descriptors: ``entries`` holds (file_id, path, name, open file, stamp,
    future of its cut) in walk order; ``close()`` -- or leaving the batch --
    closes the files and leaves it empty, to be filled again."""

    def __init__(self):
        super().__init__()
        self.entries, self.nbytes = [], 0

    def close(self) -> None:
        super().close()
        self.entries, self.nbytes = [], 0


def read_block(path, offset: int, size: int) -> bytes:
    """The bytes of one block row: `size` bytes at `offset`.

    The sync code's reader (src/sync/fs.rs:26-40) instead re-runs a fresh
    ZPAQ chunker from `offset` and returns the first chunk it cuts; for rows
    of the reference's content-defined blocks that is the same bytes (a
    chunker's state resets at every boundary), for any other
    tiling it is not.  A drop-in that indexes with fixed tiling must replace
    read_block with this ("Fixed tiling"); it is correct for
    both modes."""
    with open(path, "rb") as f:
        f.seek(offset)
        b = f.read(size)
    if len(b) != size:
        raise SyncfastError("No such chunk in file")
    return b


Chunker = object  # FixedChunker | BoundaryChunker


def signatures_of_bytes(data, chunker) -> List[Tuple[int, int, bytes]]:
    """(offset, size, digest) rows of one file's bytes, computed on the GPU."""
    if isinstance(chunker, FixedChunker):
        return host.rows_to_tuples(host.index_buffer(data, chunker.block_size))
    if isinstance(chunker, BoundaryChunker):
        # the boundaries come from the host-side chunker, as the reference's
        # do (src/index.rs:622-625); every block's SHA-1 is computed on the
        # device through the host-memory C-ABI entry (sf_index_buffer_blocks)
        raw = bytes(data)
        import io
        sizes = _sizes_ok(chunker.fn(io.BytesIO(raw)) if chunker.stream else chunker.fn(raw), len(raw))
        if not sizes:
            return []
        rows, _ = host.index_buffer_blocks(raw, _offsets(sizes), np.asarray(sizes, np.uint32))
        return host.rows_to_tuples(rows)
    raise TypeError("unknown chunker")


# -------------------------------------------------------------------- Index

class Index:
    """Index of files and blocks (src/index.rs:43-47)."""

    def __init__(self, db: sqlite3.Connection, chunker=None):
        self.db = db
        self.in_transaction = False
        self.chunker = chunker  # None: queries only; index_file / index_path refuse

    def _need_chunker(self):
        if self.chunker is None:
            raise SyncfastError(
                "this Index was opened without a chunker: pass chunker=BoundaryChunker(fn) for the reference's "
                "content-defined blocks (fn = the host chunker, e.g. cdchunking's ZPAQ 13 / 32 KiB, "
                "src/index.rs:622-625) or chunker=FixedChunker(block_size) for fixed tiling (not the "
                "reference's blocks: peers must index the same way and read blocks by (offset, size))")
        if not isinstance(self.chunker, (FixedChunker, BoundaryChunker)):
            raise TypeError("unknown chunker")

    # -- open / transactions (src/index.rs:51-74, 729-735)
    @classmethod
    def open(cls, filename, chunker=None) -> "Index":
        exists = os.path.exists(filename)
        db = sqlite3.connect(str(filename), isolation_level=None)
        if not exists:
            log.warning("Database doesn't exist, creating tables...")
            db.executescript(SCHEMA)
        return cls(db, chunker)

    @classmethod
    def open_in_memory(cls, chunker=None) -> "Index":
        db = sqlite3.connect(":memory:", isolation_level=None)
        db.executescript(SCHEMA)
        return cls(db, chunker)

    def begin(self) -> None:
        if not self.in_transaction:
            self.db.execute("BEGIN IMMEDIATE;")
            self.in_transaction = True

    def commit(self) -> None:
        if self.in_transaction:
            self.db.execute("COMMIT")
            self.in_transaction = False

    # -- queries (src/index.rs:77-384, 453-607)
    def get_block(self, hash: HashDigest) -> Optional[Tuple[PurePath, int, int]]:
        row = self.db.execute(
            "SELECT files.name, blocks.offset, blocks.size FROM blocks "
            "INNER JOIN files ON blocks.file_id = files.file_id "
            "WHERE blocks.hash = ? AND blocks.present = 1;", (hash.to_sql(),)).fetchone()
        return (PurePath(row[0]), int(row[1]), int(row[2])) if row else None

    def _lookup_table(self):
        """What a device BlockSet of this index is built from: every block row
        in rowid order as (hash, get_block would take it, file name, offset,
        size), their digests as uint8[n, 20] and those flags."""
        rows = self.db.execute(
            "SELECT blocks.hash, blocks.present = 1 AND files.file_id IS NOT NULL, files.name, blocks.offset, "
            "blocks.size FROM blocks LEFT JOIN files ON blocks.file_id = files.file_id "
            "ORDER BY blocks.rowid;").fetchall()
        table = np.frombuffer(bytes.fromhex("".join(r[0] for r in rows)), np.uint8).reshape(-1, 20)
        return rows, table, np.fromiter((bool(r[1]) for r in rows), bool, len(rows))

    def get_blocks(self, hashes: Sequence[HashDigest], device=None) -> List[Optional[Tuple[PurePath, int, int]]]:
        """get_block for a whole list of hashes -- a FILE_BLOCK run as the
        destination receives it (src/sync/fs.rs:461-476) -- answered by one
        device lookup (syncfast_amd.device.BlockSet, sf_block_set_*): the
        index's rows in rowid order go to the GPU as a hash table, and each
        hash gets the row get_block would return (present, joined to a file,
        first in rowid order), or None."""
        from .device import upload
        if not hashes:
            return []
        with self._block_set(device) as (rows, bset):
            q = upload(b"".join(h.bytes for h in hashes), bset.table.device).reshape(-1, 20)
            found = bset.lookup(q).cpu().numpy()
        return [None if r < 0 else (PurePath(rows[r][2]), int(rows[r][3]), int(rows[r][4])) for r in found]

    @contextlib.contextmanager
    def _block_set(self, device):
        """(rows, BlockSet): ``_lookup_table()`` as a lookup on ``device``
        (None: the current one), closed on leaving."""
        import torch

        from .device import BlockSet, device_of
        rows, table, present = self._lookup_table()
        dev = device_of(device)
        with BlockSet(torch.from_numpy(table.copy()).to(dev), torch.from_numpy(present).to(dev)) as bset:
            yield rows, bset

    def _store_received(self, rows, ids, closed, block_file, digests, offsets, sizes, found):
        """The database half of a received FILE_BLOCK stream: block k belongs
        to file ``ids[block_file[k]]`` and was found in row ``found[k]`` of the
        lookup's ``rows`` (or not: < 0).  ONE executemany inserts every block
        with its present flag, ``closed`` = [(file_id, size)] get their size
        and blocks_hash, and the blocks found come back as one copy list per
        entry of ``ids``, [(from_name, from_offset, to_offset, size)]."""
        self.begin()
        self.db.executemany(INSERT_BLOCK, ((bytes(d).hex(), ids[f], int(o), int(s), int(q >= 0))
                                           for d, f, o, s, q in zip(digests, block_file, offsets, sizes, found)))
        for file_id, size in closed:
            self.set_file_size_and_compute_blocks_hash(file_id, size)
        copies = [[] for _ in ids]
        for f, o, s, q in zip(block_file, offsets, sizes, found):
            if q >= 0:
                copies[f].append((PurePath(rows[q][2]), int(rows[q][3]), int(o), int(s)))
        return copies

    def receive_file_blocks(self, file_id: int, data, device=None) -> List[Tuple[PurePath, int, int, int]]:
        """The sink's GetFiles state for one incoming file
        (src/sync/fs.rs:461-498) in one device call.  ``data``: the bytes
        after the file's FILE_START up to and including FILE_END -- its
        FILE_BLOCK run.  The run is parsed, offset and looked up against this
        index's blocks (the table of ``get_blocks``) by one
        ``BlockSet.receive``; every message becomes a row of ``file_id`` in
        one executemany -- present = 1 where get_block finds the block
        (add_block), present = 0 where it does not (add_missing_block) -- and
        the file's size and blocks_hash are set from the run's end offset.

        Returns the copy list [(from_name, from_offset, to_offset, size)]: the
        blocks recorded as present are NOT written by this call (file I/O
        stays out of Index).  The caller copies each of them into the file
        before ``commit()``, as the reference copies each block before its
        add_block.  A run that does not end with FILE_END right after its
        last FILE_BLOCK raises wire.ProtocolError, and nothing is written."""
        from . import wire
        from .device import upload
        data = bytes(data)
        with self._block_set(device) as (rows, bset):
            r = bset.receive(upload(data, bset.table.device))
            digests, sizes, offsets, found = (t.cpu().numpy() for t in r[:4])
        consumed, stop, end_offset = r[4:]
        _stop_error(stop, consumed, "FILE_BLOCK run", stop != wire.SF_WIRE_OTHER or data[consumed:] != b"FILE_END\n",
                    "FILE_BLOCK run does not end with FILE_END")
        return self._store_received(rows, [file_id], [(file_id, end_offset)], [0] * len(found),
                                    digests, offsets, sizes, found)[0]

    def receive_files(self, data, device=None, open_file=None):
        """The sink's GetFiles state (src/sync/fs.rs:449-500) for a buffer of
        MANY files in one device call.  ``data``: received bytes as the wire
        delivers them -- FILE_START, FILE_BLOCKs and FILE_END of one file after
        the other, beginning and ending anywhere.  ``open_file``: the carry of
        the call before, (file_id, offset) of the file that was open when
        ``data`` began, or None.

        One upload, one table (``_lookup_table``), one ``BlockSet`` and one
        ``BlockSet.receive_files`` parse the buffer, give every block its file
        and running offset and look it up.  The names are taken from ``data``
        by the returned spans, decoded as UTF-8 (a bad encoding raises
        wire.ProtocolError, Error::BadFilenameEncoding) and resolved with
        ``get_temp_file`` (an unknown name raises SyncfastError, as
        fs.rs:455-456 does).  Then ONE executemany inserts the rows of all
        files -- present = 1 where the lookup found a row (add_block), else 0
        (add_missing_block) -- and ``set_file_size_and_compute_blocks_hash``
        runs for every closed file, in stream order.

        One lookup against the table at entry is what the reference's
        message-by-message loop gives: get_block returns the first present
        row in (hash, rowid) order, and every row added during the loop has a
        higher rowid than every row of the table at entry -- so a hash found
        at entry is found in the same row later, and a hash not found at entry
        is only ever added as missing.

        Returns (copies, consumed, carry).  copies: {temp file name: [(from_name,
        from_offset, to_offset, size)]} for every file of the call, each list
        in ``receive_file_blocks``' format (the blocks recorded as present are
        NOT written by this call).  consumed: the bytes of the accepted
        messages; an incomplete message after them is the caller's to keep for
        the next call.  carry: (file_id, offset) of the file still open after
        them, or None.  Bytes the parser raises on, a message the sink's state
        does not take, or another command right after the accepted messages
        raise wire.ProtocolError; in every raising case nothing is written."""
        from . import wire
        from .device import upload
        data = bytes(data)
        with self._block_set(device) as (rows, bset):
            r = bset.receive_files(upload(data, bset.table.device), open=open_file is not None,
                                   base_offset=open_file[1] if open_file else 0)
            digests, sizes, offsets, found, block_file, name_at, name_len, _first, file_size = (
                t.cpu().numpy() for t in r[:9])
        _stop_error(r.stop, r.consumed, "GetFiles stream", r.stop in (wire.SF_WIRE_UNEXPECTED, wire.SF_WIRE_OTHER),
                    "Unexpected message from source")
        ids = []
        for at, n in zip(name_at.tolist(), name_len.tolist()):
            if at < 0:  # the file carried in
                ids.append(int(open_file[0]))
                continue
            try:
                name = data[at:at + n].decode("utf-8")
            except UnicodeDecodeError:
                raise wire.ProtocolError("Bad filename encoding (byte %d)" % at) from None
            temp = self.get_temp_file(PurePath(name))
            if temp is None:
                raise SyncfastError("Unknown file %r" % name)
            ids.append(temp[0])
        names = [self.get_file_name(i) for i in ids]
        closed = [(ids[f], int(file_size[f])) for f in range(len(ids) - 1 if r.open else len(ids))]
        copies = {}
        for name, found_here in zip(names, self._store_received(rows, ids, closed, block_file, digests, offsets,
                                                                sizes, found)):
            copies.setdefault(name, []).extend(found_here)
        return copies, r.consumed, ((ids[-1], r.end_offset) if r.open else None)

    def receive_files_assembled(self, data, root, device=None, verify: bool = True):
        """``receive_files`` and the copies it lists in one, with the step
        between them on the device: a WHOLE GetFiles stream -- it begins with a
        FILE_START and ends with a FILE_END, no file carried in or out;
        anything else raises ValueError -- is parsed and looked up as
        ``receive_files`` does, the blocks found become one copy plan
        (``device.plan_copies``: first a query for the local files worth
        loading, then ``assemble.LocalFiles`` loads those below ``root`` with
        ``device.read_fd``, then the plan itself), ``assemble.FileImages`` is
        built from the sections' sizes and filled by ONE ``apply_jobs``, and ONE
        executemany inserts every block with the plan's present flag.

        With ``verify`` every local block is hashed on the device and compared
        with the digest the source announced before it is copied; one that
        differs -- the file was edited after it was indexed -- keeps
        present = 0, so ``get_block_requests`` asks the source for it.  The
        same goes for a block found in a row of another size, in a file now
        shorter than the row says, and in a file that cannot be read (the
        image of a temp file of this same sync among them).  On honest input
        the database ends as ``receive_files`` leaves it.

        Returns (images, plan, consumed): the ``FileImages``, the
        ``device.CopyPlan`` (per-block ``present`` / ``ask`` / ``dst`` and the
        counts) and the bytes of the stream.  Raises what ``receive_files``
        raises; in every raising case nothing is written."""
        from . import wire
        from .assemble import FileImages, LocalFiles
        from . import device as _device
        data = bytes(data)
        if data and not (data.startswith(b"FILE_START\n") and data.endswith(b"FILE_END\n")):
            raise ValueError("receive_files_assembled takes a whole GetFiles stream: no file carried in or out")
        import torch
        with self._block_set(device) as (rows, bset):
            dev = bset.table.device
            r = bset.receive_files(_device.upload(data, dev))
            _stop_error(r.stop, r.consumed, "GetFiles stream", r.stop in (wire.SF_WIRE_UNEXPECTED, wire.SF_WIRE_OTHER),
                        "Unexpected message from source")
            if r.open or r.consumed != len(data):
                raise ValueError("receive_files_assembled takes a whole GetFiles stream: it ends inside a file")
            ids = []
            for at, n in zip(r.name_at.cpu().tolist(), r.name_len.cpu().tolist()):
                try:
                    name = data[at:at + n].decode("utf-8")
                except UnicodeDecodeError:
                    raise wire.ProtocolError("Bad filename encoding (byte %d)" % at) from None
                temp = self.get_temp_file(PurePath(name))
                if temp is None:
                    raise SyncfastError("Unknown file %r" % name)
                ids.append(temp[0])
            names = [self.get_file_name(i) for i in ids]
            if len(set(names)) != len(names):
                raise ValueError("a file is sent twice in one stream: use receive_files")
            file_size = r.file_size.cpu().tolist()
            # the table's rows by the local file that holds each (rows of no file are never found)
            number: dict = {}
            table_file = np.fromiter((number.setdefault(q[2], len(number)) if q[2] is not None else 0 for q in rows),
                                     np.int32, len(rows))
            up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
            table = (up(table_file), up(np.fromiter((q[3] for q in rows), np.int64, len(rows))),
                     up(np.fromiter((q[4] for q in rows), np.uint32, len(rows)).view(np.int32)))
            local = LocalFiles(root, dev).stat(list(number))
            images = FileImages(dict(zip(names, file_size)), dev, root)
            blocks = (r.digests, r.sizes, r.offsets, r.rows, r.block_file, images.bases(names))
            query = _device.plan_copies(*blocks, *table, local.sizes())
            local.load(query.local_jobs.cpu().numpy())
            plan = _device.plan_copies(*blocks, *table, local.sizes(), local.bases(),
                                       local.arena if verify else None)
            images.apply_jobs(local.arena, plan.src_offsets, plan.dst_offsets, plan.sizes)
            digests, sizes, offsets, block_file, present = (
                t.cpu().numpy() for t in (r.digests, r.sizes, r.offsets, r.block_file, plan.present))
        self.begin()
        self.db.executemany(INSERT_BLOCK, ((bytes(d).hex(), ids[f], int(o), int(s), int(p))
                                           for d, f, o, s, p in zip(digests, block_file, offsets, sizes, present)))
        for f, file_id in enumerate(ids):
            self.set_file_size_and_compute_blocks_hash(file_id, int(file_size[f]))
            images.note_present(names[f], offsets[(block_file == f) & (present != 0)])
        return images, plan, r.consumed

    def apply_block_data(self, digests, sizes, data_offsets, ok=None):
        """The database half of ``receive_block_data``, from the parsed arrays
        (no GPU): for each message in order whose payload verified (``ok``
        None: all of them, as the reference takes them) and for every row of
        ``list_block_locations(hash)``, ``mark_block_present`` and one entry
        (name, offset, data_start, size) of the returned write list
        (src/sync/fs.rs:506-510).  Messages that did not verify come back as
        ``rejected`` digests: nothing is listed for them and their rows keep
        present = 0.  Returns (writes, rejected)."""
        writes, rejected = [], []
        for i, d in enumerate(digests):
            h = HashDigest(bytes(d))
            if ok is not None and not ok[i]:
                rejected.append(h)
                continue
            for file_id, name, offset, _size in self.list_block_locations(h):
                self.mark_block_present(file_id, h, offset)
                writes.append((name, offset, int(data_offsets[i]), int(sizes[i])))
        return writes, rejected

    def receive_block_data(self, data, device=None, verify: bool = True):
        """The sink's GetBlocks state (src/sync/fs.rs:503-516) for a whole
        received run of BLOCK_DATA messages in one device call
        (``wire.receive_block_data_device``): the run is parsed as the
        reference parser reads it and, with ``verify``, every payload is
        hashed on the device and compared with the digest it claims -- the
        check the reference leaves out (fs.rs:505-510).

        Returns (writes, rejected, consumed).  writes: for each verified
        message in order and each location that wants its block, (name,
        offset, data_start, size) -- ``data[data_start:data_start + size]``
        belongs at ``offset`` of file ``name``; the rows are marked present,
        the bytes are NOT written by this call (file I/O stays out of Index:
        write them before ``commit()``).  rejected: the digests of messages
        whose payload did not verify; their rows keep present = 0, so
        ``list_missing_blocks`` still asks for them.  consumed: the bytes of
        the whole messages; an incomplete message after them is the caller's
        to keep for the next call.  Bytes the parser raises on, or another
        command, right after the messages raise wire.ProtocolError, and
        nothing is written."""
        _run, digests, sizes, offsets, ok, consumed = self._parse_block_data(data, device, verify)
        writes, rejected = self.apply_block_data(digests.cpu().numpy(), sizes.cpu().numpy(), offsets.cpu().numpy(),
                                                 ok.cpu().numpy() if verify else None)
        return writes, rejected, consumed

    @staticmethod
    def _parse_block_data(data, device, verify: bool):
        """The first step of ``receive_block_data`` and ``place_block_data``:
        the received bytes uploaded, parsed and (``verify``) checked by
        ``wire.receive_block_data_device``.  Returns (run, digests, sizes,
        offsets, ok, consumed), all but the last on the device; raises
        wire.ProtocolError for what may not follow the messages."""
        from . import wire
        from .device import upload
        run = upload(bytes(data), device)
        digests, sizes, offsets, ok, consumed, stop, _need = wire.receive_block_data_device(run, verify=verify)
        _stop_error(stop, consumed, "BLOCK_DATA run", stop == wire.SF_WIRE_OTHER,
                    "Unexpected message in a BLOCK_DATA run")
        return run, digests, sizes, offsets, ok, consumed

    def missing_rows(self) -> List[Tuple[int, int, Optional[PurePath], int, int, HashDigest]]:
        """The rows ``list_missing_blocks`` reads (present = 0), in the same
        rowid order, each with where it lies: (rowid, file_id, name, offset,
        size, hash).  ``name`` is None for a row whose file is gone."""
        rows = self.db.execute(
            "SELECT blocks.rowid, blocks.file_id, files.name, blocks.offset, blocks.size, blocks.hash FROM blocks "
            "LEFT JOIN files ON files.file_id = blocks.file_id WHERE blocks.present = 0 ORDER BY blocks.rowid;")
        return [(int(r[0]), int(r[1]), PurePath(r[2]) if r[2] is not None else None, int(r[3]), int(r[4]),
                 HashDigest.from_sql(r[5])) for r in rows]

    @staticmethod
    def _digest_table(rows, device):
        from .device import upload
        return upload(b"".join(r[5].bytes for r in rows), device).reshape(len(rows), 20)

    def get_block_requests(self, device=None, distinct: bool = False):
        """The GET_BLOCK run the sink sends after the FILE_BLOCK runs
        (src/sync/fs.rs:485-493), built on the device from ``missing_rows()``
        (``device.get_block_requests``): byte for byte the join of
        ``write_message("GetBlock", h)`` over ``list_missing_blocks()``, or
        with ``distinct`` one request per digest.  Returns the run (a
        ``wire.BlockDataRun``: ``bytes()``, ``to_fd(fd)``, ``close()``)."""
        from . import device as _device
        run, _n = _device.get_block_requests(self._digest_table(self.missing_rows(), device), distinct=distinct)
        return run

    def place_block_data(self, data, images, device=None, verify: bool = True):
        """``receive_block_data`` and ``FileImages.apply_writes`` in one, with
        the join between them on the device: the run is parsed and verified
        (``wire.receive_block_data_device``), joined against
        ``missing_rows()`` (``device.place_block_data``: every waiting row
        takes the first verified message with its digest and its size), the
        jobs are copied into ``images`` by one ``images.apply_jobs`` call, and
        the rows that got their block are marked present in one executemany.
        ``images`` must hold an image for every file with a missing row.

        Returns (n_jobs, rejected, consumed, n_left): the rows written,
        ``rejected`` and ``consumed`` as ``receive_block_data`` gives them,
        and the rows still missing (0: ``check_temp_files`` reports nothing
        missing).  Raises what ``receive_block_data`` raises.  Unlike it, a
        payload whose length is not its row's size is not written and the row
        stays missing."""
        import torch

        from . import device as _device
        run, digests, sizes, offsets, ok, consumed = self._parse_block_data(data, device, verify)
        dev = run.device
        rows = self.missing_rows()
        n = len(rows)
        base, length = {}, {}
        for r in rows:
            if r[2] not in base:
                base[r[2]] = images.base(r[2]) if r[2] is not None else None
                length[r[2]] = images.image(r[2]).numel() if r[2] is not None else 0
            if base[r[2]] is None:
                raise KeyError(f"missing row {r[0]} belongs to no file")
            if r[3] + r[4] > length[r[2]]:
                raise ValueError(f"row [{r[3]}, {r[3] + r[4]}) ends past the {length[r[2]]} bytes of {r[2]}")
        row_sizes = torch.from_numpy(np.fromiter((r[4] for r in rows), np.uint32, n).view(np.int32)).to(dev)
        row_dst = torch.from_numpy(np.fromiter((base[r[2]] + r[3] for r in rows), np.int64, n)).to(dev)
        present = torch.zeros(n, dtype=torch.uint8, device=dev)
        src, dst, szs, job_rows, _msgs, _uses, n_left, _mismatch = _device.place_block_data(
            self._digest_table(rows, dev), row_sizes, row_dst, present, digests, sizes, offsets, ok)
        images.apply_jobs(run, src, dst, szs)
        self.begin()
        self.db.executemany("UPDATE blocks SET present = 1 WHERE rowid = ?;",
                            ((rows[k][0],) for k in job_rows.cpu().tolist()))
        rejected = [HashDigest(bytes(d)) for d, good in zip(digests.cpu().numpy(), ok.cpu().numpy()) if not good] \
            if verify else []
        return int(job_rows.numel()), rejected, consumed, n_left

    def serve_get_files(self, names, device=None):
        """The source's ``Respond`` state for a list of requested names
        (src/sync/fs.rs:177-231): each name -- the bytes of a GET_FILE -- is
        decoded as UTF-8 (a bad encoding raises wire.ProtocolError,
        Error::BadFilenameEncoding) and resolved with ``get_file``, and its
        answer is FILE_START with the name, one FILE_BLOCK per row of
        ``list_file_blocks(file_id)`` in exactly that order, and FILE_END.

        Returns (run, n_answered).  Answering stops before the first name the
        index does not hold (a temporary file's name is not held): the
        reference answers those before it and then fails with "Requested file
        is unknown", so the caller sends the run and raises that when
        ``n_answered < len(names)``, as ``BlockSet.serve`` documents for
        digests.  ``device=None`` is the definition, the ``write_message``
        loop, and ``run`` is bytes.  With a device the rows of all answered
        files go up in one upload and ONE ``wire.files_device`` call
        (sf_wire_files_device) builds the answer in HBM: ``run`` is a
        ``wire.FilesRun`` (``bytes()``, ``to_fd(fd)``, ``receive``,
        ``close()``).  Parsing the received GET_FILE run stays with
        ``wire.Parser``; the name lookup is SQLite's, on the host."""
        from . import wire
        files = []  # (name bytes, [(hash, offset, size)])
        for name in names:
            raw = bytes(name)
            try:
                text = raw.decode("utf-8")
            except UnicodeDecodeError:
                raise wire.ProtocolError("Bad filename encoding") from None
            found = self.get_file(PurePath(text))
            if found is None:
                break
            files.append((raw, self.list_file_blocks(found[0])))
        if device is None:
            return b"".join(wire.write_message("FileStart", raw)
                            + b"".join(wire.write_message("FileBlock", h, size) for h, _offset, size in blocks)
                            + wire.write_message("FileEnd") for raw, blocks in files), len(files)
        import torch

        from .device import device_of, upload
        dev = device_of(device)
        rows = [b for _raw, blocks in files for b in blocks]
        # one buffer, widest elements first so that every part starts on its own grid
        parts = [np.cumsum([0] + [len(blocks) for _raw, blocks in files], dtype=np.int64).tobytes(),
                 np.cumsum([0] + [len(raw) for raw, _blocks in files], dtype=np.int64).tobytes(),
                 np.fromiter((size for _h, _offset, size in rows), np.uint32, len(rows)).tobytes(),
                 b"".join(h.bytes for h, _offset, _size in rows), b"".join(raw for raw, _blocks in files)]
        buf = upload(b"".join(parts), dev)
        at = np.cumsum([0] + [len(p) for p in parts]).tolist()
        first, name_at, sizes, digests, packed = (buf[a:b] for a, b in zip(at, at[1:]))
        run = wire.files_device(digests.reshape(len(rows), 20), sizes.view(torch.int32), first.view(torch.int64),
                                packed, name_at.view(torch.int64))
        return run, len(files)

    def source_tables(self, device=None) -> "SourceTables":
        """The source's tables for ``serve_get_file_requests``, built once per
        sync and kept in HBM: the packed names of all non-temporary files in
        file_id order with their ``device.NameSet``, and the CSR ``file_first``
        of those rows into one digest table and one size list holding every
        file's ``list_file_blocks`` rows in that order -- all in one upload.
        A small closeable object (``close()``, or a ``with`` block)."""
        return SourceTables(self, device)

    @staticmethod
    def _get_files_on_host(data: bytes):
        """The GET_FILE messages ``wire.Parser`` reads from byte 0 of ``data``
        -> ([name], [end of each], consumed, stop): ``stop`` the SF_WIRE_* class
        of what stands behind them."""
        from . import wire
        p = wire.Parser()
        p._buf = bytearray(data)
        names, ends, pos = [], [], 0
        while True:
            if pos == len(data):
                return names, ends, pos, wire.SF_WIRE_END
            try:
                line = p._line(pos, wire.COMMAND_MAX, "Unterminated command")
                if line is None:
                    return names, ends, pos, wire.SF_WIRE_INCOMPLETE
                if line[0] in (b"FILE_ENTRY", b"END_FILES", b"FILE_START", b"FILE_END", b"GET_BLOCK", b"FILE_BLOCK",
                               b"BLOCK_DATA", b"COMPLETE"):  # another command's complete line, whatever follows it
                    return names, ends, pos, wire.SF_WIRE_OTHER
                r = p._one(pos)  # an unknown command raises
            except wire.ProtocolError:
                return names, ends, pos, wire.SF_WIRE_MALFORMED
            if r is None:
                return names, ends, pos, wire.SF_WIRE_INCOMPLETE
            msg, pos = r
            names.append(msg[1])
            ends.append(pos)

    def serve_get_file_requests(self, data, device=None, tables=None, max_run_bytes: int = 0):
        """The source's ``Respond`` state for one received buffer of GET_FILE
        requests (src/sync/fs.rs:177-231): the requests at the start of
        ``data`` are parsed, each name resolved and answered with FILE_START,
        its FILE_BLOCKs and FILE_END.  Returns (run, n_requests, n_answered,
        answered_bytes, why, consumed, stop): ``consumed`` / ``stop`` describe
        the parsed prefix as ``wire.parse_blocks_device`` does (a run that
        arrives in pieces is continued with ``data[consumed:]`` + the new
        bytes); ``run`` answers requests ``[0, n_answered)``, which occupy
        ``data[:answered_bytes]``, and ``why`` says what stopped the answering:
        wire.SF_SERVE_ALL, SF_SERVE_BAD_NAME, SF_SERVE_UNKNOWN -- the caller
        sends the run and then raises "Bad filename encoding" / "Requested file
        is unknown", as the reference does -- or SF_SERVE_FULL: with the next
        answer the run would exceed ``max_run_bytes`` (0: no bound; a peer may
        repeat one large file's name): send the run and call again with
        ``data[answered_bytes:]``.

        ``device=None`` is the definition: ``wire.Parser`` over ``data``, then
        ``serve_get_files`` name by name; ``run`` is bytes.  With a device the
        buffer goes up and ONE ``device.NameSet.serve_files`` call
        (sf_serve_get_files_device) parses it, looks every name up and builds
        the answer in HBM from ``tables`` (``source_tables(device)``: built here
        and closed again when None -- keep one for the whole sync); ``run`` is
        a ``wire.FilesRun``.  The device compares the received bytes with the
        names as the index spells them, as the reference's query does; the
        host route's ``get_file`` also finds a name that ``PurePath`` respells
        (``a//b``).  The bound of 2^32 messages per run is the device route's
        alone."""
        from . import wire
        data = bytes(data)
        if device is not None or tables is not None:
            from .device import upload
            own = tables is None
            t = self.source_tables(device) if own else tables
            try:
                got = t.name_set.serve_files(upload(data, t.device), t.file_first, t.digests, t.sizes,
                                             max_run_bytes=max_run_bytes)
            finally:
                if own:
                    t.close()
            return tuple(got)
        names, ends, consumed, stop = self._get_files_on_host(data)
        out, answered, why = [], 0, wire.SF_SERVE_ALL
        total = 0
        for name in names:
            try:
                run, n = self.serve_get_files([name])
            except wire.ProtocolError:
                why = wire.SF_SERVE_BAD_NAME
                break
            if n == 0:
                why = wire.SF_SERVE_UNKNOWN
                break
            if max_run_bytes and total + len(run) > max_run_bytes:
                why = wire.SF_SERVE_FULL
                break
            out.append(run)
            total += len(run)
            answered += 1
        return b"".join(out), len(names), answered, ends[answered - 1] if answered else 0, why, consumed, stop

    def file_entries(self, device=None):
        """The source's ``ListFiles`` state over ``list_files()``
        (src/sync/fs.rs:133-164): one FILE_ENTRY per file -- name, size,
        blocks_hash -- in that order, then END_FILES.  ``device=None`` is the
        definition, the ``write_message`` loop, and returns bytes.  With a
        device the names, sizes and hashes go up in one upload and ONE
        ``wire.file_entries_device`` call (sf_wire_file_entries_device) builds
        the list in HBM: a ``wire.EntriesRun`` (``bytes()``, ``to_fd(fd)``,
        ``receive``, ``close()``).  Both routes raise SyncfastError for the
        first file the protocol cannot carry -- a name over 100 bytes or with
        a newline, a size of 10^15 or more, no blocks_hash -- where the
        reference would send the entry and its peer would raise mid-list."""
        from . import wire
        files = []
        for _file_id, path, _modified, size, blocks_hash in self.list_files():
            raw = str(path).encode("utf-8")
            if len(raw) > wire.FILENAME_MAX or b"\n" in raw or size >= 10 ** wire.SIZE_MAX or blocks_hash is None:
                raise SyncfastError("The protocol cannot carry file %r (name, size or no blocks_hash)" % str(path))
            files.append((raw, size, blocks_hash))
        if device is None:
            return b"".join(wire.write_message("FileEntry", *f) for f in files) + wire.write_message("EndFiles")
        import torch

        from .device import device_of, upload
        dev = device_of(device)
        # one buffer, widest elements first so that every part starts on its own grid
        parts = [np.cumsum([0] + [len(raw) for raw, _s, _h in files], dtype=np.int64).tobytes(),
                 np.fromiter((s for _raw, s, _h in files), np.int64, len(files)).tobytes(),
                 b"".join(h.bytes for _raw, _s, h in files), b"".join(raw for raw, _s, _h in files)]
        buf = upload(b"".join(parts), dev)
        at = np.cumsum([0] + [len(p) for p in parts]).tolist()
        name_at, sizes, hashes, packed = (buf[a:b] for a, b in zip(at, at[1:]))
        return wire.file_entries_device(packed, name_at.view(torch.int64), sizes.view(torch.int64),
                                        hashes.reshape(len(files), 20))

    @staticmethod
    def _entries_on_host(data: bytes):
        """The FILE_ENTRY messages ``wire.Parser`` reads from byte 0 of
        ``data`` -> ([(name, size, hash)], consumed, stop): ``stop`` the
        SF_WIRE_* class of what stands behind them, SF_WIRE_END_FILES with
        END_FILES read and counted."""
        from . import wire
        p = wire.Parser()
        p._buf = bytearray(data)
        entries, pos = [], 0
        while True:
            if pos == len(data):
                return entries, pos, wire.SF_WIRE_END
            try:
                line = p._line(pos, wire.COMMAND_MAX, "Unterminated command")
                if line is None:
                    return entries, pos, wire.SF_WIRE_INCOMPLETE
                if line[0] in (b"GET_FILE", b"FILE_START", b"FILE_END", b"GET_BLOCK", b"FILE_BLOCK", b"BLOCK_DATA",
                               b"COMPLETE"):  # another command's complete line, whatever follows it
                    return entries, pos, wire.SF_WIRE_OTHER
                r = p._one(pos)  # an unknown command raises
            except wire.ProtocolError:
                return entries, pos, wire.SF_WIRE_MALFORMED
            if r is None:
                return entries, pos, wire.SF_WIRE_INCOMPLETE
            msg, pos = r
            if msg[0] == "EndFiles":
                return entries, pos, wire.SF_WIRE_END_FILES
            entries.append(msg[1:])

    def _requests_on_host(self) -> bytes:
        """The GET_FILE messages of fs.rs:415-443: one per ``list_temp_files()``
        row, in that order."""
        from . import wire
        return b"".join(wire.write_message("GetFile", str(untemp_name(t)).encode("utf-8")) for t in self.list_temp_files())

    def receive_file_entries(self, data, device=None):
        """The sink's ``FilesList`` state for one received buffer
        (src/sync/fs.rs:378-446): every FILE_ENTRY at the start of ``data`` is
        looked up by name (``get_file``), its announced blocks_hash compared
        with the recorded one, and ``add_temp_file`` run for it when they
        differ, when none is recorded or when the file is unknown; END_FILES
        ends the list.  Returns (n_entries, consumed, stop, needed_names,
        requests): ``consumed`` / ``stop`` as ``wire.parse_blocks_device``
        (``stop`` is SF_WIRE_END_FILES once END_FILES was read; a list that
        arrives in pieces is continued with ``data[consumed:]`` + the new
        bytes), ``needed_names`` the names (bytes) of the entries that got a
        temp row, in entry order -- creating those files on disk stays with
        the caller -- and ``requests`` the GET_FILE run for
        ``list_temp_files()`` in that order once END_FILES was read, else None.
        A name that is not UTF-8 raises SyncfastError("Bad filename
        encoding") after the entries before it have been applied, as the
        reference does.

        ``device=None`` is the reference's loop message by message and the
        definition; ``requests`` is bytes.  With a device the destination's
        non-temporary rows go up once, one ``device.NameSet`` is built, ONE
        sf_receive_file_entries_device call parses, looks up and compares the
        whole buffer, ``add_temp_file`` runs per needed entry in entry order
        (the database stays SQLite's), and ``requests`` is a
        ``wire.GetFilesRun`` built from the received names in place
        (sf_wire_get_files_device): from the call's need list when
        ``list_temp_files()`` is exactly the needed entries in order, else
        from an explicit pick, with the names of leftover temp rows of an
        earlier sync uploaded behind the list.  One lookup for the whole list
        equals the loop unless the index holds a non-temporary file whose last
        component starts with ``.syncfast_tmp_``: ``add_temp_file`` resets such
        a row to temporary (src/index.rs:262-300), and a later entry's
        ``get_file`` would see that.  Such an index takes the loop."""
        from . import wire
        data = bytes(data)
        if device is not None and not any(PurePath(r[0]).name.startswith(TEMP_PREFIX) for r in self.db.execute(
                "SELECT name FROM files WHERE temporary = 0 AND name LIKE ?;", ("%" + TEMP_PREFIX + "%",))):
            return self._receive_file_entries_device(data, device)
        entries, consumed, stop = self._entries_on_host(data)
        needed = []
        for name, _size, blocks_hash in entries:
            try:
                path = PurePath(name.decode("utf-8"))
            except UnicodeDecodeError:
                raise SyncfastError("Bad filename encoding") from None
            found = self.get_file(path)
            if found is None or found[2] != blocks_hash:
                self.add_temp_file(path)
                needed.append(name)
        requests = self._requests_on_host() if stop == wire.SF_WIRE_END_FILES else None
        return len(entries), consumed, stop, needed, requests

    def _receive_file_entries_device(self, data: bytes, device):
        import torch

        from . import wire
        from .device import NameSet, device_of, upload
        dev = device_of(device)
        rows = self.db.execute("SELECT name, blocks_hash FROM files WHERE temporary = 0 ORDER BY file_id;").fetchall()
        names = [str(PurePath(r[0])).encode("utf-8") for r in rows]
        hashes = [HashDigest.from_sql(r[1]).bytes if r[1] is not None else bytes(20) for r in rows]
        # one upload: the CSR first (8-B entries), then hashes, flags and names
        parts = [np.cumsum([0] + [len(n) for n in names], dtype=np.int64).tobytes(), b"".join(hashes),
                 bytes(r[1] is not None for r in rows), b"".join(names)]
        buf = upload(b"".join(parts), dev)
        at = np.cumsum([0] + [len(p) for p in parts]).tolist()
        name_at, have, have_ok, packed = (buf[a:b] for a, b in zip(at, at[1:]))
        run = upload(data, dev)
        with NameSet(packed, name_at.view(torch.int64)) as ns:
            got = ns.receive_entries(run, have.reshape(len(rows), 20), have_ok)
        n = int(got.name_at.numel())
        starts, lens = got.name_at.cpu().tolist(), got.name_len.cpu().tolist()
        need = got.need_list.cpu().tolist()
        if got.bad_name is not None:
            need = [i for i in need if i < got.bad_name]
        needed = [data[starts[i]:starts[i] + lens[i]] for i in need]
        for name in needed:
            self.add_temp_file(PurePath(name.decode("utf-8")))
        if got.bad_name is not None:
            raise SyncfastError("Bad filename encoding")
        if got.stop != wire.SF_WIRE_END_FILES:
            return n, got.consumed, got.stop, needed, None
        want = [str(untemp_name(t)).encode("utf-8") for t in self.list_temp_files()]
        if want == needed:  # the temp rows are exactly the needed entries, in order: the call's own list picks them
            requests = wire.get_files_device(run, got.name_at, got.name_len, got.need_list)
            return n, got.consumed, got.stop, needed, requests
        # leftover temp rows, or names the index spells otherwise: their bytes go behind the list
        where = {}
        for i, name in zip(need, needed):
            where.setdefault(name, i)
        extra, spans, pick = b"", [], []
        for name in want:
            if name not in where:
                where[name] = n + len(spans)
                spans.append((len(data) + len(extra), len(name)))
                extra += name
            pick.append(where[name])
        both = torch.cat([run, upload(extra, dev)])
        at2 = torch.cat([got.name_at, torch.tensor([a for a, _l in spans], dtype=torch.int64, device=dev)])
        len2 = torch.cat([got.name_len, torch.tensor([ln for _a, ln in spans], dtype=torch.int32, device=dev)])
        requests = wire.get_files_device(both, at2, len2, torch.tensor(pick, dtype=torch.int32, device=dev))
        return n, got.consumed, got.stop, needed, requests

    def get_file(self, name) -> Optional[Tuple[int, DateTimeUtc, Optional[HashDigest]]]:
        row = self.db.execute(
            "SELECT file_id, modified, blocks_hash FROM files WHERE name = ? AND temporary = 0;",
            (_name_str(name),)).fetchone()
        if not row:
            return None
        return (int(row[0]), DateTimeUtc.from_sql(row[1]),
                HashDigest.from_sql(row[2]) if row[2] is not None else None)

    def get_temp_file(self, name) -> Optional[Tuple[int, DateTimeUtc]]:
        row = self.db.execute("SELECT file_id, modified FROM files WHERE name = ? AND temporary = 1;",
                              (_name_str(temp_name(name)),)).fetchone()
        return (int(row[0]), DateTimeUtc.from_sql(row[1])) if row else None

    def get_file_name(self, file_id: int) -> Optional[PurePath]:
        row = self.db.execute("SELECT name FROM files WHERE file_id = ?;", (file_id,)).fetchone()
        return PurePath(row[0]) if row else None

    def list_files(self):
        rows = self.db.execute(
            "SELECT file_id, name, modified, size, blocks_hash FROM files WHERE temporary = 0;").fetchall()
        return [(int(r[0]), PurePath(r[1]), DateTimeUtc.from_sql(r[2]), int(r[3] or 0),
                 HashDigest.from_sql(r[4]) if r[4] is not None else None) for r in rows]

    def list_file_blocks(self, file_id: int) -> List[Tuple[HashDigest, int, int]]:
        rows = self.db.execute("SELECT hash, offset, size FROM blocks WHERE file_id = ?;", (file_id,)).fetchall()
        return [(HashDigest.from_sql(r[0]), int(r[1]), int(r[2])) for r in rows]

    def list_temp_files(self) -> List[PurePath]:
        return [PurePath(r[0]) for r in self.db.execute("SELECT name FROM files WHERE temporary = 1;")]

    def check_temp_files(self):
        rows = self.db.execute(
            "SELECT file_id, name, EXISTS (SELECT hash FROM blocks WHERE blocks.file_id = files.file_id "
            "AND present = 0) AS missing FROM files WHERE temporary = 1;").fetchall()
        return [(int(r[0]), PurePath(r[1]), bool(r[2])) for r in rows]

    def list_missing_blocks(self) -> List[HashDigest]:
        return [HashDigest.from_sql(r[0]) for r in self.db.execute("SELECT hash FROM blocks WHERE present = 0;")]

    def list_block_locations(self, hash: HashDigest):
        rows = self.db.execute(
            "SELECT files.file_id, files.name, blocks.offset, blocks.size FROM blocks "
            "INNER JOIN files ON files.file_id = blocks.file_id WHERE hash = ?;", (hash.to_sql(),)).fetchall()
        return [(int(r[0]), PurePath(r[1]), int(r[2]), int(r[3])) for r in rows]

    # -- mutations (src/index.rs:176-408, 433-451, 591-607)
    def add_file(self, name, modified) -> Tuple[int, bool]:
        """(file_id, up_to_date): the mtime gate of src/index.rs:176-218.
        ``modified``: DateTimeUtc, an aware datetime, or ns since the epoch;
        compared with the stored value as an instant (src/index.rs:183)."""
        self.begin()
        m = DateTimeUtc.coerce(modified)
        cur = self.get_file(name)
        if cur is not None and cur[1] == m:
            return cur[0], True
        if cur is not None:
            log.info("Resetting file %s, modified", name)
        else:
            log.info("Inserting new file %s", name)
        return self._put_file(cur and cur[0], name, m, 0), False

    def _put_file(self, file_id: Optional[int], name, modified: DateTimeUtc, temporary: int) -> int:
        """The file row under add_file, add_file_overwrite and add_temp_file:
        row ``file_id`` loses its blocks and is reset to ``modified`` and
        ``temporary``; None: a new row for ``name``.  Returns the file_id."""
        if file_id is not None:
            self.db.execute("DELETE FROM blocks WHERE file_id = ?;", (file_id,))
            self.db.execute("UPDATE files SET modified = ?, size = NULL, blocks_hash = NULL, temporary = ? "
                            "WHERE file_id = ?;", (modified.to_sql(), temporary, file_id))
            return file_id
        c = self.db.execute("INSERT INTO files(name, modified, temporary) VALUES(?, ?, ?);",
                            (_name_str(name), modified.to_sql(), temporary))
        return int(c.lastrowid)

    def add_file_overwrite(self, name, modified) -> int:
        self.begin()
        m = DateTimeUtc.coerce(modified)
        cur = self.get_file(name)
        return self._put_file(cur and cur[0], name, m, 0)

    def add_temp_file(self, name) -> int:
        self.begin()
        now = _now()
        tname = _name_str(temp_name(name))
        # the temp name is looked up among the files that are NOT temporary, as
        # the reference does (src/index.rs:253-290)
        row = self.db.execute("SELECT file_id FROM files WHERE name = ? AND temporary = 0;", (tname,)).fetchone()
        return self._put_file(row and int(row[0]), tname, now, 1)

    def remove_file(self, file_id: int) -> None:
        self.begin()
        self.db.execute("DELETE FROM blocks WHERE file_id = ?;", (file_id,))
        self.db.execute("DELETE FROM files WHERE file_id = ?;", (file_id,))

    def move_temp_file_into_place(self, file_id: int, destination) -> None:
        self.begin()
        dst = _name_str(destination)
        self.db.execute("DELETE FROM blocks WHERE file_id = (SELECT file_id FROM files WHERE name = ?);", (dst,))
        self.db.execute("DELETE FROM files WHERE name = ?;", (dst,))
        self.db.execute("UPDATE files SET name = ?, temporary = 0 WHERE file_id = ?;", (dst, file_id))

    def add_block(self, hash: HashDigest, file_id: int, offset: int, size: int) -> None:
        """One row, present = 1 (src/index.rs:387-408)."""
        self.begin()
        self.db.execute(INSERT_BLOCK, (hash.to_sql(), file_id, offset, size, 1))

    def add_blocks(self, file_id: int, rows: Sequence[Tuple[int, int, bytes]]) -> None:
        """add_block for a whole signature table in one executemany (the
        reference issues one un-prepared INSERT per block)."""
        self.begin()
        self.db.executemany(INSERT_BLOCK, ((d.hex(), file_id, o, s, 1) for o, s, d in rows))

    def add_missing_block(self, hash: HashDigest, file_id: int, offset: int, size: int) -> None:
        self.begin()
        self.db.execute(INSERT_BLOCK, (hash.to_sql(), file_id, offset, size, 0))

    def mark_block_present(self, file_id: int, hash: HashDigest, offset: int) -> None:
        self.begin()
        self.db.execute("UPDATE blocks SET present = 1 WHERE file_id = ? AND hash = ? AND offset = ?;",
                        (file_id, hash.to_sql(), offset))

    def set_file_size_and_compute_blocks_hash(self, file_id: int, size: int) -> None:
        self.begin()
        bh = self.compute_blocks_hash(file_id)
        self.db.execute("UPDATE files SET size = ?, blocks_hash = ? WHERE file_id = ?;", (size, bh.to_sql(), file_id))

    def compute_blocks_hash(self, file_id: int) -> HashDigest:
        """src/index.rs:661-682: SHA-1 over the raw digests, SELECT order."""
        rows = self.db.execute("SELECT hash FROM blocks WHERE file_id = ?;", (file_id,)).fetchall()
        raw = b"".join(HashDigest.from_sql(r[0]).bytes for r in rows)
        return HashDigest(host.blocks_hash(raw))

    # -- the hot path (src/index.rs:610-659)
    def index_file(self, path, name) -> None:
        """Cut a file into blocks and add them to the index.

        Native routes return the rows and the blocks_hash together: SHA-1 over
        the digests in offset order, which is the order the rows are inserted
        in and so the order compute_blocks_hash's SELECT reads them back in
        (src/index.rs:661-682) -- the same value without re-reading the rows.
        Like the reference (src/index.rs:615-625), ONE open of the file gives
        the mtime, the boundaries and the bytes: BoundaryChunker(stream=True)
        on a regular file streams the open file and the library re-reads that
        same descriptor by windows (sf_index_fd_blocks); FixedChunker:
        sf_index_fd_fixed on it (sf_index_fd for a FIFO); a BoundaryChunker
        over bytes: the file's bytes and the list go to
        sf_index_buffer_blocks.  The descriptor routes compare the file's
        stamp (fstat, taken before the chunker read it) when they start and
        after their last read: a file written while it is indexed is indexed
        again from a new open, never stored as rows that mix two versions of
        it.  A file that keeps changing (a log being appended to) is, after
        CHANGED_RETRIES attempts, indexed in ONE pass as the reference does
        (src/index.rs:615-647): its bytes are read once from one open, the
        chunker cuts those bytes and the same bytes are hashed
        (sf_index_buffer_blocks / sf_index_buffer), so the rows describe the
        bytes read whatever the writer does meanwhile.  (Stamps are only as
        fine as the filesystem's clock tick: a same-size write within the
        tick of the stamp is not seen, include/syncfast_amd.h.)"""
        self._need_chunker()
        self._index_file_retrying(path, name)

    def _index_file_retrying(self, path, name, changed: bool = False) -> None:
        """index_file's attempts: CHANGED_RETRIES, then the one-pass read.
        ``changed``: the walk's own pass over the file (in a batch, or alone)
        saw it change already.  Its row was added then, in walk order, so only
        its blocks are indexed again; that pass is the one reported, and the
        attempts here are all retries."""
        for attempt in range(-1 if changed else 0, CHANGED_RETRIES):
            if attempt >= 0:
                try:
                    self._index_file_once(path, name, force=changed or attempt > 0)
                    return
                except SfError as e:
                    if e.code != SF_EAGAIN:
                        raise
            if attempt < 0 or not changed:
                log.info("File %s changed while it was indexed, indexing it again", path)
        if not changed:
            log.info("File %s keeps changing: indexing the bytes of one read", path)
        self._index_file_once(path, name, force=True, one_pass=True)

    def _index_file_once(self, path, name, force: bool, one_pass: bool = False, opened=None) -> None:
        """One attempt of index_file; `opened`: the file already open, and the
        caller's to close (a FIFO met by the walk is indexed from that open: a
        second open would wait for another writer, and the first's data would
        be lost)."""
        ch = self.chunker
        native = None  # (rows, blocks_hash) from a native route
        # File::open first: same error on a missing file
        with (open(path, "rb") if opened is None else contextlib.nullcontext(opened)) as f:
            seekable = _seekable(f)
            stamp = host.file_stamp(f.fileno()) if seekable and not one_pass and \
                (isinstance(ch, FixedChunker) or ch.stream) else None
            file_id, up_to_date = self.add_file(name, _stamp_mtime(stamp) if stamp else _mtime(f))
            if up_to_date:
                if not force:
                    return
                # a retry after SF_EAGAIN whose mtime did not move (the writer
                # restored it, or only the ctime changed): index it anyway
                self.db.execute("DELETE FROM blocks WHERE file_id = ?;", (file_id,))
            if isinstance(ch, FixedChunker):
                if one_pass:  # the bytes of one read, hashed from host memory
                    raw = f.read()
                    rows_np = host.index_buffer(raw, ch.block_size)
                    native = (rows_np, host.blocks_hash(np.ascontiguousarray(rows_np["sha1"])))
                elif seekable:
                    native = host.index_fd_fixed(f.fileno(), ch.block_size, stamp)
                else:  # a FIFO: read sequentially from this open, as File::open + read do
                    native = host.index_fd(f.fileno(), ch.block_size)
            elif isinstance(ch, NativeChunker) and seekable and not one_pass:
                return self._index_fd_native(file_id, f, ch.threads, stamp)
            elif ch.stream and seekable and not one_pass:
                sizes = _cut_stamped(ch.fn, f, stamp)
                if sizes is None:  # written while chunked
                    raise SfError(SF_EAGAIN, f"index_file({os.fsdecode(path)})")
                native = host.index_fd_blocks(f.fileno(), _offsets(sizes), np.asarray(sizes, np.uint32), stamp)
            else:
                rows = signatures_of_bytes(f.read(), ch)
        if native is not None:
            return self._store_rows(file_id, *native)
        if log.isEnabledFor(logging.DEBUG):
            for o, sz, d in rows:
                log.debug("Adding block, offset=%d, size=%d, sha1=%s", o, sz, d.hex())
        self.add_blocks(file_id, rows)
        bh = self.compute_blocks_hash(file_id)
        self.db.execute("UPDATE files SET blocks_hash = ? WHERE file_id = ?;", (bh.to_sql(), file_id))

    def _store_rows(self, file_id: int, rows, blocks_hash, a: int = 0, b: Optional[int] = None) -> None:
        """A file's native result, stored: add_block for rows[a:b] of a native
        signature table -- the hash column hex-encoded once (HashDigest ToSql,
        src/lib.rs:78-90), one executemany -- and the file's ``blocks_hash``
        (bytes, or 20 uint8)."""
        self.begin()
        b = rows.shape[0] if b is None else b
        hx = rows["sha1"][a:b].tobytes().hex()
        offs, sizes = rows["offset"][a:b].tolist(), rows["size"][a:b].tolist()
        if log.isEnabledFor(logging.DEBUG):
            for i in range(b - a):
                log.debug("Adding block, offset=%d, size=%d, sha1=%s", offs[i], sizes[i], hx[40 * i:40 * i + 40])
        self.db.executemany(INSERT_BLOCK, zip((hx[i:i + 40] for i in range(0, len(hx), 40)), itertools.repeat(file_id),
                                              offs, sizes, itertools.repeat(1)))
        self.db.execute("UPDATE files SET blocks_hash = ? WHERE file_id = ?;", (bytes(blocks_hash).hex(), file_id))

    def _index_fd_native(self, file_id: int, f, threads: int, stamp) -> None:
        """The open, stamped regular file ``f``, already through the mtime gate
        as ``file_id``, cut and hashed in one call by the NativeChunker on
        ``threads`` threads (``index_fd``: one read), and stored."""
        self._store_rows(file_id, *self.chunker.index_fd(f.fileno(), threads, stamp))

    def index_path(self, path, batch_bytes: int = 256 << 20, chunk_threads: int = 0,
                   large_file_bytes: int = LARGE_FILE_BYTES) -> None:
        """Index files and directories recursively (src/index.rs:685-715).

        Same walk, names and mtime gate as the reference.  With a
        FixedChunker, every file that needs (re)indexing goes through ONE
        native pipeline (sf_index_files) in stages of `batch_bytes`: pinned
        host buffers filled by a pread thread pool, one H2D copy and one
        device launch per stage (blocks + every file's blocks_hash), reading
        overlapped with the device.  With BoundaryChunker(stream=True) -- the
        reference's default mode -- the chunker cuts the files on a pool of
        `chunk_threads` threads (0: one per core, at most 16; a chunker is
        per-file state, so files cut independently), and every batch of about
        `batch_bytes` of cut files goes through ONE native pipeline
        (sf_index_fds_blocks: the open descriptors re-read by windows into
        packed pinned stages, one sort + one explicit-list launch per stage)
        while the pool cuts the next batch.  A NativeChunker's files of at
        least `large_file_bytes` (64 MiB: configs[0]'s one file) are instead
        cut on `chunk_threads` threads each and hashed from one read
        (sf_index_fd_cut, Index.index_file's route), in their walk position:
        one large file alone would otherwise be cut on a single thread.
        batch_bytes=0 indexes file by file."""
        self._need_chunker()
        todo: List[Tuple[Path, PurePath]] = []
        self._index_path_rec(Path(path), PurePath(""), todo)
        if not todo:
            return
        if batch_bytes <= 0:
            for p, rel in todo:
                self.index_file(p, rel)
            return
        if isinstance(self.chunker, BoundaryChunker):
            if self.chunker.stream:
                self._index_batched_fds(todo, batch_bytes, chunk_threads, large_file_bytes)
            else:
                self._index_batched_boundaries(todo, batch_bytes)
            return
        self._index_batched(todo, batch_bytes)

    def _index_path_rec(self, root: Path, rel: PurePath, todo) -> None:
        p = root / rel
        if p.is_dir():
            log.info("Indexing directory %s (%s)", rel, p)
            for entry in os.listdir(p):  # readdir order, as read_dir (src/index.rs:698)
                if entry == INDEX_FILE_NAME:
                    continue
                self._index_path_rec(root, rel / entry, todo)
        else:
            if rel.parts[:1] == (".",):
                rel = PurePath(*rel.parts[1:])
            # index_path on a file: the reference's rel is Path::new(""), whose
            # name is the empty string (PurePath("") would print as ".")
            name = "" if rel == PurePath("") else rel
            log.info("Indexing file %s (%s)", rel, p)
            todo.append((p, name))

    def _index_batched(self, todo, batch_bytes: int) -> None:
        """Every file needing (re)indexing through ONE native pipeline
        (sf_index_files): pread thread pool into pinned stages of
        `batch_bytes`, H2D + device blocks/blocks_hash per stage, overlapped
        with the reading of the next stage."""
        bs = self.chunker.block_size
        pending = []  # (file_id, path) needing signatures
        for p, rel in todo:
            with open(p, "rb") as f:  # same error as File::open on a vanished file
                file_id, up_to_date = self.add_file(rel, _mtime(f))
                if not up_to_date and not _seekable(f):
                    # a FIFO in the tree: read it from this open (a second
                    # open would wait for another writer); rows like index_file
                    self._store_rows(file_id, *host.index_fd(f.fileno(), bs))
                    continue
            if not up_to_date:
                pending.append((file_id, p))
        if not pending:
            return
        rows, first, fh = host.index_files([p for _f, p in pending], bs, stage_bytes=batch_bytes)
        for k, (file_id, _p) in enumerate(pending):
            self._store_rows(file_id, rows, fh[k], int(first[k]), int(first[k + 1]))

    def _index_batched_fds(self, todo, batch_bytes: int, chunk_threads: int,
                           large_file_bytes: int = LARGE_FILE_BYTES) -> None:
        """The default (content-defined) mode over many files, the files cut
        in parallel and hashed as ONE pipeline per batch.

        Each file is opened once and stamped (sf_file_stamp_fd: its mtime is
        the one stored, the mtime gate runs in walk order, so file_ids are the
        reference's); the chunker streams the open file on a pool thread; a
        batch of about `batch_bytes` of cut files (and at most a quarter of
        the descriptor limit) goes to sf_index_fds_blocks on those same
        descriptors while the pool cuts the next batch.  A file written while
        it was cut or read (SF_EAGAIN for it alone) is indexed again through
        index_file, in its place, so rows stay in walk order.  Two kinds of
        file are indexed alone, in their walk position, once every batch
        before them has been stored (rows in walk order, so get_block's first
        row for a digest is the reference's, src/index.rs:80-90): a FIFO
        (streamed, as index_file streams it) and, with a NativeChunker, a
        regular file of at least `large_file_bytes` (cut on the chunker's
        threads and hashed from one read, sf_index_fd_cut, with the stamp
        taken at its open).

        With ZpaqChunker(device=True) the batched files are not cut here at
        all: they are stamped and collected, and each batch goes through one
        sf_index_fds_zpaq call, which reads every file once and cuts and
        hashes it on the device.  Everything else is as above."""
        import resource
        from concurrent.futures import ThreadPoolExecutor

        ch = self.chunker
        threads = chunk_threads if chunk_threads > 0 else min(16, os.cpu_count() or 1)
        soft = resource.getrlimit(resource.RLIMIT_NOFILE)[0]
        max_files = max(16, min(4096, (soft if soft > 0 else 1024) // 4))
        native = isinstance(ch, NativeChunker)
        on_device = isinstance(ch, ZpaqChunker) and ch.device  # the batches are cut by sf_index_fds_zpaq

        def finish(batch):
            """Hash the cut files of `batch` in one call, close them, store them."""
            entries = batch.entries
            if not entries:
                return
            if on_device:
                keep = list(range(len(entries)))
                res = host.index_fds_zpaq([e[3].fileno() for e in entries], ch.bits, ch.max_size,
                                          [e[4] for e in entries], ch.max_rounds, batch_bytes)
            else:
                cuts = [e[5].result() for e in entries]
                keep = [k for k, c in enumerate(cuts) if c is not None]
                lists = [(_offsets(cuts[k]), np.asarray(cuts[k], np.uint32)) for k in keep]
                res = host.index_fds_blocks([entries[k][3].fileno() for k in keep], lists,
                                            [entries[k][4] for k in keep], stage_bytes=batch_bytes) if keep else None
            batch.close()  # cut and hashed: nothing reads its descriptors any more
            pos = {k: j for j, k in enumerate(keep)}
            for k, (fid, p, rel, _f, _st, _fut) in enumerate(entries):
                j = pos.get(k)
                if j is not None and res[3][j] == 0:
                    rows, first, hashes, _status = res
                    self._store_rows(fid, rows, hashes[j], int(first[j]), int(first[j + 1]))
                    continue
                code = SF_EAGAIN if j is None else int(res[3][j])
                if code != SF_EAGAIN:
                    raise SfError(code, f"index_file({os.fsdecode(p)})")
                self.db.execute("DELETE FROM blocks WHERE file_id = ?;", (fid,))
                self._index_file_retrying(p, rel, changed=True)

        # Two batches: `cutting` is filled while the pool cuts its files,
        # `hashing` is the full one before it.  They own their open files: a
        # batch that was hashed is closed there (finish); leaving this block
        # closes what an exception left in them or never submitted -- after the
        # pool, which is entered last, has shut down, so no chunker is still
        # reading a descriptor that is being closed.
        with _FdBatch() as cutting, _FdBatch() as hashing, ThreadPoolExecutor(max_workers=threads) as pool:
            for p, rel in todo:
                changed = False
                with contextlib.ExitStack() as mine:  # the open file is this step's until a batch takes it
                    f = mine.enter_context(open(p, "rb"))  # File::open first: same error on a missing file
                    fifo = not _seekable(f)
                    if not fifo:
                        stamp = host.file_stamp(f.fileno())
                        file_id, up_to_date = self.add_file(rel, _stamp_mtime(stamp))
                        if up_to_date:
                            continue
                    if fifo or (native and stamp.size >= large_file_bytes > 0):
                        # indexed alone, in its walk position: every batch before it is stored first
                        finish(hashing)
                        finish(cutting)
                        try:
                            if fifo:  # read from this open, sequentially
                                self._index_file_once(p, rel, force=False, opened=f)
                            else:  # cut on the chunker's threads + hashed, one read of this open
                                self._index_fd_native(file_id, f, ch.threads or threads, stamp)
                        except SfError as e:
                            if fifo or e.code != SF_EAGAIN:
                                raise
                            changed = True
                    else:
                        cutting.enter_context(mine.pop_all())
                        cut = None if on_device else pool.submit(_cut_stamped, ch.fn, f, stamp)
                        cutting.entries.append((file_id, p, rel, f, stamp, cut))
                        cutting.nbytes += stamp.size
                if changed:
                    self._index_file_retrying(p, rel, changed=True)
                elif cutting.nbytes >= batch_bytes or len(cutting.entries) >= max_files:
                    finish(hashing)  # hashed while the pool cuts the batch that is now full
                    cutting, hashing = hashing, cutting
            finish(hashing)
            finish(cutting)

    def _index_batched_boundaries(self, todo, batch_bytes: int) -> None:
        """The default (content-defined) mode over many files: each file is
        read and cut by the host chunker, and the blocks of up to
        `batch_bytes` of files go to the device in ONE sf_index_buffer_blocks
        call (their bytes back to back, one offset-ordered list), so the
        per-call latency of a long block's chain is paid
        per batch, not per file.  Rows get file offsets back; each file's
        blocks_hash is the SHA-1 over its digests in offset order, the value
        compute_blocks_hash reads back (src/index.rs:661-682)."""
        batch = []  # (file_id, base, n_bytes, sizes)
        parts: List[bytes] = []
        nbytes = 0

        def flush():
            nonlocal batch, parts, nbytes
            if not batch:
                return
            offs = np.zeros(sum(len(sz) for _f, _b, _n, sz in batch), np.uint64)
            sizes = np.zeros(offs.size, np.uint32)
            k = 0
            for _fid, base, _n, sz in batch:
                if sz:
                    a = np.asarray(sz, np.uint64)
                    offs[k:k + a.size] = base + np.concatenate([[0], np.cumsum(a)[:-1]]).astype(np.uint64)
                    sizes[k:k + a.size] = a
                    k += a.size
            rows, _ = host.index_buffer_blocks(b"".join(parts), offs, sizes)
            k = 0
            for fid, base, _n, sz in batch:
                mine = rows[k:k + len(sz)].copy()
                k += len(sz)
                mine["offset"] -= np.uint64(base)
                self._store_rows(fid, mine, host.blocks_hash(np.ascontiguousarray(mine["sha1"])))
            batch, parts, nbytes = [], [], 0

        for p, rel in todo:
            with open(p, "rb") as f:  # File::open first: same error on a missing file
                file_id, up_to_date = self.add_file(rel, _mtime(f))
                if up_to_date:
                    continue
                raw = f.read()  # a FIFO in the tree is read from this open, to EOF
            sizes = _sizes_ok(self.chunker.fn(raw), len(raw))
            batch.append((file_id, nbytes, len(raw), sizes))
            parts.append(raw)
            nbytes += len(raw)
            if nbytes >= batch_bytes:
                flush()
        flush()

    def remove_missing_files(self, path) -> None:
        """src/index.rs:718-726."""
        for file_id, file_path, _m, _s, _bh in self.list_files():
            if not (Path(path) / file_path).is_file():
                log.info("Removing missing file %s", file_path)
                self.remove_file(file_id)


class SourceTables:
    """What the source keeps in HBM while it answers GET_FILE requests
    (``Index.source_tables``): ``names`` the names (bytes) of the index's
    non-temporary files in file_id order, ``name_set`` the ``device.NameSet``
    over them, ``file_first`` int64[rows + 1] the CSR of those rows into
    ``digests`` uint8[n, 20] / ``sizes`` int32[n], which hold every file's
    ``list_file_blocks`` rows in that order.  One upload; ``seconds`` says what
    reading the database, packing and uploading, and building the set took.
    ``close()`` frees the set (also on leaving a ``with`` block)."""

    def __init__(self, index: "Index", device=None):
        import time

        import torch

        from .device import NameSet, device_of, upload
        t0 = time.perf_counter()
        self.device = device_of(device)
        files = index.db.execute("SELECT file_id, name FROM files WHERE temporary = 0 ORDER BY file_id;").fetchall()
        self.names = [str(PurePath(r[1])).encode("utf-8") for r in files]
        blocks = [index.list_file_blocks(int(r[0])) for r in files]
        rows = [b for per_file in blocks for b in per_file]
        t1 = time.perf_counter()
        # one buffer, widest elements first so that every part starts on its own grid
        parts = [np.cumsum([0] + [len(n) for n in self.names], dtype=np.int64).tobytes(),
                 np.cumsum([0] + [len(b) for b in blocks], dtype=np.int64).tobytes(),
                 np.fromiter((size for _h, _offset, size in rows), np.uint32, len(rows)).tobytes(),
                 b"".join(h.bytes for h, _offset, _size in rows), b"".join(self.names)]
        buf = upload(b"".join(parts), self.device)
        at = np.cumsum([0] + [len(p) for p in parts]).tolist()
        name_at, first, sizes, digests, packed = (buf[a:b] for a, b in zip(at, at[1:]))
        self.file_first, self.sizes = first.view(torch.int64), sizes.view(torch.int32)
        self.digests = digests.reshape(len(rows), 20)
        torch.cuda.synchronize(self.device)
        t2 = time.perf_counter()
        self.name_set = NameSet(packed, name_at.view(torch.int64))
        torch.cuda.synchronize(self.device)
        self.seconds = {"database": t1 - t0, "pack_upload": t2 - t1, "name_set": time.perf_counter() - t2}

    def close(self) -> None:
        self.name_set.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
