"""The incoming files of a sync, assembled in HBM.

The two sink states of the reference end in file writes: read_block +
write_block for every block the destination already holds
(src/sync/fs.rs:463-470), write_block for every location of every received
payload (fs.rs:505-510), then ``finish`` renames the temp files
(fs.rs:529-548).  ``Index.receive_file_blocks`` and
``Index.receive_block_data`` return those writes as lists and write nothing.
``FileImages`` carries the lists out on the device: one HBM image per incoming
temp file, filled by the block copy kernel (``device.copy_blocks``,
sf_copy_blocks_device) in one launch per list, checked as a whole against the
rows the source announced, and written to the temp file's descriptor
(``device.write_to_fd``).  A job list that is on the device already -- the join
of ``device.place_block_data``, the plan of ``device.plan_copies`` -- goes in as
it is (``apply_jobs``).  ``LocalFiles`` is the source of the second: one HBM
arena of the destination's own files, loaded with ``device.read_fd``.
"""
from __future__ import annotations

import hashlib
import os
from pathlib import Path
from typing import Callable, Dict, List, Mapping, Optional

import numpy as np
import torch

from . import device as _device
from ._lib import SF_EAGAIN, SF_EIO, FileStamp, SfError, lib
from .index import _name_str

__all__ = ["FileImages", "LocalFiles"]


def _rounds(jobs: List[tuple]) -> List[List[tuple]]:
    """jobs = [(src_offset, dst_offset, size > 0)] in the order the reference
    would write them, split into calls of disjoint destinations: a job that
    overlaps an earlier one goes to a later call than that one.  The usual
    list overlaps nowhere and is one call, found by a sort; only the jobs that
    overlap anything are compared pair by pair."""
    if not jobs:
        return []
    involved = [False] * len(jobs)
    end, holder = -1, -1  # the furthest end among the jobs before, by start, and whose it is
    for i in sorted(range(len(jobs)), key=lambda i: jobs[i][1]):
        _s, at, size = jobs[i]
        if at < end:
            involved[i] = involved[holder] = True
        if at + size > end:
            end, holder = at + size, i
    rounds: List[List[tuple]] = [[j for i, j in enumerate(jobs) if not involved[i]]]
    placed: List[tuple] = []  # (dst_offset, end, round) of the involved jobs so far, in list order
    for i, (s, at, size) in enumerate(jobs):
        if not involved[i]:
            continue
        r = 1 + max((p[2] for p in placed if p[0] < at + size and at < p[1]), default=-1)
        placed.append((at, at + size, r))
        while len(rounds) <= r:
            rounds.append([])
        rounds[r].append((s, at, size))
    return [r for r in rounds if r]


class LocalFiles:
    """One HBM arena of the local files a copy plan reads
    (``device.plan_copies``), in the plan's numbering: file j is ``names[j]``.

    ``stat(names)`` takes every file's size (a file that cannot be stat'ed gets
    UNKNOWN_SIZE: no row in it is stale, and as it cannot be loaded either its
    blocks are unavailable).  ``load(need)`` lays the files with
    ``need[j] != 0`` (None: all) out at 256-byte-aligned bases of ONE
    allocation, opens each, stamps its descriptor and reads it with
    ``device.read_fd`` against that stamp.  A file that cannot be opened,
    whose size is no longer the one ``stat`` saw, or that changed while it was
    read gets the base UINT64_MAX (-1): the plan calls its blocks unavailable
    and they are requested from the source.  ``bases()`` and ``sizes()`` are the
    plan's ``local_base`` and ``local_size``, ``arena`` its ``src``."""

    ALIGN = 256
    NOT_LOADED = -1  # UINT64_MAX as the int64 the tensors hold
    UNKNOWN_SIZE = (1 << 63) - 1

    def __init__(self, root, device=None):
        self.root = Path(root)
        self.device = _device.device_of(device)
        self.names: List[str] = []
        self._sizes: List[int] = []
        self._bases: List[int] = []
        self.arena = torch.empty(0, dtype=torch.uint8, device=self.device)

    def stat(self, names) -> "LocalFiles":
        self.names = [_name_str(n) for n in names]
        self._sizes = []
        for name in self.names:
            try:
                self._sizes.append(os.stat(self.root / name).st_size)
            except OSError:
                self._sizes.append(self.UNKNOWN_SIZE)
        self._bases = [self.NOT_LOADED] * len(self.names)
        return self

    def load(self, need=None, stream: Optional[torch.cuda.Stream] = None) -> int:
        """Returns the number of files loaded.  One descriptor is open at a
        time: the arena is laid out from the sizes ``stat`` took, and a file
        whose descriptor shows another size is not read."""
        wanted, at = {}, 0
        for j in range(len(self.names)):
            self._bases[j] = self.NOT_LOADED
            if (need is None or need[j]) and self._sizes[j] != self.UNKNOWN_SIZE:
                wanted[j] = at
                at += (self._sizes[j] + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        with _device._on(self.device, stream):
            self.arena = torch.empty(at, dtype=torch.uint8, device=self.device)
        for j, base in wanted.items():
            try:
                fd = os.open(self.root / self.names[j], os.O_RDONLY)
            except OSError:
                continue
            try:
                stamp = FileStamp()
                if lib().sf_file_stamp_fd(fd, stamp) != 0 or stamp.size != self._sizes[j]:
                    continue
                _device.read_fd(fd, stamp.size, 0, out=self.arena[base:base + stamp.size], stamp=stamp, stream=stream)
            except SfError as e:
                if e.code not in (SF_EAGAIN, SF_EIO):
                    raise
                continue
            finally:
                os.close(fd)
            self._bases[j] = base
        return len(self.names) - self._bases.count(self.NOT_LOADED)

    def bases(self) -> torch.Tensor:
        return torch.tensor(self._bases, dtype=torch.int64, device=self.device)

    def sizes(self) -> torch.Tensor:
        return torch.tensor(self._sizes, dtype=torch.int64, device=self.device)


class FileImages:
    """One HBM allocation that holds the image of every incoming temp file.

    ``sizes`` maps each temp file's name -- as the write lists spell it, e.g.
    ``temp_name("a.bin")`` -- to the size FILE_END fixed for it.  An image has
    exactly that size: it starts zero-filled at a 256-byte-aligned base of the
    allocation, so one ``copy_blocks`` call serves all files at once, and it
    never grows.  The zero fill runs on the stream that is current at
    construction; ``apply_copies``, ``apply_writes`` and ``write`` on another
    ``stream`` wait for it there.
    """

    ALIGN = 256

    def __init__(self, sizes: Mapping, device=None, root=None):
        self.device = _device.device_of(device)
        self.root = Path(root) if root is not None else None
        self._base: Dict[str, int] = {}
        self._size: Dict[str, int] = {}
        at = 0
        for name, size in sizes.items():
            size = int(size)
            if size < 0:
                raise ValueError(f"negative size for {name}")
            self._base[_name_str(name)] = at
            self._size[_name_str(name)] = size
            at += (size + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.buffer = torch.zeros(max(at, 1), dtype=torch.uint8, device=self.device)
        # the zero fill runs on the stream current here; a copy or a write on
        # another stream waits for it (_after_fill)
        self._filled = torch.cuda.Event()
        self._filled.record(torch.cuda.current_stream(self.device))
        self._local: Dict[str, torch.Tensor] = {}
        self._copied: Dict[str, set] = {}  # per image: the offsets apply_copies filled (present at FILE_END)

    def image(self, name) -> torch.Tensor:
        """The image of temp file ``name``: a view of the allocation."""
        key = _name_str(name)
        return self.buffer[self._base[key]: self._base[key] + self._size[key]]

    def _place(self, name, offset: int, size: int) -> int:
        """Where [offset, offset + size) of ``name`` lies in the allocation."""
        key = _name_str(name)
        if key not in self._base:
            raise KeyError(f"no image for {key}")
        if offset < 0 or size < 0 or offset + size > self._size[key]:
            raise ValueError(f"bytes [{offset}, {offset + size}) end past the {self._size[key]} bytes of {key}")
        return self._base[key] + offset

    def _after_fill(self, stream) -> None:
        """`stream` (None: the current one) ordered after the zero fill, and
        the allocation marked as in use on it."""
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        s.wait_event(self._filled)
        self.buffer.record_stream(s)

    def _copy(self, src: torch.Tensor, jobs: List[tuple], stream) -> None:
        """jobs = [(src_offset, dst_offset in the allocation, size)]."""
        if not jobs:
            return
        a = np.asarray(jobs, dtype=np.int64).reshape(-1, 3)
        self._after_fill(stream)
        with _device._on(self.device, stream):  # the lists belong to the stream the copy runs on
            so = torch.from_numpy(a[:, 0].copy()).to(self.device)
            do = torch.from_numpy(a[:, 1].copy()).to(self.device)
            sz = torch.from_numpy(a[:, 2].astype(np.uint32).view(np.int32)).to(self.device)
        _device.copy_blocks(src, self.buffer, so, do, sz, stream=stream)

    def apply_writes(self, writes, data, stream: Optional[torch.cuda.Stream] = None) -> int:
        """Carry out the write list ``Index.receive_block_data`` returned:
        ``data[data_start : data_start + size]`` goes to ``offset`` of ``name``
        for every (name, offset, data_start, size).  ``data`` is the same run,
        as an HBM tensor or as bytes -- bytes are uploaded here, once, although
        ``receive_block_data`` uploaded them before: the Python mirror accepts
        the second upload, the C-ABI path keeps one run in HBM.

        The reference writes in message order, so where two writes cover the
        same bytes the later one stays.  Exact duplicates of (name, offset,
        size) keep the last one; the rest is sorted on the host, and writes that
        still overlap an earlier one of the same call (only possible with
        ``verify=False``: a payload longer than its row) are put off to a
        further stream-ordered call, in list order, so the later one wins here
        too.  A write that ends past its file's size raises ValueError before
        anything is launched -- the reference would grow the file; an image
        has the size FILE_END fixed.  Returns the number of copy calls."""
        src = data if isinstance(data, torch.Tensor) else _device.upload(bytes(data), self.device)
        last: Dict[tuple, tuple] = {}
        for name, offset, start, size in writes:
            offset, start, size = int(offset), int(start), int(size)
            at = self._place(name, offset, size)
            if start < 0 or start + size > src.numel():
                raise ValueError(f"bytes [{start}, {start + size}) lie outside the run")
            key = (_name_str(name), offset, size)
            last.pop(key, None)  # the later one covers it whole, and keeps its own place in the order
            last[key] = (start, at, size)
        rounds = _rounds([j for j in last.values() if j[2]])
        for jobs in rounds:
            self._copy(src, jobs, stream)
        return len(rounds)

    def base(self, name) -> int:
        """Where byte 0 of temp file ``name`` lies in the allocation
        (``buffer``): a row's ``dst`` for ``device.place_block_data`` is this
        plus the row's offset."""
        return self._place(name, 0, 0)

    def bases(self, names) -> torch.Tensor:
        """``base(name)`` of every name, in order, as an int64 tensor on the
        images' device: ``device.plan_copies``' ``file_base``."""
        return torch.tensor([self.base(n) for n in names], dtype=torch.int64, device=self.device)

    def note_present(self, name, offsets) -> None:
        """The offsets of ``name``'s rows that were recorded as present when
        its FILE_END came, by a caller that filled them through ``apply_jobs``
        (``apply_copies`` notes its own): ``check`` chains the digests in the
        order that fixes."""
        self._copied.setdefault(_name_str(name), set()).update(int(o) for o in offsets)

    def apply_jobs(self, src: torch.Tensor, src_offsets: torch.Tensor, dst_offsets: torch.Tensor,
                   sizes: torch.Tensor, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Carry out a job list that is on the device already -- what
        ``device.place_block_data`` returned: ``src[src_offsets[k] : +
        sizes[k]]`` goes to ``dst_offsets[k]`` of the allocation.  One
        ``copy_blocks`` call and no host pass over the jobs: their
        destinations are disjoint because the rows they come from are.  A job
        outside ``src`` or the allocation is not copied and raises
        SfError(SF_ERANGE) (the kernel's status word, read back after the
        copy)."""
        if sizes.numel() == 0:
            return
        self._after_fill(stream)
        _device.copy_blocks(src, self.buffer, src_offsets, dst_offsets, sizes, check_range=True, stream=stream)

    def _read_local(self, from_name) -> torch.Tensor:
        key = _name_str(from_name)
        if key not in self._local:
            if self.root is None:
                raise ValueError("no root to read local files from: pass root= or source=")
            self._local[key] = _device.upload(np.fromfile(self.root / key, dtype=np.uint8).tobytes(), self.device)
        return self._local[key]

    def apply_copies(self, name, copies, source: Optional[Callable] = None,
                     stream: Optional[torch.cuda.Stream] = None) -> int:
        """Carry out the copy list ``Index.receive_file_blocks`` returned for
        temp file ``name``: [(from_name, from_offset, to_offset, size)], the
        blocks the destination already holds.  ``source(from_name)`` returns
        an HBM tensor of that local file; the default reads ``root /
        from_name`` with numpy and uploads it, cached per name -- plumbing, not
        a fast path (a loader for local files is not part of the library).
        One copy call per source file.  A copy that ends past the image raises
        ValueError before anything is launched.  Returns the number of
        calls."""
        source = source or self._read_local
        per: Dict[str, List[tuple]] = {}
        placed: List[int] = []
        for from_name, from_offset, to_offset, size in copies:
            at = self._place(name, int(to_offset), int(size))
            placed.append(int(to_offset))
            if int(size):
                per.setdefault(_name_str(from_name), []).append((int(from_offset), at, int(size)))
        for from_name, jobs in per.items():
            self._copy(source(from_name), jobs, stream)
        self._copied.setdefault(_name_str(name), set()).update(placed)
        return len(per)

    def check(self, index, name) -> List[int]:
        """Is the image the file the source announced?  The rows ``index``
        holds for temp file ``name`` (``list_file_blocks``) are hashed again
        over the image by the explicit-list kernel (``index_device_blocks``);
        returns the offsets of the rows whose digest differs, in row order.
        An empty list means every block is what its row says.  Then SHA-1 of
        the image's concatenated digests is also compared with
        ``files.blocks_hash`` where the index has one, and a difference raises
        ValueError.  That hash was chained at FILE_END over the rows as the
        index's query returned them then -- through the (file_id, present)
        index of the reference's schema: the blocks still missing first, then
        the ones found locally, each group in file order -- so the digests are
        chained in that order (the local ones are those ``apply_copies`` was
        given), and in plain file order and the query's present order as well;
        one of them must give the hash.  The reference never makes this check:
        it trusts every payload."""
        key = _name_str(name)
        row = index.db.execute("SELECT file_id, blocks_hash FROM files WHERE name = ?;", (key,)).fetchone()
        if not row:
            raise KeyError(f"the index has no file {key}")
        rows = index.list_file_blocks(int(row[0]))
        img = self.image(name)
        if not rows:
            return []
        for _h, offset, size in rows:
            if offset + size > img.numel():
                raise ValueError(f"row [{offset}, {offset + size}) ends past the {img.numel()} bytes of {key}")
        offsets = torch.tensor([r[1] for r in rows], dtype=torch.int64, device=self.device)
        sizes = torch.tensor([r[2] for r in rows], dtype=torch.int32, device=self.device)
        if img.numel():
            got = _device.index_device_blocks(img, offsets, sizes).cpu().numpy()
        else:  # rows of no bytes in a file of none
            got = np.tile(np.frombuffer(hashlib.sha1(b"").digest(), np.uint8), (len(rows), 1))
        empty = np.frombuffer(hashlib.sha1(b"").digest(), np.uint8)
        bad = []
        for k, (h, offset, size) in enumerate(rows):
            d = empty if size == 0 else got[k]
            if bytes(d) != h.bytes:
                bad.append(offset)
        if not bad and row[1] is not None:
            by_offset = sorted(range(len(rows)), key=lambda k: rows[k][1])
            local = self._copied.get(key, set())
            orders = ([k for k in by_offset if rows[k][1] not in local] + [k for k in by_offset if rows[k][1] in local],
                      by_offset, range(len(rows)))
            chained = {hashlib.sha1(b"".join(bytes(empty if rows[k][2] == 0 else got[k]) for k in order)).hexdigest()
                       for order in orders}
            if str(row[1]) not in chained:
                raise ValueError(f"blocks_hash of {key} is not that of the image's blocks")
        return bad

    def write(self, name, fd: int, stream: Optional[torch.cuda.Stream] = None) -> int:
        """The image of ``name`` written from byte 0 of the open file ``fd``
        (``device.write_to_fd``); returns the bytes written."""
        self._after_fill(stream)
        return _device.write_to_fd(self.image(name), fd, 0, stream=stream)
