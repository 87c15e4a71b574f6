"""The reference's wire messages for signature tables (src/sync/ssh/proto.rs).

``write_message`` mirrors proto.rs:139-187 byte for byte for the messages a
source sends about indexed files: FILE_ENTRY (name, size, blocks_hash),
END_FILES, FILE_START, FILE_BLOCK (digest, size), FILE_END, plus GET_FILE,
GET_BLOCK, BLOCK_DATA and COMPLETE.  ``file_blocks_device`` produces a whole
file's FILE_BLOCK run on the GPU straight from the HBM digest table
(C-ABI sf_wire_file_blocks_device), as FsSource streams it after FILE_START
(src/sync/fs.rs:217-233).  ``Parser`` is the receiving side (proto.rs:189-477):
the incremental framing parser a destination runs over the same bytes.
``block_data_device`` builds the source's BLOCK_DATA run on the GPU
(sf_wire_block_data_device) as a ``BlockDataRun``, which
``device.BlockSet.serve`` also returns for a received run of GET_BLOCK
requests.  ``files_device`` builds the source's whole answer to a list of
GET_FILE requests (sf_wire_files_device) as a ``FilesRun``."""
from __future__ import annotations

import ctypes
import re
from typing import List, Tuple

from ._lib import (SF_ENOSPC, SF_OK, SF_WIRE_END, SF_WIRE_INCOMPLETE, SF_WIRE_MALFORMED,  # noqa: F401
                   SF_WIRE_END_FILES, SF_WIRE_OTHER, SF_WIRE_UNEXPECTED, check, lib)
from ._lib import SF_SERVE_ALL, SF_SERVE_BAD_NAME, SF_SERVE_FULL, SF_SERVE_UNKNOWN  # noqa: F401
from .digest import HashDigest


def _d(d) -> bytes:
    return d.bytes if isinstance(d, HashDigest) else bytes(d)


def write_message(kind: str, *args) -> bytes:
    """One message, exactly as proto.rs:139-187 writes it."""
    if kind == "FileEntry":
        name, size, digest = args
        return b"FILE_ENTRY\n" + bytes(name) + b"\n%d\n" % size + _d(digest) + b"\n"
    if kind == "EndFiles":
        return b"END_FILES\n"
    if kind == "GetFile":
        return b"GET_FILE\n" + bytes(args[0]) + b"\n"
    if kind == "FileStart":
        return b"FILE_START\n" + bytes(args[0]) + b"\n"
    if kind == "FileBlock":
        digest, size = args
        return b"FILE_BLOCK\n" + _d(digest) + b"\n%d\n" % size
    if kind == "FileEnd":
        return b"FILE_END\n"
    if kind == "GetBlock":
        return b"GET_BLOCK\n" + _d(args[0]) + b"\n"
    if kind == "BlockData":
        digest, data = args
        return b"BLOCK_DATA\n" + _d(digest) + b"\n%d\n" % len(data) + bytes(data) + b"\n"
    if kind == "Complete":
        return b"COMPLETE\n"
    raise ValueError(kind)


class ProtocolError(ValueError):
    """proto::Error: the byte stream is not a valid message sequence."""


# Framing limits of the reference parser (proto.rs:249-251).
COMMAND_MAX, FILENAME_MAX, SIZE_MAX = 20, 100, 15
_USIZE = re.compile(rb"\+?[0-9]+")  # what Rust's usize::from_str accepts


class Parser:
    """Incremental message parser, the receiving side of write_message
    (proto.rs:189-477).  ``receive(data)`` appends bytes and returns every
    message now complete, as (kind, *fields) tuples in write_message's
    argument order; an incomplete tail is kept for the next call.  Malformed
    input raises ProtocolError with the reference's message: a line longer
    than its limit (command 20, filename 100, size 15 bytes), a digest or
    data field not followed by a newline, a size that is not a usize, an
    unknown command."""

    def __init__(self):
        self._buf = bytearray()

    def receive(self, data) -> List[Tuple]:
        self._buf += bytes(data)
        out, pos = [], 0
        while True:
            r = self._one(pos)
            if r is None:
                break
            msg, pos = r
            out.append(msg)
        del self._buf[:pos]
        return out

    def _line(self, p, limit, err):
        i = self._buf.find(b"\n", p, min(len(self._buf), p + limit + 1))
        if i >= 0:
            return bytes(self._buf[p:i]), i + 1
        if len(self._buf) - p >= limit:
            raise ProtocolError(err)
        return None

    def _exact(self, p, n, err):
        if len(self._buf) - p < n + 1:
            return None
        if self._buf[p + n] != 0x0A:
            raise ProtocolError(err)
        return bytes(self._buf[p:p + n]), p + n + 1

    @staticmethod
    def _usize(b, err):
        if not _USIZE.fullmatch(b) or int(b) >= 1 << 64:
            raise ProtocolError(err)
        return int(b)

    def _one(self, p):
        if p >= len(self._buf):
            return None
        r = self._line(p, COMMAND_MAX, "Unterminated command")
        if r is None:
            return None
        cmd, p = r
        if cmd in (b"END_FILES", b"FILE_END", b"COMPLETE"):
            return ({b"END_FILES": ("EndFiles",), b"FILE_END": ("FileEnd",), b"COMPLETE": ("Complete",)}[cmd], p)
        if cmd in (b"GET_FILE", b"FILE_START"):
            r = self._line(p, FILENAME_MAX, "Unterminated filename")
            if r is None:
                return None
            return ("GetFile" if cmd == b"GET_FILE" else "FileStart", r[0]), r[1]
        if cmd == b"FILE_ENTRY":
            r = self._line(p, FILENAME_MAX, "Unterminated filename")
            if r is None:
                return None
            name, p = r
            r = self._line(p, SIZE_MAX, "Unterminated size")
            if r is None:
                return None
            size = self._usize(r[0], "Invalid file size")
            r = self._exact(r[1], 20, "Unterminated digest")
            if r is None:
                return None
            return ("FileEntry", name, size, HashDigest(r[0])), r[1]
        if cmd in (b"FILE_BLOCK", b"GET_BLOCK", b"BLOCK_DATA"):
            r = self._exact(p, 20, "Unterminated digest")
            if r is None:
                return None
            digest, p = HashDigest(r[0]), r[1]
            if cmd == b"GET_BLOCK":
                return ("GetBlock", digest), p
            r = self._line(p, SIZE_MAX, "Unterminated size" if cmd == b"FILE_BLOCK" else "Unterminated length")
            if r is None:
                return None
            size = self._usize(r[0], "Invalid block size" if cmd == b"FILE_BLOCK" else "Invalid block length")
            if cmd == b"FILE_BLOCK":
                return ("FileBlock", digest, size), r[1]
            r = self._exact(r[1], size, "Invalid data end byte")
            if r is None:
                return None
            return ("BlockData", digest, r[0]), r[1]
        raise ProtocolError("Unknown command")


def _device(t, name: str):
    """torch and .device, imported on first use (``Parser`` and
    ``write_message`` need neither), once ``t`` is seen to be a contiguous
    uint8 HBM tensor."""
    import torch

    from . import device
    device._require_device(t, name, torch.uint8)
    return torch, device


def _stream(torch, t) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _build_run(torch, name: str, digests, middle: tuple):
    """A FILE_BLOCK run as a new uint8 HBM tensor: the entry point ``name``
    called (digests, *middle, out, cap, &need, stream), once without buffers
    for the need and once to fill.  Call inside ``_on``."""
    fn, need, s = getattr(lib(), name), ctypes.c_uint64(0), _stream(torch, digests)
    rc = fn(None, *middle, None, 0, ctypes.byref(need), s)
    if rc not in (SF_OK, SF_ENOSPC):
        check(rc, name)
    out = torch.empty(need.value, dtype=torch.uint8, device=digests.device)
    if need.value:
        check(fn(digests.data_ptr(), *middle, out.data_ptr(), out.numel(), ctypes.byref(need), s), name)
    return out


def file_blocks_device(digests, block_size: int, file_len: int, stream=None):
    """FILE_BLOCK messages for every block of a fixed-tiled file, built on the
    device from a uint8[n, 20] HBM digest table -> uint8 HBM tensor."""
    torch, dev = _device(digests, "digests")
    with dev._on(digests.device, stream):
        return _build_run(torch, "sf_wire_file_blocks_device", digests, (digests.shape[0], block_size, file_len))


def _check_sizes(torch, sizes, digests):
    if (not isinstance(sizes, torch.Tensor) or sizes.numel() != digests.shape[0]
            or sizes.dtype not in (torch.int32, torch.uint32) or sizes.device != digests.device):
        raise ValueError("sizes must be one 32-bit size per digest, on the digests' device")


def blocks_device(digests, sizes, stream=None):
    """FILE_BLOCK messages for an explicit block list (content-defined
    blocks, each with its own size), built on the device from a uint8[n, 20]
    HBM digest table and an int32/uint32[n] HBM size array (bit pattern taken
    as uint32) -> uint8 HBM tensor (sf_wire_blocks_device)."""
    torch, dev = _device(digests, "digests")
    n = digests.shape[0]
    _check_sizes(torch, sizes, digests)
    with dev._on(digests.device, stream):
        sizes = sizes.contiguous()  # on the stream the kernels run on
        return _build_run(torch, "sf_wire_blocks_device", digests, (dev._ptr(sizes, n), n))


def parse_blocks_device(run, stream=None):
    """The inverse of ``blocks_device``: the FILE_BLOCK messages at the start
    of ``run``, a uint8 HBM tensor, parsed on the device
    (sf_wire_parse_blocks_device) -> (digests uint8[n, 20], sizes uint32[n],
    consumed, stop).  The n messages are exactly those ``Parser`` reads from
    byte 0 until something else stands there; ``consumed`` is their bytes and
    ``stop`` says what stands at ``run[consumed:]``: SF_WIRE_END (nothing),
    SF_WIRE_INCOMPLETE (the start of a message), SF_WIRE_OTHER (another
    command's complete line: FILE_END, FILE_START, ...) or SF_WIRE_MALFORMED
    (``Parser`` would raise there).  A size above 2^32 - 1 raises SfError
    (SF_ERANGE).  Blocking."""
    torch, dev = _device(run, "run")
    if run.dim() != 1:
        raise ValueError("run must be a flat uint8 tensor")
    n, consumed, stop = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
    with dev._on(run.device, stream):
        cap, digests, sizes = dev._receive_outputs(run, False)
        check(lib().sf_wire_parse_blocks_device(dev._ptr(run), run.numel(), digests.data_ptr(), sizes.data_ptr(), cap,
                                                ctypes.byref(n), ctypes.byref(consumed), ctypes.byref(stop),
                                                _stream(torch, run)), "sf_wire_parse_blocks_device")
    return digests[:n.value], sizes[:n.value].view(torch.uint32), consumed.value, stop.value


def parse_stats():
    """Test hook (sf_test_wire_parse_stats): (candidates, messages, whether the
    host fallback ran, 0) of this process's last FILE_BLOCK parse."""
    out = (ctypes.c_uint64 * 4)()
    check(lib().sf_test_wire_parse_stats(out), "sf_test_wire_parse_stats")
    return tuple(int(v) for v in out)


def recv_files_stats():
    """Test hook (sf_test_recv_files_stats): (candidates, accepted messages,
    whether the host fallback ran, 0) of this process's last
    ``device.BlockSet.receive_files`` / sf_receive_files_device."""
    out = (ctypes.c_uint64 * 4)()
    check(lib().sf_test_recv_files_stats(out), "sf_test_recv_files_stats")
    return tuple(int(v) for v in out)


def receive_block_data_device(run, verify: bool = True, stream=None):
    """A received run of BLOCK_DATA messages, parsed and verified on the
    device (sf_receive_block_data_device): the messages ``Parser`` reads from
    byte 0 of ``run``, a uint8 HBM tensor, until something else stands there
    -> (digests uint8[n, 20] as claimed, sizes uint32[n], data_offsets
    int64[n] of the payloads in ``run``, ok uint8[n], consumed, stop, need).
    ``ok[i]`` is 1 when payload i's SHA-1 is the digest its message claims --
    the check the reference leaves out (src/sync/fs.rs:505-510); with
    ``verify=False`` nothing is hashed and ``ok`` is None.  ``stop`` is the
    SF_WIRE_* class of what stands at ``run[consumed:]``; with
    SF_WIRE_INCOMPLETE after a whole header, ``need`` is that message's full
    length, else 0.  Payloads may hold messages of their own: the result is
    the reference parser's for any input.  Blocking."""
    torch, dev = _device(run, "run")
    if run.dim() != 1:
        raise ValueError("run must be a flat uint8 tensor")
    n, consumed, stop = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
    need, n_bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    with dev._on(run.device, stream):
        cap = run.numel() // 35 + 1  # a message is at least 35 bytes
        digests = torch.empty((cap, 20), dtype=torch.uint8, device=run.device)
        sizes = torch.empty(cap, dtype=torch.int32, device=run.device)
        offsets = torch.empty(cap, dtype=torch.int64, device=run.device)
        ok = torch.empty(cap, dtype=torch.uint8, device=run.device) if verify else None
        check(lib().sf_receive_block_data_device(dev._ptr(run), run.numel(), digests.data_ptr(), sizes.data_ptr(),
                                                 offsets.data_ptr(), dev._ptr(ok), cap, ctypes.byref(n),
                                                 ctypes.byref(consumed), ctypes.byref(stop), ctypes.byref(need),
                                                 ctypes.byref(n_bad), _stream(torch, run)),
              "sf_receive_block_data_device")
    k = n.value
    return (digests[:k], sizes[:k].view(torch.uint32), offsets[:k], ok[:k] if verify else None, consumed.value,
            stop.value, need.value)


def block_data_stats():
    """Test hook (sf_test_block_data_stats): (candidates, messages, 1 if the
    host walked the candidate list, list bytes copied back for it) of this
    process's last BLOCK_DATA parse."""
    out = (ctypes.c_uint64 * 4)()
    check(lib().sf_test_block_data_stats(out), "sf_test_block_data_stats")
    return tuple(int(v) for v in out)


class BlockDataRun:
    """A run of BLOCK_DATA messages built in HBM and owned by the library
    (sf_wire_run): what ``block_data_device`` and ``device.BlockSet.serve``
    return.  ``nbytes`` / ``n_messages`` / ``data_ptr`` describe it; the bytes
    are complete once the building stream has run past the build, and every
    method here waits for that or runs on that stream.  ``close()`` (also on
    leaving a ``with`` block, and when the object is dropped) gives the memory
    back, stream-ordered."""

    def __init__(self, handle, device, stream=None):
        self._h, self.device, self.stream = handle, device, stream
        p, nb, nm = ctypes.c_void_p(), ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(lib().sf_wire_run_info(self._h, ctypes.byref(p), ctypes.byref(nb), ctypes.byref(nm)), "sf_wire_run_info")
        self.data_ptr, self.nbytes, self.n_messages = p.value or 0, nb.value, nm.value

    def _open(self):
        if not self._h:
            raise ValueError("BlockDataRun is closed")

    def bytes(self, offset: int = 0, length: int = None) -> bytes:
        """``length`` bytes of the run from ``offset`` (default: all), copied
        to the host (sf_wire_run_read)."""
        self._open()
        length = self.nbytes - offset if length is None else length
        buf = ctypes.create_string_buffer(max(length, 1))
        check(lib().sf_wire_run_read(self._h, offset, buf, length), "sf_wire_run_read")
        return buf.raw[:length]

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.data_ptr, False), "version": 2,
                "strides": None}

    def tensor(self):
        """The run as a uint8 HBM tensor: a view of the library's memory
        through ``__cuda_array_interface__``, valid until ``close()`` (the
        tensor keeps this object alive)."""
        import torch
        self._open()
        if self.nbytes == 0:
            return torch.empty(0, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            return torch.as_tensor(self, device=self.device)

    def receive(self, verify: bool = True):
        """The run handed straight to ``receive_block_data_device``, on the
        stream it was built on."""
        return receive_block_data_device(self.tensor(), verify=verify, stream=self.stream)

    def to_fd(self, fd: int) -> int:
        """The run written to ``fd`` with write() through the pinned stages
        (sf_wire_run_to_fd); a pipe works.  Returns the bytes written; a failed
        write raises SfError(SF_EIO) whose ``written`` attribute holds the
        bytes known written."""
        self._open()
        nw = ctypes.c_uint64(0)
        rc = lib().sf_wire_run_to_fd(self._h, int(fd), ctypes.byref(nw))
        if rc != SF_OK:
            from ._lib import SfError
            err = SfError(rc, "sf_wire_run_to_fd")
            err.written = nw.value
            raise err
        return nw.value

    def close(self) -> None:
        if self._h:
            h, self._h = self._h, None
            if self.data_ptr:
                from . import device
                import torch
                with device._on(self.device, self.stream):
                    check(lib().sf_wire_run_free(h, torch.cuda.current_stream(self.device).cuda_stream),
                          "sf_wire_run_free")
            else:
                check(lib().sf_wire_run_free(h, None), "sf_wire_run_free")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def block_data_device(src, digests, src_offsets, sizes, stream=None) -> BlockDataRun:
    """The BLOCK_DATA run of an explicit job list, built on the device
    (sf_wire_block_data_device): message i carries ``src[src_offsets[i] : +
    sizes[i]]`` under ``digests[i]``, byte for byte what ``write_message``
    gives.  ``src`` uint8, ``digests`` uint8[n, 20], ``src_offsets`` int64[n]
    and ``sizes`` int32/uint32[n] (bit pattern taken as uint32) are HBM
    tensors on one device.  A job outside ``src`` raises SfError(SF_ERANGE)
    and nothing is built.  Blocking, for one read-back."""
    torch, dev = _device(src, "src")
    dev._require_device(digests, "digests", torch.uint8, src.device)
    dev._require_device(src_offsets, "src_offsets", torch.int64, src.device)
    n = digests.shape[0]
    _check_sizes(torch, sizes, digests)
    if src_offsets.numel() != n:
        raise ValueError("src_offsets and sizes differ in length")
    h = ctypes.c_void_p()
    with dev._on(src.device, stream):
        sizes = sizes.contiguous()
        # the library wants a buffer even when every size is 0
        buf = src if src.numel() else torch.empty(1, dtype=torch.uint8, device=src.device)
        check(lib().sf_wire_block_data_device(buf.data_ptr(), src.numel(), dev._ptr(digests, n),
                                              dev._ptr(src_offsets, n), dev._ptr(sizes, n), n, ctypes.byref(h),
                                              _stream(torch, src)), "sf_wire_block_data_device")
    return BlockDataRun(h, src.device, stream)


class FilesRun(BlockDataRun):
    """A whole GetFiles answer built in HBM (``files_device``,
    ``Index.serve_get_files``): FILE_START, FILE_BLOCKs and FILE_END of file
    after file in one library-owned run.  ``BlockDataRun`` in everything but
    what ``receive`` does with it."""

    def receive(self, block_set=None, open: bool = False, base_offset: int = 0):
        """The run handed straight to ``device.BlockSet.receive_files``
        (sf_receive_files_device) -- the destination's half of the exchange --
        and its ``FilesReceived``.  ``block_set`` None: a set of no rows, so
        every block comes back not found (rows -1)."""
        from . import device
        import torch
        run = self.tensor()
        if block_set is not None:
            return block_set.receive_files(run, open=open, base_offset=base_offset)
        with device.BlockSet(torch.empty((0, 20), dtype=torch.uint8, device=self.device), stream=self.stream) as none:
            return none.receive_files(run, open=open, base_offset=base_offset)


def files_device(digests, sizes, file_first, names, name_at, stream=None) -> FilesRun:
    """The source's answer to a list of GET_FILE requests, built on the device
    in one call (sf_wire_files_device): for file f ``write_message("FileStart",
    name)``, one ``write_message("FileBlock", digest, size)`` per block and
    ``write_message("FileEnd")``, file after file, byte for byte.  ``digests``
    uint8[n, 20] and ``sizes`` int32/uint32[n] (bit pattern taken as uint32)
    hold the blocks of all files in answer order; ``file_first`` int64[m + 1]
    is the CSR into them (file f owns blocks ``file_first[f]:file_first[f +
    1]``), ``names`` uint8 the packed name bytes and ``name_at`` int64[m + 1]
    the CSR into those.  All are HBM tensors on one device.  A broken CSR, or a
    name the protocol cannot carry (over 100 bytes, or holding a newline),
    raises ValueError naming the first such file, and nothing is built.
    Blocking, for one read-back."""
    torch, dev = _device(digests, "digests")
    d = digests.device
    if digests.dim() != 2 or digests.shape[1] != 20:
        raise ValueError("digests must be uint8[n, 20]")
    n = digests.shape[0]
    _check_sizes(torch, sizes, digests)
    dev._require_device(file_first, "file_first", torch.int64, d)
    dev._require_device(names, "names", torch.uint8, d)
    dev._require_device(name_at, "name_at", torch.int64, d)
    m = file_first.numel() - 1
    if m < 0 or name_at.numel() != m + 1 or file_first.dim() != 1 or name_at.dim() != 1 or names.dim() != 1:
        raise ValueError("file_first and name_at must be flat and hold one entry per file and one more")
    h, bad = ctypes.c_void_p(), ctypes.c_uint64(0)
    with dev._on(d, stream):
        sizes = sizes.contiguous()
        rc = lib().sf_wire_files_device(dev._ptr(digests, n), dev._ptr(sizes, n), n, file_first.data_ptr(),
                                        dev._ptr(names), name_at.data_ptr(), m, ctypes.byref(h), ctypes.byref(bad),
                                        _stream(torch, digests))
    if rc != SF_OK and bad.value != (1 << 64) - 1:
        raise ValueError(f"file {bad.value}: its block or name entries do not hold, or its name is over "
                         f"{FILENAME_MAX} bytes or holds a newline")
    check(rc, "sf_wire_files_device")
    return FilesRun(h, d, stream)


class EntriesRun(BlockDataRun):
    """A files list built in HBM (``file_entries_device``,
    ``Index.file_entries``): FILE_ENTRY after FILE_ENTRY and END_FILES in one
    library-owned run.  ``BlockDataRun`` in everything but what ``receive``
    does with it."""

    def receive(self, name_set=None, have_hashes=None, have_hash_ok=None):
        """The run handed straight to ``device.receive_file_entries``
        (sf_receive_file_entries_device) -- the destination's half of the
        exchange -- and its ``EntriesReceived``."""
        from . import device
        return device.receive_file_entries(self.tensor(), name_set, have_hashes, have_hash_ok,
                                           stream=None if name_set is not None else self.stream)


class GetFilesRun(BlockDataRun):
    """The destination's GET_FILE requests built in HBM (``get_files_device``,
    ``Index.receive_file_entries``).  ``BlockDataRun``, but ``receive`` has no
    device route yet: the source parses the requests with ``Parser``."""

    def receive(self, *args, **kwargs):
        return Parser().receive(self.bytes())

    def serve(self, name_set, file_first, digests, sizes, max_run_bytes: int = 0):
        """The run handed straight to ``device.NameSet.serve_files``
        (sf_serve_get_files_device) on the source's tables -- the source's half
        of the exchange, what ``EntriesRun.receive`` is for the list -- and its
        ``device.FilesServed``."""
        return name_set.serve_files(self.tensor(), file_first, digests, sizes, max_run_bytes=max_run_bytes)


def parse_get_files_device(run, stream=None):
    """The inverse of ``get_files_device``: the GET_FILE messages at the start
    of ``run``, a flat uint8 HBM tensor, parsed on the device
    (sf_wire_parse_get_files_device) -> (name_at int64[n], name_len int32[n],
    bad_name, consumed, stop).  The n requests are exactly those ``Parser``
    reads from byte 0 until something else stands there; request i's name is
    ``run[name_at[i] : + name_len[i]]`` -- the spans ``device.NameSet.lookup``
    takes -- ``bad_name`` the first request whose name is not UTF-8, or None;
    ``consumed`` / ``stop`` as ``parse_blocks_device``.  Blocking."""
    torch, dev = _device(run, "run")
    if run.dim() != 1:
        raise ValueError("run must be a flat uint8 tensor")
    n, bad, consumed, stop = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
    cap = run.numel() // 10 + 1  # a request is at least 10 bytes
    with dev._on(run.device, stream):
        name_at = torch.empty(cap, dtype=torch.int64, device=run.device)
        name_len = torch.empty(cap, dtype=torch.int32, device=run.device)
        check(lib().sf_wire_parse_get_files_device(dev._ptr(run), run.numel(), name_at.data_ptr(), name_len.data_ptr(),
                                                   cap, ctypes.byref(n), ctypes.byref(bad), ctypes.byref(consumed),
                                                   ctypes.byref(stop), _stream(torch, run)),
              "sf_wire_parse_get_files_device")
    return (name_at[:n.value], name_len[:n.value], None if bad.value == (1 << 64) - 1 else bad.value, consumed.value,
            stop.value)


def file_entries_device(names, name_at, sizes, hashes, end_files: bool = True, stream=None) -> EntriesRun:
    """The source's files list, built on the device in one call
    (sf_wire_file_entries_device): for file f ``write_message("FileEntry",
    name, size, hash)``, file after file, and ``write_message("EndFiles")``
    behind them with ``end_files``, byte for byte.  ``names`` uint8 the packed
    name bytes, ``name_at`` int64[n + 1] the CSR into them
    (``device.pack_names``), ``sizes`` int64[n], ``hashes`` uint8[n, 20]: HBM
    tensors on one device.  A broken CSR, a name the protocol cannot carry (over
    100 bytes, or holding a newline) or a size of 10^15 or more raises
    ValueError naming the first such file, and nothing is built.  Blocking, for
    one read-back."""
    torch, dev = _device(names, "names")
    d = names.device
    dev._require_device(name_at, "name_at", torch.int64, d)
    dev._require_device(sizes, "sizes", torch.int64, d)
    dev._require_device(hashes, "hashes", torch.uint8, d)
    n = name_at.numel() - 1
    if n < 0 or names.dim() != 1 or name_at.dim() != 1 or sizes.numel() != n or hashes.numel() != 20 * n:
        raise ValueError("name_at holds one entry per file and one more, sizes one and hashes 20 bytes per file")
    h, bad = ctypes.c_void_p(), ctypes.c_uint64(0)
    with dev._on(d, stream):
        rc = lib().sf_wire_file_entries_device(dev._ptr(names), name_at.data_ptr(), dev._ptr(sizes, n),
                                               dev._ptr(hashes, n), n, int(bool(end_files)), ctypes.byref(h),
                                               ctypes.byref(bad), _stream(torch, names))
    if rc != SF_OK and bad.value != (1 << 64) - 1:
        raise ValueError(f"file {bad.value}: its name entries do not hold, its name is over {FILENAME_MAX} bytes or "
                         f"holds a newline, or its size has more than {SIZE_MAX} digits")
    check(rc, "sf_wire_file_entries_device")
    return EntriesRun(h, d, stream)


def get_files_device(data, name_at, name_len, pick=None, stream=None) -> GetFilesRun:
    """The destination's request run, built on the device in one call
    (sf_wire_get_files_device): ``write_message("GetFile", name)`` of the
    names ``data[name_at[i] : + name_len[i]]`` for i in ``pick`` (int32/uint32,
    in that order, repeats allowed; None: every span in order) -- ``data`` the
    received list as a flat uint8 HBM tensor, the spans as
    ``device.receive_file_entries`` returns them, ``pick`` its ``need_list``.
    An index outside the spans, a span that leaves ``data`` or a name the
    protocol cannot carry raises ValueError naming the first such pick.
    Blocking, for one read-back."""
    torch, dev = _device(data, "data")
    d = data.device
    n = name_at.numel()
    dev._list64(name_at, "name_at", n, d)
    dev._list32(name_len, "name_len", n, d)
    if pick is not None:
        dev._list32(pick, "pick", pick.numel(), d)
    h, bad = ctypes.c_void_p(), ctypes.c_uint64(0)
    with dev._on(d, stream):
        # the library wants an array for an explicit pick of nothing
        p = None if pick is None else (pick if pick.numel() else torch.zeros(1, dtype=torch.int32, device=d))
        rc = lib().sf_wire_get_files_device(dev._ptr(data), data.numel(), dev._ptr(name_at), dev._ptr(name_len), n,
                                            None if p is None else p.data_ptr(), 0 if pick is None else pick.numel(),
                                            ctypes.byref(h), ctypes.byref(bad), _stream(torch, data))
    if rc != SF_OK and bad.value != (1 << 64) - 1:
        raise ValueError(f"pick {bad.value}: its index or its span is out of range, or its name is over "
                         f"{FILENAME_MAX} bytes or holds a newline")
    check(rc, "sf_wire_get_files_device")
    return GetFilesRun(h, d, stream)


def file_entries_stats():
    """Test hook (sf_test_file_entries_stats): see ``device.file_entries_stats``."""
    from . import device
    return device.file_entries_stats()


def blocks_to_fd(digests, sizes, fd: int, stream=None) -> int:
    """The explicit list's FILE_BLOCK run written to a file descriptor, built
    on the device in chunks and streamed back (sf_wire_blocks_fd).  Returns
    the bytes written."""
    torch, dev = _device(digests, "digests")  # an HBM table: the kernels read it on its device
    n = digests.shape[0]
    _check_sizes(torch, sizes, digests)
    out = ctypes.c_uint64(0)
    # the library's streams and chunk buffers are the current device's
    # (HostLease keys on hipGetDevice): enter the digests' device
    with dev._on(digests.device, stream):
        sizes = sizes.contiguous()  # on the stream the chunks are built after
        check(lib().sf_wire_blocks_fd(dev._ptr(digests, n), dev._ptr(sizes, n), n, int(fd), ctypes.byref(out),
                                      _stream(torch, digests)), "sf_wire_blocks_fd")
    return out.value


def file_blocks_to_fd(digests, block_size: int, file_len: int, fd: int, stream=None) -> int:
    """The FILE_BLOCK run of a fixed-tiled file written to a file descriptor
    (an SSH pipe or a file): built on the device in chunks, streamed back by
    DMA and written while the next chunk is built (sf_wire_file_blocks_fd).
    Returns the bytes written."""
    torch, dev = _device(digests, "digests")
    n = digests.shape[0]
    out = ctypes.c_uint64(0)
    with dev._on(digests.device, stream):
        check(lib().sf_wire_file_blocks_fd(dev._ptr(digests, n), n, block_size, file_len, fd, ctypes.byref(out),
                                           _stream(torch, digests)), "sf_wire_file_blocks_fd")
    return out.value
