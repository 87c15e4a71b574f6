"""Device-resident entry points over torch tensors (HBM buffers).

PyTorch is only plumbing here: it owns the HBM allocations and the stream.
Every compute call goes to a HIP kernel through the C-ABI
(``include/syncfast_amd.h``); tensors must live on a ROCm device.

Reference mapping (/root/reference):
  index_device          -> the chunk loop of Index::index_file, src/index.rs:621-647
                           (fixed-size blocks)
  index_device_blocks   -> the same loop for an explicit boundary list
                           (the reference's CDC boundaries, src/index.rs:622-625)
  index_device_batch    -> index_path_rec over many files (src/index.rs:689-715)
                           + compute_blocks_hash per file (src/index.rs:661-682)
  cut_device_zpaq       -> the reference's own chunker (cdchunking's ZPAQ,
                           src/index.rs:622-625) cut on the device
  index_device_zpaq     -> index_file's default mode end to end in HBM
  cut_zpaq_files / index_zpaq_files -> the same for many files of one buffer
                           in one call (index_path_rec's default mode)
"""
from __future__ import annotations

import contextlib
import ctypes
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import SF_ENOSPC, SF_ERANGE, ChainJob, FileDesc, SfError, check, lib, num_blocks, retry_enospc

__all__ = [
    "num_blocks", "index_device", "index_device_blocks", "index_device_batch",
    "index_device_weak", "index_device_blocks_weak", "BatchStream",
    "fill_splitmix", "splitmix_tensor", "BlockSet", "index_device_multi",
    "cut_device_zpaq", "index_device_zpaq", "zpaq_segment_len", "zpaq_device_stats",
    "cut_zpaq_files", "index_zpaq_files", "zpaq_files_stats", "ZpaqFiles",
    "copy_blocks", "copy_stats", "write_to_fd", "get_block_requests", "place_block_data",
    "device_of", "upload", "NameSet", "EntriesReceived", "receive_file_entries", "pack_names", "file_entries_stats",
    "FilesServed", "serve_files_stats", "read_fd", "plan_copies", "plan_copies_stats", "CopyPlan", "PlanCounts",
]


def _require_device(t: torch.Tensor, name: str, dtype=None, device: Optional[torch.device] = None) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must be on a ROCm device (got {t.device}); syncfast_amd has no CPU path")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, the input on {device}")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def device_of(device=None) -> torch.device:
    """``device`` as a torch.device; None: the current ROCm device."""
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def upload(data, device=None) -> torch.Tensor:
    """Bytes as a flat uint8 HBM tensor on ``device`` (``device_of``): a
    received buffer, a local file's bytes, a digest list."""
    dev = device_of(device)
    if not data:
        return torch.empty(0, dtype=torch.uint8, device=dev)
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)


def _stream_ptr(t: torch.Tensor, stream: Optional[torch.cuda.Stream]) -> int:
    s = stream if stream is not None else torch.cuda.current_stream(t.device)
    return s.cuda_stream


@contextlib.contextmanager
def _on(device: torch.device, stream: Optional[torch.cuda.Stream]):
    """`device` current and, if given, `stream` its current stream: outputs
    and status words are then allocated, zeroed and read back on the stream
    the kernel runs on (a status word zeroed or read on another stream races
    with the kernel that writes it)."""
    with torch.cuda.device(device):
        if stream is None:
            yield
        else:
            with torch.cuda.stream(stream):
                yield


def _ptr(t: Optional[torch.Tensor], n: Optional[int] = None) -> Optional[int]:
    """The address the library gets for ``t``: NULL for None and for nothing
    to read or write (``n`` elements of it in use; default: all it has)."""
    return t.data_ptr() if t is not None and (t.numel() if n is None else n) else None


def _out(out: Optional[torch.Tensor], name: str, shape: tuple, dtype, data: torch.Tensor) -> torch.Tensor:
    """An output of ``shape`` on the input's device: a new tensor, or the
    caller's once it is seen to be there, of that dtype, contiguous, large
    enough and 4-byte aligned (digest tables, hashes and weak sums are written
    as 32-bit words: include/syncfast_amd.h; a uint8 view may start anywhere).
    Call inside ``_on``: the allocation belongs to the launch stream."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=data.device)
    _require_device(out, name, dtype, data.device)
    need = math.prod(shape)
    if out.numel() < need:
        raise ValueError(f"{name} holds {out.numel()} elements, need {need}")
    if out.data_ptr() % 4:
        raise ValueError(f"{name} must start 4-byte aligned (it starts {out.data_ptr() % 4} bytes past)")
    return out


def _index_fixed(data, block_size, out, weak_out, stream, weak: bool):
    """sf_index_device_fixed / _fixed_weak: the weak form has one more output
    and the smaller of the two capacities."""
    _require_device(data, "data", torch.uint8)
    n = num_blocks(data.numel(), block_size)
    name = "sf_index_device_fixed_weak" if weak else "sf_index_device_fixed"
    with _on(data.device, stream):
        out = _out(out, "out", (n, 20), torch.uint8, data)
        outs, cap = (_ptr(out, n),), out.numel() // 20
        if weak:
            weak_out = _out(weak_out, "weak_out", (n,), torch.int32, data)
            outs, cap = outs + (_ptr(weak_out, n),), min(cap, weak_out.numel())
        nb = ctypes.c_uint64(0)
        check(getattr(lib(), name)(_ptr(data), data.numel(), block_size, *outs, cap, ctypes.byref(nb),
                                   _stream_ptr(data, stream)), name)
    return out, weak_out


def index_device(data: torch.Tensor, block_size: int, out: Optional[torch.Tensor] = None,
                 stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """SHA-1 of every fixed-size block of a uint8 HBM buffer -> uint8[n, 20]."""
    return _index_fixed(data, block_size, out, None, stream, False)[0]


def index_device_weak(data: torch.Tensor, block_size: int, out: Optional[torch.Tensor] = None,
                      weak_out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None):
    """index_device plus the opt-in weak sum: (digests uint8[n, 20], weak
    int32[n]) where weak[i] is the zlib Adler-32 of block i (bit pattern of
    the uint32), fused into the same kernel pass.  Not in the reference
    (SURVEY.md 8a row a8)."""
    return _index_fixed(data, block_size, out, weak_out, stream, True)


def _index_blocks(data, offsets, sizes, out, check_range, stream, weak: bool):
    """sf_index_device_blocks / _blocks_weak."""
    _require_device(data, "data", torch.uint8)
    _require_device(offsets, "offsets", torch.int64, data.device)
    _require_device(sizes, "sizes", torch.int32, data.device)
    n = offsets.numel()
    if sizes.numel() != n:
        raise ValueError("offsets and sizes differ in length")
    name = "sf_index_device_blocks_weak" if weak else "sf_index_device_blocks"
    with _on(data.device, stream):
        out = _out(out, "out", (n, 20), torch.uint8, data)
        wk = torch.empty(n, dtype=torch.int32, device=data.device) if weak else None
        if n == 0:
            return out, wk
        status = torch.zeros(1, dtype=torch.int32, device=data.device) if check_range else None
        outs = (out.data_ptr(), wk.data_ptr()) if weak else (out.data_ptr(),)
        check(getattr(lib(), name)(_ptr(data), data.numel(), offsets.data_ptr(), sizes.data_ptr(), n, *outs,
                                   _ptr(status), _stream_ptr(data, stream)), name)
        if status is not None and int(status.item()) != 0:
            raise SfError(SF_ERANGE, name)
    return out, wk


def index_device_blocks(data: torch.Tensor, offsets: torch.Tensor, sizes: torch.Tensor,
                        out: Optional[torch.Tensor] = None, check_range: bool = True,
                        stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """SHA-1 of explicit blocks data[offsets[i] : offsets[i] + sizes[i]].

    ``offsets`` int64 and ``sizes`` int32 tensors on the same device.  With
    ``check_range`` a block outside the buffer raises SfError(SF_ERANGE)
    (this synchronises the stream)."""
    return _index_blocks(data, offsets, sizes, out, check_range, stream, False)[0]


def index_device_blocks_weak(data: torch.Tensor, offsets: torch.Tensor, sizes: torch.Tensor,
                             check_range: bool = True, stream: Optional[torch.cuda.Stream] = None):
    """index_device_blocks plus the opt-in Adler-32 per block (0 for a block
    outside the buffer) -> (digests uint8[n, 20], weak int32[n])."""
    return _index_blocks(data, offsets, sizes, None, check_range, stream, True)


def zpaq_segment_len(max_size: int) -> int:
    """Segment length of the device ZPAQ cutter: lcm(max_size, 32) bytes, a
    function of max_size only (include/syncfast_amd.h, sf_cut_device_zpaq)."""
    return max_size // math.gcd(max_size, 32) * 32


def zpaq_device_stats() -> Tuple[int, int, int, int]:
    """(segment length, segments, join rounds, bytes cut again) of the most
    recent device cut in this process (sf_test_zpaq_device_stats)."""
    out = (ctypes.c_uint64 * 4)()
    check(lib().sf_test_zpaq_device_stats(out), "sf_test_zpaq_device_stats")
    return tuple(int(v) for v in out)


def _zpaq_call(data, bits, max_size, stream, digests: bool, blocks_hash: bool):
    """sf_cut_device_zpaq / sf_index_device_zpaq with outputs sized from a
    guess (len >> (bits - 1) + 16 blocks) and once more from the need the
    library reports with SF_ENOSPC."""
    _require_device(data, "data", torch.uint8)
    n = data.numel()
    bh = (ctypes.c_uint8 * 20)() if blocks_hash else None
    nb = ctypes.c_uint64(0)

    def call(cap):
        offs = torch.empty(cap, dtype=torch.int64, device=data.device)
        sizes = torch.empty(cap, dtype=torch.int32, device=data.device)
        dig = torch.empty((cap, 20), dtype=torch.uint8, device=data.device) if digests else None
        args = (_ptr(data), n, bits, max_size, _ptr(offs), _ptr(sizes))
        if digests:
            rc = lib().sf_index_device_zpaq(*args, _ptr(dig), cap, ctypes.byref(nb), bh, _stream_ptr(data, stream))
        else:
            rc = lib().sf_cut_device_zpaq(*args, cap, ctypes.byref(nb), _stream_ptr(data, stream))
        return rc, nb.value, (offs, sizes, dig)
    with _on(data.device, stream):
        k, (offs, sizes, dig) = retry_enospc(call, min(n, (n >> max(bits - 1, 0)) + n // max_size + 16), 2,
                                             "sf_index_device_zpaq" if digests else "sf_cut_device_zpaq")
    return offs[:k], sizes[:k], (dig[:k] if digests else None), (bytes(bh) if blocks_hash else None)


def cut_device_zpaq(data: torch.Tensor, bits: int = 13, max_size: int = 32768,
                    stream: Optional[torch.cuda.Stream] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's content-defined (ZPAQ) blocks of a uint8 HBM buffer, cut
    on the device (sf_cut_device_zpaq): (offsets int64[n], sizes int32[n]) in
    file order, exactly host.zpaq_cut_buffer's list -- what index_device_blocks
    takes.  Blocking: the stream is synchronised once per join round."""
    offs, sizes, _d, _h = _zpaq_call(data, bits, max_size, stream, False, False)
    return offs, sizes


def index_device_zpaq(data: torch.Tensor, bits: int = 13, max_size: int = 32768, blocks_hash: bool = True,
                      stream: Optional[torch.cuda.Stream] = None):
    """index_file's default mode (src/index.rs:621-656) for bytes already in
    HBM (sf_index_device_zpaq): the cut, every block's SHA-1 and, with
    ``blocks_hash``, the file's blocks_hash (bytes, chained on the host).
    Returns (offsets int64[n], sizes int32[n], digests uint8[n, 20],
    blocks_hash or None)."""
    return _zpaq_call(data, bits, max_size, stream, True, blocks_hash)


class ZpaqFiles(NamedTuple):
    """What cut_zpaq_files / index_zpaq_files return: the rows of every
    settled file in file order (offsets are positions in the buffer),
    first_row int64[n_files + 1] on the device, unsettled bool[n_files] on the
    host, and for the index form digests uint8[n, 20] and, when asked for,
    blocks_hashes uint8[n_files, 20] on the host (zeros for an unsettled
    file)."""
    offsets: torch.Tensor
    sizes: torch.Tensor
    first_row: torch.Tensor
    unsettled: np.ndarray
    digests: Optional[torch.Tensor]
    blocks_hashes: Optional[np.ndarray]


def zpaq_files_stats() -> Tuple[int, int, int, int, int, int]:
    """(segment length, segments, join launches, bytes cut again, unsettled
    files, files finished on the host) of the most recent many-file device cut
    in this process (sf_test_zpaq_files_stats)."""
    out = (ctypes.c_uint64 * 6)()
    check(lib().sf_test_zpaq_files_stats(out), "sf_test_zpaq_files_stats")
    return tuple(int(v) for v in out)


def _zpaq_files_call(data, files, bits, max_size, max_rounds, stream, digests: bool, blocks_hashes: bool) -> ZpaqFiles:
    """sf_cut_device_zpaq_files / sf_index_device_zpaq_files with outputs
    sized from a guess and once more from the need the library reports with
    SF_ENOSPC (as _zpaq_call)."""
    _require_device(data, "data", torch.uint8)
    fa = np.ascontiguousarray(np.asarray(files, dtype=np.uint64).reshape(-1, 2))
    nf = fa.shape[0]
    offs_h, lens_h = np.ascontiguousarray(fa[:, 0]), np.ascontiguousarray(fa[:, 1])
    total = int(lens_h.sum())
    name = "sf_index_device_zpaq_files" if digests else "sf_cut_device_zpaq_files"
    mask = np.zeros(nf, np.uint8)
    bh = np.zeros((nf, 20), np.uint8) if blocks_hashes else None
    nb, nu, bad = ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_uint32(0)

    def call(cap):
        offs = torch.empty(cap, dtype=torch.int64, device=data.device)
        sizes = torch.empty(cap, dtype=torch.int32, device=data.device)
        first = torch.empty(nf + 1, dtype=torch.int64, device=data.device)
        dig = torch.empty((cap, 20), dtype=torch.uint8, device=data.device) if digests else None
        head = (_ptr(data), data.numel(), offs_h.ctypes.data, lens_h.ctypes.data, nf, bits, max_size, max_rounds,
                _ptr(offs), _ptr(sizes))
        tail = (mask.ctypes.data, ctypes.byref(nu), ctypes.byref(bad), _stream_ptr(data, stream))
        if digests:
            rc = lib().sf_index_device_zpaq_files(*head, _ptr(dig), cap, _ptr(first), ctypes.byref(nb),
                                                  bh.ctypes.data if blocks_hashes else None, *tail)
        else:
            rc = lib().sf_cut_device_zpaq_files(*head, cap, _ptr(first), ctypes.byref(nb), *tail)
        return rc, nb.value, (offs, sizes, first, dig)
    with _on(data.device, stream):
        k, (offs, sizes, first, dig) = retry_enospc(
            call, (total >> max(bits - 1, 0)) + total // max_size + nf + 16, 2,
            lambda rc: f"{name}: file {bad.value}" if rc == SF_ERANGE else name)
    return ZpaqFiles(offs[:k], sizes[:k], first, mask.astype(bool), dig[:k] if digests else None, bh)


def cut_zpaq_files(data: torch.Tensor, files, bits: int = 13, max_size: int = 32768, max_rounds: int = 0,
                   stream: Optional[torch.cuda.Stream] = None) -> ZpaqFiles:
    """cut_device_zpaq for many files of one HBM buffer in one call
    (sf_cut_device_zpaq_files): ``files`` is a sequence of (offset, length);
    every file is cut as a file of its own, and the segments of all of them
    fill the device together.  ``max_rounds`` bounds the join launches
    (0: none); a file that has not settled by then has no rows and is marked
    in ``unsettled``.  Blocking: the stream is synchronised once per join
    launch."""
    return _zpaq_files_call(data, files, bits, max_size, max_rounds, stream, False, False)


def index_zpaq_files(data: torch.Tensor, files, bits: int = 13, max_size: int = 32768, max_rounds: int = 0,
                     blocks_hashes: bool = True, stream: Optional[torch.cuda.Stream] = None) -> ZpaqFiles:
    """index_zpaq for many files of one HBM buffer (sf_index_device_zpaq_files):
    cut_zpaq_files, every block's SHA-1 and, with ``blocks_hashes``, every
    file's blocks_hash (chained on the host; SHA-1("") for a file with no
    blocks, zeros for an unsettled one)."""
    return _zpaq_files_call(data, files, bits, max_size, max_rounds, stream, True, blocks_hashes)


def index_device_batch(data: torch.Tensor, files: Sequence[Tuple[int, int]], block_size: int,
                       file_hashes: bool = True, out: Optional[torch.Tensor] = None,
                       hashes_out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                       status: Optional[torch.Tensor] = None):
    """Many files inside one HBM buffer.

    ``files`` = [(offset, length), ...].  Returns (digests uint8[n,20],
    first_block int64[n_files+1], file_hashes uint8[n_files,20] or None).

    An equal-size batch with file_hashes is hashed in two column halves (two
    launches: the first half of every file's blocks_hash chain runs beside
    the second half's blocks) and a last launch for the chains' second half
    (include/syncfast_amd.h, sf_index_device_batch): no wave
    waits for another, so nothing can time out.  ``status`` (int32[1] on the
    device, may be None) is passed through and is never written; it stays
    for callers of the round-5 interface."""
    _require_device(data, "data", torch.uint8)
    nf = len(files)
    descs = (FileDesc * max(nf, 1))()
    total = 0
    for i, (o, ln) in enumerate(files):
        descs[i].offset, descs[i].len = int(o), int(ln)
        total += num_blocks(int(ln), block_size)
    with _on(data.device, stream):
        dig = _out(out, "out", (total, 20), torch.uint8, data)
        fh = _out(hashes_out, "hashes_out", (nf, 20), torch.uint8, data) if file_hashes and nf else None
        first = np.zeros(nf + 1, np.uint64)
        nb = ctypes.c_uint64(0)
        if status is not None:
            _require_device(status, "status", torch.int32, data.device)
        check(lib().sf_index_device_batch(_ptr(data), data.numel(), descs, nf, block_size, _ptr(dig, total),
                                          dig.numel() // 20, _ptr(fh), first.ctypes.data, ctypes.byref(nb),
                                          _ptr(status), _stream_ptr(data, stream)), "sf_index_device_batch")
    return dig, first.astype(np.int64), fh


class BatchStream:
    """Equal-size many-file batches streamed through the device
    (sf_index_device_batch_chained).  Every batch is n_files files of
    file_len bytes back to back in one uint8 HBM tensor.

    push(data, digests) hashes the batch's blocks into `digests` and, in the
    SAME launch, runs the per-file blocks_hash chains of earlier batches:
    with split=True (default) the second half of batch i-2's chains and the
    first half of batch i-1's, so a chain needs only half the latency cover.
    push() returns the blocks_hash tensor (uint8[n_files, 20]) of the batch
    whose chains this launch completes (i-2 split, i-1 unsplit), or None;
    finish() returns the remaining ones in batch order.  push_last(data,
    digests) pushes the stream's last batch and finishes: it returns every
    remaining blocks_hash tensor, and with split chains it hashes that batch
    in two column halves, so the first half of its chains runs beside the
    second half's blocks and only the second half of its chains runs alone.
    A batch's digest table must stay alive until its hashes have been
    returned.  The chains read a table in 16-byte pieces: a digest tensor
    that does not start 16-byte aligned (a view a few bytes into a larger
    buffer), like a batch whose blocks per file are no multiple of 4, raises
    SfError(SF_EINVAL) at the launch that would chain it (sf_chain_job in
    include/syncfast_amd.h; the states and hashes, allocated here, are
    4-byte aligned as it asks)."""

    def __init__(self, n_files: int, file_len: int, block_size: int, stream: Optional[torch.cuda.Stream] = None,
                 split: bool = True):
        if file_len <= 0 or file_len % block_size:
            raise ValueError("file_len must be a positive multiple of block_size")
        self.n_files, self.file_len, self.block_size = n_files, file_len, block_size
        self.nbf = file_len // block_size
        self.split = split and (self.nbf * 20) // 64 >= 2
        self.stream = stream
        self._b = None  # (digests, hashes): batch waiting for its first half / whole chain
        self._a = None  # (digests, hashes, state): batch waiting for its second half
        self._states = None

    def _job(self, part, entry, state=None):
        d, h = entry[0], entry[1]
        return ChainJob(d.data_ptr(), self.n_files, part, self.nbf, _ptr(state), h.data_ptr() if part != 1 else None)

    def _launch(self, data, digests, jobs, ref, cols=None):
        arr = (ChainJob * max(len(jobs), 1))(*jobs)
        lo, hi = cols if cols is not None else (0, self.nbf)
        with _on(ref.device, self.stream):
            check(lib().sf_index_device_batch_chained_cols(
                _ptr(data), self.n_files if data is not None else 0, self.file_len, self.block_size, lo, hi,
                _ptr(digests), arr, len(jobs), _stream_ptr(ref, self.stream)), "sf_index_device_batch_chained_cols")

    def _step_jobs(self):
        """Chain jobs for the next launch; advances the pipeline state."""
        jobs, done = [], None
        if self.split:
            if self._a is not None:
                jobs.append(self._job(2, self._a, self._a[2]))
                done = self._a[1]
                self._a = None
            if self._b is not None:
                if self._states is None:
                    dev = self._b[0].device
                    self._states = [torch.empty((self.n_files, 20), dtype=torch.uint8, device=dev) for _ in range(2)]
                st = self._states[0]
                self._states.reverse()  # the next first half writes the other state buffer
                jobs.append(self._job(1, self._b, st))
                self._a = (self._b[0], self._b[1], st)
                self._b = None
        elif self._b is not None:
            jobs.append(self._job(0, self._b))
            done = self._b[1]
            self._b = None
        return jobs, done

    def _check_batch(self, data, digests):
        _require_device(data, "data", torch.uint8)
        _require_device(digests, "digests", torch.uint8, data.device)
        if data.numel() != self.n_files * self.file_len or digests.numel() < 20 * self.n_files * self.nbf:
            raise ValueError("batch or digest table has the wrong size")

    def push(self, data: torch.Tensor, digests: torch.Tensor):
        self._check_batch(data, digests)
        # the chain states and this batch's blocks_hash table are allocated on
        # the stream the launches run on, like every other output here
        with _on(data.device, self.stream):
            jobs, done = self._step_jobs()
            self._launch(data, digests, jobs, data)
            self._b = (digests, torch.empty((self.n_files, 20), dtype=torch.uint8, device=data.device))
        return done

    def _half_cols(self):
        """Column split of a last batch: the first half of every chain (part
        1: bytes [0, 64 * half) of the run) reads digests [0, cut) only."""
        if not self.split or self.nbf % 64 or self.nbf < 128:
            return None
        half = (self.nbf * 20 // 64) // 2  # data chunks of part 1 (as the launcher computes them)
        need = (half * 64 + 19) // 20  # digests part 1 reads
        cut = (need + 63) // 64 * 64  # in whole block waves
        return cut if cut < self.nbf else None

    def push_last(self, data: torch.Tensor, digests: torch.Tensor):
        """Push the stream's last batch and finish; returns every remaining
        blocks_hash tensor in batch order."""
        self._check_batch(data, digests)
        cut = self._half_cols()
        if cut is None:
            done = self.push(data, digests)
            return ([done] if done is not None else []) + self.finish()
        out = []
        with _on(data.device, self.stream):
            # columns [0, cut) beside the jobs push() would run ...
            jobs, done = self._step_jobs()
            self._launch(data, digests, jobs, data, (0, cut))
            if done is not None:
                out.append(done)
            # ... then columns [cut, end) beside the next jobs, which include
            # the first half of this batch's chains (its digests [0, cut) exist)
            self._b = (digests, torch.empty((self.n_files, 20), dtype=torch.uint8, device=data.device))
            jobs, done = self._step_jobs()
            self._launch(data, digests, jobs, data, (cut, self.nbf))
            if done is not None:
                out.append(done)
        return out + self.finish()

    def finish(self):
        out = []
        while self._a is not None or self._b is not None:
            ref = (self._a or self._b)[0]
            with _on(ref.device, self.stream):
                jobs, done = self._step_jobs()
                self._launch(None, None, jobs, ref)
            if done is not None:
                out.append(done)
        return out


def _receive_outputs(run: torch.Tensor, lookup: bool):
    """(capacity, digests uint8[cap, 20], sizes int32[cap]) for the FILE_BLOCK
    messages of ``run`` and, with ``lookup``, (offsets, rows) int64[cap] too.
    Call inside ``_on``."""
    cap = run.numel() // 34 + 1  # a message is at least 34 bytes
    digests = torch.empty((cap, 20), dtype=torch.uint8, device=run.device)
    sizes = torch.empty(cap, dtype=torch.int32, device=run.device)
    if not lookup:
        return cap, digests, sizes
    offsets = torch.empty(cap, dtype=torch.int64, device=run.device)
    return cap, digests, sizes, offsets, torch.empty(cap, dtype=torch.int64, device=run.device)


class FilesReceived(NamedTuple):
    """What ``BlockSet.receive_files`` returns (sf_receive_files_device).
    Blocks, one row per FILE_BLOCK in stream order: ``digests`` uint8[n, 20],
    ``sizes`` uint32[n], ``offsets`` int64[n] within the block's file, ``rows``
    int64[n] as ``lookup`` gives them, ``block_file`` int32[n] the block's
    section.  Sections, one row per file of the call in stream order:
    ``name_at`` int64[m] / ``name_len`` int32[m] the name's bytes in the run
    (-1 / 0 for a file carried in), ``file_first`` int64[m + 1] the section's
    first block (the last entry = n), ``file_size`` int64[m] the running
    offset at the section's end.  ``consumed`` / ``stop`` as
    wire.parse_blocks_device (``stop`` may be SF_WIRE_UNEXPECTED), ``open`` /
    ``end_offset`` the state to carry into the next call."""
    digests: torch.Tensor
    sizes: torch.Tensor
    offsets: torch.Tensor
    rows: torch.Tensor
    block_file: torch.Tensor
    name_at: torch.Tensor
    name_len: torch.Tensor
    file_first: torch.Tensor
    file_size: torch.Tensor
    consumed: int
    stop: int
    open: bool
    end_offset: int


class BlockSet:
    """The receiving side's block lookup, on the device (sf_block_set_*).

    Built from a destination index's rows -- ``table`` uint8[n, 20] digests
    in rowid order, ``present`` bool/uint8[n] (None = all present) -- as an
    HBM hash table; ``lookup(digests)`` returns int64[m]: for each digest the
    row of the first present row holding it, or -1.  That is Index::get_block
    (src/index.rs:77-103: hash = ? AND present = 1, SQLite's (hash, rowid)
    order) for a whole FILE_BLOCK list at once, the question
    FsDestinationInner::sink asks per message (src/sync/fs.rs:461-476).
    The set reads ``table`` at lookup time: keep it unchanged while in use."""

    def __init__(self, table: torch.Tensor, present: Optional[torch.Tensor] = None,
                 stream: Optional[torch.cuda.Stream] = None):
        _require_device(table, "table", torch.uint8)
        if table.dim() != 2 or table.shape[1] != 20:
            raise ValueError("table must be uint8[n, 20]")
        n = table.shape[0]
        if present is not None:
            if present.dtype == torch.bool:
                present = present.view(torch.uint8)
            _require_device(present, "present", torch.uint8, table.device)
            if present.numel() != n:
                raise ValueError("present must hold one flag per row")
        self.table, self.present, self.stream = table, present, stream
        self._h = ctypes.c_void_p()
        with _on(table.device, stream):
            check(lib().sf_block_set_build(_ptr(table), _ptr(present), n, ctypes.byref(self._h),
                                           _stream_ptr(table, stream)), "sf_block_set_build")

    def lookup(self, digests: torch.Tensor) -> torch.Tensor:
        _require_device(digests, "digests", torch.uint8, self.table.device)
        if digests.dim() != 2 or digests.shape[1] != 20:
            raise ValueError("digests must be uint8[m, 20]")
        if not self._h:
            raise ValueError("BlockSet is closed")
        m = digests.shape[0]
        with _on(self.table.device, self.stream):
            rows = torch.empty(m, dtype=torch.int64, device=self.table.device)
            if m:
                check(lib().sf_block_set_lookup(self._h, digests.data_ptr(), m, rows.data_ptr(),
                                                _stream_ptr(self.table, self.stream)), "sf_block_set_lookup")
        return rows

    def receive(self, run: torch.Tensor, base_offset: int = 0):
        """A FILE_BLOCK run as the destination receives it, in one call
        (sf_receive_blocks_device): the messages at the start of ``run`` (a
        uint8 HBM tensor) are parsed on the device, each gets its offset in
        the incoming file (``base_offset`` + the sizes before it, the running
        offset of src/sync/fs.rs:477) and its lookup in this set.  Returns
        (digests uint8[n, 20], sizes uint32[n], offsets int64[n], rows
        int64[n], consumed, stop, end_offset): ``rows`` as ``lookup`` gives
        them, ``consumed`` / ``stop`` as wire.parse_blocks_device, and
        ``end_offset`` the offset after the last message -- the file's size
        when the run stops at FILE_END, or the next call's ``base_offset``
        when it arrives in pieces.  Blocking."""
        _require_device(run, "run", torch.uint8, self.table.device)
        if run.dim() != 1:
            raise ValueError("run must be a flat uint8 tensor")
        if not self._h:
            raise ValueError("BlockSet is closed")
        n, consumed, end = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        stop = ctypes.c_int(0)
        with _on(self.table.device, self.stream):
            cap, digests, sizes, offsets, rows = _receive_outputs(run, True)
            check(lib().sf_receive_blocks_device(self._h, _ptr(run), run.numel(), int(base_offset),
                                                 digests.data_ptr(), sizes.data_ptr(), offsets.data_ptr(),
                                                 rows.data_ptr(), cap, ctypes.byref(n), ctypes.byref(consumed),
                                                 ctypes.byref(stop), ctypes.byref(end),
                                                 _stream_ptr(self.table, self.stream)), "sf_receive_blocks_device")
        k = n.value
        return (digests[:k], sizes[:k].view(torch.uint32), offsets[:k], rows[:k], consumed.value, stop.value,
                end.value)

    def receive_files(self, run: torch.Tensor, open: bool = False, base_offset: int = 0) -> FilesReceived:
        """A whole GetFiles stream as the destination receives it, in one call
        (sf_receive_files_device): ``run`` (a flat uint8 HBM tensor) holds any
        number of files -- FILE_START, FILE_BLOCKs, FILE_END, back to back,
        beginning and ending anywhere -- and is parsed on the device as
        ``wire.Parser`` reads it and accepted in the sink's order
        (src/sync/fs.rs:449-500); every block gets its file, its running
        offset within that file and its lookup in this set.  ``open`` /
        ``base_offset``: a file was open when the run began (section 0 of the
        result, without a name) and its running offset.  A run that arrives in
        pieces is continued with ``run[consumed:]`` + the new bytes and the
        returned ``open`` / ``end_offset``.  The outputs are sized by a guess
        and the call is repeated once with the needs it reported when the
        guess was short.  Blocking."""
        _require_device(run, "run", torch.uint8, self.table.device)
        if run.dim() != 1:
            raise ValueError("run must be a flat uint8 tensor")
        if not self._h:
            raise ValueError("BlockSet is closed")
        dev, nbytes = self.table.device, run.numel()
        nb, nf, consumed, end = (ctypes.c_uint64(0) for _ in range(4))
        stop, open_out = ctypes.c_int(0), ctypes.c_int(0)
        bcap, fcap = nbytes // 36 + 64, nbytes // 1024 + 64  # messages of 37 bytes, files of a few blocks at least
        with _on(dev, self.stream):
            for attempt in range(2):
                e = lambda n, t: torch.empty(n, dtype=t, device=dev)  # noqa: E731
                digests, sizes, block_file = e((bcap, 20), torch.uint8), e(bcap, torch.int32), e(bcap, torch.int32)
                offsets, rows = e(bcap, torch.int64), e(bcap, torch.int64)
                name_at, name_len = e(fcap, torch.int64), e(fcap, torch.int32)
                first, fsize = e(fcap + 1, torch.int64), e(fcap, torch.int64)
                rc = lib().sf_receive_files_device(
                    self._h, _ptr(run), nbytes, int(bool(open)), int(base_offset), digests.data_ptr(), sizes.data_ptr(),
                    offsets.data_ptr(), rows.data_ptr(), block_file.data_ptr(), bcap, name_at.data_ptr(),
                    name_len.data_ptr(), first.data_ptr(), fsize.data_ptr(), fcap, ctypes.byref(nb), ctypes.byref(nf),
                    ctypes.byref(consumed), ctypes.byref(stop), ctypes.byref(open_out), ctypes.byref(end),
                    _stream_ptr(self.table, self.stream))
                if rc != SF_ENOSPC or attempt:
                    break
                bcap, fcap = max(bcap, nb.value), max(fcap, nf.value)
            check(rc, "sf_receive_files_device")
            b, f = nb.value, nf.value
            if nbytes == 0 and f:  # nothing ran: the section carried in, as the library describes it
                name_at[0], name_len[0], first[0], fsize[0] = -1, 0, 0, int(base_offset)
            if nbytes == 0:
                first[f] = 0
        return FilesReceived(digests[:b], sizes[:b].view(torch.uint32), offsets[:b], rows[:b], block_file[:b],
                             name_at[:f], name_len[:f], first[:f + 1], fsize[:f], consumed.value, stop.value,
                             bool(open_out.value), end.value)

    def serve(self, requests: torch.Tensor, src: torch.Tensor, row_offsets: torch.Tensor, row_sizes: torch.Tensor):
        """The source's answer to a received run of GET_BLOCK requests, in one
        call (sf_serve_get_blocks_device): ``requests`` (a flat uint8 HBM
        tensor) is parsed as ``wire.Parser`` reads it, every digest is looked
        up in this set, and request k becomes the BLOCK_DATA message carrying
        ``src[row_offsets[row] : + row_sizes[row]]`` -- ``row_offsets`` int64
        and ``row_sizes`` int32/uint32, one entry per row of the set, on its
        device like ``src``.  Returns (run, n_requests, n_answered, consumed,
        stop): ``run`` a ``wire.BlockDataRun`` of the first ``n_answered``
        answers, which stop at the first request whose digest the set does not
        hold (the reference answers those before it and then fails with
        "Requested block is unknown": raise that when ``n_answered <
        n_requests``); ``consumed`` = 31 * ``n_requests`` and ``stop`` the
        SF_WIRE_* class of what stands at ``requests[consumed:]``.  Blocking."""
        from .wire import BlockDataRun
        dev = self.table.device
        _require_device(requests, "requests", torch.uint8, dev)
        _require_device(src, "src", torch.uint8, dev)
        _require_device(row_offsets, "row_offsets", torch.int64, dev)
        if requests.dim() != 1:
            raise ValueError("requests must be a flat uint8 tensor")
        n = self.table.shape[0]
        if (not isinstance(row_sizes, torch.Tensor) or row_sizes.dtype not in (torch.int32, torch.uint32)
                or row_sizes.device != dev or row_sizes.numel() != n or row_offsets.numel() != n):
            raise ValueError("row_offsets (int64) and row_sizes (32-bit) must hold one entry per row of the set")
        if not self._h:
            raise ValueError("BlockSet is closed")
        h, stop = ctypes.c_void_p(), ctypes.c_int(0)
        nreq, nans, consumed = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        with _on(dev, self.stream):
            row_sizes = row_sizes.contiguous()
            # the library wants its buffers even where nothing can be read from them
            buf = src if src.numel() else torch.empty(1, dtype=torch.uint8, device=dev)
            if n == 0:
                row_offsets, row_sizes = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(
                    1, dtype=torch.int32, device=dev)
            check(lib().sf_serve_get_blocks_device(self._h, _ptr(row_offsets), _ptr(row_sizes), buf.data_ptr(),
                                                   src.numel(), _ptr(requests), requests.numel(), ctypes.byref(h),
                                                   ctypes.byref(nreq), ctypes.byref(nans), ctypes.byref(consumed),
                                                   ctypes.byref(stop), _stream_ptr(self.table, self.stream)),
                  "sf_serve_get_blocks_device")
        return BlockDataRun(h, dev, self.stream), nreq.value, nans.value, consumed.value, stop.value

    def close(self) -> None:
        if self._h:
            with _on(self.table.device, self.stream):
                check(lib().sf_block_set_free(self._h, _stream_ptr(self.table, self.stream)), "sf_block_set_free")
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EntriesReceived(NamedTuple):
    """What ``receive_file_entries`` / ``NameSet.receive_entries`` return
    (sf_receive_file_entries_device), one row per FILE_ENTRY in list order:
    ``name_at`` int64[n] / ``name_len`` int32[n] the name's bytes in the run,
    ``sizes`` int64[n] (bit pattern of a uint64), ``hashes`` uint8[n, 20] as
    announced; with a set ``rows`` int64[n] as ``NameSet.lookup`` gives them,
    ``need`` uint8[n] and ``need_list`` int32[m] the entries with need 1,
    ascending (None without a set).  ``consumed`` / ``stop`` as
    wire.parse_blocks_device (``stop`` may be SF_WIRE_END_FILES: END_FILES was
    read and is among ``consumed``); ``bad_name`` the first entry whose name
    is not UTF-8, or None."""
    name_at: torch.Tensor
    name_len: torch.Tensor
    sizes: torch.Tensor
    hashes: torch.Tensor
    rows: Optional[torch.Tensor]
    need: Optional[torch.Tensor]
    need_list: Optional[torch.Tensor]
    consumed: int
    stop: int
    bad_name: Optional[int]


class FilesServed(NamedTuple):
    """What ``NameSet.serve_files`` returns (sf_serve_get_files_device):
    ``run`` a ``wire.FilesRun`` holding the answers of requests ``[0,
    n_answered)`` of the ``n_requests`` parsed; ``answered_bytes`` the bytes of
    the request run those occupy; ``why`` what stopped the answering:
    SF_SERVE_ALL, SF_SERVE_BAD_NAME (the next name is not UTF-8),
    SF_SERVE_UNKNOWN (the set does not hold it) -- the caller sends the run and
    raises "Bad filename encoding" / "Requested file is unknown", as the
    reference does -- or SF_SERVE_FULL (the next answer would leave
    ``max_run_bytes`` or 2^32 messages: send the run and call again with the
    requests from ``answered_bytes`` on).  ``consumed`` / ``stop`` describe the
    whole parsed prefix, as wire.parse_blocks_device."""
    run: object
    n_requests: int
    n_answered: int
    answered_bytes: int
    why: int
    consumed: int
    stop: int


def serve_files_stats() -> Tuple[int, int, int, int]:
    """Test hook (sf_test_serve_files_stats): (route: 0 nothing launched, 1
    parsed and no request answered, 2 a run built; requests; answered;
    read-backs) of this process's last sf_serve_get_files_device."""
    out = (ctypes.c_uint64 * 4)()
    check(lib().sf_test_serve_files_stats(out), "sf_test_serve_files_stats")
    return tuple(int(v) for v in out)


def pack_names(names: Sequence[bytes], device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """A list of names as the library takes it: (packed bytes uint8, CSR
    int64[n + 1]) on ``device`` (``device_of``)."""
    dev = device_of(device)
    at = np.zeros(len(names) + 1, np.int64)
    np.cumsum(np.fromiter((len(n) for n in names), np.int64, len(names)), out=at[1:])
    return upload(b"".join(bytes(n) for n in names), dev), torch.from_numpy(at).to(dev)


def file_entries_stats() -> Tuple[int, int, int, int]:
    """Test hook (sf_test_file_entries_stats): (route: 0 the device chain, 1
    forced to the host, 2 the host fallback; candidates; chained entries;
    read-backs) of this process's last sf_receive_file_entries_device."""
    out = (ctypes.c_uint64 * 4)()
    check(lib().sf_test_file_entries_stats(out), "sf_test_file_entries_stats")
    return tuple(int(v) for v in out)


def receive_file_entries(run: torch.Tensor, name_set: Optional["NameSet"] = None,
                         have_hashes: Optional[torch.Tensor] = None, have_hash_ok: Optional[torch.Tensor] = None,
                         stream: Optional[torch.cuda.Stream] = None) -> EntriesReceived:
    """The sink's FilesList state for one received buffer, in one call
    (sf_receive_file_entries_device): the FILE_ENTRY messages at the start of
    ``run`` (a flat uint8 HBM tensor) parsed on the device as ``wire.Parser``
    reads them.  With ``name_set`` every name is looked up in it and every
    announced hash compared with ``have_hashes`` uint8[rows, 20] (the recorded
    blocks_hash of the set's rows; ``have_hash_ok`` uint8/bool[rows], None =
    every row has one): see ``EntriesReceived``.  A list that arrives in pieces
    is continued with ``run[consumed:]`` + the new bytes.  Blocking."""
    _require_device(run, "run", torch.uint8)
    if run.dim() != 1:
        raise ValueError("run must be a flat uint8 tensor")
    dev = run.device
    h = None
    if name_set is not None:
        if not name_set._h:
            raise ValueError("NameSet is closed")
        rows_n = name_set.n_rows
        if have_hashes is None:
            raise ValueError("a name set needs have_hashes")
        _require_device(have_hashes, "have_hashes", torch.uint8, dev)
        if have_hashes.numel() != 20 * rows_n:
            raise ValueError("have_hashes must be uint8[rows, 20]")
        have_hash_ok = _flags(have_hash_ok, "have_hash_ok", rows_n, dev)
        h, stream = name_set._h, stream if stream is not None else name_set.stream
    elif have_hashes is not None or have_hash_ok is not None:
        raise ValueError("have_hashes and have_hash_ok go with a name set")
    n, n_need, bad, consumed = (ctypes.c_uint64(0) for _ in range(4))
    stop = ctypes.c_int(0)
    cap = run.numel() // 35 + 1  # an entry is at least 35 bytes
    with _on(dev, stream):
        e = lambda k, t: torch.empty(k, dtype=t, device=dev)  # noqa: E731
        name_at, name_len, sizes, hashes = e(cap, torch.int64), e(cap, torch.int32), e(cap, torch.int64), e(
            (cap, 20), torch.uint8)
        rows, need, need_list = (e(cap, torch.int64), e(cap, torch.uint8), e(cap, torch.int32)) if h else (None,) * 3
        # the library wants a table even when the set has no row
        have = have_hashes if h is None or have_hashes.numel() else e(20, torch.uint8)
        check(lib().sf_receive_file_entries_device(
            h, _ptr(run), run.numel(), have.data_ptr() if h else None, _ptr(have_hash_ok), name_at.data_ptr(),
            name_len.data_ptr(), sizes.data_ptr(), hashes.data_ptr(), _ptr(rows), _ptr(need), _ptr(need_list), cap,
            ctypes.byref(n), ctypes.byref(n_need), ctypes.byref(bad), ctypes.byref(consumed), ctypes.byref(stop),
            _stream_ptr(run, stream)), "sf_receive_file_entries_device")
    k, m = n.value, n_need.value
    return EntriesReceived(name_at[:k], name_len[:k], sizes[:k], hashes[:k], rows[:k] if h else None,
                           need[:k] if h else None, need_list[:m] if h else None, consumed.value, stop.value,
                           None if bad.value == (1 << 64) - 1 else bad.value)


class NameSet:
    """The receiving side's lookup of files by name, on the device
    (sf_name_set_*): Index::get_file for a whole files list at once, the
    sibling of ``BlockSet``.

    Built from a destination index's file rows in file_id order -- ``names``
    uint8 the packed name bytes, ``name_at`` int64[n + 1] the CSR into them
    (``pack_names`` makes both from a list; ``NameSet.build`` does it all),
    ``present`` bool/uint8[n] (None = all; the mirror of temporary = 0).
    ``lookup`` gives for each query the lowest present row of that name, or
    -1 (SQLite's idx_files_name order: the schema has no UNIQUE on name).  A
    CSR that does not hold raises ValueError naming the first bad row.  The
    set reads ``names`` and ``name_at`` at lookup time: keep them unchanged
    while in use."""

    def __init__(self, names: torch.Tensor, name_at: torch.Tensor, present: Optional[torch.Tensor] = None,
                 stream: Optional[torch.cuda.Stream] = None):
        _require_device(names, "names", torch.uint8)
        dev = names.device
        _require_device(name_at, "name_at", torch.int64, dev)
        if names.dim() != 1 or name_at.dim() != 1 or name_at.numel() < 1:
            raise ValueError("names must be flat and name_at hold one entry per row and one more")
        n = name_at.numel() - 1
        present = _flags(present, "present", n, dev)
        self.names, self.name_at, self.present, self.stream, self.n_rows = names, name_at, present, stream, n
        self._h = ctypes.c_void_p()
        bad = ctypes.c_uint64(0)
        with _on(dev, stream):
            rc = lib().sf_name_set_build(_ptr(names), name_at.data_ptr(), _ptr(present), n, ctypes.byref(self._h),
                                         ctypes.byref(bad), _stream_ptr(names, stream))
        if rc != 0 and bad.value != (1 << 64) - 1:
            raise ValueError(f"row {bad.value}: its name_at entries do not hold")
        check(rc, "sf_name_set_build")

    @classmethod
    def build(cls, names: Sequence[bytes], present=None, device=None,
              stream: Optional[torch.cuda.Stream] = None) -> "NameSet":
        """The set of a list of names (bytes), row i = ``names[i]``;
        ``present`` a sequence of flags or None."""
        dev = device_of(device)
        packed, at = pack_names(names, dev)
        if present is not None and not isinstance(present, torch.Tensor):
            present = torch.from_numpy(np.asarray(present, dtype=np.uint8)).to(dev)
        return cls(packed, at, present, stream)

    def lookup(self, data: torch.Tensor, at: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        """int64[m]: for query i, the ``lens[i]`` bytes of ``data`` (flat uint8)
        from ``at[i]`` -- ``at`` int64[m], ``lens`` int32/uint32[m], spans
        anywhere in ``data`` -- the lowest present row of that name, or -1.  A
        span that leaves ``data`` gives -1."""
        dev = self.names.device
        _require_device(data, "data", torch.uint8, dev)
        m = at.numel()
        _list64(at, "at", m, dev)
        _list32(lens, "lens", m, dev)
        if not self._h:
            raise ValueError("NameSet is closed")
        with _on(dev, self.stream):
            rows = torch.empty(m, dtype=torch.int64, device=dev)
            if m:
                check(lib().sf_name_set_lookup(self._h, _ptr(data), data.numel(), at.data_ptr(), lens.data_ptr(), m,
                                               rows.data_ptr(), _stream_ptr(self.names, self.stream)),
                      "sf_name_set_lookup")
        return rows

    def lookup_names(self, names: Sequence[bytes]) -> torch.Tensor:
        """``lookup`` of a list of names (bytes)."""
        dev = self.names.device
        with _on(dev, self.stream):
            packed, at = pack_names(names, dev)
            lens = (at[1:] - at[:-1]).to(torch.int32)
            return self.lookup(packed, at[:-1].contiguous(), lens)

    def receive_entries(self, run: torch.Tensor, have_hashes: torch.Tensor,
                        have_hash_ok: Optional[torch.Tensor] = None) -> EntriesReceived:
        """``receive_file_entries`` of ``run`` against this set."""
        return receive_file_entries(run, self, have_hashes, have_hash_ok)

    def serve_files(self, requests: torch.Tensor, file_first: torch.Tensor, digests: torch.Tensor,
                    sizes: torch.Tensor, max_run_bytes: int = 0) -> FilesServed:
        """The source's answer to a received run of GET_FILE requests, in one
        call (sf_serve_get_files_device): ``requests`` (a flat uint8 HBM tensor)
        is parsed as ``wire.Parser`` reads it, every name is looked up in this
        set -- built over the source's non-temporary files in file_id order --
        and request k becomes FILE_START with the name, one FILE_BLOCK per
        block of its row and FILE_END.  ``file_first`` int64[rows + 1] is the
        CSR of the set's rows into the block table ``digests`` uint8[n, 20] /
        ``sizes`` int32/uint32[n] (row r owns blocks ``file_first[r] :
        file_first[r + 1]``, in list_file_blocks order), all on the set's
        device; nothing is gathered or copied per request.  ``max_run_bytes``
        (0: no bound) bounds the run the call allocates.  See ``FilesServed``.
        A row that answering reaches and whose CSR entries do not hold raises
        ValueError naming it.  Blocking, for three read-backs."""
        from .wire import FilesRun
        dev = self.names.device
        _require_device(requests, "requests", torch.uint8, dev)
        _require_device(file_first, "file_first", torch.int64, dev)
        n = _table20(digests, "digests", dev)
        _list32(sizes, "sizes", n, dev)
        if requests.dim() != 1 or file_first.dim() != 1 or file_first.numel() != self.n_rows + 1:
            raise ValueError("requests must be flat and file_first hold one entry per row of the set and one more")
        if not self._h:
            raise ValueError("NameSet is closed")
        h, stop, why = ctypes.c_void_p(), ctypes.c_int(0), ctypes.c_int(0)
        nreq, nans, used, bad, consumed = (ctypes.c_uint64(0) for _ in range(5))
        with _on(dev, self.stream):
            rc = lib().sf_serve_get_files_device(self._h, file_first.data_ptr(), _ptr(digests, n), _ptr(sizes, n), n,
                                                 _ptr(requests), requests.numel(), int(max_run_bytes), ctypes.byref(h),
                                                 ctypes.byref(nreq), ctypes.byref(nans), ctypes.byref(used),
                                                 ctypes.byref(why), ctypes.byref(bad), ctypes.byref(consumed),
                                                 ctypes.byref(stop), _stream_ptr(self.names, self.stream))
        if rc != 0 and bad.value != (1 << 64) - 1:
            raise ValueError(f"row {bad.value}: its file_first entries do not hold")
        check(rc, "sf_serve_get_files_device")
        return FilesServed(FilesRun(h, dev, self.stream), nreq.value, nans.value, used.value, why.value,
                           consumed.value, stop.value)

    def close(self) -> None:
        if self._h:
            with _on(self.names.device, self.stream):
                check(lib().sf_name_set_free(self._h, _stream_ptr(self.names, self.stream)), "sf_name_set_free")
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def index_device_multi(shards: Sequence[torch.Tensor], file_len: int, block_size: int, root: int = 0,
                       table: Optional[torch.Tensor] = None, scratch: Optional[Sequence[torch.Tensor]] = None,
                       streams: Optional[Sequence[torch.cuda.Stream]] = None,
                       gather_streams: Optional[Sequence[torch.cuda.Stream]] = None) -> torch.Tensor:
    """sf_index_device_multi_ex: shards[r] (on cuda:r) holds shard r
    (host.shard_range) of one logical file; every shard is hashed on its own
    device (on streams[r]) and the digest tables meet in `table` on cuda:root,
    gathered over xGMI with RCCL inside the library (on gather_streams[r],
    after device r's hashing; default: the hash streams).  Returns the
    (nblocks, 20) table, complete once gather_streams[root] (or streams[root])
    has run past the call.  ``streams`` None: each device's default stream.
    The scratch tables and a table allocated here are marked as in use by the
    streams the library reads and writes them on, so the caching allocator
    does not hand them out again before the exchange is done."""
    n = len(shards)
    if n < 1:
        raise ValueError("no shards")
    from .host import shard_range
    nb = num_blocks(file_len, block_size)
    for r, t in enumerate(shards):
        _require_device(t, f"shards[{r}]", torch.uint8, torch.device("cuda", r))
        if t.numel() != shard_range(file_len, block_size, n, r)[1]:
            raise ValueError(f"shards[{r}] is not shard {r} of {n}")
    for name, ss in (("streams", streams), ("gather_streams", gather_streams)):
        if ss is not None and (len(ss) != n or any(s.device != torch.device("cuda", r) for r, s in enumerate(ss))):
            raise ValueError(f"{name}[r] must be a stream of cuda:r, one per shard")
    hs = list(streams) if streams is not None else [torch.cuda.default_stream(r) for r in range(n)]
    gs = list(gather_streams) if gather_streams is not None else hs
    dev_root = torch.device("cuda", root)
    own_table = table is None
    if own_table:
        table = torch.empty((max(nb, 1), 20), dtype=torch.uint8, device=dev_root)
    _require_device(table, "table", torch.uint8, dev_root)
    if table.numel() < nb * 20:
        raise ValueError("table too small")
    own_scratch = scratch is None
    if own_scratch:
        scratch = [torch.empty((max(num_blocks(t.numel(), block_size), 1), 20), dtype=torch.uint8, device=t.device)
                   for t in shards]
    # A table or scratch allocated here comes from the current stream's pool:
    # what that stream still has queued on the block's earlier life (a fill of
    # the tensor that held it before) must land before the library's streams
    # write it, or it lands on top of the digests.
    if own_scratch:
        for r in range(n):
            for st in {hs[r], gs[r]}:
                st.wait_stream(torch.cuda.current_stream(shards[r].device))
    if own_table:
        for st in {hs[root], gs[root]}:
            st.wait_stream(torch.cuda.current_stream(dev_root))
    ptr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
    sp = (ctypes.c_void_p * n)(*[s.cuda_stream for s in hs])
    gp = (ctypes.c_void_p * n)(*[s.cuda_stream for s in gs])
    check(lib().sf_index_device_multi_ex(n, ptr(shards), file_len, block_size, ptr(scratch), root, table.data_ptr(),
                                         sp, gp), "sf_index_device_multi_ex")
    if own_scratch:  # device r's scratch is written on hs[r] and sent on gs[r]
        for r in range(n):
            for st in {hs[r], gs[r]}:
                scratch[r].record_stream(st)
    if own_table:  # the root's rows are written on hs[root], the others received on gs[root]
        for st in {hs[root], gs[root]}:
            table.record_stream(st)
    return table[:nb]


def copy_stats() -> Tuple[int, int, int, int]:
    """(T, jobs copied, tiles, launches) of this process's last copy_blocks
    (sf_test_copy_stats); synchronises that call's device."""
    out = (ctypes.c_uint64 * 4)()
    check(lib().sf_test_copy_stats(out), "sf_test_copy_stats")
    return tuple(int(v) for v in out)


def copy_blocks(src: torch.Tensor, dst: torch.Tensor, src_offsets: torch.Tensor, dst_offsets: torch.Tensor,
                sizes: torch.Tensor, take: Optional[torch.Tensor] = None, check_range: bool = True,
                stream: Optional[torch.cuda.Stream] = None) -> None:
    """dst[dst_offsets[i] : + sizes[i]] = src[src_offsets[i] : + sizes[i]] for
    every i (with ``take``, uint8 or bool: every i where it is not 0), in one
    launch of the block copy kernel (sf_copy_blocks_device).

    ``src`` and ``dst`` are uint8 HBM tensors that do not overlap; the lists
    are int64 / int64 / int32 tensors on the same device, as
    index_device_blocks takes them (a size is read as uint32).  Nothing needs
    an alignment; source ranges may overlap or repeat.  The destination ranges
    of the taken jobs must be disjoint -- where two overlap, each byte comes
    from one of them, unspecified which; ranges that abut are fine.  A job
    outside either tensor is not copied; with ``check_range`` it raises
    SfError(SF_ERANGE) after the stream is synchronised (the other jobs are
    copied all the same).  Without it the call is asynchronous."""
    _require_device(src, "src", torch.uint8)
    _require_device(dst, "dst", torch.uint8, src.device)
    _require_device(src_offsets, "src_offsets", torch.int64, src.device)
    _require_device(dst_offsets, "dst_offsets", torch.int64, src.device)
    _require_device(sizes, "sizes", torch.int32, src.device)
    n = sizes.numel()
    if src_offsets.numel() != n or dst_offsets.numel() != n:
        raise ValueError("src_offsets, dst_offsets and sizes differ in length")
    if take is not None:
        if take.dtype == torch.bool:
            take = take.view(torch.uint8)
        _require_device(take, "take", torch.uint8, src.device)
        if take.numel() != n:
            raise ValueError("take must hold one flag per job")
    with _on(src.device, stream):
        status = torch.zeros(1, dtype=torch.int32, device=src.device) if check_range and n else None
        check(lib().sf_copy_blocks_device(_ptr(src), src.numel(), _ptr(dst), dst.numel(), _ptr(src_offsets),
                                          _ptr(dst_offsets), _ptr(sizes), _ptr(take), n, _ptr(status),
                                          _stream_ptr(src, stream)), "sf_copy_blocks_device")
        if status is not None and int(status.item()) != 0:
            raise SfError(SF_ERANGE, "sf_copy_blocks_device")


def _flags(t: Optional[torch.Tensor], name: str, n: int, dev: torch.device) -> Optional[torch.Tensor]:
    """A byte-flag list (uint8, or bool seen as bytes) of ``n`` entries."""
    if t is None:
        return None
    if isinstance(t, torch.Tensor) and t.dtype == torch.bool:
        t = t.view(torch.uint8)
    _require_device(t, name, torch.uint8, dev)
    if t.numel() != n:
        raise ValueError(f"{name} must hold one flag per entry ({n})")
    return t


def _table20(t: torch.Tensor, name: str, dev: Optional[torch.device] = None) -> int:
    _require_device(t, name, torch.uint8, dev)
    if t.dim() != 2 or t.shape[1] != 20:
        raise ValueError(f"{name} must be uint8[n, 20]")
    return t.shape[0]


def _list32(t: torch.Tensor, name: str, n: int, dev: torch.device) -> None:
    if (not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.uint32) or t.device != dev
            or t.numel() != n or not t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous 32-bit tensor of {n} entries on {dev}")


def _list64(t: torch.Tensor, name: str, n: int, dev: torch.device) -> None:
    _require_device(t, name, torch.int64, dev)
    if t.numel() != n:
        raise ValueError(f"{name} must hold {n} entries")


def get_block_requests(digests: torch.Tensor, rows: Optional[torch.Tensor] = None,
                       take: Optional[torch.Tensor] = None, distinct: bool = False,
                       stream: Optional[torch.cuda.Stream] = None):
    """The destination's GET_BLOCK run, built on the device
    (sf_wire_get_blocks_device): ``digests`` uint8[n, 20] are a table's rows
    in rowid order; row i asks when ``rows`` is None or ``rows[i] < 0`` (int64,
    as ``BlockSet.receive`` returns them) and ``take`` is None or ``take[i]``
    is not 0 (uint8 or bool).  Message k is ``write_message("GetBlock", ...)``
    of the k-th asking row: over the rows with present = 0 that is byte for
    byte the join over ``Index.list_missing_blocks()``, a digest missing in
    three rows asked for three times (src/sync/fs.rs:485-493).  With
    ``distinct`` only the first asking row of each digest asks.  Returns
    (run, n_requests): ``run`` a ``wire.BlockDataRun`` (``bytes``, ``tensor``,
    ``to_fd``, ``close``).  Blocking, for one read-back."""
    from .wire import BlockDataRun
    n = _table20(digests, "digests")
    dev = digests.device
    if rows is not None:
        _list64(rows, "rows", n, dev)
    take = _flags(take, "take", n, dev)
    h, nreq = ctypes.c_void_p(), ctypes.c_uint64(0)
    with _on(dev, stream):
        check(lib().sf_wire_get_blocks_device(_ptr(digests, n), _ptr(rows, n), _ptr(take, n), n, int(bool(distinct)),
                                              ctypes.byref(h), ctypes.byref(nreq), _stream_ptr(digests, stream)),
              "sf_wire_get_blocks_device")
    return BlockDataRun(h, dev, stream), nreq.value


def place_block_data(row_digests: torch.Tensor, row_sizes: torch.Tensor, row_dst: torch.Tensor,
                     row_present: torch.Tensor, msg_digests: torch.Tensor, msg_sizes: torch.Tensor,
                     msg_offsets: torch.Tensor, msg_ok: Optional[torch.Tensor] = None,
                     stream: Optional[torch.cuda.Stream] = None):
    """A parsed BLOCK_DATA run joined against the destination's incomplete
    rows, on the device (sf_place_block_data_device): the sink's per-message
    ``list_block_locations`` + ``mark_block_present`` loop
    (src/sync/fs.rs:505-510) as one call.

    Rows, in rowid order: ``row_digests`` uint8[n, 20], ``row_sizes``
    int32/uint32[n], ``row_dst`` int64[n] (where the row's block lies in the
    image allocation: ``FileImages.base(name) + offset``) and ``row_present``
    uint8/bool[n], 0 where the row still waits -- updated in place.  Messages:
    what ``wire.receive_block_data_device`` returned (``msg_ok`` its ``ok``;
    None: all).  A waiting row takes the lowest-numbered ok message with its
    digest; when that payload has the row's size the row becomes a job and is
    marked present, else it stays missing and is counted as a size mismatch.

    Returns (src_offsets int64, dst_offsets int64, sizes int32, job_rows
    int64, job_msgs int64, msg_uses int32[m], n_left, n_size_mismatch): the
    jobs in row order -- their destinations are disjoint when the rows' are,
    so the first three lists are one ``copy_blocks`` call -- the row and the
    message of each job, how many jobs each message serves (0: nobody wanted
    it), the rows still waiting and the mismatches.  Blocking."""
    n = _table20(row_digests, "row_digests")
    dev = row_digests.device
    m = _table20(msg_digests, "msg_digests", dev)
    _list32(row_sizes, "row_sizes", n, dev)
    _list64(row_dst, "row_dst", n, dev)
    if row_present is None:
        raise ValueError("row_present is an output too: pass a tensor")
    present = _flags(row_present, "row_present", n, dev)
    _list32(msg_sizes, "msg_sizes", m, dev)
    _list64(msg_offsets, "msg_offsets", m, dev)
    msg_ok = _flags(msg_ok, "msg_ok", m, dev)
    n_jobs, n_left, n_bad = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    with _on(dev, stream):
        uses = torch.empty(m, dtype=torch.int32, device=dev)

        def call(cap):
            a = max(cap, 1)
            src, dst, rows, msgs = (torch.empty(a, dtype=torch.int64, device=dev) for _ in range(4))
            sizes = torch.empty(a, dtype=torch.int32, device=dev)
            rc = lib().sf_place_block_data_device(
                _ptr(row_digests, n), _ptr(row_sizes, n), _ptr(row_dst, n), _ptr(present, n), n,
                _ptr(msg_digests, m), _ptr(msg_sizes, m), _ptr(msg_offsets, m), _ptr(msg_ok, m), m,
                src.data_ptr(), dst.data_ptr(), sizes.data_ptr(), rows.data_ptr(), msgs.data_ptr(), cap,
                _ptr(uses, m), ctypes.byref(n_jobs), ctypes.byref(n_left), ctypes.byref(n_bad),
                _stream_ptr(row_digests, stream))
            return rc, n_jobs.value, (src, dst, sizes, rows, msgs)
        # one job per message is the usual run; a digest wanted in several rows needs more
        k, lists = retry_enospc(call, min(n, m), 2, "sf_place_block_data_device")
    return (*(t[:k] for t in lists), uses, n_left.value, n_bad.value)


def write_to_fd(t: torch.Tensor, fd: int, offset: int = 0, stream: Optional[torch.cuda.Stream] = None) -> int:
    """The bytes of a uint8 HBM tensor written at ``offset`` of the open file
    ``fd`` with pwrite -- the descriptor's position is not used or moved
    (sf_write_device_fd: pinned stages, written by the library's threads while
    the next stage comes back).  The copy starts after what ``stream`` holds at
    the call.  Returns the bytes written; a failed or short write raises
    SfError(SF_EIO) whose ``written`` attribute holds the whole stages known
    written, a descriptor that cannot seek SfError(SF_EINVAL).  Blocking."""
    _require_device(t, "t", torch.uint8)
    nw = ctypes.c_uint64(0)
    with _on(t.device, stream):
        rc = lib().sf_write_device_fd(_ptr(t), t.numel(), int(fd), int(offset), ctypes.byref(nw),
                                      _stream_ptr(t, stream))
    if rc != 0:
        err = SfError(rc, "sf_write_device_fd")
        err.written = nw.value
        raise err
    return nw.value


def read_fd(fd: int, length: int, offset: int = 0, out: Optional[torch.Tensor] = None, stamp=None,
            device=None, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Bytes [offset, offset + length) of the open file ``fd`` as a uint8 HBM
    tensor (sf_read_fd_device, the twin of ``write_to_fd``: pread by the
    library's threads into pinned stages, copied on ``stream`` while the next
    stage is read; the descriptor's position is not used or moved).  ``out``: a
    uint8 HBM tensor of at least ``length`` bytes to read into (any address);
    its first ``length`` bytes are returned.  ``stamp``: the ``FileStamp`` the
    caller took of the file; a file that is another, or that changes during
    the read, raises SfError(SF_EAGAIN), one shorter than asked SfError(SF_EIO),
    a descriptor that cannot seek SfError(SF_EINVAL).  Blocking."""
    length = int(length)
    if length < 0 or offset < 0:
        raise ValueError("length and offset must not be negative")
    if out is not None:
        _require_device(out, "out", torch.uint8)
        if out.numel() < length:
            raise ValueError(f"out holds {out.numel()} bytes, need {length}")
    dev = out.device if out is not None else device_of(device)
    with _on(dev, stream):
        t = out if out is not None else torch.empty(length, dtype=torch.uint8, device=dev)
        check(lib().sf_read_fd_device(int(fd), ctypes.byref(stamp) if stamp is not None else None, int(offset), length,
                                      _ptr(t, length), None, _stream_ptr(t, stream)), "sf_read_fd_device")
    return t[:length]


class PlanCounts(NamedTuple):
    """counts of sf_plan_copies_device, in the order of its SF_PLAN_* indices."""
    jobs: int
    bytes: int
    missing: int
    size_mismatch: int
    stale: int
    unavailable: int
    unverified: int
    empty: int


class CopyPlan(NamedTuple):
    """What ``plan_copies`` returns.  Per block: ``present`` uint8[n], ``ask``
    uint8[n] (``get_block_requests``' ``take``), ``dst`` int64[n]
    (``place_block_data``'s ``row_dst``).  The jobs in block order, one
    ``copy_blocks`` call: ``src_offsets`` / ``dst_offsets`` int64[k], ``sizes``
    int32[k], ``job_blocks`` int64[k].  ``local_jobs`` int32[n_local]: the jobs
    that read each local file.  A query has None for everything but
    ``local_jobs`` and ``counts``."""
    present: Optional[torch.Tensor]
    ask: Optional[torch.Tensor]
    dst: Optional[torch.Tensor]
    src_offsets: Optional[torch.Tensor]
    dst_offsets: Optional[torch.Tensor]
    sizes: Optional[torch.Tensor]
    job_blocks: Optional[torch.Tensor]
    local_jobs: torch.Tensor
    counts: PlanCounts


def plan_copies_stats() -> Tuple[int, int, int, int]:
    """(read-backs, candidates hashed, jobs, 1 for a query) of this process's
    last ``plan_copies`` (sf_test_plan_copies_stats)."""
    out = (ctypes.c_uint64 * 4)()
    check(lib().sf_test_plan_copies_stats(out), "sf_test_plan_copies_stats")
    return tuple(int(v) for v in out)


def plan_copies(digests: torch.Tensor, sizes: torch.Tensor, offsets: torch.Tensor, rows: torch.Tensor,
                block_file: torch.Tensor, file_base: torch.Tensor, table_file: torch.Tensor,
                table_offset: torch.Tensor, table_size: torch.Tensor, local_size: torch.Tensor,
                local_base: Optional[torch.Tensor] = None, src: Optional[torch.Tensor] = None,
                stream: Optional[torch.cuda.Stream] = None) -> CopyPlan:
    """The blocks of a received GetFiles stream that the destination already
    holds, turned into one copy list on the device (sf_plan_copies_device):
    the sink's per-block get_block / read_block / write_block / add_block
    (src/sync/fs.rs:461-471) as one call, with every local block hashed and
    compared with the digest the source announced before it is used.

    Blocks: the first five results of ``BlockSet.receive_files``;
    ``file_base`` int64[m] where each section's byte 0 lies in the image
    allocation (``FileImages.bases``).  The table the set was built from, in
    rowid order: ``table_file`` int32[t] the local file holding each row (the
    caller's numbering), ``table_offset`` int64[t], ``table_size`` int32[t].
    Local files: ``local_size`` int64[l] and ``local_base`` int64[l], where
    each lies in the arena ``src`` (-1, i.e. UINT64_MAX: not loaded).

    ``local_base`` None is a query: only ``local_jobs`` -- how many jobs would
    read each local file, the files worth loading -- and ``counts`` come back.
    ``src`` None plans without verification.  A block found in a row of another
    size, in a file shorter than the row says, in a file that is not loaded, or
    whose bytes no longer hash to its digest keeps present = 0 and asks the
    source.  Blocking: one read-back, two with verification."""
    n = _table20(digests, "digests")
    dev = digests.device
    _list32(sizes, "sizes", n, dev)
    _list64(offsets, "offsets", n, dev)
    _list64(rows, "rows", n, dev)
    _list32(block_file, "block_file", n, dev)
    m, t, nl = file_base.numel(), table_file.numel(), local_size.numel()
    _list64(file_base, "file_base", m, dev)
    _list32(table_file, "table_file", t, dev)
    _list64(table_offset, "table_offset", t, dev)
    _list32(table_size, "table_size", t, dev)
    _list64(local_size, "local_size", nl, dev)
    query = local_base is None
    if not query:
        _list64(local_base, "local_base", nl, dev)
    if src is not None:
        _require_device(src, "src", torch.uint8, dev)
    counts = (ctypes.c_uint64 * 8)()
    with _on(dev, stream):
        local_jobs = torch.empty(nl, dtype=torch.int32, device=dev)
        e = lambda k, dt: None if query else torch.empty(k, dtype=dt, device=dev)  # noqa: E731
        present, ask, dst = e(n, torch.uint8), e(n, torch.uint8), e(n, torch.int64)
        so, do, jb, js = e(n, torch.int64), e(n, torch.int64), e(n, torch.int64), e(n, torch.int32)
        # no local file at all is not a query: the library tells the two apart by the pointer
        lb = local_base if query or nl else torch.zeros(1, dtype=torch.int64, device=dev)
        rc = lib().sf_plan_copies_device(
            _ptr(digests, n), _ptr(sizes, n), _ptr(offsets, n), _ptr(rows, n), _ptr(block_file, n), n,
            _ptr(file_base), m, _ptr(table_file), _ptr(table_offset), _ptr(table_size), t,
            None if query else lb.data_ptr(), _ptr(local_size), nl,
            _ptr(src) if src is not None and not query else None, src.numel() if src is not None else 0,
            _ptr(present), _ptr(ask), _ptr(dst), _ptr(so), _ptr(do), _ptr(js), _ptr(jb), 0 if query else n,
            _ptr(local_jobs), counts, _stream_ptr(digests, stream))
    c = PlanCounts(*(int(v) for v in counts))
    if query:
        if rc not in (0, SF_ENOSPC):
            check(rc, "sf_plan_copies_device")
        return CopyPlan(None, None, None, None, None, None, None, local_jobs, c)
    check(rc, "sf_plan_copies_device")
    k = c.jobs
    return CopyPlan(present, ask, dst, so[:k], do[:k], js[:k], jb[:k], local_jobs, c)


def fill_splitmix(out: torch.Tensor, seed: int, start: int = 0,
                  stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Fill a uint8 HBM buffer with bytes [start, start+len) of the
    splitmix64 stream `seed` (the synthetic input of bench.py / tests)."""
    _require_device(out, "out", torch.uint8)
    with torch.cuda.device(out.device):
        check(lib().sf_fill_splitmix_device(_ptr(out), out.numel(),
                                            seed & 0xFFFFFFFFFFFFFFFF, start, _stream_ptr(out, stream)),
              "sf_fill_splitmix_device")
    return out


def splitmix_tensor(length: int, seed: int, device="cuda", start: int = 0) -> torch.Tensor:
    t = torch.empty(length, dtype=torch.uint8, device=device)
    return fill_splitmix(t, seed, start)
