"""CPU: the copy plan and the local-file loader as far as no device is needed
(sf_plan_copies_device, sf_read_fd_device): the symbols and the Python names,
every argument check that comes before any device call, the plan of no blocks,
and Index.receive_files_assembled refusing a stream that carries a file in or
out before it uploads anything."""
import ctypes
import os

import pytest

import syncfast_amd
from syncfast_amd import _lib
from syncfast_amd.index import Index

EINVAL = _lib.SF_EINVAL
NAMES = ("digests", "sizes", "offsets", "rows", "block_file", "n_blocks", "file_base", "n_files", "table_file",
         "table_offset", "table_size", "n_table", "local_base", "local_size", "n_local", "src", "src_len", "present",
         "ask", "dst", "src_offsets", "dst_offsets", "job_sizes", "job_blocks", "cap", "local_jobs")


def _args(a, **change):
    """A call with one block, section, row and local file whose every list is
    `a` (8-B aligned host memory that no failing call reads), then the changes."""
    args = {k: a for k in NAMES}
    args.update(n_blocks=1, n_files=1, n_table=1, n_local=1, src_len=8, cap=1)
    args.update(change)
    return tuple(args[k] for k in NAMES)


def test_symbols_and_python_names():
    L = syncfast_amd.lib()
    assert {"sf_plan_copies_device", "sf_read_fd_device"} <= set(_lib.EXPORTED)
    assert "sf_test_plan_copies_stats" in _lib.EXPORTED_TEST
    assert callable(L.sf_plan_copies_device) and callable(L.sf_read_fd_device)
    from syncfast_amd import device
    from syncfast_amd.assemble import FileImages, LocalFiles
    assert callable(device.plan_copies) and callable(device.read_fd) and callable(device.plan_copies_stats)
    assert device.CopyPlan._fields[-2:] == ("local_jobs", "counts")
    assert device.PlanCounts._fields == ("jobs", "bytes", "missing", "size_mismatch", "stale", "unavailable",
                                         "unverified", "empty")
    assert callable(FileImages.bases) and callable(LocalFiles.bases) and callable(LocalFiles.sizes)
    assert callable(Index.receive_files_assembled)


def test_plan_checks_arguments_before_any_device_call():
    L = syncfast_amd.lib()
    buf = (ctypes.c_uint64 * 8)()
    a = ctypes.addressof(buf)
    counts = (ctypes.c_uint64 * 8)(*[7] * 8)
    # no place for the counts, with and without blocks
    assert L.sf_plan_copies_device(*_args(a), None, None) == EINVAL
    assert L.sf_plan_copies_device(*_args(None, n_blocks=0, n_files=0, n_table=0, n_local=0, cap=0), None, None) == EINVAL
    bad = [{k: (1 << 31) + 1} for k in ("n_blocks", "n_files", "n_table", "n_local")]
    bad += [{k: None} for k in ("digests", "sizes", "offsets", "rows", "block_file", "file_base", "table_file",
                                "table_offset", "table_size", "local_size", "present", "ask", "dst")]
    bad += [{k: a + 2} for k in ("digests", "sizes", "block_file", "table_file", "table_size", "job_sizes",
                                 "local_jobs")]
    bad += [{k: a + 4} for k in ("offsets", "rows", "file_base", "table_offset", "local_base", "local_size", "dst",
                                 "src_offsets", "dst_offsets", "job_blocks")]
    for change in bad:
        assert L.sf_plan_copies_device(*_args(a, **change), counts, None) == EINVAL, change
        assert list(counts) == [7] * 8  # untouched
    # a misaligned list is refused with no blocks too: nothing is read from it, but the caller's bug is there
    assert L.sf_plan_copies_device(*_args(a, n_blocks=0, dst=a + 4), counts, None) == EINVAL
    stats = (ctypes.c_uint64 * 4)(9, 9, 9, 9)
    assert L.sf_test_plan_copies_stats(stats) == 0 and list(stats) == [0, 0, 0, 0]
    assert L.sf_test_plan_copies_stats(None) == EINVAL


def test_no_blocks_need_no_device():
    L = syncfast_amd.lib()
    counts = (ctypes.c_uint64 * 8)(*[7] * 8)
    none = _args(None, n_blocks=0, n_files=0, n_table=0, n_local=0, cap=0)
    assert L.sf_plan_copies_device(*none, counts, None) == 0 and list(counts) == [0] * 8
    # lists of a full call with no blocks in them, the counters' list left out
    buf = (ctypes.c_uint64 * 8)()
    counts = (ctypes.c_uint64 * 8)(*[7] * 8)
    args = _args(ctypes.addressof(buf), n_blocks=0, local_jobs=None)
    assert L.sf_plan_copies_device(*args, counts, None) == 0 and list(counts) == [0] * 8
    assert list(buf) == [0] * 8


def test_read_fd_checks_arguments_before_any_device_call(tmp_path):
    L = syncfast_amd.lib()
    n = ctypes.c_uint64(7)
    buf = (ctypes.c_uint64 * 8)()
    a = ctypes.addressof(buf)
    assert L.sf_read_fd_device(-1, None, 0, 8, a, ctypes.byref(n), None) == EINVAL and n.value == 0
    r, w = os.pipe()
    try:
        for fd in (r, w):  # a descriptor that cannot seek, with and without bytes to read
            n.value = 7
            assert L.sf_read_fd_device(fd, None, 0, 8, a, ctypes.byref(n), None) == EINVAL and n.value == 0
            assert L.sf_read_fd_device(fd, None, 0, 0, None, None, None) == EINVAL
    finally:
        os.close(r)
        os.close(w)
    path = tmp_path / "f.bin"
    path.write_bytes(b"x" * 100)
    with open(path, "rb") as f:
        n.value = 7
        assert L.sf_read_fd_device(f.fileno(), None, 0, 8, None, ctypes.byref(n), None) == EINVAL and n.value == 0
        # nothing to read: no device, and the stamp is still held against the file
        assert L.sf_read_fd_device(f.fileno(), None, 0, 0, None, ctypes.byref(n), None) == 0 and n.value == 0
        assert L.sf_read_fd_device(f.fileno(), None, 100, 0, a, None, None) == 0
        stamp = _lib.FileStamp()
        assert L.sf_file_stamp_fd(f.fileno(), stamp) == 0
        assert L.sf_read_fd_device(f.fileno(), stamp, 0, 0, None, None, None) == 0
        stamp.size += 1
        assert L.sf_read_fd_device(f.fileno(), stamp, 0, 0, None, None, None) == _lib.SF_EAGAIN
    assert list(buf) == [0] * 8


@pytest.mark.parametrize("data", [
    b"FILE_BLOCK\n" + bytes(20) + b"5\nFILE_END\n",                      # a file carried in
    b"FILE_START\na.bin\nFILE_BLOCK\n" + bytes(20) + b"5\n",             # a file carried out
    b"FILE_START\na.bin\nFILE_BLOCK\n" + bytes(20) + b"5\nFILE_END\nFILE_START\nb.bin\n",
    b"FILE_END\n",
])
def test_receive_files_assembled_takes_a_whole_stream_only(data, tmp_path):
    idx = Index.open_in_memory()
    idx.add_temp_file("a.bin")
    idx.commit()
    before = idx.db.execute("SELECT COUNT(*) FROM blocks;").fetchone()
    with pytest.raises(ValueError, match="whole GetFiles stream"):
        idx.receive_files_assembled(data, tmp_path)
    assert idx.db.execute("SELECT COUNT(*) FROM blocks;").fetchone() == before
