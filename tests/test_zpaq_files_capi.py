"""CPU: the C-ABI of the many-file device ZPAQ cut -- sf_cut_device_zpaq_files,
sf_index_device_zpaq_files, sf_index_fds_zpaq and the hook
sf_test_zpaq_files_stats -- without a device: the symbols are bound, every
argument error of include/syncfast_amd.h comes back before any device call
(the device addresses here are made up and nothing may touch them), a call
with no file is SF_OK, and ZpaqChunker(device=False) does not take the new
route."""
import ctypes
import os

import numpy as np
import pytest

from syncfast_amd import _lib, host
from syncfast_amd.index import Index, ZpaqChunker

R = ctypes.byref
IN, OUT = 0x10000, 0x40000  # a made-up input buffer of 4096 bytes; the base of the outputs
CUT, INDEX, FDS, HOOK = ("sf_cut_device_zpaq_files", "sf_index_device_zpaq_files", "sf_index_fds_zpaq",
                         "sf_test_zpaq_files_stats")


def _cut(offs, lens, bits=6, max_size=256, o=OUT, z=OUT + 0x1000, fr=OUT + 0x2000, d=None, data_len=4096, cap=100,
         index=False):
    """(rc, n_blocks, n_unsettled, bad_file) of one call."""
    fo, fl = np.array(offs, np.uint64), np.array(lens, np.uint64)
    nb, nu, bad = ctypes.c_uint64(7), ctypes.c_uint32(7), ctypes.c_uint32(7)
    head = (IN, data_len, fo.ctypes.data, fl.ctypes.data, len(offs), bits, max_size, 0, o, z)
    if index:
        rc = _lib.lib().sf_index_device_zpaq_files(*head, d, cap, fr, R(nb), None, None, R(nu), R(bad), None)
    else:
        rc = _lib.lib().sf_cut_device_zpaq_files(*head, cap, fr, R(nb), None, R(nu), R(bad), None)
    return rc, nb.value, nu.value, bad.value


def test_the_symbols_are_bound_and_declared():
    assert {CUT, INDEX, FDS} <= set(_lib.EXPORTED) and HOOK in _lib.EXPORTED_TEST
    for name in (CUT, INDEX, FDS, HOOK):
        assert getattr(_lib.lib(), name).argtypes is not None
    assert len(_lib._PUBLIC[CUT][1]) == 17 and len(_lib._PUBLIC[INDEX][1]) == 19 and len(_lib._PUBLIC[FDS][1]) == 13


@pytest.mark.parametrize("index", [False, True])
def test_parameters_outside_the_device_range_are_einval(index):
    for bits, max_size in ((0, 256), (32, 256), (6, 15), (6, (1 << 20) + 1)):
        assert _cut([0], [100], bits, max_size, index=index, d=OUT + 0x3000) == (_lib.SF_EINVAL, 0, 0, 0)


@pytest.mark.parametrize("index", [False, True])
def test_misaligned_outputs_are_einval(index):
    d = OUT + 0x3000
    for kw in ({"o": OUT + 1}, {"o": OUT + 4}, {"z": OUT + 0x1001}, {"z": OUT + 0x1002}, {"fr": OUT + 0x2001},
               {"fr": OUT + 0x2004}):
        assert _cut([0], [100], index=index, d=d, **kw) == (_lib.SF_EINVAL, 0, 0, 0), kw
    if index:
        for off in (1, 2, 3):
            assert _cut([0], [100], index=True, d=d + off) == (_lib.SF_EINVAL, 0, 0, 0)
    # NULL host arrays with files to read them for
    nb = ctypes.c_uint64(7)
    assert _lib.lib().sf_cut_device_zpaq_files(IN, 4096, None, None, 2, 6, 256, 0, OUT, OUT, 10, OUT, R(nb), None, None,
                                               None, None) == _lib.SF_EINVAL
    assert _lib.lib().sf_cut_device_zpaq_files(IN, 4096, None, None, 0, 6, 256, 0, OUT, OUT, 10, None, None, None, None,
                                               None, None) == _lib.SF_EINVAL  # no n_blocks


@pytest.mark.parametrize("index", [False, True])
def test_a_file_outside_the_buffer_is_erange_and_named(index):
    d = OUT + 0x3000
    assert _cut([0, 4000, 10], [10, 97, 5], index=index, d=d) == (_lib.SF_ERANGE, 0, 0, 1)  # one byte past the end
    assert _cut([0, 10, 4097], [10, 5, 0], index=index, d=d) == (_lib.SF_ERANGE, 0, 0, 2)   # empty, but past the end
    assert _cut([2 ** 64 - 1], [2], index=index, d=d) == (_lib.SF_ERANGE, 0, 0, 0)          # off + len passes 2^64
    assert _cut([5], [2 ** 64 - 1], index=index, d=d) == (_lib.SF_ERANGE, 0, 0, 0)
    assert _cut([4096, 0], [0, 0], index=index, d=d, fr=None) == (0, 0, 0, 0)  # an empty file at the very end lies inside


@pytest.mark.parametrize("index", [False, True])
def test_no_file_and_only_empty_files_need_no_device(index):
    assert _cut([], [], index=index, fr=None) == (0, 0, 0, 0)
    assert _cut([3, 3, 9], [0, 0, 0], index=index, fr=None, o=None, z=None, cap=0) == (0, 0, 0, 0)
    stats = (ctypes.c_uint64 * 6)(*[9] * 6)
    assert _lib.lib().sf_test_zpaq_files_stats(stats) == 0 and list(stats) == [0] * 6
    assert _lib.lib().sf_test_zpaq_files_stats(None) == _lib.SF_EINVAL


def test_blocks_hashes_of_empty_files_without_a_device():
    import hashlib
    fo, fl = np.zeros(3, np.uint64), np.zeros(3, np.uint64)
    nb, bh = ctypes.c_uint64(7), np.full(60, 7, np.uint8)
    rc = _lib.lib().sf_index_device_zpaq_files(IN, 4096, fo.ctypes.data, fl.ctypes.data, 3, 6, 256, 0, None, None, None, 0,
                                               None, R(nb), bh.ctypes.data, None, None, None, None)
    assert (rc, nb.value) == (0, 0) and bh.tobytes() == hashlib.sha1(b"").digest() * 3


def test_index_fds_zpaq_argument_errors_and_no_file():
    rows, first, hashes, status = host.index_fds_zpaq([], 6, 256)
    assert rows.size == 0 and first.tolist() == [0] and hashes.shape == (0, 20) and status.size == 0
    p, n = ctypes.POINTER(_lib.BlockSig)(), ctypes.c_uint64(7)
    f = lambda *a: _lib.lib().sf_index_fds_zpaq(*a)
    fd = np.array([0], np.int32)
    first, bh = np.zeros(2, np.uint64), np.zeros(20, np.uint8)
    fp = first.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    for bits, max_size in ((0, 256), (32, 256), (6, 15), (6, (1 << 20) + 1)):
        assert f(fd.ctypes.data, None, 1, bits, max_size, 0, 0, R(p), R(n), fp, bh.ctypes.data, None, None) == _lib.SF_EINVAL
        assert not p and n.value == 0
    assert f(fd.ctypes.data, None, 1, 6, 256, 0, 0, None, R(n), fp, bh.ctypes.data, None, None) == _lib.SF_EINVAL
    assert f(None, None, 1, 6, 256, 0, 0, R(p), R(n), fp, bh.ctypes.data, None, None) == _lib.SF_EINVAL
    assert f(fd.ctypes.data, None, 1, 6, 256, 0, 0, R(p), R(n), None, bh.ctypes.data, None, None) == _lib.SF_EINVAL
    with pytest.raises(ValueError):
        host.index_fds_zpaq([0, 1], 6, 256, stamps=[])


def test_files_that_fail_alone_need_no_device(tmp_path):
    """A pipe, a closed descriptor, a stale stamp and an empty file: nothing
    is read, so no device is touched; each file has its own status, no rows,
    and the empty file SHA-1("")."""
    import hashlib
    (tmp_path / "a").write_bytes(b"x" * 100)
    (tmp_path / "e").write_bytes(b"")
    r, w = os.pipe()
    with open(tmp_path / "a", "rb") as a, open(tmp_path / "e", "rb") as e:
        stale = host.file_stamp(a.fileno())
        stale.mtime_nsec += 1
        stamps = [host.file_stamp(e.fileno()), host.file_stamp(e.fileno()), stale, host.file_stamp(e.fileno())]
        rows, first, hashes, status = host.index_fds_zpaq([r, e.fileno(), a.fileno(), -1], 6, 256, stamps)
    os.close(r)
    os.close(w)
    assert status.tolist() == [_lib.SF_EINVAL, 0, _lib.SF_EAGAIN, _lib.SF_EINVAL]
    assert rows.size == 0 and first.tolist() == [0] * 5
    assert bytes(hashes[1]) == hashlib.sha1(b"").digest() and not hashes[[0, 2, 3]].any()


def test_the_host_chunker_does_not_take_the_new_route(tmp_path, monkeypatch):
    """Index.index_path with ZpaqChunker(device=False) takes exactly the
    route it took before: host.index_fds_zpaq is never called (it would
    raise), the files go to the cutting pool and host.index_fds_blocks."""
    (tmp_path / "t").mkdir()
    for k in range(3):
        (tmp_path / "t" / f"f{k}").write_bytes(bytes([k]) * (1000 * k))
    calls = []

    def boom(*a, **kw):
        raise AssertionError("ZpaqChunker(device=False) went to sf_index_fds_zpaq")

    def fake_blocks(fds, lists, stamps=None, stage_bytes=0):
        calls.append(len(fds))
        raise _lib.SfError(_lib.SF_ENODEV, "stop here: the test needs no device")
    monkeypatch.setattr(host, "index_fds_zpaq", boom)
    monkeypatch.setattr(host, "index_fds_blocks", fake_blocks)
    assert ZpaqChunker().device is False and ZpaqChunker().max_rounds == host.ZPAQ_MAX_ROUNDS
    idx = Index.open(tmp_path / "i.db", ZpaqChunker())
    with pytest.raises(_lib.SfError):
        idx.index_path(tmp_path / "t")
    assert calls == [3]
    # and device=True hands the batch to the new call, uncut
    seen = []

    def fake_zpaq(fds, bits, max_size, stamps, max_rounds, stage_bytes):
        seen.append((len(fds), bits, max_size, len(stamps), max_rounds, stage_bytes))
        raise _lib.SfError(_lib.SF_ENODEV, "stop here: the test needs no device")
    monkeypatch.setattr(host, "index_fds_zpaq", fake_zpaq)
    idx2 = Index.open(tmp_path / "j.db", ZpaqChunker(6, 256, device=True, max_rounds=5))
    with pytest.raises(_lib.SfError):
        idx2.index_path(tmp_path / "t", batch_bytes=1 << 20)
    assert seen == [(3, 6, 256, 3, 5, 1 << 20)] and calls == [3]
