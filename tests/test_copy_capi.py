"""CPU: what sf_copy_blocks_device and sf_write_device_fd answer before any
device call -- argument errors, the empty list -- and that the new symbols are
part of the binding table."""
import ctypes

import numpy as np

import syncfast_amd
from syncfast_amd import _lib


def _lists(n=3):
    return (np.zeros(n, np.uint64), np.arange(n, dtype=np.uint64) * 8, np.full(n, 8, np.uint32))


def test_new_symbols_are_bound():
    assert "sf_copy_blocks_device" in _lib.EXPORTED and "sf_write_device_fd" in _lib.EXPORTED
    assert "sf_test_copy_stats" in _lib.EXPORTED_TEST
    L = syncfast_amd.lib()
    for name in ("sf_copy_blocks_device", "sf_write_device_fd", "sf_test_copy_stats"):
        assert getattr(L, name)


def test_empty_list_is_ok_and_launches_nothing():
    L = syncfast_amd.lib()
    assert L.sf_copy_blocks_device(None, 0, None, 0, None, None, None, None, 0, None, None) == _lib.SF_OK
    buf = np.zeros(64, np.uint8)
    assert L.sf_copy_blocks_device(buf.ctypes.data, 32, buf.ctypes.data + 32, 32, None, None, None, None, 0, None,
                                   None) == _lib.SF_OK
    out = (ctypes.c_uint64 * 4)(9, 9, 9, 9)
    assert L.sf_test_copy_stats(out) == _lib.SF_OK
    T = out[0]
    assert T >= 1024 and T & (T - 1) == 0  # a power of two that holds a wave's 16-byte stores
    assert list(out)[1:] == [0, 0, 0]
    assert L.sf_test_copy_stats(None) == _lib.SF_EINVAL


def test_argument_errors_come_before_any_device_call():
    """Host memory stands in for the buffers: nothing may be launched or read."""
    L = syncfast_amd.lib()
    a, b = np.zeros(256, np.uint8), np.zeros(256, np.uint8)
    so, do, sz = _lists()
    good = [a.ctypes.data, 256, b.ctypes.data, 256, so.ctypes.data, do.ctypes.data, sz.ctypes.data, None, 3, None, None]
    for k in (0, 2, 4, 5, 6):  # a NULL buffer, a NULL list
        args = list(good)
        args[k] = None
        assert L.sf_copy_blocks_device(*args) == _lib.SF_EINVAL, k
    # the two buffers overlap: by one byte, one inside the other, the same
    both = np.zeros(512, np.uint8)
    p = both.ctypes.data
    for s, sl, d, dl in ((p, 256, p + 255, 256), (p + 255, 256, p, 256), (p, 512, p + 100, 10), (p + 100, 10, p, 512),
                         (p, 512, p, 512)):
        args = list(good)
        args[0:4] = [s, sl, d, dl]
        assert L.sf_copy_blocks_device(*args) == _lib.SF_EINVAL, (s - p, sl, d - p, dl)
    args = list(good)
    args[8] = (1 << 32) + 1  # more jobs than a call takes
    assert L.sf_copy_blocks_device(*args) == _lib.SF_EINVAL
    out = (ctypes.c_uint64 * 4)()
    assert L.sf_test_copy_stats(out) == _lib.SF_OK and list(out)[1:] == [0, 0, 0]


def test_write_device_fd_argument_errors(tmp_path):
    import os
    L = syncfast_amd.lib()
    buf = np.zeros(16, np.uint8)
    nw = ctypes.c_uint64(7)
    assert L.sf_write_device_fd(buf.ctypes.data, 16, -1, 0, ctypes.byref(nw), None) == _lib.SF_EINVAL
    assert nw.value == 0
    r, w = os.pipe()
    try:
        nw.value = 7
        assert L.sf_write_device_fd(buf.ctypes.data, 16, w, 0, ctypes.byref(nw), None) == _lib.SF_EINVAL
        assert nw.value == 0
    finally:
        os.close(r)
        os.close(w)
    fd = os.open(tmp_path / "f", os.O_RDWR | os.O_CREAT)
    try:
        assert L.sf_write_device_fd(None, 0, fd, 0, ctypes.byref(nw), None) == _lib.SF_OK  # nothing to write
        assert L.sf_write_device_fd(None, 16, fd, 0, None, None) == _lib.SF_EINVAL
        assert os.fstat(fd).st_size == 0
    finally:
        os.close(fd)
