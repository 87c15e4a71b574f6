"""GPU: sf_read_fd_device, the loader of the destination's local files, with
1 MiB stages (SF_TEST_STREAM_STAGE_MIB): lengths around one stage and over
three, odd file offsets and odd device addresses, every byte around the read
left as it was; a file shorter than asked, a stamp that does not match, and
the copy ordered after work pending on the caller's stream."""
import ctypes
import os

import numpy as np
import pytest
import torch

import stream_order as so
from syncfast_amd import _lib, device

pytestmark = pytest.mark.gpu

STAGE = 1 << 20
FILL = 0xEE
GUARD = 64


@pytest.fixture(scope="module")
def local_file(tmp_path_factory):
    """3 stages + a bit of bytes that differ at every stage's distance."""
    data = np.random.default_rng(8).integers(0, 256, 3 * STAGE + 4000, dtype=np.uint8)
    path = tmp_path_factory.mktemp("read_fd") / "local.bin"
    data.tofile(path)
    return str(path), data


def _read(fd, stamp, offset, length, dst_ptr, gpu):
    n = ctypes.c_uint64(77)
    rc = _lib.lib().sf_read_fd_device(fd, ctypes.byref(stamp) if stamp is not None else None, offset, length, dst_ptr,
                                      ctypes.byref(n), torch.cuda.current_stream(gpu).cuda_stream)
    return rc, n.value


@pytest.mark.parametrize("shift", [0, 1, 7])
@pytest.mark.parametrize("length", [0, 1, STAGE - 1, STAGE, STAGE + 1, 3 * STAGE + 17])
def test_bytes_arrive_where_they_belong_and_nowhere_else(gpu, knobs, local_file, length, shift):
    knobs.set("SF_TEST_STREAM_STAGE_MIB", 1)
    path, data = local_file
    offset = {0: 0, 1: 1, 7: 3001}[shift]  # odd file offsets with the odd addresses
    buf = torch.full((length + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device=gpu)
    at = GUARD + (shift - buf.data_ptr()) % 16  # `shift` bytes past a 16-byte boundary
    with open(path, "rb") as f:
        os.lseek(f.fileno(), 5, os.SEEK_SET)
        stamp = _lib.FileStamp()
        assert _lib.lib().sf_file_stamp_fd(f.fileno(), stamp) == 0
        rc, n = _read(f.fileno(), stamp, offset, length, buf.data_ptr() + at if length else None, gpu)
        assert os.lseek(f.fileno(), 0, os.SEEK_CUR) == 5  # pread: the position is not used or moved
    assert (rc, n) == (0, length)
    want = np.full(buf.numel(), FILL, np.uint8)
    want[at:at + length] = data[offset:offset + length]
    assert np.array_equal(buf.cpu().numpy(), want)


def test_the_wrapper_reads_into_a_tensor_of_its_own_or_the_callers(gpu, knobs, local_file):
    knobs.set("SF_TEST_STREAM_STAGE_MIB", 1)
    path, data = local_file
    with open(path, "rb") as f:
        t = device.read_fd(f.fileno(), 2 * STAGE + 5, 11, device=gpu)
        assert t.device == gpu and np.array_equal(t.cpu().numpy(), data[11:11 + 2 * STAGE + 5])
        out = torch.zeros(1000, dtype=torch.uint8, device=gpu)
        got = device.read_fd(f.fileno(), 600, 0, out=out[3:])
        assert got.data_ptr() == out.data_ptr() + 3 and np.array_equal(out[3:603].cpu().numpy(), data[:600])
        assert int(out[603:].max()) == 0 and int(out[:3].max()) == 0
        with pytest.raises(ValueError):
            device.read_fd(f.fileno(), 1001, 0, out=out)


def test_a_file_shorter_than_asked_is_eio(gpu, knobs, local_file):
    knobs.set("SF_TEST_STREAM_STAGE_MIB", 1)
    path, data = local_file
    buf = torch.full((data.size + 100,), FILL, dtype=torch.uint8, device=gpu)
    with open(path, "rb") as f:
        rc, n = _read(f.fileno(), None, 0, data.size + 1, buf.data_ptr(), gpu)  # one byte past the end, in stage 3
        assert rc == _lib.SF_EIO and n % STAGE == 0 and n <= 3 * STAGE
        rc, n = _read(f.fileno(), None, data.size - 10, 11, buf.data_ptr(), gpu)
        assert (rc, n) == (_lib.SF_EIO, 0)
        rc, n = _read(f.fileno(), None, data.size - 10, 10, buf.data_ptr(), gpu)  # the last byte is there
        assert (rc, n) == (0, 10)
    torch.cuda.synchronize()
    assert int(buf[data.size + 1:].min()) == FILL  # nothing outside d_dst[0, len)


def test_a_stamp_that_does_not_match_is_eagain(gpu, tmp_path):
    path = tmp_path / "f.bin"
    path.write_bytes(b"a" * 5000)
    buf = torch.full((6000,), FILL, dtype=torch.uint8, device=gpu)
    with open(path, "rb") as f:
        stamp = _lib.FileStamp()
        assert _lib.lib().sf_file_stamp_fd(f.fileno(), stamp) == 0
        assert _read(f.fileno(), stamp, 0, 5000, buf.data_ptr(), gpu) == (0, 5000)
        with open(path, "ab") as g:  # the file grows after it was stamped
            g.write(b"b")
        rc, n = _read(f.fileno(), stamp, 0, 5000, buf.data_ptr() + 500, gpu)
        assert (rc, n) == (_lib.SF_EAGAIN, 0)
        with pytest.raises(_lib.SfError) as e:
            device.read_fd(f.fileno(), 5000, stamp=stamp, device=gpu)
        assert e.value.code == _lib.SF_EAGAIN
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert bytes(got[:5000]) == b"a" * 5000 and (got[5000:] == FILL).all()  # refused before anything was read


def test_the_copy_follows_the_callers_stream(gpu, knobs, local_file):
    """The destination is filled with 0xEE behind a hold on a fresh stream:
    a copy that did not wait for the stream would be overwritten by the fill."""
    knobs.set("SF_TEST_STREAM_STAGE_MIB", 1)
    path, data = local_file
    length = 2 * STAGE + 100
    with open(path, "rb") as f:
        H = so.hold_ms(so.timed_ms(lambda: device.read_fd(f.fileno(), length, device=gpu), gpu))
        S = so.fresh_stream(gpu)
        with torch.cuda.stream(S):
            out = torch.empty(length, dtype=torch.uint8, device=gpu)
            S.synchronize()
            so.hold(S, H)
            out.fill_(FILL)
            got = device.read_fd(f.fileno(), length, out=out, stream=S)
            snap = got.clone()
        S.synchronize()
    measured, asked = so.held_ms(S)
    assert measured >= asked
    assert np.array_equal(snap.cpu().numpy(), data[:length])
