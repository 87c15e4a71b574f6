"""GPU: sf_write_device_fd / device.write_to_fd -- an HBM tensor to an open
file through the pinned stages, with pwrite."""
import os

import pytest
import torch

from syncfast_amd import _lib, device

pytestmark = pytest.mark.gpu

MIB = 1 << 20


@pytest.fixture(scope="module")
def content(gpu):
    t = device.splitmix_tensor(5 * MIB + 3 + 1, 4242, gpu)  # one byte more: the views below do not start the allocation
    return t[1:], bytes(t[1:].cpu().numpy())


@pytest.mark.parametrize("offset", [0, 4097])
@pytest.mark.parametrize("length", [0, 1, MIB - 1, MIB, 2 * MIB + 1, 5 * MIB + 3])
def test_lengths_and_offsets_with_one_mib_stages(gpu, knobs, tmp_path, content, length, offset):
    """1 MiB stages: lengths below, at and above a stage and of several, at
    file offset 0 and at an odd one.  The file reads back equal to the tensor,
    the bytes before the offset are unchanged, the position does not move."""
    knobs.set("SF_TEST_STREAM_STAGE_MIB", 1)
    t, host = content
    before = bytes(range(256)) * 17  # 4352 bytes that were there
    path = tmp_path / "out.bin"
    path.write_bytes(before)
    fd = os.open(path, os.O_RDWR)
    try:
        os.lseek(fd, 123, os.SEEK_SET)
        assert device.write_to_fd(t[:length], fd, offset) == length
        assert os.lseek(fd, 0, os.SEEK_CUR) == 123
    finally:
        os.close(fd)
    got = path.read_bytes()
    want = bytearray(before)
    want[offset:offset + length] = host[:length]
    if length == 0:
        assert got == before
    else:
        assert len(got) == max(len(before), offset + length)
        assert got[:offset] == before[:offset]
        assert got == bytes(want)


def test_written_after_the_callers_stream(gpu, knobs, tmp_path):
    """The bytes are produced on the caller's stream just before the call."""
    knobs.set("SF_TEST_STREAM_STAGE_MIB", 1)
    st = torch.cuda.Stream(gpu)
    with torch.cuda.stream(st):
        t = torch.zeros(3 * MIB + 5, dtype=torch.uint8, device=gpu)
        device.fill_splitmix(t, 7, stream=st)
    fd = os.open(tmp_path / "s.bin", os.O_RDWR | os.O_CREAT)
    try:
        assert device.write_to_fd(t, fd, 0, stream=st) == t.numel()
    finally:
        os.close(fd)
    st.synchronize()
    assert (tmp_path / "s.bin").read_bytes() == bytes(t.cpu().numpy())


def test_a_pipe_is_einval(gpu, content):
    t, _ = content
    r, w = os.pipe()
    try:
        with pytest.raises(_lib.SfError) as e:
            device.write_to_fd(t[:100], w)
        assert e.value.code == _lib.SF_EINVAL and e.value.written == 0
    finally:
        os.close(r)
        os.close(w)


def test_a_read_only_descriptor_is_eio_with_nothing_written(gpu, knobs, tmp_path, content):
    knobs.set("SF_TEST_STREAM_STAGE_MIB", 1)
    t, _ = content
    path = tmp_path / "ro.bin"
    path.write_bytes(b"keep")
    fd = os.open(path, os.O_RDONLY)
    try:
        with pytest.raises(_lib.SfError) as e:
            device.write_to_fd(t[:3 * MIB], fd)
        assert e.value.code == _lib.SF_EIO and e.value.written == 0
    finally:
        os.close(fd)
    assert path.read_bytes() == b"keep"
