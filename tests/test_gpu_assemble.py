"""GPU: the incoming files assembled in HBM (syncfast_amd.assemble.FileImages)
-- the scenario of test_gpu_recv_data.py's end-to-end test with the images in
place of the Python write loop, and with a local half: some blocks already sit
in a file of the destination."""
import hashlib
import os
import random
from pathlib import PurePath

import numpy as np
import pytest
import torch

from data_expect import expected, message
from syncfast_amd import wire
from syncfast_amd.assemble import FileImages, _rounds
from syncfast_amd.digest import HashDigest
from syncfast_amd.index import Index, temp_name
from syncfast_amd.timestamp import DateTimeUtc


def _digest(b: bytes) -> HashDigest:
    return HashDigest(hashlib.sha1(b).digest())


def _flip(run: bytes, at: int) -> bytes:
    return run[:at] + bytes([run[at] ^ 0x10]) + run[at + 1:]


def _image(images, name) -> bytes:
    return bytes(images.image(name).cpu().numpy())


@pytest.mark.gpu
def test_images_in_place_of_the_write_loop(gpu, tmp_path):
    rng = random.Random(61)
    blocks = [rng.randbytes(s) for s in (5000, 1, 32768, 0, 777, 4096)]  # these arrive as BLOCK_DATA
    local = [rng.randbytes(s) for s in (3000, 9001)]                      # these the destination holds
    pad = rng.randbytes(101)
    # the destination's own file: pad, local[0], local[1]
    (tmp_path / "old.bin").write_bytes(pad + local[0] + local[1])
    idx = Index.open_in_memory()
    old_id, _ = idx.add_file(PurePath("old.bin"), DateTimeUtc.from_ns(1))
    at = 0
    for b in (pad, local[0], local[1]):
        idx.add_block(_digest(b), old_id, at, len(b))
        at += len(b)
    idx.commit()
    pool = {i: b for i, b in enumerate(blocks)}
    pool.update({"L0": local[0], "L1": local[1]})
    files = {"a.bin": [0, "L0", 1, 2, 0, "L1", 3], "sub/b.bin": [4, 2, "L1", 5]}
    source = {name: b"".join(pool[k] for k in order) for name, order in files.items()}
    # GetFiles: each incoming file's FILE_BLOCK run; the local blocks come back as copies
    copies = {}
    for name, order in files.items():
        fid = idx.add_temp_file(name)
        run = b"".join(wire.write_message("FileBlock", _digest(pool[k]), len(pool[k])) for k in order)
        copies[name] = idx.receive_file_blocks(fid, run + wire.write_message("FileEnd"), device=gpu)
    assert [c[3] for c in copies["a.bin"]] == [3000, 9001] and [c[3] for c in copies["sub/b.bin"]] == [9001]
    idx.commit()
    # GetBlocks: the rest as BLOCK_DATA, block 4 corrupted, the next message not yet whole
    run = b"".join(message(b) for b in blocks)
    run = _flip(run, expected(run)[2][4] + 100)
    data = run + message(rng.randbytes(50))[:60]
    writes, rejected, consumed = idx.receive_block_data(data, device=gpu)
    assert consumed == len(run) and rejected == [_digest(blocks[4])]

    images = FileImages({temp_name(name): len(source[name]) for name in files}, device=gpu, root=tmp_path)
    for name in files:
        assert images.apply_copies(temp_name(name), copies[name]) == 1  # one source file, one call
    assert images.apply_writes(writes, data) == 1
    want_b = bytearray(source["sub/b.bin"])
    want_b[:777] = bytes(777)  # the rejected block was not written: still zero
    assert _image(images, temp_name("a.bin")) == source["a.bin"]
    assert _image(images, temp_name("sub/b.bin")) == bytes(want_b)
    assert images.check(idx, temp_name("a.bin")) == []
    assert images.check(idx, temp_name("sub/b.bin")) == [0]  # exactly the rejected block's offset
    # the source sends the block again
    again = message(blocks[4])
    writes, rejected, _ = idx.receive_block_data(again, device=gpu)
    assert rejected == [] and idx.list_missing_blocks() == []
    run_t = torch.frombuffer(bytearray(again), dtype=torch.uint8).to(gpu)
    assert images.apply_writes(writes, run_t) == 1  # the run as an HBM tensor
    assert images.check(idx, temp_name("sub/b.bin")) == []
    # to the temp files
    (tmp_path / "sub").mkdir()
    for name in files:
        path = tmp_path / temp_name(name)
        fd = os.open(path, os.O_RDWR | os.O_CREAT)
        try:
            assert images.write(temp_name(name), fd) == len(source[name])
        finally:
            os.close(fd)
        assert path.read_bytes() == source[name]
    # a block of the image damaged afterwards is found by the check
    images.image(temp_name("a.bin"))[5000 + 3000] ^= 1  # the one byte of block 1
    assert images.check(idx, temp_name("a.bin")) == [8000]


def _unverified(gpu, rows, size):
    """An index whose temp file c has the given (payload, offset) rows missing,
    and its image."""
    idx = Index.open_in_memory()
    fid = idx.add_temp_file("c")
    for payload, offset in rows:
        idx.add_missing_block(_digest(payload), fid, offset, len(payload))
    idx.commit()
    return idx, FileImages({temp_name("c"): size}, device=gpu)


@pytest.mark.gpu
def test_two_payloads_claim_one_digest_the_last_one_stays(gpu):
    rng = random.Random(62)
    real = rng.randbytes(600)
    first, second = rng.randbytes(600), rng.randbytes(600)
    idx, images = _unverified(gpu, [(real, 7)], 700)
    h = _digest(real).bytes
    data = message(first, h) + message(second, h)
    writes, rejected, _ = idx.receive_block_data(data, device=gpu, verify=False)
    assert rejected == [] and len(writes) == 2 and writes[0][:2] == writes[1][:2]
    assert images.apply_writes(writes, data) == 1
    assert _image(images, temp_name("c")) == bytes(7) + second + bytes(93)
    assert images.check(idx, temp_name("c")) == [7]  # and the check says it is not the announced block


@pytest.mark.gpu
@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0), (1, 2, 0)])
def test_a_payload_longer_than_its_row_lands_as_the_sequential_loop_writes_it(gpu, order):
    rng = random.Random(63)
    rows = [(rng.randbytes(100), 0), (rng.randbytes(100), 100), (rng.randbytes(100), 200)]
    idx, images = _unverified(gpu, rows, 330)
    longer = [rng.randbytes(130), rng.randbytes(150), rng.randbytes(110)]  # each runs into the next row
    data = b"".join(message(longer[k], _digest(rows[k][0]).bytes) for k in order)
    writes, _, _ = idx.receive_block_data(data, device=gpu, verify=False)
    assert [w[3] for w in writes] == [len(longer[k]) for k in order]
    want = bytearray(330)
    for _name, offset, start, size in writes:  # the reference's loop: in message order
        want[offset:offset + size] = data[start:start + size]
    calls = images.apply_writes(writes, data)
    assert _image(images, temp_name("c")) == bytes(want)
    assert calls == {(0, 1, 2): 3, (2, 1, 0): 3, (1, 2, 0): 2}[order]  # rows 0 and 2 do not overlap


@pytest.mark.gpu
def test_a_write_past_the_end_of_its_file_raises_and_nothing_changes(gpu):
    rng = random.Random(64)
    rows = [(rng.randbytes(50), 0), (rng.randbytes(50), 50)]
    idx, images = _unverified(gpu, rows, 100)
    data = message(rows[0][0]) + message(rng.randbytes(51), _digest(rows[1][0]).bytes)
    writes, _, _ = idx.receive_block_data(data, device=gpu, verify=False)
    assert len(writes) == 2
    with pytest.raises(ValueError):
        images.apply_writes(writes, data)
    assert _image(images, temp_name("c")) == bytes(100)  # not even the good one was launched
    with pytest.raises(ValueError):
        images.apply_copies(temp_name("c"), [(PurePath("x"), 0, 90, 11)], source=lambda name: images.buffer)
    with pytest.raises(KeyError):
        images.apply_writes([(PurePath("nope"), 0, 0, 1)], data)
    assert _image(images, temp_name("c")) == bytes(100)


def test_rounds_keep_the_later_write_on_top():
    """(host only) the split of an overlapping list into calls."""
    assert _rounds([]) == []
    assert _rounds([(0, 0, 10), (10, 10, 10), (20, 30, 5)]) == [[(0, 0, 10), (10, 10, 10), (20, 30, 5)]]
    a, b, c, d = (0, 0, 10), (10, 5, 10), (20, 12, 2), (30, 100, 4)
    assert _rounds([a, b, c, d]) == [[d, a], [b], [c]]
    assert _rounds([c, a, d, b]) == [[d, c, a], [b]]
    got = _rounds([(i, 3 * i, 4) for i in range(50)])  # a chain: each overlaps the one before
    assert [len(r) for r in got] == [1] * 50 and np.array_equal([r[0][0] for r in got], range(50))
