"""GPU: Index.receive_files_assembled end to end on two small indices.

The destination holds two local files of 4 KiB blocks, indexed; the source
sends three files whose blocks are partly the destination's (in another
order, some twice), partly new, one of them with a short last block and one
empty.  On honest input the assembled route must leave the database as
receive_files leaves it and the images as apply_copies leaves them.  A local
file edited after it was indexed, and one that is gone, cost requests -- and
after the source's BLOCK_DATA the images are the source's files all the same."""
import hashlib
import os
import shutil
from pathlib import PurePath

import numpy as np
import pytest

from syncfast_amd import wire
from syncfast_amd.assemble import FileImages
from syncfast_amd.digest import HashDigest
from syncfast_amd.index import Index, temp_name
from syncfast_amd.timestamp import DateTimeUtc

pytestmark = pytest.mark.gpu

B = 4096
LOCAL = {"old1.bin": 50, "dir/old2.bin": 30}  # blocks
EDITED = 7  # the block of old1.bin that is edited after indexing


def _blocks(data: bytes):
    return [data[o:o + B] for o in range(0, len(data), B)]


@pytest.fixture(scope="module")
def world():
    """(local files' bytes, source files' bytes by name, the GetFiles stream,
    the source's blocks by digest)."""
    rng = np.random.default_rng(2024)
    local = {name: rng.integers(0, 256, n * B, dtype=np.uint8).tobytes() for name, n in LOCAL.items()}
    b1, b2 = _blocks(local["old1.bin"]), _blocks(local["dir/old2.bin"])
    fresh = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    source = {
        # old1's blocks backwards (the edited one once), new blocks between them
        "new1.bin": b"".join(b1[k] + (fresh(B) if k % 5 == 0 else b"") for k in reversed(range(40))),
        # both files' blocks, one of old2's twice, a short last block of its own
        "sub/new2.bin": b"".join(b2[:20]) + b"".join(b1[40:]) + b2[3] + fresh(B) + b"".join(b2[20:]) + fresh(1234),
        "empty.bin": b"",
    }
    stream, by_digest = b"", {}
    for name, data in source.items():
        stream += wire.write_message("FileStart", name.encode())
        for blk in _blocks(data):
            d = hashlib.sha1(blk).digest()
            by_digest[d] = blk
            stream += wire.write_message("FileBlock", d, len(blk))
        stream += wire.write_message("FileEnd")
    return local, source, stream, by_digest


def _destination(root, local):
    """The local files below `root` and the index that knows them, with a temp
    file for every incoming one."""
    idx = Index.open_in_memory()
    for name, data in local.items():
        path = root / name
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_bytes(data)
        fid, _ = idx.add_file(PurePath(name), DateTimeUtc.from_ns(1))
        for k, blk in enumerate(_blocks(data)):
            idx.add_block(HashDigest(hashlib.sha1(blk).digest()), fid, k * B, len(blk))
    for name in ("new1.bin", "sub/new2.bin", "empty.bin"):
        idx.add_temp_file(name)
    idx.commit()
    return idx


def _tables(idx):
    return (idx.db.execute("SELECT rowid, * FROM blocks ORDER BY rowid;").fetchall(),
            idx.db.execute("SELECT * FROM files ORDER BY file_id;").fetchall())


def _answer(idx, by_digest, gpu) -> bytes:
    """The source's BLOCK_DATA run for the requests the index sends."""
    with idx.get_block_requests(device=gpu) as req:
        requests = req.bytes()
    assert len(requests) % 31 == 0
    return b"".join(wire.write_message("BlockData", requests[k + 10:k + 30], by_digest[requests[k + 10:k + 30]])
                    for k in range(0, len(requests), 31))


def _finish(idx, images, by_digest, gpu):
    data = _answer(idx, by_digest, gpu)
    n_jobs, rejected, used, n_left = idx.place_block_data(data, images, device=gpu)
    assert (rejected, used, n_left) == ([], len(data), 0)
    idx.commit()
    return n_jobs


def _requested(idx):
    return [h.bytes for h in idx.list_missing_blocks()]


def test_honest_input_ends_as_receive_files_and_apply_copies_end(gpu, tmp_path, world):
    local, source, stream, by_digest = world
    idx_a, idx_b = _destination(tmp_path, local), Index.open_in_memory()
    idx_a.db.backup(idx_b.db)  # a copy of the index: the temp files' timestamps too
    assert _tables(idx_a) == _tables(idx_b)
    copies, consumed, carry = idx_a.receive_files(stream, device=gpu)
    idx_a.commit()
    assert (consumed, carry) == (len(stream), None)
    images_a = FileImages({temp_name(n): len(d) for n, d in source.items()}, device=gpu, root=tmp_path)
    for name, copy_list in copies.items():
        images_a.apply_copies(name, copy_list)
    images_b, plan, consumed = idx_b.receive_files_assembled(stream, tmp_path, device=gpu)
    idx_b.commit()
    assert consumed == len(stream)
    assert _tables(idx_a) == _tables(idx_b)
    assert np.array_equal(images_a.buffer.cpu().numpy(), images_b.buffer.cpu().numpy())
    held = sum(len(c) for c in copies.values())
    c = plan.counts
    assert (c.jobs, c.bytes, c.unverified, c.stale, c.unavailable, c.size_mismatch, c.empty) == \
        (held, held * B, 0, 0, 0, 0, 0) and c.jobs == 40 + 10 + 30 + 1
    assert c.missing == plan.present.numel() - held == int(plan.ask.sum()) == 8 + 2
    assert plan.local_jobs.cpu().tolist() == [50, 31]
    # both finish alike
    for idx, images in ((idx_a, images_a), (idx_b, images_b)):
        assert _finish(idx, images, by_digest, gpu) == 10
        for name, data in source.items():
            assert bytes(images.image(temp_name(name)).cpu().numpy()) == data
            assert images.check(idx, temp_name(name)) == []
    assert _tables(idx_a) == _tables(idx_b)


def _edit(root):
    path = root / "old1.bin"
    data = bytearray(path.read_bytes())
    data[EDITED * B + 100] ^= 1
    path.write_bytes(bytes(data))


def test_an_edited_local_block_is_requested_from_the_source(gpu, tmp_path, world):
    local, source, stream, by_digest = world
    idx = _destination(tmp_path, local)
    _edit(tmp_path)
    digest = hashlib.sha1(_blocks(local["old1.bin"])[EDITED]).digest()
    images, plan, _consumed = idx.receive_files_assembled(stream, tmp_path, device=gpu, verify=True)
    idx.commit()
    assert (plan.counts.unverified, plan.counts.jobs, plan.counts.missing) == (1, 80, 10)
    fid = idx.get_temp_file(PurePath("new1.bin"))[0]
    offset = source["new1.bin"].index(by_digest[digest])
    assert idx.db.execute("SELECT present FROM blocks WHERE file_id = ? AND offset = ?;",
                          (fid, offset)).fetchone() == (0,)
    assert idx.db.execute("SELECT COUNT(*) FROM blocks WHERE present = 0;").fetchone() == (11,)
    assert digest in _requested(idx) and len(_requested(idx)) == 11
    assert _finish(idx, images, by_digest, gpu) == 11
    for name, data in source.items():
        assert images.check(idx, temp_name(name)) == []
        assert bytes(images.image(temp_name(name)).cpu().numpy()) == data


def test_without_verification_the_edit_reaches_the_image(gpu, tmp_path, world):
    local, source, stream, by_digest = world
    idx = _destination(tmp_path, local)
    _edit(tmp_path)
    images, plan, _consumed = idx.receive_files_assembled(stream, tmp_path, device=gpu, verify=False)
    idx.commit()
    assert (plan.counts.unverified, plan.counts.jobs) == (0, 81)
    assert _finish(idx, images, by_digest, gpu) == 10
    offset = source["new1.bin"].index(_blocks(local["old1.bin"])[EDITED])
    assert images.check(idx, temp_name("new1.bin")) == [offset]  # found at the end, when nobody can be asked
    assert images.check(idx, temp_name("sub/new2.bin")) == [] and images.check(idx, temp_name("empty.bin")) == []


def test_a_local_file_that_is_gone_has_all_its_blocks_requested(gpu, tmp_path, world):
    local, source, stream, by_digest = world
    idx = _destination(tmp_path, local)
    shutil.rmtree(tmp_path / "dir")
    images, plan, _consumed = idx.receive_files_assembled(stream, tmp_path, device=gpu)
    idx.commit()
    c = plan.counts
    assert (c.unavailable, c.jobs, c.stale, c.unverified) == (31, 50, 0, 0)
    assert plan.local_jobs.cpu().tolist() == [50, 0]
    assert len(_requested(idx)) == 10 + 31
    assert _finish(idx, images, by_digest, gpu) == 41
    for name, data in source.items():
        assert images.check(idx, temp_name(name)) == []
        assert bytes(images.image(temp_name(name)).cpu().numpy()) == data
    assert not os.path.exists(tmp_path / "dir")
