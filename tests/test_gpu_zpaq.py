"""GPU: the reference's content-defined (ZPAQ) boundaries cut on the device
(sf_cut_device_zpaq, sf_index_device_zpaq, sf_index_fd_zpaq,
index.ZpaqChunker(device=True)).  Every comparison is exact equality with
the host cutter sf_zpaq_cut_buffer, which tests/test_zpaq.py ties to the
reference's known-answer test and to an independent restatement."""
import ctypes
import hashlib
import os
import random
import time
from pathlib import PurePath

import numpy as np
import pytest
import torch

import oracle
import syncfast_amd
from syncfast_amd import _lib, device, host
from syncfast_amd.digest import HashDigest
from syncfast_amd.index import Index, ZpaqChunker

from test_zpaq import word_salad, zpaq_inputs

pytestmark = pytest.mark.gpu

MIB = 1 << 20


def _dev(data, gpu, shift=0):
    """`data` in HBM, its first byte `shift` bytes past an aligned address."""
    t = torch.empty(len(data) + shift + 16, dtype=torch.uint8, device=gpu)
    a = np.frombuffer(data, np.uint8) if len(data) else np.zeros(0, np.uint8)
    t[shift:shift + len(data)] = torch.from_numpy(a.copy())
    return t[shift:shift + len(data)]


def _host_cut(data, bits, max_size):
    offs, sizes = host.zpaq_cut_buffer(data, bits, max_size)
    return offs.astype(np.int64), sizes.astype(np.int32)


def _check_cut(data, gpu, bits, max_size, shift=0, what=""):
    offs, sizes = device.cut_device_zpaq(_dev(data, gpu, shift), bits, max_size)
    wo, wz = _host_cut(data, bits, max_size)
    assert offs.dtype == torch.int64 and sizes.dtype == torch.int32
    assert np.array_equal(offs.cpu().numpy(), wo) and np.array_equal(sizes.cpu().numpy(), wz), what
    return device.zpaq_device_stats()


def test_kat_on_the_device(gpu, golden):
    g = golden["reference_kat"]
    t = _dev(oracle.kat_input(), gpu)
    offs, sizes = device.cut_device_zpaq(t)
    assert list(zip(offs.tolist(), sizes.tolist())) == [(b["offset"], b["size"]) for b in g["blocks"]]
    offs, sizes, dig, bh = device.index_device_zpaq(t)
    assert list(zip(offs.tolist(), sizes.tolist())) == [(0, 11579), (11579, 32768), (44347, 546)]
    assert [bytes(r).hex() for r in dig.cpu().numpy()] == [b["sha1"] for b in g["blocks"]]
    assert bh.hex() == g["blocks_hash"] == "84c25d78edcdb67631639c43604cf0149564f044"


@pytest.fixture(scope="module")
def inputs():
    return zpaq_inputs()


@pytest.mark.parametrize("bits,max_size", [(6, 256), (8, 1024)])
def test_device_cut_equals_the_host_cut_small_segments(gpu, inputs, bits, max_size):
    """150,000 bytes are hundreds of segments; the constant and periodic
    inputs join one segment per round (nseg - 1 rounds), the smallest shapes
    at which a wrong join shows."""
    L = device.zpaq_segment_len(max_size)
    nseg = -(-150_000 // L)
    for name, data in inputs.items():
        seg_len, segs, rounds, _recut = _check_cut(data, gpu, bits, max_size, what=name)
        assert (seg_len, segs) == (L, nseg) and rounds <= nseg
    assert nseg >= 64


@pytest.mark.parametrize("name,n", [("random", 8 * MIB), ("text", 8 * MIB), ("zeros", MIB), ("period13", MIB),
                                    ("ff", 150_000), ("random_then_zeros", 150_000)])
def test_device_cut_equals_the_host_cut_default_parameters(gpu, inputs, name, n):
    if name == "random":
        data = random.Random(77).randbytes(n)
    elif name == "text":
        data = word_salad(n, 3)
    elif n > len(inputs[name]):
        data = (inputs[name][:13 * 1000] * (n // 13000 + 1))[:n]  # 13000: a multiple of the period
    else:
        data = inputs[name]
    _check_cut(data, gpu, 13, 32768, what=name)


@pytest.mark.parametrize("bits,max_size", [(6, 256), (5, 48)])
def test_device_cut_edges(gpu, bits, max_size):
    L = device.zpaq_segment_len(max_size)
    assert L % max_size == 0 and L % 32 == 0 and L >= max_size
    base = random.Random(9).randbytes(3 * L + 7 + 16)
    for n in (0, 1, L - 1, L, L + 1, 3 * L + 7):
        for shift in (0, 1, 3, 13):
            _check_cut(base[shift:shift + n], gpu, bits, max_size, shift, what=(n, shift))


def test_device_cut_natural_cuts_at_segment_seams(gpu):
    """A natural cut (the hash's, a chunk shorter than max_size) that ends on
    a segment's last byte -- the next segment's incoming cut is its own first
    byte -- and one that ends on a segment's first byte.  With every earlier
    cut forced, a cut on a segment's last byte is at once natural and forced
    (L is a multiple of max_size), so the natural ones searched for here
    follow an earlier natural cut."""
    bits, max_size = 6, 256
    L = device.zpaq_segment_len(max_size)
    rng = random.Random(11)
    on_last = on_first = None
    for _ in range(20_000):
        data = rng.randbytes(4 * L)
        offs, sizes = host.zpaq_cut_buffer(data, bits, max_size)
        nat = [int(o + z) for o, z in zip(offs, sizes) if z < max_size and o + z < len(data)]
        if on_last is None and any(e % L == 0 for e in nat):
            on_last = data
        if on_first is None and any(e % L == 1 for e in nat):
            on_first = data
        if on_last is not None and on_first is not None:
            break
    assert on_last is not None and on_first is not None
    _check_cut(on_last, gpu, bits, max_size, what="cut on a segment's last byte")
    _check_cut(on_first, gpu, bits, max_size, what="cut on a segment's first byte")


def test_device_cut_capacity(gpu):
    data = zpaq_inputs()["text"]
    wo, wz = _host_cut(data, 8, 1024)
    k = wo.size
    t = _dev(data, gpu)
    L = syncfast_amd.lib()
    n = ctypes.c_uint64(0)
    offs = torch.full((k + 8,), -1, dtype=torch.int64, device=gpu)
    sizes = torch.full((k + 8,), -1, dtype=torch.int32, device=gpu)
    s = torch.cuda.current_stream(gpu).cuda_stream
    assert L.sf_cut_device_zpaq(t.data_ptr(), t.numel(), 8, 1024, offs.data_ptr(), sizes.data_ptr(), k - 1,
                                ctypes.byref(n), s) == _lib.SF_ENOSPC
    assert n.value == k  # the exact need
    torch.cuda.synchronize()
    assert int((offs != -1).sum()) == 0 and int((sizes != -1).sum()) == 0
    assert L.sf_cut_device_zpaq(t.data_ptr(), t.numel(), 8, 1024, offs.data_ptr(), sizes.data_ptr(), k,
                                ctypes.byref(n), s) == 0 and n.value == k
    torch.cuda.synchronize()
    assert np.array_equal(offs[:k].cpu().numpy(), wo) and np.array_equal(sizes[:k].cpu().numpy(), wz)
    assert int((offs[k:] != -1).sum()) == 0 and int((sizes[k:] != -1).sum()) == 0  # nothing past cap


def test_index_device_zpaq_digests_and_blocks_hash(gpu):
    data = word_salad(MIB, 4)
    offs, sizes, dig, bh = device.index_device_zpaq(_dev(data, gpu))
    wo, wz = _host_cut(data, 13, 32768)
    assert np.array_equal(offs.cpu().numpy(), wo) and np.array_equal(sizes.cpu().numpy(), wz)
    want = [hashlib.sha1(data[o:o + s]).digest() for o, s in zip(wo.tolist(), wz.tolist())]
    assert [bytes(r) for r in dig.cpu().numpy()] == want
    assert bh == host.blocks_hash(b"".join(want))
    _o, _s, _d, none = device.index_device_zpaq(_dev(data, gpu), blocks_hash=False)
    assert none is None


@pytest.fixture
def mixed_file(tmp_path):
    rng = random.Random(21)
    data = rng.randbytes(MIB) + bytes(MIB // 2) + word_salad(MIB, 5) + rng.randbytes(MIB // 2)
    assert len(data) == 3 * MIB
    p = tmp_path / "mixed"
    p.write_bytes(data)
    return p


def test_index_fd_zpaq_across_windows(gpu, mixed_file, knobs):
    knobs.set("SF_TEST_ZPAQ_WINDOW", 700_000)  # 3 MiB: five windows
    ops = host.ZpaqOps()
    with open(mixed_file, "rb") as f:
        st = host.file_stamp(f.fileno())
        want_rows, want_bh = host.index_fd_cut(f.fileno(), ops.address, 4, st)
        rows, bh = host.index_fd_zpaq(f.fileno(), stamp=st)
    assert rows.size == want_rows.size and rows.tobytes() == want_rows.tobytes()
    assert bh == want_bh
    assert int(rows["size"].sum()) == 3 * MIB
    host.release_cache()


def test_index_fd_zpaq_file_changed_under_the_call(gpu, mixed_file, knobs):
    knobs.set("SF_TEST_ZPAQ_WINDOW", 700_000)
    fired = []

    def hook(window):
        if window == 1 and not fired:
            fired.append(window)
            time.sleep(0.02)  # past the filesystem clock's tick
            with open(mixed_file, "r+b") as g:
                g.seek(1000)
                g.write(b"\x5A" * 3000)

    _lib.set_read_hook(hook)
    try:
        with open(mixed_file, "rb") as f:
            with pytest.raises(_lib.SfError) as e:
                host.index_fd_zpaq(f.fileno(), stamp=host.file_stamp(f.fileno()))
    finally:
        _lib.set_read_hook(None)
        host.release_cache()
    assert fired and e.value.code == _lib.SF_EAGAIN


def test_index_kat_with_the_device_chunker(gpu, tmp_path):
    """tests/test_zpaq.py::test_index_kat_with_no_boundaries_handed_in, cut on
    the device (Index.index_file -> sf_index_fd_zpaq)."""
    p = tmp_path / "kat"
    p.write_bytes(oracle.kat_input())
    name = PurePath("dir/name")
    rows = {}
    for dev_cut in (False, True):
        index = Index.open_in_memory(chunker=ZpaqChunker(device=dev_cut))
        index.index_file(p, name)
        index.commit()
        assert index.get_block(HashDigest(b"12345678901234567890")) is None
        assert index.get_block(HashDigest(bytes.fromhex("fb5ef7ebadd82c8085c5ff63823622bae0e263f6"))) == \
            (name, 0, 11579)
        assert index.get_block(HashDigest(bytes.fromhex("570d8b30fcfd585e4127b561f5ecd376ff4d0101"))) == \
            (name, 11579, 32768)
        assert index.get_block(HashDigest(bytes.fromhex("b9a8c2641af2cf8fd8f36a2456a3eaa95c029127"))) == \
            (name, 44347, 546)
        file1 = index.get_file(name)
        assert file1[0] == 1
        assert file1[2] == HashDigest(bytes.fromhex("84c25d78edcdb67631639c43604cf0149564f044"))
        rows[dev_cut] = index.list_file_blocks(1)
    assert rows[True] == rows[False]


def test_index_path_large_file_route_with_the_device_chunker(gpu, tmp_path):
    root = tmp_path / "tree"
    root.mkdir()
    data = word_salad(2 * MIB, 6)
    (root / "big").write_bytes(data)
    (root / "small").write_bytes(data[:50_000])
    idx = Index.open_in_memory(chunker=ZpaqChunker(device=True))
    idx.index_path(root, large_file_bytes=MIB)  # "big" takes the large-file route, "small" the batch
    idx.commit()
    for n, d in (("big", data), ("small", data[:50_000])):
        fid, _m, bh = idx.get_file(n)
        wo, wz = _host_cut(d, 13, 32768)
        got = idx.list_file_blocks(fid)
        assert [(g[1], g[2]) for g in got] == list(zip(wo.tolist(), wz.tolist()))
        want = [hashlib.sha1(d[o:o + s]).digest() for o, s in zip(wo.tolist(), wz.tolist())]
        assert [g[0].bytes for g in got] == want
        assert bh.bytes == host.blocks_hash(b"".join(want))
