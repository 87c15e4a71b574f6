"""GPU: the join of the device ZPAQ cut (sf_cdc.hip) on content chosen to
reach each way a segment's join can go.  tests/zpaq_join.py restates the join
over the host cutter (pinned by test_zpaq_join.py); every case first asserts
there what it is meant to reach, then compares device.cut_device_zpaq with
host.zpaq_cut_buffer (offsets, sizes, dtypes) and the device's own counters
(L, nseg, rounds, recut) with the simulation.  Every comparison is exact."""
import hashlib
import random

import numpy as np
import pytest
import torch

import zpaq_join as zj
from syncfast_amd import device, host
from zpaq_join import ALIGNED, SYNCED, UNSYNCED

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SHIFTS = (0, 1, 8, 15)


def _dev(data, gpu, shift):
    """`data` in HBM, its first byte `shift` bytes past a 16-byte boundary."""
    t = torch.empty(len(data) + 32, dtype=torch.uint8, device=gpu)
    shift += -t.data_ptr() % 16
    t[shift:shift + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return t[shift:shift + len(data)]


def _check(data, gpu, bits, max_size, j, shifts=SHIFTS):
    """The device cut of `data` at each shift: the host's list, and the
    restatement's counters."""
    wo, wz = host.zpaq_cut_buffer(data, bits, max_size)
    assert (wo.astype(np.int64) + wz).tolist() == j.true_ends
    for shift in shifts:
        t = _dev(data, gpu, shift)
        assert t.data_ptr() % 16 == shift
        offs, sizes = device.cut_device_zpaq(t, bits, max_size)
        stats = device.zpaq_device_stats()
        assert offs.dtype == torch.int64 and sizes.dtype == torch.int32
        assert np.array_equal(offs.cpu().numpy(), wo.astype(np.int64)), shift
        assert np.array_equal(sizes.cpu().numpy(), wz.astype(np.int32)), shift
        assert stats == (j.L, j.nseg, j.rounds, j.recut), shift


def _count(j, what):
    return sum(c == what for c in j.classes[1:])


ISLAND_PARAMS = [(6, 256, 1), (5, 48, 1), (6, 17, 1), (7, 100, 1), (4, 33, 1), (9, 1023, 1)]


@pytest.mark.parametrize("bits,max_size,seed", ISLAND_PARAMS)
def test_islands_reach_every_kind_of_join(gpu, bits, max_size, seed):
    """Segments that sync part-way, segments that never sync, and three or
    more of those in a row (each waits a round for the one before it)."""
    L = zj.segment_len(max_size)
    assert (L // max_size > 1) == (max_size % 32 != 0)  # 17, 100, 33, 48, 1023: several forced chunks per segment
    data = zj.islands(L, seed)
    j = zj.restate(data, bits, max_size)
    assert _count(j, SYNCED) >= 3 and _count(j, UNSYNCED) >= 3
    assert zj.longest_run(j.classes, UNSYNCED) >= 3 and j.rounds >= 2
    _check(data, gpu, bits, max_size, j)


def test_dense_cuts_one_word_per_segment(gpu):
    """(1, 16): L = 32, a segment is one word of the bitmaps and half of all
    hash values cut."""
    data = zj.islands(32, 1)
    j = zj.restate(data, 1, 16)
    assert j.L == 32
    assert 2 * _count(j, ALIGNED) > j.nseg - 1
    per_word = np.bincount((np.array(j.true_ends) - 1) >> 5)
    assert per_word.max() >= 8
    _check(data, gpu, 1, 16, j)


def test_forced_cuts_only(gpu):
    data = zj.islands(4096, 1)
    j = zj.restate(data, 31, 4096)
    assert j.nseg >= 3 and j.classes[1:] == [ALIGNED] * (j.nseg - 1) and j.recut == 0 and j.rounds == 0
    assert all(e % 4096 == 0 for e in j.true_ends[:-1])
    _check(data, gpu, 31, 4096, j)


@pytest.mark.parametrize("bits,kind", [(13, "random"), (20, "zeros")])
def test_largest_max_size(gpu, bits, kind):
    """max_size = 2^20, the upper end of the device range: L = 1 MiB."""
    data = random.Random(31).randbytes(3 * MIB + 5) if kind == "random" else bytes(5 * MIB // 2)
    j = zj.restate(data, bits, MIB)
    assert j.L == MIB and j.nseg == -(-len(data) // MIB) >= 3
    _check(data, gpu, bits, MIB, j)


def test_smallest_max_size(gpu):
    """max_size = 16, the lower end: L = 32, every segment two forced chunks
    unless the hash cuts."""
    data = zj.islands(32, 1)
    j = zj.restate(data, 8, 16)
    assert j.L == 32 and _count(j, UNSYNCED) >= 3 and j.rounds >= 2
    _check(data, gpu, 8, 16, j)


@pytest.mark.parametrize("bits,max_size", [(6, 256), (6, 17)])
def test_lengths_at_the_workgroup_edges(gpu, bits, max_size):
    """Prefixes of one island input that end one byte before, on and one
    byte after a segment's end, at 1, 2 segments, around the 64 segments of a
    round-0 / join workgroup and the 256 of a count / emit workgroup."""
    L = zj.segment_len(max_size)
    whole = zj.islands(L, 2, pairs=50)
    assert len(whole) >= 257 * L + 1
    for k in (1, 2, 63, 64, 65, 255, 256, 257):
        for n in (k * L - 1, k * L, k * L + 1):
            data = whole[:n]
            j = zj.restate(data, bits, max_size)
            assert j.nseg == k + (n > k * L)
            _check(data, gpu, bits, max_size, j)


@pytest.fixture
def island_file(tmp_path):
    data = zj.islands(256, 3, pairs=30)[:40_000]
    assert len(data) == 40_000
    p = tmp_path / "islands"
    p.write_bytes(data)
    return p, data


def _check_windows(path, data, bits, max_size, knobs, window):
    knobs.set("SF_TEST_ZPAQ_WINDOW", window)
    wo, wz = host.zpaq_cut_buffer(data, bits, max_size)
    want = [hashlib.sha1(data[o:o + s]).digest() for o, s in zip(wo.tolist(), wz.tolist())]
    try:
        with open(path, "rb") as f:
            rows, bh = host.index_fd_zpaq(f.fileno(), bits, max_size, host.file_stamp(f.fileno()))
    finally:
        host.release_cache()
    assert rows["offset"].tolist() == wo.tolist() and rows["size"].tolist() == wz.tolist()
    assert [bytes(r) for r in rows["sha1"]] == want
    assert bh == host.blocks_hash(b"".join(want))
    return wz


@pytest.mark.parametrize("window", [1, 3 * 256 + 7])
def test_index_fd_zpaq_small_windows(gpu, island_file, knobs, window):
    """The knob at 1 is raised to 2 max_size = 512 bytes, the minimum window:
    each keeps its blocks but the last, so 40,000 bytes are at least 78
    windows; 3 * 256 + 7 is a window that is no multiple of anything."""
    p, data = island_file
    _check_windows(p, data, 6, 256, knobs, window)


def test_index_fd_zpaq_windows_of_two_forced_chunks(gpu, tmp_path, knobs):
    data = random.Random(41).randbytes(10_000)
    p = tmp_path / "random"
    p.write_bytes(data)
    sizes = _check_windows(p, data, 31, 256, knobs, 1)
    assert sizes.tolist() == [256] * 39 + [16]  # every window: two forced chunks, one kept
