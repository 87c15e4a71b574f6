"""tests/zpaq_join.py (the restatement of the device cut's join that
test_gpu_zpaq_join.py asserts against) on inputs whose answer is worked out by
hand from two lists: the true cuts and every segment's cuts from its first
byte.  Both lists are asserted here against `zpaq_cuts`, the Python chunker
of test_zpaq.py, so nothing in these cases rests on the code they pin.  No
GPU."""
import random

import pytest

import zpaq_join as zj
from test_zpaq import zpaq_cuts
from zpaq_join import ALIGNED, SYNCED, UNSYNCED


def py_ends(data, bits, max_size):
    return [o + s for o, s in zpaq_cuts(bytes(data), bits, max_size)]


def _lists(data, bits, max_size, L):
    """(true ends, [segment s cut from s0 on its own, ends in (s0, s1]])"""
    n = len(data)
    spec = []
    for s0 in range(0, n, L):
        s1 = min(n, s0 + L)
        spec.append([s0 + e for e in py_ends(data[s0:s1 + 1], bits, max_size) if s0 + e <= s1])
    return py_ends(data, bits, max_size), spec


def test_segment_len():
    assert [zj.segment_len(m) for m in (16, 17, 33, 48, 100, 256, 1023, 4096, 1 << 20)] == \
        [32, 544, 1056, 96, 800, 256, 32736, 4096, 1 << 20]


def test_hand_checked_sync_then_walk_then_sync():
    """(4, 16): L = 32, 150 bytes, five segments.
    round 0   last = [32, 61, 91, 128, 150], used = [0, 32, 64, 96, 128]
    round 1   s1: 32 == used.  s2: from 61, a true cut, so the true list
              follows: 75, then 91 which is speculative: stops there, 30
              bytes, last[2] = 91 (the speculative list's last).  s3 reads
              the OLD last[2] = 91 != 96: from 91, true again: 107, 123, none
              speculative: walks to 128, 37 bytes, last[3] = 123.  s4: the old
              last[3] = 128 == used.
    round 2   s3: 91 == used.  s4: from 123: 137, then 150 = len, which counts
              in both lists: 27 bytes.
    round 3   nothing changes: 2 rounds, 30 + 37 + 27 = 94 bytes."""
    data = random.Random(39).randbytes(150)
    true, spec = _lists(data, 4, 16, 32)
    assert true == [16, 32, 48, 61, 75, 91, 107, 123, 137, 150]
    assert spec == [[16, 32], [48, 61], [80, 91], [112, 128], [133, 138, 150]]
    j = zj.restate(data, 4, 16)
    assert (j.L, j.nseg, j.true_ends, j.spec) == (32, 5, true, spec)
    assert j.classes == [None, ALIGNED, SYNCED, UNSYNCED, SYNCED]
    assert (j.rounds, j.recut) == (2, 94)
    assert zj.longest_run(j.classes, UNSYNCED) == 1 and zj.longest_run(j.classes, SYNCED) == 1


def test_hand_checked_sync_on_the_second_cut():
    """(4, 16), 150 bytes.  last = [32, 61, 93, 128, 150] after round 0.
    round 1   s2 from 61 (true): 66, then 71 which is speculative: 10 bytes,
              last[2] = 93.  s3 from the old last[2] = 93 (true): 104, 119,
              122, none speculative: 128 - 93 = 35 bytes, last[3] = 122.
    round 2   s4 from 122: 134, 146, 150 = len: 28 bytes.  73 in all."""
    data = random.Random(22).randbytes(150)
    true, spec = _lists(data, 4, 16, 32)
    assert true == [16, 32, 36, 52, 61, 66, 71, 74, 86, 93, 104, 119, 122, 134, 146, 150]
    assert spec == [[16, 32], [36, 52, 61], [71, 74, 86, 93], [112, 128], [144, 150]]
    j = zj.restate(data, 4, 16)
    assert j.classes == [None, ALIGNED, SYNCED, UNSYNCED, SYNCED]
    assert (j.rounds, j.recut) == (2, 73)


def test_forced_cuts_only_are_aligned():
    # bits = 31: the hash never cuts 2^-31 of the time; every cut is at a multiple of max_size
    data = random.Random(1).randbytes(5 * 96 + 7)
    j = zj.restate(data, 31, 48)
    assert (j.L, j.nseg) == (96, 6) and j.true_ends == list(range(48, 487, 48)) + [487]
    assert j.classes == [None] + [ALIGNED] * 5 and (j.rounds, j.recut) == (0, 0)


def test_one_segment_and_empty():
    j = zj.restate(b"x" * 32, 4, 16)
    assert (j.nseg, j.classes, j.rounds, j.recut) == (1, [None], 0, 0)
    j = zj.restate(b"", 4, 16)
    assert (j.nseg, j.classes, j.rounds, j.recut, j.true_ends) == (0, [None], 0, 0, [])


def test_hand_checked_zeros():
    """(6, 256) cuts zeros every 83 bytes, from wherever it starts; L = 256.
    Three segments, 768 bytes: true cuts 83 k and 768; segment 1 alone cuts
    339, 422, 505, segment 2 alone 595, 678, 761 and 768 = len.
    round 1   s1 from 249: 332, 415, 498, none speculative: to 512, 263
              bytes, last[1] = 498.  s2 from the old last[1] = 505: 588, 671,
              754, then len: 263 bytes.
    round 2   s2 from 498: 581, 664, 747, len: 270 bytes.  796 in all."""
    data = bytes(768)
    true, spec = _lists(data, 6, 256, 256)
    assert true == list(range(83, 768, 83)) + [768]
    assert spec == [[83, 166, 249], [339, 422, 505], [595, 678, 761, 768]]
    j = zj.restate(data, 6, 256)
    assert j.classes == [None, UNSYNCED, SYNCED] and (j.rounds, j.recut) == (2, 796)


def test_constant_bytes_join_one_segment_per_round():
    """sf_cdc.hip's header: on constant data speculative and true cuts never
    coincide (256 s is a multiple of 83 only from segment 83 on), so the join
    advances one segment per round; only the last segment syncs, at len."""
    j = zj.restate(bytes(40 * 256), 6, 256)
    assert j.classes == [None] + [UNSYNCED] * 38 + [SYNCED]
    assert j.rounds == j.nseg - 1 == 39 and zj.longest_run(j.classes, UNSYNCED) == 38


@pytest.mark.parametrize("bits,max_size", [(4, 16), (5, 48), (6, 17), (4, 33)])
def test_the_c_cutter_and_the_python_chunker_give_the_same_join(bits, max_size):
    L = zj.segment_len(max_size)
    for seed in range(3):
        data = zj.islands(L, seed, pairs=2)
        assert zj.restate(data, bits, max_size) == zj.restate(data, bits, max_size, ends=py_ends)


def test_islands_recipe():
    L = 96
    a, b = zj.islands(L, 7), zj.islands(L, 7)
    assert a == b and a != zj.islands(L, 8)
    assert 6 * (L // 2 + L) <= len(a) <= 6 * (4 * L + 6 * L)
    # walk the recipe with the same generator: lengths in range, the pattern periodic
    rng = random.Random(7)
    pos = 0
    for _ in range(6):
        n = rng.randint(L // 2, 4 * L)
        assert a[pos:pos + n] == rng.randbytes(n)
        pos += n
        period = rng.choice(zj.PERIODS)
        pattern = rng.randbytes(period)
        n = rng.randint(L, 6 * L)
        assert L <= n <= 6 * L and all(a[pos + k] == pattern[k % period] for k in range(n))
        pos += n
    assert pos == len(a)
