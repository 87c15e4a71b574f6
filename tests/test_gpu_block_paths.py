"""GPU: every staging path of the block kernels, reached on purpose.

The SHA-1/Adler block kernels choose a staging path per wave (block_paths.py
restates the choice).  Each case here builds its input, asserts the path the
classifier gives it BEFORE it calls the library, so a case that stops
reaching its path fails, and then compares every digest with
oracle.index_blocks / index_fixed, every weak sum with oracle.adler_blocks /
adler_fixed, and the weak build's digests with the plain build's.  All
comparisons are exact.

What the other files leave out and these cases run:
  * the LDS-tile path of the weak explicit-list kernel
    (hash_wave<128, false, true> with lds_ok): LDS steps, then each lane's
    SHA-1 through build_tail_chunk over many whole chunks and its Adler-32
    through the c_done .. size / 64 loop (mixed_long, mixed_with_empty,
    out_of_range, pieces, worst_case_bytes);
  * the tile path of the plain list kernel, now reached only by equal-size
    aligned waves (equal);
  * a weak list over several launches (pieces);
  * fixed block sizes that are odd multiples of 64 above 64, where the
    uniform padding chunk must not be taken (192, 320, 4032, 4160).
"""
import functools
import zlib

import numpy as np
import pytest
import torch

import oracle
from block_paths import fixed_waves, table_waves
from syncfast_amd import SfError, device

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ inputs
# numpy only, so the CPU suite (test_block_paths.py) can classify them too

def aligned_layout(rng, sizes):
    """16-B aligned offsets for `sizes`, blocks apart from each other (16 to
    64 B between neighbours) and laid out in memory in a shuffled order ->
    (offsets, bytes needed)."""
    m = sizes.size
    stride = (sizes + 15) // 16 * 16 + 16 * rng.integers(1, 5, m)
    mem = rng.permutation(m)  # mem[k] = the block at the k-th place in memory
    offs = np.zeros(m, np.int64)
    offs[mem] = np.concatenate([[0], np.cumsum(stride[mem])[:-1]])
    return offs, int(stride.sum())


def equal_list(S):
    """130 blocks of S bytes (two full waves and a 2-lane wave), two of them
    at the same offset."""
    rng = np.random.default_rng(500 + S)
    sizes = np.full(130, S, np.int64)
    offs, n = aligned_layout(rng, sizes)
    offs[77] = offs[5]
    return offs, sizes, n


MIXED_LONG_FORCED = (183, 184, 191, 192, 247, 248)  # size % 64 in 55, 56, 63, 0


def mixed_long_list():
    rng = np.random.default_rng(2)
    sizes = rng.integers(128, 3000, 200).astype(np.int64)
    sizes[[3, 40, 70, 100, 130, 195]] = MIXED_LONG_FORCED
    offs, n = aligned_layout(rng, sizes)
    return offs, sizes, n


MIXED_EMPTY_FORCED = (0, 55, 56, 63, 64, 119, 120)


def mixed_with_empty_list():
    rng = np.random.default_rng(1)
    sizes = rng.integers(0, 3000, 200).astype(np.int64)
    sizes[[2, 9, 17, 25, 33, 41, 49]] = MIXED_EMPTY_FORCED  # all in the first wave of the list
    offs, n = aligned_layout(rng, sizes)
    return offs, sizes, n


OUT_OF_RANGE_ROWS = (10, 80, 150, 199)  # one per wave of the list


def out_of_range_list():
    offs, sizes, n = mixed_long_list()
    offs = offs.copy()
    offs[list(OUT_OF_RANGE_ROWS)] = n - sizes[list(OUT_OF_RANGE_ROWS)] + 16  # ends 16 B past the end
    return offs, sizes, n


def worst_case_list():
    """mixed_long's layout with sizes 64 k + 63: after the reduced chunks the
    fused sum takes 63 single bytes (Adler::byte)."""
    rng = np.random.default_rng(3)
    sizes = (64 * rng.integers(2, 46, 200) + 63).astype(np.int64)
    offs, n = aligned_layout(rng, sizes)
    return offs, sizes, n


# --------------------------------------------------------------- references
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _table_case(name, arg=None):
    """(data, offsets, sizes, digests, sums) of a list, computed once; rows of
    blocks outside the data are zero, as the library leaves them."""
    build = {"equal": equal_list, "mixed_long": mixed_long_list, "mixed_with_empty": mixed_with_empty_list,
             "out_of_range": out_of_range_list, "worst_case_bytes": worst_case_list}[name]
    offs, sizes, n = build() if arg is None else build(arg)
    assert n < (1 << 20) and offs.size <= 300
    data = np.full(n, 255, np.uint8) if name == "worst_case_bytes" else oracle.splitmix_bytes(n, 7000 + len(name) + (arg or 0))
    good = offs + sizes <= n
    dig = np.zeros((offs.size, 20), np.uint8)
    sums = np.zeros(offs.size, np.uint32)
    dig[good] = oracle.index_blocks(data, offs[good], sizes[good]).reshape(-1, 20)
    sums[good] = oracle.adler_blocks(data, offs[good], sizes[good])
    return _frozen(data, offs, sizes, dig, sums)


def _place(data, gpu, mod16):
    """`data` on the device at an address = mod16 (mod 16)."""
    t = torch.empty(data.size + 32, dtype=torch.uint8, device=gpu)
    shift = (mod16 - t.data_ptr()) % 16
    v = t[shift:shift + data.size]
    v.copy_(torch.from_numpy(np.array(data)).to(gpu))
    assert v.data_ptr() % 16 == mod16
    return v


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _check_table(gpu, case, mod16=0, check_range=True):
    """Run both builds over the placed list and compare every row."""
    data, offs, sizes, dig, sums = case
    t = _place(data, gpu, mod16)
    to, tz = torch.from_numpy(np.array(offs)).to(gpu), torch.from_numpy(sizes.astype(np.int32)).to(gpu)
    dw, w = device.index_device_blocks_weak(t, to, tz, check_range=check_range)
    dp = device.index_device_blocks(t, to, tz, check_range=check_range)
    assert np.array_equal(dw.cpu().numpy(), dig)
    assert np.array_equal(_u32(w), sums)
    assert torch.equal(dw, dp)
    return t, to, tz


def _paths(waves):
    return [w[0] for w in waves]


# -------------------------------------------------------------- table cases
SORTS = pytest.mark.parametrize("sort", [0, 1], ids=["list_order", "sorted"])


@SORTS
@pytest.mark.parametrize("S", [0, 16, 48, 64, 128, 192, 256, 320, 4096, 4160])
def test_equal(gpu, knobs, S, sort):
    # equal sizes at aligned offsets: the LDS tile in both builds (the only
    # waves of the plain build that still take it), 2 and 64 valid lanes
    knobs.set("SF_TEST_TABLE_SORT", sort)
    case = _table_case("equal", S)
    data, offs, sizes = case[:3]
    assert offs[77] == offs[5] and (offs % 16 == 0).all() and not (np.diff(offs) > 0).all()
    for weak in (True, False):
        waves = table_waves(0, offs, sizes, data.size, weak, bool(sort))
        assert waves == [("tile", (S // 64) // 2, (S + 8) // 64 + 1 - 2 * ((S // 64) // 2))] * 3, (weak, waves)
    _check_table(gpu, case)


@SORTS
def test_mixed_long(gpu, knobs, sort):
    knobs.set("SF_TEST_TABLE_SORT", sort)
    case = _table_case("mixed_long")
    data, offs, sizes = case[:3]
    assert set(MIXED_LONG_FORCED) <= set(sizes.tolist()) and sizes.min() >= 128
    weak = table_waves(0, offs, sizes, data.size, True, bool(sort))
    assert _paths(weak) == ["tile"] * 4
    if not sort:
        assert any(st >= 1 and lc > 2 for _, st, lc in weak[:3]), weak
    assert _paths(table_waves(0, offs, sizes, data.size, False, bool(sort))) == ["slot"] * 4
    _check_table(gpu, case)


# mixed_with_empty_list() under the weak build's sorted launch (block_paths.table_waves)
MIXED_EMPTY_SORTED_WEAK = [("tile", 16, 15), ("tile", 8, 19), ("tile", 0, 18), ("tile", 0, 2)]


@SORTS
def test_mixed_with_empty(gpu, knobs, sort):
    knobs.set("SF_TEST_TABLE_SORT", sort)
    case = _table_case("mixed_with_empty")
    data, offs, sizes = case[:3]
    assert set(MIXED_EMPTY_FORCED) <= set(sizes[:64].tolist())
    weak = table_waves(0, offs, sizes, data.size, True, bool(sort))
    assert _paths(weak) == ["tile"] * 4
    if sort:
        # the longest blocks first: LDS steps and a long per-lane tail in one wave
        assert weak == MIXED_EMPTY_SORTED_WEAK
    else:
        assert weak[0][1] == 0  # an empty block in the wave: nothing staged, all per lane
    assert _paths(table_waves(0, offs, sizes, data.size, False, bool(sort))) == ["slot"] * 4
    _check_table(gpu, case)


@SORTS
def test_out_of_range(gpu, knobs, sort):
    # a block outside the data is hashed as (0, 0): the wave keeps its path,
    # stages nothing (min size 0) and leaves zero rows at the block's index
    knobs.set("SF_TEST_TABLE_SORT", sort)
    case = _table_case("out_of_range")
    data, offs, sizes, dig, sums = case
    bad = list(OUT_OF_RANGE_ROWS)
    assert (offs[bad] + sizes[bad] > data.size).all() and not dig[bad].any() and not sums[bad].any()
    assert dig[np.setdiff1d(np.arange(200), bad)].any(axis=1).all()
    assert _paths(table_waves(0, offs, sizes, data.size, True, bool(sort))) == ["tile"] * 4
    assert _paths(table_waves(0, offs, sizes, data.size, False, bool(sort))) == ["slot"] * 4
    t, to, tz = _check_table(gpu, case, check_range=False)
    with pytest.raises(SfError):
        device.index_device_blocks_weak(t, to, tz)
    with pytest.raises(SfError):
        device.index_device_blocks(t, to, tz)


@SORTS
def test_pieces(gpu, knobs, sort):
    # a weak list over five launches: every sum and digest at its block's own
    # index (launch_table's `weak + first`), each piece a tile wave
    knobs.set("SF_TEST_TABLE_SORT", sort)
    knobs.set("SF_TEST_LAUNCH_MAX_BLOCKS", 48)
    case = _table_case("mixed_long")
    data, offs, sizes = case[:3]
    for first in range(0, 200, 48):
        piece = table_waves(0, offs[first:first + 48], sizes[first:first + 48], data.size, True, bool(sort))
        assert _paths(piece) == ["tile"] and piece[0][1] >= 1, (first, piece)
    _check_table(gpu, case)


@SORTS
def test_worst_case_bytes(gpu, knobs, sort):
    # all-0xFF blocks of 64 k + 63 bytes: the largest partial sums through the
    # per-lane chunk loop and then 63 single bytes
    knobs.set("SF_TEST_TABLE_SORT", sort)
    case = _table_case("worst_case_bytes")
    data, offs, sizes, _, sums = case
    assert (sizes % 64 == 63).all() and (data == 255).all()
    assert sums[:64].tolist() == [zlib.adler32(b"\xff" * int(s)) for s in sizes[:64]]
    weak = table_waves(0, offs, sizes, data.size, True, bool(sort))
    assert _paths(weak) == ["tile"] * 4 and all(st >= 1 for _, st, _ in weak)
    _check_table(gpu, case)


@SORTS
@pytest.mark.parametrize("mod16", [4, 1])
def test_unaligned_pointer(gpu, knobs, mod16, sort):
    # the same aligned offsets under a shifted pointer: every lane on its own
    knobs.set("SF_TEST_TABLE_SORT", sort)
    case = _table_case("mixed_long")
    data, offs, sizes = case[:3]
    for weak in (True, False):
        assert _paths(table_waves(mod16, offs, sizes, data.size, weak, bool(sort))) == ["lane"] * 4
    _check_table(gpu, case, mod16=mod16)


# -------------------------------------------------------------- fixed cases
# How a full wave of each block size ends.  4032 = 63 * 64 is an odd multiple
# of 64 like 192, 320 and 4160: the LDS steps stop one chunk short of the
# block (c_done != nfull), so the uniform padding chunk must not be taken.
FIXED_FULL_WAVE = {128: "tile+pad", 192: "tile", 320: "tile", 4032: "tile", 4096: "tile+pad", 4160: "tile"}
FIXED_TAILS = (0, 1, 55, 56, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def _fixed_case(bs):
    """The longest input of block size bs and the references of each length
    70 bs + d: {d: (digests, sums)}."""
    data = oracle.splitmix_bytes(70 * bs + max(FIXED_TAILS), 8000 + bs)
    refs = {}
    for d in FIXED_TAILS:
        part = data[:70 * bs + d]
        refs[d] = _frozen(oracle.index_fixed(part, bs)[2].reshape(-1, 20), oracle.adler_fixed(part, bs))
    return _frozen(data)[0], refs


@pytest.mark.parametrize("mod16", [0, 4, 1])
@pytest.mark.parametrize("bs", sorted(FIXED_FULL_WAVE))
def test_fixed(gpu, bs, mod16):
    data, refs = _fixed_case(bs)
    t = _place(data, gpu, mod16)
    for d in FIXED_TAILS:
        n = 70 * bs + d
        full = FIXED_FULL_WAVE[bs] if mod16 == 0 else "lane"
        ragged = "tile" if mod16 == 0 else "lane"  # a last wave ending in a short block
        assert fixed_waves(mod16, bs, n) == [full, full if d == 0 else ragged], (bs, d)
        dig, sums = refs[d]
        part = t[:n]
        assert part.data_ptr() % 16 == mod16
        dw, w = device.index_device_weak(part, bs)
        dp = device.index_device(part, bs)
        assert np.array_equal(dp.cpu().numpy(), dig), (bs, d)
        assert np.array_equal(dw.cpu().numpy(), dig), (bs, d)
        assert np.array_equal(_u32(w), sums), (bs, d)


def test_fixed_batch_odd_chunks(gpu):
    # the same kernel under the many-file entry point: 70 equal, contiguous
    # files of 8 blocks of 192 B, every digest and every blocks_hash
    nfiles, nbf, bs = 70, 8, 192
    data = oracle.splitmix_bytes(nfiles * nbf * bs, 8192)
    assert fixed_waves(0, bs, data.size) == ["tile"] * 9
    want = oracle.index_fixed(data, bs)[2].reshape(-1, 20)
    files = [(i * nbf * bs, nbf * bs) for i in range(nfiles)]
    dig, first, fh = device.index_device_batch(_place(data, gpu, 0), files, bs)
    assert list(first) == [i * nbf for i in range(nfiles + 1)]
    assert np.array_equal(dig.cpu().numpy(), want)
    fhn = fh.cpu().numpy()
    for i in range(nfiles):
        assert bytes(fhn[i]) == oracle.blocks_hash(want[nbf * i:nbf * (i + 1)]), i
