"""CPU: block_paths.py, the block kernels' path dispatch restated in numpy.

Pins the classifier on hand-written waves, one per outcome, whose paths follow
from the conditions in its docstring by hand; then runs it over the draws of
the weak explicit-list tests that were written before test_gpu_block_paths.py
and asserts that none of them holds a wave on the LDS-tile path: that is why
that file exists."""
import numpy as np
import pytest

from block_paths import TABLE_SORT_MIN, fixed_waves, processing_order, table_waves

ALIGNED = np.arange(64, dtype=np.int64) * 4112  # 64 starts, 16-B aligned, 4112 B apart
N = 64 * 4112


def both(ptr_mod16, offs, sizes, length, sort=False):
    return tuple(table_waves(ptr_mod16, offs, sizes, length, weak, sort) for weak in (True, False))


def test_equal_aligned_wave_is_a_tile_in_both_builds():
    # 256 B = 4 data chunks = 2 steps; n_chunks(256) = 5, so one compression
    # (the padding) is left to the lane
    weak, plain = both(0, ALIGNED, np.full(64, 256), N)
    assert weak == plain == [("tile", 2, 1)]


def test_aligned_wave_of_mixed_sizes_is_a_slot_wave_unless_weak():
    sizes = np.full(64, 4096)
    sizes[7] = 300  # 4 whole chunks -> 2 steps; the longest block has 65 compressions
    weak, plain = both(0, ALIGNED, sizes, N)
    assert weak == [("tile", 2, 61)]
    assert plain == [("slot", None, None)]


def test_one_unaligned_offset():
    offs = ALIGNED.copy()
    offs[63] += 4
    weak, plain = both(0, offs, np.full(64, 256), N)
    assert weak == [("lane", None, None)]
    assert plain == [("slot", None, None)]  # equal sizes, but not lds_ok


def test_out_of_range_block_counts_as_empty_at_zero():
    offs = ALIGNED.copy() + 4112
    sizes = np.full(64, 256)
    offs[5] = N + 4112 + 1  # off > len
    sizes[9] = N            # size > len - off
    weak, plain = both(0, offs, sizes, N + 4112)
    assert weak == [("tile", 0, 5)]          # min size 0: nothing staged
    assert plain == [("slot", None, None)]   # min != max
    # and its offset 0 is aligned whatever the block claimed
    offs[5] = N + 4112 + 3
    assert table_waves(0, offs, sizes, N + 4112, True, False) == [("tile", 0, 5)]


def test_partial_last_wave_counts_its_own_lanes_only():
    offs = np.arange(70, dtype=np.int64) * 4112
    sizes = np.concatenate([np.full(64, 256), np.full(6, 128)])
    weak, plain = both(0, offs, sizes, 70 * 4112)
    assert weak == plain == [("tile", 2, 1), ("tile", 1, 1)]
    sizes[69] = 100  # the 6-lane wave: min 100, max 128 (3 compressions)
    weak, plain = both(0, offs, sizes, 70 * 4112)
    assert weak == [("tile", 2, 1), ("tile", 0, 3)]
    assert plain == [("tile", 2, 1), ("slot", None, None)]


@pytest.mark.parametrize("sizes", [np.full(64, 256), np.arange(64) * 10])
def test_shifted_pointer_is_per_lane_everywhere(sizes):
    weak, plain = both(4, ALIGNED, sizes, N)
    assert weak == plain == [("lane", None, None)]


def test_span_limit():
    # two blocks 0xF0000000 apart: neither the tile nor the slots reach that far
    offs = np.array([0, 0xF0000000], np.int64)
    weak, plain = both(0, offs, np.array([256, 256]), 0xF0000100)
    assert weak == plain == [("lane", None, None)]
    # the slots start at lo & ~15: hi - lo is under the limit in both, hi - (lo & ~15) in the first only
    offs = np.array([8, 0xF0000000 - 256], np.int64)
    assert table_waves(0, offs, np.array([100, 255]), 0xF0000100, False, False) == [("slot", None, None)]
    assert table_waves(0, offs, np.array([100, 256]), 0xF0000100, False, False) == [("lane", None, None)]


def test_sorted_order_is_by_class_largest_first_and_stable():
    sizes = np.tile([64, 4096], 64)  # list order: every wave mixed
    offs = np.arange(128, dtype=np.int64) * 4112
    assert processing_order(sizes, False).tolist() == list(range(128))
    assert processing_order(sizes, True).tolist() == list(range(1, 128, 2)) + list(range(0, 128, 2))
    weak, plain = both(0, offs, sizes, 128 * 4112)
    assert weak == [("tile", 0, 65)] * 2 and plain == [("slot", None, None)] * 2
    weak, plain = both(0, offs, sizes, 128 * 4112, sort=True)
    assert weak == plain == [("tile", 32, 1), ("tile", 0, 2)]
    assert TABLE_SORT_MIN == 65


def test_fixed_waves():
    assert fixed_waves(0, 128, 70 * 128) == ["tile+pad", "tile+pad"]  # 2 chunks = 1 step
    assert fixed_waves(0, 128, 70 * 128 + 1) == ["tile+pad", "tile"]   # a 1-B last block
    assert fixed_waves(0, 128, 64 * 128 + 127) == ["tile+pad", "tile"]
    assert fixed_waves(0, 128, 63 * 128 + 64) == ["tile"]
    assert fixed_waves(0, 128, 63 * 128) == ["tile+pad"]               # 63 lanes, all whole
    for bs in (64, 192, 320, 4032, 4160):  # an odd number of chunks: the steps stop one short
        assert fixed_waves(0, bs, 70 * bs) == ["tile", "tile"], bs
    assert fixed_waves(0, 4096, 70 * 4096) == ["tile+pad", "tile+pad"]
    assert fixed_waves(0, 4112, 70 * 4112) == ["tile", "tile"]         # aligned, no 64-B multiple
    assert fixed_waves(0, 100, 70 * 100) == ["lane", "lane"]           # bs % 16
    assert fixed_waves(4, 128, 70 * 128) == ["lane", "lane"]
    assert fixed_waves(0, 128, 0) == []


# ------------------------------------------------ the older weak list tests
def _older_weak_lists():
    """(test, ptr_mod16, offsets, sizes, length) of every explicit list that
    the weak tests written before test_gpu_block_paths.py hash, drawn as they
    draw them."""
    from test_gpu_binding import _lists
    from test_gpu_table_order import _cdc_like

    # test_gpu_weak.py::test_blocks_weak_ragged_and_range
    rng = np.random.default_rng(21)
    n = 600_000
    sizes = rng.integers(0, 70_000, 300)
    offs = np.array([int(rng.integers(0, n - s)) for s in sizes], np.int64)
    offs[::4] = offs[::4] // 16 * 16
    yield "test_blocks_weak_ragged_and_range", 0, offs, sizes, n

    # test_gpu_table_order.py::test_sorted_weak_blocks
    for case in range(6):
        rng = np.random.default_rng(34_000 + case)
        n = int(rng.integers(1, 6 << 20))
        offs, sizes = _cdc_like(rng, n, mean=4096)
        yield f"test_sorted_weak_blocks[{case}]", int(rng.integers(0, 16)), offs, sizes, n

    # test_gpu_table_order.py::test_sorted_round_reversal_weak
    rng = np.random.default_rng(39_000)
    sizes = rng.integers(0, 600, 64 * 2048 + 77).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    yield "test_sorted_round_reversal_weak", 0, offs, sizes, int(sizes.sum())

    # test_gpu_binding.py::test_list_forms
    data, offs, sizes = _lists()[0]
    yield "test_list_forms", 0, offs, sizes, data.size


def test_no_older_weak_list_reaches_the_tile_path():
    seen = 0
    for name, mod16, offs, sizes, n in _older_weak_lists():
        for sort in (False, True):
            # at the pointer the test uses, and at an aligned one (the most a
            # pointer can do for the tile path)
            for m in {mod16, 0}:
                waves = table_waves(m, offs, sizes, n, True, sort)
                assert all(w[0] == "lane" for w in waves), (name, sort, m)
                seen += len(waves)
    assert seen > 4000


# ------------------------------------------- the lists of the new GPU tests
def test_new_gpu_lists_classify_as_their_tests_say():
    # the same assertions test_gpu_block_paths.py makes before it calls the
    # library, where no GPU is needed to make them
    import test_gpu_block_paths as g
    for S in (0, 16, 48, 64, 128, 192, 256, 320, 4096, 4160):
        offs, sizes, n = g.equal_list(S)
        for sort in (False, True):
            weak, plain = both(0, offs, sizes, n, sort)
            assert weak == plain and [w[:2] for w in weak] == [("tile", (S // 64) // 2)] * 3
    for build in (g.mixed_long_list, g.mixed_with_empty_list, g.out_of_range_list, g.worst_case_list):
        offs, sizes, n = build()
        assert n < (1 << 20) and offs.size == 200 and (offs[offs + sizes <= n] % 16 == 0).all()
        for sort in (False, True):
            weak, plain = both(0, offs, sizes, n, sort)
            assert [w[0] for w in weak] == ["tile"] * 4 and [w[0] for w in plain] == ["slot"] * 4
            for m in (4, 1):
                assert both(m, offs, sizes, n, sort) == ([("lane", None, None)] * 4,) * 2
    offs, sizes, n = g.mixed_long_list()
    assert any(st >= 1 and lc > 2 for _, st, lc in table_waves(0, offs, sizes, n, True, False)[:3])
    offs, sizes, n = g.mixed_with_empty_list()
    assert table_waves(0, offs, sizes, n, True, True) == g.MIXED_EMPTY_SORTED_WEAK
