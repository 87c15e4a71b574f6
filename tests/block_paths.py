"""Which staging path the SHA-1/Adler block kernels take, restated in numpy.

Test helper: no GPU, no call into the library.  The kernels choose a path per
wave of 64 blocks; a test that means to run one of them asks here first and
asserts the answer, so a case that no longer reaches its path fails instead of
quietly checking another one.

The conditions, and where they stand (syncfast_amd/csrc/sf_block_hash.hpp
unless another file is named):

explicit lists, `table_group` in sf_table.hip (kernel sha1_table_kernel<128, WEAK>)
  * group g of the list is blocks 64g .. 64g + 63 of the processing order:
    list order, or the stable sort by length class, largest first
    (`table_order` in sf_table.hip, `length_class` in sf_sort.hip; the launcher sorts from
    `table_sort_min()` = TABLE_SORT_MIN blocks unless SF_TEST_TABLE_SORT
    says 0 / 1).  The round-1 reversal of sha1_table_kernel permutes whole
    groups, not a group's contents, and is left out here;
  * a block with off > len or size > len - off is hashed as (0, 0);
  * over the wave's valid lanes: lo = min off, hi = max (off + size), the
    minimum and maximum size, max_nch = max n_chunks_wide(size);
  * lds_ok = every off % 16 == 0 and data % 16 == 0 and hi - lo < 0xF0000000;
  * list_path = !WEAK and (!lds_ok or min != max) and data % 16 == 0 and
    hi - (lo & ~15) < 0xF0000000  -> `hash_wave_list`, the 144-B slots: "slot";
  * otherwise `hash_wave<128, false, WEAK>`: with lds_ok the LDS tile, "tile",
    which stages steps = (min / 64) / 2 steps of 128 B of every block and
    leaves the lane's other chunks, max_nch - 2 * steps compressions for the
    wave's longest block, to the per-lane tail loop (`build_tail_chunk`;
    with WEAK the Adler sum's `c_done .. size / 64` loop too); without
    lds_ok every lane streams its own block: "lane".

fixed tiling, `fixed_wave` (kernel sha1_fixed_kernel<128, 1, WEAK>)
  * wave w is blocks 64w .. 64w + 63 of ceil(len / bs);
  * lds_ok = bs % 16 == 0 and data % 16 == 0 (and 64 * bs < 0xF0000000,
    which SF_MAX_BLOCK_SIZE guarantees);
  * min_size = the size of the wave's last block, max_size = bs,
    steps = (min_size / 64) / 2;
  * in `hash_wave<128, true, WEAK>` the uniform padding chunk
    (`compress_uniform`) ends a wave when pad.bytes == min_size == max_size
    (bs a multiple of 64, `pad_schedule` in sf_batch.cpp) and c_done == nfull,
    i.e. 2 * steps == bs / 64: "tile+pad"; any other lds_ok wave ends per
    lane: "tile"; without lds_ok "lane" (which then takes the padding chunk
    for a uniform bs % 64 == 0 wave on its own account; not told apart here).
"""
import numpy as np

TABLE_SORT_MIN = 65   # kTableSortMinBlocks, sf_table.hip
_SPAN_MAX = 0xF0000000


def _n_chunks(size):
    """SHA-1 compressions of a message of `size` bytes (n_chunks_wide)."""
    return (size + 8) // 64 + 1


def processing_order(sizes, sort):
    """The order in which a launch takes the blocks of a list."""
    sizes = np.asarray(sizes, dtype=np.int64)
    if not sort:
        return np.arange(sizes.size)
    from test_gpu_table_order import _class_keys  # numpy restatement of length_class
    return np.argsort(-_class_keys(sizes), kind="stable")


def table_waves(ptr_mod16, offsets, sizes, length, weak, sort):
    """[(path, steps, lane_chunks)] for each wave of 64 blocks of one launch
    of the explicit list (offsets, sizes) over `length` bytes at an address
    = ptr_mod16 mod 16, in processing order.  path is "slot", "tile" or
    "lane"; steps and lane_chunks are None unless path is "tile"."""
    offsets = np.asarray(offsets, dtype=np.int64)
    sizes = np.asarray(sizes, dtype=np.int64)
    assert offsets.shape == sizes.shape and offsets.ndim == 1
    order = processing_order(sizes, sort)  # by the claimed sizes, as the launcher sorts
    bad = (offsets > length) | (sizes > length - offsets)
    offs = np.where(bad, 0, offsets)[order]
    szs = np.where(bad, 0, sizes)[order]
    out = []
    for first in range(0, offs.size, 64):
        o, s = offs[first:first + 64], szs[first:first + 64]
        lo, hi = int(o.min()), int((o + s).max())
        mn, mx = int(s.min()), int(s.max())
        lds_ok = bool((o % 16 == 0).all()) and ptr_mod16 == 0 and hi - lo < _SPAN_MAX
        slot = (not weak) and (not lds_ok or mn != mx) and ptr_mod16 == 0 and hi - (lo & ~15) < _SPAN_MAX
        if slot:
            out.append(("slot", None, None))
        elif lds_ok:
            steps = (mn // 64) // 2
            out.append(("tile", steps, _n_chunks(mx) - 2 * steps))
        else:
            out.append(("lane", None, None))
    return out


def fixed_waves(ptr_mod16, bs, length):
    """["tile+pad" | "tile" | "lane"] for each wave of 64 blocks of the fixed
    tiling of `length` bytes into blocks of `bs` at an address = ptr_mod16
    mod 16."""
    nblocks = -(-length // bs)
    lds_ok = bs % 16 == 0 and ptr_mod16 == 0
    out = []
    for first in range(0, nblocks, 64):
        last = min(first + 63, nblocks - 1)
        min_size = min(bs, length - last * bs)
        steps = (min_size // 64) // 2
        if not lds_ok:
            out.append("lane")
        elif bs % 64 == 0 and min_size == bs and 2 * steps == bs // 64:
            out.append("tile+pad")
        else:
            out.append("tile")
    return out
