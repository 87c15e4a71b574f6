"""GPU: sf_cut_device_zpaq_files and sf_index_device_zpaq_files write their
device outputs and nothing else -- their scenarios for
test_gpu_written_extent.py's list, in that file's manner (as
test_gpu_serve_files_extent.py does for the GET_FILE parse).

The row lists, the digests and first_row are carved from one allocation full
of a pattern (tests/placement.py), each with a few rows more than the call may
write; after the call the whole allocation is the host's bytes (the host
cutter per file, hashlib) in the rows the call must write and the pattern
everywhere else.  Capacities: room to spare, exact, and one short (nothing
written, first_row and the digests included).  One scenario per entry point
runs under a cap of 6 join launches that leaves three files unsettled:
first_row is written whole, and no row past the settled files' count.  The
scenarios are entered into that file's list through its own `scenario`
decorator when this module is imported, and run here at the same three
placements and under the same two patterns."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest
import torch

import placement
import test_gpu_written_extent as extent
import zpaq_files_join as zfj
from syncfast_amd import _lib, host

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
EXTRA = extent.EXTRA
MINE = {}
CUT, INDEX = "sf_cut_device_zpaq_files", "sf_index_device_zpaq_files"
BITS, MAX_SIZE = 6, 256


def _scenario(name, entry_point):
    def add(fn):
        MINE[name] = extent.scenario(name, entry_point)(fn)
        return fn
    return add


@functools.lru_cache(None)
def _ref(cap_rounds):
    """The table's files (tests/zpaq_files_join.py) with an empty one first
    and last, packed with gaps; the rows of the files that settle under
    `cap_rounds` join launches (0: all of them)."""
    files = [b""] + [d for _n, d, _r in zfj.table_files()] + [b""]
    j = zfj.restate_files(files, BITS, MAX_SIZE, cap_rounds)
    assert sum(j.unsettled) == (3 if cap_rounds else 0)
    spans, at = [], 0
    for k, d in enumerate(files):
        at += 1 + 3 * k
        spans.append((at, len(d)))
        at += len(d)
    buf = np.full(at + 9, 0x3C, np.uint8)
    offs, sizes, digs, hashes, first = [], [], [], [], [0]
    for (o, n), d, u in zip(spans, files, j.unsettled):
        buf[o:o + n] = np.frombuffer(d, np.uint8)
        mine = []
        if not u:
            fo, fz = host.zpaq_cut_buffer(np.frombuffer(d, np.uint8), BITS, MAX_SIZE)
            offs += (fo.astype(np.uint64) + np.uint64(o)).tolist()
            sizes += fz.tolist()
            mine = [hashlib.sha1(d[a:a + z]).digest() for a, z in zip(fo.tolist(), fz.tolist())]
        digs += mine
        hashes.append(bytes(20) if u else hashlib.sha1(b"".join(mine)).digest())
        first.append(len(offs))
    assert len(offs) > 64
    return (buf, np.array(spans, np.uint64), j, np.array(offs, np.uint64), np.array(sizes, np.uint32),
            np.frombuffer(b"".join(digs), np.uint8).reshape(-1, 20), b"".join(hashes), np.array(first, np.uint64))


def _files(index, delta, cap_rounds):
    def run(gpu, a, ph, knobs):
        buf, spans, j, offs, sizes, digs, hashes, first = _ref(cap_rounds)
        n, nf = offs.size, spans.shape[0]
        cap = n + delta
        x = extent._dev(buf, gpu)
        o = a.carve("offsets", 8 * (n + EXTRA), I64, ph(0, 8))
        z = a.carve("sizes", 4 * (n + EXTRA), I32, ph(1, 4))
        fr = a.carve("first_row", 8 * (nf + 1 + EXTRA), I64, ph(2, 8))
        d = a.carve("digests", 20 * (n + EXTRA), U8, ph(3, 4)) if index else None
        a.watch(data=x)
        fo, fl = np.ascontiguousarray(spans[:, 0]), np.ascontiguousarray(spans[:, 1])
        nb, nu, bad = extent._u64(), ctypes.c_uint32(77), ctypes.c_uint32(77)
        mask, bh = np.full(nf, 7, np.uint8), np.full(20 * nf, 7, np.uint8)
        head = (x.data_ptr(), x.numel(), fo.ctypes.data, fl.ctypes.data, nf, BITS, MAX_SIZE, cap_rounds, o.data_ptr(),
                z.data_ptr())
        tail = (mask.ctypes.data, ctypes.byref(nu), ctypes.byref(bad), extent._s(gpu))
        if index:
            rc = _lib.lib().sf_index_device_zpaq_files(*head, d.data_ptr(), cap, fr.data_ptr(), ctypes.byref(nb),
                                                       bh.ctypes.data, *tail)
        else:
            rc = _lib.lib().sf_cut_device_zpaq_files(*head, cap, fr.data_ptr(), ctypes.byref(nb), *tail)
        assert (nb.value, nu.value, mask.tolist()) == (n, sum(j.unsettled), [int(u) for u in j.unsettled])
        if delta < 0:  # nothing written: first_row and the digests included
            assert rc == _lib.SF_ENOSPC
            a.check({})
            return
        assert rc == 0
        want = {"offsets": offs, "sizes": sizes, "first_row": first}
        if index:
            assert bh.tobytes() == hashes
            want["digests"] = digs
        a.check(want)
    return run


for _index in (False, True):
    _entry = INDEX if _index else CUT
    for _delta, _tag in ((EXTRA, "cap+3"), (0, "cap=n"), (-1, "cap-1")):
        _scenario(f"{_entry[3:]}-{_tag}", _entry)(_files(_index, _delta, 0))
    _scenario(f"{_entry[3:]}-unsettled", _entry)(_files(_index, 0, 6))


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", placement.PATTERNS, ids=lambda p: f"{p:#04x}")
@pytest.mark.parametrize("place", range(3))
@pytest.mark.parametrize("name", list(MINE))
def test_outputs_and_nothing_else(gpu, knobs, name, place, pattern):
    arena = placement.Arena(gpu, pattern)
    MINE[name](gpu, arena, lambda j, align: placement.phase(place, j, align), knobs)


def test_the_scenarios_are_in_the_written_extent_list():
    covered = {e for entries, _fn in extent.SCENARIOS.values() for e in entries}
    assert {CUT, INDEX} <= covered and set(MINE) <= set(extent.SCENARIOS) and len(MINE) == 8
    with open(extent.os.path.join(extent.ROOT, "include", "syncfast_amd.h")) as f:
        found = extent.device_output_functions(f.read())
    assert found[CUT] == ["d_offsets", "d_sizes", "d_first_row"]
    assert found[INDEX] == ["d_offsets", "d_sizes", "d_digests", "d_first_row"]
