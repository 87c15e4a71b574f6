"""GPU: sf_receive_files_device writes its nine device outputs and nothing
else -- its scenarios for test_gpu_written_extent.py's list, in that file's
manner (as test_gpu_want_extent.py does for sf_place_block_data_device).

The five block lists and the four section lists are carved from one
allocation full of a pattern (tests/placement.py), each with a few rows more
than the call may write; after the call the whole allocation is the model's
bytes (files_expect: wire.Parser and the sink's rule) in the rows the call
must write and the pattern everywhere else.  Three routes -- the chain on the
device, SF_TEST_WIRE_PARSE_HOST, and the fallback after a start forged by an
honest name -- at five capacities: room to spare, exact, blocks one short,
files one short, and the NULL-output query; with and without a set.  The
scenarios are entered into that file's list through its own `scenario`
decorator when this module is imported, and run here at the same three
placements and under the same two patterns."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
import placement
import test_gpu_written_extent as extent
from files_expect import FILE_END, OTHER, block, expected, needs_fallback, start
from syncfast_amd import _lib, device, wire

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
EXTRA = extent.EXTRA
BASE = (1 << 40) + 5
MINE = {}
ENTRY = "sf_receive_files_device"
# name, dtype, bytes per row, alignment, a section list
OUTPUTS = (("digests", U8, 20, 4, False), ("sizes", I32, 4, 4, False), ("offsets", I64, 8, 8, False),
           ("rows", I64, 8, 8, False), ("block_file", I32, 4, 4, False), ("name_at", I64, 8, 8, True),
           ("name_len", I32, 4, 4, True), ("first", I64, 8, 8, True), ("file_size", I64, 8, 8, True))


def _scenario(name):
    def add(fn):
        MINE[name] = extent.scenario(name, ENTRY)(fn)
        return fn
    return add


@functools.lru_cache(None)
def _ref(forged: bool):
    """A buffer that begins inside a file (a section carried in), then four
    files, one of them empty, and stops at another command."""
    rng = np.random.default_rng(17)
    pool = rng.integers(0, 256, (12, 20), dtype=np.uint8)
    table, present = pool[rng.integers(0, 8, 30)], rng.random(30) < 0.6  # digests 8..11 are in no row
    pick = lambda: block(pool[int(rng.integers(0, 12))].tobytes(), int(rng.integers(0, 1 << 20)))  # noqa: E731
    data = pick() + pick() + FILE_END
    for f, n in enumerate((5, 0, 9, 3)):
        data += start(b"x/FILE_END" if forged and f == 2 else b"dir/file%d" % f) + b"".join(pick() for _ in range(n))
        data += FILE_END
    data += b"COMPLETE\n"
    assert needs_fallback(data, True) == forged
    e = expected(data, True, BASE)
    assert (len(e.sizes), len(e.name_at), e.stop, e.open) == (19, 5, OTHER, False)
    digests = np.frombuffer(b"".join(e.digests), np.uint8).reshape(-1, 20)
    rows = oracle.block_lookup(table, present, digests)
    assert (rows >= 0).any() and (rows < 0).any()
    want = {"digests": digests, "sizes": np.array(e.sizes, np.uint32), "offsets": np.array(e.offsets, np.uint64),
            "rows": rows.astype(np.int64), "block_file": np.array(e.block_file, np.uint32),
            "name_at": np.array(e.name_at, np.uint64), "name_len": np.array(e.name_len, np.uint32),
            "first": np.array(e.first, np.uint64), "file_size": np.array(e.file_size, np.uint64)}
    return data, table, present, e, want


CAPS = ("cap+3", "cap=n", "blocks-1", "files-1", "query")
ROUTES = ("device", "host", "forged")


def _receive(route, cap, with_set=True):
    def run(gpu, a, ph, knobs):
        data, table, present, e, want = _ref(route == "forged")
        nb, nf = len(e.sizes), len(e.name_at)
        if route == "host":
            knobs.set("SF_TEST_WIRE_PARSE_HOST", 1)
        x = extent._dev(np.frombuffer(data, np.uint8).copy(), gpu)
        t, p = extent._dev(table, gpu), extent._dev(present, gpu)
        outs = {}
        for j, (name, dtype, width, align, section) in enumerate(OUTPUTS):
            rows = (nf + 1 if name == "first" else nf if section else nb) + EXTRA
            outs[name] = a.carve(name, width * rows, dtype, ph(j, align))
        a.watch(run=x, table=t, present=p)
        bs = device.BlockSet(t, p) if with_set else None
        bcap = {"cap+3": nb + 3, "blocks-1": nb - 1}.get(cap, nb)
        fcap = {"cap+3": nf + 3, "files-1": nf - 1}.get(cap, nf)
        ptr = {k: None if cap == "query" and k != "rows" else v.data_ptr() for k, v in outs.items()}
        n_blocks, n_files, used, end = (ctypes.c_uint64(77) for _ in range(4))
        why, still = ctypes.c_int(77), ctypes.c_int(77)
        rc = _lib.lib().sf_receive_files_device(
            bs._h if bs else None, x.data_ptr(), x.numel(), 1, BASE, ptr["digests"], ptr["sizes"], ptr["offsets"],
            ptr["rows"], ptr["block_file"], bcap, ptr["name_at"], ptr["name_len"], ptr["first"], ptr["file_size"], fcap,
            ctypes.byref(n_blocks), ctypes.byref(n_files), ctypes.byref(used), ctypes.byref(why), ctypes.byref(still),
            ctypes.byref(end), extent._s(gpu))
        assert (n_blocks.value, n_files.value, used.value, why.value, still.value) == (nb, nf, e.consumed, e.stop, 0)
        assert wire.recv_files_stats()[2] == int(route != "device")
        if cap in ("cap+3", "cap=n"):
            assert rc == 0 and end.value == e.end_offset
            a.check(want if with_set else {k: v for k, v in want.items() if k != "rows"})  # no set: d_rows untouched
        else:  # the parse's rows that fit: no offset, no file size, no row, not the last entry of first
            assert rc == _lib.SF_ENOSPC
            b, f = (0, 0) if cap == "query" else (min(nb, bcap), min(nf, fcap))
            a.check({k: want[k][:b] for k in ("digests", "sizes", "block_file")}
                    | {k: want[k][:f] for k in ("name_at", "name_len", "first")})
        if bs:
            bs.close()
    return run


for _route in ROUTES:
    for _cap in CAPS:
        _scenario(f"receive_files_device-{_route}-{_cap}")(_receive(_route, _cap))
for _cap in ("cap+3", "blocks-1"):
    _scenario(f"receive_files_device-noset-{_cap}")(_receive("device", _cap, with_set=False))


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", placement.PATTERNS, ids=lambda p: f"{p:#04x}")
@pytest.mark.parametrize("place", range(3))
@pytest.mark.parametrize("name", list(MINE))
def test_outputs_and_nothing_else(gpu, knobs, name, place, pattern):
    arena = placement.Arena(gpu, pattern)
    MINE[name](gpu, arena, lambda j, align: placement.phase(place, j, align), knobs)


def test_the_scenarios_are_in_the_written_extent_list():
    covered = {e for entries, _fn in extent.SCENARIOS.values() for e in entries}
    assert ENTRY in covered and set(MINE) <= set(extent.SCENARIOS) and len(MINE) == 17
    with open(extent.os.path.join(extent.ROOT, "include", "syncfast_amd.h")) as f:
        found = extent.device_output_functions(f.read())
    assert found[ENTRY] == ["d_digests", "d_sizes", "d_offsets", "d_rows", "d_block_file", "d_file_name_at",
                            "d_file_name_len", "d_file_first", "d_file_size"]
