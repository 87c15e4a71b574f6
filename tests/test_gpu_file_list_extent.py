"""GPU: sf_receive_file_entries_device writes its seven device outputs and
nothing else, and sf_name_set_lookup its rows -- their scenarios for
test_gpu_written_extent.py's list, in that file's manner (as
test_gpu_recv_files_extent.py does for sf_receive_files_device).

The four parsed lists and the three lookup lists are carved from one
allocation full of a pattern (tests/placement.py), each with a few rows more
than the call may write; after the call the whole allocation is the model's
bytes (entries_expect: wire.Parser; the need by the definition of
include/syncfast_amd.h over a dict) in the rows the call must write and the
pattern everywhere else.  Three routes -- the chain on the device,
SF_TEST_WIRE_PARSE_HOST, and the fallback after a start forged by a digest --
at four capacities: room to spare, exact, one short, and the NULL-output
query; with and without a set.  The scenarios are entered into that file's
list through its own `scenario` decorator when this module is imported, and
run here at the same three placements and under the same two patterns."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import placement
import test_gpu_written_extent as extent
from entries_expect import END_FILES, entry, expected, needs_fallback
from syncfast_amd import _lib, device

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
EXTRA = extent.EXTRA
MINE = {}
ENTRY, LOOKUP = "sf_receive_file_entries_device", "sf_name_set_lookup"
# name, dtype, bytes per row, alignment, a lookup output
OUTPUTS = (("name_at", I64, 8, 8, False), ("name_len", I32, 4, 4, False), ("sizes", I64, 8, 8, False),
           ("hashes", U8, 20, 4, False), ("rows", I64, 8, 8, True), ("need", U8, 1, 1, True),
           ("need_list", I32, 4, 4, True))
NAMES = [b"same", b"changed", b"twice", b"twice", b"", b"nohash", b"dir/\xc3\xa9", b"n" * 100]  # the destination's rows
PRESENT = [1, 1, 0, 1, 1, 1, 1, 1]  # the first "twice" is temporary: the second answers


def _scenario(name, entry_point):
    def add(fn):
        MINE[name] = extent.scenario(name, entry_point)(fn)
        return fn
    return add


def model_rows(queries):
    """The lowest present row of each name, or -1."""
    first = {}
    for r, (n, p) in enumerate(zip(NAMES, PRESENT)):
        if p:
            first.setdefault(n, r)
    return np.array([first.get(q, -1) for q in queries], np.int64)


@functools.lru_cache(None)
def _ref(forged: bool):
    """Eleven entries, END_FILES and a late entry nobody reads."""
    rng = np.random.default_rng(23)
    have = rng.integers(0, 256, (len(NAMES), 20), dtype=np.uint8)
    have_ok = np.array([1, 1, 1, 1, 1, 0, 1, 1], np.uint8)
    h = lambda r: have[r].tobytes()  # noqa: E731
    other = bytes(rng.integers(0, 256, 20, dtype=np.uint8))
    first_byte, last_byte = bytes([have[7][0] ^ 1]) + h(7)[1:], h(6)[:19] + bytes([have[6][19] ^ 0x80])
    head = b"FILE_ENTRY\n\n1\n" + b"z" * 6  # a digest that spells an entry's start; the 2-byte name behind it completes it
    data = (entry(b"same", 5, h(0)) + entry(b"changed", 10 ** 15 - 1, other) + entry(b"unknown", 0, h(0))
            + entry(b"twice", 1, h(3)) + entry(b"", 2, h(4)) + entry(b"nohash", 3, h(5))
            + entry(b"dir/\xc3\xa9", 4, last_byte) + entry(b"n" * 100, 5, first_byte)
            + entry(b"f", 6, head if forged else other) + entry(b"ab", 7, other) + entry(b"twice", b"+007", h(2))
            + b"END_FILES\n" + entry(b"late", 1, other))
    assert needs_fallback(data) == forged
    e = expected(data)
    assert (len(e.sizes), e.stop, e.bad_name) == (11, END_FILES, None)
    rows = model_rows(e.names)
    need = np.array([r < 0 or not have_ok[r] or e.hashes[i] != h(r) for i, r in enumerate(rows)], np.uint8)
    assert need.tolist() == [0, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1] and rows[3] == 3 and rows[10] == 3
    want = {"name_at": np.array(e.name_at, np.uint64), "name_len": np.array(e.name_len, np.uint32),
            "sizes": np.array(e.sizes, np.uint64), "hashes": np.frombuffer(b"".join(e.hashes), np.uint8),
            "rows": rows, "need": need, "need_list": np.flatnonzero(need).astype(np.uint32)}
    return data, have, have_ok, e, want


CAPS = ("cap+3", "cap=n", "n-1", "query")
ROUTES = ("device", "host", "forged")


def _receive(route, cap, with_set=True):
    def run(gpu, a, ph, knobs):
        data, have, have_ok, e, want = _ref(route == "forged")
        n = len(e.sizes)
        if route == "host":
            knobs.set("SF_TEST_WIRE_PARSE_HOST", 1)
        x = extent._dev(np.frombuffer(data, np.uint8).copy(), gpu)
        hv, ok = extent._dev(have, gpu), extent._dev(have_ok, gpu)
        outs = {}
        for j, (name, dtype, width, align, lookup) in enumerate(OUTPUTS):
            outs[name] = a.carve(name, width * (n + EXTRA), dtype, ph(j, align))
        a.watch(run=x, have=hv, have_ok=ok)
        ns = device.NameSet.build(NAMES, PRESENT, gpu) if with_set else None
        if ns:
            a.watch(names=ns.names, name_at=ns.name_at, present=ns.present)
        c = {"cap+3": n + 3, "n-1": n - 1}.get(cap, n)
        ptr = {k: None if (cap == "query" and k != "rows") or (lookup and not ns) else outs[k].data_ptr()
               for k, _d, _w, _a, lookup in OUTPUTS}
        n_out, n_need, bad, used = (ctypes.c_uint64(77) for _ in range(4))
        why = ctypes.c_int(77)
        rc = _lib.lib().sf_receive_file_entries_device(
            ns._h if ns else None, x.data_ptr(), x.numel(), hv.data_ptr() if ns else None, ok.data_ptr() if ns else None,
            *(ptr[k] for k, *_ in OUTPUTS), c, ctypes.byref(n_out), ctypes.byref(n_need), ctypes.byref(bad),
            ctypes.byref(used), ctypes.byref(why), extent._s(gpu))
        assert (n_out.value, bad.value, used.value, why.value) == (n, (1 << 64) - 1, e.consumed, e.stop)
        stats = device.file_entries_stats()
        assert stats[0] == ROUTES.index(route) and stats[2] == n
        parsed = ("name_at", "name_len", "sizes", "hashes")
        if cap in ("cap+3", "cap=n"):
            assert rc == 0 and n_need.value == (int(want["need"].sum()) if ns else 0)
            a.check(want if ns else {k: want[k] for k in parsed})
            assert stats[3] == (1 if route == "device" else 2 if route == "forged" else 1) + (1 if ns else 0)
        else:  # the parse's rows that fit: no row, no need, no list entry
            assert rc == _lib.SF_ENOSPC and n_need.value == 0
            k = 0 if cap == "query" else c
            a.check({"name_at": want["name_at"][:k], "name_len": want["name_len"][:k], "sizes": want["sizes"][:k],
                     "hashes": want["hashes"][:20 * k]})
        if ns:
            ns.close()
    return run


for _route in ROUTES:
    for _cap in CAPS:
        _scenario(f"receive_file_entries-{_route}-{_cap}", ENTRY)(_receive(_route, _cap))
for _cap in ("cap+3", "n-1"):
    _scenario(f"receive_file_entries-noset-{_cap}", ENTRY)(_receive("device", _cap, with_set=False))


@_scenario("name_set_lookup", LOOKUP)
def _lookup(gpu, a, ph, knobs):
    queries = [b"twice", b"", b"n" * 100, b"n" * 99, b"nohas", b"nohash", b"nohash\0", b"dir/\xc3\xa9", b"same", b"x"]
    packed, at = device.pack_names(queries, gpu)
    lens = (at[1:] - at[:-1]).to(I32)
    starts = at[:-1].contiguous()
    rows = a.carve("rows", 8 * (len(queries) + EXTRA), I64, ph(0, 8))  # the rows beyond n_query stay
    with device.NameSet.build(NAMES, PRESENT, gpu) as ns:
        a.watch(bytes=packed, at=starts, lens=lens, names=ns.names, name_at=ns.name_at, present=ns.present)
        rc = _lib.lib().sf_name_set_lookup(ns._h, packed.data_ptr(), packed.numel(), starts.data_ptr(), lens.data_ptr(),
                                           len(queries), rows.data_ptr(), extent._s(gpu))
        assert rc == 0
        want = model_rows(queries)
        assert want.tolist() == [3, 4, 7, -1, -1, 5, -1, 6, 0, -1]
        a.check({"rows": want})


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", placement.PATTERNS, ids=lambda p: f"{p:#04x}")
@pytest.mark.parametrize("place", range(3))
@pytest.mark.parametrize("name", list(MINE))
def test_outputs_and_nothing_else(gpu, knobs, name, place, pattern):
    arena = placement.Arena(gpu, pattern)
    MINE[name](gpu, arena, lambda j, align: placement.phase(place, j, align), knobs)


def test_the_scenarios_are_in_the_written_extent_list():
    covered = {e for entries, _fn in extent.SCENARIOS.values() for e in entries}
    assert {ENTRY, LOOKUP} <= covered and set(MINE) <= set(extent.SCENARIOS) and len(MINE) == 15
    with open(extent.os.path.join(extent.ROOT, "include", "syncfast_amd.h")) as f:
        found = extent.device_output_functions(f.read())
    assert found[ENTRY] == ["d_name_at", "d_name_len", "d_sizes", "d_hashes", "d_rows", "d_need", "d_need_list"]
    assert found[LOOKUP] == ["d_rows"]
    assert not {"sf_name_set_build", "sf_wire_file_entries_device", "sf_wire_get_files_device"} & set(found)
