"""GPU: sf_wire_parse_get_files_device writes its two device outputs and
nothing else -- its scenarios for test_gpu_written_extent.py's list, in that
file's manner (as test_gpu_file_list_extent.py does for the files list).

The two span lists are carved from one allocation full of a pattern
(tests/placement.py), each with a few rows more than the call may write; after
the call the whole allocation is the model's bytes (get_files_expect:
wire.Parser) in the rows the call must write and the pattern everywhere else.
Two runs -- one that ends with the buffer, one that stops at a malformed line
in the middle with requests behind it -- at four capacities: room to spare,
exact, one short, and the NULL-output query.  The scenarios are entered into
that file's list through its own `scenario` decorator when this module is
imported, and run here at the same three placements and under the same two
patterns.  sf_serve_get_files_device has no device output of the caller's: its
run is the library's own allocation."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import placement
import test_gpu_written_extent as extent
from entries_expect import get_files_run
from get_files_expect import END, MALFORMED, expected
from syncfast_amd import _lib

I32, I64 = torch.int32, torch.int64
EXTRA = extent.EXTRA
MINE = {}
PARSE, SERVE = "sf_wire_parse_get_files_device", "sf_serve_get_files_device"
OUTPUTS = (("name_at", I64, 8, 8), ("name_len", I32, 4, 4))  # name, dtype, bytes per row, alignment
CAPS = ("cap+3", "cap=n", "n-1", "query")
RUNS = ("whole", "stopped")


def _scenario(name, entry_point):
    def add(fn):
        MINE[name] = extent.scenario(name, entry_point)(fn)
        return fn
    return add


@functools.lru_cache(None)
def _ref(run):
    """Seventy requests (more than one bitmap word's worth of newlines, names
    of 0 to 100 bytes); `stopped`: a name of 101 bytes behind the 40th."""
    rng = np.random.default_rng(29)
    names = [bytes(rng.integers(97, 123, int(rng.choice((0, 1, 7, 33, 100))), dtype=np.uint8)) for _ in range(70)]
    names[5] = b"bad\xff"
    if run == "whole":
        data = get_files_run(names)
    else:
        data = get_files_run(names[:40]) + b"GET_FILE\n" + b"z" * 101 + b"\n" + get_files_run(names[40:])
    e = expected(data)
    assert (len(e.names), e.stop, e.bad_name) == ((70, END, 5) if run == "whole" else (40, MALFORMED, 5))
    return data, e, {"name_at": np.array(e.name_at, np.uint64), "name_len": np.array(e.name_len, np.uint32)}


def _parse(run, cap):
    def go(gpu, a, ph, knobs):
        data, e, want = _ref(run)
        n = len(e.names)
        x = extent._dev(np.frombuffer(data, np.uint8).copy(), gpu)
        outs = {name: a.carve(name, width * (n + EXTRA), dtype, ph(j, align))
                for j, (name, dtype, width, align) in enumerate(OUTPUTS)}
        a.watch(run=x)
        c = {"cap+3": n + 3, "n-1": n - 1}.get(cap, n)
        ptr = {k: None if cap == "query" and k == "name_len" else outs[k].data_ptr() for k in outs}
        n_out, bad, used = (ctypes.c_uint64(77) for _ in range(3))
        stop = ctypes.c_int(77)
        rc = _lib.lib().sf_wire_parse_get_files_device(x.data_ptr(), x.numel(), ptr["name_at"], ptr["name_len"], c,
                                                       ctypes.byref(n_out), ctypes.byref(bad), ctypes.byref(used),
                                                       ctypes.byref(stop), extent._s(gpu))
        assert (n_out.value, bad.value, used.value, stop.value) == (n, e.bad_name, e.consumed, e.stop)
        if cap in ("cap+3", "cap=n"):
            assert rc == 0
            a.check(want)
        else:  # the rows that fit, none for a query
            assert rc == _lib.SF_ENOSPC
            k = 0 if cap == "query" else c
            a.check({"name_at": want["name_at"][:k], "name_len": want["name_len"][:k]})
    return go


for _run in RUNS:
    for _cap in CAPS:
        _scenario(f"parse_get_files-{_run}-{_cap}", PARSE)(_parse(_run, _cap))


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", placement.PATTERNS, ids=lambda p: f"{p:#04x}")
@pytest.mark.parametrize("place", range(3))
@pytest.mark.parametrize("name", list(MINE))
def test_outputs_and_nothing_else(gpu, knobs, name, place, pattern):
    arena = placement.Arena(gpu, pattern)
    MINE[name](gpu, arena, lambda j, align: placement.phase(place, j, align), knobs)


def test_the_scenarios_are_in_the_written_extent_list():
    covered = {e for entries, _fn in extent.SCENARIOS.values() for e in entries}
    assert PARSE in covered and set(MINE) <= set(extent.SCENARIOS) and len(MINE) == 8
    with open(extent.os.path.join(extent.ROOT, "include", "syncfast_amd.h")) as f:
        found = extent.device_output_functions(f.read())
    assert found[PARSE] == ["d_name_at", "d_name_len"]
    assert SERVE not in found  # its run is the library's own allocation: no output of the caller's on the device
