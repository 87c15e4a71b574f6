"""GPU: sf_place_block_data_device writes its outputs and nothing else -- its
scenarios for test_gpu_written_extent.py's list, in that file's manner.

test_gpu_written_extent.py holds a list of written-extent scenarios against
the header (test_every_device_output_has_a_scenario): every entry point with
a device output has one.  The join of sf_want.hip has seven device outputs;
its scenarios are defined here, entered into that list through that file's
own `scenario` decorator when this module is imported (pytest imports every
test module of a run before it runs any test), and run here -- at the same
three placements and under the same two patterns, through the same arena
(tests/placement.py): the five job lists, the use counters and the rows'
present flags are carved from one allocation full of a pattern, and after the
call the whole allocation is the dict model's bytes in the rows the call must
write and the pattern everywhere else.
"""
import ctypes

import numpy as np
import pytest
import torch

import placement
import test_gpu_written_extent as extent
from syncfast_amd import _lib
from want_expect import join_case, place_model

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
EXTRA = extent.EXTRA
MINE = {}  # the scenarios of this file: name -> run(gpu, arena, ph, knobs)


def _scenario(name):
    def add(fn):
        MINE[name] = extent.scenario(name, "sf_place_block_data_device")(fn)
        return fn
    return add


def _place(short: bool, query: bool = False):
    def run(gpu, a, ph, knobs):
        case = join_case(71, many_rows=40)
        jobs, present, uses, n_left, mismatch = place_model(**case)
        need, n, m = len(jobs), len(case["row_digests"]), len(case["msg_digests"])
        assert need > m and mismatch == 1  # a fan-out, and a row that must stay as it is
        dev = lambda v, t: extent._dev(np.array(v, t), gpu)  # noqa: E731
        table = lambda ds: extent._dev(np.frombuffer(b"".join(ds), np.uint8).reshape(-1, 20), gpu)  # noqa: E731
        rd, md = table(case["row_digests"]), table(case["msg_digests"])
        rs, ms = (extent._dev(np.array(case[k], np.uint32).view(np.int32), gpu) for k in ("row_sizes", "msg_sizes"))
        rdst, moff, ok = dev(case["row_dst"], np.int64), dev(case["msg_offsets"], np.int64), dev(case["msg_ok"], np.uint8)
        outs = {}
        for j, (name, dtype, size) in enumerate((("src", I64, 8), ("dst", I64, 8), ("sizes", I32, 4), ("rows", I64, 8),
                                                 ("msgs", I64, 8))):
            outs[name] = a.carve(name, size * (need + EXTRA), dtype, ph(j, size))
        outs["uses"] = a.carve("uses", 4 * (m + EXTRA), I32, ph(5, 4))
        flags = a.carve("present", n, U8, ph(6, 1))  # in/out: the caller's flags, then the marks
        flags.copy_(dev(case["row_present"], np.uint8))
        a.watch(row_digests=rd, row_sizes=rs, row_dst=rdst, msg_digests=md, msg_sizes=ms, msg_offsets=moff, msg_ok=ok)
        n_jobs, left, bad = (ctypes.c_uint64(77) for _ in range(3))
        p = {k: None if query else v.data_ptr() for k, v in outs.items()}
        cap = need - 1 if short else need + EXTRA
        rc = _lib.lib().sf_place_block_data_device(
            rd.data_ptr(), rs.data_ptr(), rdst.data_ptr(), flags.data_ptr(), n, md.data_ptr(), ms.data_ptr(),
            moff.data_ptr(), ok.data_ptr(), m, p["src"], p["dst"], p["sizes"], p["rows"], p["msgs"], cap, p["uses"],
            ctypes.byref(n_jobs), ctypes.byref(left), ctypes.byref(bad), extent._s(gpu))
        before = np.array(case["row_present"], np.uint8)
        if short or query:  # the need, and nothing marked or written
            assert (rc, n_jobs.value, left.value, bad.value) == (_lib.SF_ENOSPC, need, int((before == 0).sum()), 1)
            a.check({"present": before})
        else:
            assert (rc, n_jobs.value, left.value, bad.value) == (0, need, n_left, 1)
            col = lambda k, t: np.array([j[k] for j in jobs], t)  # noqa: E731
            a.check({"src": col(0, np.int64), "dst": col(1, np.int64), "sizes": col(2, np.uint32),
                     "rows": col(3, np.int64), "msgs": col(4, np.int64), "uses": np.array(uses, np.int32),
                     "present": np.array(present, np.uint8)})
    return run


_scenario("place_block_data")(_place(False))
_scenario("place_block_data-short")(_place(True))
_scenario("place_block_data-query")(_place(False, query=True))


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", placement.PATTERNS, ids=lambda p: f"{p:#04x}")
@pytest.mark.parametrize("place", range(3))
@pytest.mark.parametrize("name", list(MINE))
def test_outputs_and_nothing_else(gpu, knobs, name, place, pattern):
    arena = placement.Arena(gpu, pattern)
    MINE[name](gpu, arena, lambda j, align: placement.phase(place, j, align), knobs)


def test_the_scenarios_are_in_the_written_extent_list():
    covered = {e for entries, _fn in extent.SCENARIOS.values() for e in entries}
    assert "sf_place_block_data_device" in covered and set(MINE) <= set(extent.SCENARIOS)
    with open(extent.os.path.join(extent.ROOT, "include", "syncfast_amd.h")) as f:
        found = extent.device_output_functions(f.read())
    assert found["sf_place_block_data_device"] == ["d_row_present", "d_src_offsets", "d_dst_offsets", "d_sizes",
                                                   "d_job_rows", "d_job_msgs", "d_msg_uses"]
    assert "sf_wire_get_blocks_device" not in found  # its one output is the library's run
