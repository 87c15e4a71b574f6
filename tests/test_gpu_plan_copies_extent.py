"""GPU: sf_plan_copies_device and sf_read_fd_device write their outputs and
nothing else -- their scenarios for test_gpu_written_extent.py's list, in that
file's manner.

test_gpu_written_extent.py holds a list of written-extent scenarios against
the header (test_every_device_output_has_a_scenario): every entry point with
a device output has one.  The plan has eight device outputs and the loader
one; their scenarios are defined here, entered into that list through that
file's own `scenario` decorator when this module is imported, and run here --
at the same three placements and under the same two patterns, through the same
arena (tests/placement.py): every output is carved from one allocation full of
a pattern, and after the call the whole allocation is the dict model's bytes
(tests/plan_expect.py) in the rows the call must write and the pattern
everywhere else.  A call whose cap is one short and a query write
d_local_jobs and nothing else."""
import ctypes

import numpy as np
import pytest
import torch

import placement
import plan_expect as pe
import test_gpu_written_extent as extent
from syncfast_amd import _lib
from test_gpu_plan_copies import model_of, on_device

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
EXTRA = extent.EXTRA
MINE = {}  # the scenarios of this file: name -> run(gpu, arena, ph, knobs)
N = 130


def _scenario(name, entry):
    def add(fn):
        MINE[name] = extent.scenario(name, entry)(fn)
        return fn
    return add


def _plan(how):
    def run(gpu, a, ph, knobs):
        query, short = how == "query", how == "short"
        case = pe.mixed_case(88, N)
        m = model_of(case, query=query)
        need, nl = len(m["jobs"]), len(case["local_size"])
        assert need > 10 and all(c > 0 for k, c in zip(pe.COUNTS, m["counts"]) if not (query and k in
                                                                                       ("unverified", "unavailable")))
        x = on_device(case, gpu)
        o = {"present": a.carve("present", N + EXTRA, U8, ph(0, 1)), "ask": a.carve("ask", N + EXTRA, U8, ph(1, 1)),
             "dst": a.carve("dst", 8 * (N + EXTRA), I64, ph(2, 8))}
        for j, (name, dtype, size) in enumerate((("src_offsets", I64, 8), ("dst_offsets", I64, 8),
                                                 ("job_sizes", I32, 4), ("job_blocks", I64, 8))):
            o[name] = a.carve(name, size * (need + EXTRA), dtype, ph(3 + j, size))
        o["local_jobs"] = a.carve("local_jobs", 4 * (nl + EXTRA), I32, ph(7, 4))
        a.watch(**x)
        counts = (ctypes.c_uint64 * 8)()
        cap = need - 1 if short else need + EXTRA
        p = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
        rc = _lib.lib().sf_plan_copies_device(
            p(x["digests"]), p(x["sizes"]), p(x["offsets"]), p(x["rows"]), p(x["block_file"]), N, p(x["file_base"]),
            x["file_base"].numel(), p(x["table_file"]), p(x["table_offset"]), p(x["table_size"]),
            x["table_file"].numel(), None if query else p(x["local_base"]), p(x["local_size"]), nl, p(x["src"]),
            x["src"].numel(), p(o["present"]), p(o["ask"]), p(o["dst"]), p(o["src_offsets"]), p(o["dst_offsets"]),
            p(o["job_sizes"]), p(o["job_blocks"]), cap, p(o["local_jobs"]), counts, extent._s(gpu))
        assert list(counts) == m["counts"]
        want = {"local_jobs": np.array(m["local_jobs"], np.uint32)}
        if short or query:  # the need, the files to load, and nothing else
            assert rc == _lib.SF_ENOSPC
        else:
            assert rc == 0
            col = lambda k, t: np.array([j[k] for j in m["jobs"]], t)  # noqa: E731
            want.update(present=np.array(m["present"], np.uint8), ask=np.array(m["ask"], np.uint8),
                        dst=np.array(m["dst"], np.uint64), src_offsets=col(0, np.uint64), dst_offsets=col(1, np.uint64),
                        job_sizes=col(2, np.uint32), job_blocks=col(3, np.int64))
        a.check(want)
    return run


_scenario("plan_copies", "sf_plan_copies_device")(_plan("full"))
_scenario("plan_copies-short", "sf_plan_copies_device")(_plan("short"))
_scenario("plan_copies-query", "sf_plan_copies_device")(_plan("query"))


def _read_fd(length, offset):
    def run(gpu, a, ph, knobs):
        import tempfile
        data = extent._bytes(length + offset, length + offset + 50)
        out = a.carve("dst", length + 7, U8, ph(0, 1))
        n = ctypes.c_uint64(0)
        with tempfile.TemporaryFile() as f:
            f.write(data.tobytes())
            f.flush()
            rc = _lib.lib().sf_read_fd_device(f.fileno(), None, offset, length, out.data_ptr(), ctypes.byref(n),
                                              extent._s(gpu))
        assert (rc, n.value) == (0, length)
        a.check({"dst": data[offset:offset + length]})  # the 7 bytes after the read stay
    return run


_scenario("read_fd-5001-at3", "sf_read_fd_device")(_read_fd(5001, 3))
_scenario("read_fd-15-at0", "sf_read_fd_device")(_read_fd(15, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", placement.PATTERNS, ids=lambda p: f"{p:#04x}")
@pytest.mark.parametrize("place", range(3))
@pytest.mark.parametrize("name", list(MINE))
def test_outputs_and_nothing_else(gpu, knobs, name, place, pattern):
    arena = placement.Arena(gpu, pattern)
    MINE[name](gpu, arena, lambda j, align: placement.phase(place, j, align), knobs)


def test_the_scenarios_are_in_the_written_extent_list():
    covered = {e for entries, _fn in extent.SCENARIOS.values() for e in entries}
    assert {"sf_plan_copies_device", "sf_read_fd_device"} <= covered and set(MINE) <= set(extent.SCENARIOS)
    with open(extent.os.path.join(extent.ROOT, "include", "syncfast_amd.h")) as f:
        found = extent.device_output_functions(f.read())
    assert found["sf_plan_copies_device"] == ["d_present", "d_ask", "d_dst", "d_src_offsets", "d_dst_offsets",
                                              "d_job_sizes", "d_job_blocks", "d_local_jobs"]
    assert found["sf_read_fd_device"] == ["d_dst"]
