"""CPU: the plan of the block copy kernel (syncfast_amd/csrc/sf_copy_plan.hpp)
-- the tile count of a job, the head / body / tail split of a tile, the loads
of a 16-byte store and the range test -- executed on the host by
tests/native/copy_plan.cpp: a stand-alone program with its own main, built
with ASan + UBSan and run directly (nothing is loaded into Python under a
sanitizer).  The kernel of sf_copy.hip calls the same constexpr functions."""
import os
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
ENV = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("copy_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode or \
            subprocess.run([str(tmp / "probe")], capture_output=True).returncode:
        pytest.skip("g++ -fsanitize=address,undefined unavailable")
    exe = tmp / "copy_plan"
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "copy_plan.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def test_plan_covers_every_job_exactly_and_loads_stay_inside_under_asan_ubsan(program):
    """Every (source address & 15, destination address & 15), every size
    0..80 and T - 1, T, T + 1, 2T + 1, with the destination at a window's
    start and just before its end, and with the source buffer ending exactly
    at the job's end and starting exactly at its start (heap copies of exact
    length): the pieces store every destination byte exactly once and no other,
    at most 15 byte stores at each end and aligned 16-byte stores between,
    every modelled load lies inside the source buffer, the bytes that arrive
    are the source's; and the range test, offset = 2^64 - 1 with size = 2
    included."""
    r = subprocess.run([program], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) == 16 * 16 * 85 * 2 * 4 + 2
