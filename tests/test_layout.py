"""CPU: how a device entry point divides its one scratch allocation and cuts
a launch into pieces (syncfast_amd/csrc/sf_layout.hpp: ScratchLayout,
for_pieces), executed on the host by tests/native/layout.cpp: a stand-alone
program with its own main, built with ASan + UBSan and run directly (nothing
is loaded into Python under a sanitizer).  The .hip files use the same header;
their split loops only split above 2^30 items, so this is where they run."""
import os
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
ENV = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("layout")
    probe = tmp / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode or \
            subprocess.run([str(tmp / "probe")], capture_output=True).returncode:
        pytest.skip("g++ -fsanitize=address,undefined unavailable")
    exe = tmp / "layout"
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "layout.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def test_scratch_parts_and_launch_pieces_under_asan_ubsan(program):
    """ScratchLayout: every offset a multiple of 256, the parts in declaration
    order and disjoint (each filled over its whole size inside a heap block of
    exactly total() bytes), total() = the last offset + its rounded size, with
    a zero-byte part and the conditional part of sf_want.hip (distinct ? n * 8
    : 0) against the sum it replaced.  for_pieces with max = 4 and n in {0, 1,
    3, 4, 5, 13}: the pieces tile [0, n) exactly and in order, each <= max, no
    call for n = 0, and an error from any call stops the loop and is returned;
    with the entry points' bound 2^30, n = 2^30 is one piece and 2^30 + 1 two."""
    r = subprocess.run([program], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    # 48 layouts; per n one tiling and one error run per piece (15), the two 2^30 cases
    assert words[0] == "ok" and int(words[1]) == 48 + 15 + 2
