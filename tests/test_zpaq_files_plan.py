"""CPU: the plan of the many-file device ZPAQ cut
(syncfast_amd/csrc/sf_cdc_files_plan.hpp) -- segments and bitmap words per
file, a segment's file, its incoming cut, the unsettled rule, the row bases --
executed on the host by tests/native/cdc_files_plan.cpp: a stand-alone program
with its own main, built with ASan + UBSan together with the host cutter
(sf_zpaq.cpp) and run directly (nothing is loaded into Python under a
sanitizer).  The kernels of sf_cdc_files.hip call the same constexpr
functions."""
import os
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
ENV = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cdc_files_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode or \
            subprocess.run([str(tmp / "probe")], capture_output=True).returncode:
        pytest.skip("g++ -fsanitize=address,undefined unavailable")
    exe = tmp / "cdc_files_plan"
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "native", "cdc_files_plan.cpp"),
                    os.path.join(ROOT, "syncfast_amd", "csrc", "sf_zpaq.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_plan_stores_every_word_and_row_once_and_gives_the_host_cutters_rows_under_asan_ubsan(program):
    """(bits, max_size) = (4, 16), (6, 256), (5, 48); files of 0, 1, 15, 16,
    L - 1, L, L + 1, 2 L, 9.5 L and 40 L bytes with empty files first, last
    and three in a row, as random, all-zero, period-7 and islands content
    (4 batches of 15 files); 32 batches of 6 mixed files whose bases take
    every byte phase 0..31; no file; only empty files.  Each batch is run
    with no cap and under caps of 1, 2 and 6 join launches: every bitmap word
    is stored only by the segment that owns it (in round 0 every word exactly
    once), every row is written exactly once inside [0, total), every settled
    file's rows are sf_zpaq_cut_buffer's, and the unsettled files are exactly
    those whose own round count is at least the cap."""
    r = subprocess.run([program], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) == 3 * (4 + 32 + 2) and int(words[2]) == 3 * (4 * 15 + 32 * 6 + 3)
