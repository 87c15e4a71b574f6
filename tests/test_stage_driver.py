"""The host pipelines' stage driver and file reader
(syncfast_amd/csrc/sf_stage.hpp) alone: tests/native/stage_driver.cpp, a
stand-alone program with its own main, built with ASan + UBSan and run
directly.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_stage_driver_under_asan_ubsan(tmp_path):
    """two_stage: order, exactly-once harvest and buffer-set reuse for 0..5
    stages; an error from issue(k) or harvest(k) is the last call and the
    result; the no-more-stages answer at k = 0..3 harvests what was issued.
    read_fully / read_slices / for_slices against files of 0, 1, 4 MiB - 1
    and 4 MiB + 1 bytes, and a request past EOF."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode:
        pytest.skip("g++ -fsanitize=address,undefined unavailable")
    exe = tmp_path / "stage_driver"
    subprocess.run(["g++", *san, "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "stage_driver.cpp"),
                    "-o", str(exe), "-lpthread"], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and not r.stderr, r.stderr[-4000:]
