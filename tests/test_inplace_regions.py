"""CPU: the page-lock regions of the in-place routes
(syncfast_amd/csrc/sf_inplace.hpp: InplaceRegions), executed on the host by
tests/native/inplace_regions.cpp: a stand-alone program with its own main,
built with ASan + UBSan and run directly (nothing is loaded into Python under
a sanitizer).  index_inplace and index_list_pipeline (sf_host.cpp) hold the
same class over lock_pages / unlock_pages."""
import os
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
ENV = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("inplace_regions")
    probe = tmp / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode or \
            subprocess.run([str(tmp / "probe")], capture_output=True).returncode:
        pytest.skip("g++ -fsanitize=address,undefined unavailable")
    exe = tmp / "inplace_regions"
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "native", "inplace_regions.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_regions_locks_heads_and_unlocks_under_asan_ubsan(program):
    """Page size 4096, first start at a page edge + 3, runs of 1 to 4 stages of
    256 pages, 1,048,000 bytes or two pages and a byte, the last one also of
    one byte (160 runs), each driven as the pipelines drive it.  Per run: the
    edges; lock() asked for page ranges that overlap no earlier one and tile
    [page_down(first start), page_up(end)) in order; both pieces of every
    stage's copy, [src, src + head) and [src + head, src + n), inside one range
    locked before the stage was issued, head(0) = 0 and head <= n; a lock()
    that answers pinned-by-caller gives direct stages and no unlock; fail_at
    and a lock() that refuses, at region 0, 1, 2 and the last: every region
    from there on failed without a further lock(), direct(k) true exactly
    before it; on destruction unlock() once per locked range, by its start,
    and for nothing else; the serial form (one start): one lock(lo, hi), one
    unlock, every head 0.  And a tracker of no stages asks and frees nothing."""
    r = subprocess.run([program], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    # 4 + 12 + 36 + 108 runs; per run: default, pinned, 4 fail_at, 4 refusals, serial; the empty tracker
    assert words[0] == "ok" and int(words[1]) == 160 * 11 + 1
