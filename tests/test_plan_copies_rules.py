"""CPU: the per-block rules of sf_plan_copies_device alone
(syncfast_amd/csrc/sf_plan_copies.hpp), executed by tests/native/plan_copies.cpp:
a stand-alone program with its own main, built with ASan + UBSan and run
directly (nothing is loaded into Python under a sanitizer).  Without an
argument it holds every class, the first-match order and the edges of the sums
against their definitions; with a case file it makes the whole plan serially,
as the kernels do, and the expected plan is the Python model's
(tests/plan_expect.py)."""
import hashlib
import os
import subprocess

import pytest

import plan_expect as pe

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
ENV = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
CLASS_NUMBER = {"missing": 0, "size_mismatch": 1, "stale": 2, "unavailable": 3, "empty": 4, "job": 6, "unverified": 7}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("plan_copies")
    probe = tmp / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode or \
            subprocess.run([str(tmp / "probe")], capture_output=True).returncode:
        pytest.skip("g++ -fsanitize=address,undefined unavailable")
    exe = tmp / "plan_copies"
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "native", "plan_copies.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _run(program, *args):
    r = subprocess.run([program, *args], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_rules_under_asan_ubsan(program):
    assert _run(program).strip() == "ok"


def _case_file(case, query, verify):
    """The case as tests/native/plan_copies.cpp reads it; hashlib stands for
    the explicit-list kernel (a block with no bytes to hash gets zeros)."""
    src, lines = case["src"], []
    n = len(case["sizes"])
    for i in range(n):
        r, computed = case["rows"][i], bytes(20)
        if 0 <= r < len(case["table_file"]) and case["table_file"][r] < len(case["local_base"]):
            base = case["local_base"][case["table_file"][r]]
            at = base + case["table_offset"][r]
            if base != pe.NOT_LOADED and at + case["sizes"][i] <= len(src):
                computed = hashlib.sha1(src[at:at + case["sizes"][i]]).digest()
        lines.append(f"{r} {case['sizes'][i]} {case['offsets'][i]} {case['block_file'][i]} "
                     f"{bytes(case['digests'][i]).hex()} {computed.hex()}")
    lines += [str(b) for b in case["file_base"]]
    lines += [f"{j} {o} {z}" for j, o, z in zip(case["table_file"], case["table_offset"], case["table_size"])]
    lines += [f"{b} {z}" for b, z in zip(case["local_base"], case["local_size"])]
    head = (f"{n} {len(case['file_base'])} {len(case['table_file'])} {len(case['local_size'])} {int(query)} "
            f"{int(verify)} {len(src)}")
    return "\n".join([head] + lines) + "\n"


def _model_text(case, query, verify):
    m = pe.plan_model(**dict(case, local_base=None if query else case["local_base"],
                             src=case["src"] if verify else None))
    if m == pe.ERANGE:
        return "ERANGE\n"
    out = [" ".join(str(c) for c in m["counts"])]
    out += [f"{CLASS_NUMBER[c]} {p} {a} {d}" for c, p, a, d in zip(m["cls"], m["present"], m["ask"], m["dst"])]
    out += [f"{s} {d} {z} {i}" for s, d, z, i in m["jobs"]]
    out += [str(k) for k in m["local_jobs"]]
    return "\n".join(out) + "\n"


@pytest.mark.parametrize("n", [0, 1, 7, 64, 65, 300])
def test_the_serial_plan_is_the_models(program, tmp_path, n):
    case = pe.mixed_case(500 + n, n)
    path = tmp_path / "case.txt"
    for query, verify in ((False, True), (False, False), (True, False), (True, True)):
        path.write_text(_case_file(case, query, verify))
        assert _run(program, str(path)) == _model_text(case, query, verify), (query, verify)
    if n >= 7:  # the mixed case holds every class
        m = pe.plan_model(**case)
        assert all(c > 0 for c in m["counts"])


@pytest.mark.parametrize("what", ["row", "file", "section", "dst", "dst-ok", "arena", "arena-ok"])
def test_bad_input_is_refused_as_the_model_refuses_it(program, tmp_path, what):
    case = pe.mixed_case(77, 20)
    job = pe.plan_model(**case)["jobs"][0][3]  # a block that is a job
    r = case["rows"][job]
    if what == "row":
        case["rows"][3] = len(case["table_file"])
    elif what == "file":
        case["table_file"][r] = len(case["local_size"])
    elif what == "section":
        case["block_file"][-1] = len(case["file_base"])
    elif what in ("dst", "dst-ok"):  # the sum one past 2^64 - 1, and at it
        case["file_base"][1] = pe.U64 - case["offsets"][-1] - (what == "dst-ok")
    else:  # the last candidate byte one past the arena's last, and at it
        m = pe.plan_model(**case)
        end = max(case["local_base"][case["table_file"][case["rows"][i]]] + case["table_offset"][case["rows"][i]]
                  + case["sizes"][i] for i, c in enumerate(m["cls"]) if c in ("job", "unverified"))
        case["src"] = case["src"][:end - (what == "arena")]
    path = tmp_path / "case.txt"
    path.write_text(_case_file(case, False, True))
    got = _run(program, str(path))
    assert got == _model_text(case, False, True)
    assert (got == "ERANGE\n") == (not what.endswith("-ok"))
