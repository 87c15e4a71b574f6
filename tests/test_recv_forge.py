"""tests/recv_forge.py (the forged and hostile FILE_BLOCK runs of
test_gpu_recv_forge.py) held against the parser: every forged form forges
exactly one start, and no parser reading from byte 0 sees it.  No GPU."""
import numpy as np

import recv_forge as rf
from recv_expect import END, MALFORMED, OTHER, expected, message


def _reads_a_message(run, q):
    return len(expected(run[q:])[0]) >= 1


def test_the_36_forms():
    forms = rf.forms()
    assert len(forms) == 36 and len(set(forms)) == 36
    assert sum(f == 1 for _j, _d, f in forms) == 8 and sum(f == 2 for _j, _d, f in forms) == 28
    assert all((f == 1) == (j == d + 1) and (f == 2) == (j >= d + 2) for j, d, f in forms)
    for j, d, _f in forms:
        run, p, _family = rf.forge(j, d)
        a_len = 33 + d
        assert p == 11 + j and run[p:p + 11] == rf.TAG
        # whole messages stand at 0, p and len(A), and nowhere else
        assert [q for q in range(len(run)) if _reads_a_message(run, q)] == [0, p, a_len], (j, d)
        assert sorted(rf.candidates(run)) == [0, p, a_len]
        digests, sizes, consumed, stop = expected(run)
        assert (len(digests), consumed, stop) == (2, len(run), END) and len(str(sizes[0])) == d and sizes[1] == 99
        assert rf.forged_start_in_chain(run) and rf.forged_start_in_chain(run + b"FILE_END\n")


def test_every_other_j_d_has_no_form():
    assert [(j, d) for j in range(10) for d in range(1, 11) if rf.forge(j, d) is None] == \
        [(j, d) for j in range(10) for d in range(1, 11) if j < d + 1]
    assert rf.forge(10, 1) is None and rf.forge(5, 0) is None and rf.forge(5, 11) is None


def test_candidates_are_where_the_parser_reads_a_message():
    rng = np.random.default_rng(1)
    run = rf.hostile_run(60, rng) + b"FILE_END\n" + rf.forge(9, 1)[0]
    assert sorted(rf.candidates(run)) == [q for q in range(len(run)) if _reads_a_message(run, q)]


def test_forged_start_in_chain():
    honest = rf.honest_prefix(500, np.random.default_rng(2))
    pair = rf.forge(6, 3)[0]
    assert not rf.forged_start_in_chain(honest) and not rf.forged_start_in_chain(b"") and \
        not rf.forged_start_in_chain(b"FILE_END\n" + pair)
    assert rf.forged_start_in_chain(honest + pair) and rf.forged_start_in_chain(pair + honest)
    assert not rf.forged_start_in_chain(honest + b"FILE_END\n" + pair)  # behind the stop
    broken = b"FILE_BLOCK\n" + bytes(20) + b"x12\n"
    assert expected(honest + broken + pair)[2:] == (500, MALFORMED)
    assert not rf.forged_start_in_chain(honest + broken + pair)
    assert expected(honest + b"FILE_END\n" + pair)[2:] == (500, OTHER)


def test_honest_prefix_lengths():
    rng = np.random.default_rng(3)
    for total in [0, 34, 43, 68, 86, 136, 137, 200, 4096 + 17, 16384 + 63]:
        run = rf.honest_prefix(total, rng)
        digests, sizes, consumed, stop = expected(run)
        assert (consumed, stop) == (total, END) and len(run) == total
        assert all(34 <= 33 + len(str(s)) <= 43 for s in sizes)
        assert sorted(rf.candidates(run)) == np.cumsum([0] + [33 + len(str(s)) for s in sizes])[:-1].tolist()


def test_hostile_seeds_of_the_gpu_test_forge_and_do_not():
    got = [rf.forged_start_in_chain(rf.hostile_run(2000, np.random.default_rng(seed))) for seed in (0, 1, 2, 3)]
    assert got == [True, False, True, False]


def test_hostile_runs_are_read_whole():
    rng = np.random.default_rng(4)
    fields = [rf.hostile_size_field(rng) for _ in range(4000)]
    assert {len(f) for f in fields} == set(range(1, 16))
    assert any(f.startswith(b"+0") for f in fields) and any(f.startswith(b"00") for f in fields)
    run = rf.hostile_run(300, rng)
    digests, sizes, consumed, stop = expected(run)
    assert (len(digests), consumed, stop) == (300, len(run), END) and max(sizes) < 1 << 32
    body = b"".join(digests)
    hostile = set(b"\n+0123456789" + rf.TAG)
    assert sum(c in hostile for c in body) > len(body) * 3 // 4
    assert body.count(b"\n") > 300 and body.count(rf.TAG) > 30
    assert message(digests[0], sizes[0])[:31] == run[:31]
