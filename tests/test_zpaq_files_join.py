"""tests/zpaq_files_join.py (the restatement of the many-file device cut's
join that test_gpu_zpaq_files.py asserts against) on the batch those tests use,
with every file's round count pinned by `zpaq_cuts`, the Python chunker of
test_zpaq.py -- so nothing in these cases rests on the code they pin -- and on
small batches whose launch count, unsettled set and row bases are worked out
by hand from the per-file counts.  No GPU."""
import pytest

import zpaq_files_join as zfj
import zpaq_join as zj
from test_zpaq_join import py_ends

BITS, MAX_SIZE = 6, 256


@pytest.fixture(scope="module")
def table():
    return zfj.table_files()


def test_the_tables_round_counts_with_the_python_chunker(table):
    """zeros join one segment per round (40 L: 39 rounds; 12 L + 5: 12, the
    5-byte tail segment included), so does period 7 until its last segments
    sync (20 L: 18); random bytes sync at once; the islands take 5."""
    assert zj.segment_len(MAX_SIZE) == zfj.L_TABLE
    for name, data, rounds in table:
        assert zj.restate(data, BITS, MAX_SIZE, ends=py_ends).rounds == rounds, name
    j = zfj.restate_files([d for _n, d, _r in table], BITS, MAX_SIZE, ends=py_ends)
    assert j.rounds == [39, 12, 18, 1, 0, 1, 5]
    assert j == zfj.restate_files([d for _n, d, _r in table], BITS, MAX_SIZE)  # the C cutter gives the same


def test_no_cap_runs_to_the_slowest_file_and_one_launch_more(table):
    files = [d for _n, d, _r in table]
    j = zfj.restate_files(files, BITS, MAX_SIZE)
    assert j.launches == 40 and j.unsettled == [False] * 7
    assert j.segments == 40 + 13 + 20 + 10 + 1 + 2 + zj.restate(files[6], BITS, MAX_SIZE).nseg
    assert j.recut == sum(zj.restate(d, BITS, MAX_SIZE).recut for d in files)
    assert j.first_row[-1] == sum(len(t) for t in j.true_ends)
    assert [b - a for a, b in zip(j.first_row, j.first_row[1:])] == [len(t) for t in j.true_ends]


def test_a_cap_of_six_leaves_the_three_constant_or_periodic_files(table):
    files = [d for _n, d, _r in table]
    j = zfj.restate_files(files, BITS, MAX_SIZE, max_rounds=6)
    assert j.launches == 6 and j.recut is None
    assert j.unsettled == [True, True, True, False, False, False, False]
    assert j.first_row[:4] == [0, 0, 0, 0]  # no rows
    assert [b - a for a, b in zip(j.first_row[3:], j.first_row[4:])] == [len(t) for t in j.true_ends[3:]]


def test_the_cap_at_and_beside_a_files_own_count(table):
    """islands: 5 rounds.  With random-L+1 (1 round): no cap makes 6 launches;
    a cap of 6 is not reached by anything (the sixth launch changes nothing);
    a cap of 5 ends the loop with the islands still cutting in launch 5; a cap
    of 1 leaves both files."""
    files = [table[6][1], table[5][1]]
    assert [zfj.restate_files(files, BITS, MAX_SIZE, m).launches for m in (0, 7, 6, 5, 1)] == [6, 6, 6, 5, 1]
    assert zfj.restate_files(files, BITS, MAX_SIZE, 6).unsettled == [False, False]
    assert zfj.restate_files(files, BITS, MAX_SIZE, 6).recut is not None
    assert zfj.restate_files(files, BITS, MAX_SIZE, 5).unsettled == [True, False]
    assert zfj.restate_files(files, BITS, MAX_SIZE, 2).unsettled == [True, False]
    assert zfj.restate_files(files, BITS, MAX_SIZE, 1).unsettled == [True, True]


def test_one_segment_files_and_empty_batches_make_no_launch(table):
    one = [table[4][1], b"", b"x" * 15, b""]
    j = zfj.restate_files(one, BITS, MAX_SIZE, 6)
    assert (j.launches, j.segments, j.recut, j.unsettled) == (0, 2, 0, [False] * 4)
    assert j.first_row[1] == j.first_row[2] and j.first_row[3] == j.first_row[4]
    j = zfj.restate_files([], BITS, MAX_SIZE)
    assert (j.launches, j.segments, j.first_row) == (0, 0, [0])
    assert zfj.restate_files([b"", b""], BITS, MAX_SIZE).first_row == [0, 0, 0]
