"""GPU: the device parse of FILE_BLOCK runs (sf_recv.hip) on content chosen
to forge message starts, at the positions and run lengths where its kernels
change path: 16 positions per lane, 64 per bitmap word, the 20 bytes a
lane's dword path needs, 4096 positions per candidates workgroup, 16384 per
chain workgroup.  What a run parses to is recv_expect.expected (wire.Parser);
the forged runs and the scan that says whether a run must fall back are
tests/recv_forge.py, pinned by test_recv_forge.py."""
import numpy as np
import pytest
import torch

import oracle
import recv_forge as rf
from recv_expect import END, INCOMPLETE, MALFORMED, OTHER, expected
from syncfast_amd import wire
from syncfast_amd.device import BlockSet
from test_gpu_recv import _check, _dev, _honest

pytestmark = pytest.mark.gpu

FORMS = rf.forms()
ONE_OF_EACH = [(2, 1), (9, 4)]  # family 1 (j = d + 1) and family 2 (j >= d + 2)


def test_one_of_each_family():
    assert [rf.forge(j, d)[2] for j, d in ONE_OF_EACH] == [1, 2] and len(FORMS) == 36


@pytest.mark.parametrize("j,d,family", FORMS)
def test_every_forged_form_alone(gpu, j, d, family):
    run, p, got_family = rf.forge(j, d)
    assert got_family == family
    assert sorted(rf.candidates(run)) == [0, p, 33 + d]
    stats = _check(run, gpu)
    assert stats[0] == 3 and stats[2] == 1
    stats = _check(run + b"FILE_END\n", gpu)
    assert stats[0] == 3 and stats[2] == 1


def _starts(run):
    """Where the parser's messages start."""
    out, q = [], 0
    cand = rf.candidates(run)
    _d, _s, consumed, _stop = expected(run)
    while q < consumed:
        out.append(q)
        q += cand[q]
    return out


def _prefix_for(p, residue, beyond, rng):
    """Honest messages after which the forged start p lands at `residue`
    mod 64, at or past `beyond`."""
    total = max(beyond - p, 0)
    while (total + p) % 64 != residue or 0 < total < 136:
        total += 1
    return rf.honest_prefix(total, rng)


@pytest.mark.parametrize("beyond", [0, 4096, 16384])
@pytest.mark.parametrize("j,d", ONE_OF_EACH)
def test_forged_start_at_word_lane_and_workgroup_edges(gpu, j, d, beyond):
    pair, p, _family = rf.forge(j, d)
    rng = np.random.default_rng(100 * j + d)
    tail = rf.honest_prefix(200, rng)
    # residues 0, 15, 16, 17, 47 and 63 of the first reachable word, and 0 of the word after it
    for residue, further in ((0, 0), (15, 0), (16, 0), (17, 0), (47, 0), (63, 0), (0, 64)):
        before = _prefix_for(p, residue, beyond + further, rng)
        at = len(before) + p
        assert at % 64 == residue and at >= beyond and at < beyond + 64 + 64 + 136
        run = before + pair + tail
        n_msgs = len(expected(before)[0]) + 2 + len(expected(tail)[0])
        assert sorted(set(rf.candidates(run)) - {at}) == sorted(_starts(run)) and len(_starts(run)) == n_msgs
        stats = _check(run, gpu)
        assert stats[0] == n_msgs + 1 and stats[2] == 1, residue


@pytest.mark.parametrize("j,d", ONE_OF_EACH)
def test_forged_start_inside_the_last_chained_message(gpu, j, d):
    """The forged pair as the last two of 300 messages: the forged start lies
    in message 298, the last whose link the chain kernel finds bad."""
    pair = rf.forge(j, d)[0]
    before, _, _ = _honest(298, seed=61)
    run = before + pair
    assert len(expected(run)[0]) == 300 and rf.forged_start_in_chain(run)
    assert max(rf.candidates(run)) == len(before) + 33 + d and len(rf.candidates(run)) == 301
    for tail, stop in ((b"", END), (b"FILE_END\n", OTHER)):
        assert expected(run + tail)[3] == stop
        stats = _check(run + tail, gpu)
        assert stats[0] == 301 and stats[2] == 1


@pytest.mark.parametrize("j,d", ONE_OF_EACH)
def test_forged_pair_behind_the_stop_does_not_fall_back(gpu, j, d):
    pair = rf.forge(j, d)[0]
    before, _, _ = _honest(70, seed=62)
    broken = b"FILE_BLOCK\n" + bytes(range(60, 80)) + b"x12\n"  # the digest is not terminated
    for stopper, stop in ((b"FILE_END\n", OTHER), (broken, MALFORMED)):
        run = before + stopper + pair
        digests, _s, consumed, got = expected(run)
        assert (len(digests), consumed, got) == (70, len(before), stop)
        assert not rf.forged_start_in_chain(run) and len(rf.candidates(run)) == 73  # whole candidates behind E
        stats = _check(run, gpu)
        assert stats[0] == 73 and stats[2] == 0


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_hostile_honest_runs(gpu, seed):
    """2,000 messages whose digests are newlines, 'F', digits, '+' and pieces
    of the tag, sizes in every accepted form.  Whether a digest forged a
    start is found by the Python scan, not assumed (seeds 0 and 2 do, 1 and
    3 do not)."""
    run = rf.hostile_run(2000, np.random.default_rng(seed))
    digests, sizes, consumed, stop = expected(run)
    assert (len(digests), consumed, stop) == (2000, len(run), END)
    want = rf.forged_start_in_chain(run)
    assert want == (len(rf.candidates(run)) > 2000)
    stats = _check(run, gpu)
    assert stats[0] == len(rf.candidates(run)) and stats[2] == int(want)
    stats = _check(run + b"FILE_END\n", gpu)
    assert stats[2] == int(want)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_run_lengths_at_the_kernels_edges(gpu, lead):
    """One honest run cut to n bytes, ending with its allocation: n around a
    lane's 16 positions, the 20 bytes of its dword path (16 + 4, one dword
    more when the run starts off a dword), a word's 64, and one and three
    candidates workgroups (4096 positions each)."""
    run, _, _ = _honest(400, seed=63)
    assert len(run) > 12288 + 20
    lengths = [1, 15, 16, 17, 19, 20, 21, 33, 34, 63, 64, 65]
    lengths += [base + r for base in (4096, 12288) for r in (-1, 0, 1, 19, 20)]
    for n in lengths:
        cut = run[:n]
        digests, _s, consumed, stop = expected(cut)
        assert stop in (INCOMPLETE, END) and n - consumed < 43
        stats = _check(cut, gpu, lead)
        assert stats[0] == len(digests) and stats[2] == 0, n


def test_block_set_receive_of_forged_and_hostile_runs(gpu):
    rng = np.random.default_rng(64)
    hostile = rf.hostile_run(2000, np.random.default_rng(0))
    forged = rf.honest_prefix(4096 - 20, rng) + rf.forge(9, 4)[0] + rf.honest_prefix(300, rng)
    assert rf.forged_start_in_chain(hostile) and rf.forged_start_in_chain(forged)
    base = 2 ** 40
    for run in (forged, hostile):
        want_d, want_s, want_c, _stop = expected(run + b"FILE_END\n")
        assert want_c == len(run)
        q = np.frombuffer(b"".join(want_d), np.uint8).reshape(-1, 20)
        table = np.concatenate([q[::3], rng.integers(0, 256, (500, 20), dtype=np.uint8), q[::7]])
        present = rng.random(table.shape[0]) < 0.7
        want_rows = oracle.block_lookup(table, present, q)
        assert (want_rows >= 0).any() and (want_rows < 0).any()
        with BlockSet(torch.from_numpy(table).to(gpu), torch.from_numpy(present).to(gpu)) as bset:
            d, s, offsets, rows, consumed, stop, end = bset.receive(_dev(run + b"FILE_END\n", gpu), base_offset=base)
            assert wire.parse_stats()[2] == 1
        assert (consumed, stop) == (want_c, OTHER)
        assert d.cpu().numpy().tobytes() == b"".join(want_d) and s.cpu().numpy().tolist() == want_s
        assert np.array_equal(rows.cpu().numpy(), want_rows)
        cum = np.cumsum(np.array([0] + want_s, dtype=object))
        assert offsets.cpu().numpy().tolist() == [base + int(c) for c in cum[:-1]]
        assert end == base + int(cum[-1])
