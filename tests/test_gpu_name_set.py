"""GPU: the name set (sf_name_set_build / _lookup / _free, device.NameSet)
against a dict model -- the lowest present row whose name has the query's
length and bytes, or -1 -- and against Index.get_file on an index that holds a
name twice.  Shapes are the smallest that reach each path: 0, 1 and 3,000 rows;
names of 0, 1, 3, 4, 5, 100, 101 and 300 bytes; a prefix of another name, names
that differ in the last byte or by a trailing 0 byte; duplicates under every
`present` pattern; the whole set with every name in two probe sequences and in
one (SF_TEST_NAME_HASH_MASK); query spans at every address phase and at the
buffer's last byte; a broken CSR."""
import ctypes
import itertools
from pathlib import PurePath

import numpy as np
import pytest
import torch

from file_list_cases import H, put
from syncfast_amd import _lib, device
from syncfast_amd.index import Index

pytestmark = pytest.mark.gpu


def model(names, present, queries):
    first = {}
    for r, n in enumerate(names):
        if present is None or present[r]:
            first.setdefault(n, r)
    return [first.get(q, -1) for q in queries]


def special_names():
    n = [b"", b"a", b"abc", b"abcd", b"abcde", b"n" * 100, b"n" * 101, b"n" * 300, b"n" * 99,  # the lengths
         b"dir/file", b"dir/fil", b"dir/file2",             # one a prefix of another
         b"x" * 40 + b"1", b"x" * 40 + b"2",                # the last byte only
         b"zero", b"zero\0", b"zero\0\0", b"\0", b"\0\0",   # a trailing 0 byte
         b"dir/\xc3\xa9", b"dir/\xc3\xa8", b"new\nline", b"\xff\xfe"]
    assert len(set(n)) == len(n)
    return n


def many_names(k, seed=3):
    rng = np.random.default_rng(seed)
    out = [b"d%d/f%05d.%s" % (i % 37, i, bytes(rng.integers(97, 123, int(rng.integers(0, 30)), dtype=np.uint8)))
           for i in range(k)]
    for i in range(0, k, 50):  # repeated names, rows apart
        out[(i * 7 + 11) % k] = out[i]
    return out


def queries_for(names):
    rng = np.random.default_rng(9)
    q = list(names) + [n + b"x" for n in names[:40]] + [n[:-1] for n in names[:40] if n] + [b"", b"absent"]
    return [q[i] for i in rng.permutation(len(q))]


@pytest.mark.parametrize("mask", [0, 1, -(1 << 63)], ids=["mask0", "two_sequences", "one_slot"])  # bit 63 alone
def test_lookup_is_the_dict_model(gpu, knobs, mask):
    knobs.set("SF_TEST_NAME_HASH_MASK", mask)
    names = special_names() + many_names(3000 - len(special_names()))
    assert len(names) == 3000
    rng = np.random.default_rng(4)
    present = (rng.random(len(names)) < 0.8).astype(np.uint8)
    queries = queries_for(names)
    want = model(names, present, queries)
    assert sum(w >= 0 for w in want) > 2000 and sum(w < 0 for w in want) > 80
    with device.NameSet.build(names, present, gpu) as ns:
        knobs.set("SF_TEST_NAME_HASH_MASK", 0)  # the set keeps the mask it was built with
        assert ns.lookup_names(queries).cpu().tolist() == want
    with device.NameSet.build(names, None, gpu) as ns:  # no flags: every row is present
        assert ns.lookup_names(queries).cpu().tolist() == model(names, None, queries)


@pytest.mark.parametrize("rows", [0, 1])
def test_tiny_sets(gpu, rows):
    names = [b"only"][:rows]
    with device.NameSet.build(names, None, gpu) as ns:
        assert ns.lookup_names([b"only", b"", b"onl", b"only\0"]).cpu().tolist() == [0 if rows else -1, -1, -1, -1]
        assert ns.lookup_names([]).numel() == 0
    with device.NameSet.build(names, [0] * rows, gpu) as ns:
        assert ns.lookup_names([b"only"]).cpu().tolist() == [-1]


def test_duplicates_under_every_present_pattern(gpu, knobs):
    """Four rows of one name among others: the lowest present one answers,
    with the rows spread over the table and all in one probe sequence."""
    names = [b"a", b"dup", b"b", b"dup", b"dup", b"c", b"dup"]
    dups = [1, 3, 4, 6]
    for mask in (0, -(1 << 63)):
        knobs.set("SF_TEST_NAME_HASH_MASK", mask)
        for flags in itertools.product((0, 1), repeat=4):
            present = np.ones(len(names), np.uint8)
            present[dups] = flags
            with device.NameSet.build(names, present, gpu) as ns:
                got = ns.lookup_names([b"dup", b"a", b"c", b"du"]).cpu().tolist()
            assert got == [next((r for r, f in zip(dups, flags) if f), -1), 0, 5, -1], (mask, flags)


def test_query_spans_at_every_phase_and_at_the_last_byte(gpu):
    names = [b"abcde", b"e", b"bcd", b""]
    with device.NameSet.build(names, None, gpu) as ns:
        raw = torch.empty(64 + 16, dtype=torch.uint8, device=gpu)
        for phase in range(8):
            lead = (phase - raw.data_ptr()) % 8
            data = raw[lead:lead + 13]
            data.copy_(torch.frombuffer(bytearray(b"xxabcdexbcdxe"), dtype=torch.uint8))
            assert data.data_ptr() % 8 == phase
            at = torch.tensor([2, 3, 6, 12, 13, 8, 0, 12, 13, 14, 1 << 62], dtype=torch.int64, device=gpu)
            lens = torch.tensor([5, 3, 1, 1, 0, 3, 0, 2, 1, 0, 5], dtype=torch.int32, device=gpu)
            # the last three leave the buffer: not read, -1; the span of the last byte and the empty span at the end hold
            assert ns.lookup(data, at, lens).cpu().tolist() == [0, 2, 1, 1, 3, 2, 3, -1, -1, -1, -1], phase


def test_a_broken_csr_is_refused_with_its_row(gpu):
    names, at = device.pack_names([b"aa", b"bbb", b"c", b"dddd"], gpu)
    # at = 0 2 5 6 10: a first entry that is not 0, an entry above its successor, one above the last one (twice)
    for change, row in (({0: 1}, 0), ({2: 1}, 1), ({3: 99}, 2), ({4: 5}, 2), ({1: 7, 2: 6}, 1)):
        bad_at = at.clone()
        for k, v in change.items():
            bad_at[k] = v
        with pytest.raises(ValueError, match=f"row {row}:"):
            device.NameSet(names, bad_at)
    h, bad = ctypes.c_void_p(5), ctypes.c_uint64(0)
    bad_at = at.clone()
    bad_at[2] = 1
    s = torch.cuda.current_stream(gpu).cuda_stream
    rc = _lib.lib().sf_name_set_build(names.data_ptr(), bad_at.data_ptr(), None, 4, ctypes.byref(h), ctypes.byref(bad), s)
    assert (rc, h.value, bad.value) == (_lib.SF_EINVAL, None, 1)
    with device.NameSet(names, at) as ns:  # the good one still builds
        assert ns.lookup_names([b"c", b"bbb"]).cpu().tolist() == [2, 1]


def test_lookup_is_get_file_on_an_index_with_a_repeated_name(gpu):
    idx = Index.open_in_memory()
    for k, (name, temporary) in enumerate([("a", 0), ("twice", 1), ("b", 0), ("twice", 0), ("twice", 0), ("t", 1),
                                           ("dir/é", 0)]):
        put(idx, name, H(k), temporary=temporary)
    rows = idx.db.execute("SELECT file_id, name, temporary FROM files ORDER BY file_id;").fetchall()
    with device.NameSet.build([r[1].encode() for r in rows], [not r[2] for r in rows], gpu) as ns:
        asked = ["a", "twice", "b", "t", "dir/é", "absent", "twic"]
        got = ns.lookup_names([n.encode() for n in asked]).cpu().tolist()
    for name, row in zip(asked, got):
        found = idx.get_file(PurePath(name))
        assert (found[0] if found else None) == (rows[row][0] if row >= 0 else None), name
    assert got == [0, 3, 2, -1, 6, -1, -1]
