"""GPU: every device entry point writes its outputs and nothing else.

One scenario per device output (tests/placement.py is the harness): the
outputs of a call are carved from one arena full of a pattern, among guard
bytes, each with a few rows more than the call may write; after the call the
whole arena is compared with a host image -- the host reference's bytes in the
rows the call must write (oracle, hashlib, wire.Parser / write_message, the
host cutter), the pattern in every other byte: the rows past `cap` or past the
count, the guards, a status word the call does not own.  The inputs are
compared with their own copies.  Every scenario runs at three placements (all
outputs shifted at once, each to another phase of {0, A, 16 - A} past a
256-byte boundary, A the alignment include/syncfast_amd.h states for it) and
under two patterns.

The C-ABI is called directly: the Python wrappers allocate most outputs
themselves.  test_every_device_output_has_a_scenario (no GPU) holds the list
of scenarios against the header.

Measured on one MI355X: the whole file takes 3.1 s (477 tests; the slowest,
the first, 0.18 s).  Not committed, each run once against this file, each a
stray write of one row at the most, inside the arena:
  - `i > cap` for `i >= cap` in recv_extract_kernel: 42 tests fail, the cap
    n - 1 and cap 0 cases of both FILE_BLOCK parsers on the device route (with
    and without a set) and the forged run's cap 0 cases, where the kernel runs
    before the host fallback;
  - parse_on_host uploading out->count rows instead of `up`, run on the cap
    n - 1 cases only: the 24 host-route and forged-run tests fail;
  - `weak + first + 1` in launch_fixed's piece loop: the 6 tests of
    fixed_weak-bs64-n257-max48 fail (every piece after the first one entry
    late, the last entry past the table);
  - the alignment check of sf_test_table_order dropped:
    test_output_alignment_is_checked_without_device fails (test_wire.py).
"""
import ctypes
import functools
import hashlib
import os
import random
import re

import numpy as np
import pytest
import torch

import data_expect
import oracle
import placement
import recv_expect
import recv_forge as rf
from syncfast_amd import _lib, device, host, wire

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCENARIOS = {}  # name -> (the entry points it covers, run(gpu, arena, ph, knobs))


def scenario(name, *entries):
    def add(fn):
        assert name not in SCENARIOS, name
        SCENARIOS[name] = (entries, fn)
        return fn
    return add


def _bytes(seed, n) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _u8(b: bytes) -> np.ndarray:
    return np.frombuffer(b, np.uint8).copy()


def _dev(a, gpu) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _s(gpu) -> int:
    """The stream the arena was filled on."""
    return torch.cuda.current_stream(gpu).cuda_stream


def _u64():
    return ctypes.c_uint64(0)


L = _lib.lib
R = ctypes.byref
EXTRA = 3  # rows every table has beyond what its call may write


# ---------------------------------------------------------------- fixed tiling

@functools.lru_cache(None)
def _fixed_ref(bs, n):
    data = _bytes(1000 * bs + n, (n - 1) * bs + (37 if bs == 64 else 1000))  # the last block short
    return data, oracle.index_fixed(data, bs)[2], oracle.adler_fixed(data, bs)


def _fixed(bs, n, weak, max_blocks=0, short=False):
    def run(gpu, a, ph, knobs):
        data, dig, adl = _fixed_ref(bs, n)
        if max_blocks:  # pieces of 48 blocks: seams at digests + first * 20, weak + first
            knobs.set("SF_TEST_LAUNCH_MAX_BLOCKS", max_blocks)
        x = _dev(data, gpu)
        d = a.carve("digests", 20 * (n + EXTRA), U8, ph(0, 4))
        w = a.carve("weak", 4 * (n + EXTRA), I32, ph(1, 4)) if weak else None
        a.watch(data=x)
        nb, cap = _u64(), n - 1 if short else n + EXTRA
        if weak:
            rc = L().sf_index_device_fixed_weak(x.data_ptr(), x.numel(), bs, d.data_ptr(), w.data_ptr(), cap, R(nb),
                                                _s(gpu))
        else:
            rc = L().sf_index_device_fixed(x.data_ptr(), x.numel(), bs, d.data_ptr(), cap, R(nb), _s(gpu))
        assert nb.value == n
        if short:
            assert rc == _lib.SF_ENOSPC
            a.check({})
        else:
            assert rc == 0
            a.check({"digests": dig, "weak": adl} if weak else {"digests": dig})
    return run


for _weak in (False, True):
    _name = "fixed_weak" if _weak else "fixed"
    for _bs, _n, _kw in [(64, 65, {}), (64, 257, {}), (4096, 65, {}), (64, 257, {"max_blocks": 48}),
                         (64, 65, {"short": True})]:
        _tag = "".join(f"-{k}" if v is True else f"-max{v}" for k, v in _kw.items())
        scenario(f"{_name}-bs{_bs}-n{_n}{_tag}", f"sf_index_device_{_name}")(_fixed(_bs, _n, _weak, **_kw))


# -------------------------------------------------------------- explicit lists

N_LIST, LEN_LIST = 65, 5000  # 65 blocks: the sorted launch


@functools.lru_cache(None)
def _list_ref():
    """Blocks anywhere in the buffer (they overlap), two of them empty, two
    outside it; an out-of-range block's digest is zeroed and its weak sum 0."""
    rng = np.random.default_rng(77)
    data = _bytes(78, LEN_LIST)
    sizes = rng.integers(1, 300, N_LIST).astype(np.int32)
    offsets = rng.integers(0, LEN_LIST - 300, N_LIST).astype(np.int64)
    sizes[[5, 40]] = 0
    offsets[10] = offsets[9] + 1
    offsets[20], sizes[20] = LEN_LIST - 10, 11
    offsets[64], sizes[64] = 1 << 40, 5
    bad = offsets + sizes > LEN_LIST
    assert bad.sum() == 2
    o, z = np.where(bad, 0, offsets), np.where(bad, 0, sizes)
    dig, adl = oracle.index_blocks(data, o, z), oracle.adler_blocks(data, o, z)
    dig[bad], adl[bad] = 0, 0
    return data, offsets, sizes, dig, adl


def _blocks(weak, sort):
    def run(gpu, a, ph, knobs):
        data, offsets, sizes, dig, adl = _list_ref()
        if sort is not None:
            knobs.set("SF_TEST_TABLE_SORT", sort)
        x, o, z = _dev(data, gpu), _dev(offsets, gpu), _dev(sizes, gpu)
        d = a.carve("digests", 20 * (N_LIST + EXTRA), U8, ph(0, 4))
        w = a.carve("weak", 4 * (N_LIST + EXTRA), I32, ph(1, 4)) if weak else None
        status = a.carve("status", 4, I32, ph(2, 4))
        status.zero_()  # the caller initialises it
        a.watch(data=x, offsets=o, sizes=z)
        if weak:
            rc = L().sf_index_device_blocks_weak(x.data_ptr(), LEN_LIST, o.data_ptr(), z.data_ptr(), N_LIST,
                                                 d.data_ptr(), w.data_ptr(), status.data_ptr(), _s(gpu))
        else:
            rc = L().sf_index_device_blocks(x.data_ptr(), LEN_LIST, o.data_ptr(), z.data_ptr(), N_LIST, d.data_ptr(),
                                            status.data_ptr(), _s(gpu))
        assert rc == 0
        want = {"digests": dig, "status": np.array([_lib.SF_ERANGE], np.int32)}
        if weak:
            want["weak"] = adl
        a.check(want)
    return run


for _weak in (False, True):
    _name = "blocks_weak" if _weak else "blocks"
    scenario(f"{_name}-sorted", f"sf_index_device_{_name}")(_blocks(_weak, None))
    scenario(f"{_name}-sort0", f"sf_index_device_{_name}")(_blocks(_weak, 0))


# ------------------------------------------------------------ many-file batches

BS_BATCH = 64
BATCHES = {  # files (offset, length) inside one buffer
    "3x128": [(i * 128 * 64, 128 * 64) for i in range(3)],  # the column halves
    "3x8": [(i * 8 * 64, 8 * 64) for i in range(3)],        # blocks, then the chain helper waves
    "3x6": [(i * 6 * 64, 6 * 64) for i in range(3)],        # nbf % 4 != 0: the per-lane chain kernel
    "aligned-unequal": [(0, 5 * 64), (5 * 64, 9 * 64), (14 * 64, 2 * 64)],  # fixed blocks, the table chain
    "ragged": [(3, 1), (9, 64), (78, 0), (83, 65), (153, 300)],
    "empty": [(0, 0), (5, 0), (16, 0)],  # total == 0: hashes of the empty string
}


@functools.lru_cache(None)
def _batch_ref(kind):
    files = BATCHES[kind]
    data = _bytes(len(kind) + 200, max(16, max(o + n for o, n in files)))
    digs = [oracle.index_fixed(data[o:o + n], BS_BATCH)[2] for o, n in files]
    first = np.concatenate([[0], np.cumsum([d.shape[0] for d in digs])]).astype(np.uint64)
    hashes = np.stack([np.frombuffer(oracle.blocks_hash(d), np.uint8) for d in digs])
    return data, np.concatenate(digs), first, hashes


def _batch(kind, fused=None):
    def run(gpu, a, ph, knobs):
        data, dig, first, hashes = _batch_ref(kind)
        files = BATCHES[kind]
        if fused is not None:
            knobs.set("SF_BATCH_FUSED", fused)
        total, nf = dig.shape[0], len(files)
        x = _dev(data, gpu)
        d = a.carve("digests", 20 * (total + EXTRA), U8, ph(0, 4))
        fh = a.carve("file_hashes", 20 * (nf + EXTRA), U8, ph(1, 4))
        status = a.carve("status", 4, I32, ph(2, 4))  # passed in, never written
        a.watch(data=x)
        descs = (_lib.FileDesc * nf)(*[_lib.FileDesc(o, n) for o, n in files])
        got_first, nb = np.zeros(nf + 1, np.uint64), _u64()
        rc = L().sf_index_device_batch(x.data_ptr(), x.numel(), descs, nf, BS_BATCH, d.data_ptr(), total + EXTRA,
                                       fh.data_ptr(), got_first.ctypes.data, R(nb), status.data_ptr(), _s(gpu))
        assert rc == 0 and nb.value == total and np.array_equal(got_first, first)
        a.check({"digests": dig, "file_hashes": hashes})
    return run


for _kind in BATCHES:
    scenario(f"batch-{_kind}", "sf_index_device_batch")(_batch(_kind))
scenario("batch-3x128-fused0", "sf_index_device_batch")(_batch("3x128", 0))


# ------------------------------------------------------------------ the block set

N_ROWS, N_QUERIES = 100, 130


@functools.lru_cache(None)
def _set_ref():
    rng = np.random.default_rng(90)
    table = rng.integers(0, 256, (N_ROWS, 20), dtype=np.uint8)
    table[rng.integers(0, N_ROWS, 20)] = table[rng.integers(0, N_ROWS, 20)]  # repeated digests
    present = (rng.random(N_ROWS) < 0.7).astype(np.uint8)
    queries = table[rng.integers(0, N_ROWS, N_QUERIES)].copy()
    miss = rng.random(N_QUERIES) < 0.33
    queries[miss] = rng.integers(0, 256, (int(miss.sum()), 20), dtype=np.uint8)
    return table, present, queries, oracle.block_lookup(table, present, queries)


@scenario("block_set_lookup", "sf_block_set_lookup")
def _lookup(gpu, a, ph, knobs):
    table, present, queries, want = _set_ref()
    t, p, q = _dev(table, gpu), _dev(present, gpu), _dev(queries, gpu)
    rows = a.carve("rows", 8 * (N_QUERIES + EXTRA), I64, ph(0, 8))  # the rows beyond n_query stay
    a.watch(table=t, present=p, queries=q)
    with device.BlockSet(t, p) as bs:
        assert L().sf_block_set_lookup(bs._h, q.data_ptr(), N_QUERIES, rows.data_ptr(), _s(gpu)) == 0
        a.check({"rows": want})


# ------------------------------------------------------------- the wire builders

N_WIRE, BS_WIRE = 70, 4096
FILE_LEN_WIRE = (N_WIRE - 1) * BS_WIRE + 77


@functools.lru_cache(None)
def _wire_ref(fixed):
    rng = np.random.default_rng(40 + fixed)
    digests = rng.integers(0, 256, (N_WIRE, 20), dtype=np.uint8)
    if fixed:
        sizes = np.array([BS_WIRE] * (N_WIRE - 1) + [77], np.uint32)
    else:  # size fields of 1 to 10 digits
        sizes = np.array([int(rng.integers(10 ** (i % 10) if i % 10 else 0, min(10 ** (i % 10 + 1), 1 << 32)))
                          for i in range(N_WIRE)], np.uint32)
    run = b"".join(wire.write_message("FileBlock", digests[i].tobytes(), int(sizes[i])) for i in range(N_WIRE))
    return digests, sizes, run


def _wire(fixed, short):
    def run(gpu, a, ph, knobs):
        digests, sizes, want = _wire_ref(fixed)
        need = len(want)
        d, z = _dev(digests, gpu), _dev(sizes.view(np.int32), gpu)
        out = a.carve("out", need + 7, U8, ph(0, 1))
        a.watch(digests=d, sizes=z)
        n_out, cap = _u64(), need - 1 if short else need + 7
        if fixed:
            rc = L().sf_wire_file_blocks_device(d.data_ptr(), N_WIRE, BS_WIRE, FILE_LEN_WIRE, out.data_ptr(), cap,
                                                R(n_out), _s(gpu))
        else:
            rc = L().sf_wire_blocks_device(d.data_ptr(), z.data_ptr(), N_WIRE, out.data_ptr(), cap, R(n_out), _s(gpu))
        assert n_out.value == need
        if short:
            assert rc == _lib.SF_ENOSPC
            a.check({})
        else:
            assert rc == 0
            a.check({"out": want})  # the 7 bytes after the run stay
    return run


for _fixed_form in (True, False):
    _name = "sf_wire_file_blocks_device" if _fixed_form else "sf_wire_blocks_device"
    scenario(f"{_name[3:]}-cap+7", _name)(_wire(_fixed_form, False))
    scenario(f"{_name[3:]}-cap-1", _name)(_wire(_fixed_form, True))


# -------------------------------------------------------------- FILE_BLOCK runs

N_MSG = 70
BASE_OFFSET = 1 << 33


def _honest(rng, digits, digests=None):
    out = []
    for i, d in enumerate(digits):
        size = int(rng.integers(10 ** (d - 1) if d > 1 else 0, min(10 ** d, 1 << 32)))
        digest = digests[i].tobytes() if digests is not None else rng.integers(0, 256, 20, dtype=np.uint8).tobytes()
        out.append(recv_expect.message(digest, size))
    return b"".join(out)


@functools.lru_cache(None)
def _run_ref(forged):
    """70 messages + FILE_END; the destination's table holds some of their
    digests.  The forged run has recv_forge's pair (A's digest holds a message
    start) in the middle: the device hands it to the host parser."""
    rng = np.random.default_rng(80 + forged)
    table, present, queries, _rows = _set_ref()
    digits = [i % 10 + 1 for i in range(N_MSG)]
    if forged:
        pair, _p, _family = rf.forge(2, 1)
        run = _honest(rng, digits[:30], queries) + pair + _honest(rng, digits[32:], queries[32:])
    else:
        run = _honest(rng, digits, queries)
    run += b"FILE_END\n"
    assert rf.forged_start_in_chain(run) == bool(forged)
    digests, sizes, consumed, stop = recv_expect.expected(run)
    assert len(digests) == N_MSG and stop == recv_expect.OTHER
    digests, sizes = _u8(b"".join(digests)).reshape(-1, 20), np.array(sizes, np.uint32)
    ends = BASE_OFFSET + np.cumsum(sizes.astype(np.uint64))
    offsets = np.concatenate([[BASE_OFFSET], ends[:-1]]).astype(np.uint64)
    return run, digests, sizes, offsets, oracle.block_lookup(table, present, digests), consumed, stop, int(ends[-1])


CAPS = {"cap+3": N_MSG + 3, "cap=n": N_MSG, "cap-1": N_MSG - 1, "cap0": 0}
ROUTES = ("device", "host", "forged")  # the chain on the device; SF_TEST_WIRE_PARSE_HOST; the fallback


def _parse(receive, route, cap, with_set=True):
    def run(gpu, a, ph, knobs):
        wire_run, digests, sizes, offsets, rows, consumed, stop, end = _run_ref(route == "forged")
        if route == "host":
            knobs.set("SF_TEST_WIRE_PARSE_HOST", 1)
        x = _dev(_u8(wire_run), gpu)
        d = a.carve("digests", 20 * (N_MSG + EXTRA), U8, ph(0, 4))
        z = a.carve("sizes", 4 * (N_MSG + EXTRA), I32, ph(1, 4))
        a.watch(run=x)
        n, used, why, last = _u64(), _u64(), ctypes.c_int(-1), _u64()
        k = min(N_MSG, cap)
        want = {"digests": digests[:k], "sizes": sizes[:k]}
        if not receive:
            rc = L().sf_wire_parse_blocks_device(x.data_ptr(), x.numel(), d.data_ptr(), z.data_ptr(), cap, R(n), R(used),
                                                 R(why), _s(gpu))
        else:
            o = a.carve("offsets", 8 * (N_MSG + EXTRA), I64, ph(2, 8))
            r = a.carve("rows", 8 * (N_MSG + EXTRA), I64, ph(3, 8))
            table, present, _q, _r = _set_ref()
            t, p = _dev(table, gpu), _dev(present, gpu)
            a.watch(table=t, present=p)
            bs = device.BlockSet(t, p) if with_set else None
            rc = L().sf_receive_blocks_device(bs._h if bs else None, x.data_ptr(), x.numel(), BASE_OFFSET, d.data_ptr(),
                                              z.data_ptr(), o.data_ptr(), r.data_ptr(), cap, R(n), R(used), R(why),
                                              R(last), _s(gpu))
            if cap >= N_MSG:  # with SF_ENOSPC the offsets and the rows are untouched
                assert last.value == end
                want["offsets"] = offsets
                if with_set:  # without a set d_rows is untouched
                    want["rows"] = rows
        assert rc == (0 if cap >= N_MSG else _lib.SF_ENOSPC)
        assert (n.value, used.value, why.value) == (N_MSG, consumed, stop)
        assert wire.parse_stats()[2] == int(route != "device")
        a.check(want)
        if receive and bs:
            bs.close()
    return run


for _receive in (False, True):
    _name = "sf_receive_blocks_device" if _receive else "sf_wire_parse_blocks_device"
    for _route in ROUTES:
        for _cap_name, _cap in CAPS.items():
            scenario(f"{_name[3:]}-{_route}-{_cap_name}", _name)(_parse(_receive, _route, _cap))
for _cap_name in ("cap+3", "cap-1"):
    scenario(f"receive_blocks_device-noset-{_cap_name}", "sf_receive_blocks_device")(
        _parse(True, "device", CAPS[_cap_name], with_set=False))


# -------------------------------------------------------------- BLOCK_DATA runs

N_DATA, CORRUPT = 20, 7
DATA_CAPS = {"cap+3": N_DATA + 3, "cap=n": N_DATA, "cap-1": N_DATA - 1, "cap0": 0}


@functools.lru_cache(None)
def _data_ref():
    rng = random.Random(11)
    lengths = [0, 1, 55, 56, 64, 300, 119, 120, 299, 17] * 2  # payloads of 0 to 300 bytes
    run = b"".join(data_expect.message(rng.randbytes(n)) for n in lengths)
    at = data_expect.expected(run)[2][CORRUPT] + 60  # inside message 7's 120-byte payload
    run = run[:at] + bytes([run[at] ^ 0x10]) + run[at + 1:]
    assert not data_expect.needs_walk(run)
    digests, sizes, offsets, consumed, stop, need = data_expect.expected(run)
    assert len(digests) == N_DATA
    ok = np.array([hashlib.sha1(run[o:o + n]).digest() == d for d, n, o in zip(digests, sizes, offsets)], np.uint8)
    assert ok.tolist() == [int(i != CORRUPT) for i in range(N_DATA)]
    return (run, _u8(b"".join(digests)).reshape(-1, 20), np.array(sizes, np.uint32), np.array(offsets, np.uint64), ok,
            consumed, stop, need)


def _block_data(cap, verify, walk):
    def run(gpu, a, ph, knobs):
        wire_run, digests, sizes, offsets, ok, consumed, stop, need = _data_ref()
        knobs.set("SF_TEST_BLOCK_DATA_WALK", walk)
        x = _dev(_u8(wire_run), gpu)
        d = a.carve("digests", 20 * (N_DATA + EXTRA), U8, ph(0, 4))
        z = a.carve("sizes", 4 * (N_DATA + EXTRA), I32, ph(1, 4))
        o = a.carve("data_offsets", 8 * (N_DATA + EXTRA), I64, ph(2, 8))
        good = a.carve("ok", N_DATA + EXTRA, U8, ph(3, 1))
        a.watch(run=x)
        n, used, why, more, bad = _u64(), _u64(), ctypes.c_int(-1), _u64(), _u64()
        rc = L().sf_receive_block_data_device(x.data_ptr(), x.numel(), d.data_ptr(), z.data_ptr(), o.data_ptr(),
                                              good.data_ptr() if verify else None, cap, R(n), R(used), R(why),
                                              R(more), R(bad), _s(gpu))
        assert rc == (0 if cap >= N_DATA else _lib.SF_ENOSPC)
        assert (n.value, used.value, why.value, more.value) == (N_DATA, consumed, stop, need)
        assert wire.block_data_stats()[2] == walk
        k = min(N_DATA, cap)  # past cap nothing is written; with SF_ENOSPC nothing is hashed
        want = {"digests": digests[:k], "sizes": sizes[:k], "data_offsets": offsets[:k]}
        if verify and cap >= N_DATA:
            assert bad.value == 1
            want["ok"] = ok
        else:
            assert bad.value == 0
        a.check(want)
    return run


for _cap_name, _cap in DATA_CAPS.items():
    for _verify in (True, False):
        for _walk in (0, 1):
            scenario(f"receive_block_data_device-{_cap_name}-{'ok' if _verify else 'parse'}-walk{_walk}",
                     "sf_receive_block_data_device")(_block_data(_cap, _verify, _walk))


# ------------------------------------------------------------------ the ZPAQ cut

LEN_ZPAQ, BITS, MAX_SIZE = 20_000, 6, 256


@functools.lru_cache(None)
def _zpaq_ref():
    data = _bytes(9, LEN_ZPAQ)
    offs, sizes = host.zpaq_cut_buffer(data, BITS, MAX_SIZE)
    raw = data.tobytes()
    digs = [hashlib.sha1(raw[o:o + n]).digest() for o, n in zip(offs.tolist(), sizes.tolist())]
    assert len(digs) > 64
    return (data, offs.astype(np.uint64), sizes.astype(np.uint32), _u8(b"".join(digs)).reshape(-1, 20),
            hashlib.sha1(b"".join(digs)).digest())


def _zpaq(index, delta):
    def run(gpu, a, ph, knobs):
        data, offs, sizes, digs, chain = _zpaq_ref()
        n = offs.size
        cap = n + delta
        x = _dev(data, gpu)
        o = a.carve("offsets", 8 * (n + EXTRA), I64, ph(0, 8))
        z = a.carve("sizes", 4 * (n + EXTRA), I32, ph(1, 4))
        d = a.carve("digests", 20 * (n + EXTRA), U8, ph(2, 4)) if index else None
        a.watch(data=x)
        nb, bh = _u64(), (ctypes.c_uint8 * 20)()
        if index:
            rc = L().sf_index_device_zpaq(x.data_ptr(), LEN_ZPAQ, BITS, MAX_SIZE, o.data_ptr(), z.data_ptr(),
                                          d.data_ptr(), cap, R(nb), bh, _s(gpu))
        else:
            rc = L().sf_cut_device_zpaq(x.data_ptr(), LEN_ZPAQ, BITS, MAX_SIZE, o.data_ptr(), z.data_ptr(), cap, R(nb),
                                        _s(gpu))
        assert nb.value == n
        if delta < 0:  # nothing written, the digests included
            assert rc == _lib.SF_ENOSPC
            a.check({})
            return
        assert rc == 0
        want = {"offsets": offs, "sizes": sizes}
        if index:
            assert bytes(bh) == chain
            want["digests"] = digs
        a.check(want)
    return run


for _index in (False, True):
    _name = "sf_index_device_zpaq" if _index else "sf_cut_device_zpaq"
    for _delta, _tag in ((EXTRA, "cap+3"), (0, "cap=n"), (-1, "cap-1")):
        scenario(f"{_name[3:]}-{_tag}", _name)(_zpaq(_index, _delta))


# ------------------------------------------------- the explicit list's sort order

N_ORDER = 2049


@functools.lru_cache(None)
def _order_ref():
    from test_gpu_table_order import _class_keys  # numpy restatement of length_class
    rng = np.random.default_rng(38)
    sizes = np.concatenate([rng.geometric(1 / 8192, N_ORDER // 2), rng.integers(0, 1 << 31, N_ORDER - N_ORDER // 2)])
    sizes = rng.permutation(np.minimum(sizes, (1 << 31) - 1)).astype(np.uint32)
    want = np.argsort((255 - _class_keys(sizes)).astype(np.uint8), kind="stable")  # descending, stable
    return sizes, want.astype(np.uint32)


@scenario("test_table_order", "sf_test_table_order")
def _order(gpu, a, ph, knobs):
    sizes, want = _order_ref()
    z = _dev(sizes.view(np.int32), gpu)
    order = a.carve("order", 4 * (N_ORDER + EXTRA), I32, ph(0, 4))
    a.watch(sizes=z)
    assert L().sf_test_table_order(z.data_ptr(), N_ORDER, order.data_ptr(), _s(gpu)) == 0
    a.check({"order": want})


# ----------------------------------------------------------------- the block copy

@scenario("copy_blocks-status", "sf_copy_blocks_device")
def _copy_status(gpu, a, ph, knobs):
    """Only the status word is carved here, among guards: the destination has
    guards of its own in test_gpu_copy_blocks.py."""
    src = _bytes(5, 1000)
    jobs = [(0, 10, 100), (500, 2000, 8), (900, 300, 100)]  # (source, destination, size); the second is out of range
    s, dst = _dev(src, gpu), torch.full((1000,), 0xEE, dtype=U8, device=gpu)
    so, do, sz = (_dev(np.array([j[k] for j in jobs], t), gpu) for k, t in enumerate((np.int64, np.int64, np.int32)))
    status = a.carve("status", 4, I32, ph(0, 4))
    status.zero_()
    a.watch(src=s, src_offsets=so, dst_offsets=do, sizes=sz)
    assert L().sf_copy_blocks_device(s.data_ptr(), 1000, dst.data_ptr(), 1000, so.data_ptr(), do.data_ptr(),
                                     sz.data_ptr(), None, 3, status.data_ptr(), _s(gpu)) == 0
    a.check({"status": np.array([_lib.SF_ERANGE], np.int32)})
    want = np.full(1000, 0xEE, np.uint8)
    want[10:110], want[300:400] = src[0:100], src[900:1000]
    assert np.array_equal(dst.cpu().numpy(), want)


# ------------------------------------------------------------------ the generator

def _fill(length, start):
    def run(gpu, a, ph, knobs):
        out = a.carve("out", length + 7, U8, ph(0, 1))
        assert L().sf_fill_splitmix_device(out.data_ptr(), length, 0x5EED, start, _s(gpu)) == 0
        a.check({"out": oracle.splitmix_bytes(length, 0x5EED, start)})
    return run


for _length, _start in ((1005, 16), (1005, 3), (15, 0)):
    scenario(f"fill_splitmix-{_length}-start{_start}", "sf_fill_splitmix_device")(_fill(_length, _start))


# ------------------------------------------------------------------- the runs

@pytest.mark.gpu
@pytest.mark.parametrize("pattern", placement.PATTERNS, ids=lambda p: f"{p:#04x}")
@pytest.mark.parametrize("place", range(3))
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_outputs_and_nothing_else(gpu, knobs, name, place, pattern):
    arena = placement.Arena(gpu, pattern)
    SCENARIOS[name][1](gpu, arena, lambda j, align: placement.phase(place, j, align), knobs)


@pytest.mark.gpu
def test_the_arena_reports_a_stray_byte(gpu):
    """The harness itself: one byte past an output's written rows, one in a
    guard and a modified input are each reported, and named."""
    for spoil, told in (("row", "digests + 40"), ("guard", "guard between digests and weak"), ("input", "input data")):
        a = placement.Arena(gpu, 0xA5)
        d = a.carve("digests", 60, U8, 4)
        w = a.carve("weak", 12, I32, 12)
        x = torch.zeros(8, dtype=U8, device=gpu)
        a.watch(data=x)
        d[:40] = 1
        w[:] = 7
        if spoil == "row":
            d[40] = 0xA4
        elif spoil == "guard":
            a.buf[a.carved[1][1] - 1] = 0
        else:
            x[3] = 1
        with pytest.raises(AssertionError, match=re.escape(told)):
            a.check({"digests": np.ones(40, np.uint8), "weak": np.full(3, 7, np.int32)})


@pytest.mark.gpu
def test_the_wrappers_refuse_an_output_at_an_odd_address(gpu):
    data = device.splitmix_tensor(64 * 5, 1, gpu)
    raw = torch.empty(20 * 5 + 8, dtype=U8, device=gpu)
    for off in (1, 2, 3):
        with pytest.raises(ValueError, match="4-byte aligned"):
            device.index_device(data, 64, out=raw[off:off + 100])
        with pytest.raises(ValueError, match="4-byte aligned"):
            device.index_device_batch(data, [(0, 320)], 64, hashes_out=raw[off:off + 20])
    want = oracle.index_fixed(data.cpu().numpy(), 64)[2]
    assert np.array_equal(device.index_device(data, 64, out=raw[4:104]).cpu().numpy().reshape(-1, 20), want)


# ------------------------------------------------------- the list is complete

# Entry points with a device output that have no scenario here, and why.
EXEMPT = {
    "sf_index_device_multi": "several GPUs: tests/test_gpu_multi.py",
    "sf_index_device_multi_ex": "several GPUs: tests/test_gpu_multi.py",
    "sf_index_device_batch_chained": "under guard rows in tests/test_gpu_chain_jobs.py",
    "sf_index_device_batch_chained_cols": "under guard rows in tests/test_gpu_chain_jobs.py",
}


def device_output_functions(header: str):
    """{function: [its non-const pointer parameters named d_*]} of a header."""
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(sf_\w+)\s*\(([^()]*)\)\s*;", text):
        outs = []
        for p in params.split(","):
            m = re.fullmatch(r"\s*([\w\s]+?)\s*\*\s*(d_\w+)\s*", p)
            if m and "const" not in m.group(1).split():
                outs.append(m.group(2))
        if outs:
            out[name] = outs
    return out


def test_every_device_output_has_a_scenario():
    with open(os.path.join(ROOT, "include", "syncfast_amd.h")) as f:
        found = device_output_functions(f.read())
    # the parse sees what it should: a few known answers
    assert found["sf_index_device_blocks_weak"] == ["d_digests", "d_weak", "d_status"]
    assert found["sf_receive_block_data_device"] == ["d_digests", "d_sizes", "d_data_offsets", "d_ok"]
    assert found["sf_index_device_multi"] == ["d_table"]
    assert "sf_block_set_build" not in found and "sf_write_device_fd" not in found
    covered = {e for entries, _fn in SCENARIOS.values() for e in entries}
    assert not covered & set(EXEMPT)
    missing = set(found) - covered - set(EXEMPT)
    assert not missing, f"device outputs with no written-extent scenario: {sorted(missing)}"
    assert set(EXEMPT) <= set(found), "an exemption for a function the header does not declare"
    assert len(EXEMPT) <= 4 and all(EXEMPT.values())
    assert "sf_test_table_order" in covered  # include/syncfast_amd_test.h: the one test hook with a device output
