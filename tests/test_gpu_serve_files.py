"""GPU: a received GET_FILE run parsed and answered on the device --
sf_wire_parse_get_files_device against get_files_expect (wire.Parser alone),
sf_serve_get_files_device byte for byte against wire.write_message over the
reference's Respond loop and against Index.serve_get_files, the exchange end
to end over two indices, and each blocking call once behind a hold on a fresh
stream (tests/stream_order.py).

Shapes are the smallest that reach each path: runs of 3 to 257 requests, one of
3,000; a source of 13 rows and 0 to 70 blocks per file, sets of 63 to 3,000
messages.  The fixed table and the plan table are test_wire_get_files.py's,
which the rules header passes on the CPU; here the kernels that call the same
rules must give the same answers."""
import ctypes
import random
from pathlib import PurePath

import numpy as np
import pytest
import torch

import oracle
import stream_order as so
from entries_expect import END_FILES, get_file, get_files_run
from file_list_cases import H, destination, put
from get_files_expect import (ALL, BAD_NAME, END, FULL, INCOMPLETE, THREE, UNKNOWN, csr, expected, plan_cases,
                              plan_source, served, table)
from placement import PATTERNS, Arena
from send_files_expect import files_with_messages, parse_back
from syncfast_amd import _lib, device, wire
from syncfast_amd.digest import HashDigest
from syncfast_amd.index import Index

pytestmark = pytest.mark.gpu

READBACKS = 3  # include/syncfast_amd.h, DESIGN.md 3.16: whatever the number of requests


def _dev(b: bytes, gpu):
    return device.upload(b, gpu)


# ------------------------------------------------------------------- the parse

def _hold(got, stream: bytes, what=None):
    """One result of wire.parse_get_files_device against the model."""
    name_at, name_len, bad_name, consumed, stop = got
    e = expected(stream)
    assert (consumed, stop, bad_name) == (e.consumed, e.stop, e.bad_name), what
    assert name_at.cpu().tolist() == e.name_at and name_len.cpu().tolist() == e.name_len, what
    assert name_at.dtype == torch.int64 and name_len.dtype == torch.int32
    return e


def test_fixed_table(gpu):
    stops = set()
    for name, stream in table():
        stops.add(_hold(wire.parse_get_files_device(_dev(stream, gpu)), stream, name).stop)
    assert stops == {0, 1, 2, 3}


def test_a_run_cut_at_every_byte_and_continued(gpu):
    e = expected(THREE)
    assert len(THREE) < 64
    for cut in range(len(THREE) + 1):
        first = wire.parse_get_files_device(_dev(THREE[:cut], gpu))
        _hold(first, THREE[:cut], cut)
        assert first[4] in (END, INCOMPLETE)
        rest = THREE[first[3]:]
        second = wire.parse_get_files_device(_dev(rest, gpu))
        _hold(second, rest, cut)
        assert second[4] == END and first[3] + second[3] == len(THREE)
        names = [THREE[a:a + n] for a, n in zip(first[0].tolist(), first[1].tolist())]
        names += [rest[a:a + n] for a, n in zip(second[0].tolist(), second[1].tolist())]
        assert names == e.names


def test_requests_at_every_phase_of_the_pointer_and_of_a_word(gpu):
    """The base pointer at 0..15 moves the dword loads of the newline kernel;
    the first name's length 0..63 moves every later newline through the 64 bits
    of a bitmap word and the 16 positions of a lane."""
    raw = torch.empty(4096, dtype=torch.uint8, device=gpu)

    def at_phase(stream, phase):
        lead = (phase - raw.data_ptr()) % 16
        run = raw[lead:lead + len(stream)]
        run.copy_(torch.frombuffer(bytearray(stream), dtype=torch.uint8))
        assert run.data_ptr() % 16 == phase
        return run
    for phase in range(16):
        assert len(_hold(wire.parse_get_files_device(at_phase(THREE, phase)), THREE, phase).names) == 3
    for pad in range(64):
        stream = get_file(b"p" * pad) + THREE + get_file(b"q" * 100) + THREE + b"GET_FILE\nhalf"
        e = _hold(wire.parse_get_files_device(at_phase(stream, pad % 16)), stream, pad)
        assert len(e.names) == 8 and e.stop == INCOMPLETE


def _many(n: int, seed: int = 0):
    rng = random.Random(1000 * n + seed)
    return [bytes(rng.choice(b"abcdefgh/._-") for _ in range(rng.choice((0, 1, 5, 17, 64, 99, 100)))) for _ in range(n)]


@pytest.mark.parametrize("n", [63, 64, 65, 257, 3000])
def test_runs_across_lane_word_and_workgroup_seams(gpu, n):
    names = _many(n)
    for tail in (b"", b"COMPLETE\n"):
        stream = get_files_run(names) + tail
        e = _hold(wire.parse_get_files_device(_dev(stream, gpu)), stream, n)
        assert e.names == names and e.consumed == len(stream) - len(tail)
    # a line that fails in the middle ends the requests there, whatever follows
    stream = get_files_run(names[:n // 2]) + b"GET_FILE\n" + b"z" * 101 + b"\n" + get_files_run(names[n // 2:])
    assert len(_hold(wire.parse_get_files_device(_dev(stream, gpu)), stream, n).names) == n // 2


def _raw_parse(gpu, stream, cap, null=None):
    x = _dev(stream, gpu)
    outs = [torch.full(((cap + 2) * w,), 0x5A, dtype=torch.uint8, device=gpu).view(t) for t, w in ((torch.int64, 8), (torch.int32, 4))]
    n, bad, used = (ctypes.c_uint64(9) for _ in range(3))
    stop = ctypes.c_int(9)
    rc = _lib.lib().sf_wire_parse_get_files_device(
        x.data_ptr(), x.numel(), *(None if null == j else o.data_ptr() for j, o in enumerate(outs)), cap,
        *(ctypes.byref(v) for v in (n, bad, used, stop)), torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize(gpu)
    return rc, n.value, bad.value, used.value, stop.value, [o.cpu().numpy() for o in outs]


def test_capacity_exact_one_short_and_the_query(gpu):
    stream = get_files_run(_many(6) + [b"\xff"]) + b"GET_FILE\n"
    e = expected(stream)
    assert len(e.names) == 7 and e.bad_name == 6
    for cap, null in ((7, None), (9, None), (6, None), (7, 0), (7, 1), (0, None)):
        rc, n, bad, used, stop, outs = _raw_parse(gpu, stream, cap, null)
        assert (n, bad, used, stop) == (7, 6, e.consumed, INCOMPLETE)
        k = 0 if null is not None else min(cap, 7)
        assert rc == (0 if k == 7 else _lib.SF_ENOSPC)
        assert outs[0][:k].tolist() == e.name_at[:k] and outs[1][:k].tolist() == e.name_len[:k]
        for o in outs:  # nothing past the rows that fit
            assert set(o.view(np.uint8)[k * o.itemsize:].tolist()) == {0x5A}


# ------------------------------------------------------------------ the answer

class Tables:
    """A get_files_expect source on the device: the set and the three arrays."""

    def __init__(self, source, gpu, stream=None):
        names, present, first, digests, sizes = csr(source)
        self.set = device.NameSet.build(names, present, gpu, stream=stream)
        self.first = torch.tensor(first, dtype=torch.int64, device=gpu)
        self.digests = _dev(digests, gpu).reshape(-1, 20)
        self.sizes = torch.from_numpy(np.array(sizes, np.uint32).view(np.int32)).to(gpu)

    def serve(self, stream: bytes, max_run_bytes=0):
        return self.set.serve_files(_dev(stream, self.first.device), self.first, self.digests, self.sizes, max_run_bytes)

    def close(self):
        self.set.close()


def _served(got, want, what=None):
    """One ``device.FilesServed`` against the model; returns the run's bytes."""
    with got.run as run:
        data = run.bytes()
        assert (got.n_requests, got.n_answered, got.answered_bytes, got.why, got.consumed, got.stop) == tuple(want[1:7]), what
        assert data == want.run and run.n_messages == want.messages and isinstance(run, wire.FilesRun), what
    return data


@pytest.fixture(scope="module")
def plan(gpu):
    source = plan_source(random.Random(40))
    t = Tables(source, gpu)
    yield source, t
    t.close()


def test_the_plan_table(plan):
    source, t = plan
    whys = set()
    for name, stream, bound in plan_cases(source):
        want = served(stream, source, bound)
        _served(t.serve(stream, bound), want, name)
        route, requests, answered, readbacks = device.serve_files_stats()
        assert (requests, answered) == (want.n_requests, want.n_answered), name
        # (no answer: the coarse stop alone may show it, before the third read-back)
        assert (route, readbacks) == (2, READBACKS) if want.n_answered else (route == 1 and readbacks in (2, READBACKS)), name
        whys.add(want.why)
    assert whys == {ALL, BAD_NAME, UNKNOWN, FULL}


def test_no_request_and_no_bytes(plan):
    source, t = plan
    for stream, readbacks in ((b"", 0), (b"GET_FILE\n", 1), (b"COMPLETE\n", 1), (b"X" * 30, 1)):
        _served(t.serve(stream), served(stream, source), stream)
        assert device.serve_files_stats() == (1 if stream else 0, 0, 0, readbacks)


def _index_of(files):
    """An index holding ``files`` = [(name, [(digest, size)])], and a few rows
    that are not to be found: a temporary file and a second row of a name."""
    idx = Index.open_in_memory()
    idx.add_temp_file("incoming.bin")
    for k, (name, rows) in enumerate(files):
        fid = put(idx, name.decode(), H(k % 200), size=sum(s for _d, s in rows))
        at = 0
        for d, s in rows:
            idx.add_block(HashDigest(d), fid, at, s)
            at += s
        if k == 1:
            put(idx, name.decode(), H(201))  # the same name again, with no block: the first row wins
    idx.commit()
    return idx


@pytest.mark.parametrize("total", [63, 64, 65, 257, 3000])
def test_sets_requested_in_shuffled_order_with_repeats(gpu, total):
    rng = random.Random(total)
    files = [(b"d%d/f%04d" % (k % 7, k), [(d, max(s, 1)) for d, s in rows])
             for k, (_n, rows) in enumerate(files_with_messages(rng, total))]
    idx = _index_of(files)
    names = [n for n, _r in files]
    asked = names + rng.choices(names, k=len(names) // 2 + 2)
    rng.shuffle(asked)
    want, n = idx.serve_get_files(asked)
    assert n == len(asked)
    stream = get_files_run(asked)
    with idx.source_tables(gpu) as t:
        assert t.names[2] == t.names[1] and int(t.file_first[-1]) == sum(len(r) for _n, r in files)
        run, n_requests, n_answered, used, why, consumed, stop = idx.serve_get_file_requests(stream, tables=t)
        with run:
            assert (n_requests, n_answered, used, why, consumed, stop) == (len(asked), len(asked), len(stream), ALL, len(stream), END)
            assert run.bytes() == want
            assert device.serve_files_stats() == (2, len(asked), len(asked), READBACKS)
            if total in (65, 3000):  # through the parser, and through the destination's half
                by_name = dict(files)
                assert parse_back(want) == [(a, by_name[a]) for a in asked]
                tab = np.frombuffer(b"".join(d for _n, rows in files for d, _s in rows), np.uint8).reshape(-1, 20)
                present = np.ones(len(tab), np.uint8)
                present[::3] = 0
                with device.BlockSet(torch.from_numpy(tab.copy()).to(gpu), torch.from_numpy(present).to(gpu)) as bset:
                    r = run.receive(bset)
                    got_digests = r.digests.cpu().numpy()
                    assert (r.consumed, r.stop, r.open) == (len(want), wire.SF_WIRE_END, False)
                    assert got_digests.tobytes() == b"".join(d for a in asked for d, _s in by_name[a])
                    assert r.file_first.tolist()[-1] == sum(len(by_name[a]) for a in asked) and len(r.file_first) == len(asked) + 1
                    assert np.array_equal(r.rows.cpu().numpy(), oracle.block_lookup(tab, present, got_digests))
    # the one-call form builds its own tables and gives them back
    run = idx.serve_get_file_requests(stream, device=gpu)[0]
    with run:
        assert run.bytes() == want


@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda p: f"{p:#04x}")
@pytest.mark.parametrize("phase", [0, 1, 6, 15])
def test_inputs_carved_from_a_patterned_allocation_stay_bit_identical(gpu, phase, pattern):
    source = plan_source(random.Random(41 + phase))
    names, present, first, digests, sizes = csr(source)
    asked = [n for n, p, _r in source if p] * 2
    random.Random(phase).shuffle(asked)
    stream = get_files_run(asked) + b"GET_FILE\nhal"
    at = np.zeros(len(names) + 1, np.int64)
    np.cumsum([len(n) for n in names], out=at[1:])
    arrays = {"requests": np.frombuffer(stream, np.uint8), "names": np.frombuffer(b"".join(names), np.uint8), "name_at": at,
              "present": np.array(present, np.uint8), "first": np.array(first, np.int64),
              "digests": np.frombuffer(digests, np.uint8).reshape(-1, 20), "sizes": np.array(sizes, np.uint32).view(np.int32)}
    phases = {"requests": phase, "names": (phase * 7) % 16, "name_at": 8, "present": 3, "first": 8, "digests": 4, "sizes": 12}
    a = Arena(gpu, pattern, capacity=1 << 16)
    t = {}
    for k, v in arrays.items():
        t[k] = a.carve(k, v.nbytes, torch.from_numpy(v.copy()).dtype, phases[k]).view(v.shape)
        t[k].copy_(torch.from_numpy(v.copy()))
    a.watch(**t)
    with device.NameSet(t["names"], t["name_at"], t["present"]) as ns:
        got = ns.serve_files(t["requests"], t["first"], t["digests"], t["sizes"])
        want = served(stream, source)
        assert want.stop == INCOMPLETE and want.n_answered == len(asked)
        _served(got, want)
    a.check(dict(arrays))


def test_a_broken_row_is_refused_where_answering_reaches_it(plan, gpu):
    source, t = plan
    first = t.first.clone()
    n_blocks = int(first[-1])
    first[8] = n_blocks + 5  # row 8 above its successor; row 7's end past the table
    g = get_files_run

    def call(stream, bound=0):
        return t.set.serve_files(_dev(stream, gpu), first, t.digests, t.sizes, bound)
    for stream, bound, row in ((g([b"a.bin", b"x/FILE_END"]), 0, 8), (g([b"x/FILE_END"]), 1, 8), (g([b"twice"]), 0, 7)):
        with pytest.raises(ValueError, match=f"row {row}:"):
            call(stream, bound)
        h, bad = ctypes.c_void_p(5), ctypes.c_uint64(0)
        v = [ctypes.c_uint64(0) for _ in range(4)]
        why, stop = ctypes.c_int(0), ctypes.c_int(0)
        x = _dev(stream, gpu)
        rc = _lib.lib().sf_serve_get_files_device(t.set._h, first.data_ptr(), t.digests.data_ptr(), t.sizes.data_ptr(), n_blocks,
                                                  x.data_ptr(), x.numel(), bound, ctypes.byref(h), ctypes.byref(v[0]),
                                                  ctypes.byref(v[1]), ctypes.byref(v[2]), ctypes.byref(why), ctypes.byref(bad),
                                                  ctypes.byref(v[3]), ctypes.byref(stop), torch.cuda.current_stream(gpu).cuda_stream)
        assert (rc, bad.value, h.value) == (_lib.SF_EINVAL, row, None)
    # the same rows unused, or behind the stop: SF_OK
    for stream, bound in ((g([b"a.bin", b"dir/b.bin", b""]), 0), (g([b"a.bin", b"nope", b"x/FILE_END"]), 0),
                          (g([b"a.bin", b"\xff", b"twice"]), 0), (g([b"dir/b.bin", b"x/FILE_END"]), 100)):
        _served(call(stream, bound), served(stream, source, bound), stream)


def test_the_full_continuation_loop(plan, gpu):
    source, t = plan
    asked = [b"a.bin", b"dir/b.bin", b"e1", b"dir/b.bin", b"n" * 100, b"", b"empty_last", b"x/FILE_END"]
    stream = get_files_run(asked) + b"COMPLETE\n"
    whole = served(stream, source)
    bound = max(len(served(get_file(n), source).run) for n in asked)
    rest, pieces, calls = stream, [], 0
    while True:
        got = t.serve(rest, bound)
        data = _served(got, served(rest, source, bound), calls)
        pieces.append(data)
        calls += 1
        assert len(data) <= bound and got.stop == wire.SF_WIRE_OTHER
        if got.why != FULL:
            break
        assert got.n_answered > 0
        rest = rest[got.answered_bytes:]
    assert b"".join(pieces) == whole.run and calls > 2 and got.why == ALL
    assert rest[got.consumed:] == b"COMPLETE\n"


def test_readbacks_do_not_grow_with_the_requests(plan):
    source, t = plan
    counts = []
    for n in (3, 3000):
        asked = [b"a.bin", b"e1", b"twice"] * (n // 3)
        got = t.serve(get_files_run(asked))
        assert (got.n_answered, got.why) == (n, ALL)
        got.run.close()
        counts.append(device.serve_files_stats())
    assert [c[3] for c in counts] == [READBACKS, READBACKS] and [c[1] for c in counts] == [3, 3000]


# --------------------------------------------------------------- the stream order

def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy())


def _behind_a_hold(gpu, real, decoy, call, keep):
    """``call(inputs, stream)`` with its inputs still in production on a fresh
    stream (stream_order.pending), against the same call on finished inputs."""
    def on_host(result):
        return tuple(so._plain(r).cpu().numpy() if isinstance(r, torch.Tensor) else r for r in result)
    real = {k: v.to(gpu) for k, v in real.items()}
    decoy = {k: v.to(gpu) for k, v in decoy.items()}
    torch.cuda.synchronize(gpu)
    want, other = on_host(call(real, None)), on_host(call(decoy, None))
    assert not so.same(other, want)  # the decoy has another answer: an early read shows as a wrong result
    ms = so.timed_ms(lambda: call(real, None), gpu)
    S = so.fresh_stream(gpu)
    x, _ = so.pending(S, real, decoy, so.hold_ms(ms))
    got = so.settle(S, x, decoy, call(x, S))
    assert so.same(got, want), so.first_difference(got, want)
    for k in keep:
        k.close()


def test_each_blocking_call_keeps_its_callers_stream_order(gpu):
    keep = []
    rng = np.random.default_rng(3)

    def inputs(prefix, salt):
        names = [prefix + b"%03d" % i for i in range(200)]
        at = np.zeros(201, np.int64)
        np.cumsum([len(n) for n in names], out=at[1:])
        first = np.arange(0, 201 * 3, 3, dtype=np.int64)
        asked = [names[(7 * i + salt) % 200] for i in range(300)]
        return dict(requests=_t(np.frombuffer(get_files_run(asked), np.uint8)), names=_t(np.frombuffer(b"".join(names), np.uint8)),
                    name_at=_t(at), first=_t(first), digests=_t(rng.integers(0, 256, (600, 20), dtype=np.uint8)),
                    sizes=_t(rng.integers(0, 1 << 31, 600, dtype=np.int64).astype(np.int32)))
    real, decoy = inputs(b"f", 0), inputs(b"g", 1)  # the same lengths: a decoy has its input's shape

    def parse(x, s):
        return wire.parse_get_files_device(x["requests"], stream=s)
    _behind_a_hold(gpu, {"requests": real["requests"]}, {"requests": _t(np.frombuffer(get_files_run(
        [b"h%02d" % (i % 100) for i in range(330)])[:real["requests"].numel()], np.uint8))}, parse, keep)

    def serve(x, s):
        ns = device.NameSet(x["names"], x["name_at"], stream=s)
        got = ns.serve_files(x["requests"], x["first"], x["digests"], x["sizes"])
        keep.extend((got.run, ns))
        return (got.run.tensor(),) + tuple(got[1:])
    _behind_a_hold(gpu, real, decoy, serve, keep)


# ------------------------------------------------------------------- end to end

def test_two_indices_exchange_a_sync_on_the_device(gpu):
    """The destination's Index.receive_file_entries(device) builds the request
    run; its GetFilesRun.serve answers it from the source's tables; the
    destination's Index.receive_files takes the answer.  No forged bytes."""
    from file_list_cases import H_first, H_last
    src = Index.open_in_memory()
    for k, (name, h) in enumerate((("same", H(1)), ("changed", H(9)), ("unknown", H(10)), ("nohash", H(12)),
                                   ("last_byte", H_last(5)), ("first_byte", H_first(6)), ("dir/é.txt", H(7)))):
        fid = put(src, name, h, size=11 * k)
        src.add_blocks(fid, [(11 * j, 11, H(40 + k + j).bytes) for j in range(k)])  # 0 to 6 blocks
    src.commit()
    dst = destination(leftover=False)
    n, _consumed, stop, needed, requests = dst.receive_file_entries(src.file_entries(), device=gpu)
    assert (n, stop) == (7, END_FILES) and needed == [b"changed", b"unknown", b"nohash", b"last_byte", b"first_byte"]
    with requests, src.source_tables(gpu) as t:
        assert isinstance(requests, wire.GetFilesRun) and requests.bytes() == get_files_run(needed)
        got = requests.serve(t.name_set, t.file_first, t.digests, t.sizes)
        assert (got.n_requests, got.n_answered, got.why, got.stop) == (5, 5, ALL, END)
        assert got.answered_bytes == got.consumed == requests.nbytes
        with got.run as run:
            data = run.bytes()
    assert (data, 5) == src.serve_get_files(needed)
    copies, consumed, carry = dst.receive_files(data, device=gpu)
    dst.commit()
    assert (consumed, carry) == (len(data), None)
    for name in needed:
        got_rows = dst.list_file_blocks(dst.get_temp_file(PurePath(name.decode()))[0])
        assert got_rows == src.list_file_blocks(src.get_file(PurePath(name.decode()))[0]), name
    assert len(dst.list_missing_blocks()) == 1 + 2 + 3 + 4 + 5
