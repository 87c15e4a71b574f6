"""GPU: the files-list phase on the device -- sf_receive_file_entries_device
against entries_expect (wire.Parser alone), both writers byte for byte against
wire.write_message, the round trip through Index on both routes, and each
blocking call once behind a hold on a fresh stream (tests/stream_order.py).

Shapes are the smallest that reach each path: lists of 1 to 300 entries, one of
3,000.  The fixed table is test_wire_entries.py's, which the rules header
passes on the CPU; here the kernels that call the same rules must give the same
answers, on the device chain, on the forced host route and on the fallback."""
import ctypes
import os

import numpy as np
import pytest
import torch

import stream_order as so
from entries_expect import (END, END_FILES, END_FILES_MSG, INCOMPLETE, entries_run, entry, expected, get_files_run,
                            needs_fallback)
from file_list_cases import SCENARIOS, copy, destination, run_pieces, table as files_table
from test_gpu_file_list_extent import NAMES, PRESENT, _ref
from test_wire_entries import D1, D2, table
from syncfast_amd import _lib, device, wire
from syncfast_amd.index import Index, SyncfastError

pytestmark = pytest.mark.gpu

DEVICE, FORCED, FALLBACK = 0, 1, 2


def _dev(b: bytes, gpu):
    return device.upload(b, gpu)


def _hold(got, stream: bytes, what=None):
    """One ``EntriesReceived`` (a parse only) against the model."""
    e = expected(stream)
    assert (got.consumed, got.stop, got.bad_name) == (e.consumed, e.stop, e.bad_name), what
    assert got.name_at.cpu().tolist() == e.name_at and got.name_len.cpu().tolist() == e.name_len, what
    assert got.sizes.cpu().tolist() == e.sizes and got.hashes.cpu().numpy().tobytes() == b"".join(e.hashes), what
    assert got.rows is None and got.need is None and got.need_list is None
    return e


def test_fixed_table_on_the_device_chain_and_the_fallback(gpu):
    routes = set()
    for name, stream in table():
        e = _hold(device.receive_file_entries(_dev(stream, gpu)), stream, name)
        route, cand, chained, readbacks = device.file_entries_stats()
        if not stream:
            assert (route, cand, chained, readbacks) == (0, 0, 0, 0)  # nothing launched
            continue
        assert route == (FALLBACK if needs_fallback(stream) else DEVICE), name
        assert chained == len(e.sizes) and readbacks == (2 if route == FALLBACK else 1), name
        routes.add((name, route))
    assert {(k, FALLBACK) for k in ("forged_digest", "forged_digest_last", "forged_name")} <= routes
    assert ("name_tag_honest", DEVICE) in routes and sum(r == FALLBACK for _n, r in routes) == 3


def test_forced_host_route(gpu, knobs):
    knobs.set("SF_TEST_WIRE_PARSE_HOST", 1)
    for name, stream in table()[::7]:
        _hold(device.receive_file_entries(_dev(stream, gpu)), stream, name)
        if stream:
            assert device.file_entries_stats()[::3] == (FORCED, 1), name


def _list(first_len: int, n: int = 5) -> bytes:
    rng = np.random.default_rng(first_len)
    out = entry(b"p" * first_len, first_len, D1)
    for k in range(n - 1):
        out += entry(bytes(rng.integers(97, 123, int(rng.integers(0, 101)), dtype=np.uint8)), int(rng.integers(0, 10 ** 15)),
                     bytes(rng.integers(0, 256, 20, dtype=np.uint8)))
    return out + END_FILES_MSG


def test_entries_start_at_every_phase_of_a_word_and_of_the_pointer(gpu):
    """The first name's length 0..63 moves every later entry through the 64
    phases of a bitmap word and the 16 of a lane; the base pointer at 0..15
    moves the dword loads of the candidates kernel."""
    raw = torch.empty(4096, dtype=torch.uint8, device=gpu)
    for first_len in range(64):
        stream = _list(first_len)
        for phase in (range(16) if first_len in (0, 37) else (first_len % 16,)):
            lead = (phase - raw.data_ptr()) % 16
            run = raw[lead:lead + len(stream)]
            run.copy_(torch.frombuffer(bytearray(stream), dtype=torch.uint8))
            assert run.data_ptr() % 16 == phase
            e = _hold(device.receive_file_entries(run), stream, (first_len, phase))
            assert len(e.sizes) == 5 and e.stop == END_FILES and device.file_entries_stats()[0] == DEVICE


def test_a_list_cut_at_every_byte_and_continued(gpu):
    whole = entry(b"dir/a", 5, D1) + entry(b"", 0, D2) + entry(b"b" * 7, 10 ** 15 - 1, D1) + END_FILES_MSG
    e = expected(whole)
    for cut in range(len(whole) + 1):
        first = device.receive_file_entries(_dev(whole[:cut], gpu))
        _hold(first, whole[:cut], cut)
        rest = whole[first.consumed:]
        if first.stop == END_FILES:
            assert cut == len(whole) and not rest
            continue
        assert first.stop in (END, INCOMPLETE) or whole[cut - 15:cut] == b"9" * 15  # "Unterminated size": the parser's
        second = device.receive_file_entries(_dev(rest, gpu))
        _hold(second, rest, cut)
        assert second.stop == END_FILES and first.consumed + second.consumed == len(whole)
        names = [whole[a:a + n] for a, n in zip(first.name_at.cpu().tolist(), first.name_len.cpu().tolist())]
        names += [rest[a:a + n] for a, n in zip(second.name_at.cpu().tolist(), second.name_len.cpu().tolist())]
        assert names == e.names and first.sizes.cpu().tolist() + second.sizes.cpu().tolist() == e.sizes


def test_three_thousand_entries(gpu):
    rng = np.random.default_rng(8)
    files = [(b"d%d/f%d" % (i % 41, i) + b"x" * int(rng.integers(0, 60)), int(rng.integers(0, 1 << 40)),
              bytes(rng.integers(0, 256, 20, dtype=np.uint8))) for i in range(3000)]
    stream = entries_run(files)
    e = _hold(device.receive_file_entries(_dev(stream, gpu)), stream)
    assert len(e.sizes) == 3000 and device.file_entries_stats()[0] == DEVICE


def _raw_receive(gpu, stream, cap, null=False):
    x = _dev(stream, gpu)
    e = lambda k, t, width: torch.full((k * width,), 0x5A, dtype=torch.uint8, device=gpu).view(t)  # noqa: E731
    outs = [e(cap + 2, torch.int64, 8), e(cap + 2, torch.int32, 4), e(cap + 2, torch.int64, 8),
            e(20 * (cap + 2), torch.uint8, 1)]  # every byte 0x5A
    n, need, bad, used = (ctypes.c_uint64(9) for _ in range(4))
    why = ctypes.c_int(9)
    rc = _lib.lib().sf_receive_file_entries_device(
        None, x.data_ptr(), x.numel(), None, None, *(None if null and j == 2 else o.data_ptr() for j, o in enumerate(outs)),
        None, None, None, cap, *(ctypes.byref(v) for v in (n, need, bad, used, why)),
        torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize(gpu)
    return rc, n.value, used.value, why.value, [o.cpu().numpy() for o in outs]


def test_capacity_exact_one_short_and_the_query(gpu):
    stream = _list(9, n=6)
    e = expected(stream)
    for cap, null in ((6, False), (5, False), (6, True), (0, False)):
        rc, n, used, why, outs = _raw_receive(gpu, stream, cap, null)
        assert (n, used, why) == (6, e.consumed, END_FILES)
        k = 0 if null else min(cap, 6)
        assert rc == (0 if k == 6 else _lib.SF_ENOSPC)
        assert outs[0][:k].tolist() == e.name_at[:k] and outs[1][:k].tolist() == e.name_len[:k]
        assert outs[2][:k].tolist() == e.sizes[:k] and outs[3][:20 * k].tobytes() == b"".join(e.hashes[:k])
        for o in outs:  # nothing past the rows that fit
            assert set(o.view(np.uint8)[k * o.itemsize * (20 if o.dtype == np.uint8 else 1):].tolist()) == {0x5A}


@pytest.mark.parametrize("route", ["device", "host", "forged"])
def test_need_and_the_need_list(gpu, knobs, route):
    """Hashes that differ in the first byte only and in the last byte only, a
    row without a recorded hash, an absent row, a repeated name whose first row
    is temporary: rows, need and the list against the model (the data set of
    test_gpu_file_list_extent.py)."""
    data, have, have_ok, e, want = _ref(route == "forged")
    if route == "host":
        knobs.set("SF_TEST_WIRE_PARSE_HOST", 1)
    with device.NameSet.build(NAMES, PRESENT, gpu) as ns:
        hv, ok = torch.from_numpy(have).to(gpu), torch.from_numpy(have_ok).to(gpu)
        got = ns.receive_entries(_dev(data, gpu), hv, ok)
        assert device.file_entries_stats()[0] == ("device", "host", "forged").index(route)
        assert got.rows.cpu().tolist() == want["rows"].tolist() and got.need.cpu().tolist() == want["need"].tolist()
        assert got.need_list.cpu().tolist() == want["need_list"].tolist()
        assert (got.consumed, got.stop, got.bad_name) == (e.consumed, e.stop, None)
        # no flags: every row has a recorded hash, so "nohash" is compared like the others
        got = ns.receive_entries(_dev(data, gpu), hv)
        assert got.need.cpu().tolist() == [0 if i == 5 else v for i, v in enumerate(want["need"].tolist())]
    with device.NameSet.build([], None, gpu) as none:  # a set of no rows: every entry is needed
        got = none.receive_entries(_dev(data, gpu), torch.empty((0, 20), dtype=torch.uint8, device=gpu))
        assert got.rows.cpu().tolist() == [-1] * 11 and got.need_list.cpu().tolist() == list(range(11))


@pytest.mark.parametrize("where", [0, 2, 4])
def test_bad_name_first_middle_and_last(gpu, knobs, where):
    names = [b"a", b"b\xc3\xa9", b"c", b"d", b"e"]
    names[where] = b"bad\xed\xa0\x80"  # a surrogate
    if where == 2:
        names[3] = b"\xff"  # a later one does not lower it
    stream = entries_run([(n, 1, D1) for n in names])
    for host in (0, 1):
        knobs.set("SF_TEST_WIRE_PARSE_HOST", host)
        got = device.receive_file_entries(_dev(stream, gpu))
        e = _hold(got, stream)
        assert got.bad_name == where == e.bad_name and len(e.sizes) == 5  # the entries behind it are still there


# ------------------------------------------------------------------ the writers

def _carved(gpu, parts, phases):
    """Tensors holding ``parts`` (numpy arrays) inside one patterned
    allocation, part j ``phases[j]`` bytes past a 64-byte boundary; returns
    (the allocation, its host image, the views)."""
    buf = torch.full((1 << 16,), 0xC3, dtype=torch.uint8, device=gpu)
    at, views = 64, []
    for p, ph in zip(parts, phases):
        raw = np.ascontiguousarray(p).view(np.uint8).reshape(-1)
        at = -(-at // 64) * 64 + ph
        buf[at:at + raw.size] = torch.from_numpy(raw.copy()).to(gpu)
        views.append(buf[at:at + raw.size].view({np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32,
                                                 np.dtype(np.uint8): torch.uint8}[p.dtype]))
        at += raw.size + 64
    torch.cuda.synchronize(gpu)
    return buf, buf.cpu().numpy().copy(), views


FILES = [(b"", 0, D1), (b"a", 9, D2), (b"n" * 99, 10, b"\n" * 20), (b"n" * 100, 10 ** 15 - 1, D1),
         (b"dir/\xc3\xa9", 123456789012, D2), (b"x/FILE_ENTRY", 1 << 40, b"FILE_ENTRY\n\n1\n" + b"z" * 6), (b"ab", 99999, D1)]


def _entry_inputs(files):
    at = np.zeros(len(files) + 1, np.int64)
    np.cumsum([len(n) for n, _s, _h in files], out=at[1:])
    return [np.frombuffer(b"".join(n for n, _s, _h in files) or b"\0", np.uint8), at,
            np.array([s for _n, s, _h in files], np.uint64).view(np.int64),
            np.frombuffer(b"".join(h for _n, _s, h in files), np.uint8)]


def test_file_entries_run_is_write_message_at_every_name_phase(gpu):
    for phase in range(8):
        buf, image, (names, at, sizes, hashes) = _carved(gpu, _entry_inputs(FILES), (phase, 8, 24, 4 * (phase % 4)))
        for end in (True, False):
            with wire.file_entries_device(names[:sum(len(f[0]) for f in FILES)], at, sizes, hashes.reshape(-1, 20), end) as run:
                assert run.bytes() == entries_run(FILES, end) and run.n_messages == len(FILES) + end
                if phase == 0 and end:  # through the parser, and the descriptor route once
                    msgs = wire.Parser().receive(run.bytes())
                    assert [(m[1], m[2], m[3].bytes) for m in msgs[:-1]] == FILES and msgs[-1] == ("EndFiles",)
                    r, w = os.pipe()
                    assert run.to_fd(w) == run.nbytes
                    os.close(w)
                    with os.fdopen(r, "rb") as f:
                        assert f.read() == entries_run(FILES)
                    got = run.receive()  # straight into the receiver: the forged digest takes the fallback
                    assert got.stop == END_FILES and got.name_len.cpu().tolist() == [len(f[0]) for f in FILES]
                    assert device.file_entries_stats()[0] == FALLBACK
        torch.cuda.synchronize(gpu)
        assert np.array_equal(buf.cpu().numpy(), image)  # the inputs and everything around them, bit-identical


def test_file_entries_run_of_no_file(gpu):
    z = lambda t: torch.zeros(1, dtype=t, device=gpu)  # noqa: E731
    with wire.file_entries_device(torch.empty(0, dtype=torch.uint8, device=gpu), z(torch.int64),
                                  torch.empty(0, dtype=torch.int64, device=gpu),
                                  torch.empty((0, 20), dtype=torch.uint8, device=gpu), True) as run:
        assert run.bytes() == END_FILES_MSG and run.n_messages == 1
    with wire.file_entries_device(torch.empty(0, dtype=torch.uint8, device=gpu), z(torch.int64),
                                  torch.empty(0, dtype=torch.int64, device=gpu),
                                  torch.empty((0, 20), dtype=torch.uint8, device=gpu), False) as run:
        assert run.bytes() == b"" and run.n_messages == 0


def test_file_entries_refuses_the_first_bad_file(gpu):
    bads = [(b"x", 10 ** 15, D1), (b"n" * 101, 1, D1), (b"a\nb", 1, D1), (b"x", (1 << 64) - 1, D1)]
    for k, bad in enumerate(bads):
        files = FILES[:k + 1] + [bad] + FILES[:2] + [bads[0]]
        names, at, sizes, hashes = (torch.from_numpy(p.copy()).to(gpu) for p in _entry_inputs(files))
        with pytest.raises(ValueError, match=f"file {k + 1}:"):
            wire.file_entries_device(names, at, sizes, hashes.reshape(-1, 20))
    names, at, sizes, hashes = (torch.from_numpy(p.copy()).to(gpu) for p in _entry_inputs(FILES))
    for change, f in (({0: 1}, 0), ({3: 0}, 2), ({7: 1 << 40}, 6), ({2: 1 << 40}, 1)):  # the CSR
        bad_at = at.clone()
        for i, v in change.items():
            bad_at[i] = v
        with pytest.raises(ValueError, match=f"file {f}:"):
            wire.file_entries_device(names, bad_at, sizes, hashes.reshape(-1, 20))
    with wire.file_entries_device(names, at, sizes, hashes.reshape(-1, 20)) as run:  # nothing was kept or broken
        assert run.bytes() == entries_run(FILES)


def test_get_files_run_is_write_message(gpu):
    stream = entries_run(FILES)
    e = expected(stream)
    for phase in range(4):
        spans_at, spans_len = np.array(e.name_at, np.int64) , np.array(e.name_len, np.int32)
        buf, image, (data, at, ln, pick) = _carved(
            gpu, [np.frombuffer(stream, np.uint8), spans_at, spans_len, np.array([6, 0, 3, 3, 5, 1, 6], np.int32)],
            (phase, 8, 4, 12))
        with wire.get_files_device(data, at, ln) as run:  # all, in order
            assert run.bytes() == get_files_run(e.names) and run.n_messages == len(FILES)
            assert [m[1] for m in run.receive()] == e.names  # through the parser
        with wire.get_files_device(data, at, ln, pick) as run:  # repeated and out of order
            assert run.bytes() == get_files_run([e.names[i] for i in (6, 0, 3, 3, 5, 1, 6)])
            if phase == 0:
                r, w = os.pipe()
                assert run.to_fd(w) == run.nbytes
                os.close(w)
                with os.fdopen(r, "rb") as f:
                    assert f.read() == run.bytes()
        with wire.get_files_device(data, at, ln, pick[:0]) as run:
            assert run.bytes() == b"" and run.n_messages == 0
        torch.cuda.synchronize(gpu)
        assert np.array_equal(buf.cpu().numpy(), image)


def test_get_files_refuses_the_first_bad_pick(gpu):
    stream = entries_run(FILES) + b"n" * 101
    e = expected(stream)
    n = len(stream)
    at = e.name_at + [n - 101, n - 3, n + 1, e.name_at[3] - 1]  # 101 bytes; leaves the buffer; starts past it; holds '\n'
    ln = e.name_len + [101, 4, 0, 3]
    data = _dev(stream, gpu)
    t = lambda v, d: torch.tensor(v, dtype=d, device=gpu)  # noqa: E731
    for pick, bad in (([0, 1, 7], 2), ([8, 0], 0), ([2, 2, 9], 2), ([10], 0), ([1, 11], 1), ([0, -1], 1), (None, 7)):
        with pytest.raises(ValueError, match=f"pick {bad}:"):
            wire.get_files_device(data, t(at, torch.int64), t(ln, torch.int32), None if pick is None else t(pick, torch.int32))
    with wire.get_files_device(data, t(at, torch.int64), t(ln, torch.int32), t([6, 6], torch.int32)) as run:
        assert run.bytes() == get_files_run([b"ab", b"ab"])


# --------------------------------------------------------------- the round trip

def _source() -> Index:
    from file_list_cases import H, H_first, H_last, put
    idx = Index.open_in_memory()
    for name, h in (("same", H(1)), ("changed", H(9)), ("unknown", H(10)), ("twice", H(11)), ("dup", H(3)),
                    ("nohash", H(12)), ("last_byte", H_last(5)), ("first_byte", H_first(6)), ("dir/é.txt", H(7)),
                    ("old", H(13))):
        fid = put(idx, name, h, size=11)
        idx.add_blocks(fid, [(0, 5, h.bytes), (5, 6, H(40).bytes)])
    idx.commit()
    return idx


def test_round_trip_source_to_destination_and_back(gpu):
    """Index.file_entries on the device, the list received by
    Index.receive_file_entries(device=gpu), its requests parsed by wire.Parser
    and answered by serve_get_files: tables, names and request bytes equal the
    device=None route's on copies of the same two indexes."""
    src = _source()
    host_list = src.file_entries()
    with src.file_entries(device=gpu) as run:
        assert run.bytes() == host_list
    base = destination()
    on_host, on_gpu = copy(base), copy(base)
    n, consumed, stop, needed, requests = on_host.receive_file_entries(host_list)
    k, used, why, names, req = on_gpu.receive_file_entries(host_list, device=gpu)
    assert (k, used, why, names, req.bytes()) == (n, consumed, stop, needed, requests) and stop == END_FILES
    assert files_table(on_gpu) == files_table(on_host) != files_table(base) and device.file_entries_stats()[0] == DEVICE
    asked = [m[1] for m in wire.Parser().receive(req.bytes())]
    assert asked[0] == b"dir/old" and asked[1:] == needed  # the leftover temp row first: an explicit pick
    answer, answered = src.serve_get_files(asked[1:], device=gpu)
    assert answered == len(needed) and answer.bytes() == src.serve_get_files(asked[1:])[0]
    assert src.serve_get_files(asked)[1] == 0  # the source does not hold the leftover's name


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_receive_file_entries_on_the_device_equals_the_loop(gpu, monkeypatch, name):
    kwargs, pieces, expect = SCENARIOS[name]
    base = destination(**kwargs)
    on_host, on_gpu = copy(base), copy(base)
    if kwargs.get("tmp_nontemp"):  # one lookup would differ from the loop here: the device route is not taken
        def never(*_a):
            raise AssertionError("the device route was taken")
        monkeypatch.setattr(Index, "_receive_file_entries_device", never)
    if isinstance(expect, str):
        for idx, dev in ((on_host, None), (on_gpu, gpu)):
            with pytest.raises(SyncfastError, match=expect):
                run_pieces(idx, pieces, dev)
        assert files_table(on_gpu) == files_table(on_host) != files_table(base)
        return
    want = run_pieces(on_host, pieces)
    assert run_pieces(on_gpu, pieces, gpu) == want and want[1] == expect
    assert files_table(on_gpu) == files_table(on_host)


# ------------------------------------------------------------- the stream order

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


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_each_blocking_call_keeps_its_callers_stream_order(gpu):
    keep = []
    files = [(b"f%03d" % i, i, bytes([i]) * 20) for i in range(200)]
    others = [(b"g%03d" % i, i, bytes([255 - i]) * 20) for i in range(200)]  # the same lengths: a decoy has its input's shape
    inputs = lambda fs: dict(zip(("names", "at", "sizes", "hashes"), (_t(p.copy()) for p in _entry_inputs(fs))))  # noqa: E731

    def entries(x, s):
        run = wire.file_entries_device(x["names"], x["at"], x["sizes"], x["hashes"].reshape(-1, 20), stream=s)
        keep.append(run)
        return (run.tensor(),)
    _behind_a_hold(gpu, inputs(files), inputs(others), entries, keep)

    stream, decoy = entries_run(files), entries_run(others)
    assert len(stream) == len(decoy)

    def lookup(x, s):
        ns = device.NameSet(x["names"], x["at"], stream=s)
        keep.append(ns)
        got = device.receive_file_entries(x["run"], ns, x["have"], stream=s)
        return got.name_at, got.sizes, got.hashes, got.rows, got.need, got.need_list, got.consumed, got.stop
    have = np.frombuffer(b"".join(h for _n, _s, h in files), np.uint8).reshape(-1, 20).copy()
    have[::2] ^= 1
    real = dict(inputs(files), run=_t(np.frombuffer(stream, np.uint8).copy()), have=_t(have))
    fake = dict(inputs(others), run=_t(np.frombuffer(decoy, np.uint8).copy()), have=_t(have[::-1].copy()))
    for d in (real, fake):
        del d["sizes"], d["hashes"]
    _behind_a_hold(gpu, real, fake, lookup, keep)

    def requests(x, s):
        run = wire.get_files_device(x["run"], x["name_at"], x["name_len"], x["pick"], stream=s)
        keep.append(run)
        return (run.tensor(),)
    e = expected(stream)
    spans = dict(run=_t(np.frombuffer(stream, np.uint8).copy()), name_at=_t(np.array(e.name_at, np.int64)),
                 name_len=_t(np.array(e.name_len, np.int32)), pick=_t(np.arange(0, 200, 2, dtype=np.int32)))
    fake = dict(run=_t(np.frombuffer(decoy, np.uint8).copy()), name_at=spans["name_at"].clone(),
                name_len=spans["name_len"].clone(), pick=_t(np.arange(1, 201, 2, dtype=np.int32)))
    _behind_a_hold(gpu, spans, fake, requests, keep)
