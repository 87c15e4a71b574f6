"""GPU: the destination's missing blocks on the device -- the GET_BLOCK run of
its missing rows (device.get_block_requests, sf_wire_get_blocks_device) and a
parsed BLOCK_DATA run joined against them (device.place_block_data,
sf_place_block_data_device), then both through Index and FileImages beside
the host route they replace.  Every expected value is wire.write_message's,
wire.Parser's (send_expect.py), the dict model's (want_expect.py) or the
existing route's (Index.receive_block_data + FileImages.apply_writes)."""
import ctypes
import hashlib
import os
import random
from collections import Counter
from pathlib import PurePath

import numpy as np
import pytest
import torch

import stream_order as so
from send_expect import END, OTHER, expected_requests as parsed_requests
from syncfast_amd import _lib, device, host, wire
from syncfast_amd.assemble import FileImages
from syncfast_amd.digest import HashDigest
from syncfast_amd.index import Index, temp_name
from syncfast_amd.timestamp import DateTimeUtc
from want_expect import e2e_files, expected_requests, join_case, missing_of, place_model

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
GUARD = 0xEE


def _up(b: bytes, gpu):
    return torch.frombuffer(bytearray(b), dtype=U8).to(gpu) if b else torch.empty(0, dtype=U8, device=gpu)


def _table(digests, gpu):
    return _up(b"".join(digests), gpu).reshape(len(digests), 20)


def _t(values, dtype, gpu):
    return torch.tensor(list(values), dtype=dtype, device=gpu)


def _u32(values, gpu):
    return torch.from_numpy(np.array(list(values), np.uint32).view(np.int32)).to(gpu)


# ------------------------------------------------------------------ requests

def _ask(digests, gpu, rows=None, take=None, distinct=False):
    """(run bytes, n_requests) of the device call, with the run's own counts
    checked against them."""
    run, n = device.get_block_requests(_table(digests, gpu), None if rows is None else _t(rows, I64, gpu),
                                       None if take is None else _t(take, U8, gpu), distinct=distinct)
    with run:
        got = run.bytes()
        assert (run.nbytes, run.n_messages) == (len(got), n) and len(got) == 31 * n
        assert run.tensor().cpu().numpy().tobytes() == got
    return got, n


def _masks(rng, n):
    rows = [rng.choice((-1, -1, 0, 7, -(1 << 40), 1 << 40)) for _ in range(n)]
    take = [rng.choice((0, 1, 1, 255)) for _ in range(n)]
    return {"none": (None, None), "all": (None, [1] * n), "take": (None, take), "rows": (rows, None),
            "both": (rows, take), "nothing": ([0] * n, None), "nothing-taken": (None, [0] * n)}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 5000])
def test_the_request_run_is_write_message_over_the_asking_rows(gpu, n):
    rng = random.Random(1000 + n)
    digests = [rng.randbytes(20) for _ in range(n)]
    if n >= 3:  # digests of tags and newlines, and one that repeats
        digests[0], digests[n // 2], digests[n - 1] = b"GET_BLOCK\n" * 2, b"\n" * 20, digests[1]
    for name, (rows, take) in _masks(rng, n).items():
        want = expected_requests(digests, rows, take)
        got, count = _ask(digests, gpu, rows, take)
        assert got == want, (name, n)
        assert count == len(want) // 31
        assert count == {"none": n, "all": n, "nothing": 0, "nothing-taken": 0}.get(name, count)
        # the reference parser reads the same digests back
        back, consumed, stop = parsed_requests(got)
        assert (consumed, stop) == (len(got), END)
        assert b"".join(wire.write_message("GetBlock", d) for d in back) == want
        # and with distinct, the first asking row of each digest alone
        assert _ask(digests, gpu, rows, take, distinct=True)[0] == expected_requests(digests, rows, take, True), name


@pytest.mark.gpu
def test_distinct_keeps_the_first_asking_row(gpu):
    rng = random.Random(21)
    # a zero-filled file: one digest in 300 rows, between others
    zero = hashlib.sha1(bytes(32768)).digest()
    table = [rng.randbytes(20) for _ in range(40)] + [zero] * 300 + [rng.randbytes(20) for _ in range(40)]
    table[10] = table[350] = zero
    got, n = _ask(table, gpu, distinct=True)
    assert n == 80 - 1 and got == expected_requests(table, distinct=True)
    assert got.count(zero) == 1 and got.index(zero) == 31 * 10 + 10
    assert _ask(table, gpu)[1] == 380
    # its first rows do not ask: the first that does is the one
    take = [1] * 380
    for i in (10, 40, 41, 42):
        take[i] = 0
    got, n = _ask(table, gpu, take=take, distinct=True)
    assert got == expected_requests(table, None, take, True) and got.index(zero) == 31 * 39 + 10
    rows = [-1] * 380
    rows[10] = rows[40] = 5
    assert _ask(table, gpu, rows=rows, take=take, distinct=True)[0] == expected_requests(table, rows, take, True)
    # digests that share bytes 0-10: the same slot and the same fingerprint in the set
    head = rng.randbytes(11)
    close = [head + rng.randbytes(9) for _ in range(50)]
    table = [close[rng.randrange(50)] for _ in range(700)] + [rng.randbytes(20) for _ in range(30)]
    rng.shuffle(table)
    take = [int(rng.random() < 0.7) for _ in table]
    for t in (None, take):
        got, n = _ask(table, gpu, take=t, distinct=True)
        want = expected_requests(table, None, t, True)
        assert got == want and n == len(want) // 31
        asked = parsed_requests(got)[0]
        assert len(asked) == len(set(asked)) and 50 < len(asked) <= 80
    # hostile digests, repeated
    table = [b"GET_BLOCK\n" * 2, b"\n" * 20, b"GET_BLOCK\n" * 2, b"\n" * 20, b"\n" * 20]
    assert _ask(table, gpu, distinct=True)[0] == expected_requests(table[:2])
    assert _ask(table, gpu)[0] == expected_requests(table)


@pytest.mark.gpu
def test_the_source_serves_the_device_built_requests(gpu):
    rng = random.Random(22)
    blocks = [rng.randbytes(rng.randrange(1, 3000)) for _ in range(60)] + [b"GET_BLOCK\n" * 2, b"\n" * 20]
    src = b"".join(blocks)
    offs = np.cumsum([0] + [len(b) for b in blocks[:-1]])
    # the source's table: true digests, and two rows under hostile ones
    s_dig = [hashlib.sha1(b).digest() for b in blocks[:60]] + [b"GET_BLOCK\n" * 2, b"\n" * 20]
    wanted = [s_dig[rng.randrange(62)] for _ in range(150)] + s_dig[60:]
    take = [int(rng.random() < 0.8) for _ in wanted]
    with device.BlockSet(_table(s_dig, gpu)) as bset:
        for distinct in (False, True):
            run, n = device.get_block_requests(_table(wanted, gpu), take=_t(take, U8, gpu), distinct=distinct)
            with run:
                answer, n_requests, n_answered, consumed, stop = bset.serve(
                    run.tensor(), _up(src, gpu), _t(offs, I64, gpu), _u32((len(b) for b in blocks), gpu))
                with answer:
                    assert (n_requests, n_answered, consumed, stop) == (n, n, 31 * n, END)
                    asked = parsed_requests(expected_requests(wanted, None, take, distinct))[0]
                    assert len(asked) == n and (n < sum(take)) == distinct
                    assert answer.bytes() == b"".join(
                        wire.write_message("BlockData", d, blocks[s_dig.index(d)]) for d in asked)


# ---------------------------------------------------------------------- join

_join_case = join_case


def _dev(case, gpu):
    return dict(row_digests=_table(case["row_digests"], gpu), row_sizes=_u32(case["row_sizes"], gpu),
                row_dst=_t(case["row_dst"], I64, gpu), row_present=_t(case["row_present"], U8, gpu),
                msg_digests=_table(case["msg_digests"], gpu), msg_sizes=_u32(case["msg_sizes"], gpu),
                msg_offsets=_t(case["msg_offsets"], I64, gpu),
                msg_ok=None if case["msg_ok"] is None else _t(case["msg_ok"], U8, gpu))


def _check_join(case, gpu):
    jobs, present, uses, n_left, mismatch = place_model(**case)
    t = _dev(case, gpu)
    src, dst, sizes, job_rows, job_msgs, msg_uses, got_left, got_mismatch = device.place_block_data(**t)
    got = list(zip(src.tolist(), dst.tolist(), sizes.cpu().numpy().view(np.uint32).tolist(), job_rows.tolist(),
                   job_msgs.tolist()))
    assert got == jobs
    assert msg_uses.tolist() == uses and (got_left, got_mismatch) == (n_left, mismatch)
    assert t["row_present"].tolist() == present
    return jobs, uses, n_left, mismatch


@pytest.mark.gpu
def test_the_join_is_the_dict_models(gpu):
    case = _join_case(31)
    jobs, uses, n_left, mismatch = _check_join(case, gpu)
    # the case holds what it is meant to hold
    by_msg = Counter(j[4] for j in jobs)
    assert max(by_msg.values()) >= 200 and {1, 2, 3} <= set(by_msg.values())
    assert uses.count(0) >= 8 and uses[0] == 0  # unsolicited, superseded and unverified messages
    assert mismatch == 1 and n_left >= 3 and sum(case["row_present"]) > 20
    assert len(jobs) > len(case["msg_digests"])  # more jobs than messages: the wrapper asked twice
    assert [j[3] for j in jobs] == sorted(j[3] for j in jobs)
    # an unverified run: every message counts, the first copy is taken
    case = dict(_join_case(32), msg_ok=None)
    jobs, uses, _left, _m = _check_join(case, gpu)
    assert uses[0] >= 1 and {j[4] for j in jobs if case["row_digests"][j[3]] == case["msg_digests"][0]} == {0}
    # a second call finds nothing left to do for the rows the first one served
    t = _dev(_join_case(31), gpu)
    first = device.place_block_data(**t)
    again = device.place_block_data(**t)
    assert again[0].numel() == 0 and again[5].tolist() == [0] * len(case["msg_digests"])
    assert again[6:] == first[6:]


@pytest.mark.gpu
def test_the_join_without_rows_or_without_messages(gpu):
    case = _join_case(33)
    none = dict(msg_digests=[], msg_sizes=[], msg_offsets=[], msg_ok=None)
    jobs, uses, n_left, _m = _check_join({**case, **none}, gpu)
    assert jobs == [] and uses == [] and n_left == case["row_present"].count(0) > 300
    no_rows = dict(row_digests=[], row_sizes=[], row_dst=[], row_present=[])
    jobs, uses, n_left, _m = _check_join({**case, **no_rows}, gpu)
    assert jobs == [] and uses == [0] * len(case["msg_digests"]) and n_left == 0
    assert _check_join({**no_rows, **none}, gpu) == ([], [], 0, 0)
    # messages that are all unverified are no messages
    assert _check_join({**case, "msg_ok": [0] * len(case["msg_digests"])}, gpu)[0] == []


def _raw_place(t, outs, cap, gpu):
    """sf_place_block_data_device itself, with the caller's outputs and cap."""
    n_jobs, n_left, n_bad = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint64(77)
    p = lambda x: x.data_ptr() if x is not None and x.numel() else None  # noqa: E731
    rc = _lib.lib().sf_place_block_data_device(
        p(t["row_digests"]), p(t["row_sizes"]), p(t["row_dst"]), p(t["row_present"]), t["row_digests"].shape[0],
        p(t["msg_digests"]), p(t["msg_sizes"]), p(t["msg_offsets"]), p(t["msg_ok"]), t["msg_digests"].shape[0],
        p(outs["src"]), p(outs["dst"]), p(outs["sizes"]), p(outs["rows"]), p(outs["msgs"]), cap, p(outs["uses"]),
        ctypes.byref(n_jobs), ctypes.byref(n_left), ctypes.byref(n_bad), torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize(gpu)
    return rc, n_jobs.value, n_left.value, n_bad.value


def _guarded_outs(n, m, gpu):
    outs = {k: torch.empty(n, dtype=I64, device=gpu) for k in ("src", "dst", "rows", "msgs")}
    outs["sizes"] = torch.empty(n, dtype=I32, device=gpu)
    outs["uses"] = torch.empty(m + 5, dtype=I32, device=gpu)
    for v in outs.values():
        v.view(U8).fill_(GUARD)
    return outs


def _raw_bytes(d):
    return {k: v.view(U8).cpu().numpy().tobytes() for k, v in d.items() if v is not None}


@pytest.mark.gpu
def test_a_cap_too_small_marks_nothing_and_a_full_cap_writes_its_jobs_only(gpu):
    case = _join_case(34)
    jobs, present, uses, n_left, mismatch = place_model(**case)
    need, m = len(jobs), len(case["msg_digests"])
    t = _dev(case, gpu)
    before = _raw_bytes(t)
    outs = _guarded_outs(need + 9, m, gpu)
    untouched = _raw_bytes(outs)
    # one too small: the need, and not a byte of the rows' flags or of any output changes
    assert _raw_place(t, outs, need - 1, gpu) == (_lib.SF_ENOSPC, need, case["row_present"].count(0), mismatch)
    assert _raw_bytes(t) == before and _raw_bytes(outs) == untouched
    # a query: no lists at all
    nothing = dict.fromkeys(outs)
    assert _raw_place(t, nothing, 1 << 40, gpu)[:2] == (_lib.SF_ENOSPC, need)
    assert _raw_bytes(t) == before
    # exactly enough: the first `need` entries, the m counters, and nothing behind either
    assert _raw_place(t, outs, need, gpu) == (0, need, n_left, mismatch)
    for k, col in (("src", 0), ("dst", 1), ("sizes", 2), ("rows", 3), ("msgs", 4)):
        got = outs[k].cpu().numpy()
        assert (got.view(np.uint32) if k == "sizes" else got)[:need].tolist() == [j[col] for j in jobs], k
        assert set(got[need:].view(np.uint8).tolist()) == {GUARD}, k
    got = outs["uses"].cpu().numpy()
    assert got[:m].tolist() == uses and set(got[m:].view(np.uint8).tolist()) == {GUARD}
    assert t["row_present"].tolist() == present
    # the inputs are read only
    after = _raw_bytes(t)
    assert {k: v for k, v in after.items() if k != "row_present"} == \
        {k: v for k, v in before.items() if k != "row_present"}


# -------------------------------------------------------------- stream order

def _behind_a_hold(gpu, real, decoy, call, want):
    """`call(x, stream)` with its inputs still in production behind a hold on
    a fresh stream (stream_order.py); `want` is the result for `real`."""
    to = lambda a: {k: torch.from_numpy(v).to(gpu) for k, v in a.items()}  # noqa: E731
    real_t, decoy_t = to(real), to(decoy)
    first = tuple(r.cpu().numpy() if isinstance(r, torch.Tensor) else r for r in call(real_t, None))
    assert so.same(first, want), so.first_difference(first, want)
    H = so.hold_ms(so.timed_ms(lambda: call(real_t, None), gpu))
    S = so.fresh_stream(gpu)
    x, _o = so.pending(S, real_t, decoy_t, H)
    got = so.settle(S, x, decoy_t, call(x, S))
    assert so.same(got, want), so.first_difference(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("distinct", [False, True])
def test_requests_wait_for_inputs_pending_on_the_callers_stream(gpu, distinct):
    def inputs(seed):
        rng = np.random.default_rng(seed)
        digests = rng.integers(0, 256, (3000, 20), dtype=np.uint8)
        digests[rng.integers(0, 3000, 600)] = digests[rng.integers(0, 3000, 600)]
        return {"digests": digests, "rows": rng.choice(np.array([-1, -1, 4], np.int64), 3000),
                "take": (rng.random(3000) < 0.8).astype(np.uint8)}
    real, decoy = inputs(41), inputs(42)
    keep = []

    def call(x, s):
        run, n = device.get_block_requests(x["digests"], x["rows"], x["take"], distinct=distinct, stream=s)
        keep.append(run)  # alive until its tensor has been cloned
        return run.tensor(), n
    want = expected_requests([d.tobytes() for d in real["digests"]], real["rows"].tolist(), real["take"].tolist(),
                             distinct)
    assert want != expected_requests([d.tobytes() for d in decoy["digests"]], decoy["rows"].tolist(),
                                     decoy["take"].tolist(), distinct)
    _behind_a_hold(gpu, real, decoy, call, (np.frombuffer(want, np.uint8), len(want) // 31))
    for run in keep:
        run.close()


@pytest.mark.gpu
def test_the_join_waits_for_inputs_pending_on_the_callers_stream(gpu):
    def inputs(seed):
        c = _join_case(seed)
        return {"row_digests": np.frombuffer(b"".join(c["row_digests"]), np.uint8).reshape(-1, 20).copy(),
                "row_sizes": np.array(c["row_sizes"], np.uint32).view(np.int32),
                "row_dst": np.array(c["row_dst"], np.int64), "row_present": np.array(c["row_present"], np.uint8),
                "msg_digests": np.frombuffer(b"".join(c["msg_digests"]), np.uint8).reshape(-1, 20).copy(),
                "msg_sizes": np.array(c["msg_sizes"], np.uint32).view(np.int32),
                "msg_offsets": np.array(c["msg_offsets"], np.int64), "msg_ok": np.array(c["msg_ok"], np.uint8)}, c
    (real, case), (decoy, _c) = inputs(51), inputs(52)
    jobs, present, uses, n_left, mismatch = place_model(**case)

    def call(x, s):
        x = dict(x)
        if s is None:  # the call marks rows: the timing runs work on a copy
            x["row_present"] = x["row_present"].clone()
        return device.place_block_data(**x, stream=s) + (x["row_present"],)
    cols = [np.array([j[k] for j in jobs], np.int64) for k in range(5)]
    cols[2] = cols[2].astype(np.uint32).view(np.int32)
    want = (*cols, np.array(uses, np.int32), n_left, mismatch, np.array(present, np.uint8))
    _behind_a_hold(gpu, real, decoy, call, want)


# ------------------------------------------------- both routes, nothing forged

def _destination(gpu, old, s_dig, s_sizes):
    """The destination's index after the FILE_BLOCK run: (index, copies)."""
    d_offs, d_sizes, d_dig, _ = device.index_device_zpaq(_up(old, gpu))
    idx = Index.open_in_memory()
    old_id, _ = idx.add_file(PurePath("old.bin"), DateTimeUtc.from_ns(1))
    for o, s, d in zip(d_offs.cpu().tolist(), d_sizes.cpu().tolist(), d_dig.cpu().numpy()):
        idx.add_block(HashDigest(d.tobytes()), old_id, o, s)
    idx.commit()
    file_blocks = bytes(wire.blocks_device(s_dig, s_sizes).cpu().numpy())
    fid = idx.add_temp_file("new.bin")
    copies = idx.receive_file_blocks(fid, file_blocks + wire.write_message("FileEnd"), device=gpu)
    idx.commit()
    return idx, copies


def _blocks_table(idx):
    return idx.db.execute("SELECT rowid, * FROM blocks ORDER BY rowid;").fetchall()


@pytest.mark.gpu
def test_both_routes_end_to_end(gpu, tmp_path):
    """The exchange of test_source_and_destination_end_to_end on a source with
    a region held three times and 200 KB of zeros, through the old route and
    the new on copies of one index.  The zeros are cut into 931 blocks of 210
    bytes under one digest, and the old route runs list_block_locations for
    each of the 931 messages and gets 931 rows each time: 867,000 updates and
    write tuples in Python.  That loop alone takes 6 s on a CPU, of this test's
    7.7 s on an MI355X."""
    source, old = e2e_files()
    (tmp_path / "old.bin").write_bytes(old)
    name = temp_name("new.bin")
    src_t = _up(source, gpu)
    # the source's blocks: cut on the host (a run of zeros is the device cutter's slow case, and the cutter
    # is not what this test is about; the boundaries are the same), hashed on the device
    offs, sizes = host.zpaq_cut_buffer(source)
    s_offs = torch.from_numpy(offs.astype(np.int64)).to(gpu)
    s_sizes = torch.from_numpy(sizes.view(np.int32)).to(gpu)
    s_dig = device.index_device_blocks(src_t, s_offs, s_sizes)
    idx_a, copies = _destination(gpu, old, s_dig, s_sizes)
    idx_b, idx_c = Index.open_in_memory(), Index.open_in_memory()  # two copies of the index, one per route
    for other in (idx_b, idx_c):
        idx_a.db.backup(other.db)
    copies_b = copies_c = copies
    # the input is what this test is about, before anything else
    missing = idx_a.list_missing_blocks()
    assert len(missing) > len(set(missing)) and max(Counter(missing).values()) >= 3
    old_rows = idx_a.list_file_blocks(idx_a.get_file("old.bin")[0])
    assert copies and [h.bytes for h in missing] == missing_of([d.tobytes() for d in s_dig.cpu().numpy()],
                                                                 [r[0].bytes for r in old_rows])
    assert len(_blocks_table(idx_a)) == len(old_rows) + s_offs.numel()
    assert _blocks_table(idx_a) == _blocks_table(idx_b) == _blocks_table(idx_c)

    def answer(requests_t, bset):
        run, n_requests, n_answered, consumed, stop = bset.serve(requests_t, src_t, s_offs, s_sizes)
        assert n_requests == n_answered and consumed == 31 * n_requests
        return run, n_answered, stop

    def images_of(idx, copy_list):
        images = FileImages({name: len(source)}, device=gpu, root=tmp_path)
        assert images.apply_copies(name, copy_list) == 1
        return images

    with device.BlockSet(s_dig) as bset:
        # the old route: Python requests, the per-message loop, the host-sorted write list
        requests = b"".join(wire.write_message("GetBlock", h) for h in missing)
        run, n_a, stop = answer(_up(requests + wire.write_message("Complete"), gpu), bset)
        with run:
            assert (n_a, stop) == (len(missing), OTHER)
            data = run.bytes()
            writes, rejected, used = idx_a.receive_block_data(data, device=gpu)
            assert rejected == [] and used == len(data)
            images_a = images_of(idx_a, copies)
            assert images_a.apply_writes(writes, run.tensor()) == 1
        idx_a.commit()
        # the new route: the same requests from the device, the join on the device, one copy
        with idx_b.get_block_requests(device=gpu) as req:
            assert req.bytes() == requests and req.n_messages == len(missing)
            run, n_b, stop = answer(req.tensor(), bset)
        with run:
            assert (n_b, stop) == (len(missing), END) and run.bytes() == data
            images_b = images_of(idx_b, copies_b)
            assert idx_b.place_block_data(data, images_b, device=gpu) == (len(missing), [], len(data), 0)
        idx_b.commit()
        # one request per digest: fewer answers, the same file
        with idx_c.get_block_requests(device=gpu, distinct=True) as req:
            assert req.n_messages == len(set(missing)) and parsed_requests(req.bytes())[0] == \
                list(dict.fromkeys(h.bytes for h in missing))
            run, n_c, _stop = answer(req.tensor(), bset)
        with run:
            assert n_c == len(set(missing)) < n_b and run.nbytes < len(data)
            images_c = images_of(idx_c, copies_c)
            n_jobs, rejected, used, n_left = idx_c.place_block_data(run.bytes(), images_c, device=gpu)
            assert (n_jobs, rejected, used, n_left) == (len(missing), [], run.nbytes, 0)
        idx_c.commit()
    assert _blocks_table(idx_a) == _blocks_table(idx_b) == _blocks_table(idx_c)
    want = np.frombuffer(source, np.uint8)
    for idx, images in ((idx_a, images_a), (idx_b, images_b), (idx_c, images_c)):
        assert idx.list_missing_blocks() == [] and idx.missing_rows() == []
        assert [missing for _id, _n, missing in idx.check_temp_files()] == [False]
        assert np.array_equal(images.buffer.cpu().numpy(), images_a.buffer.cpu().numpy())
        assert np.array_equal(images.image(name).cpu().numpy(), want)
        assert images.check(idx, name) == []
    path = tmp_path / name
    fd = os.open(path, os.O_RDWR | os.O_CREAT)
    try:
        assert images_b.write(name, fd) == len(source)
    finally:
        os.close(fd)
    assert path.read_bytes() == source


@pytest.mark.gpu
def test_index_place_block_data_rejects_what_receive_block_data_rejects(gpu):
    rng = random.Random(61)
    blocks = [rng.randbytes(rng.randrange(100, 2000)) for _ in range(6)]
    at = sum(len(b) for b in blocks)

    def index():
        idx = Index.open_in_memory()
        fid = idx.add_temp_file("f.bin")
        for k, b in enumerate(blocks):
            idx.add_missing_block(HashDigest(hashlib.sha1(b).digest()), fid, sum(len(x) for x in blocks[:k]), len(b))
        idx.commit()
        return idx
    idx, other = index(), index()
    images = FileImages({temp_name("f.bin"): at}, device=gpu)
    msgs = [wire.write_message("BlockData", hashlib.sha1(b).digest(), b) for b in blocks]
    spoilt = bytearray(msgs[2])
    spoilt[-5] ^= 1
    data = b"".join(msgs[:2]) + bytes(spoilt) + msgs[3] + msgs[4][:50]  # one corrupt, one cut, one never sent
    _w, want_rejected, want_used = other.receive_block_data(data, device=gpu)
    n_jobs, rejected, used, n_left = idx.place_block_data(data, images, device=gpu)
    assert (n_jobs, rejected, used, n_left) == (3, want_rejected, want_used, 3)
    assert rejected == [HashDigest(hashlib.sha1(blocks[2]).digest())]
    idx.commit()
    other.commit()
    assert _blocks_table(idx) == _blocks_table(other)
    want = bytearray(at)
    for k in (0, 1, 3):
        o = sum(len(b) for b in blocks[:k])
        want[o:o + len(blocks[k])] = blocks[k]
    assert images.image(temp_name("f.bin")).cpu().numpy().tobytes() == bytes(want)
    for bad in (b"".join(msgs[:2]) + b"NOPE\n", b"".join(msgs[:2]) + wire.write_message("Complete")):
        with pytest.raises(wire.ProtocolError):
            idx.place_block_data(bad, images, device=gpu)
    assert len(idx.missing_rows()) == 3
