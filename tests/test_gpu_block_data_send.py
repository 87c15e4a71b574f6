"""GPU: BLOCK_DATA runs built on the device (wire.block_data_device,
sf_wire_block_data_device) and a received GET_BLOCK run answered in one call
(device.BlockSet.serve, sf_serve_get_blocks_device).  Every expected value is
wire.write_message's, wire.Parser's (send_expect.py, data_expect.py),
hashlib's, oracle.block_lookup's or the Index mirror's."""
import ctypes
import hashlib
import os
import random
import signal
import threading
from pathlib import PurePath

import numpy as np
import pytest
import torch

import oracle
from data_expect import expected, header, message
from send_expect import END, INCOMPLETE, MALFORMED, OTHER, OTHERS, expected_requests, get_block, hostile_requests
from syncfast_amd import _lib, device, wire
from syncfast_amd.assemble import FileImages
from syncfast_amd.digest import HashDigest
from syncfast_amd.index import Index, temp_name
from syncfast_amd.timestamp import DateTimeUtc

U8 = torch.uint8


def _up(b: bytes, gpu, dtype=U8):
    return torch.frombuffer(bytearray(b), dtype=dtype).to(gpu) if b else torch.empty(0, dtype=dtype, device=gpu)


def _lists(jobs, digests, gpu):
    """(digests uint8[n, 20], offsets int64[n], sizes int32[n]) on the device."""
    offs = torch.tensor([o for o, _ in jobs], dtype=torch.int64, device=gpu)
    sizes = torch.from_numpy(np.array([s for _, s in jobs], np.uint32).view(np.int32)).to(gpu)
    return _up(b"".join(digests), gpu).reshape(-1, 20), offs, sizes


def _want(src: bytes, jobs, digests) -> bytes:
    return b"".join(wire.write_message("BlockData", d, src[o:o + s]) for (o, s), d in zip(jobs, digests))


SRC_LEN = 1_300_000
SIZES = [0, 1, 2, 9, 10, 15, 16, 17, 99, 100, 999, 1000, 4095, 4096, 4097, 9999, 10000, 99999, 100000, 1000000]


@pytest.fixture(scope="module")
def case(gpu):
    """The job list of the byte-exact test, with true SHA-1 digests, built
    once: (source bytes, jobs, digests, expected run, the built run)."""
    rng = random.Random(101)
    src = bytearray(rng.randbytes(SRC_LEN))
    nested = message(rng.randbytes(300)) + message(b"")  # a payload that is itself whole messages
    forged = header(5000) + rng.randbytes(20)            # and one that is a header announcing more than there is
    src[70_000:70_000 + len(nested)] = nested
    src[80_003:80_003 + len(forged)] = forged
    src = bytes(src)
    jobs = []
    for i, s in enumerate(SIZES):
        jobs.append((rng.randrange(0, SRC_LEN - s - 15) // 16 * 16 + (5 * i) % 16, s))
    for j in range(64):  # sizes 33 .. 96, every source residue mod 16 four times, neighbours overlapping
        jobs.append((200_000 + 48 * j + j % 16, 33 + j))
    jobs[0] = (0, 0)
    jobs[3] = (0, 9)                          # one starts at byte 0
    jobs[12] = (SRC_LEN - 4095, 4095)         # one ends exactly at src_len
    jobs += [jobs[30], jobs[5]]               # two repeat
    jobs.append((70_000, len(nested)))
    jobs.append((80_003, len(forged)))
    digests = [hashlib.sha1(src[o:o + s]).digest() for o, s in jobs]
    src_t = _up(src, gpu)
    lists = _lists(jobs, digests, gpu)
    before = [t.clone() for t in (src_t, *lists)]
    run = wire.block_data_device(src_t, *lists)
    torch.cuda.synchronize()
    yield {"src": src, "src_t": src_t, "jobs": jobs, "digests": digests, "lists": lists, "before": before,
           "want": _want(src, jobs, digests), "run": run}
    run.close()


@pytest.mark.gpu
def test_the_run_is_write_messages_byte_for_byte(case):
    run, want, jobs = case["run"], case["want"], case["jobs"]
    assert run.n_messages == len(jobs) and run.nbytes == len(want)
    got = run.bytes()
    assert hashlib.sha1(got).digest() == hashlib.sha1(want).digest() and got == want
    assert run.bytes(5, 40) == want[5:45] and run.bytes(run.nbytes, 0) == b""
    # every phase of a payload's first byte against the copy's 16-byte stores, source and destination
    _d, _s, offsets, _c, _st, _n = expected(want)
    assert {(case["src_t"].data_ptr() + o) % 16 for o, s in jobs if s} == set(range(16))
    assert {(run.data_ptr + o) % 16 for o, (_, s) in zip(offsets, jobs) if s} == set(range(16))
    assert {s for _, s in jobs} >= set(SIZES) | set(range(33, 97))
    assert any(a < b + sb and b < a + sa for (a, sa), (b, sb) in zip(jobs[20:83], jobs[21:84]))  # overlaps
    # the inputs are as they were
    for t, b in zip((case["src_t"], *case["lists"]), case["before"]):
        assert torch.equal(t, b)


@pytest.mark.gpu
def test_the_run_goes_through_the_receiver(case):
    run, want, jobs = case["run"], case["want"], case["jobs"]
    digests, sizes, offsets, ok, consumed, stop, need = run.receive()
    w_digests, w_sizes, w_offsets, w_consumed, w_stop, _ = expected(want)
    assert len(w_sizes) == len(jobs) and w_sizes == [s for _, s in jobs]
    assert digests.cpu().numpy().tobytes() == b"".join(w_digests) == b"".join(case["digests"])
    assert sizes.cpu().numpy().astype(np.int64).tolist() == w_sizes
    assert offsets.cpu().numpy().tolist() == w_offsets
    assert ok.cpu().numpy().tolist() == [1] * len(jobs)
    assert (consumed, stop, need) == (run.nbytes, END, 0) == (w_consumed, w_stop, 0)
    # the payloads that look like messages came out whole
    t = run.tensor()
    assert t.dtype == U8 and t.is_cuda and t.numel() == run.nbytes and t.data_ptr() == run.data_ptr
    for k in (-2, -1):
        o, s = jobs[k]
        assert bytes(t[w_offsets[k]:w_offsets[k] + s].cpu().numpy()) == case["src"][o:o + s]


@pytest.mark.gpu
def test_a_run_past_4_gib(gpu):
    size, n = 32 << 20, 130
    src_t = device.splitmix_tensor(size + 160, 7, gpu)
    jobs = [(k + (k > 64) * 17, size) for k in range(n)]  # every job from another byte offset
    assert len({o for o, _ in jobs}) == n and max(o for o, _ in jobs) + size <= size + 160
    offs = torch.tensor([o for o, _ in jobs], dtype=torch.int64, device=gpu)
    sizes = torch.full((n,), size, dtype=torch.int32, device=gpu)
    # the digests are inputs: the library's explicit-list kernel, held against hashlib on three jobs
    dig = device.index_device_blocks(src_t, offs, sizes)
    src = src_t.cpu().numpy().tobytes()
    dig_h = dig.cpu().numpy()
    for k in (0, 65, n - 1):
        assert dig_h[k].tobytes() == hashlib.sha1(src[jobs[k][0]:jobs[k][0] + size]).digest()
    with wire.block_data_device(src_t, dig, offs, sizes) as run:
        per = 34 + 8 + size
        assert run.n_messages == n and run.nbytes == n * per > 1 << 32
        cap = 256
        digests = torch.empty((cap, 20), dtype=U8, device=gpu)
        o_sizes = torch.empty(cap, dtype=torch.int32, device=gpu)
        o_offs = torch.empty(cap, dtype=torch.int64, device=gpu)
        ok = torch.zeros(cap, dtype=U8, device=gpu)
        n_out, consumed, need, n_bad = (ctypes.c_uint64(9) for _ in range(4))
        stop = ctypes.c_int(9)
        _lib.check(_lib.lib().sf_receive_block_data_device(
            run.data_ptr, run.nbytes, digests.data_ptr(), o_sizes.data_ptr(), o_offs.data_ptr(), ok.data_ptr(), cap,
            ctypes.byref(n_out), ctypes.byref(consumed), ctypes.byref(stop), ctypes.byref(need), ctypes.byref(n_bad),
            torch.cuda.current_stream(gpu).cuda_stream), "sf_receive_block_data_device")
        assert (n_out.value, consumed.value, stop.value, need.value, n_bad.value) == (n, run.nbytes, END, 0, 0)
        assert ok[:n].cpu().numpy().tolist() == [1] * n
        assert torch.equal(digests[:n], dig)
        msg = {k: wire.write_message("BlockData", dig_h[k].tobytes(), src[jobs[k][0]:jobs[k][0] + size])
               for k in (0, 65, n - 1)}
        assert len(msg[0]) == per
        assert o_offs[:n].cpu().numpy().tolist() == [k * per + per - size - 1 for k in range(n)]
        assert run.bytes(0, 64) == msg[0][:64] and run.bytes(run.nbytes - 64, 64) == msg[n - 1][-64:]
        # a message that starts past 2^31 and one past 2^32
        assert 65 * per > 1 << 31 and (n - 1) * per > 1 << 32
        assert run.bytes(65 * per, 64) == msg[65][:64] and run.bytes(66 * per - 64, 64) == msg[65][-64:]
        assert run.bytes((n - 1) * per, 64) == msg[n - 1][:64]


@pytest.mark.gpu
def test_a_job_out_of_range_builds_nothing(gpu):
    rng = random.Random(102)
    src = rng.randbytes(5000)
    src_t = _up(src, gpu)
    good = [(0, 100), (4800, 200), (17, 0)]
    L = _lib.lib()
    s = torch.cuda.current_stream(gpu).cuda_stream
    for bad in ((4801, 200), ((1 << 64) - 100 - (1 << 64), 200), (5001, 0), (0, 5001)):
        jobs = good + [bad] + good
        dig, offs, sizes = _lists(jobs, [bytes(20)] * len(jobs), gpu)
        h = ctypes.c_void_p(7)
        rc = L.sf_wire_block_data_device(src_t.data_ptr(), len(src), dig.data_ptr(), offs.data_ptr(), sizes.data_ptr(),
                                         len(jobs), ctypes.byref(h), s)
        assert rc == _lib.SF_ERANGE and h.value is None, bad
        with pytest.raises(_lib.SfError) as e:
            wire.block_data_device(src_t, dig, offs, sizes)
        assert e.value.code == _lib.SF_ERANGE
        # the stream is fine: a good call right behind it
        digests = [rng.randbytes(20) for _ in good]
        with wire.block_data_device(src_t, *_lists(good, digests, gpu)) as run:
            assert run.bytes() == _want(src, good, digests)


@pytest.mark.gpu
def test_the_build_follows_its_stream(gpu):
    n = 256 << 20
    src_t = torch.zeros(n, dtype=U8, device=gpu)
    torch.cuda.synchronize()
    rng = random.Random(103)
    jobs = [(rng.randrange(0, n - 3000), rng.randrange(1, 3000)) for _ in range(40)] + [(n - 777, 777), (0, 50)]
    digests = [rng.randbytes(20) for _ in jobs]
    side = torch.cuda.Stream(gpu)
    with torch.cuda.stream(side):
        lists = _lists(jobs, digests, gpu)
    device.fill_splitmix(src_t, 21, stream=side)
    run = wire.block_data_device(src_t, *lists, stream=side)  # no synchronisation between the two
    got = run.bytes()
    side.synchronize()
    want = b"".join(wire.write_message("BlockData", d, oracle.splitmix_bytes(s, 21, o).tobytes())
                    for (o, s), d in zip(jobs, digests))
    assert got == want
    run.close()


@pytest.mark.gpu
def test_to_fd_through_three_stages(gpu, knobs, tmp_path):
    knobs.set("SF_TEST_STREAM_STAGE_MIB", 1)
    rng = random.Random(104)
    src = rng.randbytes(900_000)
    jobs = [(0, 900_000), (11, 870_000), (50_001, 849_999), (3, 0), (899_999, 1)]
    digests = [rng.randbytes(20) for _ in jobs]
    want = _want(src, jobs, digests)
    assert 2 << 20 < len(want) <= 3 << 20  # three stages of 1 MiB
    old = signal.signal(signal.SIGPIPE, signal.SIG_IGN)
    try:
        with wire.block_data_device(_up(src, gpu), *_lists(jobs, digests, gpu)) as run:
            r, w = os.pipe()
            got = []

            def drain():
                while True:
                    b = os.read(r, 1 << 16)
                    if not b:
                        return
                    got.append(b)
            t = threading.Thread(target=drain)
            t.start()
            try:
                assert run.to_fd(w) == len(want)
            finally:
                os.close(w)
                t.join()
                os.close(r)
            assert b"".join(got) == want
            path = tmp_path / "run.bin"
            with open(path, "wb") as f:
                f.write(b"head")
                f.flush()
                assert run.to_fd(f.fileno()) == len(want)  # from the descriptor's position on
            assert path.read_bytes() == b"head" + want
            r, w = os.pipe()
            os.close(r)
            try:
                with pytest.raises(_lib.SfError) as e:
                    run.to_fd(w)
                assert e.value.code == _lib.SF_EIO and e.value.written == 0
            finally:
                os.close(w)
            assert run.bytes() == want  # and the run is still whole
    finally:
        signal.signal(signal.SIGPIPE, old)


# ------------------------------------------------------------------ serve

@pytest.fixture(scope="module")
def served(gpu):
    """A source of 300 rows: labels (not hashes) as digests, so that rows
    sharing one differ in their bytes; every fifth label doubles an earlier
    one, some rows are not present, some labels only have rows that are not."""
    rng = random.Random(105)
    n = 300
    src = rng.randbytes(40_000)
    rows = [(rng.randrange(0, len(src) - 400), rng.choice([0, 1, 31, 64, 100, 257, 399])) for _ in range(n)]
    labels = [rng.randbytes(20) for _ in range(n)]
    for i in range(5, n, 5):
        labels[i] = labels[rng.randrange(0, i)]
    present = np.array([rng.random() < 0.8 for _ in range(n)])
    table = np.frombuffer(b"".join(labels), np.uint8).reshape(n, 20)
    first = oracle.block_lookup(table, present, table)  # per row: the row the reference answers its label with
    known = sorted({labels[i] for i in range(n) if first[i] >= 0})
    unknown = sorted({labels[i] for i in range(n) if first[i] < 0})
    assert len(unknown) >= 10 and any(first[i] not in (-1, i) for i in range(n))
    table_t = _up(table.tobytes(), gpu).reshape(n, 20)
    bset = device.BlockSet(table_t, torch.from_numpy(present).to(gpu))
    offs = torch.tensor([o for o, _ in rows], dtype=torch.int64, device=gpu)
    sizes = torch.tensor([s for _, s in rows], dtype=torch.int32, device=gpu)

    def answer(digests):
        """What the reference's loop sends for these requests, all known."""
        found = oracle.block_lookup(table, present, np.frombuffer(b"".join(digests), np.uint8).reshape(-1, 20))
        assert (found >= 0).all()
        return b"".join(wire.write_message("BlockData", d, src[rows[r][0]:rows[r][0] + rows[r][1]])
                        for d, r in zip(digests, found))

    def serve(requests: bytes):
        return bset.serve(_up(requests, gpu), src_t, offs, sizes)
    src_t = _up(src, gpu)
    yield {"known": known, "unknown": unknown, "answer": answer, "serve": serve, "rng": rng}
    bset.close()


@pytest.mark.gpu
def test_serve_answers_every_request(served):
    rng = served["rng"]
    asked = served["known"] * 2 + served["known"][:40] * 3  # repeats are answered each time
    rng.shuffle(asked)
    n = len(asked)
    assert n > 512  # more than one workgroup of slots
    requests = b"".join(get_block(d) for d in asked) + wire.write_message("Complete")
    run, n_requests, n_answered, consumed, stop = served["serve"](requests)
    with run:
        assert (n_requests, n_answered, consumed, stop) == (n, n, 31 * n, OTHER)
        assert run.n_messages == n and run.bytes() == served["answer"](asked)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "second", "last"])
def test_serve_stops_at_an_unknown_digest(served, where):
    asked = list(served["known"][:70])
    n = len(asked)
    k = {"first": 0, "second": 1, "last": n - 1}[where]
    asked[k] = served["unknown"][k % len(served["unknown"])]
    if k + 5 < n:
        asked[k + 5] = served["unknown"][3]  # a later one changes nothing
    run, n_requests, n_answered, consumed, stop = served["serve"](b"".join(get_block(d) for d in asked))
    with run:
        assert (n_requests, n_answered, consumed, stop) == (n, k, 31 * n, END)
        assert run.n_messages == k and run.bytes() == served["answer"](asked[:k])


@pytest.mark.gpu
def test_serve_stop_classes_are_wire_parsers(served):
    known = served["known"]
    three = b"".join(get_block(d) for d in known[:3])
    runs = [b"", three, three + b"COMPLETE\n"]
    runs += [three[:62 + k] for k in range(1, 31)]                       # every proper prefix of the last request
    runs += [three[:k] for k in (1, 9, 10, 30)]
    runs += [three[:92] + b"x", three[:61] + b"\0" + three[62:], three + b"NOPE\n", three + b"A" * 20, three + b"A" * 19]
    runs += [three + o + b"\n" + bytes(40) for o in OTHERS]
    runs += [get_block(b"GET_BLOCK\nGET_BLOCK\n") + three, get_block(b"\n" * 20) + three]  # unknown digests of tags and newlines
    rng = random.Random(106)
    runs += [hostile_requests(rng) for _ in range(40)]
    stops, prefixes = set(), 0
    for req in runs:
        digests, w_consumed, w_stop = expected_requests(req)
        answered = next((i for i, d in enumerate(digests) if d not in known), len(digests))
        run, n_requests, n_answered, consumed, stop = served["serve"](req)
        with run:
            assert (n_requests, n_answered, consumed, stop) == (len(digests), answered, w_consumed, w_stop), req
            assert run.bytes() == served["answer"](digests[:answered]), req
        stops.add(stop)
        prefixes += w_stop == INCOMPLETE and len(digests) == 2 and req[:62] == three[:62]
    assert stops == {END, INCOMPLETE, OTHER, MALFORMED} and prefixes == 30


@pytest.mark.gpu
def test_serve_with_an_empty_set_and_an_empty_run(gpu, served):
    empty = device.BlockSet(torch.empty((0, 20), dtype=U8, device=gpu))
    none64, none32 = torch.empty(0, dtype=torch.int64, device=gpu), torch.empty(0, dtype=torch.int32, device=gpu)
    req = _up(get_block(bytes(20)) * 2, gpu)
    run, n_requests, n_answered, consumed, stop = empty.serve(req, torch.empty(0, dtype=U8, device=gpu), none64, none32)
    assert (run.nbytes, run.n_messages, n_requests, n_answered, consumed, stop) == (0, 0, 2, 0, 62, END)
    assert run.bytes() == b"" and run.tensor().numel() == 0 and run.to_fd(1) == 0
    run.close()
    run.close()
    with pytest.raises(ValueError):
        run.bytes()
    run, *rest = served["serve"](b"")
    assert rest == [0, 0, 0, END] and run.nbytes == 0
    empty.close()


# ------------------------------------------------ both sides, nothing forged

@pytest.mark.gpu
def test_source_and_destination_end_to_end(gpu, tmp_path):
    rng = random.Random(107)
    source = rng.randbytes(600_000)
    old = rng.randbytes(30_000) + source[100_000:350_000] + rng.randbytes(20_000)
    (tmp_path / "old.bin").write_bytes(old)
    # the source indexes its file on the device, content-defined blocks
    src_t = _up(source, gpu)
    s_offs, s_sizes, s_dig, _bh = device.index_device_zpaq(src_t)
    assert s_offs.numel() > 40
    # the destination indexed what it holds the same way
    d_offs, d_sizes, d_dig, _ = device.index_device_zpaq(_up(old, gpu))
    idx = Index.open_in_memory()
    old_id, _ = idx.add_file(PurePath("old.bin"), DateTimeUtc.from_ns(1))
    for o, s, d in zip(d_offs.cpu().tolist(), d_sizes.cpu().tolist(), d_dig.cpu().numpy()):
        idx.add_block(HashDigest(d.tobytes()), old_id, o, s)
    idx.commit()
    # source -> destination: the FILE_BLOCK run; BlockSet.receive sorts it into copies and missing blocks
    file_blocks = bytes(wire.blocks_device(s_dig, s_sizes).cpu().numpy())
    fid = idx.add_temp_file("new.bin")
    copies = idx.receive_file_blocks(fid, file_blocks + wire.write_message("FileEnd"), device=gpu)
    idx.commit()
    missing = idx.list_missing_blocks()
    assert copies and missing and len(copies) + len(missing) == s_offs.numel()
    # destination -> source: the requests
    requests = b"".join(wire.write_message("GetBlock", h) for h in missing) + wire.write_message("Complete")
    # source: the answer, in one call
    with device.BlockSet(s_dig) as bset:
        run, n_requests, n_answered, consumed, stop = bset.serve(_up(requests, gpu), src_t, s_offs, s_sizes)
    assert (n_requests, n_answered, consumed, stop) == (len(missing), len(missing), 31 * len(missing), OTHER)
    with run:
        # source -> destination: the BLOCK_DATA run
        data = run.bytes()
        writes, rejected, used = idx.receive_block_data(data, device=gpu)
        assert rejected == [] and used == len(data) and idx.list_missing_blocks() == []
        images = FileImages({temp_name("new.bin"): len(source)}, device=gpu, root=tmp_path)
        assert images.apply_copies(temp_name("new.bin"), copies) == 1
        assert images.apply_writes(writes, run.tensor()) == 1
    assert images.check(idx, temp_name("new.bin")) == []
    path = tmp_path / temp_name("new.bin")
    fd = os.open(path, os.O_RDWR | os.O_CREAT)
    try:
        assert images.write(temp_name("new.bin"), fd) == len(source)
    finally:
        os.close(fd)
    assert path.read_bytes() == source
