"""GPU: the source's whole answer to a list of GET_FILE requests built on the
device (wire.files_device, sf_wire_files_device; sf_send_files.hip), then
through FilesRun.receive and Index.serve_get_files with the destination's half
(sf_receive_files_device) behind it, nothing forged.  Every expected byte is
wire.write_message's (send_files_expect.py); lookups are oracle.block_lookup's."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import oracle
import stream_order as so
from placement import PATTERNS, Arena
from send_files_expect import (NO_FILE, csr, expected, files_with_messages, first_bad_file, parse_back, reference_loop,
                                source_index, table)
from syncfast_amd import _lib, device, wire
from syncfast_amd.index import Index

U8, I32, I64 = torch.uint8, torch.int32, torch.int64


def _arrays(digests, sizes, first, names, name_at):
    """The call's five arrays as numpy, in wire.files_device's order."""
    return {"digests": np.frombuffer(b"".join(digests), np.uint8).reshape(len(digests), 20).copy(),
            "sizes": np.array(sizes, np.uint32).view(np.int32), "first": np.array(first, np.int64),
            "names": np.frombuffer(names, np.uint8).copy(), "name_at": np.array(name_at, np.int64)}


def _tensors(arrays, gpu):
    return {k: torch.from_numpy(v).to(gpu) for k, v in arrays.items()}


def _call(t, stream=None):
    return wire.files_device(t["digests"], t["sizes"], t["first"], t["names"], t["name_at"], stream=stream)


def _check(files, gpu):
    """The device run of a case against write_message; returns the bytes."""
    want, _starts, _ends, blocks = expected(files)
    with _call(_tensors(_arrays(*csr(files)), gpu)) as run:
        got = run.bytes()
        assert (run.nbytes, run.n_messages) == (len(want), len(blocks) + 2 * len(files))
        assert got == want, files
        assert run.tensor().cpu().numpy().tobytes() == want
    return got


# --------------------------------------------------------- table and random sets

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(table()))
def test_the_table_is_write_messages(gpu, name):
    files = table()[name]
    assert parse_back(_check(files, gpu)) == files


@pytest.mark.gpu
@pytest.mark.parametrize("total", [63, 64, 65, 255, 256, 257, 3000])
def test_random_sets_across_lane_wave_and_workgroup_edges(gpu, total):
    files = files_with_messages(random.Random(total), total)
    assert sum(len(r) + 2 for _n, r in files) == total
    assert parse_back(_check(files, gpu)) == files


# -------------------------------------------------------------------- the search

@pytest.mark.gpu
def test_every_block_finds_its_file(gpu):
    rng = random.Random(3)
    row = lambda: (rng.randbytes(20), rng.randrange(1 << 32))  # noqa: E731
    # one file of 1,000 blocks between two empty files
    _check([(b"before", []), (b"big", [row() for _ in range(1000)]), (b"after", [])], gpu)
    # 300 files of exactly one block: every lane of a wave in a file of its own, names of every length
    _check([(b"n" * (k % 101), [row()]) for k in range(300)], gpu)
    # 500 empty files, then one block in the last file
    _check([(b"e%d" % k, []) for k in range(500)] + [(b"last", [row()])], gpu)
    # empty files in runs of every length up to 70 between files of one or two blocks
    files = []
    for k in range(70):
        files += [(b"", [])] * k + [(b"f%d" % k, [row() for _ in range(1 + k % 2)])]
    _check(files, gpu)


# ------------------------------------------------------ inputs at odd placements

@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("names_phase", [0, 1, 2, 3])
def test_inputs_at_their_minimum_alignment_stay_as_they_are(gpu, pattern, names_phase):
    """Every input carved from one patterned allocation: the names at each
    base phase mod 4, digests and sizes 4 bytes past a 256-byte boundary, the
    CSRs 8 past.  The run is exact, and the allocation -- inputs and the guards
    around them -- is bit for bit what it was: the call writes no input."""
    files = files_with_messages(random.Random(40 + names_phase), 400)
    want = expected(files)[0]
    arrays = _arrays(*csr(files))
    a = Arena(gpu, pattern, capacity=1 << 17)
    phases = {"digests": 4, "sizes": 4, "first": 8, "names": names_phase, "name_at": 8}
    t = {}
    for k, v in arrays.items():
        t[k] = a.carve(k, v.nbytes, torch.from_numpy(v).dtype, phases[k]).view(v.shape)
        t[k].copy_(torch.from_numpy(v))
    a.watch(**t)
    with _call(t) as run:
        assert run.bytes() == want
    a.check({k: v for k, v in arrays.items()})


# ---------------------------------------------------------------------- refusals

def _raw(t, n_blocks, n_files, gpu):
    """sf_wire_files_device itself: (rc, handle, bad_file)."""
    h, bad = ctypes.c_void_p(7), ctypes.c_uint64(7)
    p = lambda x: x.data_ptr() if x.numel() else None  # noqa: E731
    rc = _lib.lib().sf_wire_files_device(p(t["digests"]), p(t["sizes"]), n_blocks, p(t["first"]), p(t["names"]),
                                         p(t["name_at"]), n_files, ctypes.byref(h), ctypes.byref(bad),
                                         torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize(gpu)
    return rc, h.value, bad.value


@pytest.mark.gpu
def test_bad_entries_are_refused_with_the_first_bad_file(gpu):
    rng = random.Random(8)
    # more files than one workgroup of lanes, every name of two bytes or more
    good = [(b"f%d" % k + b"x" * (k % 7), [(rng.randbytes(20), rng.randrange(1 << 32)) for _ in range(k % 3)])
            for k in range(400)]
    base = csr(good)
    want = expected(good)[0]
    m, nb = len(good), len(base[0])
    long_name = next(f for f in range(300, m) if base[4][f + 1] - base[4][f] >= 2)  # a file past the first workgroup

    def changed(first=(), name_at=(), newline_in=(), grow=None):
        digests, sizes, fi, names, na = base[0], base[1], list(base[2]), bytearray(base[3]), list(base[4])
        for i, v in first:
            fi[i] = v
        for i, v in name_at:
            na[i] = v
        for f in newline_in:
            names[na[f + 1] - 1] = 0x0A  # its last byte
        if grow is not None:  # file `grow` gets a name of 101 bytes
            add = 101 - (na[grow + 1] - na[grow])
            names[na[grow + 1]:na[grow + 1]] = b"g" * add
            na = na[:grow + 1] + [v + add for v in na[grow + 1:]]
        return digests, sizes, fi, bytes(names), na
    f = next(f for f in range(5, m) if base[2][f + 1] > base[2][f])  # a file with blocks
    cases = {
        "first decreasing": changed(first=[(f + 1, base[2][f] - 1)] if base[2][f] else [(f + 1, 0)]),
        "first does not end at n_blocks": changed(first=[(m, nb + 1)]),
        "first[0] is not 0": changed(first=[(0, 1)]),
        "name_at decreasing": changed(name_at=[(long_name + 1, base[4][long_name] - 1)]),
        "a name of 101 bytes": changed(grow=long_name),
        "a newline in a name": changed(newline_in=[long_name]),
        "two bad files": changed(newline_in=[long_name, 290], grow=long_name + 3),
    }
    seen = set()
    for name, c in cases.items():
        bad = first_bad_file(c[2], c[3], c[4], nb)  # the header's rule, file by file
        assert bad != NO_FILE, name
        seen.add(bad)
        t = _tensors(_arrays(*c), gpu)
        assert _raw(t, nb, m, gpu) == (_lib.SF_EINVAL, None, bad), name
        with pytest.raises(ValueError, match=f"file {bad}:"):
            _call(t)
        # a following good call is exact
        rc, h, none = _raw(_tensors(_arrays(*base), gpu), nb, m, gpu)
        assert (rc, none) == (0, NO_FILE) and h
        with wire.FilesRun(ctypes.c_void_p(h), gpu) as run:
            assert run.bytes() == want
    assert first_bad_file(*cases["two bad files"][2:5], nb) == 290  # the smaller of the two
    assert {0, m - 1, long_name} <= seen and len(seen) >= 5
    # a name and no bytes for it
    t = _tensors(_arrays(*base), gpu)
    t["names"] = torch.empty(0, dtype=U8, device=gpu)
    first_named = next(f for f in range(m) if base[4][f + 1] > base[4][f])
    assert _raw(t, nb, m, gpu) == (_lib.SF_EINVAL, None, first_named)


# ------------------------------------------------------------------ stream order

@pytest.mark.gpu
def test_the_call_waits_for_inputs_pending_on_the_callers_stream(gpu):
    def inputs(seed):
        rng = random.Random(seed)
        # both have 150 files, 2,700 blocks and 3,000 name bytes: equal shapes, other contents
        counts = [0] * 150
        for _ in range(2700):
            counts[rng.randrange(150)] += 1
        lens = [20] * 150
        for _ in range(500):
            i, j = rng.randrange(150), rng.randrange(150)
            if i != j and lens[i] > 0 and lens[j] < 100:
                lens[i], lens[j] = lens[i] - 1, lens[j] + 1
        return [(bytes(rng.choice(b"abcdef/") for _ in range(n)), [(rng.randbytes(20), rng.randrange(1 << 32))
                                                                   for _ in range(c)]) for n, c in zip(lens, counts)]
    real, decoy = inputs(71), inputs(72)
    want = expected(real)[0]
    assert want != expected(decoy)[0]
    real_t, decoy_t = _tensors(_arrays(*csr(real)), gpu), _tensors(_arrays(*csr(decoy)), gpu)
    keep = []

    def call(x, s):
        run = _call(x, stream=s)
        keep.append(run)  # alive until its tensor has been cloned
        return run.tensor(), run.n_messages
    expect = (np.frombuffer(want, np.uint8), 2700 + 300)
    first = tuple(r.cpu().numpy() if isinstance(r, torch.Tensor) else r for r in call(real_t, None))
    assert so.same(first, expect), so.first_difference(first, expect)
    H = so.hold_ms(so.timed_ms(lambda: call(real_t, None), gpu))
    S = so.fresh_stream(gpu)
    x, _o = so.pending(S, real_t, decoy_t, H, shift={"digests": 4, "sizes": 4, "first": 8, "names": 1, "name_at": 8})
    got = so.settle(S, x, decoy_t, call(x, S))
    assert so.same(got, expect), so.first_difference(got, expect)
    for run in keep:
        run.close()


# ----------------------------------------------------- round trip, nothing forged

@pytest.mark.gpu
def test_the_run_round_trips_through_the_receiver(gpu):
    rng = random.Random(9)
    row = lambda: (rng.randbytes(20), rng.randrange(1 << 32))  # noqa: E731
    files = [(b"x/FILE_END", [row() for _ in range(40)]), (b"", []), (b"dir/a", [row() for _ in range(700)]),
             (b"FILE_START", [row()]), (b"empty", []), (b"n" * 100, [row() for _ in range(3)])]
    files[2][1][5] = files[0][1][7]  # one digest in two files
    digests, sizes, first, names, name_at = csr(files)
    want, starts, _ends, _blocks = expected(files)
    # the destination's table: half of the blocks, one of them twice and one not present, among strangers
    table_rows = digests[::2] + [digests[0]] + [rng.randbytes(20) for _ in range(50)]
    rng.shuffle(table_rows)
    present = [rng.random() < 0.9 for _ in table_rows]
    tab = np.frombuffer(b"".join(table_rows), np.uint8).reshape(-1, 20).copy()
    with _call(_tensors(_arrays(digests, sizes, first, names, name_at), gpu)) as run, \
            device.BlockSet(torch.from_numpy(tab).to(gpu), torch.tensor(present, device=gpu)) as bset:
        assert run.bytes() == want
        for r, rows_want in ((run.receive(bset), oracle.block_lookup(tab, np.array(present), np.array(
                [list(d) for d in digests], np.uint8))), (run.receive(), np.full(len(digests), -1, np.int64))):
            assert (r.consumed, r.stop, r.open) == (len(want), wire.SF_WIRE_END, False)
            assert r.digests.cpu().numpy().tobytes() == b"".join(digests)
            assert r.sizes.cpu().numpy().view(np.uint32).tolist() == sizes
            assert r.file_first.tolist() == first
            assert r.block_file.tolist() == [f for f, (_n, rows) in enumerate(files) for _ in rows]
            offsets = [sum(s for _d, s in rows[:k]) for _n, rows in files for k in range(len(rows))]
            assert r.offsets.tolist() == offsets
            assert r.file_size.tolist() == [sum(s for _d, s in rows) for _n, rows in files]
            assert r.name_at.tolist() == [s + 11 for s in starts]
            assert r.name_len.tolist() == [len(n) for n, _r in files]
            assert [want[a:a + n] for a, n in zip(r.name_at.tolist(), r.name_len.tolist())] == [n for n, _r in files]
            assert np.array_equal(r.rows.cpu().numpy(), rows_want)
        assert (rows_want < 0).all()
    # x/FILE_END holds a whole FILE_END, a candidate inside a message, which the receiver may settle on the host;
    # without such a name the same exchange stays on the device
    files = [f for f in files if f[0] not in (b"x/FILE_END", b"FILE_START")]
    with _call(_tensors(_arrays(*csr(files)), gpu)) as run:
        r = run.receive()
        assert (r.consumed, r.stop, r.file_first.tolist()) == (run.nbytes, wire.SF_WIRE_END, csr(files)[2])
        assert r.digests.cpu().numpy().tobytes() == b"".join(csr(files)[0]) and wire.recv_files_stats()[2] == 0


@pytest.mark.gpu
def test_the_run_goes_to_a_descriptor(gpu):
    files = files_with_messages(random.Random(10), 1000)
    want = expected(files)[0]
    assert len(want) < 60000  # fits a pipe's buffer: no reader thread is needed
    r, w = os.pipe()
    try:
        with _call(_tensors(_arrays(*csr(files)), gpu)) as run:
            assert run.to_fd(w) == len(want)
        os.close(w)
        w = None
        got = b""
        while chunk := os.read(r, 1 << 16):
            got += chunk
    finally:
        os.close(r)
        if w is not None:
            os.close(w)
    assert got == want


# -------------------------------------------------------------------- end to end

@pytest.mark.gpu
def test_index_serve_get_files_end_to_end(gpu):
    src, _added = source_index(random.Random(5))
    names = [b"dir/b.bin", b"dir/empty", b"a.bin", b"x/FILE_END", b"z"]
    want, n = src.serve_get_files(names)
    assert (want, n) == reference_loop(src, names) and n == len(names)
    run, n_dev = src.serve_get_files(names, device=gpu)
    with run:
        assert isinstance(run, wire.FilesRun) and n_dev == n
        assert run.bytes() == want and run.n_messages == len(wire.Parser().receive(want))
        data = run.bytes()
    # an unknown name in the middle, a repeated name, and nothing at all
    for asked in ([b"a.bin", b"nope", b"z"], [b"a.bin", b"a.bin", b"dir/empty"], [], [b"nope"]):
        run, k = src.serve_get_files(asked, device=gpu)
        with run:
            assert (run.bytes(), k) == src.serve_get_files(asked) == reference_loop(src, asked)
    # the destination takes the device-built stream and ends with the source's rows
    dst = Index.open_in_memory()
    for name in names:
        dst.add_temp_file(name.decode())
    dst.commit()
    copies, consumed, carry = dst.receive_files(data, device=gpu)
    dst.commit()
    assert (consumed, carry) == (len(data), None) and not any(copies.values())
    for name in names:
        got = dst.list_file_blocks(dst.get_temp_file(name.decode())[0])
        assert got == src.list_file_blocks(src.get_file(name.decode())[0]), name
    assert len(dst.list_missing_blocks()) == 5 + 70 + 3 + 1
