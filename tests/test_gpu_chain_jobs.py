"""GPU: the per-file blocks_hash chain jobs, driven directly through
sf_index_device_batch_chained_cols with sf_chain_job tables of arbitrary
bytes, against hashlib and the plain SHA-1 states of tests/chain_ref.py.

Two device routes take a job: alone (no batch: sha1_chain_helper_kernel, a
helper wave building schedules four chunks ahead) and beside a batch's blocks
(chain_job as wave 0 of the first workgroups of sha1_fixed_chained_kernel).
A third, one lane per file (sha1_chain_kernel), serves equal-size batches
whose runs are not 16-B aligned; it is reached through index_device_batch.

Every output table has a guard row before and after its files' rows, filled
with 0xA5 like the rows themselves; every check reads the whole table."""
import hashlib

import numpy as np
import pytest
import torch

import chain_ref
from syncfast_amd import device
from syncfast_amd._lib import ChainJob, lib

pytestmark = pytest.mark.gpu

BS = 64  # block size of every batch here
ROUTES = ["alone", "beside"]


def _rng(*key):
    return np.random.default_rng([0xC4A1] + [int(k) for k in key])


def _block_digests(host, bs=BS):
    """hashlib.sha1 of every bs-byte block of uint8[n * bs] -> uint8[n, 20]."""
    return chain_ref.run_hashes(host.reshape(-1, bs))


class Table:
    """uint8[rows + 2, 20] on the device, all 0xA5: `rows` rows for a job or
    a batch between two guard rows.  The library gets the address of row 1."""

    def __init__(self, rows, dev, fill=None):
        host = np.full((rows + 2, 20), 0xA5, np.uint8)
        if fill is not None:
            host[1:-1] = fill
        self.before = host
        self.t = torch.from_numpy(host.copy()).to(dev)
        self.ptr = self.t.data_ptr() + 20

    def rows(self, what=""):
        """The rows between the guards, once the guards are seen intact."""
        got = self.t.cpu().numpy()
        assert (got[0] == 0xA5).all() and (got[-1] == 0xA5).all(), ("guard row written", what)
        return got[1:-1]

    def untouched(self, what=""):
        assert np.array_equal(self.t.cpu().numpy(), self.before), ("table written", what)


class Runs:
    """A job's runs table: uint8[files, 20 * blocks] of the test's own bytes."""

    def __init__(self, host, dev):
        self.host = np.ascontiguousarray(host, np.uint8)
        self.files, self.run_len = self.host.shape
        self.blocks = self.run_len // 20
        self.t = torch.from_numpy(self.host.copy()).to(dev)
        assert self.t.data_ptr() % 16 == 0
        self.hashes = chain_ref.run_hashes(self.host)
        self.half = chain_ref.job_chunks(self.blocks)[2]
        self.state = chain_ref.state_bytes(chain_ref.state_after(self.host, self.half))

    def job(self, part, state=None, hashes=None):
        return ChainJob(self.t.data_ptr(), self.files, part, self.blocks, state.ptr if state else None,
                        hashes.ptr if hashes else None)

    def unchanged(self, what=""):
        assert np.array_equal(self.t.cpu().numpy(), self.host), ("runs table written", what)


def _random_runs(files, blocks, dev, *key):
    return Runs(_rng(files, blocks, *key).integers(0, 256, (files, 20 * blocks), dtype=np.uint8), dev)


class Batch:
    """files x nbf blocks of BS random bytes on the device, hashlib's digest
    of every block, and a guarded digest table per launch."""

    def __init__(self, files, nbf, dev, seed=0):
        self.files, self.nbf, self.dev = files, nbf, dev
        self.host = _rng(files, nbf, seed).integers(0, 256, files * nbf * BS, dtype=np.uint8)
        self.t = torch.from_numpy(self.host.copy()).to(dev)
        self.want = _block_digests(self.host).reshape(files, nbf, 20)

    def launch(self, jobs, cols=None, what=""):
        """One launch of columns `cols` (default: whole files) beside `jobs`;
        exactly the range's rows must then hold their digests."""
        lo, hi = cols if cols is not None else (0, self.nbf)
        table = Table(self.files * self.nbf, self.dev)
        _call(self.dev, jobs, self.t.data_ptr(), self.files, self.nbf * BS, lo, hi, table.ptr)
        got = table.rows(what).reshape(self.files, self.nbf, 20)
        assert np.array_equal(got[:, lo:hi], self.want[:, lo:hi]), ("block digests", what)
        assert (got[:, :lo] == 0xA5).all() and (got[:, hi:] == 0xA5).all(), ("rows outside the range", what)
        assert np.array_equal(self.t.cpu().numpy(), self.host), ("batch written", what)


def _call(dev, jobs, data=None, files=0, flen=BS, lo=0, hi=None, digests=None):
    arr = (ChainJob * 2)(*jobs)
    rc = lib().sf_index_device_batch_chained_cols(data, files, flen, BS, lo, flen // BS if hi is None else hi,
                                                  digests, arr, len(jobs), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc


@pytest.fixture(scope="module")
def small_batch(gpu):
    return Batch(5, 4, gpu)  # 20 blocks: one ragged block wave beside the chain waves


def _launch(route, gpu, small_batch, jobs, what=""):
    if route == "alone":
        _call(gpu, jobs)
    else:
        small_batch.launch(jobs, what=what)


# ------------------------------------------------------------ a. shapes

@pytest.mark.parametrize("files", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("route", ROUTES)
def test_every_part_at_every_small_shape(gpu, small_batch, route, files):
    # blocks 4 .. 64: 0, 16, 32 and 48 bytes after the last whole chunk, odd
    # and even chunk counts in every part, and 0 .. 9 and 16 data chunks in
    # a part around the helper's depth of 4
    seen = set()
    for blocks in range(4, 65, 4):
        what = (route, files, blocks)
        r = _random_runs(files, blocks, gpu)
        run_len, data_ch, half = chain_ref.job_chunks(blocks)
        seen |= {half, data_ch - half, data_ch}
        h0, h1, h2, h3 = (Table(files, gpu) for _ in range(4))
        st = Table(files, gpu)
        st_ref = Table(files, gpu, fill=r.state)
        _launch(route, gpu, small_batch, [r.job(0, None, h0)], what)
        _launch(route, gpu, small_batch, [r.job(1, st, h1)], what)
        assert np.array_equal(st.rows(what), r.state), ("part 1 state", what)
        _launch(route, gpu, small_batch, [r.job(2, st, h2)], what)
        _launch(route, gpu, small_batch, [r.job(2, st_ref, h3)], what)
        assert np.array_equal(h0.rows(what), r.hashes), ("part 0", what)
        h1.untouched(what)  # part 1 writes no hash
        assert np.array_equal(h2.rows(what), r.hashes), ("part 2 from the device's state", what)
        assert np.array_equal(st.rows(what), r.state), ("part 2 wrote the state", what)
        assert np.array_equal(h3.rows(what), r.hashes), ("part 2 from the reference's state", what)
        st_ref.untouched(what)
        r.unchanged(what)
    assert seen >= set(range(10)) | {16}


# --------------------------------------------------- b. crossed halves

@pytest.mark.parametrize("second", ROUTES)
@pytest.mark.parametrize("first", ROUTES)
def test_halves_on_either_route(gpu, small_batch, first, second):
    files = 65
    for blocks in (4, 24, 36, 60):
        what = (first, second, blocks)
        r = _random_runs(files, blocks, gpu, 1)
        st, h = Table(files, gpu), Table(files, gpu)
        _launch(first, gpu, small_batch, [r.job(1, st, None)], what)
        _launch(second, gpu, small_batch, [r.job(2, st, h)], what)
        assert np.array_equal(st.rows(what), r.state), ("state", what)
        assert np.array_equal(h.rows(what), r.hashes), ("hashes", what)
        r.unchanged(what)


# ----------------------------------------------------------- c. content

def _content(kind, files, blocks):
    run_len = 20 * blocks
    rng = _rng(files, blocks, 2)
    if kind == "zeros":
        return np.zeros((files, run_len), np.uint8)
    if kind == "ones":
        return np.full((files, run_len), 0xFF, np.uint8)
    if kind == "padding":
        # the last 64 bytes are what SHA-1 would append to the bytes before them
        runs = rng.integers(0, 256, (files, run_len), dtype=np.uint8)
        pad = bytes([0x80]) + bytes(55) + (8 * (run_len - 64)).to_bytes(8, "big")
        runs[:, -64:] = np.frombuffer(pad, np.uint8)
        return runs
    assert kind == "rotated"
    # file f is file 0 rotated by 16 f bytes: neighbours differ only by where each 16-B piece sits
    row = rng.integers(0, 256, run_len, dtype=np.uint8)
    return np.stack([np.roll(row, 16 * f) for f in range(files)])


@pytest.mark.parametrize("kind", ["zeros", "ones", "padding", "rotated"])
@pytest.mark.parametrize("route", ROUTES)
def test_content(gpu, small_batch, route, kind):
    files = 65
    for blocks in (16, 28):
        what = (route, kind, blocks)
        r = Runs(_content(kind, files, blocks), gpu)
        if kind == "zeros":
            assert all(bytes(x) == hashlib.sha1(bytes(20 * blocks)).digest() for x in r.hashes)
        if kind == "rotated":
            assert len({bytes(x) for x in r.hashes}) == min(files, 20 * blocks // 16)
        h0, h2, st = Table(files, gpu), Table(files, gpu), Table(files, gpu)
        _launch(route, gpu, small_batch, [r.job(0, None, h0)], what)
        _launch(route, gpu, small_batch, [r.job(1, st, None)], what)
        _launch(route, gpu, small_batch, [r.job(2, st, h2)], what)
        assert np.array_equal(h0.rows(what), r.hashes), ("part 0", what)
        assert np.array_equal(st.rows(what), r.state), ("part 1 state", what)
        assert np.array_equal(h2.rows(what), r.hashes), ("part 2", what)
        r.unchanged(what)


# ------------------------------------- d. two different jobs in a launch

class Spec:
    """One job of a launch with its own tables, and what they must hold after."""

    def __init__(self, files, blocks, part, dev, key):
        self.part = part
        self.r = _random_runs(files, blocks, dev, 3, key)
        self.st = Table(files, dev, fill=self.r.state if part == 2 else None)
        self.h = Table(files, dev)
        self.job = self.r.job(part, None if part == 0 else self.st, self.h)

    def check(self, what):
        if self.part == 1:
            assert np.array_equal(self.st.rows(what), self.r.state), ("state", what)
            self.h.untouched(what)
        else:
            assert np.array_equal(self.h.rows(what), self.r.hashes), ("hashes", what)
            self.st.untouched(what)
        self.r.unchanged(what)


PAIRS = {
    "part2_65x12_then_part1_3x40": ((65, 12, 2), (3, 40, 1)),
    "part1_3x40_then_part2_65x12": ((3, 40, 1), (65, 12, 2)),
    "whole_129x8_then_whole_1x64": ((129, 8, 0), (1, 64, 0)),
    "empty_then_whole_65x12": (None, (65, 12, 0)),
}


@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("route", ROUTES)
def test_two_different_jobs(gpu, small_batch, route, pair):
    specs = [Spec(*s, gpu, k) if s else None for k, s in enumerate(PAIRS[pair])]
    # jobs[0] with n_files = 0 is skipped: its other fields are never read
    jobs = [s.job if s else ChainJob(None, 0, 7, 3, None, None) for s in specs]
    _launch(route, gpu, small_batch, jobs, (route, pair))
    for k, s in enumerate(specs):
        if s:
            s.check((route, pair, k))


# ------------------------------ e. block waves around the chain waves

@pytest.fixture(scope="module")
def five_chain_waves(gpu):
    """129 + 65 files: 3 + 2 chain waves, so the first five workgroups of a
    launch run block waves 0 .. 14 beside them."""
    return [Spec(129, 8, 0, gpu, 10), Spec(65, 12, 0, gpu, 11)]


@pytest.mark.parametrize("files,nbf,cols", [
    (1, 64, None), (15, 64, None), (16, 64, None), (3, 100, None),
    (1, 128, (0, 64)), (1, 128, (64, 128)), (5, 192, (64, 192)),
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_block_waves_around_chain_waves(gpu, five_chain_waves, files, nbf, cols):
    # fewer block waves than the 15 slots of the mixed workgroups, exactly 15,
    # one more, a ragged last wave, and column ranges whose spare slots map
    # past the batch
    what = (files, nbf, cols)
    for s in five_chain_waves:
        s.h.t.copy_(torch.from_numpy(s.h.before))
    Batch(files, nbf, gpu, 4).launch([s.job for s in five_chain_waves], cols, what)
    for s in five_chain_waves:
        s.check(what)


# ------------------------------------------------- f. one lane per file

@pytest.mark.parametrize("files", [1, 63, 65])
def test_batch_entry_point_small_files(gpu, files):
    # blocks per file no multiple of 4: one lane per file (3, 6, 19 and 22
    # end in two padding chunks); 4, 16 and 60: helper waves, whole chains
    for nbf in (1, 2, 3, 5, 6, 7, 9, 13, 19, 22, 4, 16, 60):
        host = _rng(files, nbf, 5).integers(0, 256, files * nbf * BS, dtype=np.uint8)
        want = _block_digests(host)
        if nbf in (3, 6, 19, 22):
            assert (20 * nbf) % 64 >= 56
        t = torch.from_numpy(host.copy()).to(gpu)
        dig, first, fh = device.index_device_batch(t, [(i * nbf * BS, nbf * BS) for i in range(files)], BS)
        assert list(first) == [i * nbf for i in range(files + 1)], nbf
        assert np.array_equal(dig.cpu().numpy(), want), nbf
        assert np.array_equal(fh.cpu().numpy(), chain_ref.run_hashes(want.reshape(files, nbf * 20))), nbf
