"""The receiving side's block lookup (sf_block_set_*, device.BlockSet,
Index.get_blocks): for each incoming digest, the row Index::get_block
(src/index.rs:77-103) returns -- first present row with that hash, rowid
order -- or none.

The oracle (oracle.block_lookup) is pinned on CPU against the reference's
own SQL, run by the Index mirror on randomized indexes with repeated digests,
missing blocks and temporary files; the GPU tests compare the device lookup
with the oracle and with Index.get_block."""
from pathlib import PurePath

import numpy as np
import pytest
import torch

import oracle
from syncfast_amd.digest import HashDigest
from syncfast_amd.index import Index
from syncfast_amd.timestamp import DateTimeUtc


def _random_index(seed, n_files=6, per_file=40):
    """An in-memory index: files (one temporary) with blocks drawn from a small
    pool of digests (so digests repeat within and across files), some rows
    recorded as missing (present = 0)."""
    rng = np.random.default_rng(seed)
    pool = [HashDigest(rng.integers(0, 256, 20, dtype=np.uint8).tobytes()) for _ in range(60)]
    idx = Index.open_in_memory()
    for f in range(n_files):
        if f == n_files - 1:
            fid = idx.add_temp_file(PurePath(f"dir/t{f}"))
        else:
            fid, _ = idx.add_file(PurePath(f"dir/f{f}"), DateTimeUtc.from_ns(f))
        for b in range(per_file):
            h = pool[int(rng.integers(0, len(pool)))]
            if rng.random() < 0.3:
                idx.add_missing_block(h, fid, b * 4096, 4096)
            else:
                idx.add_block(h, fid, b * 4096, 4096)
    idx.commit()
    return idx, pool


def _rows(idx):
    rows = idx.db.execute("SELECT blocks.hash, blocks.present = 1 AND files.file_id IS NOT NULL, files.name, "
                          "blocks.offset, blocks.size FROM blocks LEFT JOIN files ON blocks.file_id = files.file_id "
                          "ORDER BY blocks.rowid;").fetchall()
    table = np.frombuffer(bytes.fromhex("".join(r[0] for r in rows)), np.uint8).reshape(-1, 20)
    present = np.array([bool(r[1]) for r in rows])
    return rows, table, present


@pytest.mark.parametrize("seed", range(8))
def test_oracle_is_get_block(seed):
    # the reference's SQL (Index.get_block) and the oracle agree on every
    # digest of the pool and on digests absent from the index
    idx, pool = _random_index(seed)
    rows, table, present = _rows(idx)
    extra = [HashDigest(bytes([seed] * 20))]
    q = pool + extra
    got = oracle.block_lookup(table, present, np.frombuffer(b"".join(h.bytes for h in q), np.uint8).reshape(-1, 20))
    for h, r in zip(q, got):
        want = idx.get_block(h)
        assert (None if r < 0 else (PurePath(rows[r][2]), int(rows[r][3]), int(rows[r][4]))) == want


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(4))
def test_index_get_blocks_on_device_is_get_block(gpu, seed):
    idx, pool = _random_index(100 + seed, n_files=12, per_file=300)
    q = pool + [HashDigest(bytes([7] * 20))] + pool[::-1]
    assert idx.get_blocks(q, device=gpu) == [idx.get_block(h) for h in q]


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,dup,with_present", [(0, 10, 0, False), (1, 5, 0, True), (1000, 3000, 50, True),
                                                   (100_000, 200_000, 5000, True), (100_000, 50_000, 0, False)])
def test_block_set_matches_oracle(gpu, n, m, dup, with_present):
    from syncfast_amd.device import BlockSet
    rng = np.random.default_rng(n + m)
    table = rng.integers(0, 256, (n, 20), dtype=np.uint8)
    if dup and n:  # repeated digests at random later rows
        src = rng.integers(0, n, dup)
        dst = rng.integers(0, n, dup)
        table[dst] = table[src]
    present = rng.random(n) < 0.7 if with_present else None
    # queries: rows of the table (hits, or misses when not present), fresh digests
    picks = table[rng.integers(0, max(n, 1), m // 2)] if n else np.zeros((0, 20), np.uint8)
    fresh = rng.integers(0, 256, (m - picks.shape[0], 20), dtype=np.uint8)
    queries = np.concatenate([picks, fresh])
    rng.shuffle(queries)
    t = torch.from_numpy(table).to(gpu)
    with BlockSet(t, torch.from_numpy(present).to(gpu) if present is not None else None) as bset:
        got = bset.lookup(torch.from_numpy(queries).to(gpu)).cpu().numpy()
    assert np.array_equal(got, oracle.block_lookup(table, present, queries))


@pytest.mark.gpu
def test_block_set_colliding_slots(gpu):
    # digests that share their slot bits (bytes 0-7) and fingerprint (8-10)
    # but differ later: the probe must compare whole digests
    from syncfast_amd.device import BlockSet
    base = np.zeros((64, 20), np.uint8)
    base[:, 19] = np.arange(64)  # same first 19 bytes, different last byte
    table = np.concatenate([base, base[::2]])  # repeats: the first row wins
    present = np.ones(table.shape[0], bool)
    present[:8] = False  # the first copies of rows 0..7 are missing: rows 0,2,4,6 resolve to the repeats
    q = np.concatenate([base, np.full((1, 20), 255, np.uint8)])
    t = torch.from_numpy(table).to(gpu)
    with BlockSet(t, torch.from_numpy(present).to(gpu)) as bset:
        got = bset.lookup(torch.from_numpy(q).to(gpu)).cpu().numpy()
    assert np.array_equal(got, oracle.block_lookup(table, present, q))
    assert got[0] == 64 and got[1] == -1 and got[8] == 8 and got[-1] == -1


def _lookup(gpu, table, present, q):
    from syncfast_amd.device import BlockSet
    t = torch.from_numpy(np.ascontiguousarray(table)).to(gpu)
    with BlockSet(t, torch.from_numpy(present).to(gpu) if present is not None else None) as bset:
        got = bset.lookup(torch.from_numpy(np.ascontiguousarray(q)).to(gpu)).cpu().numpy()
    assert np.array_equal(got, oracle.block_lookup(table, present, q))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("before_last", [False, True])
def test_block_set_probe_wraps_past_the_last_slot(gpu, before_last):
    """Digests whose bytes 0-7 are all 0xFF have the table's last slot as
    their home at any capacity, so their cluster goes on from slot 0; with 200
    more whose home is the slot before it (byte 0 = 0xFE) the cluster starts
    there.  A query absent from the table, same slot and fingerprint, walks
    the whole wrapped cluster to the first empty slot."""
    rng = np.random.default_rng(7)

    def family(n, byte0):
        d = np.full((n, 20), 0xFF, np.uint8)
        d[:, 0] = byte0
        d[:, 8:11] = 0x5A  # one fingerprint
        d[:, 11:] = rng.integers(0, 256, (n, 9), dtype=np.uint8)
        d[:, 11] = np.arange(n) & 0xFF
        d[:, 12] = np.arange(n) >> 8  # distinct
        return d

    last = family(300, 0xFF)
    table = np.concatenate([last[:40], last, family(200, 0xFE)] if before_last else [last[:40], last])
    present = np.ones(table.shape[0], bool)
    present[:20] = False         # first copies not present: the later copy answers
    present[40 + 100:40 + 110] = False  # single copies not present: no answer
    absent = family(50, 0xFF)
    absent[:, 13] ^= 0x80
    absent2 = family(50, 0xFE)
    absent2[:, 14] ^= 0x01
    q = np.concatenate([table, absent, absent2])
    assert len({bytes(r) for r in table}) == (500 if before_last else 300)
    assert not {bytes(r) for r in table} & {bytes(r) for r in np.concatenate([absent, absent2])}
    got = _lookup(gpu, table, present, q)
    assert got[0] == 40 and got[20] == 20 and got[40 + 105] == -1 and (got[table.shape[0]:] == -1).all()
    assert (got[40 + 110:table.shape[0]] == np.arange(40 + 110, table.shape[0])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", [511, 512, 513, 1024, 1025])
def test_block_set_capacity_edges(gpu, n_rows):
    """512 rows fill the smallest table (capacity 1024) to exactly 1/2; 513
    and 1025 rows are the first at the next capacity."""
    rng = np.random.default_rng(n_rows)
    table = rng.integers(0, 256, (n_rows, 20), dtype=np.uint8)
    q = np.concatenate([table, rng.integers(0, 256, (64, 20), dtype=np.uint8)])
    got = _lookup(gpu, table, None, q)
    assert np.array_equal(got[:n_rows], np.arange(n_rows)) and (got[n_rows:] == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("first_present", [90_000, None])
def test_block_set_one_digest_in_every_row(gpu, first_present):
    """100,000 rows insert one digest into one slot; the smallest present row
    wins whatever order the lanes arrive in."""
    table = np.tile(np.arange(20, dtype=np.uint8) * 11, (100_000, 1))
    present = np.zeros(100_000, bool)
    if first_present is not None:
        present[first_present:] = True
    q = np.concatenate([table[:3], table[:1] ^ 1])
    got = _lookup(gpu, table, present, q)
    assert got.tolist() == [first_present if first_present is not None else -1] * 3 + [-1]


@pytest.mark.gpu
def test_block_set_config2_table(gpu):
    # config 2's whole signature table (2^21 digests of the 8 GiB stream) as a
    # destination index, looked up with the same table shuffled plus as many
    # fresh digests: every answer vs the oracle
    from syncfast_amd import device
    from syncfast_amd.device import BlockSet
    data = device.splitmix_tensor(8 << 30, 0x5EED0000, device=gpu)
    dig = device.index_device(data, 4096)
    del data
    n = dig.shape[0]
    perm = torch.randperm(n, device=gpu)
    fresh = torch.randint(0, 256, (n, 20), dtype=torch.uint8, device=gpu)
    q = torch.cat([dig[perm], fresh])
    with BlockSet(dig) as bset:
        got = bset.lookup(q)
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    assert np.array_equal(g[:n], perm.cpu().numpy())  # the splitmix blocks are all distinct
    assert np.array_equal(g, oracle.block_lookup(dig.cpu().numpy(), None, q.cpu().numpy()))
