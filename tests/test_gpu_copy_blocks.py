"""GPU: the block copy kernel (sf_copy_blocks_device, device.copy_blocks).

What a copy must give always comes from a host model, never from the code
under test:

    want = bytearray(dst0); for each taken, in-range job: want[d:d+n] = src[s:s+n]

and every test compares the whole destination allocation, guard bytes
included, with it (the 2^32 - 1 byte job is judged by torch on the device)."""
import random

import numpy as np
import pytest
import torch

import syncfast_amd
from syncfast_amd import _lib, device

pytestmark = pytest.mark.gpu

FILL = 0xA5
TOP = (1 << 64) - 1


def _i64(values):
    """uint64 values as the int64 tensor elements the wrapper takes."""
    return np.array(values, dtype=np.uint64).view(np.int64)


def _i32(values):
    return np.array(values, dtype=np.uint32).view(np.int32)


def _random(rng, n) -> np.ndarray:
    return np.frombuffer(rng.randbytes(n), np.uint8).copy()


def _place(data: np.ndarray, gpu, lead=0, tail=0):
    """`data` in HBM, `lead` bytes into an allocation and `tail` bytes before
    its end (0: the allocation ends with it); the rest holds FILL.  Returns
    (allocation, view)."""
    t = torch.full((lead + data.size + tail,), FILL, dtype=torch.uint8, device=gpu)
    if data.size:
        t[lead:lead + data.size] = torch.from_numpy(data).to(gpu)
    return t, t[lead:lead + data.size]


def _model(src: np.ndarray, alloc0: np.ndarray, lead: int, dst_len: int, jobs, take=None) -> np.ndarray:
    want = alloc0.copy()
    for i, (s, d, n) in enumerate(jobs):
        if take is not None and not take[i]:
            continue
        if s > src.size or n > src.size - s or d > dst_len or n > dst_len - d:
            continue
        want[lead + d: lead + d + n] = src[s:s + n]
    return want


def _lists(jobs, gpu):
    so = torch.from_numpy(_i64([j[0] for j in jobs])).to(gpu)
    do = torch.from_numpy(_i64([j[1] for j in jobs])).to(gpu)
    sz = torch.from_numpy(_i32([j[2] for j in jobs])).to(gpu)
    return so, do, sz


def _copy_and_compare(gpu, src: np.ndarray, dst_len: int, jobs, take=None, lead_s=0, lead_d=0, guard=0,
                      check_range=True):
    """One copy_blocks call over fresh allocations, against the model."""
    _sa, s = _place(src, gpu, lead_s)
    da, d = _place(np.full(dst_len, FILL, np.uint8), gpu, lead_d + guard, guard)
    alloc0 = da.cpu().numpy()
    so, do, sz = _lists(jobs, gpu)
    tk = torch.from_numpy(np.asarray(take, np.uint8)).to(gpu) if take is not None else None
    device.copy_blocks(s, d, so, do, sz, take=tk, check_range=check_range)
    torch.cuda.synchronize(gpu)
    got = da.cpu().numpy()
    want = _model(src, alloc0, lead_d + guard, dst_len, jobs, take)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    return device.copy_stats()


def _tile():
    return device.copy_stats()[0]


@pytest.mark.parametrize("lead_s,lead_d", [(0, 0), (1, 3), (2, 15), (3, 1), (5, 2), (15, 5)])
def test_every_alignment_every_edge_one_call(gpu, lead_s, lead_d):
    """Every (source offset mod 16, destination offset mod 16) with every size
    of the edge list, laid out in shuffled order with gaps of 0 to 15 bytes of
    the fill pattern; each size also from the first and from the last bytes of
    the source, which ends with its allocation."""
    T = _tile()
    sizes = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025,
             T - 1, T, T + 1, 2 * T + 1]
    rng = random.Random(1000 + 16 * lead_s + lead_d)
    src = _random(rng, 4 * T + 77)
    shapes = [(sa, da, n) for sa in range(16) for da in range(16) for n in sizes]
    shapes += [(None, rng.randrange(16), n) for n in sizes for _ in (0, 1)]  # from the source's two ends
    rng.shuffle(shapes)
    jobs, at, ends = [], 0, 0
    for sa, da, n in shapes:
        at += (da - at) % 16  # a gap of 0 to 15 bytes
        if sa is None:
            s = (src.size - n) if ends & 1 else 0
            ends += 1
        else:
            s = 16 * rng.randrange((src.size - n - sa) // 16 + 1) + sa
        jobs.append((s, at, n))
        at += n
    assert {j[0] % 16 for j in jobs} == set(range(16)) == {j[1] % 16 for j in jobs}
    stats = _copy_and_compare(gpu, src, at + 9, jobs, lead_s=lead_s, lead_d=lead_d, guard=32)
    assert stats[1] == len(jobs) and stats[3] == 1
    assert stats[2] >= sum(-(-j[2] // T) for j in jobs)


def test_abutting_neighbours(gpu):
    """A destination tiled without gaps by 20,000 jobs of 0 to 300 bytes, runs
    of one-byte jobs beside empty ones among them, from shuffled source
    positions; guard bytes before and after."""
    rng = random.Random(5)
    sizes = [rng.randrange(301) for _ in range(20000)]
    for k in range(0, 20000, 500):  # 1, 0, 1, 1, 0, ... in a row
        sizes[k:k + 12] = [1, 0, 1, 1, 0, 0, 1, 2, 1, 0, 1, 1]
    order = list(range(len(sizes)))
    rng.shuffle(order)
    src_at, p = [0] * len(sizes), 0
    for i in order:
        src_at[i] = p
        p += sizes[i]
    src = _random(rng, p)
    jobs, at = [], 0
    for i, n in enumerate(sizes):
        jobs.append((src_at[i], at, n))
        at += n
    stats = _copy_and_compare(gpu, src, at, jobs, lead_s=1, lead_d=7, guard=64)
    assert stats[1] == len(jobs)


def test_fan_out_and_overlapping_sources(gpu):
    rng = random.Random(6)
    src = _random(rng, 20000)
    jobs, at = [], 3
    for _ in range(100):  # one range to 100 places
        jobs.append((13, at, 5001))
        at += 5001 + rng.randrange(3)
    for j in range(150):  # ranges that overlap each other
        jobs.append((7 * j, at, 1000 + j))
        at += 1000 + j
    _copy_and_compare(gpu, src, at + 5, jobs, lead_s=3, lead_d=1, guard=16)


def test_take_mask(gpu):
    rng = random.Random(7)
    src = _random(rng, 50000)
    jobs, at = [], 0
    for _ in range(3000):
        n = rng.choice([0, 1, 5, 16, 100, 700, 5000])
        jobs.append((rng.randrange(src.size - n + 1), at, n))
        at += n
    take = [rng.randrange(2) * rng.choice([1, 1, 255]) for _ in jobs]
    stats = _copy_and_compare(gpu, src, at, jobs, take=take, guard=16)
    assert stats[1] == sum(1 for t in take if t)
    stats = _copy_and_compare(gpu, src, at, jobs, take=[0] * len(jobs), guard=16)  # nothing changes
    assert stats[1:3] == (0, 0) and stats[3] == 1


def test_range(gpu):
    """Among 50 good jobs: a source past src_len, a destination past dst_len,
    a job that ends one byte past each, offset 2^64 - 1 with size 2 on either
    side.  Status SF_ERANGE, each bad job's destination untouched, the 50
    exact; d_status NULL is accepted; the wrapper raises with check_range."""
    rng = random.Random(8)
    src = _random(rng, 9000)
    dst_len = 50 * 200 + 6 * 64 + 3
    slot = lambda k: 50 * 200 + 64 * k  # noqa: E731  (a free place for each bad job)
    bad = [(src.size + 5, slot(0), 4), (10, dst_len + 5, 4), (src.size - 10, slot(1), 11), (10, dst_len - 10, 11),
           (TOP, slot(2), 2), (10, TOP, 2), (src.size, slot(3), 1), (src.size + 1, slot(4), 0)]
    jobs = [(rng.randrange(src.size - 200), 200 * i, rng.randrange(1, 201)) for i in range(50)]
    for k, b in enumerate(bad):
        jobs.insert(6 * k + 1, b)
    _sa, s = _place(src, gpu, 1)
    da, d = _place(np.full(dst_len, FILL, np.uint8), gpu, 5, 32)
    alloc0 = da.cpu().numpy()
    want = _model(src, alloc0, 5, dst_len, jobs)
    assert (want != alloc0).sum() > 2000 and (want[5 + 50 * 200:] == FILL).all()
    so, do, sz = _lists(jobs, gpu)
    L = syncfast_amd.lib()
    for with_status in (True, False):
        da[:] = torch.from_numpy(alloc0).to(gpu)
        status = torch.zeros(1, dtype=torch.int32, device=gpu)
        stream = torch.cuda.current_stream(gpu).cuda_stream
        rc = L.sf_copy_blocks_device(s.data_ptr(), s.numel(), d.data_ptr(), d.numel(), so.data_ptr(), do.data_ptr(),
                                     sz.data_ptr(), None, len(jobs), status.data_ptr() if with_status else None, stream)
        assert rc == 0
        torch.cuda.synchronize(gpu)
        assert int(status.item()) == (_lib.SF_ERANGE if with_status else 0)
        assert np.array_equal(da.cpu().numpy(), want)
        assert device.copy_stats()[1] == 50  # the in-range jobs alone
    da[:] = torch.from_numpy(alloc0).to(gpu)
    with pytest.raises(_lib.SfError) as e:
        device.copy_blocks(s, d, so, do, sz)
    assert e.value.code == _lib.SF_ERANGE
    assert np.array_equal(da.cpu().numpy(), want)  # the good ones were copied all the same
    device.copy_blocks(s, d, so, do, sz, check_range=False)  # asynchronous, no status
    # a list that is all in range raises nothing
    ok = [j for j in jobs if j not in bad]
    device.copy_blocks(s, d, *_lists(ok, gpu))
    torch.cuda.synchronize(gpu)


def test_balance_one_long_job_beside_100000_one_byte_jobs(gpu):
    n_long, n_small = (64 << 20) + 1, 100000
    src_t = device.splitmix_tensor(n_long + 3 + n_small, 77, gpu)
    src = src_t.cpu().numpy()
    jobs = [(3 + n_long + i, n_small - 1 - i, 1) for i in range(n_small)]  # reversed, one byte each
    jobs.insert(n_small // 2, (3, n_small + 1, n_long))
    dst_len = n_small + 1 + n_long
    da = torch.full((5 + dst_len + 16,), FILL, dtype=torch.uint8, device=gpu)
    d = da[5:5 + dst_len]
    alloc0 = da.cpu().numpy()
    so, do, sz = _lists(jobs, gpu)
    device.copy_blocks(src_t, d, so, do, sz)
    torch.cuda.synchronize(gpu)
    want = _model(src, alloc0, 5, dst_len, jobs)
    assert np.array_equal(da.cpu().numpy(), want)
    T, copied, tiles, launches = device.copy_stats()
    assert copied == n_small + 1 and launches == 1
    assert n_small + n_long // T <= tiles <= n_small + n_long // T + 2


def test_one_job_of_4_gib_less_one_byte(gpu):
    """2^32 - 1 bytes from source offset 2^32 + 3 to destination offset 5:
    sizes are any uint32, offsets any uint64.  torch is the judge."""
    n, s_off, d_off = (1 << 32) - 1, (1 << 32) + 3, 5
    src = torch.empty(s_off + n, dtype=torch.uint8, device=gpu)
    device.fill_splitmix(src[1 << 32:], 99)  # the bytes the job reads (and the three before them)
    dst = torch.full((d_off + n + 11,), FILL, dtype=torch.uint8, device=gpu)
    so, do, sz = _lists([(s_off, d_off, n)], gpu)
    device.copy_blocks(src, dst[:d_off + n + 4], so, do, sz)
    torch.cuda.synchronize(gpu)
    assert torch.equal(dst[d_off:d_off + n], src[s_off:s_off + n])
    assert bool((dst[:d_off] == FILL).all()) and bool((dst[d_off + n:] == FILL).all())
    T, copied, tiles, _ = device.copy_stats()
    assert copied == 1 and tiles == (1 << 32) // T + 1


def test_two_streams_into_disjoint_halves(gpu):
    rng = random.Random(10)
    src = _random(rng, 300000)
    half = 1 << 20
    halves = []
    for h in range(2):
        jobs, at = [], h * half
        while at < (h + 1) * half - 9000:
            n = rng.randrange(1, 9000)
            jobs.append((rng.randrange(src.size - n), at, n))
            at += n
        halves.append(jobs)
    _sa, s = _place(src, gpu, 2)
    da, d = _place(np.full(2 * half, FILL, np.uint8), gpu, 9, 16)
    alloc0 = da.cpu().numpy()
    lists = [_lists(j, gpu) for j in halves]
    torch.cuda.synchronize(gpu)
    streams = [torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)]
    for st, (so, do, sz) in zip(streams, lists):
        device.copy_blocks(s, d, so, do, sz, check_range=False, stream=st)
    for st in streams:
        st.synchronize()
    want = _model(src, alloc0, 9, 2 * half, halves[0] + halves[1])
    assert np.array_equal(da.cpu().numpy(), want)


def test_empty_list_and_empty_jobs(gpu):
    src = np.arange(100, dtype=np.uint8)
    _copy_and_compare(gpu, src, 50, [])
    stats = _copy_and_compare(gpu, src, 50, [(0, 0, 0), (100, 50, 0), (5, 7, 0)])
    assert stats[1:3] == (3, 0)
