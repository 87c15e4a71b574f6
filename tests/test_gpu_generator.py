"""GPU: the splitmix64 generator (fill_splitmix_kernel, device.fill_splitmix)
at its edges.  It writes the input of every large test and of the benchmark,
which hash what it wrote and so cannot see its errors.  Every fill is compared
byte for byte with oracle.splitmix_bytes(n, seed, start) -- three of them with
the pure-Python stream as well -- between 32 guard bytes of 0xA5 on each
side, which must come back unchanged."""
import numpy as np
import pytest
import torch

import oracle
from syncfast_amd import device

pytestmark = pytest.mark.gpu

GUARD, FILL = 32, 0xA5
SHIFTS = (0, 1, 8, 15)  # the output pointer, in bytes past a 16-byte boundary
STARTS = (0, 1, 7, 8, 15, 16, 17, (1 << 32) - 3, 1 << 32, (1 << 35) + 16, (1 << 40) + 5)
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 4095, 4097, 65536 * 16 + 9)  # the last: the tail on threads 0 .. 8
SEEDS = (0, (1 << 64) - 1)
WINDOW = 4096


def _guarded(n, shift, gpu):
    """(allocation, view): n bytes whose first lies `shift` bytes past a
    16-byte boundary, at least GUARD bytes of FILL before and after."""
    t = torch.full((GUARD + 16 + n + GUARD,), FILL, dtype=torch.uint8, device=gpu)
    lead = GUARD + (shift - (t.data_ptr() + GUARD)) % 16
    view = t[lead:lead + n]
    assert n == 0 or view.data_ptr() % 16 == shift
    return t, lead, view


def _guards_intact(t, lead, n):
    return bool((t[:lead] == FILL).all()) and bool((t[lead + n:] == FILL).all())


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("shift", SHIFTS)
def test_every_start_and_length_at_this_pointer(gpu, shift, seed):
    """start % 16 == 0 with shift 0 is the 16-byte fast path; an aligned start
    at an unaligned pointer and an unaligned start at an aligned pointer take
    the byte path; starts above 2^32 are what the sharded tests pass."""
    for start in STARTS:
        for n in LENGTHS:
            t, lead, view = _guarded(n, shift, gpu)
            assert device.fill_splitmix(view, seed, start) is view
            got = t.cpu().numpy()
            want = oracle.splitmix_bytes(n, seed, start)
            bad = np.flatnonzero(got[lead:lead + n] != want)
            assert bad.size == 0, (start, n, bad[:8])
            assert (got[:lead] == FILL).all() and (got[lead + n:] == FILL).all(), (start, n)


@pytest.mark.parametrize("shift,start,n,seed", [(0, 16, 65536 * 16 + 9, (1 << 64) - 1), (15, (1 << 40) + 5, 4097, 0),
                                                (0, (1 << 32) - 3, 4095, (1 << 64) - 1)])
def test_the_c_oracle_is_not_the_only_judge(gpu, shift, start, n, seed):
    t, lead, view = _guarded(n, shift, gpu)
    device.fill_splitmix(view, seed, start)
    assert bytes(view.cpu().numpy()) == oracle.py_splitmix_bytes(n, seed, start)
    assert _guards_intact(t, lead, n)


@pytest.mark.parametrize("shift,start,n,per_pass", [(0, 16, (1 << 28) + (1 << 20) + 5, 1 << 28),
                                                    (0, 3, (1 << 24) + 3 * (1 << 20) + 1, 1 << 24)])
def test_the_second_grid_stride_pass(gpu, shift, start, n, per_pass):
    """The launch is capped at 65,536 workgroups of 256 threads: one pass of
    the fast path covers 2^28 bytes, one of the byte path 2^24.  Windows of
    4 KiB at offset 0, around the end of the first pass and at the end are
    compared with the oracle at those starts; the host never generates the
    whole stream."""
    seed = 0x5EED
    t, lead, view = _guarded(n, shift, gpu)
    device.fill_splitmix(view, seed, start)
    for at in (0, per_pass - WINDOW // 2, n - WINDOW):
        got = view[at:at + WINDOW].cpu().numpy()
        assert np.array_equal(got, oracle.splitmix_bytes(WINDOW, seed, start + at)), at
    assert _guards_intact(t, lead, n)
