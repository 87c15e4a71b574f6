"""GPU: the shared bodies under index_device / index_device_weak and
index_device_blocks / index_device_blocks_weak (syncfast_amd/device.py), at
the smallest shapes where a slip in what they share would show: which
pointers are NULL for an empty input, the capacity passed for a caller's
output, the extra output of the weak forms.  Digests and weak sums against
the oracle.  SF_ERANGE from the plain explicit-list form is
test_gpu_parity.py::test_table_out_of_range_reports_erange."""
import numpy as np
import pytest
import torch

import oracle
from syncfast_amd import SfError, device
from syncfast_amd._lib import SF_ERANGE

pytestmark = pytest.mark.gpu

BS = 64
FILL = 0xAA


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def filled(shape, dtype, dev):
    return torch.full(shape, FILL if dtype == torch.uint8 else -1, dtype=dtype, device=dev)


@pytest.mark.parametrize("own_out", [False, True])
@pytest.mark.parametrize("weak", [False, True])
@pytest.mark.parametrize("length", [0, 1, BS, BS + 1])
def test_fixed_forms(gpu, length, weak, own_out):
    data = oracle.splitmix_bytes(length, 900 + length)
    n = device.num_blocks(length, BS)
    want = oracle.index_fixed(data, BS)[2].reshape(-1, 20)
    # a caller's outputs have one row more than needed: it must stay as it was
    out = filled((n + 1, 20), torch.uint8, gpu) if own_out else None
    wout = filled((n + 1,), torch.int32, gpu) if own_out else None
    t = to_dev(data, gpu)
    if weak:
        d, w = device.index_device_weak(t, BS, out=out, weak_out=wout)
        assert w.dtype == torch.int32 and (w is wout if own_out else w.shape == (n,))
        assert np.array_equal(w.cpu().numpy()[:n].view(np.uint32), oracle.adler_fixed(data, BS))
        assert not own_out or int(w[n]) == -1
    else:
        d = device.index_device(t, BS, out=out)
    assert d.dtype == torch.uint8 and (d is out if own_out else d.shape == (n, 20))
    assert np.array_equal(d.cpu().numpy()[:n], want)
    assert not own_out or bool((d[n] == FILL).all())


def _lists():
    """(data, offsets, sizes): 65 blocks (the first length at which the
    library sorts a list) with empty and overlapping ones, and no block."""
    rng = np.random.default_rng(65)
    data = oracle.splitmix_bytes(4096, 965)
    sizes = rng.integers(0, 200, 65).astype(np.int64)
    sizes[[3, 64]] = 0
    offs = np.array([int(rng.integers(0, data.size - s + 1)) for s in sizes], np.int64)
    return [(data, offs, sizes), (data, offs[:0], sizes[:0])]


# the weak form takes no output of the caller's
@pytest.mark.parametrize("weak, own_out", [(False, False), (False, True), (True, False)])
@pytest.mark.parametrize("case", [0, 1], ids=["65_blocks", "no_block"])
def test_list_forms(gpu, case, weak, own_out):
    data, offs, sizes = _lists()[case]
    n = offs.size
    t, o, z = to_dev(data, gpu), to_dev(offs, gpu), to_dev(sizes.astype(np.int32), gpu)
    if weak:
        d, w = device.index_device_blocks_weak(t, o, z)
        assert w.dtype == torch.int32 and w.shape == (n,)
        assert np.array_equal(w.cpu().numpy().view(np.uint32), oracle.adler_blocks(data, offs, sizes))
    else:
        out = filled((n + 1, 20), torch.uint8, gpu) if own_out else None
        d = device.index_device_blocks(t, o, z, out=out)
        assert not own_out or (d is out and bool((d[n] == FILL).all()))
    assert d.dtype == torch.uint8 and (own_out or d.shape == (n, 20))
    assert np.array_equal(d.cpu().numpy()[:n], oracle.index_blocks(data, offs, sizes).reshape(-1, 20))


def test_an_output_one_digest_short_is_refused_before_any_launch(gpu):
    data, offs, sizes = _lists()[0]
    t, o, z = to_dev(data, gpu), to_dev(offs, gpu), to_dev(sizes.astype(np.int32), gpu)
    n = device.num_blocks(data.size, BS)
    short, short_list = filled((n - 1, 20), torch.uint8, gpu), filled((offs.size - 1, 20), torch.uint8, gpu)
    weak_ok, weak_short = filled((n,), torch.int32, gpu), filled((n - 1,), torch.int32, gpu)
    full = filled((n, 20), torch.uint8, gpu)
    for call in (lambda: device.index_device(t, BS, out=short),
                 lambda: device.index_device_weak(t, BS, out=short, weak_out=weak_ok),
                 lambda: device.index_device_weak(t, BS, out=full, weak_out=weak_short),
                 lambda: device.index_device_blocks(t, o, z, out=short_list)):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    for untouched in (short, short_list, full):
        assert bool((untouched == FILL).all())
    for untouched in (weak_ok, weak_short):
        assert bool((untouched == -1).all())


def test_weak_list_form_reports_erange(gpu):
    t = to_dev(oracle.splitmix_bytes(1000, 966), gpu)
    o = torch.tensor([0, 990], dtype=torch.int64, device=gpu)
    z = torch.tensor([10, 11], dtype=torch.int32, device=gpu)
    with pytest.raises(SfError) as e:
        device.index_device_blocks_weak(t, o, z)
    assert e.value.code == SF_ERANGE
