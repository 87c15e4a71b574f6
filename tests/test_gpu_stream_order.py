"""GPU: every device entry point keeps its caller's stream order.

One scenario per entry point (tests/stream_order.py is the harness): the
inputs sit behind a delay on the caller's own, non-default stream and hold a
decoy until it ends; caller-supplied outputs are filled with 0xEE behind the
same delay; after the call the outputs are cloned on that stream, the inputs
overwritten with the decoy again, the stream synchronised, and the clones
compared with a host reference of the *real* inputs (oracle, hashlib,
wire.Parser / wire.write_message, the host cutter, the copy model) -- always
exactly.  A launch on another stream, a missing event wait towards an internal
stream, a status word zeroed on another stream or scratch freed under an
internal stream's reads gives the decoy's answer, 0xEE, or garbage.

The delay is ten times the longest call of any scenario, timed on the idle
device by the `scenarios` fixture (at least 5 ms), and test_the_hold_has_teeth
shows that a call the *test* puts on a second stream does see the decoy.  The
caller's stream is one the default stream verifiably runs beside, and for the
entry points that work on the library's two internal streams one those run
beside too (so.fresh_stream): on a shared hardware queue a misplaced launch
would wait for the hold all the same.

Measured on one MI355X: longest call 6.9 ms (index_device_zpaq on 1 MiB),
H = 69 ms, 2.38e6 _sleep cycles per ms; the shortest hold lasted 1.85 times
what was asked.  Not committed, each run once: with device._stream_ptr
returning the default stream all 27 tests that go through it fail (FileImages
does not: its blocking list upload waits for the caller's stream first); with
one of the two hipStreamWaitEvent(st[i], ready) of sf_wire_file_blocks_fd
dropped both fixed-form fd scenarios fail; with FileImages._after_fill a no-op
test_the_images_wait_for_their_zero_fill fails.
"""
import contextlib
import hashlib
import random
import tempfile
from pathlib import PurePath

import numpy as np
import pytest
import torch

import data_expect
import oracle
import recv_expect
import recv_forge as rf
import stream_order as so
import zpaq_join as zj
from syncfast_amd import _lib, device, host, wire
from syncfast_amd.assemble import FileImages
from syncfast_amd.index import temp_name
from test_gpu_copy_blocks import _model as copy_model

pytestmark = pytest.mark.gpu

U8, I32 = torch.uint8, torch.int32


def _bytes(seed, n) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _u8(b: bytes) -> np.ndarray:
    return np.frombuffer(b, np.uint8).copy()


def _sptr(stream, gpu) -> int:
    return (stream if stream is not None else torch.cuda.current_stream(gpu)).cuda_stream


@contextlib.contextmanager
def _knobs(values: dict):
    old = {k: _lib.set_knob(k, v) for k, v in values.items()}
    try:
        yield
    finally:
        for k, v in old.items():
            _lib.set_knob(k, v)


class Sc:
    """One scenario: `real` and `decoy` {name: numpy array} of equal shapes,
    `call(x, o, stream)` -> a tuple of device tensors and plain values from
    the device inputs x and the caller-supplied outputs o, `want(inputs)` ->
    the same tuple from the host arrays alone."""

    def __init__(self, real, decoy, call, want, out=None, shift=None, knobs=None, internal=False):
        assert real.keys() == decoy.keys()
        self.internal = internal  # the entry point works on the library's two internal streams
        self.real, self.decoy, self.call, self.want = real, decoy, call, want
        self.out, self.shift, self.knobs = out or {}, shift or {}, knobs or {}
        self.want_real = None  # computed once, by the fixture


BUILDERS = {}


def scenario(*names):
    def add(fn):
        for name in names or (fn.__name__,):
            BUILDERS[name] = fn
        return fn
    return add


# ---------------------------------------------------------------- fixed tiling

BS, N_FIXED = 4096, 70 * 4096 + 333


@scenario("index_device-shift0", "index_device-shift3", "index_device_weak-shift0", "index_device_weak-shift3")
def _fixed(name):
    weak, shift = "weak" in name, int(name[-1])
    nb = device.num_blocks(N_FIXED, BS)
    out = {"out": ((nb, 20), U8)}
    if weak:
        out["weak_out"] = ((nb,), I32)

    def call(x, o, s):
        if weak:
            return device.index_device_weak(x["data"], BS, out=o.get("out"), weak_out=o.get("weak_out"), stream=s)
        return (device.index_device(x["data"], BS, out=o.get("out"), stream=s),)

    def want(a):
        d = oracle.index_fixed(a["data"], BS)[2]
        return (d, oracle.adler_fixed(a["data"], BS)) if weak else (d,)
    return Sc({"data": _bytes(1, N_FIXED)}, {"data": _bytes(2, N_FIXED)}, call, want, out=out, shift={"data": shift})


# -------------------------------------------------------------- explicit lists

def _ragged(seed, n, length):
    """n blocks of 0 to 4000 bytes anywhere in `length` bytes, in no order."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 4001, n).astype(np.int32)
    sizes[::17] = rng.integers(0, 70, sizes[::17].size)
    offsets = (rng.integers(0, length - 4000, n)).astype(np.int64)
    return offsets, sizes


N_LIST, LEN_LIST = 300, 500_000 + 7


def _list_inputs(seed):
    offsets, sizes = _ragged(seed + 10, N_LIST, LEN_LIST)
    return {"data": _bytes(seed, LEN_LIST), "offsets": offsets, "sizes": sizes}


@scenario("index_device_blocks-sort1", "index_device_blocks-sort0", "index_device_blocks_weak-sort1",
          "index_device_blocks_weak-sort0")
def _blocks(name):
    weak = "weak" in name

    def call(x, o, s):
        if weak:
            return device.index_device_blocks_weak(x["data"], x["offsets"], x["sizes"], stream=s)
        return (device.index_device_blocks(x["data"], x["offsets"], x["sizes"], stream=s),)

    def want(a):
        d = oracle.index_blocks(a["data"], a["offsets"], a["sizes"])
        return (d, oracle.adler_blocks(a["data"], a["offsets"], a["sizes"])) if weak else (d,)
    return Sc(_list_inputs(3), _list_inputs(4), call, want, knobs={"SF_TEST_TABLE_SORT": int(name[-1])})


BAD_ROW = 123


@scenario("index_device_blocks-status-sort1", "index_device_blocks-status-sort0")
def _blocks_status(name):
    """check_range=False is the C call with a status word of the caller's:
    zeroed, written and read on the stream, one row of the real list out of
    range (none of the decoy's)."""
    real, decoy = _list_inputs(5), _list_inputs(6)
    real["offsets"][BAD_ROW], real["sizes"][BAD_ROW] = LEN_LIST - 10, 11

    def call(x, o, s):
        gpu = x["data"].device
        with device._on(gpu, s):
            out = torch.empty((N_LIST, 20), dtype=U8, device=gpu)
            status = torch.zeros(1, dtype=I32, device=gpu)
            rc = _lib.lib().sf_index_device_blocks(x["data"].data_ptr(), LEN_LIST, x["offsets"].data_ptr(),
                                                   x["sizes"].data_ptr(), N_LIST, out.data_ptr(), status.data_ptr(),
                                                   _sptr(s, gpu))
        assert rc == 0
        return out, status

    def want(a):
        offsets, sizes = a["offsets"].copy(), a["sizes"].copy()
        bad = offsets + sizes > LEN_LIST
        offsets[bad], sizes[bad] = 0, 0
        digests = oracle.index_blocks(a["data"], offsets, sizes)
        digests[bad] = 0  # a block outside the buffer is not read: its digest is zeroed
        return digests, np.array([_lib.SF_ERANGE if bad.any() else 0], np.int32)
    return Sc(real, decoy, call, want, knobs={"SF_TEST_TABLE_SORT": int(name[-1])})


# ------------------------------------------------------------ many-file batches

NF, NBF, BS_BATCH = 65, 128, 1024
FLEN = NBF * BS_BATCH
RAGGED_LENS = [1, 1024, 1025, 40_000, 5, 65_536, 3_000, 12_345, 1023, 70_001, 2048, 64, 9_999, 33_333, 7, 20_480]


def _batch_want(data, files, bs):
    digs = [oracle.index_fixed(data[o:o + n], bs)[2] for o, n in files]
    first = np.concatenate([[0], np.cumsum([d.shape[0] for d in digs])]).astype(np.int64)
    hashes = np.stack([np.frombuffer(oracle.blocks_hash(d), np.uint8) for d in digs])
    return np.concatenate(digs), first, hashes


@scenario("index_device_batch-equal-fused1", "index_device_batch-equal-fused0", "index_device_batch-ragged-fused1",
          "index_device_batch-ragged-fused0")
def _batch(name):
    if "equal" in name:
        files = [(i * FLEN, FLEN) for i in range(NF)]
        total, out = NF * FLEN, {"out": ((NF * NBF, 20), U8), "hashes_out": ((NF, 20), U8)}
    else:
        files, at = [], 3
        for n in RAGGED_LENS:
            files.append((at, n))
            at += n + 5
        total, out = at, {}

    def call(x, o, s):
        return device.index_device_batch(x["data"], files, BS_BATCH, out=o.get("out"), hashes_out=o.get("hashes_out"),
                                         stream=s)
    return Sc({"data": _bytes(7, total)}, {"data": _bytes(8, total)}, call,
              lambda a: _batch_want(a["data"], files, BS_BATCH), out=out, knobs={"SF_BATCH_FUSED": int(name[-1])})


@scenario("BatchStream-finish", "BatchStream-push_last")
def _batch_stream(name):
    files = [(i * FLEN, FLEN) for i in range(NF)]

    def call(x, o, s):
        st = device.BatchStream(NF, FLEN, BS_BATCH, stream=s)
        tables = [o[f"d{k}"] if o else torch.empty((NF * NBF, 20), dtype=U8, device=x["b0"].device) for k in range(3)]
        hashes = []
        for k in range(3):
            if k == 2 and name.endswith("push_last"):
                assert st._half_cols() is not None  # the column halves
                hashes += st.push_last(x[f"b{k}"], tables[k])
            else:
                h = st.push(x[f"b{k}"], tables[k])
                hashes += [h] if h is not None else []
        hashes += st.finish()
        assert len(hashes) == 3
        return tuple(tables) + tuple(hashes)

    def want(a):
        per = [_batch_want(a[f"b{k}"], files, BS_BATCH) for k in range(3)]
        return tuple(p[0] for p in per) + tuple(p[2] for p in per)
    return Sc({f"b{k}": _bytes(20 + k, NF * FLEN) for k in range(3)}, {f"b{k}": _bytes(30 + k, NF * FLEN) for k in range(3)},
              call, want, out={f"d{k}": ((NF * NBF, 20), U8) for k in range(3)})


# ------------------------------------------------------------------ the ZPAQ cut

def _zpaq_want(data, bits, max_size, digests):
    offs, sizes = host.zpaq_cut_buffer(data, bits, max_size)
    offs, sizes = offs.astype(np.int64), sizes.astype(np.int32)
    if not digests:
        return offs, sizes
    raw = data.tobytes()
    digs = [hashlib.sha1(raw[o:o + n]).digest() for o, n in zip(offs.tolist(), sizes.tolist())]
    return offs, sizes, _u8(b"".join(digs)).reshape(-1, 20), hashlib.sha1(b"".join(digs)).digest()


@scenario("cut_device_zpaq-islands", "cut_device_zpaq-1mib", "index_device_zpaq-islands", "index_device_zpaq-1mib")
def _zpaq(name):
    digests = name.startswith("index")
    if name.endswith("islands"):
        bits, max_size = 6, 256
        raw = zj.islands(zj.segment_len(max_size), 1)
        assert zj.restate(raw, bits, max_size).rounds >= 2  # a host read per join round
        real = _u8(raw)
    else:
        bits, max_size = 13, 32768
        real = _bytes(9, 1 << 20)

    def call(x, o, s):
        if digests:
            return device.index_device_zpaq(x["data"], bits, max_size, stream=s)
        return device.cut_device_zpaq(x["data"], bits, max_size, stream=s)
    return Sc({"data": real}, {"data": np.zeros_like(real)}, call, lambda a: _zpaq_want(a["data"], bits, max_size, digests))


# ------------------------------------------------------------- the wire builders

N_WIRE = 2500
FILE_LEN_WIRE = (N_WIRE - 1) * BS + 77


def _wire_sizes(seed):
    """One size per row, 1 to 10 digits in turn: uint32 as the int32 the
    wrapper takes."""
    rng = np.random.default_rng(seed)
    sizes = [int(rng.integers(10 ** (i % 10), min(10 ** (i % 10 + 1), 1 << 32))) for i in range(N_WIRE)]
    return np.array(sizes, np.uint32).view(np.int32)


def _wire_want(a, fixed):
    if fixed:
        sizes = [BS] * (N_WIRE - 1) + [77]
    else:
        sizes = a["sizes"].view(np.uint32).tolist()
    return b"".join(wire.write_message("FileBlock", a["digests"][i].tobytes(), sizes[i]) for i in range(N_WIRE))


def _wire_inputs(seed, fixed):
    a = {"digests": _bytes(seed, N_WIRE * 20).reshape(N_WIRE, 20)}
    if not fixed:
        a["sizes"] = _wire_sizes(seed + 1)  # the decoy's sizes have the real ones' digits: a run of the same length
    return a


@scenario("wire.file_blocks_device", "wire.blocks_device")
def _wire_device(name):
    fixed = "file_blocks" in name

    def call(x, o, s):
        if fixed:
            return (wire.file_blocks_device(x["digests"], BS, FILE_LEN_WIRE, stream=s),)
        return (wire.blocks_device(x["digests"], x["sizes"], stream=s),)
    return Sc(_wire_inputs(40, fixed), _wire_inputs(50, fixed), call, lambda a: (_u8(_wire_want(a, fixed)),))


@scenario("wire.file_blocks_to_fd-chunk7", "wire.file_blocks_to_fd-chunk1000", "wire.blocks_to_fd-chunk7",
          "wire.blocks_to_fd-chunk1000")
def _wire_fd(name):
    fixed = "file_blocks" in name
    chunk = int(name.split("chunk")[1])
    assert N_WIRE // chunk >= 2  # several chunks, so both internal streams build some

    def call(x, o, s):
        with tempfile.TemporaryFile() as f:
            if fixed:
                n = wire.file_blocks_to_fd(x["digests"], BS, FILE_LEN_WIRE, f.fileno(), stream=s)
            else:
                n = wire.blocks_to_fd(x["digests"], x["sizes"], f.fileno(), stream=s)
            f.seek(0)
            return n, f.read()

    def want(a):
        run = _wire_want(a, fixed)
        return len(run), run
    return Sc(_wire_inputs(60, fixed), _wire_inputs(70, fixed), call, want, knobs={"SF_TEST_WIRE_CHUNK": chunk},
              internal=True)


# -------------------------------------------------------------- FILE_BLOCK runs

def _file_block_run(seed, digits) -> bytes:
    """Honest messages whose sizes have the given numbers of digits."""
    rng = np.random.default_rng(seed)
    out = []
    for d in digits:
        size = int(rng.integers(10 ** (d - 1) if d > 1 else 0, min(10 ** d, 1 << 32)))
        out.append(recv_expect.message(rng.integers(0, 256, 20, dtype=np.uint8).tobytes(), size))
    return b"".join(out)


def _parse_want(run: bytes):
    digests, sizes, consumed, stop = recv_expect.expected(run)
    return _u8(b"".join(digests)).reshape(-1, 20), np.array(sizes, np.uint32), consumed, stop


DIGITS = [i % 10 + 1 for i in range(300)]


@scenario("wire.parse_blocks_device-clean", "wire.parse_blocks_device-forged")
def _parse(name):
    forged = name.endswith("forged")
    tail = b"FILE_END\n"
    if forged:
        pair, _p, _family = rf.forge(2, 1)  # A has a 1-digit size, B (size 99) 2 digits
        real = _file_block_run(80, DIGITS) + pair + _file_block_run(81, DIGITS[:50]) + tail
        decoy = _file_block_run(82, DIGITS + [1, 2] + DIGITS[:50]) + tail
        assert rf.forged_start_in_chain(real)  # the device hands this run to the host parser
    else:
        real, decoy = _file_block_run(83, DIGITS) + tail, _file_block_run(84, DIGITS) + tail
        assert not rf.forged_start_in_chain(real)
    assert len(real) == len(decoy) and not rf.forged_start_in_chain(decoy)

    def call(x, o, s):
        return wire.parse_blocks_device(x["run"], stream=s) + (wire.parse_stats()[2],)
    return Sc({"run": _u8(real)}, {"run": _u8(decoy)}, call,
              lambda a: _parse_want(a["run"].tobytes()) + (int(rf.forged_start_in_chain(a["run"].tobytes())),))


# -------------------------------------------------------------- BLOCK_DATA runs

def _block_data_want(run: bytes, verify: bool):
    digests, sizes, offsets, consumed, stop, need = data_expect.expected(run)
    ok = np.array([hashlib.sha1(run[o:o + n]).digest() == d for d, n, o in zip(digests, sizes, offsets)], np.uint8)
    return (_u8(b"".join(digests)).reshape(-1, 20), np.array(sizes, np.uint32), np.array(offsets, np.int64),
            ok if verify else None, consumed, stop, need)


N_DATA, CORRUPT = 14, 10


@scenario("wire.receive_block_data_device-chain", "wire.receive_block_data_device-walk",
          "wire.receive_block_data_device-chain-unverified")
def _block_data(name):
    walk, verify = int("walk" in name), "unverified" not in name
    real = data_expect.honest_run(random.Random(7), N_DATA)
    decoy = data_expect.honest_run(random.Random(8), N_DATA)
    at = data_expect.expected(real)[2][CORRUPT] + 100  # inside the 4096-byte payload
    real = real[:at] + bytes([real[at] ^ 0x10]) + real[at + 1:]
    assert len(real) == len(decoy) and not data_expect.needs_walk(real)
    want_real = _block_data_want(real, True)
    assert want_real[3].tolist() == [int(i != CORRUPT) for i in range(N_DATA)]

    def call(x, o, s):
        return wire.receive_block_data_device(x["run"], verify=verify, stream=s) + (wire.block_data_stats()[2],)
    return Sc({"run": _u8(real)}, {"run": _u8(decoy)}, call,
              lambda a: _block_data_want(a["run"].tobytes(), verify) + (walk,), knobs={"SF_TEST_BLOCK_DATA_WALK": walk})


# ------------------------------------------------------------------ the block set

N_ROWS, N_QUERIES = 1000, 3000


def _set_inputs(seed):
    """A table with repeated digests and absent rows; queries that repeat,
    a third of them digests the table does not hold."""
    rng = np.random.default_rng(seed)
    table = rng.integers(0, 256, (N_ROWS, 20), dtype=np.uint8)
    table[rng.integers(0, N_ROWS, 200)] = table[rng.integers(0, N_ROWS, 200)]
    present = (rng.random(N_ROWS) < 0.7).astype(np.uint8)
    queries = table[rng.integers(0, N_ROWS, N_QUERIES)].copy()
    miss = rng.random(N_QUERIES) < 0.33
    queries[miss] = rng.integers(0, 256, (int(miss.sum()), 20), dtype=np.uint8)
    return {"table": table, "present": present, "queries": queries}


@scenario("BlockSet-build-lookup-close")
def _set_lookup(name):
    def call(x, o, s):
        bs = device.BlockSet(x["table"], x["present"], stream=s)
        rows = bs.lookup(x["queries"])
        bs.close()  # stream-ordered: after the lookup
        return (rows,)
    return Sc(_set_inputs(90), _set_inputs(91), call,
              lambda a: (oracle.block_lookup(a["table"], a["present"], a["queries"]),))


@scenario("BlockSet-receive")
def _set_receive(name):
    def inputs(seed):
        a = _set_inputs(seed)
        rng = np.random.default_rng(seed + 5)
        q = a.pop("queries")[:len(DIGITS)]
        run = b"".join(recv_expect.message(q[i].tobytes(), int(rng.integers(10 ** (d - 1) if d > 1 else 0,
                                                                             min(10 ** d, 1 << 32))))
                       for i, d in enumerate(DIGITS)) + b"FILE_END\n"
        a["run"] = _u8(run)
        return a

    def call(x, o, s):
        with device.BlockSet(x["table"], x["present"], stream=s) as bs:
            return bs.receive(x["run"], base_offset=1 << 33)

    def want(a):
        digests, sizes, consumed, stop = _parse_want(a["run"].tobytes())
        ends = (1 << 33) + np.cumsum(sizes.astype(np.int64))
        offsets = np.concatenate([[1 << 33], ends[:-1]]).astype(np.int64)
        return digests, sizes, offsets, oracle.block_lookup(a["table"], a["present"], digests), consumed, stop, int(ends[-1])
    real, decoy = inputs(92), inputs(93)
    assert real["run"].size == decoy["run"].size
    return Sc(real, decoy, call, want)


# ----------------------------------------------------------------- the block copy

N_JOBS, LEN_SRC = 3000, 50_000


def _copy_inputs(seed):
    """test_take_mask's list: sizes of 0 to 5000 bytes laid out back to back,
    from anywhere in the source, about half of them taken."""
    rng = random.Random(seed)
    jobs, at = [], 0
    for _ in range(N_JOBS):
        n = rng.choice([0, 1, 5, 16, 100, 700, 5000])
        jobs.append((rng.randrange(LEN_SRC - n + 1), at, n))
        at += n
    take = [rng.randrange(2) * rng.choice([1, 1, 255]) for _ in jobs]
    return {"src": _u8(rng.randbytes(LEN_SRC)), "so": np.array([j[0] for j in jobs], np.int64),
            "do": np.array([j[1] for j in jobs], np.int64), "sz": np.array([j[2] for j in jobs], np.int32),
            "take": np.array(take, np.uint8)}


LEN_DST = N_JOBS * 5000  # room for any such list


def _copy_want(a):
    jobs = list(zip(a["so"].tolist(), a["do"].tolist(), a["sz"].tolist()))
    return (copy_model(a["src"], np.full(LEN_DST, so.PREFILL, np.uint8), 0, LEN_DST, jobs, a["take"].tolist()),)


@scenario("copy_blocks")
def _copy(name):
    def call(x, o, s):
        dst = o["dst"] if o else torch.full((LEN_DST,), so.PREFILL, dtype=U8, device=x["src"].device)
        device.copy_blocks(x["src"], dst, x["so"], x["do"], x["sz"], take=x["take"], check_range=False, stream=s)
        return (dst,)
    return Sc(_copy_inputs(7), _copy_inputs(8), call, _copy_want, out={"dst": ((LEN_DST,), U8)})


# ------------------------------------------------------------- bytes to a file

N_WRITE = (3 << 20) + 5


@scenario("write_to_fd")
def _write_fd(name):
    def call(x, o, s):
        with tempfile.TemporaryFile() as f:
            n = device.write_to_fd(x["bytes"], f.fileno(), 0, stream=s)
            f.seek(0)
            return n, f.read()
    return Sc({"bytes": _bytes(100, N_WRITE)}, {"bytes": _bytes(101, N_WRITE)}, call,
              lambda a: (N_WRITE, a["bytes"].tobytes()), knobs={"SF_TEST_STREAM_STAGE_MIB": 1}, internal=True)


# ------------------------------------------------------------------ the generator

N_FILL = (1 << 20) + 5


@scenario("fill_splitmix")
def _fill(name):
    """No input: a write after the 0xEE write of the caller's."""
    def call(x, o, s):
        out = o["out"] if o else torch.empty(N_FILL, dtype=U8, device=torch.device("cuda", 0))
        return (device.fill_splitmix(out, 0x5EED, 16, stream=s),)
    return Sc({}, {}, call, lambda a: (oracle.splitmix_bytes(N_FILL, 0x5EED, 16),), out={"out": ((N_FILL,), U8)})


# --------------------------------------------------------------- the file images

def _images_plan(seed):
    """test_images_in_place_of_the_write_loop's sync, smaller, with its lists
    written down directly: two incoming files made of blocks that arrive as
    BLOCK_DATA and blocks a file of the destination holds."""
    rng = random.Random(seed)
    blocks = [rng.randbytes(n) for n in (5000, 1, 9000, 0, 777, 4096)]
    local = [rng.randbytes(n) for n in (3000, 9001)]
    pad = rng.randbytes(101)
    old = pad + local[0] + local[1]
    local_at = {"L0": (len(pad), 3000), "L1": (len(pad) + 3000, 9001)}
    files = {"a.bin": [0, "L0", 1, 2, 0, "L1", 3], "sub/b.bin": [4, 2, "L1", 5]}
    run = b"".join(data_expect.message(b) for b in blocks)
    payload_at = data_expect.expected(run)[2]
    copies, writes, source = {}, [], {}
    for name, order in files.items():
        at, out, copies[name] = 0, b"", []
        for k in order:
            if isinstance(k, str):
                copies[name].append((PurePath("old.bin"), local_at[k][0], at, local_at[k][1]))
                piece = old[local_at[k][0]:local_at[k][0] + local_at[k][1]]
            else:
                writes.append((temp_name(name), at, payload_at[k], len(blocks[k])))
                piece = blocks[k]
            out += piece
            at += len(piece)
        source[name] = out
    return {"old": _u8(old), "run": _u8(run)}, copies, writes, source


@scenario("FileImages")
def _images(name):
    real, copies, writes, source = _images_plan(61)
    decoy = {k: _bytes(62 + i, v.size) for i, (k, v) in enumerate(real.items())}
    names = list(source)

    def call(x, o, s):
        images = FileImages({temp_name(n): len(source[n]) for n in names}, device=x["old"].device)
        for n in names:  # right after construction
            assert images.apply_copies(temp_name(n), copies[n], source=lambda _name: x["old"], stream=s) == 1
        assert images.apply_writes(writes, x["run"], stream=s) == 1
        written = []
        for n in names:
            with tempfile.TemporaryFile() as f:
                assert images.write(temp_name(n), f.fileno(), stream=s) == len(source[n])
                f.seek(0)
                written.append(f.read())
        return tuple(images.image(temp_name(n)) for n in names) + tuple(written)

    def want(a):
        old, run = a["old"].tobytes(), a["run"].tobytes()
        out = []
        for n in names:
            img = bytearray(len(source[n]))
            for _from, src_at, at, size in copies[n]:
                img[at:at + size] = old[src_at:src_at + size]
            for to, at, start, size in writes:
                if to == temp_name(n):
                    img[at:at + size] = run[start:start + size]
            out.append(bytes(img))
        assert a is not real or out == [source[n] for n in names]  # the plan itself
        return tuple(_u8(b) for b in out) + tuple(out)
    return Sc(real, decoy, call, want, internal=True)


# ------------------------------------------------------------------- the runs

ALL = list(BUILDERS)
# The control puts these two on a second stream, where they read the decoy: an
# asynchronous entry point and a blocking one.  (The small cut: the device cut
# of a MiB of zeros takes 31 join rounds, 20 times the cut of random bytes.)
CONTROLS = ["index_device-shift0", "cut_device_zpaq-islands"]


def _device_inputs(sc, gpu):
    real = {k: torch.from_numpy(v).to(gpu) for k, v in sc.real.items()}
    decoy = {k: torch.from_numpy(v).to(gpu) for k, v in sc.decoy.items()}
    torch.cuda.synchronize(gpu)
    return real, decoy


def _host_result(result):
    return tuple(r.cpu().numpy() if isinstance(r, torch.Tensor) else r for r in result)


@pytest.fixture(scope="module")
def scenarios(gpu):
    """Every scenario, its reference computed once, and the hold: each call is
    run on the idle default stream (once to load what a first call loads, then
    once under the host's wall clock, synchronise included; the controls'
    also on their decoys, which is what a misplaced call reads); H is ten
    times the longest, at least 5 ms."""
    built, longest, slowest = {}, 0.0, None
    for name in ALL:
        sc = BUILDERS[name](name)
        sc.want_real = sc.want(sc.real)
        real, _decoy = _device_inputs(sc, gpu)
        with _knobs(sc.knobs):
            got = _host_result(sc.call(real, {}, None))
            assert so.same(got, sc.want_real), (name, so.first_difference(got, sc.want_real))
            ms = so.timed_ms(lambda: sc.call(real, {}, None), gpu)
            if name in CONTROLS:  # the control's call reads the decoy
                ms = max(ms, so.timed_ms(lambda: sc.call(_decoy, {}, None), gpu))
        if ms > longest:
            longest, slowest = ms, name
        built[name] = sc
    H = so.hold_ms(longest)
    print(f"\nstream_order: longest call {longest:.3f} ms ({slowest}), hold H = {H:.3f} ms, "
          f"{so.cycles_per_ms(gpu):.0f} sleep cycles per ms")
    yield built, H
    print(f"\nstream_order: the shortest hold lasted {so.shortest_hold[0]:.2f} of what was asked")


def _internal_streams_busy(gpu):
    """A call that gets through only if the library's two internal streams
    do: three stages of write_to_fd, from bytes that are ready, on the default
    stream (so.fresh_stream's `beside`)."""
    ready = torch.zeros((2 << 20) + 1, dtype=U8, device=gpu)
    torch.cuda.synchronize(gpu)

    def call():
        with _knobs({"SF_TEST_STREAM_STAGE_MIB": 1}), tempfile.TemporaryFile() as f:
            device.write_to_fd(ready, f.fileno(), 0)
    return call


def _run(sc, gpu, H, call_stream=None, with_out=True, current=False):
    """The scenario behind a hold of H ms on a fresh stream S.  The call gets
    stream=S -- or `call_stream`, the control's misuse; or, with `current`,
    stream=None while S is the current stream."""
    real, decoy = _device_inputs(sc, gpu)
    S = so.fresh_stream(gpu, beside=_internal_streams_busy(gpu) if sc.internal else None)
    if call_stream == "another":
        call_stream = so.fresh_stream(gpu, [S, torch.cuda.default_stream(gpu)])
    with _knobs(sc.knobs):
        x, o = so.pending(S, real, decoy, H, sc.shift, sc.out if with_out else None)
        if current:
            with torch.cuda.stream(S):
                result = sc.call(x, o, None)
        else:
            result = sc.call(x, o, call_stream if call_stream is not None else S)
        return so.settle(S, x, decoy, result)


@pytest.mark.parametrize("name", ALL)
def test_inputs_pending_on_the_callers_stream(gpu, scenarios, name):
    built, H = scenarios
    sc = built[name]
    got = _run(sc, gpu, H)
    assert so.same(got, sc.want_real), so.first_difference(got, sc.want_real)


@pytest.mark.parametrize("name", CONTROLS)
def test_the_hold_has_teeth(gpu, scenarios, name):
    """The control: the test itself gives the call a second stream, which
    nothing orders after S.  The call runs inside the hold and must see the
    decoy -- an asynchronous entry point and a blocking one.  (No output of
    the caller's here: the 0xEE fill would land on top of the early result.)"""
    built, H = scenarios
    sc = built[name]
    got = _run(sc, gpu, H, call_stream="another", with_out=False)
    want = sc.want(sc.decoy)
    assert not so.same(want, sc.want_real)
    assert so.same(got, want), so.first_difference(got, want)


@pytest.mark.parametrize("name", ["index_device_blocks-sort1", "index_device_blocks-status-sort1"])
def test_the_default_stream_is_not_special(gpu, scenarios, name):
    """stream=None with the caller's stream made current: the path every
    wire.py wrapper takes, through _stream() inside _on."""
    built, H = scenarios
    sc = built[name]
    got = _run(sc, gpu, H, current=True)
    assert so.same(got, sc.want_real), so.first_difference(got, sc.want_real)


def test_the_images_wait_for_their_zero_fill(gpu, scenarios):
    """FileImages zero-fills its allocation on the stream that is current at
    construction; copies on another stream must land after that fill, also
    while the constructing stream is still busy.  (Before the images waited
    for the fill by an event, only the blocking upload of the copy lists on
    the constructing stream kept the two in order.)"""
    built, H = scenarios
    sc = built["FileImages"]
    real, _decoy = _device_inputs(sc, gpu)
    C = so.fresh_stream(gpu)
    S = so.fresh_stream(gpu, [C])
    with torch.cuda.stream(C):
        so.hold(C, H)
        result = sc.call(real, {}, S)  # constructed under C behind its hold, filled on S
    C.synchronize()
    S.synchronize()
    measured, asked = so.held_ms(C)
    assert measured >= asked, (measured, asked)
    got = _host_result(result)
    assert so.same(got, sc.want_real), so.first_difference(got, sc.want_real)


# ------------------------------------------------- two streams, one scratch pool

def _two_streams(gpu, H, inputs, call, want, knobs=None):
    """`call` queued on streams A and B alternately, six times, each stream
    behind its own hold and every call on inputs of its own, so the queued
    work overlaps when the holds end.  The library's pool gives a freed block
    back only to the stream that freed it: every result must be exact."""
    sets = [inputs(1000 + i) for i in range(6)]
    wants = [want(a) for a in sets]
    streams = [so.fresh_stream(gpu)]
    streams.append(so.fresh_stream(gpu, [streams[0], torch.cuda.default_stream(gpu)]))
    with _knobs(knobs or {}):
        reals, decoys = [], []  # kept until the end: the copies from them are queued behind the holds
        for k in range(2):  # stream k takes sets k, k + 2, k + 4
            mine = {f"{name}{i}": v for i in range(k, 6, 2) for name, v in sets[i].items()}
            reals.append({n: torch.from_numpy(v).to(gpu) for n, v in mine.items()})
            decoys.append({n: torch.zeros_like(t) for n, t in reals[k].items()})
        torch.cuda.synchronize(gpu)
        xs = [(so.pending(S, reals[k], decoys[k], H)[0], decoys[k]) for k, S in enumerate(streams)]
        results = []
        for i in range(6):
            x = {name: xs[i % 2][0][f"{name}{i}"] for name in sets[i]}
            results.append(call(x, streams[i % 2]))
        got = [None] * 6
        for k, S in enumerate(streams):
            mine = so.settle(S, xs[k][0], xs[k][1], [r for i in range(k, 6, 2) for r in results[i]])
            per = len(results[k])
            for j, i in enumerate(range(k, 6, 2)):
                got[i] = mine[j * per:(j + 1) * per]
    for i in range(6):
        assert so.same(got[i], wants[i]), (i, so.first_difference(got[i], wants[i]))


def test_two_streams_share_the_scratch_pool_forced_sort(gpu, scenarios):
    def call(x, s):
        return (device.index_device_blocks(x["data"], x["offsets"], x["sizes"], check_range=False, stream=s),)
    _two_streams(gpu, scenarios[1], _list_inputs, call,
                 lambda a: (oracle.index_blocks(a["data"], a["offsets"], a["sizes"]),), {"SF_TEST_TABLE_SORT": 1})


def test_two_streams_share_the_scratch_pool_block_set(gpu, scenarios):
    def call(x, s):
        bs = device.BlockSet(x["table"], x["present"], stream=s)
        rows = bs.lookup(x["queries"])
        bs.close()
        return (rows,)
    _two_streams(gpu, scenarios[1], _set_inputs, call,
                 lambda a: (oracle.block_lookup(a["table"], a["present"], a["queries"]),))


def test_two_streams_share_the_scratch_pool_copy_blocks(gpu, scenarios):
    def call(x, s):
        with torch.cuda.stream(s):
            dst = torch.full((LEN_DST,), so.PREFILL, dtype=U8, device=gpu)
        device.copy_blocks(x["src"], dst, x["so"], x["do"], x["sz"], take=x["take"], check_range=False, stream=s)
        return (dst,)
    _two_streams(gpu, scenarios[1], _copy_inputs, call, _copy_want)
