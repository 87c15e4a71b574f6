"""The reference's content-defined (ZPAQ) chunker in the library, on the host:
sf_zpaq_cut_buffer (the definition of the boundaries), sf_zpaq_chunker_ops
(the same chunker for sf_cut_fd on N threads) and index.ZpaqChunker.

Every comparison is exact equality.  `zpaq_cuts` below is an independent
restatement of the recurrence in Python; the known-answer test is the
reference's own (src/index.rs:761-792, tests/golden/golden.json)."""
import ctypes
import hashlib
import os
import random
from pathlib import PurePath

import numpy as np
import pytest

import oracle
import syncfast_amd
from syncfast_amd import _lib, host
from syncfast_amd.digest import HashDigest
from syncfast_amd.index import Index, NativeChunker, ZpaqChunker

HM = 123456791
PARAMS = [(6, 256), (8, 1024), (13, 32768), (1, 16), (31, 4096)]
N = 150_000


def zpaq_cuts(data, bits=13, max_size=32768):  # -> [(offset, size)]
    lim = 1 << (32 - bits)
    out = []
    start = 0
    h, c1, o1 = HM, 0, [0] * 256  # fresh state: h = HM, not 0
    for i, b in enumerate(data):
        h = (h * HM * (1 if b == o1[c1] else 2) + b + 1) & 0xFFFFFFFF
        o1[c1] = b
        c1 = b
        if h < lim or i + 1 - start == max_size:  # cut AFTER byte i
            out.append((start, i + 1 - start))
            start = i + 1
            h, c1, o1 = HM, 0, [0] * 256  # restart at every cut
    if start < len(data):
        out.append((start, len(data) - start))
    return out


def word_salad(n, seed):
    rng = random.Random(seed)
    words = [b"alpha", b"beta", b"gamma", b"delta", b"the", b"of", b"and", b"sync", b"block", b"signature",
             b"index", b"file", b"\n"]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + b" "
    return bytes(out[:n])


def zpaq_inputs(n=N):
    """The six inputs of the comparison, by name."""
    rnd = random.Random(20260)
    return {
        "random": rnd.randbytes(n),
        "text": word_salad(n, 1),
        "zeros": bytes(n),
        "ff": b"\xff" * n,
        "period13": (b"Test content\n" * (n // 13 + 1))[:n],
        "random_then_zeros": rnd.randbytes(5000) + bytes(n - 5000),
    }


def lib_cuts(data, bits, max_size):
    offs, sizes = host.zpaq_cut_buffer(data, bits, max_size)
    return list(zip(offs.tolist(), sizes.tolist()))


def test_kat_boundaries_digests_and_blocks_hash(golden):
    g = golden["reference_kat"]
    data = oracle.kat_input()
    got = lib_cuts(data, 13, 32768)
    assert got == [(b["offset"], b["size"]) for b in g["blocks"]]
    assert got == [(0, 11579), (11579, 32768), (44347, 546)]
    digs = [host.sha1(data[o:o + s]) for o, s in got]
    assert [d.hex() for d in digs] == [b["sha1"] for b in g["blocks"]]
    assert host.blocks_hash(b"".join(digs)).hex() == g["blocks_hash"]
    assert zpaq_cuts(data) == got


@pytest.fixture(scope="module")
def inputs():
    return zpaq_inputs()


@pytest.mark.parametrize("bits,max_size", PARAMS)
def test_cut_buffer_equals_the_python_restatement(inputs, bits, max_size):
    for name, data in inputs.items():
        want = zpaq_cuts(data, bits, max_size)
        assert lib_cuts(data, bits, max_size) == want, name
        assert sum(s for _o, s in want) == len(data) and all(0 < s <= max_size for _o, s in want)
    base = inputs["random"]
    for n in (0, 1, max_size - 1, max_size, max_size + 1):
        for data in (base[:n], bytes(n)):
            assert lib_cuts(data, bits, max_size) == zpaq_cuts(data, bits, max_size), n


# every (bits, max_size) pair the device join is tested at (test_gpu_zpaq_join.py)
JOIN_PARAMS = [(6, 256), (5, 48), (6, 17), (7, 100), (4, 33), (9, 1023), (1, 16), (31, 4096), (13, 1 << 20),
               (20, 1 << 20), (8, 16)]


@pytest.mark.parametrize("bits,max_size", JOIN_PARAMS)
def test_cut_buffer_equals_the_python_restatement_on_islands(bits, max_size):
    """The host cutter is the reference of the device join's tests: held
    against `zpaq_cuts` at each of their parameter pairs, on that file's kind
    of input (random stretches alternating with periodic ones)."""
    from zpaq_join import islands
    data = islands(1024, 20261)
    assert len(data) >= 20_000
    if (bits, max_size) in ((13, 1 << 20), (9, 1023)):
        # long enough to hold a forced cut.  In "1 1 2 2 ..." every byte follows its
        # predecessor for the other time round, so every step multiplies h by 2 HM:
        # h is a function of the last 32 bytes, four values in all, none below 2^23.
        data += b"\x01\x01\x02\x02" * (max_size // 4 + 1025) + data[:4097]
    want = zpaq_cuts(data, bits, max_size)
    assert lib_cuts(data, bits, max_size) == want
    assert sum(s for _o, s in want) == len(data) and all(0 < s <= max_size for _o, s in want)
    if (bits, max_size) in ((13, 1 << 20), (9, 1023), (31, 4096)):
        assert any(s == max_size for _o, s in want[:-1])


def test_device_cut_parameter_limits_clear_the_count():
    """sf_cut_device_zpaq at the first values outside its range: SF_EINVAL
    and *n_blocks = 0, before any device work (test_argument_validation_
    without_device checks the return codes alone)."""
    L = syncfast_amd.lib()
    for bits, max_size in ((13, 15), (13, (1 << 20) + 1), (0, 256), (32, 256)):
        n = ctypes.c_uint64(77)
        assert L.sf_cut_device_zpaq(1 << 20, 100, bits, max_size, None, None, 0, ctypes.byref(n), None) == \
            _lib.SF_EINVAL
        assert n.value == 0, (bits, max_size)


@pytest.fixture(scope="module")
def text_file(tmp_path_factory):
    data = word_salad(20 << 20, 2)
    p = tmp_path_factory.mktemp("zpaq") / "text"
    p.write_bytes(data)
    return p, zpaq_cuts(data)


@pytest.mark.parametrize("threads", [1, 4])
def test_cut_fd_with_the_zpaq_ops(text_file, threads):
    """sf_cut_fd over sf_zpaq_chunker_ops: the restatement's list for a 20 MiB
    file (five 4 MiB segments at threads=4), whatever the thread count."""
    p, want = text_file
    ops = host.ZpaqOps()
    with open(p, "rb") as f:
        offs, sizes = host.cut_fd(f.fileno(), ops.address, threads, host.file_stamp(f.fileno()))
    assert list(zip(offs.tolist(), sizes.tolist())) == want


def test_zpaq_chunker_is_a_native_chunker():
    ch = ZpaqChunker()
    assert isinstance(ch, NativeChunker) and ch.stream and not ch.device and (ch.bits, ch.max_size) == (13, 32768)
    assert ch._cut_bytes(oracle.kat_input()) == [11579, 32768, 546]
    assert ch._cut_bytes(b"") == []
    small = ZpaqChunker(bits=6, max_size=256)
    data = zpaq_inputs(20_000)["text"]
    assert small._cut_bytes(data) == [s for _o, s in zpaq_cuts(data, 6, 256)]


@pytest.mark.gpu
def test_index_kat_with_no_boundaries_handed_in(gpu, tmp_path):
    """src/index.rs:747-793: the reference's own test, the blocks cut by the
    library's chunker (test_reference_index_kat is given its boundaries)."""
    p = tmp_path / "kat"
    p.write_bytes(oracle.kat_input())
    name = PurePath("dir/name")
    index = Index.open_in_memory(chunker=ZpaqChunker())
    index.index_file(p, name)
    index.commit()
    assert index.get_block(HashDigest(b"12345678901234567890")) is None
    block1 = index.get_block(HashDigest(bytes.fromhex("fb5ef7ebadd82c8085c5ff63823622bae0e263f6")))
    assert block1 == (name, 0, 11579)
    block2 = index.get_block(HashDigest(bytes.fromhex("570d8b30fcfd585e4127b561f5ecd376ff4d0101")))
    assert block2 == (name, 11579, 32768)
    block3 = index.get_block(HashDigest(bytes.fromhex("b9a8c2641af2cf8fd8f36a2456a3eaa95c029127")))
    assert block3 == (name, 44347, 546)
    assert block3[1] - block2[1] == 1 << 15  # MAX_BLOCK_SIZE
    file1 = index.get_file(name)
    assert file1[0] == 1
    assert file1[2] == HashDigest(bytes.fromhex("84c25d78edcdb67631639c43604cf0149564f044"))


def test_argument_validation_without_device(tmp_path):
    L = syncfast_amd.lib()
    data = np.frombuffer(random.Random(5).randbytes(4096), np.uint8)
    n = ctypes.c_uint64(77)
    o, z = np.zeros(64, np.uint64), np.zeros(64, np.uint32)

    def cut(bits, max_size, cap=64, length=data.size, d=data.ctypes.data, pn=ctypes.byref(n)):
        return L.sf_zpaq_cut_buffer(d, length, bits, max_size, o.ctypes.data, z.ctypes.data, cap, pn)

    E = _lib.SF_EINVAL
    assert cut(0, 256) == E and cut(32, 256) == E and cut(13, 0) == E
    assert cut(13, 256, pn=None) == E and cut(13, 256, d=None) == E
    assert cut(13, 256, length=0, d=None) == 0 and n.value == 0
    assert cut(1, 1 << 31, length=40) == 0  # bits 1..31 and any max_size >= 1 are the host range
    want = zpaq_cuts(data.tobytes(), 13, 256)
    k = len(want)
    assert 16 <= k < 64
    assert cut(13, 256, cap=k) == 0 and n.value == k
    o[:] = 0
    assert cut(13, 256, cap=k - 1) == _lib.SF_ENOSPC and n.value == k  # the need
    assert o[k - 1] == 0 and list(zip(o[:k - 1].tolist(), z[:k - 1].tolist())) == want[:k - 1]  # nothing past cap
    assert L.sf_zpaq_cut_buffer(data.ctypes.data, data.size, 13, 256, None, None, 0, ctypes.byref(n)) == \
        _lib.SF_ENOSPC and n.value == k  # a query
    ops = host.ZpaqOps(6, 256)
    assert ops.create and ops.next and ops.destroy and ops.ctx
    for bits, max_size in ((0, 256), (32, 256), (13, 0)):
        with pytest.raises(_lib.SfError) as e:
            host.ZpaqOps(bits, max_size)
        assert e.value.code == E
    assert L.sf_zpaq_chunker_ops(13, 32768, None) == E
    # the device forms check their parameters before any device work: the
    # device range of max_size is 16 .. 2^20
    for bits, max_size in ((0, 256), (32, 256), (13, 15), (13, (1 << 20) + 1)):
        assert L.sf_cut_device_zpaq(1 << 20, 100, bits, max_size, None, None, 0, ctypes.byref(n), None) == E
        assert L.sf_index_device_zpaq(1 << 20, 100, bits, max_size, None, None, None, 0, ctypes.byref(n), None,
                                      None) == E
    assert L.sf_cut_device_zpaq(None, 100, 13, 32768, None, None, 0, ctypes.byref(n), None) == E  # no data
    assert L.sf_cut_device_zpaq(None, 100, 13, 32768, None, None, 0, None, None) == E
    n.value = 77
    assert L.sf_cut_device_zpaq(None, 0, 13, 32768, None, None, 0, ctypes.byref(n), None) == 0 and n.value == 0
    bh = (ctypes.c_uint8 * 20)()
    assert L.sf_index_device_zpaq(None, 0, 13, 32768, None, None, None, 0, ctypes.byref(n), bh, None) == 0
    assert bytes(bh) == hashlib.sha1(b"").digest()
    rows = ctypes.POINTER(_lib.BlockSig)()
    pr = ctypes.byref(rows)
    assert L.sf_index_fd_zpaq(-1, None, 13, 32768, pr, ctypes.byref(n), bh) == E
    p = tmp_path / "f"
    p.write_bytes(b"x" * 1000)
    e0 = tmp_path / "empty"
    e0.write_bytes(b"")
    with open(p, "rb") as f:
        assert L.sf_index_fd_zpaq(f.fileno(), None, 13, 8, pr, ctypes.byref(n), bh) == E
        assert L.sf_index_fd_zpaq(f.fileno(), None, 13, 32768, None, ctypes.byref(n), bh) == E
        stale = host.file_stamp(f.fileno())
        stale.ctime_nsec += 1
        assert L.sf_index_fd_zpaq(f.fileno(), ctypes.byref(stale), 13, 32768, pr, ctypes.byref(n), bh) == \
            _lib.SF_EAGAIN
    with open(e0, "rb") as f:  # an empty file: no blocks, SHA1(""), no device needed
        got, h = host.index_fd_zpaq(f.fileno(), stamp=host.file_stamp(f.fileno()))
        assert got.size == 0 and h == hashlib.sha1(b"").digest()
    r, w = os.pipe()
    try:
        assert L.sf_index_fd_zpaq(r, None, 13, 32768, pr, ctypes.byref(n), bh) == E  # not a regular file
    finally:
        os.close(r)
        os.close(w)


def test_host_cutter_under_asan_ubsan(tmp_path):
    """examples/zpaq_cut.c + the host cutter's one translation unit, built
    with ASan + UBSan as a stand-alone program (what `make -C examples
    asan-zpaq` builds): its built-in inputs, and the KAT file's blocks."""
    import subprocess
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void){return 0;}\n")
    if subprocess.run(["gcc", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode:
        pytest.skip("gcc -fsanitize=address,undefined unavailable")
    subprocess.run(["gcc", *san, "-Wall", "-I", os.path.join(root, "include"), "-c",
                    os.path.join(root, "examples", "zpaq_cut.c"), "-o", str(tmp_path / "zpaq_cut.o")], check=True)
    subprocess.run(["g++", *san, "-std=c++17", "-c", os.path.join(root, "syncfast_amd", "csrc", "sf_zpaq.cpp"),
                    "-o", str(tmp_path / "sf_zpaq.o")], check=True)
    exe = tmp_path / "zpaq_cut"
    subprocess.run(["g++", "-fsanitize=address,undefined", str(tmp_path / "zpaq_cut.o"), str(tmp_path / "sf_zpaq.o"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "periodic" in r.stdout and not r.stderr, r.stderr[-2000:]
    kat = tmp_path / "kat"
    kat.write_bytes(oracle.kat_input())
    r = subprocess.run([str(exe), "-p", "7", str(kat)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    assert r.stdout.split("\n")[1:4] == ["0 11579", "11579 32768", "44347 546"]
