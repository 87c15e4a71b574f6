"""CPU: tests/chain_ref.py, the reference of the GPU chain-job tests, against
hashlib and against the library's own arithmetic, before anything leans on it."""
import hashlib
import struct

import numpy as np
import pytest

import chain_ref
from syncfast_amd.device import BatchStream


def _padded(msg: bytes) -> bytes:
    """FIPS 180-4 section 5.1.1 by hand: 0x80, zeros to 56 mod 64, the bit
    length as a big-endian 64-bit word."""
    out = msg + b"\x80"
    out += bytes((56 - len(out)) % 64)
    return out + struct.pack(">Q", 8 * len(msg))


def _contents(n):
    rng = np.random.default_rng(0xC4A1 + n)
    return {"random": rng.integers(0, 256, n, dtype=np.uint8).tobytes(), "zeros": bytes(n), "ones": b"\xff" * n}


@pytest.mark.parametrize("n", [0, 55, 56, 63, 64, 80, 1200])
def test_state_after_all_chunks_is_hashlib(n):
    msgs = _contents(n)
    padded = [_padded(m) for m in msgs.values()]
    assert len({len(p) for p in padded}) == 1 and len(padded[0]) % 64 == 0
    assert len(padded[0]) == ((n + 8) // 64 + 1) * 64
    rows = np.frombuffer(b"".join(padded), np.uint8).reshape(len(padded), -1)
    st = chain_ref.state_after(rows, rows.shape[1] // 64)
    assert st.dtype == np.uint32 and st.shape == (3, 5)
    for name, m, s in zip(msgs, msgs.values(), st):
        assert struct.pack(">5I", *(int(v) for v in s)) == hashlib.sha1(m).digest(), (n, name)


def test_state_after_zero_chunks_is_the_initial_vector():
    rows = np.frombuffer(_contents(128)["random"], np.uint8).reshape(2, 64)
    st = chain_ref.state_after(rows, 0)
    assert st.tolist() == [[0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]] * 2
    # a chunk changes it, and a partial count stops where it says
    one = chain_ref.state_after(rows, 1)
    assert (one != st).any(axis=1).all()
    both = np.concatenate([rows, rows[::-1]], axis=1)
    assert np.array_equal(chain_ref.state_after(both, 1), one)


def test_run_hashes_and_state_bytes():
    rows = np.frombuffer(_contents(3 * 80)["random"], np.uint8).reshape(3, 80)
    got = chain_ref.run_hashes(rows)
    assert got.dtype == np.uint8 and got.shape == (3, 20)
    assert [bytes(r) for r in got] == [hashlib.sha1(bytes(r)).digest() for r in rows]
    assert chain_ref.run_hashes(np.zeros((0, 80), np.uint8)).shape == (0, 20)
    sb = chain_ref.state_bytes(np.array([[1, 0x01020304, 0xFFFFFFFF, 0, 0x80000000]], np.uint32))
    assert sb.dtype == np.uint8 and sb.shape == (1, 20)
    assert bytes(sb[0]) == struct.pack("=5I", 1, 0x01020304, 0xFFFFFFFF, 0, 0x80000000)


def test_job_chunks_table_and_batch_stream_half():
    # (run_len, data chunks, chunks of part 1) written out by hand
    assert chain_ref.job_chunks(4) == (80, 1, 0)
    assert chain_ref.job_chunks(16) == (320, 5, 2)
    assert chain_ref.job_chunks(24) == (480, 7, 3)
    assert chain_ref.job_chunks(60) == (1200, 18, 9)
    for nbf in range(128, 4097, 64):
        run_len, data_ch, half = chain_ref.job_chunks(nbf)
        cut = BatchStream(3, nbf * 64, 64)._half_cols()
        # _half_cols cuts at the first whole block wave that holds the digests
        # of `half` chunks: its half is the one job_chunks states
        assert cut == -(-(-(-half * 64 // 20)) // 64) * 64, nbf
        assert (cut - 64) * 20 < half * 64 <= cut * 20 and (half + 1) * 2 > data_ch >= half * 2, nbf
