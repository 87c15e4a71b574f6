"""A plain reference for the per-file blocks_hash chain jobs
(sf_index_device_batch_chained_cols): hashlib for whole runs, and a FIPS 180-4
SHA-1 compression, written from the standard, for the state between the two
halves of a chain.  It imports nothing of this project; tests/test_chain_ref.py
holds it against hashlib before any GPU test leans on it."""
import hashlib

import numpy as np

# FIPS 180-4 section 5.3.1: the initial hash value H(0)
IV = (0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0)
# section 4.2.1: K_t for t in [0, 20), [20, 40), [40, 60), [60, 80)
K = (0x5A827999, 0x6ED9EBA1, 0x8F1BBCDC, 0xCA62C1D6)


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def _f(t, b, c, d):
    """Section 4.1.1: Ch, Parity, Maj, Parity."""
    if t < 20:
        return (b & c) ^ (~b & d)
    if 40 <= t < 60:
        return (b & c) ^ (b & d) ^ (c & d)
    return b ^ c ^ d


def _compress(h, block):
    """Section 6.1.2 for every row at once: h is five uint32[n], block is
    uint8[n, 64].  Returns the next five uint32[n]."""
    m = block.reshape(len(block), 16, 4).astype(np.uint32)  # big-endian words M_0..M_15
    words = (m[:, :, 0] << np.uint32(24)) | (m[:, :, 1] << np.uint32(16)) | (m[:, :, 2] << np.uint32(8)) | m[:, :, 3]
    w = [words[:, t] for t in range(16)]
    for t in range(16, 80):
        w.append(_rotl(w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16], 1))
    a, b, c, d, e = h
    for t in range(80):
        tmp = _rotl(a, 5) + _f(t, b, c, d) + e + np.uint32(K[t // 20]) + w[t]
        e, d, c, b, a = d, c, _rotl(b, 30), a, tmp
    return [x + y for x, y in zip(h, (a, b, c, d, e))]


def run_hashes(runs):
    """hashlib.sha1 of each row of uint8[n_files, run_len] -> uint8[n_files, 20]."""
    runs = np.asarray(runs, np.uint8)
    out = np.empty((runs.shape[0], 20), np.uint8)
    for i, row in enumerate(runs):
        out[i] = np.frombuffer(hashlib.sha1(row.tobytes()).digest(), np.uint8)
    return out


def state_after(runs, n_chunks):
    """h0..h4 of each row after its first n_chunks whole 64-byte chunks ->
    uint32[n_files, 5]."""
    runs = np.asarray(runs, np.uint8)
    n = runs.shape[0]
    assert runs.ndim == 2 and 64 * n_chunks <= runs.shape[1]
    h = [np.full(n, v, np.uint32) for v in IV]
    with np.errstate(over="ignore"):
        for c in range(n_chunks):
            h = _compress(h, runs[:, 64 * c:64 * c + 64])
    return np.stack(h, 1)


def state_bytes(states):
    """The 20 bytes the kernels keep per file between the halves of a chain:
    h0..h4 as five host-order uint32 -> uint8[n_files, 20]."""
    return np.ascontiguousarray(np.asarray(states, np.uint32)).view(np.uint8).reshape(-1, 20)


def job_chunks(blocks):
    """(run_len, data_ch, half) of a chain job over `blocks` 20-byte digests
    per file: the run's bytes, its whole 64-byte chunks, and how many of
    those part 1 takes (part 2 takes the rest and the padding)."""
    run_len = 20 * blocks
    data_ch = run_len // 64
    return run_len, data_ch, data_ch // 2
