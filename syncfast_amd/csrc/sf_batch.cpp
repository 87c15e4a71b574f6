// sf_batch.cpp -- host planning of the device-resident batch entry points:
// sf_index_device_batch, sf_index_device_batch_chained and _chained_cols.
// Nothing here launches a kernel itself: a batch is cut into calls of the
// launchers of sf_launch.hpp, so this file builds with the host compiler.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "sf_launch.hpp"

namespace sfi {

sf::PadSchedule pad_schedule(uint32_t bytes) {
  sf::PadSchedule p{};
  if (bytes == 0 || (bytes & 63u)) return p;
  // W = {0x80000000, 0 x 13, bit length hi, lo}
  uint32_t w[80] = {0};
  w[0] = 0x80000000u;
  w[14] = bytes >> 29;
  w[15] = bytes << 3;
  for (int t = 16; t < 80; t++) {
    const uint32_t x = w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16];
    w[t] = (x << 1) | (x >> 31);
  }
  for (int t = 0; t < 80; t++) {
    const uint32_t k = t < 20 ? 0x5A827999u : t < 40 ? 0x6ED9EBA1u : t < 60 ? 0x8F1BBCDCu : 0xCA62C1D6u;
    p.kw[t] = k + w[t];
  }
  p.bytes = bytes;
  return p;
}

// Many equal-size, block-aligned files back to back, with their per-file
// blocks_hash (src/index.rs:661-682), and no wave waiting for another
// (round 6).  A file's blocks_hash is one sequential SHA-1 over its digest
// run, which exists only once its blocks are hashed; the batch is therefore
// hashed as the batch stream hashes its last batch, from
// this stream's pieces (sf_stream.hip, sf_chain.hip):
//   1. block columns [0, cut) of every file (sha1_fixed_chained_kernel, no jobs);
//   2. columns [cut, nbf) beside the FIRST half of every file's chain (its
//      digests [0, cut) exist: launch 1 finished them), the SHA-1 state kept
//      in HBM;
//   3. the second half of every chain alone, with schedule-building helper
//      waves (sha1_chain_helper_kernel).
// Round 5's single fused launch (sha1_staged_kernel: chain lanes polling
// per-stage counters, bounded) gave up once in five rounds for a reason no
// probe reproduced; this form runs config 3's shape at 2.76
// ms per 8 GiB against that launch's 2.71 and 2.97 for blocks-then-chains
// (profiles/r06/batch/).  Other shapes (runs not 16-B aligned, fewer than 128
// blocks per file, not a multiple of 64 or more than 16,384, SF_BATCH_FUSED=0):
// the block kernel, then the chain kernel.  d_status is not written.
static int batch_with_hashes(const uint8_t* base, uint64_t flen, uint32_t bs, uint32_t nfiles, uint64_t nbf,
                             uint8_t* dig, uint8_t* fh, bool halves, hipStream_t s) {
  uint64_t cut = 0;
  // Files of more than 16,384 blocks (64 MiB at 4 KiB): chains of over 5,120
  // compressions run faster whole and alone with their helper waves than half
  // beside the blocks (64 x 128 MiB: 11.5 ms that way, 12.4 in halves; 16 x
  // 512 MiB 37.2 against 44.0; 256 x 32 MiB the other way, 4.89 against 4.28).
  // (the chained entry point refuses a table that is not 16-B aligned and
  // hashes that are not 4-B aligned: such a batch keeps the route below)
  if (halves && nbf % 64 == 0 && nbf >= 128 && nbf <= 16384 && (reinterpret_cast<uintptr_t>(dig) & 15) == 0 &&
      (reinterpret_cast<uintptr_t>(fh) & 3) == 0 && nbf * nfiles <= launch_max_blocks()) {
    const uint64_t half = (nbf * 20 / 64) / 2;  // data chunks of part 1 (as the chained launcher cuts them)
    const uint64_t need = ceil_div(half * 64, 20);  // digests part 1 reads
    cut = ceil_div(need, 64) * 64;                  // in whole block waves
    if (cut >= nbf) cut = 0;
  }
  if (!cut) {
    int rc = launch_fixed(base, nbf * nfiles * (uint64_t)bs, bs, nbf * nfiles, dig, s);
    if (rc) return rc;
    if (nbf % 4 == 0 && nbf * 20 <= 0xFFFFFFF0ull && (reinterpret_cast<uintptr_t>(dig) & 15) == 0) {
      // 16-B aligned runs: chains with schedule-building helper waves
      sf::ChainJob j = {}, none = {};
      j.runs = dig;
      j.hashes = fh;
      j.files = nfiles;
      j.run_len = (uint32_t)(nbf * 20);
      j.lo = 0;
      j.hi = j.run_len / 64;
      j.part = 0;
      j.waves = (uint32_t)ceil_div(nfiles, 64);
      return launch_chain_helper(j, none, s);
    }
    return launch_chain_plain(dig, nbf * 20, nfiles, (uint32_t)(nbf * 20), fh, s);
  }
  void* state = nullptr;  // every file's SHA-1 state between the two halves of its chain
  {
    const int arc = stream_alloc(&state, (size_t)nfiles * 20, s);
    if (arc != SF_OK) return arc;
  }
  const sf_chain_job first = {dig, nfiles, 1, nbf, state, nullptr};
  const sf_chain_job second = {dig, nfiles, 2, nbf, state, fh};
  int rc = sf_index_device_batch_chained_cols(base, nfiles, flen, bs, 0, cut, dig, nullptr, 0, s);
  if (rc == SF_OK) rc = sf_index_device_batch_chained_cols(base, nfiles, flen, bs, cut, nbf, dig, &first, 1, s);
  if (rc == SF_OK) rc = sf_index_device_batch_chained_cols(nullptr, 0, flen, bs, 0, nbf, nullptr, &second, 1, s);
  stream_free(state, s);
  return rc;
}

static int index_device_batch(const void* d_data, uint64_t len, const sf_file_desc* files, uint32_t n_files,
                              uint32_t block_size, void* d_digests, uint64_t cap_blocks, void* d_file_hashes,
                              uint64_t* first_block, uint64_t* n_blocks, void* stream) {
  int rc = check_block_size(block_size);
  if (rc) return rc;
  if (n_files && !files) return SF_EINVAL;
  // digests and blocks_hashes are written as dwords by every route below
  // (d_status is never written: it needs none)
  if (misaligned(d_digests, 4) || misaligned(d_file_hashes, 4)) return SF_EINVAL;
  hipStream_t s = as_stream(stream);
  // Plan: per-file block ranges (host, O(n_files)).
  std::vector<uint64_t> fb(n_files + 1);
  uint64_t total = 0;
  bool contiguous_aligned = true;  // files back to back, every file a whole number of blocks
  uint64_t expect = files && n_files ? files[0].offset : 0;
  for (uint32_t f = 0; f < n_files; f++) {
    if (files[f].offset > len || files[f].len > len - files[f].offset) return SF_ERANGE;
    fb[f] = total;
    total += files[f].len ? ceil_div(files[f].len, block_size) : 0;
    if (files[f].offset != expect || files[f].len % block_size) contiguous_aligned = false;
    expect = files[f].offset + files[f].len;
  }
  fb[n_files] = total;
  if (first_block) memcpy(first_block, fb.data(), sizeof(uint64_t) * (n_files + 1));
  if (n_blocks) *n_blocks = total;
  if (total > cap_blocks) return SF_ENOSPC;
  if (n_files == 0) return SF_OK;
  if ((!d_data && len) || (total && !d_digests)) return SF_EINVAL;  // all-empty files need no data

  // Equal-size, block-aligned, back-to-back files: the block table is a fixed
  // tiling of the batch, and each file's digest run is a fixed tiling of the
  // digest table (block = nbf*20 bytes), so nothing needs uploading.
  bool equal_files = contiguous_aligned && total > 0;
  for (uint32_t f = 1; f < n_files && equal_files; f++)
    if (files[f].len != files[0].len) equal_files = false;
  if (equal_files && total / n_files * 20 <= 0xFFFFFFFFull) {
    const uint64_t nbf = total / n_files;
    const uint8_t* base = static_cast<const uint8_t*>(d_data) + files[0].offset;
    if (!d_file_hashes)
      return launch_fixed(base, total * (uint64_t)block_size, block_size, total, d_digests, s);
    return batch_with_hashes(base, files[0].len, block_size, n_files, nbf, static_cast<uint8_t*>(d_digests),
                             static_cast<uint8_t*>(d_file_hashes), knob(K_BATCH_FUSED) != 0, s);
  }

  // Block table for the ragged case, file table for blocks_hash; one device
  // workspace, uploaded once.
  const bool need_table = !contiguous_aligned && total > 0;
  const bool need_fh = d_file_hashes != nullptr;
  // block table: offsets (u64) then sizes (u32), padded to 16 B so the file
  // table's u64 offsets that follow stay 8-B aligned (host and device)
  const size_t tbl_bytes = need_table ? (total * (sizeof(uint64_t) + sizeof(uint32_t)) + 15) & ~(size_t)15 : 0;
  const size_t fh_bytes = need_fh ? (size_t)n_files * (sizeof(uint64_t) + sizeof(uint32_t)) : 0;
  std::vector<uint8_t> host_ws(tbl_bytes + fh_bytes + 16);
  uint64_t* h_off = reinterpret_cast<uint64_t*>(host_ws.data());
  uint32_t* h_sz = reinterpret_cast<uint32_t*>(host_ws.data() + total * sizeof(uint64_t) * (need_table ? 1 : 0));
  if (need_table) {
    uint64_t i = 0;
    for (uint32_t f = 0; f < n_files; f++)
      for (uint64_t o = 0; o < files[f].len; o += block_size, i++) {
        h_off[i] = files[f].offset + o;
        h_sz[i] = (uint32_t)std::min<uint64_t>(block_size, files[f].len - o);
      }
  }
  uint64_t* h_foff = reinterpret_cast<uint64_t*>(host_ws.data() + tbl_bytes);
  uint32_t* h_fsz = reinterpret_cast<uint32_t*>(host_ws.data() + tbl_bytes + (need_fh ? n_files * sizeof(uint64_t) : 0));
  if (need_fh) {
    for (uint32_t f = 0; f < n_files; f++) {
      const uint64_t nbf = fb[f + 1] - fb[f];
      if (nbf * 20 > 0xFFFFFFFFull) return SF_EINVAL;
      h_foff[f] = fb[f] * 20;
      h_fsz[f] = (uint32_t)(nbf * 20);
    }
  }
  // Stream-ordered workspace: allocated, filled, used and freed on `s`, so
  // the call stays asynchronous.  (hipMemcpyAsync from pageable memory
  // returns once the bytes are staged, so host_ws may go out of scope.)
  uint8_t* dws = nullptr;
  const size_t ws_bytes = tbl_bytes + fh_bytes;
  if (ws_bytes) {
    if ((rc = stream_alloc(reinterpret_cast<void**>(&dws), ws_bytes, s)) != SF_OK) return rc;
    SF_HIP(hipMemcpyAsync(dws, host_ws.data(), ws_bytes, hipMemcpyHostToDevice, s));
  }
  do {
    if (total) {
      if (contiguous_aligned) {
        const uint8_t* base = static_cast<const uint8_t*>(d_data) + files[0].offset;
        rc = launch_fixed(base, fb[n_files] * (uint64_t)block_size, block_size, total, d_digests, s);
      } else {
        rc = launch_table(d_data, len, reinterpret_cast<const uint64_t*>(dws),
                          reinterpret_cast<const uint32_t*>(dws + total * sizeof(uint64_t)), total, d_digests,
                          nullptr, s);
      }
      if (rc) break;
    }
    if (need_fh) {
      // blocks_hash of every file at once: one lane per file hashes its own
      // run of 20-byte digests (a file with no blocks hashes the empty string).
      const uint8_t* dg =
          total ? static_cast<const uint8_t*>(d_digests) : static_cast<const uint8_t*>(d_file_hashes);
      rc = launch_table(dg, total * 20, reinterpret_cast<const uint64_t*>(dws + tbl_bytes),
                        reinterpret_cast<const uint32_t*>(dws + tbl_bytes + n_files * sizeof(uint64_t)), n_files,
                        d_file_hashes, nullptr, s);
    }
  } while (0);
  stream_free(dws, s);
  return rc;
}

}  // namespace sfi

using namespace sfi;

extern "C" {

// The body above, exceptions turned into error codes.
int sf_index_device_batch(const void* d_data, uint64_t len, const sf_file_desc* files, uint32_t n_files,
                          uint32_t block_size, void* d_digests, uint64_t cap_blocks, void* d_file_hashes,
                          uint64_t* first_block, uint64_t* n_blocks, int* d_status, void* stream) {
  (void)d_status;
  return guarded([&] {
    return index_device_batch(d_data, len, files, n_files, block_size, d_digests, cap_blocks, d_file_hashes,
                              first_block, n_blocks, stream);
  });
}

int sf_index_device_batch_chained(const void* d_data, uint32_t n_files, uint64_t file_len, uint32_t block_size,
                                  void* d_digests, const sf_chain_job* jobs, uint32_t n_jobs, void* stream) {
  const uint64_t nbf = block_size ? file_len / block_size : 0;
  return sf_index_device_batch_chained_cols(d_data, n_files, file_len, block_size, 0, nbf, d_digests, jobs, n_jobs,
                                            stream);
}

int sf_index_device_batch_chained_cols(const void* d_data, uint32_t n_files, uint64_t file_len, uint32_t block_size,
                                       uint64_t col_lo, uint64_t col_hi, void* d_digests, const sf_chain_job* jobs,
                                       uint32_t n_jobs, void* stream) {
  int rc = check_block_size(block_size);
  if (rc) return rc;
  if (n_files && (file_len == 0 || file_len % block_size)) return SF_EINVAL;
  if (n_jobs > 2 || (n_jobs && !jobs)) return SF_EINVAL;
  const uint64_t nbf = file_len / block_size;
  // the whole files, or a column range in whole block waves of whole-wave files
  const bool whole = col_lo == 0 && col_hi == nbf;
  if (n_files && !whole && (col_lo >= col_hi || col_hi > nbf || nbf % 64 || col_lo % 64 || col_hi % 64))
    return SF_EINVAL;
  const uint64_t total = n_files ? nbf * n_files : 0;
  if (total && (!d_data || !d_digests)) return SF_EINVAL;
  if (total > launch_max_blocks()) return SF_EINVAL;  // one launch per batch: split the batch
  sf::ChainJob cj[2] = {};
  for (uint32_t k = 0; k < n_jobs; k++) {
    const sf_chain_job& j = jobs[k];
    if (!j.n_files) continue;
    // each file's digest run must start 16-B aligned: the table does, and
    // 20 * blocks % 16 == 0 (both chain kernels read the runs as uint4)
    if (!j.d_digests || j.blocks == 0 || j.blocks % 4 || j.blocks * 20 > 0xFFFFFFF0ull || j.part > 2 ||
        (j.part != 0 && !j.d_state) || (j.part != 1 && !j.d_hashes))
      return SF_EINVAL;
    // d_state and d_hashes are read and written as uint32 words
    if (misaligned(j.d_digests, 16) || misaligned(j.d_state, 4) || misaligned(j.d_hashes, 4)) return SF_EINVAL;
    const uint32_t run_len = (uint32_t)(j.blocks * 20), data_ch = run_len / 64, half = data_ch / 2;
    cj[k].runs = static_cast<const uint8_t*>(j.d_digests);
    cj[k].state = static_cast<uint8_t*>(j.d_state);
    cj[k].hashes = static_cast<uint8_t*>(j.d_hashes);
    cj[k].files = j.n_files;
    cj[k].run_len = run_len;
    cj[k].lo = j.part == 2 ? half : 0;
    cj[k].hi = j.part == 1 ? half : data_ch;
    cj[k].part = j.part;
    cj[k].waves = (uint32_t)ceil_div(j.n_files, 64);  // chain waves, one per workgroup
  }
  const uint32_t wpf = whole ? 1u : (uint32_t)(nbf / 64), wpp = whole ? 1u : (uint32_t)((col_hi - col_lo) / 64);
  const uint64_t bwaves = whole ? ceil_div(total, 64) : (uint64_t)n_files * wpp;
  if (total == 0) return launch_chain_helper(cj[0], cj[1], as_stream(stream));  // chains alone: helper waves
  // A chain wave of the block launch stages 64 files' runs through one
  // buffer resource with 32-bit offsets (file b of the wave at b * run_len):
  // runs of 62.9 MB or more (3.1 M blocks per file) could pass 4 GiB within
  // one wave and wrap.  Such a job runs first, alone, on the helper-wave
  // chain kernel (64-bit addressing), stream-ordered before this launch:
  // its digests and states were completed by earlier launches.
  for (int k = 0; k < 2; k++) {
    if (!cj[k].waves || 64ull * cj[k].run_len + 128 <= 0xF0000000ull) continue;
    const sf::ChainJob none = {};
    if ((rc = launch_chain_helper(cj[k], none, as_stream(stream))) != SF_OK) return rc;
    cj[k] = none;
  }
  return launch_chained(static_cast<const uint8_t*>(d_data), total * (uint64_t)block_size, block_size, total,
                        static_cast<uint8_t*>(d_digests), pad_schedule(block_size), cj[0], cj[1], bwaves, wpf, wpp,
                        whole ? 0u : (uint32_t)(col_lo / 64), as_stream(stream));
}

}  // extern "C"
