// sf_table.hip -- explicit block lists: the 144-B
// slot staging of blocks at any byte offset, sha1_table_kernel, and the host
// side that decides how a list is launched (sorted by length class or not, in
// how many pieces).
//
// Its own translation unit: its code object holds sha1_table_kernel's two
// forms alone, and its compiler options (TABLEFLAGS) can differ from the
// other block kernels'.  It shares the wave functions of sf_block_hash.hpp
// with them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "sf_block_hash.hpp"
#include "sf_device.hpp"

namespace sf {

// ------------------------------------------- explicit lists at any offset
// The reference's default blocks are content-defined (cdchunking ZPAQ,
// src/index.rs:622-625): they start at any byte.  A wave of such blocks still
// stages them through LDS by DMA (round 3):
//   * step t stages 9 pieces of 16 B of every block, [a + 128t, a + 128t +
//     144) with a = off rounded down to 4 B (the DMA takes any dword-aligned
//     source), which holds the block's message bytes [off + 128t, off + 128t
//     + 128) whatever off & 3 is;
//   * a block's 9 pieces sit back to back in LDS (144-B slots, 9 KiB per
//     wave), so one DMA wave-instruction reads ~7 blocks x 144 contiguous
//     bytes, and with a slot stride of 9 quads the lanes' ds_read_b128 are
//     conflict-free;
//   * one v_perm per word shifts by off & 3 and byte-swaps at once (selector
//     in a VGPR): as many VALU as the aligned path's plain byte swap;
//   * a lane's last chunks (the partial one with the 0x80 byte, and the
//     length) are built from the same LDS words, so no lane issues a global
//     load of its own; chunks past a lane's message are skipped (exec mask),
//     which in a length-sorted wave costs ~1 chunk of 130.
// Each 128-B line of a block is touched by two consecutive steps (the window
// is 144 B and advances 128 B); the second touch is an L2 hit ~80 % of the
// time with the default cache policy (PMC: 1.21x the algorithmic bytes).
// With nt on every piece it was 1.95x; nt on the first 8 pieces and the
// default on the 9th (a 9th DMA instruction) 1.42x, since the 8-piece window
// itself ends in the next line (profiles/r03/).
constexpr int kListPieces = 9;

// Cache policy of the slot DMA: the default (0), not the aligned path's nt
// (see above).
constexpr int kListLoadAux = 0;

// Words of chunk c of a message of `size` bytes whose data words (already
// big-endian) are in w: keep the rem = size - 64c data bytes, then the 0x80
// byte, zeros, and the bit length if c is the last chunk (nch - 1).
__device__ __forceinline__ void finish_chunk(uint32_t (&w)[16], uint32_t size, uint32_t c, uint32_t nch) {
  // size < 0xF0000000 on the slot path, so c * 64 does not wrap; the
  // difference is taken in uint32 and then read as signed: a padding-only
  // chunk (c * 64 > size) gives a small negative rem for sizes >= 2^31 too
  const int rem = (int)(size - c * 64u);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int v = rem - 4 * j;  // data bytes in word j
    uint32_t x;
    if (v >= 4) x = w[j];
    else if (v > 0) x = (w[j] & (0xFFFFFFFFu << (32 - 8 * v))) | (0x80u << (24 - 8 * v));
    else if (v == 0) x = 0x80000000u;
    else x = 0u;
    w[j] = x;
  }
  if (c + 1 == nch) {
    w[14] = size >> 29;
    w[15] = size << 3;
  }
}

// A lane's 36 dwords of one step out of its 144-B LDS slot (9 b128 reads;
// a slot stride of 9 quads puts any 16 lanes' reads on 16 distinct bank
// quads).  Per-lane dword reads at (off & 15) >> 2 from 16-B aligned pieces
// were tried first: 4-way bank conflicts, no faster (profiles/r03/).
__device__ __forceinline__ void list_read(uint32_t (&d)[36], const uint4* myq) {
#pragma unroll
  for (int k = 0; k < kListPieces; ++k) {
    const uint4 v = myq[k];
    d[4 * k + 0] = v.x;
    d[4 * k + 1] = v.y;
    d[4 * k + 2] = v.z;
    d[4 * k + 3] = v.w;
  }
}

// Step t of nsteps: wait for its DMA, take this lane's dwords out of its
// slot, and issue step t + 1's DMA behind them.
__device__ __forceinline__ void list_step(uint32_t (&d)[36], const uint4* myq, const uint8_t* span_ptr,
                                          uint64_t span4, uint32_t t, uint32_t nsteps,
                                          const uint32_t (&voff)[kListPieces], uint4* wave_tile) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  list_read(d, myq);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (t + 1 < nsteps) issue_dma<kListPieces, 128, kListLoadAux>(span_ptr, span4, t + 1, voff, wave_tile);
}

// Hash this lane's block (off, size) of an explicit list through 144-B LDS
// slots; all 64 lanes enter together.  base = the wave's lowest block start
// rounded down to 16 B; span = bytes from base to the wave's highest block
// end (< 4 GiB); data 16-B aligned.  The DMA is range-checked per dword
// against span rounded up to 4 B: it reads only dwords that hold a byte of
// the wave's span (past it, zeros).
__device__ __forceinline__ void hash_wave_list(const uint8_t* __restrict__ data, uint64_t off, uint32_t size,
                                               bool valid, uint64_t base, uint64_t span, uint4* __restrict__ wave_tile,
                                               Sha1& st) {
  const int lane = lane_id();
  st.init();
  // compressions of this lane's message (the slot path's blocks are < 3.75
  // GiB, so the 32-bit form cannot wrap; the wide form cost 5 spilled VGPRs)
  const uint32_t nch = n_chunks(size);
  const uint32_t mine = valid ? size / 64u : 0u;       // its whole data chunks
  const uint32_t nsteps = wave_max_u32(valid ? (nch + 1u) / 2u : 0u);
  const uint32_t rel = valid ? (uint32_t)((off & ~3ull) - base) : 0u;  // pieces start at the block's dword
  uint32_t voff[kListPieces];
#pragma unroll
  for (int j = 0; j < kListPieces; ++j) {
    const int p = 64 * j + lane;  // piece p of the tile: block p / 9, piece p % 9
    const uint32_t rel_b = (uint32_t)__shfl((int)rel, p / kListPieces, 64);
    voff[j] = rel_b + 16u * (uint32_t)(p % kListPieces);
  }
  const uint4* myq = wave_tile + lane * kListPieces;  // 144-B slots
  const uint32_t sel = 0x00010203u + ((uint32_t)off & 3u) * 0x01010101u;  // shift by off & 3, then byte swap
  const uint8_t* span_ptr = data + base;
  const uint64_t span4 = (span + 3u) & ~3ull;  // range-checked per dword: a dword holding a block byte is read
  // Steps in which every lane has two whole data chunks run branch-free (one
  // basic block per step: the scheduler interleaves the two compressions, as
  // in the aligned path); only the wave's last steps test each lane.
  const uint32_t nfast = wave_min_u32(valid ? mine / 2u : 0xFFFFFFFFu);
  if (nsteps > 0) issue_dma<kListPieces, 128, kListLoadAux>(span_ptr, span4, 0, voff, wave_tile);
  uint32_t t = 0;
  for (; t < nfast; ++t) {
    uint32_t d[36];
    list_step(d, myq, span_ptr, span4, t, nsteps, voff, wave_tile);
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      uint32_t w[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) w[j] = __builtin_amdgcn_perm(d[16 * ch + j + 1], d[16 * ch + j], sel);
      st.compress(w);
    }
  }
  for (; t < nsteps; ++t) {
    uint32_t d[36];
    list_step(d, myq, span_ptr, span4, t, nsteps, voff, wave_tile);
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const uint32_t c = 2 * t + ch;
      uint32_t w[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) w[j] = __builtin_amdgcn_perm(d[16 * ch + j + 1], d[16 * ch + j], sel);
      if (c < nch) {
        if (c >= mine) finish_chunk(w, size, c, nch);
        st.compress(w);
      }
    }
  }
}

constexpr int kTableWavesPerSimd = 3;  // waves/SIMD the explicit-list kernel's register budget is sized for
constexpr int kTableWG = 4;             // its waves per workgroup
constexpr uint32_t kTableRound = 1024u; // waves per dispatch round: MI355X's SIMDs (256 CUs x 4)
constexpr uint32_t kTableReversedRounds = 2u;  // bit r: round r takes its groups in reverse (round 1 only)

// Explicit block list: block i = data[offsets[i], offsets[i] + sizes[i]).
// Used for content-defined boundaries, the reference KAT boundaries, ragged
// many-file batches, and (over the digest table) per-file blocks_hash.
// A block outside [0, len) is not read: its digest is zeroed and *status is
// set to -34 (SF_ERANGE).
// Group g of the list = 64 blocks, one lane each: order[64g .. 64g + 63] when
// the launcher sorted the list (each digest is written at the block's own
// index), else blocks 64g .. 64g + 63.
template <int TILE, bool WEAK>
__device__ __forceinline__ void table_group(const uint8_t* __restrict__ data, uint64_t len,
                                            const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ sizes,
                                            uint64_t nblocks, uint8_t* __restrict__ digests, int* __restrict__ status,
                                            uint32_t* __restrict__ weak, const uint32_t* __restrict__ order,
                                            uint64_t g, uint4* __restrict__ tile) {
  const int lane = lane_id();
  const uint64_t first = g * 64;
  bool valid = first + lane < nblocks;
  const uint64_t blk = (order && valid) ? (uint64_t)order[first + lane] : first + lane;
  uint64_t off = 0;
  uint32_t size = 0;
  bool bad = false;
  if (valid) {
    off = offsets[blk];
    size = sizes[blk];
    if (off > len || (uint64_t)size > len - off) {
      bad = true;
      off = 0;
      size = 0;
    }
  }
  WaveGeo geo;
  const uint64_t lo = wave_min_u64(valid ? off : ~0ull);
  const uint64_t hi = wave_max_u64(valid ? off + size : 0ull);
  geo.base = lo;
  geo.span = hi - lo;
  geo.min_size = wave_min_u32(valid ? size : 0xFFFFFFFFu);
  geo.max_size = wave_max_u32(valid ? size : 0u);
  geo.max_nch = wave_max_u32(valid ? n_chunks_wide(size) : 0u);
  const bool aligned = !valid || ((off & 15u) == 0);
  geo.lds_ok = __builtin_amdgcn_readfirstlane(__all(aligned)) &&
               ((reinterpret_cast<uintptr_t>(data) & 15u) == 0) && geo.span < 0xF0000000ull;
  const uint32_t rel = valid ? (uint32_t)(off - lo) : 0u;

  Sha1 st;
  Adler wk;
  // The slot path also takes aligned waves whose blocks differ in size: the
  // aligned path stages only the wave's shortest block's chunks through LDS
  // and loads the rest per lane (a CDC-like list laid out 16-B aligned: 2772
  // GiB/s that way, 3045 through the slots; equal 8 KiB blocks: 3165 aligned,
  // 3138 at byte offsets through the slots; profiles/r03/cdcx/).
  const uint64_t lo16 = lo & ~15ull;
  const bool list_path = !WEAK && (!geo.lds_ok || geo.min_size != geo.max_size) &&
                         ((reinterpret_cast<uintptr_t>(data) & 15u) == 0) && hi - lo16 < 0xF0000000ull;
  if (list_path)
    hash_wave_list(data, off, size, valid, lo16, hi - lo16, tile, st);
  else
    hash_wave<TILE, false, WEAK>(data, off, size, rel, valid, geo, tile, st, PadSchedule{}, wk);
  if (valid) {
    if (bad) {
      uint32_t* o = reinterpret_cast<uint32_t*>(digests + blk * 20);
      o[0] = o[1] = o[2] = o[3] = o[4] = 0;
      if constexpr (WEAK) weak[blk] = 0u;
      if (status) *status = SF_ERANGE;
    } else {
      st.store(digests + blk * 20);
      if constexpr (WEAK) weak[blk] = wk.fin();
    }
  }
}

// The explicit-list kernel: wave w of the grid hashes group w (one group of
// 64 blocks per wave, kTableWG waves per workgroup).  How the waves of a
// sorted list are scheduled decides its rate (DESIGN.md section 3.4, round
// 4, where the per-wave traces and the persistent forms measured against it
// are recorded):
//   * the sequencer issues the OLDEST wave of a SIMD first, so a wave that
//     starts first -- with the sort, one of the longest groups -- runs at
//     nearly the rate it would alone (1.33 us per compression beside two
//     other waves, the 4 KiB list's waves 2.9 us), and the younger waves
//     fill its gaps: hardware dispatch in the sort's order already gives the
//     longest groups the critical path;
//   * persistent waves that claim groups from a counter lose that: a wave's
//     age is its launch, not its group's, so an old wave that keeps claiming
//     groups starves a younger neighbour, whose group then ends last;
//   * what is left is the end of the launch, and most of it is set by the
//     first round: waves w, w + 1024 and w + 2048 land on one SIMD, so in
//     the sort's order the same SIMDs would start with every round's
//     longest group.  Round 1 therefore takes its groups in reverse (below):
//     SIMD work max/mean 1.07 -> 1.047, the CDC-like list 2 % faster.
template <int TILE, bool WEAK = false>
__global__ void __launch_bounds__(64 * kTableWG, kTableWavesPerSimd)
sha1_table_kernel(const uint8_t* __restrict__ data, uint64_t len, const uint64_t* __restrict__ offsets,
                  const uint32_t* __restrict__ sizes, uint64_t nblocks, uint8_t* __restrict__ digests,
                  int* __restrict__ status, uint32_t* __restrict__ weak, const uint32_t* __restrict__ order) {
  constexpr int kWaveTile = 64 * (TILE / 16) > 64 * kListPieces ? 64 * (TILE / 16) : 64 * kListPieces;
  __shared__ uint4 smem[kTableWG * kWaveTile];
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint4* tile = smem + wid * kWaveTile;
  const uint32_t ngroups = (uint32_t)((nblocks + 63) / 64);  // <= 2^25: the launcher splits at 2^31 blocks
  uint32_t g = blockIdx.x * kTableWG + wid;
  // The first rounds of waves land one per SIMD per round (wave w and
  // w + kTableRound on the same SIMD, traces of round 4), so in the sort's
  // order SIMD i would start with groups i, R + i and 2R + i: the longest
  // group of every round on the same SIMDs (first-round work per SIMD
  // 589..967 compressions, mean 764, on the CDC-like list).  Round 1 takes
  // its groups in reverse, pairing the longest of round 0 with the shortest
  // of round 1.  R is MI355X's 1024 SIMDs at compile time: a runtime R moved
  // this kernel's compiled form and cost the 4 KiB list 6 % (profiles/r04/s18/);
  // on a device with fewer SIMDs (a CPX/QPX partition) the reversal is one
  // harmless permutation of round 1 whose gain does not carry over.
  if (order) {
    const uint32_t R = kTableRound, r = g / R;
    if (r < 8 && ((kTableReversedRounds >> r) & 1u) && (r + 1) * R <= ngroups) g = r * R + (R - 1u - g % R);
  }
  if (g < ngroups) table_group<TILE, WEAK>(data, len, offsets, sizes, nblocks, digests, status, weak, order, g, tile);
}

}  // namespace sf

namespace sfi {

// Explicit block lists of more than one wave's blocks are hashed in order of
// length (sha1_table_kernel's `order`): a wave runs as long as its longest
// block, so 64 blocks of mixed sizes side by side waste most lanes -- a list
// of content-defined sizes (mean 8 KiB, up to 32 KiB) hashed at 312 GiB/s in
// list order against 1834 GiB/s sorted (scripts/ragged_probe.py).  Small
// lists too (round 6; until then only from 2^17 blocks, on the reasoning that
// with every wave resident at once the longest block sets the time either
// way): a mixed wave also runs every step in the slot path's per-lane tail
// loop, its shortest block ending the branch-free steps, one compression at a
// time; sorted, the wave holding the longest blocks runs them two at a time.
// configs[0]'s one-window list (8,415 blocks): the kernel 1.28 -> 0.69 ms,
// the sort's three kernels 19 us (profiles/r06/sort_small/).  One wave has
// nothing to reorder.  SF_TEST_TABLE_SORT=0 / 1 never / always sorts (test hook).
constexpr uint64_t kTableSortMinBlocks = 65;
static uint64_t table_sort_min() {
  const int64_t v = knob(K_TEST_TABLE_SORT);
  if (v >= 0) return v ? 1 : ~0ull;
  return kTableSortMinBlocks;
}
constexpr uint64_t kSortMaxBlocks = 1ull << 27;  // blocks per sorted piece (~1.2 GiB of workspace at most)

// Stream-ordered workspace holding the processing order of blocks [0, n) of
// a list: stable sort of the blocks by length class, descending, on `s`
// (list order within a class).  Stability matters: a wave's 64 blocks are
// then alike in length AND close together in memory; a class-bucketing by
// atomics scattered each class's blocks across the buffer and the list ran
// at half the rate (1410 vs 2609 GiB/s on one box, profiles/r03/bucket_sort_rejected/).
// The key takes the counting sort of sf_sort.hip (three kernels, ~21 us for
// 0.5 M blocks with the default 8-bit key, against ~56 us of GPU time for
// rocprim's radix sort with its key kernel; profiles/r03/sort/), the 9- and
// 10-bit keys of the SF_TABLE_CLASS_BITS knob too (512 / 1024 bins).
// Returns nullptr (unsorted launch) if anything fails.
static uint32_t* table_order(const uint32_t* d_sizes, uint64_t n, hipStream_t s, void** ws_out) {
  *ws_out = nullptr;
  // mantissa bits of the length class, 1..6 (SF_TABLE_CLASS_BITS, A/B knob)
  const uint32_t mbits = (uint32_t)std::min<int64_t>(6, std::max<int64_t>(1, knob(K_TABLE_CLASS_BITS)));

  // classes < 32 << mbits; the key is clamped at (16 << mbits) - 1, so every
  // block of 2^16+ compressions (>= 4 MiB) shares the top class: 8 bits with
  // 4 mantissa bits (the default; class width 6.25 %), 9 with 5, 10 with 6
  // (1.6 %), all one counting pass of sf_sort.hip.
  const unsigned kbits = mbits <= 4 ? 8u : 4u + mbits;
  const uint32_t kmax = (1u << kbits) - 1u;
  // one counting pass over 256 / 512 / 1024 classes (sf_sort.hip)
  ScratchLayout L;
  const size_t order_at = L.add(n * 4), sort_at = L.add(class_order_workspace(n, kmax));
  void* ws = nullptr;
  if (stream_alloc(&ws, L.total(), s) != SF_OK) {
    (void)hipGetLastError();
    return nullptr;
  }
  uint32_t* order = L.at<uint32_t>(ws, order_at);
  if (class_order(d_sizes, n, mbits, kmax, L.at<void>(ws, sort_at), order, s) != SF_OK) {
    (void)hipGetLastError();
    stream_free(ws, s);
    return nullptr;
  }
  *ws_out = ws;
  return order;
}

// sha1_table_kernel<128, weak != NULL>, one group of 64 blocks per wave;
// SF_OK or the launch error.
static int launch_table_kernel(const uint8_t* d_data, uint64_t len, const uint64_t* d_offsets,
                               const uint32_t* d_sizes, uint64_t nblocks, uint8_t* d_digests, int* d_status,
                               uint32_t* weak, const uint32_t* order, hipStream_t stream) {
  const uint64_t ngroups = (nblocks + 63) / 64;
  const unsigned grid = (unsigned)((ngroups + sf::kTableWG - 1) / sf::kTableWG);
  if (weak)
    return launch(sf::sha1_table_kernel<128, true>, dim3(grid), dim3(64 * sf::kTableWG), stream, d_data, len, d_offsets,
                  d_sizes, nblocks, d_digests, d_status, weak, order);
  return launch(sf::sha1_table_kernel<128, false>, dim3(grid), dim3(64 * sf::kTableWG), stream, d_data, len, d_offsets,
                d_sizes, nblocks, d_digests, d_status, nullptr, order);
}

int launch_table(const void* d_data, uint64_t len, const uint64_t* d_offsets, const uint32_t* d_sizes,
                 uint64_t nblocks, void* d_digests, int* d_status, hipStream_t stream, uint32_t* weak) {
  if (nblocks == 0) return SF_OK;
  const bool sorted = nblocks >= table_sort_min();
  const uint64_t maxb = sorted ? std::min(launch_max_blocks(), kSortMaxBlocks) : launch_max_blocks();
  if (nblocks > maxb) {  // consecutive pieces of the table, one launch each
    for (uint64_t first = 0; first < nblocks; first += maxb) {
      const int rc = launch_table(d_data, len, d_offsets + first, d_sizes + first, std::min(maxb, nblocks - first),
                                  static_cast<uint8_t*>(d_digests) + first * 20, d_status, stream,
                                  weak ? weak + first : nullptr);
      if (rc) return rc;
    }
    return SF_OK;
  }
  void* ws = nullptr;
  const uint32_t* order = sorted ? table_order(d_sizes, nblocks, stream, &ws) : nullptr;
  const int rc = launch_table_kernel(static_cast<const uint8_t*>(d_data), len, d_offsets, d_sizes, nblocks,
                                     static_cast<uint8_t*>(d_digests), d_status, weak, order, stream);
  stream_free(ws, stream);
  return rc;
}

}  // namespace sfi
