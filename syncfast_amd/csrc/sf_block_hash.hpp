// sf_block_hash.hpp -- how a wave hashes its 64 blocks: the device functions
// the SHA-1 block kernels share.  No kernel is defined here; each is in the
// file that launches it: sha1_fixed_kernel in sf_capi.hip,
// sha1_fixed_chained_kernel in sf_stream.hip, sha1_table_kernel in
// sf_table.hip.
//
// Replaces the hot loop of Index::index_file, the reference's src/index.rs:
// 629-647 (SHA-1 of every block; `Sha1::update` / `digest` / `reset`) and is
// reused for compute_blocks_hash (src/index.rs:661-682) of many files at once.
//
// Design (DESIGN.md "Kernels"):
//   * one LANE per block: SHA-1 is sequential inside a message, so a block is
//     a lane's private message and a wave hashes 64 blocks in lockstep;
//   * a wave's 64 blocks are streamed through a per-wave LDS tile of
//     64 blocks x TILE bytes, filled by LDS-DMA (`buffer_load_dwordx4 ... lds`):
//     every DMA wave-instruction moves TILE/16 full 16-B pieces of 1024/TILE
//     blocks, so each instruction reads whole 128-B lines; the piece order is
//     XOR-swizzled on the SOURCE address so that the per-lane `ds_read_b128`
//     of a block's own pieces is bank-conflict free;
//   * the tile for step t+1 is issued right after step t's words are in
//     registers, so one DMA per wave is always in flight behind TILE/64
//     compressions of VALU work;
//   * the final (padding) chunk(s) of each block are built with per-lane,
//     bounds-checked loads, so nothing is ever read outside [0, len).
// Buffer resources carry num_records = bytes left in the wave's span, so a
// DMA lane past the end reads zeros instead of faulting.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_launch.hpp"
#include "sha1_device.hpp"

namespace sf {

constexpr int kWave = 64;
constexpr int kWavesPerWG = 4;
constexpr int kThreads = kWave * kWavesPerWG;
constexpr uint32_t kRsrcWord3 = 0x00020000u;  // raw buffer, gfx9 family

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// ---------------------------------------------------------- wave helpers
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
// A value identical in every lane, moved to SGPRs so that everything derived
// from it (buffer resources, loop bounds) stays scalar.
__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m, 64));
  return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m, 64));
  return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    uint64_t o = __shfl_xor((unsigned long long)v, m, 64);
    v = o < v ? o : v;
  }
  return uniform_u64(v);
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    uint64_t o = __shfl_xor((unsigned long long)v, m, 64);
    v = o > v ? o : v;
  }
  return uniform_u64(v);
}

// 64 bytes at any byte address (four 16-B loads; unaligned global access).
__device__ __forceinline__ void ld_chunk_any(uint4 (&v)[4], const uint8_t* p) {
#pragma unroll
  for (int q = 0; q < 4; ++q) __builtin_memcpy(&v[q], p + 16 * q, 16);
}

// 64 bytes at a 4-B aligned address (four 16-B loads).
__device__ __forceinline__ void ld_chunk_al(uint4 (&v)[4], const uint32_t* p) {
#pragma unroll
  for (int k = 0; k < 4; ++k) __builtin_memcpy(&v[k], p + 4 * k, 16);
}

// Per-wave geometry of the blocks handled by this wave.
struct WaveGeo {
  uint64_t base;      // byte offset of the wave's span in `data`
  uint64_t span;      // bytes in [base, end of last block)
  uint32_t min_size;  // min block size over valid lanes
  uint32_t max_size;  // max block size over valid lanes
  uint32_t max_nch;   // max compressions over valid lanes
  bool lds_ok;        // 16-B aligned pieces and span < 4 GiB
};

// Cache policy of the aligned path's LDS-DMA: nt, the input is streamed once
// (+1.4 % in A/B, profiles/r01/tune_sched_nt.log).
constexpr int kLoadAux = 2;

// Issue the LDS-DMA fill of step `step` into the wave's tile: N wave-
// instructions, instruction j moving each lane's 16-B piece at voff[j] past
// the step's start (STRIDE bytes per step) with cache policy AUX.  The buffer
// resource starts at the step and covers the rest of the span, so lanes past
// the span read zeros.
template <int N, int STRIDE, int AUX>
__device__ __forceinline__ void issue_dma(const uint8_t* span_ptr, uint64_t span, uint32_t step,
                                          const uint32_t* voff, uint4* wave_tile) {
  // All operands are wave-uniform; readfirstlane keeps the resource in SGPRs
  // (a VGPR resource makes hipcc wrap every DMA in a waterfall loop).
  const uint64_t toff = (uint64_t)step * STRIDE;
  const uint64_t left = span > toff ? span - toff : 0;
  const uint32_t nrec = __builtin_amdgcn_readfirstlane(left > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)left);
  const uint64_t ptr = uniform_u64(reinterpret_cast<uint64_t>(span_ptr + toff));
  __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(ptr), (short)0, (int)nrec, (int)kRsrcWord3);
#pragma unroll
  for (int j = 0; j < N; ++j)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)(wave_tile + j * 64), 16, voff[j], 0, 0, AUX);
}

// The 16 big-endian message words of the 64 bytes in v[0..3].
__device__ __forceinline__ void be_words(uint32_t (&w)[16], const uint4* v) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    w[4 * q + 0] = bswap32(v[q].x);
    w[4 * q + 1] = bswap32(v[q].y);
    w[4 * q + 2] = bswap32(v[q].z);
    w[4 * q + 3] = bswap32(v[q].w);
  }
}

// Hash the block (off, size) owned by this lane; all 64 lanes of the wave
// enter together.  `rel` = off - geo.base (valid lanes).  TILE = bytes of
// each block staged per LDS step.  WEAK: also fold the same words into the
// lane's Adler-32 (opt-in weak sum, sha1_device.hpp).
template <int TILE, bool HAS_PAD, bool WEAK = false>
__device__ __forceinline__ void hash_wave(const uint8_t* __restrict__ data, uint64_t off, uint32_t size,
                                          uint32_t rel, bool valid, const WaveGeo& geo,
                                          uint4* __restrict__ wave_tile, Sha1& st, const PadSchedule pad,
                                          Adler& wk) {
  constexpr int PIECES = TILE / 16;           // 16-B pieces per block per step
  constexpr int CH = TILE / 64;               // compressions per step
  constexpr int GSHIFT = PIECES == 4 ? 2 : (PIECES == 8 ? 1 : 0);
  constexpr int BLK_PER_DMA = 1024 / TILE;    // blocks covered by one DMA wave-instruction
  static_assert(PIECES == 4 || PIECES == 8 || PIECES == 16, "TILE must be 64, 128 or 256");
  const int lane = lane_id();

  st.init();
  if constexpr (WEAK) wk.init();
  const uint32_t nfull = geo.min_size / 64u;
  uint32_t c_done = 0;  // this lane's chunks done
  if (geo.lds_ok) {
    const uint32_t nsteps = nfull / CH;
    // Source offsets (relative to the span base) of this lane's 16-B piece in
    // each of the PIECES DMA instructions of one step.  Instruction j writes
    // LDS bytes [j*1024, j*1024+1024): lane -> block b, slot s; slot s holds
    // piece k = s ^ g(b) so that the reads below are conflict free.
    uint32_t voff[PIECES];
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const int b = j * BLK_PER_DMA + lane / PIECES;
      const int s = lane % PIECES;
      const int k = s ^ ((b >> GSHIFT) & (PIECES - 1));
      const uint32_t rel_b = (uint32_t)__shfl((int)rel, b, 64);
      voff[j] = rel_b + (uint32_t)k * 16u;
    }
    const int g = (lane >> GSHIFT) & (PIECES - 1);
    const uint4* my = wave_tile + lane * PIECES;
    const uint8_t* span_ptr = data + geo.base;

    if (nsteps > 0) issue_dma<PIECES, TILE, kLoadAux>(span_ptr, geo.span, 0, voff, wave_tile);
    for (uint32_t t = 0; t < nsteps; ++t) {
      uint4 raw[PIECES];
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int k = 0; k < PIECES; ++k) raw[k] = my[k ^ g];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (t + 1 < nsteps) issue_dma<PIECES, TILE, kLoadAux>(span_ptr, geo.span, t + 1, voff, wave_tile);
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) {
        uint32_t w[16];
        be_words(w, raw + ch * 4);
        if constexpr (WEAK) {
          uint32_t le[16];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const uint4 v = raw[ch * 4 + q];
            le[4 * q + 0] = v.x;
            le[4 * q + 1] = v.y;
            le[4 * q + 2] = v.z;
            le[4 * q + 3] = v.w;
          }
          wk.chunk(le);
        }
        st.compress(w);
      }
    }
    c_done = nsteps * CH;
  } else {
    if constexpr (HAS_PAD) {
      // (fixed tiling, only for a misaligned data pointer or block size: the
      // hot kernel's code -- any change here moves its register assignment,
      // and one such move cost the headline launch 3.7 %)
      // Misaligned or > 4 GiB span: each lane streams its own block, 64 B per
      // compression with four (unaligned) 16-B loads, the next chunk's loads
      // in flight while the current one is compressed.
      const uint8_t* p = data + off;
      uint4 nx[4];
      if (nfull) ld_chunk_any(nx, p);
      for (uint32_t c = 0; c < nfull; ++c) {
        uint32_t le[16], w[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          le[4 * q + 0] = nx[q].x;
          le[4 * q + 1] = nx[q].y;
          le[4 * q + 2] = nx[q].z;
          le[4 * q + 3] = nx[q].w;
        }
        if (c + 1 < nfull) ld_chunk_any(nx, p + (uint64_t)(c + 1) * 64);
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = bswap32(le[j]);
        if constexpr (WEAK) wk.chunk(le);
        st.compress(w);
      }
      c_done = nfull;
    } else {
      // Misaligned or > 4 GiB span: each lane streams its own block, 64 B per
      // compression, the next chunk's loads in flight while the current one is
      // compressed, up to ITS OWN last whole chunk (lanes whose block has fewer
      // whole chunks than the wave's longest idle meanwhile).  Loads are
      // dword-aligned (a byte-aligned 16-B load costs the address unit several
      // times over: 4 KiB blocks at byte offset +1 ran at 1911 GiB/s, at +4 at
      // 2832, scripts/ragged_probe.py): the lane reads 17 dwords from its block
      // start rounded down to 4 B and shifts the message words out of them
      // (v_alignbyte by the lane's byte offset r).  Every dword read holds at
      // least one byte of the block, so nothing is touched outside the dwords
      // the block's bytes lie in.
      const uint8_t* p = data + off;
      const uint32_t r = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
      const uint32_t* q = reinterpret_cast<const uint32_t*>(p - r);
      const uint32_t mine = valid ? size / 64u : 0u;  // this lane's whole chunks
      const uint32_t upto = geo.max_size / 64u;       // the wave's most
      uint4 nx[4];
      uint32_t nx16 = 0u;  // dword 16 of the chunk in nx (needed when r != 0)
      if (mine) {
        ld_chunk_al(nx, q);
        if (r != 0u || mine > 1) nx16 = q[16];
      }
      for (uint32_t c = 0; c < upto; ++c) {
        if (c < mine) {
          uint32_t d[17], le[16], w[16];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            d[4 * k + 0] = nx[k].x;
            d[4 * k + 1] = nx[k].y;
            d[4 * k + 2] = nx[k].z;
            d[4 * k + 3] = nx[k].w;
          }
          d[16] = nx16;
          if (c + 1 < mine) {
            ld_chunk_al(nx, q + 16 * (uint64_t)(c + 1));
            if (r != 0u || c + 2 < mine) nx16 = q[16 * (uint64_t)(c + 2)];
          }
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            le[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], r);
            w[j] = bswap32(le[j]);
          }
          if constexpr (WEAK) wk.chunk(le);
          st.compress(w);
        }
      }
      c_done = mine;
    }
  }
  // Weak sum of this lane's bytes past the chunks both paths consumed
  // (whole chunks, then < 64 single bytes); never reads outside the block.
  if constexpr (WEAK) {
    if (valid) {
      const uint8_t* p = data + off;
      const uint32_t full = size / 64u;
      for (uint32_t c = c_done; c < full; ++c) {
        uint32_t le[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) le[j] = ld_u32_any(p + (uint64_t)c * 64 + 4 * j);
        wk.chunk(le);
      }
      for (uint32_t i = full * 64u; i < size; ++i) wk.byte(p[i]);
    }
  }
  // Every block of the wave has the same 64-B multiple size and all its data
  // chunks are done: the last chunk is the same padding for every lane.
  // (pad is passed by value, never by address: a kernel argument whose
  // address escapes is copied to scratch.)
  if (HAS_PAD && pad.bytes == geo.min_size && geo.min_size == geo.max_size && c_done == nfull) {
    st.compress_uniform(pad.kw);
    return;
  }
  // Remaining data chunks and the padding chunk(s), per lane.
  if constexpr (HAS_PAD) {
    const uint32_t nch = n_chunks(size);
    for (uint32_t c = c_done; c < geo.max_nch; ++c) {
      if (valid && c < nch) {
        uint32_t w[16];
        build_tail_chunk(w, data + off, size, c, nch);
        st.compress(w);
      }
    }
  } else {
    // An explicit list's block may be any uint32 size: the index of its last
    // chunk, (size + 8) / 64, without the 32-bit wrap of n_chunks from
    // 2^32 - 8.
    const uint32_t last = (size >> 6) + ((size & 63u) >= 56u ? 1u : 0u);
    for (uint32_t c = c_done; c < geo.max_nch; ++c) {
      if (valid && c <= last) {
        uint32_t w[16];
        build_tail_chunk(w, data + off, size, c, last + 1u);
        st.compress(w);
      }
    }
  }
}

// Fixed tiling: block i = data[i*bs, min((i+1)*bs, len)).  One workgroup
// `group` of it (4 waves x 64 consecutive blocks): the body of
// sha1_fixed_kernel and of the block part of sha1_fixed_chained_kernel.
template <int TILE, bool WEAK>
__device__ __forceinline__ void fixed_wave(const uint8_t* __restrict__ data, uint64_t len, uint32_t bs,
                                           uint64_t nblocks, uint8_t* __restrict__ digests, const PadSchedule pad,
                                           uint32_t* __restrict__ weak, uint64_t wave, uint4* __restrict__ tile) {
  const int lane = lane_id();
  const uint64_t first = wave * 64;  // this wave's 64 consecutive blocks
  if (first >= nblocks) return;
  const uint64_t blk = first + lane;
  const bool valid = blk < nblocks;
  const uint64_t off = valid ? blk * bs : first * bs;
  const uint32_t size = valid ? (uint32_t)(len - off < bs ? len - off : bs) : 0u;

  WaveGeo geo;
  geo.base = first * bs;
  const uint64_t last = (first + 64 <= nblocks) ? first + 63 : nblocks - 1;
  geo.span = len - geo.base < (last - first + 1) * (uint64_t)bs ? len - geo.base : (last - first + 1) * (uint64_t)bs;
  const uint32_t last_size = (uint32_t)(len - last * bs < bs ? len - last * bs : bs);
  geo.min_size = last_size < bs ? last_size : bs;
  geo.max_size = bs;
  geo.max_nch = n_chunks(bs);
  geo.lds_ok = ((bs & 15u) == 0) && ((reinterpret_cast<uintptr_t>(data) & 15u) == 0) &&
               (64ull * bs < 0xF0000000ull);
  const uint32_t rel = (uint32_t)((uint64_t)lane * bs);

  Sha1 st;
  Adler wk;
  hash_wave<TILE, true, WEAK>(data, off, size, rel, valid, geo, tile, st, pad, wk);
  if (valid) {
    st.store(digests + blk * 20);
    if constexpr (WEAK) weak[blk] = wk.fin();
  }
}

}  // namespace sf
