// sf_stream.hip -- config 3 as a stream of batches:
// sha1_fixed_chained_kernel, one launch per batch hashing its blocks with
// the blocks_hash chains of earlier batches in its first workgroups.
//
// Its own translation unit: how its block part is compiled decides its rate
// (one compiled form of the same source ran 3 % slower than the plain kernel,
// another at its rate).  Its code object holds this kernel alone; what can
// still move it is a change to the wave functions of sf_block_hash.hpp, which
// it shares with the other block kernels.  The measured form's machine code is
// recorded in profiles/r03/c3/chained_kernel.json.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_block_hash.hpp"
#include "sf_device.hpp"

namespace sf {

constexpr int kChainPrio = 3;  // wave priority of the stream's chain waves
// A stream's chain job on the chain wave of a block launch (wave 0 of one
// of the first workgroups, sha1_fixed_chained_kernel).  Its digest loads are
// staged through the workgroup's LDS tile (unused by a chain wave
// otherwise), as the block waves stage theirs: per step, 8 DMA
// wave-instructions each move whole 128-B lines of 8 files, so one
// instruction touches 8 lines instead of the 64 that a lane-per-file load
// touches.  The lane-per-file loads (4 chunks in flight per lane) cost the
// launch 0.050 ms per batch of chains, the staged form 0.032 (config 3
// launch sequence, profiles/r03/c3/seq/seq_chain_lds.txt).  Data chunks
// [lo, hi) of each lane's run; part 0/2 then the padding chunk(s).
__device__ __forceinline__ void chain_job(const ChainJob& j, uint32_t wave, uint4* __restrict__ tile) {
  __builtin_amdgcn_s_setprio(kChainPrio);  // latency-bound chains issue first on a shared SIMD
  const int lane = lane_id();
  const uint32_t f = wave * 64 + lane;
  const bool valid = f < j.files;
  Sha1 st;
  if (j.part == 2 && valid) {
    const uint32_t* sv = reinterpret_cast<const uint32_t*>(j.state + (uint64_t)f * 20);
    st.h0 = sv[0]; st.h1 = sv[1]; st.h2 = sv[2]; st.h3 = sv[3]; st.h4 = sv[4];
  } else {
    st.init();
  }
  const uint32_t n = j.hi - j.lo;                 // data chunks, uniform
  const uint32_t nsteps = (n + 1) / 2;
  const uint8_t* span_ptr = j.runs + (uint64_t)wave * 64 * j.run_len + (uint64_t)j.lo * 64;
  const uint64_t files_here = j.files - wave * 64 < 64 ? j.files - wave * 64 : 64;
  const uint64_t span = (files_here - 1) * j.run_len + (uint64_t)n * 64;
  uint32_t voff[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int b = q * 8 + lane / 8;  // file of the wave
    const int s = lane % 8;
    const int k = s ^ ((b >> 1) & 7);
    voff[q] = (uint32_t)b * j.run_len + (uint32_t)k * 16u;
  }
  const int g = (lane >> 1) & 7;
  const uint4* my = tile + lane * 8;
  if (nsteps > 0) issue_dma<8, 128, kLoadAux>(span_ptr, span, 0, voff, tile);
  for (uint32_t t = 0; t < nsteps; ++t) {
    uint4 raw[8];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int k = 0; k < 8; ++k) raw[k] = my[k ^ g];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (t + 1 < nsteps) issue_dma<8, 128, kLoadAux>(span_ptr, span, t + 1, voff, tile);
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      if (2 * t + ch < n) {
        uint32_t w[16];
        be_words(w, raw + 4 * ch);
        st.compress(w);
      }
    }
  }
  if (!valid) return;
  const uint8_t* p = j.runs + (uint64_t)f * j.run_len;
  if (j.part == 1) {
    uint32_t* sv = reinterpret_cast<uint32_t*>(j.state + (uint64_t)f * 20);
    sv[0] = st.h0; sv[1] = st.h1; sv[2] = st.h2; sv[3] = st.h3; sv[4] = st.h4;
    return;
  }
  const uint32_t nch = n_chunks(j.run_len);
  for (uint32_t c = j.run_len / 64; c < nch; ++c) {
    uint32_t w[16];
    build_tail_chunk(w, p, j.run_len, c, nch);
    st.compress(w);
  }
  st.store(j.hashes + (uint64_t)f * 20);
}

// Equal-size many-file batches as a stream (BASELINE configs[2], batch after
// batch): ONE launch hashes every block of batch i (fixed_wave) and, in its
// first workgroups, up to two chain jobs of earlier batches (j0 then j1):
// with split chains, the second half of batch i-2's and the first half of
// batch i-1's.  Their digest tables and saved states were completed by
// earlier launches on the same stream, so no workgroup of this launch waits
// on another.  Halving each chain halves the latency it needs to hide: a
// chain lane beside the block waves runs ~3x slower than alone.
template <int TILE>
__global__ void __launch_bounds__(kThreads, 1)
sha1_fixed_chained_kernel(const uint8_t* __restrict__ data, uint64_t len, uint32_t bs, uint64_t nblocks,
                          uint8_t* __restrict__ digests, const PadSchedule pad, const ChainJob j0,
                          const ChainJob j1, const uint32_t wpf, const uint32_t wpp, const uint32_t poff) {
  // Chain waves are spread one per workgroup: workgroup g < C runs chain
  // wave g as its wave 0 (job 0's waves first) and block waves 3g..3g+2 as
  // its waves 1-3; the other workgroups run 4 block waves each.  So no CU
  // hosts more than one chain wave per workgroup, and the chains' scattered
  // digest loads are spread over C CUs instead of C/4.
  __shared__ uint4 smem[kWavesPerWG * 64 * (TILE / 16)];
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t C = j0.waves + j1.waves;  // chain waves
  const uint32_t g = blockIdx.x;
  uint64_t bw;
  if (g < C) {
    if (wid == 0) {
      if (g < j0.waves) chain_job(j0, g, smem);
      else chain_job(j1, g - j0.waves, smem);
      return;
    }
    bw = (uint64_t)g * 3 + (wid - 1);
  } else {
    bw = (uint64_t)C * 3 + (uint64_t)(g - C) * kWavesPerWG + wid;
  }
  // A column-range launch (wpp < wpf: every file's block waves [poff,
  // poff + wpp) of its wpf) maps its wave bw to the file's wave.
  if (wpp != wpf) bw = (uint64_t)((uint32_t)bw / wpp) * wpf + poff + (uint32_t)bw % wpp;
  fixed_wave<TILE, false>(data, len, bs, nblocks, digests, pad, nullptr, bw, smem + wid * 64 * (TILE / 16));
}

}  // namespace sf

namespace sfi {

int launch_chained(const uint8_t* data, uint64_t len, uint32_t bs, uint64_t nblocks, uint8_t* digests,
                   const sf::PadSchedule& pad, const sf::ChainJob& j0, const sf::ChainJob& j1, uint64_t bwaves,
                   uint32_t wpf, uint32_t wpp, uint32_t poff, hipStream_t stream) {
  // grid: C mixed workgroups (1 chain wave + 3 block waves), then 4 block
  // waves per workgroup for the rest
  const uint64_t C = j0.waves + j1.waves;
  const uint64_t rest = bwaves > 3 * C ? bwaves - 3 * C : 0;
  const unsigned grid = (unsigned)(C + ceil_div(rest, sf::kWavesPerWG));
  if (grid == 0) return SF_OK;
  return launch(sf::sha1_fixed_chained_kernel<128>, dim3(grid), dim3(sf::kThreads), stream, data, len, bs, nblocks,
                digests, pad, j0, j1, wpf, wpp, poff);
}

}  // namespace sfi
