// sf_launch.hpp -- the launchers of the SHA-1 block kernels and the two plain
// structs their kernels take by value.  No device code: the host-compiled
// translation units (sf_batch.cpp and the pipelines) include it as the .hip
// files do.  Each launcher is defined beside its kernel.
#pragma once
#include <stdint.h>

#include "sf_internal.hpp"

namespace sf {

// K_t + W_t of the padding-only chunk ending a block of `bytes` bytes
// (bytes % 64 == 0), filled by the host (pad_schedule) and passed by value.
struct PadSchedule {
  uint32_t bytes;  // 0 = not available
  uint32_t kw[80];
};

// One per-file blocks_hash chain job (src/index.rs:661-682) of a batch of
// equal-size files: one lane per file over its run of run_len digest bytes,
// data chunks [lo, hi) (64-B units) of the run.  part 0 = the whole chain;
// part 1 = chunks [0, hi), the 5-word SHA-1 state saved to state[f]; part 2
// = resume from state[f], chunks [lo, end) + the padding chunk(s), hash to
// hashes[f].
struct ChainJob {
  const uint8_t* runs;
  uint8_t* state;
  uint8_t* hashes;
  uint32_t files, run_len, lo, hi, part, waves;  // waves = chain waves (64 files each)
};

}  // namespace sf

namespace sfi __attribute__((visibility("hidden"))) {

// Most blocks one launch takes.  HIP caps a launch at 2^32 - 1 work-items
// (gridDim.x * blockDim.x), i.e. about 2^32 blocks at one lane per block;
// larger tables -- reachable only with tiny blocks, e.g. 16-B blocks over
// 64 GiB -- are hashed as several launches over consecutive block ranges
// (blocks are independent).  A multiple of 16, so every piece of a 16-B
// aligned fixed tiling stays 16-B aligned.  SF_TEST_LAUNCH_MAX_BLOCKS lowers
// it (test hook: exercises the split at small sizes).  (sf_capi.hip)
uint64_t launch_max_blocks();

// K_t + W_t for the padding-only chunk of a `bytes`-long message (bytes a
// multiple of 64); bytes = 0 in the result if there is none.  (sf_batch.cpp)
sf::PadSchedule pad_schedule(uint32_t bytes);

// Fixed tiling (sha1_fixed_kernel, sf_capi.hip); weak: also every block's
// Adler-32.
int launch_fixed(const void* d_data, uint64_t len, uint32_t bs, uint64_t nblocks, void* d_digests,
                 hipStream_t stream, uint32_t* weak = nullptr);
// Stand-alone chains, one lane per file over its whole run (sha1_chain_kernel,
// sf_capi.hip): file f's run of run_len bytes starts at d_runs + f * run_stride.
int launch_chain_plain(const uint8_t* d_runs, uint64_t run_stride, uint32_t nfiles, uint32_t run_len,
                       uint8_t* d_hashes, hipStream_t stream);
// Explicit block list (sha1_table_kernel, sf_table.hip; sorted by length class
// from 65 blocks).  d_status may be NULL.
int launch_table(const void* d_data, uint64_t len, const uint64_t* d_offsets, const uint32_t* d_sizes,
                 uint64_t nblocks, void* d_digests, int* d_status, hipStream_t stream, uint32_t* weak = nullptr);
// The FILE_BLOCK messages of digests [0, n) of a fixed tiling
// (wire_file_blocks_kernel, sf_wire.hip): every message is 33 + digits(bs)
// bytes but the last, whose size field is `last`.
int launch_wire(const uint8_t* d_digests, uint64_t n, uint32_t bs, uint32_t last, uint8_t* d_out,
                hipStream_t stream);
// sha1_fixed_chained_kernel<128> (sf_stream.hip): `bwaves` block waves of 64
// blocks (a column range: wpp of every file's wpf waves from poff) beside
// the chain waves of j0 and j1.
int launch_chained(const uint8_t* data, uint64_t len, uint32_t bs, uint64_t nblocks, uint8_t* digests,
                   const sf::PadSchedule& pad, const sf::ChainJob& j0, const sf::ChainJob& j1, uint64_t bwaves,
                   uint32_t wpf, uint32_t wpp, uint32_t poff, hipStream_t stream);
// sha1_chain_helper_kernel (sf_chain.hip) over jobs j0 (its j0.waves chain
// waves first) and j1 on `stream`; SF_OK or the launch error.
int launch_chain_helper(const sf::ChainJob& j0, const sf::ChainJob& j1, hipStream_t stream);

}  // namespace sfi
