// sf_internal.hpp -- library-internal declarations shared by the C-ABI's
// translation units (not part of include/syncfast_amd.h).  The .hip files are
// compiled for the GPU, each into a code object of its own; the SHA-1 block
// kernels share the wave functions of sf_block_hash.hpp and are launched
// through sf_launch.hpp:
//   sf_capi.hip   sha1_fixed_kernel (the headline), the stand-alone chain
//                 kernel, the splitmix fill and the simple device-resident
//                 entry points;
//   sf_stream.hip sha1_fixed_chained_kernel: a batch's blocks beside the
//                 blocks_hash chains of earlier batches;
//   sf_chain.hip  sha1_chain_helper_kernel: chains alone, with helper waves;
//   sf_table.hip  sha1_table_kernel: explicit block lists, and how a list is
//                 launched;
//   sf_sort.hip   the counting sort that orders a list by length class;
//   sf_wire.hip   FILE_BLOCK runs written on the device;
//   sf_match.hip  digest lookup; sf_litmus.hip  a memory-model probe;
//   sf_batch.cpp  the device-resident batch entry points (host planning over
//                 the launchers);
//   sf_host.cpp   the host-memory indexing entry points: per-device cache of
//                 streams and staging buffers, the buffer / file / fd / range
//                 pipelines, stamp and host SHA-1 helpers;
//   sf_host_out.cpp  the device-to-descriptor writers: FILE_BLOCK runs,
//                 device bytes and BLOCK_DATA runs streamed to an fd; and the
//                 descriptor-to-device loader of the local files;
//   sf_pagelock.cpp  the registry of host ranges page-locked by the in-place
//                 routes (the region rule itself is sf_inplace.hpp: host
//                 arithmetic, executed by tests/native/inplace_regions.cpp);
//   sf_files.cpp  sf_index_files, the many-file pipeline;
//   sf_fds.cpp    sf_index_fds_blocks, the default mode over many files;
//   sf_multi.cpp  one process, N devices;
//   sf_stage.cpp  what those pipelines share (sf_stage.hpp: the stage driver);
//   sf_pool.cpp   the host worker threads of every pipeline (run_pool);
//   sf_zpaq.cpp   the reference's ZPAQ chunker on the host;
//   sf_cdc.hip    the same boundaries cut on the device (its own kernels);
//   sf_cdc_files.hip  the same for many files of one buffer in one call (its
//                 own kernels; the lane code is sf_cdc_lane.hpp, shared with
//                 sf_cdc.hip; the geometry is sf_cdc_files_plan.hpp);
//   sf_recv.hip   FILE_BLOCK runs parsed on the device (its own kernels; the
//                 host parser is sf_wire_parse.hpp);
//   sf_recv_data.hip  BLOCK_DATA runs parsed and their payloads verified on
//                 the device (its own kernels; the rules are sf_wire_data.hpp;
//                 what the three parsers share is sf_recv_scan.hpp).
//   sf_recv_files.hip  a whole GetFiles stream -- many files' FILE_START,
//                 FILE_BLOCK and FILE_END in one buffer -- parsed, offset and
//                 looked up in one call (its own kernels; the rules are
//                 sf_wire_files.hpp; the scan is sf_recv_scan.hpp's).
//   sf_copy.hip   the block copy kernel that assembles the incoming files in
//                 HBM (its own kernels; the arithmetic is sf_copy_plan.hpp).
//   sf_send.hip   BLOCK_DATA runs built on the device, and a GET_BLOCK run
//                 answered in one call (its own kernels; the rules are
//                 sf_wire_data.hpp; the payloads go through sf_copy.hip).
//   sf_send_files.hip  the source's answer to a list of GET_FILE requests --
//                 every file's FILE_START, FILE_BLOCKs and FILE_END -- built
//                 in one call (its own kernels; the rules are
//                 sf_wire_send_files.hpp; the block scan is sf_wire.hip's).
//   sf_want.hip   the destination's GET_BLOCK run built from its missing rows,
//                 and a parsed BLOCK_DATA run joined against them into a copy
//                 list (its own kernels; the rules are sf_want_plan.hpp; the
//                 lookups are sf_match.hip's).
//   sf_names.hip  the destination's lookup of files by name: the name set
//                 (its own kernels; the name hash is sf_wire_entries.hpp's).
//   sf_send_entries.hip  the files list (FILE_ENTRY, END_FILES) and the
//                 GET_FILE requests built in one call each (its own kernels;
//                 the rules are sf_wire_entries.hpp).
//   sf_recv_entries.hip  a received files list parsed, looked up in a name
//                 set and compared in one call (its own kernels; the rules are
//                 sf_wire_entries.hpp; the scan is sf_recv_scan.hpp's).
//   sf_serve_files.hip  a received run of GET_FILE requests parsed, and
//                 answered from the index's own block table in one call (its
//                 own kernels; the rules are sf_wire_get_files.hpp; the newline
//                 bitmap is sf_recv_scan.hpp's, the lookup sf_names.hip's, the
//                 block scan sf_wire.hip's).
//   sf_plan_copies.hip  the received blocks the destination already holds
//                 turned into a copy list and the rows' present flags in one
//                 call, each local block hashed before it is used (its own
//                 kernels; the rules are sf_plan_copies.hpp; the hashing is
//                 sf_table.hip's).
// Every .hip file launches its kernels and runs its rocprim scans through
// sf_device.hpp (launch, grid256, scan_inclusive, scan_exclusive), and divides
// its scratch with sf_layout.hpp (ScratchLayout, for_pieces: host arithmetic,
// executed by tests/native/layout.cpp).
// The .cpp files use only the HIP runtime API (no kernels), so they build
// with the host compiler.
#pragma once
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <sys/types.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <mutex>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/syncfast_amd.h"
#include "sf_layout.hpp"
#include "sf_stage.hpp"

// Internal status of the in-place route (never returned through the C-ABI):
// the caller's pages could not be page-locked, take the staged route.
#define SF_ENOTSUP (-95)

#define SF_HIP(call)                       \
  do {                                     \
    hipError_t _e = (call);                \
    if (_e != hipSuccess) return sfi::hip_err(_e); \
  } while (0)

// The opaque handle of include/syncfast_amd.h: a BLOCK_DATA run built in HBM
// (sf_send.hip builds and frees it, sf_host_out.cpp streams it to a descriptor).
// bytes: stream-ordered scratch of `device` (NULL for an empty run, which
// needs no device); done: recorded on the building stream behind the last
// kernel that writes the run (NULL for an empty run).
struct sf_wire_run {
  uint8_t* bytes;
  uint64_t n_bytes, n_messages;
  int device;
  hipEvent_t done;
};

namespace sfi __attribute__((visibility("hidden"))) {

// Environment knobs, read once when the library is loaded (sf_knobs.cpp);
// the launch and copy paths read these slots, never the environment.
// Order = kKnobDefs[] (names, defaults).
enum Knob {
  K_IO_THREADS, K_INPLACE_MIN_MIB, K_INPLACE_SERIAL, K_FADVISE, K_NO_HOSTREG, K_TABLE_CLASS_BITS, K_TRACE,
  K_BATCH_FUSED,
  K_TEST_INPLACE_FAIL_AT, K_TEST_WIRE_CHUNK, K_TEST_STREAM_STAGE_MIB, K_TEST_LAUNCH_MAX_BLOCKS, K_TEST_TABLE_SORT,
  K_TEST_MULTI_SELF_GATHER, K_TEST_CUT_WINDOW_MIB, K_TEST_STREAM_POOL, K_TEST_ZPAQ_WINDOW, K_TEST_WIRE_PARSE_HOST,
  K_TEST_BLOCK_DATA_WALK, K_TEST_NAME_HASH_MASK,
  K_COUNT
};
struct KnobDef {
  const char* env;
  int64_t dflt;
};
extern const KnobDef kKnobDefs[K_COUNT];
extern std::atomic<int64_t> g_knob[K_COUNT];
inline int64_t knob(Knob k) { return g_knob[k].load(std::memory_order_relaxed); }

// Counters of the routes the host entry points took (read by the tests
// through sf_test_get_stat): pages the library page-locked, and ranges it
// refused to page-lock because they are not private anonymous memory.
enum Stat { S_PAGES_LOCKED, S_NOT_ANON_REFUSED, S_COUNT };
extern std::atomic<int64_t> g_stat[S_COUNT];
inline void stat_add(Stat s, int64_t v = 1) { g_stat[s].fetch_add(v, std::memory_order_relaxed); }

// Test hook (sf_test_set_read_hook, sf_knobs.cpp): the pread routes call it
// after each window of a regular file has been read.
void read_hook(uint64_t window);

// A C++ exception must not cross the extern "C" boundary: a C or Rust caller
// would get std::terminate.  Every entry point that allocates, starts threads
// or takes locks on the host runs its body through guarded(): host allocation
// failure -> SF_ENOMEM, a thread or lock the system refuses (EAGAIN and the
// like) -> SF_ENOMEM, anything else -> SF_EIO.
template <typename F>
inline int guarded(F&& body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return SF_ENOMEM;
  } catch (const std::system_error&) {
    return SF_ENOMEM;
  } catch (...) {
    return SF_EIO;
  }
}

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline int hip_err(hipError_t e) {
  if (e == hipSuccess) return SF_OK;
  if (e == hipErrorOutOfMemory) return SF_ENOMEM;
  return SF_ENODEV;
}

inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// Whether an output pointer breaks the alignment include/syncfast_amd.h states
// for it (a power of two: the widest store a kernel makes to it -- digests and
// hashes are five dword stores, Sha1::store).  NULL is aligned.  The entry
// points refuse such a pointer with SF_EINVAL before any device call.
inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// A fixed tiling's block size: 1 .. SF_MAX_BLOCK_SIZE.
inline int check_block_size(uint32_t bs) { return bs == 0 || bs > SF_MAX_BLOCK_SIZE ? SF_EINVAL : SF_OK; }

// Stream-ordered scratch (sf_alloc.cpp): allocated, used and freed on one
// stream, from the library's pool of the stream's device, whose blocks are
// reused on the freeing stream only.  stream_alloc returns an SF_ code.
int stream_alloc(void** p, size_t bytes, hipStream_t s);
void stream_free(void* p, hipStream_t s);
// Such scratch, given back on every path out of a call.
struct Scratch {
  void* p = nullptr;
  hipStream_t s;
  explicit Scratch(hipStream_t s_) : s(s_) {}
  ~Scratch() { stream_free(p, s); }
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
};

// The life of a run (sf_send.hip), for the entry points that build one:
// the empty run (no device, no bytes, no event); a run of n_bytes /
// n_messages on the current device, its bytes allocated on s and its event
// created (*run stays NULL on failure); and the end of the build, rc being
// what the build returned so far: the event is recorded on s and *out = run,
// or on any error the run (which may be NULL) is given back and the error
// returned.
sf_wire_run* wire_run_empty();
int wire_run_begin(uint64_t n_bytes, uint64_t n_messages, hipStream_t s, sf_wire_run** run);
int wire_run_finish(sf_wire_run* run, int rc, hipStream_t s, sf_wire_run** out);

// The four numbers an entry point keeps of its last call for its
// sf_test_*_stats reader.
struct Stats4 {
  std::atomic<uint64_t> v[4];
  void reset() {
    for (auto& x : v) x.store(0, std::memory_order_relaxed);
  }
  void set(int k, uint64_t x) { v[k].store(x, std::memory_order_relaxed); }
  int read(uint64_t out[4]) const {
    if (!out) return SF_EINVAL;
    for (int k = 0; k < 4; k++) out[k] = v[k].load(std::memory_order_relaxed);
    return SF_OK;
  }
};
// FILE_BLOCK runs of explicit lists (sf_wire.hip): end offsets of every
// message (stream-ordered allocation, hipFreeAsync on s), the end offset of
// every chunk of `per` messages, and messages [first, first + cnt) written
// from the start of d_out (base = end offset of message first - 1).
int wire_plan(const uint32_t* d_sizes, uint64_t n, uint64_t** d_ends, hipStream_t s);
int wire_chunk_ends(const uint64_t* d_ends, uint64_t n, uint64_t per, uint64_t* d_chunk_ends, hipStream_t s);
int wire_build(const uint8_t* d_digests, const uint32_t* d_sizes, const uint64_t* d_ends, uint64_t first,
               uint64_t cnt, uint64_t base, uint8_t* d_out, hipStream_t s);

// The block copy (sf_copy.hip): what sf_copy_blocks_device does, for the
// library's own callers (sf_send.hip writes a run's payloads with it).
int copy_blocks(const uint8_t* d_src, uint64_t src_len, uint8_t* d_dst, uint64_t dst_len, const uint64_t* d_src_off,
                const uint64_t* d_dst_off, const uint32_t* d_sizes, const uint8_t* d_take, uint64_t n, int* d_status,
                hipStream_t s);

// Per-device resources of the host-memory entry points (streams, events,
// device stage buffers, digest table, pinned stages), kept between calls:
// setting them up cost ~8 ms per call (hipMalloc / hipHostMalloc of the
// stages), ten times the PCIe time of a 64 MiB file.  One call at a time uses
// a device's set; a concurrent call gets a private set.  Capacities only
// grow, up to kCacheMax per buffer; a larger buffer is allocated for the call
// alone.  sf_release_host_cache() frees the sets.  They are never freed from
// a static destructor: the HIP runtime may already be gone at exit.
constexpr uint64_t kCacheMax = 512ull << 20;
constexpr int kMaxDevices = 64;

struct HostRes {
  hipStream_t s[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  // Slots (device and pinned alike): enum Slot in sf_stage.hpp names them; 7 = unused.
  static constexpr int kSlots = 8;
  void* dev[kSlots] = {};
  uint64_t dev_cap[kSlots] = {};
  void* pin[kSlots] = {};
  uint64_t pin_cap[kSlots] = {};
  void free_all() {
    for (int i = 0; i < kSlots; i++) {
      if (dev[i]) (void)hipFree(dev[i]);
      if (pin[i]) (void)hipHostFree(pin[i]);
      dev[i] = pin[i] = nullptr;
      dev_cap[i] = pin_cap[i] = 0;
    }
    for (int i = 0; i < 2; i++) {
      if (s[i]) (void)hipStreamDestroy(s[i]);
      if (ev[i]) (void)hipEventDestroy(ev[i]);
      s[i] = nullptr;
      ev[i] = nullptr;
    }
  }
};

// Defined in sf_host.cpp.
extern std::mutex g_res_mu[kMaxDevices];
extern HostRes* g_res[kMaxDevices];

class HostLease {
 public:
  HostLease() {
    int d = 0;
    if (hipGetDevice(&d) == hipSuccess && d >= 0 && d < kMaxDevices) {
      lk_ = std::unique_lock<std::mutex>(g_res_mu[d], std::try_to_lock);
      if (lk_.owns_lock()) {
        if (!g_res[d]) g_res[d] = new HostRes;
        r_ = g_res[d];
        return;
      }
    } else {
      (void)hipGetLastError();
    }
    own_ = new HostRes;
    r_ = own_;
  }
  ~HostLease() {
    for (int i = 0; i < 2; i++)  // an early error return may leave copies in flight
      if (r_->s[i]) (void)hipStreamSynchronize(r_->s[i]);
    for (void* p : tmp_dev_) (void)hipFree(p);
    for (void* p : tmp_pin_) (void)hipHostFree(p);
    if (own_) {
      own_->free_all();
      delete own_;
    }
  }
  HostLease(const HostLease&) = delete;
  HostLease& operator=(const HostLease&) = delete;
  int streams(hipStream_t*& s, hipEvent_t*& ev) {
    for (int i = 0; i < 2; i++) {
      if (!r_->s[i]) SF_HIP(hipStreamCreateWithFlags(&r_->s[i], hipStreamNonBlocking));
      if (!r_->ev[i]) SF_HIP(hipEventCreateWithFlags(&r_->ev[i], hipEventDisableTiming));
    }
    s = r_->s;
    ev = r_->ev;
    return SF_OK;
  }
  int dev(int i, uint64_t need, void** out) { return get(r_->dev[i], r_->dev_cap[i], need, false, out); }
  int pin(int i, uint64_t need, void** out) { return get(r_->pin[i], r_->pin_cap[i], need, true, out); }

 private:
  int get(void*& slot, uint64_t& cap, uint64_t need, bool pinned, void** out) {
    need = std::max<uint64_t>(need, 1);
    if (need <= cap) {
      *out = slot;
      return SF_OK;
    }
    // Cached buffers grow in steps (powers of two to 16 MiB, then 16 MiB
    // multiples): a stage of packed small files (just under 256 MiB) and then
    // a stage of 8 MiB files (exactly 256 MiB) share one allocation instead of
    // paying a free + reallocation of every stage buffer (~0.13 ms per MiB,
    // pinned and device: scripts/files_trace.py, scripts/pin_alloc_probe.py).
    if (need <= kCacheMax) {
      uint64_t r = need <= (16ull << 20) ? 4096 : need;
      if (need <= (16ull << 20))
        while (r < need) r <<= 1;
      else
        r = (need + (16ull << 20) - 1) & ~((16ull << 20) - 1);
      need = std::min(r, kCacheMax);
    }
    void* p = nullptr;
    if (pinned) SF_HIP(hipHostMalloc(&p, need, hipHostMallocDefault));
    else SF_HIP(hipMalloc(&p, need));
    if (need > kCacheMax) {
      (pinned ? tmp_pin_ : tmp_dev_).push_back(p);
    } else {
      if (slot) (void)(pinned ? hipHostFree(slot) : hipFree(slot));
      slot = p;
      cap = need;
    }
    *out = p;
    return SF_OK;
  }
  std::unique_lock<std::mutex> lk_;
  HostRes* r_ = nullptr;
  HostRes* own_ = nullptr;
  std::vector<void*> tmp_dev_, tmp_pin_;
};

// Fixed tiling of bytes [base, base + len) of the regular file open on fd
// (base a multiple of bs) through the staged pread pipeline (sf_host.cpp) on
// the calling thread's current device: rows (file offsets) into out[0, ...),
// blocks_hash (may be NULL) over this range's digests.  A short read is SF_EIO.
int index_file_pread(int fd, uint64_t base, uint64_t len, uint32_t bs, sf_block_sig* out, uint8_t* blocks_hash);

// Reader threads of the pread routes (sf_index_file, sf_index_files).
// SF_IO_THREADS overrides the default of 16 (A/B knob, latched at load).  With the stat phase
// parallel too, 16 readers beat 8 on many small files (10,537 files of
// 0-200 KiB: 29.3 vs 24.1 GB/s, 12 and 24 no better; 8 MiB files flat at
// 33-34 GB/s; profiles/r02/e2e/io_threads_8_12_16_24.log).
inline unsigned io_threads() {
  const int64_t v = knob(K_IO_THREADS);
  return v > 0 ? (unsigned)std::min<int64_t>(v, 64) : 16u;
}

// Processing order of an explicit block list (sf_sort.hip): d_order[0, n)
// receives the block indices sorted by length class (kmax < 1024: one
// counting pass over 256, 512 or 1024 bins), descending, list order within a
// class.  d_ws: class_order_workspace(n, kmax) bytes of device memory.
// Stream-ordered on s.
size_t class_order_workspace(uint64_t n, uint32_t kmax);
int class_order(const uint32_t* d_sizes, uint64_t n, uint32_t mbits, uint32_t kmax, void* d_ws, uint32_t* d_order,
                hipStream_t s);

// The device ZPAQ cutter (sf_cdc.hip): a plan is the cut of one buffer up to
// its block count (blocking: a synchronisation per join round and one for the
// count), zpaq_cut_emit writes its `total` rows (asynchronous), zpaq_cut_free
// gives its stream-ordered scratch back.  zpaq_segment_len: the segment
// length, a function of max_size only.
struct ZpaqPlan {
  void* ws = nullptr;
  uint64_t len = 0, L = 0, nseg = 0, total = 0;
  const void *cur = nullptr, *ends = nullptr, *last = nullptr;
};
uint64_t zpaq_segment_len(uint32_t max_size);
int zpaq_check_device_params(uint32_t bits, uint32_t max_size);
int zpaq_cut_plan(const uint8_t* d_data, uint64_t len, uint32_t bits, uint32_t max_size, hipStream_t s, ZpaqPlan* p);
int zpaq_cut_emit(const ZpaqPlan& p, uint64_t* d_offsets, uint32_t* d_sizes, hipStream_t s);
void zpaq_cut_free(ZpaqPlan* p, hipStream_t s);
// The windows of sf_index_fd_zpaq over the `len` bytes of the regular file
// open on fd: the rows (file offsets) appended to rb, folded into bh.
int fd_zpaq_windows(int fd, uint64_t len, uint32_t bits, uint32_t max_size, RowBuf& rb, sf_host_sha1_stream* bh);

// The same over many files of one buffer (sf_cdc_files.hip; the geometry is
// sf_cdc_files_plan.hpp).  zpaq_files_check: every file lies in the buffer, or
// SF_ERANGE and *bad_file.  A plan is the cut of the checked files (at least
// one not empty) up to the count, in two parts: zpaq_files_begin allocates,
// uploads the per-file arrays (`host`: it lives until `synced`, or until the
// stream has been synchronised) and launches round 0, asynchronously;
// zpaq_files_finish makes at most max_rounds join launches (0 = no cap) and
// counts, blocking as zpaq_cut_plan: `total` rows of the settled files,
// unsettled[f] = 1 for the others.  zpaq_files_emit writes the rows and
// first_row[0 .. n_files] (asynchronous).
struct ZpaqFilesPlan {
  void* ws = nullptr;
  uint64_t L = 0, nseg = 0, total = 0, most = 0, recut = 0;
  uint32_t n_files = 0, launches = 0, n_unsettled = 0, bits = 0, max_size = 0;
  bool synced = false;
  const void* d_data = nullptr;
  void *spec = nullptr, *cur = nullptr, *seg[6] = {}, *ctr = nullptr, *d_files = nullptr, *round = nullptr,
       *scan_tmp = nullptr;
  size_t scan_bytes = 0;
  const void *ends = nullptr, *last = nullptr;
  std::vector<uint64_t> host;
  std::vector<uint8_t> unsettled;
};
int zpaq_files_check(uint64_t data_len, const uint64_t* offs, const uint64_t* lens, uint32_t n, uint32_t* bad_file);
int zpaq_files_begin(const uint8_t* d_data, const uint64_t* offs, const uint64_t* lens, uint32_t n, uint32_t bits,
                     uint32_t max_size, hipStream_t s, ZpaqFilesPlan* p);
int zpaq_files_finish(ZpaqFilesPlan* p, uint32_t max_rounds, hipStream_t s);
int zpaq_files_emit(const ZpaqFilesPlan& p, uint64_t* d_offsets, uint32_t* d_sizes, uint64_t* d_first_row,
                    hipStream_t s);
void zpaq_files_free(ZpaqFilesPlan* p, hipStream_t s);
void zpaq_files_stat(int k, uint64_t v);  // field k of sf_test_zpaq_files_stats

}  // namespace sfi
