// sf_stage.hpp -- what the host pipelines share (sf_host.cpp, sf_host_out.cpp,
// sf_files.cpp, sf_fds.cpp, sf_cut.cpp, sf_cdc.hip): the two-stage driver, the
// file reader and its sliced form, the checks and windows of an explicit list,
// the rows of a malloc'd result, the named slots of the per-device buffer
// cache, the stamp bracket of the descriptor routes and the page-lock
// registry of the in-place routes.
// No HIP here: what needs the runtime or the worker threads is declared and
// lives in sf_stage.cpp, sf_host.cpp, sf_pagelock.cpp and sf_pool.cpp, so a
// stand-alone program can test the templates on a CPU
// (tests/native/stage_driver.cpp).
// sf_internal.hpp includes this header.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/types.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>

#include "../../include/syncfast_amd.h"
#include "host_sha1.h"
#include "sf_inplace.hpp"

namespace sfi __attribute__((visibility("hidden"))) {

// What issue() answers when there is no stage k (input that ends where it
// ends: a pipe).  Positive: never an SF_ code.
constexpr int kNoMoreStages = 1;

// The pipeline every staged route runs: stage k is filled and enqueued on
// buffer set b = k & 1 (issue(k, b)) while stage k-1 is on the device, after
// stage k-2 -- the previous user of set b -- has been consumed (harvest(k-2,
// b), which waits for that stage's own event); then the at most two stages
// still in flight are harvested.  Stages are harvested once each, in
// increasing k.  issue returns SF_OK, an error or kNoMoreStages (stages
// [0, k) were all there is; n_stages = UINT64_MAX when only issue knows).
// The first result that is not SF_OK ends the run and is returned: nothing is
// issued or harvested after it.  Work it leaves in flight is the caller's to
// wait for (HostLease's destructor does).
template <typename Issue, typename Harvest>
int two_stage(uint64_t n_stages, Issue&& issue, Harvest&& harvest) {
  uint64_t issued = 0, harvested = 0;
  int rc;
  while (issued < n_stages) {
    if (issued >= 2) {
      if ((rc = harvest(harvested, (int)(harvested & 1))) != SF_OK) return rc;
      harvested++;
    }
    if ((rc = issue(issued, (int)(issued & 1))) == kNoMoreStages) break;
    if (rc != SF_OK) return rc;
    issued++;
  }
  for (; harvested < issued; harvested++)
    if ((rc = harvest(harvested, (int)(harvested & 1))) != SF_OK) return rc;
  return SF_OK;
}

// Bytes [pos, pos + want) of fd into dst (pread: the descriptor's position is
// not used or moved).  A signal (a profiler's, a Python handler's) is not a
// bad file: EINTR is tried again.  false: an error, or EOF before `want` bytes
// (the file is shorter than the caller was told: it shrank).
inline bool read_fully(int fd, uint8_t* dst, uint64_t pos, uint64_t want) {
  for (uint64_t got = 0; got < want;) {
    const ssize_t r = pread(fd, dst + got, want - got, (off_t)(pos + got));
    if (r < 0 && errno == EINTR) continue;
    if (r <= 0) return false;
    got += (uint64_t)r;
  }
  return true;
}

// A descriptor the call opened itself: closed on every return, and if an
// exception unwinds (to guarded(), in an entry point).
struct Fd {
  int fd;
  ~Fd() { if (fd >= 0) close(fd); }
};

// read_fully's write twin: src[0, want) to bytes [pos, pos + want) of fd
// (pwrite: the position is not used or moved), EINTR tried again.  false: an
// error, or a write that made no progress.
inline bool write_fully(int fd, const uint8_t* src, uint64_t pos, uint64_t want) {
  for (uint64_t put = 0; put < want;) {
    const ssize_t w = pwrite(fd, src + put, want - put, (off_t)(pos + put));
    if (w < 0 && errno == EINTR) continue;
    if (w <= 0) return false;
    put += (uint64_t)w;
  }
  return true;
}

// fn(a, e) -> SF_ code over [0, n) in slices of at least 4 MiB, about one per
// thread (one thread moves 10-16 GB/s from the page cache, below the PCIe link
// the stage is waiting for).  `run(nworkers, worker)` starts the workers,
// which take slices from an atomic counter; the first failure stops the rest
// and is returned.
constexpr uint64_t kMinSlice = 4ull << 20;
template <typename Run, typename Fn>
int for_slices(uint64_t n, unsigned threads, Run&& run, Fn&& fn) {
  const uint64_t slice = std::max<uint64_t>(kMinSlice, (n + threads - 1) / threads);
  const uint64_t nslices = (n + slice - 1) / slice;
  std::atomic<uint64_t> next{0};
  std::atomic<int> rc{SF_OK};
  auto worker = [&] {
    for (uint64_t i; (i = next.fetch_add(1)) < nslices && rc.load() == SF_OK;) {
      const int r = fn(i * slice, std::min(n, (i + 1) * slice));
      if (r != SF_OK) rc.store(r);
    }
  };
  run((unsigned)std::min<uint64_t>(threads, std::max<uint64_t>(nslices, 1)), worker);
  return rc.load();
}

// Bytes [pos, pos + n) of fd into dst, by slices.  A short read is SF_EIO.
template <typename Run>
int read_slices(int fd, uint8_t* dst, uint64_t pos, uint64_t n, unsigned threads, Run&& run) {
  return for_slices(n, threads, run, [&](uint64_t a, uint64_t e) {
    return read_fully(fd, dst + a, pos + a, e - a) ? SF_OK : SF_EIO;
  });
}

// An explicit list against the `len` bytes it cuts: block by block, SF_ERANGE
// (the block does not lie in [0, len)) before SF_EINVAL (its offset is below
// the previous block's); the first failing block's code.
inline int check_list(uint64_t len, const uint64_t* offsets, const uint32_t* sizes, uint64_t n) {
  for (uint64_t i = 0; i < n; i++) {
    if (offsets[i] > len || sizes[i] > len - offsets[i]) return SF_ERANGE;
    if (i && offsets[i] < offsets[i - 1]) return SF_EINVAL;
  }
  return SF_OK;
}

// One stage's share of an explicit list: blocks [b0, b1), whose bytes all lie
// in the window [w0, w1).  next_list_window takes the consecutive blocks from
// i (< n) whose window spans at most `target` bytes (a larger block is a
// window of its own), kMaxStageBlocks at most: a stage's list and digests
// stay ~135 MiB.
struct ListWindow {
  uint64_t b0, b1, w0, w1;
};
constexpr uint64_t kMaxStageBlocks = 1ull << 22;
inline ListWindow next_list_window(const uint64_t* offsets, const uint32_t* sizes, uint64_t n, uint64_t i,
                                   uint64_t target) {
  ListWindow s{i, i + 1, offsets[i], offsets[i] + sizes[i]};
  for (i++; i < n && i - s.b0 < kMaxStageBlocks; i++) {
    const uint64_t e = std::max(s.w1, offsets[i] + sizes[i]);
    if (e - s.w0 > target) break;
    s.w1 = e;
  }
  s.b1 = i;
  return s;
}

// Rows in a growing malloc'd buffer, handed to the caller by release() (the
// routes whose row count is known only at the end: sf_free_rows frees them).
struct RowBuf {
  sf_block_sig* p = nullptr;
  uint64_t n = 0, cap = 0;
  ~RowBuf() { free(p); }
  bool grow(uint64_t need) {
    if (need <= cap) return true;
    uint64_t c = std::max<uint64_t>({need, 2 * cap, 1024});
    void* q = realloc(p, c * sizeof(sf_block_sig));
    if (!q) return false;
    p = static_cast<sf_block_sig*>(q);
    cap = c;
    return true;
  }
  sf_block_sig* release() {
    sf_block_sig* q = p;
    p = nullptr;
    n = cap = 0;
    return q;
  }
};

// Runs `worker` on the calling thread and on up to nthreads-1 of the
// library's kept helper threads (sf_pool.cpp).  The workers share an atomic
// work counter, so helpers busy elsewhere or a thread the system refuses only
// lower the parallelism.  Returns when every helper that started the worker
// has finished it; an exception from any of them is rethrown here.
void run_pool_fn(unsigned nthreads, const std::function<void()>& worker);
template <typename F>
inline void run_pool(unsigned nthreads, F&& worker) {
  if (nthreads <= 1) {
    worker();
    return;
  }
  run_pool_fn(nthreads, std::function<void()>(std::ref(worker)));
}

// Reader threads for `items` work items: min(io_threads(), the machine's
// hardware threads, items), one at least (sf_stage.cpp).
unsigned pool_threads(uint64_t items = UINT64_MAX);

// for_slices / read_slices on the library's worker threads.
template <typename Fn>
int sliced(uint64_t n, Fn&& fn) {
  return for_slices(n, pool_threads(), [](unsigned t, auto& worker) { run_pool(t, worker); }, fn);
}
inline int read_sliced(int fd, uint8_t* dst, uint64_t pos, uint64_t n) {
  return read_slices(fd, dst, pos, n, pool_threads(), [](unsigned t, auto& worker) { run_pool(t, worker); });
}

// fstat(fd) as a stamp (and the file's mode); false if fstat fails.  Two
// stamps match when dev, ino, size and mtime are equal and, unless the link
// count changed, ctime too (include/syncfast_amd.h, sf_file_stamp).
// Defined in sf_host.cpp.
bool stamp_of(int fd, sf_file_stamp* s, mode_t* mode);
bool same_stamp(const sf_file_stamp& a, const sf_file_stamp& b);

// The process-wide registry of host ranges this library page-locked
// (sf_pagelock.cpp), behind the lock / unlock of InplaceRegions.  lock_pages
// page-locks [a, e) (page edges) if it is private anonymous memory that no
// concurrent call of ours has locked -- a file mapping never is; the counters
// pages_locked and not_anon_refused record what it did -- and unlock_pages
// undoes one lock_pages by its start.  range_locked_by_us: [a, e) overlaps a
// range of the registry.  pinned_by_hip: the HIP runtime knows both ends of
// [a, e) as page-locked host memory (hipHostMalloc, hipHostRegister).
PageLock lock_pages(uintptr_t a, uintptr_t e);
void unlock_pages(uintptr_t a);
bool range_locked_by_us(uintptr_t a, uintptr_t e);
bool pinned_by_hip(uintptr_t a, uintptr_t e);

// HostRes slots, device and pinned alike: the two stages' bytes; the digest
// table of one whole file (the in-place route); the two stages' digests; the
// two stages' block lists (offsets, then sizes) or, in sf_index_files, their
// files' blocks_hash values.  Set b of a pair is slot + b.
enum Slot { kSlotData = 0, kSlotFileTable = 2, kSlotDigests = 3, kSlotAux = 5 };

// The buffers of set b: data_bytes of stage bytes, digests of `blocks` blocks,
// aux_bytes of list (or file hashes); a part asked for with kNoBuf is not
// acquired (0 is: the cache's smallest buffer).  sf_stage.cpp.
class HostLease;
constexpr uint64_t kNoBuf = UINT64_MAX;
struct StageBufs {
  void *ddata = nullptr, *pin = nullptr, *ddig = nullptr, *pdig = nullptr, *daux = nullptr, *paux = nullptr;
};
int stage_bufs(HostLease& res, int b, uint64_t data_bytes, uint64_t blocks, uint64_t aux_bytes, StageBufs* s);
constexpr uint64_t kListEntry = sizeof(uint64_t) + sizeof(uint32_t);  // bytes of a list per block

// body(stamp, mode) between two stamps of fd: the first against the caller's
// (`expect`, taken before its chunker read the file; may be NULL).  A read
// that came up short (the file shrank: SF_EIO) or a complete one over a file
// whose stamp moved is SF_EAGAIN, never rows that mix one version's
// boundaries with another's bytes; other results (argument errors, SF_ENOSPC,
// device errors) pass.
template <typename Body>
int stamped(int fd, const sf_file_stamp* expect, Body body) {
  sf_file_stamp before{}, after{};
  mode_t mode = 0;
  if (!stamp_of(fd, &before, &mode)) return SF_EIO;
  if (expect && !same_stamp(before, *expect)) return SF_EAGAIN;
  const int rc = body(before, mode);
  if (rc != SF_OK && rc != SF_EIO) return rc;
  if (!stamp_of(fd, &after, nullptr)) return SF_EIO;
  return same_stamp(before, after) ? rc : SF_EAGAIN;
}

// The first `keep` rows of a window that starts at byte A of its file, from
// the window's pinned list (n offsets in the window, then n sizes) and its
// digests, folded into the file's blocks_hash (compute_blocks_hash,
// src/index.rs:661-682) in order.  false: no memory.
inline bool append_window_rows(RowBuf& rows, uint64_t A, const void* plist, const void* pdig, uint64_t n,
                               uint64_t keep, sf_host_sha1_stream* bh) {
  const uint64_t* lo = static_cast<const uint64_t*>(plist);
  const uint32_t* lz = reinterpret_cast<const uint32_t*>(lo + n);
  const uint8_t* dg = static_cast<const uint8_t*>(pdig);
  if (!rows.grow(rows.n + keep)) return false;
  sf_block_sig* o = rows.p + rows.n;
  for (uint64_t j = 0; j < keep; j++) {
    o[j].offset = A + lo[j];
    o[j].size = lz[j];
    memcpy(o[j].sha1, dg + 20 * j, 20);
  }
  rows.n += keep;
  sf_host_sha1_update(bh, dg, keep * 20);
  return true;
}

// SF_TRACE=1: phase times of a many-file call on stderr (probe only).  `pre`:
// the route's own phases before its pipeline.
struct Trace {
  bool on;
  std::chrono::steady_clock::time_point t0, last;
  double pre_ms[2] = {0, 0}, read_ms = 0, issue_ms = 0, wait_ms = 0, harvest_ms = 0;
  explicit Trace(bool on_) : on(on_) { t0 = last = std::chrono::steady_clock::now(); }
  void lap(double& acc) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    acc += std::chrono::duration<double, std::milli>(now - last).count();
    last = now;
  }
  void report(const char* head) {  // head: "<entry point> trace: <counts>: <pre phases>"
    const double tot = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "%s read %.2f issue %.2f wait %.2f harvest %.2f total %.2f ms\n", head, read_ms, issue_ms, wait_ms,
            harvest_ms, tot);
  }
};

}  // namespace sfi
