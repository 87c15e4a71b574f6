// sf_host.cpp -- the C-ABI's host-memory indexing entry points
// (include/syncfast_amd.h): bytes in host memory, in a file or behind a
// descriptor -> pinned stages, or the caller's own pages page-locked region by
// region (sf_inplace.hpp, sf_pagelock.cpp) -> H2D -> the gfx950 kernels
// (launched through sf_launch.hpp) -> D2H of the rows, plus the per-device
// cache of streams and buffers the host entry points share, the stamp helpers
// and the host SHA-1 helpers.  The device-to-descriptor writers are
// sf_host_out.cpp.  HIP runtime API only: built with the host compiler.
#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "host_sha1.h"
#include "sf_launch.hpp"
#include "sf_stage.hpp"

namespace sfi __attribute__((visibility("hidden"))) {
std::mutex g_res_mu[kMaxDevices];
HostRes* g_res[kMaxDevices];
}  // namespace sfi

using namespace sfi;

namespace {

// RAII pinned allocation (the in-place route's bounce buffer).
struct PinBuf {
  void* p = nullptr;
  ~PinBuf() { if (p) (void)hipHostFree(p); }
};

// Smallest host buffer that sf_index_buffer / sf_index_buffer_blocks copy in
// place (page-locked) instead of staging through the pinned stages.  Per call,
// with the per-device set cached (scripts/inplace_min_probe.py): a buffer
// gains in place from 1 MiB up (7.6 vs 6.1 GB/s; 32 MiB: 45 vs 21).
// SF_INPLACE_MIN_MIB overrides it (A/B knob).
inline uint64_t inplace_min_bytes() {
  const int64_t v = knob(K_INPLACE_MIN_MIB);
  return v >= 0 ? (uint64_t)v << 20 : 1ull << 20;
}

// Chunk of input handled per pipeline stage, staged or in place: a whole
// number of blocks, about 256 MiB.
inline uint64_t file_stage_bytes(uint32_t bs) {
  const int64_t sm = knob(K_TEST_STREAM_STAGE_MIB);  // test hook: small stages exercise the pipeline
  const uint64_t want = sm > 0 ? (uint64_t)sm << 20 : (256ull << 20);
  return std::max<uint64_t>(1, want / bs) * bs;
}

// A stage's digests on their way back to the host, behind the kernel that
// wrote them on s, and the stage's event behind that copy: what a harvest
// waits for before it reads pdig.
inline int digests_back(void* pdig, const void* ddig, uint64_t nb, hipStream_t s, hipEvent_t done) {
  SF_HIP(hipMemcpyAsync(pdig, ddig, nb * 20, hipMemcpyDeviceToHost, s));
  SF_HIP(hipEventRecord(done, s));
  return SF_OK;
}

// Rows [first, first + nb) of a fixed tiling from their digests; `bytes`: what
// the input holds from row `first` on (the last row may be short).
inline void write_rows(sf_block_sig* o, uint64_t first, uint64_t nb, const uint8_t* dg, uint64_t bytes, uint32_t bs) {
  for (uint64_t i = 0; i < nb; i++) {
    o[i].offset = (first + i) * bs;
    o[i].size = (uint32_t)std::min<uint64_t>(bs, bytes - i * bs);
    memcpy(o[i].sha1, dg + 20 * i, 20);
  }
}

void empty_blocks_hash(uint8_t* blocks_hash) {  // compute_blocks_hash of no blocks: SHA-1("")
  if (!blocks_hash) return;
  sf_host_sha1_stream bh;
  sf_host_sha1_begin(&bh);
  sf_host_sha1_final(&bh, blocks_hash);
}

// In-place route of sf_index_buffer: the DMA engine reads the caller's pages
// directly, no staging memcpy.  Only private anonymous memory is page-locked
// (lock_pages); a file mapping passed as a buffer takes the staged route.  Per
// ~256 MiB stage, on alternating streams: H2D, the block kernel, D2H of the
// stage's digests.  The host overlaps the rest with the PCIe link:
//   - the pages are page-locked (hipHostRegister) one region ahead of the
//     copy that reads them, instead of all before the first copy;
//   - stage k-1's rows are written and its digests folded into the file's
//     blocks_hash (src/index.rs:661-682) while stage k is on the link.
// The regions are InplaceRegions' (sf_inplace.hpp): a stage's bytes lie in
// regions k-1 (its head, up to the first page edge) and k, and no page is
// registered twice.  A region that cannot be registered after the first one
// switches the rest of the stages to a pinned bounce buffer (memcpy, one stage
// at a time): slower, same result.  Returns SF_ENOTSUP (nothing done) when the
// first region cannot be registered, so the caller can take its staged route.
// SF_INPLACE_SERIAL=1 registers the whole range first, as one region, and
// writes rows and blocks_hash after the last stage (the previous form; A/B
// knob).
int index_inplace(const uint8_t* data, uint64_t len, uint32_t bs, sf_block_sig* out, uint64_t cap,
                  uint64_t* n_out, uint8_t* blocks_hash) {
  const uint64_t nblocks = ceil_div(len, bs);
  if (n_out) *n_out = nblocks;
  if (nblocks > cap) return SF_ENOSPC;
  const bool serial = knob(K_INPLACE_SERIAL) != 0;
  const uint64_t stage = std::min<uint64_t>(file_stage_bytes(bs), len);
  const uint64_t nstages = ceil_div(len, stage);
  const uintptr_t pg = (uintptr_t)sysconf(_SC_PAGESIZE);
  const uintptr_t lo = (uintptr_t)data, hi = lo + len;
  std::vector<uintptr_t> starts(serial ? 1 : nstages);
  for (size_t k = 0; k < starts.size(); k++) starts[k] = lo + k * stage;
  // A buffer that is already page-locked (hipHostMalloc, or registered by the
  // caller) is copied from as it is: hipHostRegister would refuse it.
  // (pages a concurrent call of ours locked are not the caller's pinning)
  const bool prepinned = pinned_by_hip(lo, hi) && !range_locked_by_us(lo & ~(pg - 1), (hi + pg - 1) & ~(pg - 1));
  // Declared before bounce and the lease: the lease's release waits for the
  // streams first, then the regions are unlocked.
  InplaceRegions regions(
      pg, starts, hi, [&](uintptr_t a, uintptr_t e) { return prepinned ? kPinnedByCaller : lock_pages(a, e); },
      unlock_pages, prepinned ? -1 : knob(K_TEST_INPLACE_FAIL_AT));
  regions.lock_ahead(0);
  if (!regions.direct(0)) return SF_ENOTSUP;
  PinBuf bounce;  // only if a region after the first cannot be registered
  HostLease res;
  hipStream_t* st;
  hipEvent_t* done;
  void *ddata[2], *ddig, *pdig;
  int rc = res.streams(st, done);
  for (int i = 0; i < 2 && rc == SF_OK; i++) rc = res.dev(kSlotData + i, stage, &ddata[i]);
  if (rc == SF_OK) rc = res.dev(kSlotFileTable, nblocks * 20, &ddig);
  if (rc == SF_OK) rc = res.pin(kSlotFileTable, nblocks * 20, &pdig);
  if (rc != SF_OK) return rc;
  sf_host_sha1_stream bh;
  sf_host_sha1_begin(&bh);
  const uint8_t* dg = static_cast<const uint8_t*>(pdig);
  auto rows = [&](uint64_t k) {  // rows + blocks_hash of stage k (its digests are on the host)
    const uint64_t b0 = k * stage / bs, b1 = std::min(nblocks, ceil_div((k + 1) * stage, bs));
    write_rows(out + b0, b0, b1 - b0, dg + 20 * b0, len - b0 * bs, bs);
    if (blocks_hash) sf_host_sha1_update(&bh, dg + 20 * b0, (b1 - b0) * 20);
  };
  // An error return leaves the rest to the lease, which waits for both streams.
  for (uint64_t k = 0; k < nstages; k++) {
    const int b = (int)(k & 1);
    const uint64_t off = k * stage;
    const uint64_t n = std::min(stage, len - off);
    const uint64_t b0 = off / bs, nb = ceil_div(n, bs);
    uint8_t* dd = static_cast<uint8_t*>(ddig) + b0 * 20;
    const uint8_t* src = data + off;
    const uint64_t r = serial ? 0 : k;  // the region stage k ends in
    // A copy must lie inside ONE registration: a stage that starts mid-page
    // copies its head (up to the page edge, in region k-1) separately from
    // the rest (region k).
    uint64_t head = 0;
    if (regions.direct(r)) {
      head = regions.head(r, (uintptr_t)src, n);
    } else {  // region k is not page-locked: bounce
      for (int i = 0; i < 2; i++) SF_HIP(hipStreamSynchronize(st[i]));
      if (!bounce.p) SF_HIP(hipHostMalloc(&bounce.p, stage, hipHostMallocDefault));
      memcpy(bounce.p, src, n);
      src = static_cast<const uint8_t*>(bounce.p);
    }
    // stream b is in order: the copy into ddata[b] waits for the kernel of
    // stage k-2 that read it.
    if (head) SF_HIP(hipMemcpyAsync(ddata[b], src, head, hipMemcpyHostToDevice, st[b]));
    if (n > head)
      SF_HIP(hipMemcpyAsync(static_cast<uint8_t*>(ddata[b]) + head, src + head, n - head, hipMemcpyHostToDevice,
                            st[b]));
    if ((rc = launch_fixed(ddata[b], n, bs, nb, dd, st[b])) != SF_OK) return rc;
    if (serial) continue;
    if ((rc = digests_back(static_cast<uint8_t*>(pdig) + b0 * 20, dd, nb, st[b], done[b])) != SF_OK) return rc;
    regions.lock_ahead(k + 1);
    if (k >= 1) {
      SF_HIP(hipEventSynchronize(done[b ^ 1]));
      rows(k - 1);
    }
  }
  for (int i = 0; i < 2; i++) SF_HIP(hipStreamSynchronize(st[i]));
  if (serial) {
    SF_HIP(hipMemcpyAsync(pdig, ddig, nblocks * 20, hipMemcpyDeviceToHost, st[0]));
    SF_HIP(hipStreamSynchronize(st[0]));
    for (uint64_t k = 0; k < nstages; k++) rows(k);
  } else {
    rows(nstages - 1);
  }
  if (blocks_hash) sf_host_sha1_final(&bh, blocks_hash);
  return SF_OK;
}

// Staged pipeline (sf_index_file's pread route, the sequential route of
// sf_index_fd, sf_index_buffer below its in-place size): two pinned stages of
// whole blocks (the last one short).  `fill(dst, off, cap, &n, &eof)` puts the
// next input bytes into a pinned stage; per stage, on alternating streams, H2D
// + block kernel + D2H of the stage's digests.  While stage k is being filled, stage k-1 is on the
// device and stage k-2's rows are emitted (`emit(first_block, n_blocks,
// digests, stage_bytes)`) and its digests folded into the streaming
// blocks_hash (src/index.rs:661-682), in order.  No device memory maps or
// registers the caller's file: the host only ever reads it with read/pread.
template <typename FillFn, typename EmitFn>
int staged_pipeline(uint32_t bs, uint64_t stage, FillFn fill, EmitFn emit, uint8_t* blocks_hash) {
  HostLease res;
  hipStream_t* st;
  hipEvent_t* done;
  StageBufs sb[2];
  int rc = res.streams(st, done);
  for (int i = 0; i < 2 && rc == SF_OK; i++) rc = stage_bufs(res, i, stage, stage / bs, kNoBuf, &sb[i]);
  if (rc != SF_OK) return rc;
  sf_host_sha1_stream bh;
  sf_host_sha1_begin(&bh);
  uint64_t bytes_of[2] = {0, 0}, first_of[2] = {0, 0};
  uint64_t total = 0;
  bool eof = false;
  rc = two_stage(
      UINT64_MAX,
      [&](uint64_t, int b) {
        if (eof) return kNoMoreStages;
        uint8_t* dst = static_cast<uint8_t*>(sb[b].pin);
        uint64_t n = 0;
        const int r = fill(dst, total, stage, &n, &eof);
        if (r != SF_OK) return r;
        if (n == 0) return kNoMoreStages;
        const uint64_t nb = ceil_div(n, bs);
        bytes_of[b] = n;
        first_of[b] = total / bs;  // every earlier stage was whole blocks
        total += n;
        SF_HIP(hipMemcpyAsync(sb[b].ddata, dst, n, hipMemcpyHostToDevice, st[b]));
        if (const int rl = launch_fixed(sb[b].ddata, n, bs, nb, sb[b].ddig, st[b])) return rl;
        return digests_back(sb[b].pdig, sb[b].ddig, nb, st[b], done[b]);
      },
      [&](uint64_t, int b) {
        SF_HIP(hipEventSynchronize(done[b]));
        const uint64_t nb = ceil_div(bytes_of[b], bs);
        const uint8_t* dg = static_cast<const uint8_t*>(sb[b].pdig);
        const int r = emit(first_of[b], nb, dg, bytes_of[b]);
        if (r != SF_OK) return r;
        if (blocks_hash) sf_host_sha1_update(&bh, dg, nb * 20);
        return SF_OK;
      });
  if (rc == SF_OK && blocks_hash) sf_host_sha1_final(&bh, blocks_hash);
  return rc;
}

// Sequential route (input that cannot seek: a pipe, FIFO, socket or
// character device -- what index_file's File::open + read accepts,
// src/index.rs:615,625): read() to EOF.
static int index_stream(int fd, uint32_t bs, RowBuf& rows, uint8_t* blocks_hash) {
  auto fill = [&](uint8_t* dst, uint64_t, uint64_t cap, uint64_t* n, bool* eof) {
    *n = 0;
    while (*n < cap) {
      const ssize_t r = read(fd, dst + *n, cap - *n);
      if (r < 0 && errno == EINTR) continue;
      if (r < 0) return SF_EIO;
      if (r == 0) { *eof = true; break; }
      *n += (uint64_t)r;
    }
    return SF_OK;
  };
  auto emit = [&](uint64_t first, uint64_t nb, const uint8_t* dg, uint64_t bytes) {
    if (!rows.grow(rows.n + nb)) return SF_ENOMEM;
    write_rows(rows.p + rows.n, first, nb, dg, bytes, bs);
    rows.n += nb;
    return SF_OK;
  };
  return staged_pipeline(bs, file_stage_bytes(bs), fill, emit, blocks_hash);
}

// Regular file of known length: each stage is read by several threads in
// parallel (one pread stream per slice; one thread copies from the page
// cache at ~16 GB/s, below PCIe).  A short read (the file shrank) is SF_EIO.
// Read-ahead (SF_FADVISE, default on): the file is declared sequential and,
// before stage k is read, the kernel is asked to start fetching stage k+1
// (POSIX_FADV_WILLNEED), so a file that is not in the page cache streams from
// the disk while stage k is copied; for a resident file both are no-ops.
inline bool fadvise_on() { return knob(K_FADVISE) != 0; }

}  // namespace

namespace sfi {

// Bytes [base, base + len) of the file (base a multiple of bs: a shard of
// one logical file); row offsets are file offsets.
int index_file_pread(int fd, uint64_t base, uint64_t len, uint32_t bs, sf_block_sig* out, uint8_t* blocks_hash) {
  const bool adv = fadvise_on();
  if (adv) (void)posix_fadvise(fd, (off_t)base, (off_t)len, POSIX_FADV_SEQUENTIAL);
  uint64_t window = 0;
  auto fill = [&](uint8_t* dst, uint64_t off, uint64_t cap, uint64_t* nout, bool* eof) {
    const uint64_t n = std::min(cap, len - off);
    *nout = n;
    *eof = off + n >= len;
    if (adv && !*eof)
      (void)posix_fadvise(fd, (off_t)(base + off + n), (off_t)std::min(cap, len - off - n), POSIX_FADV_WILLNEED);
    const int rc = read_sliced(fd, dst, base + off, n);
    read_hook(window++);
    return rc;
  };
  auto emit = [&](uint64_t first, uint64_t nb, const uint8_t* dg, uint64_t bytes) {
    write_rows(out + first, base / bs + first, nb, dg, bytes, bs);
    return SF_OK;
  };
  return staged_pipeline(bs, file_stage_bytes(bs), fill, emit, blocks_hash);
}

}  // namespace sfi

namespace {

// The whole regular file open on fd, len bytes long, in fixed blocks: the
// count to *n_out, against cap, then its rows and blocks_hash.
int index_regular(int fd, uint64_t len, uint32_t bs, sf_block_sig* out, uint64_t cap, uint64_t* n_out,
                  uint8_t* blocks_hash) {
  const uint64_t nb = len ? ceil_div(len, bs) : 0;
  if (n_out) *n_out = nb;
  if (nb > cap) return SF_ENOSPC;
  if (nb && !out) return SF_EINVAL;
  if (nb == 0) {
    empty_blocks_hash(blocks_hash);
    return SF_OK;
  }
  return index_file_pread(fd, 0, len, bs, out, blocks_hash);
}

}  // namespace

namespace {

// Copy n bytes into a pinned stage with several threads (one thread moves
// ~10-16 GB/s, below the PCIe link the stage is waiting for).
inline void par_memcpy(uint8_t* dst, const uint8_t* src, uint64_t n) {
  (void)sliced(n, [&](uint64_t a, uint64_t e) {
    memcpy(dst + a, src + a, e - a);
    return SF_OK;
  });
}

// sf_index_buffer_blocks: the list is cut into stages of consecutive blocks
// whose window spans at most ~256 MiB (a larger block is a stage of its own);
// per stage, on alternating streams: the window and the stage's list
// (offsets relative to the window, sizes) are copied into pinned buffers and
// to HBM, sha1_table_kernel hashes the blocks, the digests come back.  While
// stage k is copied in, stage k-1 is on the device and stage k-2's rows are
// written and folded into blocks_hash, in list order.
// `fill(dst, w0, w1)` puts bytes [w0, w1) of the input into the pinned stage.
// `direct` (the buffer form): the caller's bytes, copied to HBM in place --
// page-locked region by region one stage ahead (InplaceRegions), as
// index_inplace does -- when
// the stage windows are disjoint and at least two pages each (a chunker's
// list); a region that cannot be page-locked sends it and every later stage
// through `fill`.
template <typename FillFn>
int index_list_pipeline(FillFn fill, const uint64_t* offsets, const uint32_t* sizes, uint64_t n, sf_block_sig* out,
                        uint8_t* blocks_hash, const uint8_t* direct = nullptr) {
  const uint64_t target = file_stage_bytes(1);  // ~256 MiB (SF_TEST_STREAM_STAGE_MIB test hook)
  std::vector<ListWindow> stages;
  uint64_t max_win = 0, max_blocks = 0;
  for (uint64_t i = 0; i < n; i = stages.back().b1) {
    const ListWindow s = next_list_window(offsets, sizes, n, i, target);
    max_win = std::max(max_win, s.w1 - s.w0);
    max_blocks = std::max(max_blocks, s.b1 - s.b0);
    stages.push_back(s);
  }
  // In place only when every stage's window is at least two pages and the
  // windows are disjoint; otherwise there are no regions, and every stage is
  // filled.
  const uint64_t pg = (uint64_t)sysconf(_SC_PAGESIZE);
  const size_t nst = stages.size();
  bool inplace = direct != nullptr;
  if (inplace) {
    inplace = knob(K_NO_HOSTREG) == 0 && stages.back().w1 - stages[0].w0 >= inplace_min_bytes();
    for (size_t k = 0; k < nst && inplace; k++)
      inplace = stages[k].w1 - stages[k].w0 >= 2 * pg && (k == 0 || stages[k - 1].w1 <= stages[k].w0);
  }
  std::vector<uintptr_t> starts(inplace ? nst : 0);
  for (size_t k = 0; k < starts.size(); k++) starts[k] = (uintptr_t)direct + stages[k].w0;
  // Declared before the lease: the lease's release waits for the streams
  // first, then the regions are unlocked.
  InplaceRegions regions(pg, starts, (uintptr_t)direct + stages.back().w1, lock_pages, unlock_pages,
                         knob(K_TEST_INPLACE_FAIL_AT));
  regions.lock_ahead(0);
  HostLease res;
  hipStream_t* st;
  hipEvent_t* done;
  StageBufs sb[2];
  int rc = res.streams(st, done);
  for (int i = 0; i < 2 && rc == SF_OK; i++)
    rc = stage_bufs(res, i, max_win, max_blocks, max_blocks * kListEntry, &sb[i]);
  if (rc != SF_OK) return rc;
  sf_host_sha1_stream bh;
  sf_host_sha1_begin(&bh);
  rc = two_stage(
      nst,
      [&](uint64_t k, int b) {
        const ListWindow& s = stages[k];
        const uint64_t nb = s.b1 - s.b0, win = s.w1 - s.w0;
        const bool direct_k = regions.direct(k);
        if (!direct_k)
          if (const int r = fill(static_cast<uint8_t*>(sb[b].pin), s.w0, s.w1)) return r;
        uint64_t* lo = static_cast<uint64_t*>(sb[b].paux);
        uint32_t* lz = reinterpret_cast<uint32_t*>(lo + nb);
        for (uint64_t i = 0; i < nb; i++) {
          lo[i] = offsets[s.b0 + i] - s.w0;
          lz[i] = sizes[s.b0 + i];
        }
        const uint64_t* d_off = static_cast<const uint64_t*>(sb[b].daux);
        const uint32_t* d_sz = reinterpret_cast<const uint32_t*>(d_off + nb);
        if (direct_k) {  // a copy lies inside ONE registration: the head (region k-1) apart from the rest
          const uint8_t* src = direct + s.w0;
          const uint64_t head = regions.head(k, (uintptr_t)src, win);
          if (head) SF_HIP(hipMemcpyAsync(sb[b].ddata, src, head, hipMemcpyHostToDevice, st[b]));
          if (win > head)
            SF_HIP(hipMemcpyAsync(static_cast<uint8_t*>(sb[b].ddata) + head, src + head, win - head,
                                  hipMemcpyHostToDevice, st[b]));
        } else if (win) {
          SF_HIP(hipMemcpyAsync(sb[b].ddata, sb[b].pin, win, hipMemcpyHostToDevice, st[b]));
        }
        SF_HIP(hipMemcpyAsync(sb[b].daux, sb[b].paux, nb * kListEntry, hipMemcpyHostToDevice, st[b]));
        regions.lock_ahead(k + 1);  // one region ahead of the copies that read it
        // every block was checked to lie in [0, len), so in its window: no status word
        if (const int r = launch_table(sb[b].ddata, win, d_off, d_sz, nb, sb[b].ddig, nullptr, st[b])) return r;
        return digests_back(sb[b].pdig, sb[b].ddig, nb, st[b], done[b]);
      },
      [&](uint64_t k, int b) {
        SF_HIP(hipEventSynchronize(done[b]));
        const ListWindow& s = stages[k];
        const uint8_t* dg = static_cast<const uint8_t*>(sb[b].pdig);
        for (uint64_t i = s.b0; i < s.b1; i++) {
          out[i].offset = offsets[i];
          out[i].size = sizes[i];
          memcpy(out[i].sha1, dg + 20 * (i - s.b0), 20);
        }
        if (blocks_hash) sf_host_sha1_update(&bh, dg, (s.b1 - s.b0) * 20);
        return SF_OK;
      });
  if (rc == SF_OK && blocks_hash) sf_host_sha1_final(&bh, blocks_hash);
  return rc;
}

// ------------------------------------------------ one open regular file
// index_file opens the file once and takes its mtime, its boundaries and its
// bytes from that one handle (src/index.rs:615-625).  The descriptor routes
// read the caller's open file with pread and compare its stamp (fstat) when
// the call starts -- against the caller's, taken before its chunker read the
// file -- and after the last window is read: a file changed in between gives
// SF_EAGAIN, never rows that mix one version's boundaries with another's bytes.
}  // namespace

namespace sfi {

bool stamp_of(int fd, sf_file_stamp* s, mode_t* mode) {
  struct stat sb;
  if (fstat(fd, &sb) != 0) return false;
  s->dev = (uint64_t)sb.st_dev;
  s->ino = (uint64_t)sb.st_ino;
  s->size = (uint64_t)sb.st_size;
  s->nlink = (uint64_t)sb.st_nlink;
  s->mtime_sec = (int64_t)sb.st_mtim.tv_sec;
  s->mtime_nsec = (int64_t)sb.st_mtim.tv_nsec;
  s->ctime_sec = (int64_t)sb.st_ctim.tv_sec;
  s->ctime_nsec = (int64_t)sb.st_ctim.tv_nsec;
  if (mode) *mode = sb.st_mode;
  return true;
}

// ctime also moves when a link is added or removed (a rename over the path
// unlinks the open file, whose bytes do not change): it is compared only
// while the link count stays the same (include/syncfast_amd.h).
bool same_stamp(const sf_file_stamp& a, const sf_file_stamp& b) {
  return a.dev == b.dev && a.ino == b.ino && a.size == b.size && a.mtime_sec == b.mtime_sec &&
         a.mtime_nsec == b.mtime_nsec &&
         (a.nlink != b.nlink || (a.ctime_sec == b.ctime_sec && a.ctime_nsec == b.ctime_nsec));
}

}  // namespace sfi

namespace {

// An explicit list over the regular file open on fd, len bytes long: checked
// against len, then windows pread into the pinned stages of the list pipeline.
int index_fd_list(int fd, uint64_t len, const uint64_t* offsets, const uint32_t* sizes, uint64_t n,
                  sf_block_sig* out, uint8_t* blocks_hash) {
  if (const int rc = check_list(len, offsets, sizes, n)) return rc;
  if (n == 0) {
    empty_blocks_hash(blocks_hash);
    return SF_OK;
  }
  uint64_t window = 0;
  auto fill = [&](uint8_t* dst, uint64_t w0, uint64_t w1) {
    const int r = read_sliced(fd, dst, w0, w1 - w0);
    read_hook(window++);
    return r;
  };
  return index_list_pipeline(fill, offsets, sizes, n, out, blocks_hash);
}

}  // namespace

// C-ABI entry points: each body runs inside guarded(), which turns a C++
// exception into an error code.
extern "C" {

int sf_release_host_cache(void) {
  return guarded([&] {
    for (int d = 0; d < kMaxDevices; d++) {
      std::lock_guard<std::mutex> lk(g_res_mu[d]);  // waits for a call using the set
      if (g_res[d]) {
        g_res[d]->free_all();
        delete g_res[d];
        g_res[d] = nullptr;
      }
    }
    return SF_OK;
  });
}

int sf_index_buffer_blocks(const uint8_t* data, uint64_t len, const uint64_t* offsets, const uint32_t* sizes,
                           uint64_t n, sf_block_sig* out, uint8_t blocks_hash[20]) {
  return guarded([&] {
    if (n && (!offsets || !sizes || !out)) return SF_EINVAL;
    if (len && !data) return SF_EINVAL;
    // The whole list is checked before any byte moves (the device form zeroes
    // an out-of-range block's digest instead; a host caller gets the error).
    if (const int rc = check_list(len, offsets, sizes, n)) return rc;
    if (n == 0) {
      empty_blocks_hash(blocks_hash);
      return SF_OK;
    }
    auto fill = [&](uint8_t* dst, uint64_t w0, uint64_t w1) {
      par_memcpy(dst, data + w0, w1 - w0);
      return SF_OK;
    };
    return index_list_pipeline(fill, offsets, sizes, n, out, blocks_hash, data);
  });
}

int sf_index_file_blocks(const char* path, const uint64_t* offsets, const uint32_t* sizes, uint64_t n,
                         sf_block_sig* out, uint8_t blocks_hash[20]) {
  return guarded([&] {
    if (!path || (n && (!offsets || !sizes || !out))) return SF_EINVAL;
    const Fd f{open(path, O_RDONLY | O_NONBLOCK)};  // a FIFO is refused below, not waited on
    if (f.fd < 0) return SF_EIO;
    return stamped(f.fd, nullptr, [&](const sf_file_stamp& st, mode_t mode) {
      if (!S_ISREG(mode)) return SF_EIO;  // the list names file offsets: a seekable file
      return index_fd_list(f.fd, st.size, offsets, sizes, n, out, blocks_hash);
    });
  });
}

int sf_index_fd_blocks(int fd, const sf_file_stamp* expect, const uint64_t* offsets, const uint32_t* sizes,
                       uint64_t n, sf_block_sig* out, uint8_t blocks_hash[20]) {
  return guarded([&] {
    if (fd < 0 || (n && (!offsets || !sizes || !out))) return SF_EINVAL;
    return stamped(fd, expect, [&](const sf_file_stamp& st, mode_t mode) {
      if (!S_ISREG(mode)) return SF_EINVAL;  // a pipe cannot be read twice: sf_index_buffer_blocks
      return index_fd_list(fd, st.size, offsets, sizes, n, out, blocks_hash);
    });
  });
}

int sf_index_fd_fixed(int fd, const sf_file_stamp* expect, uint32_t block_size, sf_block_sig* out, uint64_t cap,
                      uint64_t* n_out, uint8_t blocks_hash[20]) {
  return guarded([&] {
    if (n_out) *n_out = 0;
    if (const int rc = check_block_size(block_size)) return rc;
    if (fd < 0) return SF_EINVAL;
    return stamped(fd, expect, [&](const sf_file_stamp& st, mode_t mode) {
      if (!S_ISREG(mode)) return SF_EINVAL;  // a stream: sf_index_fd
      return index_regular(fd, st.size, block_size, out, cap, n_out, blocks_hash);
    });
  });
}

int sf_file_stamp_fd(int fd, sf_file_stamp* out) {
  if (fd < 0 || !out) return SF_EINVAL;
  return stamp_of(fd, out, nullptr) ? SF_OK : SF_EIO;
}

int sf_index_buffer(const uint8_t* data, uint64_t len, uint32_t block_size, sf_block_sig* out, uint64_t cap,
                    uint64_t* n_out) {
  return guarded([&] {
    int rc = check_block_size(block_size);
    if (rc) return rc;
    if (len && (!data || !out)) return SF_EINVAL;
    // Large buffers of private anonymous memory: page-locked in place (no
    // staging memcpy); SF_NO_HOSTREG=1 forces the staged path (A/B knob).
    if (len && len >= inplace_min_bytes() && knob(K_NO_HOSTREG) == 0) {
      rc = index_inplace(data, len, block_size, out, cap, n_out, nullptr);
      if (rc != SF_ENOTSUP) return rc;
    }
    // Staged: memcpy into the pinned stages, the file route's pipeline.
    const uint64_t nb = len ? ceil_div(len, block_size) : 0;
    if (n_out) *n_out = nb;
    if (nb > cap) return SF_ENOSPC;
    if (nb == 0) return SF_OK;
    auto fill = [&](uint8_t* dst, uint64_t off, uint64_t scap, uint64_t* n, bool* eof) {
      *n = std::min(scap, len - off);
      *eof = off + *n >= len;
      memcpy(dst, data + off, *n);
      return SF_OK;
    };
    auto emit = [&](uint64_t first, uint64_t nbk, const uint8_t* dg, uint64_t bytes) {
      write_rows(out + first, first, nbk, dg, bytes, block_size);
      return SF_OK;
    };
    return staged_pipeline(block_size, std::min(file_stage_bytes(block_size), nb * block_size), fill, emit, nullptr);
  });
}

int sf_index_file(const char* path, uint32_t block_size, sf_block_sig* out, uint64_t cap, uint64_t* n_out,
                  uint8_t blocks_hash[20]) {
  return guarded([&] {
    int rc = check_block_size(block_size);
    if (rc) return rc;
    if (!path) return SF_EINVAL;
    const Fd f{open(path, O_RDONLY)};
    if (f.fd < 0) return SF_EIO;
    struct stat sb;
    if (fstat(f.fd, &sb) != 0 || S_ISDIR(sb.st_mode)) return SF_EIO;
    if (!S_ISREG(sb.st_mode)) {
      // Not seekable (FIFO, socket, character device): the sequential route.
      // The input is consumed, so with too small a cap the rows are lost and
      // SF_ENOSPC reports the need (sf_index_fd has no cap to miss).
      RowBuf rows;
      uint8_t bh[20];
      rc = index_stream(f.fd, block_size, rows, bh);
      if (rc != SF_OK) return rc;
      if (n_out) *n_out = rows.n;
      if (rows.n > cap) return SF_ENOSPC;
      if (rows.n && !out) return SF_EINVAL;
      if (rows.n) memcpy(out, rows.p, rows.n * sizeof(sf_block_sig));
      if (blocks_hash) memcpy(blocks_hash, bh, 20);
      return SF_OK;
    }
    const off_t end = lseek(f.fd, 0, SEEK_END);
    if (end < 0) return SF_EIO;
    // The file is only ever read (pread into the pinned stages), never mapped
    // and page-locked: a registered file mapping is a GPU userptr, and a
    // concurrent truncation of the file invalidates it under the in-flight
    // copies -- measured on MI355X, the process's queues then never resumed
    // (DESIGN.md 6).  A file that shrinks mid-call gives SF_EIO, like the short
    // read the reference would see.
    return index_regular(f.fd, (uint64_t)end, block_size, out, cap, n_out, blocks_hash);
  });
}

int sf_index_file_range(const char* path, uint64_t start, uint64_t len, uint32_t block_size, sf_block_sig* out,
                        uint64_t cap, uint64_t* n_out) {
  return guarded([&] {
    if (const int rc = check_block_size(block_size)) return rc;
    if (!path || (len && start % block_size)) return SF_EINVAL;  // an empty shard may start anywhere up to EOF
    const uint64_t nb = len ? ceil_div(len, block_size) : 0;
    if (n_out) *n_out = nb;
    if (nb > cap) return SF_ENOSPC;
    if (nb && !out) return SF_EINVAL;
    const Fd f{open(path, O_RDONLY)};
    if (f.fd < 0) return SF_EIO;
    struct stat sb;
    if (fstat(f.fd, &sb) != 0 || !S_ISREG(sb.st_mode)) return SF_EIO;
    if (start > (uint64_t)sb.st_size || len > (uint64_t)sb.st_size - start) return SF_ERANGE;
    return nb ? index_file_pread(f.fd, start, len, block_size, out, nullptr) : SF_OK;
  });
}

int sf_index_fd(int fd, uint32_t block_size, sf_block_sig** rows, uint64_t* n_out, uint8_t blocks_hash[20]) {
  return guarded([&] {
    if (rows) *rows = nullptr;
    if (n_out) *n_out = 0;
    int rc = check_block_size(block_size);
    if (rc) return rc;
    if (fd < 0 || !rows || !n_out) return SF_EINVAL;
    RowBuf rb;
    rc = index_stream(fd, block_size, rb, blocks_hash);
    if (rc != SF_OK) return rc;
    *n_out = rb.n;
    *rows = rb.release();
    return SF_OK;
  });
}

void sf_free_rows(sf_block_sig* rows) { free(rows); }

int sf_sha1_host(const uint8_t* data, uint64_t len, uint8_t out[20]) {
  if (!out || (len && !data)) return SF_EINVAL;
  sf_host_sha1_impl(data, len, out, 0);
  return SF_OK;
}

int sf_blocks_hash(const uint8_t* digests, uint64_t n, uint8_t out[20]) {
  if (!out || (n && !digests)) return SF_EINVAL;
  sf_host_sha1_impl(digests, n * 20, out, 0);
  return SF_OK;
}

int sf_blocks_hash_sigs(const sf_block_sig* sigs, uint64_t n, uint8_t out[20]) {
  return guarded([&] {
    if (!out || (n && !sigs)) return SF_EINVAL;
    // The digests gathered into contiguous runs (AoS rows are 32 B apart), a
    // fixed buffer at a time, streamed through one SHA-1.
    uint8_t buf[20 * 3276];
    sf_host_sha1_stream h;
    sf_host_sha1_begin(&h);
    for (uint64_t i = 0; i < n;) {
      const uint64_t m = std::min<uint64_t>(n - i, sizeof(buf) / 20);
      for (uint64_t j = 0; j < m; j++) memcpy(buf + 20 * j, sigs[i + j].sha1, 20);
      sf_host_sha1_update(&h, buf, m * 20);
      i += m;
    }
    sf_host_sha1_final(&h, out);
    return SF_OK;
  });
}

}  // extern "C"
