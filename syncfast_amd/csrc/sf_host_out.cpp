// sf_host_out.cpp -- the C-ABI's device-to-descriptor writers
// (include/syncfast_amd.h): FILE_BLOCK runs built on the device, device bytes
// and built BLOCK_DATA runs, each brought back through two pinned buffers and
// written to the caller's descriptor while the next buffer is on the link;
// and the way back, a descriptor's bytes read into HBM through the same buffers.
// HIP runtime API only: built with the host compiler.
#include <errno.h>
#include <unistd.h>

#include <algorithm>
#include <vector>

#include "sf_launch.hpp"
#include "sf_stage.hpp"

using namespace sfi;

namespace {

#ifndef SF_WIRE_CHUNK_DEFAULT
#define SF_WIRE_CHUNK_DEFAULT (1ull << 18)
#endif
// Messages per chunk of a FILE_BLOCK run: 2^18 (~9.4 MB at 4 KiB blocks);
// SF_TEST_WIRE_CHUNK is a test's small ones.
inline uint64_t wire_chunk() {
  const int64_t wc = knob(K_TEST_WIRE_CHUNK);
  return wc > 0 ? (uint64_t)wc : SF_WIRE_CHUNK_DEFAULT;
}

// Bytes per stage of `len` device bytes on their way to a descriptor: 64 MiB;
// SF_TEST_STREAM_STAGE_MIB is a test's small ones.
inline uint64_t out_stage_bytes(uint64_t len) {
  const int64_t sm = knob(K_TEST_STREAM_STAGE_MIB);
  return std::min<uint64_t>(len, sm > 0 ? (uint64_t)sm << 20 : (64ull << 20));
}

// An event of the call's own, destroyed on every path out.
struct CallEvent {
  hipEvent_t e = nullptr;
  ~CallEvent() { if (e) (void)hipEventDestroy(e); }
};

// What a writer holds for the length of its call, and its host end.  Streams,
// events and the two buffer sets come from the per-device set the other host
// entry points keep between calls: pinning two buffers per call cost more
// than the call's copies.  Buffer b's bytes come back into its pinned buffer
// (copy_back, behind the work of stream b that made them) and are written to
// fd, in order, once they are there (flush).
struct WireOut {
  int fd;
  CallEvent ready;  // before the lease: its release waits for the streams first
  HostLease res;
  hipStream_t* st = nullptr;
  hipEvent_t* ev = nullptr;
  StageBufs sb[2];
  uint64_t bytes_of[2] = {0, 0}, written = 0;
  explicit WireOut(int fd_) : fd(fd_) {}
  // Two pinned buffers of `bytes`, with device buffers beside them if `dev`.
  int open(uint64_t bytes, bool dev) {
    int rc = res.streams(st, ev);
    for (int i = 0; i < 2 && rc == SF_OK; i++)
      rc = dev ? stage_bufs(res, i, bytes, kNoBuf, kNoBuf, &sb[i]) : res.pin(kSlotData + i, bytes, &sb[i].pin);
    return rc;
  }
  // Both streams wait for what the caller's stream holds now: the bytes or
  // digests the call reads are produced there.
  int follow(hipStream_t caller) {
    SF_HIP(hipEventCreateWithFlags(&ready.e, hipEventDisableTiming));
    SF_HIP(hipEventRecord(ready.e, caller));
    for (int i = 0; i < 2; i++) SF_HIP(hipStreamWaitEvent(st[i], ready.e, 0));
    return SF_OK;
  }
  int copy_back(int b) {
    SF_HIP(hipMemcpyAsync(sb[b].pin, sb[b].ddata, bytes_of[b], hipMemcpyDeviceToHost, st[b]));
    SF_HIP(hipEventRecord(ev[b], st[b]));
    return SF_OK;
  }
  int flush(int b) {
    SF_HIP(hipEventSynchronize(ev[b]));
    const uint8_t* p = static_cast<const uint8_t*>(sb[b].pin);
    for (uint64_t done = 0; done < bytes_of[b];) {
      const ssize_t w = write(fd, p + done, bytes_of[b] - done);
      if (w < 0 && errno == EINTR) continue;
      if (w <= 0) return SF_EIO;
      done += (uint64_t)w;
      written += (uint64_t)w;
    }
    return SF_OK;
  }
  // The pipeline: stage k is issued while the host writes stage k-2; then,
  // whatever came of it, both streams are waited for (the caller may free
  // what they read) and the bytes known written are reported.
  template <typename Issue, typename Harvest>
  int run(uint64_t n_stages, uint64_t* n_written, Issue&& issue, Harvest&& harvest) {
    const int rc = two_stage(n_stages, issue, harvest);
    for (int i = 0; i < 2; i++) (void)hipStreamSynchronize(st[i]);
    if (n_written) *n_written = written;
    return rc;
  }
  // Stage k of `stage` bytes out of the `len` at d: where copy_back finds it.
  void stage_of(const uint8_t* d, uint64_t len, uint64_t stage, uint64_t k, int b) {
    sb[b].ddata = const_cast<uint8_t*>(d) + k * stage;
    bytes_of[b] = std::min(stage, len - k * stage);
  }
};

}  // namespace

extern "C" {

int sf_wire_file_blocks_fd(const void* d_digests, uint64_t n_blocks, uint32_t block_size, uint64_t file_len, int fd,
                           uint64_t* n_written, void* stream) {
  return guarded([&] {
    if (n_written) *n_written = 0;
    if (block_size == 0 || block_size > SF_MAX_BLOCK_SIZE) return SF_EINVAL;
    const uint64_t nb = file_len ? ceil_div(file_len, block_size) : 0;
    if (nb != n_blocks) return SF_EINVAL;
    if (!nb) return SF_OK;
    if (!d_digests || fd < 0) return SF_EINVAL;
    uint64_t db = 1;
    for (uint64_t v = block_size; v >= 10; v /= 10) db++;
    const uint32_t last = (uint32_t)(file_len - (nb - 1) * block_size);
    uint64_t dl = 1;
    for (uint64_t v = last; v >= 10; v /= 10) dl++;
    const uint64_t msg = 33 + db;  // every message but the last
    const uint64_t per = wire_chunk();
    WireOut w(fd);
    int rc = w.open(std::min(per, nb) * msg + (33 + dl), true);
    if (rc == SF_OK) rc = w.follow(as_stream(stream));
    if (rc != SF_OK) return rc;
    // chunk k: device builds its messages, D2H into its pinned buffer; the host
    // writes chunk k-2 while the device works on chunk k.
    return w.run(
        ceil_div(nb, per), n_written,
        [&](uint64_t k, int b) {
          const uint64_t i0 = k * per, n = std::min(per, nb - i0);
          const bool final_chunk = i0 + n == nb;
          const uint32_t lsz = final_chunk ? last : block_size;
          w.bytes_of[b] = (n - 1) * msg + (final_chunk ? 33 + dl : msg);
          if (launch_wire(static_cast<const uint8_t*>(d_digests) + i0 * 20, n, block_size, lsz,
                          static_cast<uint8_t*>(w.sb[b].ddata), w.st[b]) != SF_OK)
            return SF_ENODEV;
          return w.copy_back(b);
        },
        [&](uint64_t, int b) { return w.flush(b); });
  });
}

// The FILE_BLOCK run of an explicit list streamed to fd: chunks of
// SF_TEST_WIRE_CHUNK messages (default 2^18).  The whole run is planned once
// (message lengths, one scan, every chunk's end offset read back in one copy:
// the only wait before the chunks), then chunk k is built on the device and
// copied back while the host writes chunk k-2 -- no per-chunk host stall.
int sf_wire_blocks_fd(const void* d_digests, const uint32_t* d_sizes, uint64_t n_blocks, int fd, uint64_t* n_written,
                      void* stream) {
  return guarded([&] {
    if (n_written) *n_written = 0;
    if (n_blocks == 0) return SF_OK;
    if (!d_digests || !d_sizes || fd < 0) return SF_EINVAL;
    const uint64_t per = wire_chunk();
    const uint64_t nchunks = ceil_div(n_blocks, per);
    hipStream_t cs = as_stream(stream);  // digests and sizes are produced on the caller's stream
    uint64_t* ends = nullptr;
    int rc = wire_plan(d_sizes, n_blocks, &ends, cs);
    if (rc != SF_OK) return rc;
    struct FreeEnds {
      uint64_t* p;
      hipStream_t s;
      ~FreeEnds() { stream_free(p, s); }
    } free_ends{ends, cs};
    std::vector<uint64_t> cend(nchunks);
    uint64_t* d_cend = nullptr;
    if ((rc = stream_alloc(reinterpret_cast<void**>(&d_cend), nchunks * 8, cs)) != SF_OK) return rc;
    if ((rc = wire_chunk_ends(ends, n_blocks, per, d_cend, cs)) == SF_OK &&
        (rc = hip_err(hipMemcpyAsync(cend.data(), d_cend, nchunks * 8, hipMemcpyDeviceToHost, cs))) == SF_OK)
      rc = hip_err(hipStreamSynchronize(cs));
    stream_free(d_cend, cs);
    if (rc != SF_OK) return rc;
    uint64_t cap = 1;
    for (uint64_t k = 0; k < nchunks; k++) cap = std::max(cap, cend[k] - (k ? cend[k - 1] : 0));
    WireOut w(fd);  // after free_ends: both streams are waited for before the plan is freed on cs
    if ((rc = w.open(cap, true)) != SF_OK) return rc;  // (the plan is complete: cs was synchronised above)
    return w.run(
        nchunks, n_written,
        [&](uint64_t k, int b) {
          const uint64_t i0 = k * per, cnt = std::min(per, n_blocks - i0), base = k ? cend[k - 1] : 0;
          w.bytes_of[b] = cend[k] - base;
          const int r = wire_build(static_cast<const uint8_t*>(d_digests), d_sizes, ends, i0, cnt, base,
                                   static_cast<uint8_t*>(w.sb[b].ddata), w.st[b]);
          return r != SF_OK ? r : w.copy_back(b);
        },
        [&](uint64_t, int b) { return w.flush(b); });
  });
}

// d_data[0, len) to bytes [file_offset, + len) of fd: stage k comes back by
// DMA into its pinned buffer while stage k-2 is written with pwrite, in slices
// on the pool threads (one thread does not keep up with the link).  Stages are
// 64 MiB (SF_TEST_STREAM_STAGE_MIB: a test's small ones); *n_written counts
// whole stages known written.
int sf_write_device_fd(const void* d_data, uint64_t len, int fd, uint64_t file_offset, uint64_t* n_written,
                       void* stream) {
  return guarded([&] {
    if (n_written) *n_written = 0;
    if (fd < 0) return SF_EINVAL;
    if (lseek(fd, 0, SEEK_CUR) == (off_t)-1 && errno == ESPIPE) return SF_EINVAL;  // pwrite would refuse it too
    if (len == 0) return SF_OK;
    if (!d_data) return SF_EINVAL;
    const uint64_t stage = out_stage_bytes(len);
    WireOut w(fd);
    int rc = w.open(stage, false);
    if (rc == SF_OK) rc = w.follow(as_stream(stream));
    if (rc != SF_OK) return rc;
    return w.run(
        ceil_div(len, stage), n_written,
        [&](uint64_t k, int b) {
          w.stage_of(static_cast<const uint8_t*>(d_data), len, stage, k, b);
          return w.copy_back(b);
        },
        [&](uint64_t k, int b) {
          SF_HIP(hipEventSynchronize(w.ev[b]));
          const uint64_t o = file_offset + k * stage, m = w.bytes_of[b];
          const uint8_t* p = static_cast<const uint8_t*>(w.sb[b].pin);
          const int r = sliced(m, [&](uint64_t a, uint64_t e) {
            return write_fully(fd, p + a, o + a, e - a) ? SF_OK : SF_EIO;
          });
          if (r == SF_OK) w.written += m;
          return r;
        });
  });
}

// The other direction, the loader of the destination's local files: bytes
// [file_offset, + len) of fd to d_dst[0, len).  Stage k is read with pread, in
// slices on the pool threads, into pinned buffer k & 1 and copied from there
// on the caller's own stream, while stage k-1's copy is on the link; buffer
// k & 1 is read into again once the copy of stage k-2 is known done.  The
// whole read lies between two stamps of the file (stamped).  *n_read counts
// whole stages known copied.
int sf_read_fd_device(int fd, const sf_file_stamp* expect, uint64_t file_offset, uint64_t len, void* d_dst,
                      uint64_t* n_read, void* stream) {
  return guarded([&] {
    if (n_read) *n_read = 0;
    if (fd < 0) return SF_EINVAL;
    if (lseek(fd, 0, SEEK_CUR) == (off_t)-1 && errno == ESPIPE) return SF_EINVAL;  // pread would refuse it too
    if (len && !d_dst) return SF_EINVAL;
    return stamped(fd, expect, [&](const sf_file_stamp&, mode_t) {
      if (len == 0) return SF_OK;
      const uint64_t stage = out_stage_bytes(len);
      hipStream_t cs = as_stream(stream);
      WireOut w(fd);
      int rc = w.open(stage, false);
      if (rc != SF_OK) return rc;
      rc = two_stage(
          ceil_div(len, stage),
          [&](uint64_t k, int b) {
            const uint64_t m = std::min(stage, len - k * stage);
            w.bytes_of[b] = m;
            const int r = read_sliced(fd, static_cast<uint8_t*>(w.sb[b].pin), file_offset + k * stage, m);
            if (r != SF_OK) return r;
            SF_HIP(hipMemcpyAsync(static_cast<uint8_t*>(d_dst) + k * stage, w.sb[b].pin, m, hipMemcpyHostToDevice,
                                  cs));
            SF_HIP(hipEventRecord(w.ev[b], cs));
            return SF_OK;
          },
          [&](uint64_t, int b) {
            SF_HIP(hipEventSynchronize(w.ev[b]));
            w.written += w.bytes_of[b];
            return SF_OK;
          });
      (void)hipStreamSynchronize(cs);  // whatever came of it: no copy still reads a pinned buffer
      if (n_read) *n_read = w.written;
      return rc;
    });
  });
}

// A built BLOCK_DATA run (sf_send.hip) written to fd with write(), in order: a
// pipe works.  Stage k comes back by DMA into its pinned buffer, behind the
// run's last kernel, while stage k-2 is written.  Stages are 64 MiB
// (SF_TEST_STREAM_STAGE_MIB: a test's small ones).
int sf_wire_run_to_fd(const sf_wire_run* run, int fd, uint64_t* n_written) {
  return guarded([&] {
    if (n_written) *n_written = 0;
    if (!run || fd < 0) return SF_EINVAL;
    if (run->n_bytes == 0) return SF_OK;
    int cur = 0;
    SF_HIP(hipGetDevice(&cur));
    struct Device {
      int back;
      ~Device() { if (back >= 0) (void)hipSetDevice(back); }
    } restore{cur != run->device ? cur : -1};
    if (cur != run->device) SF_HIP(hipSetDevice(run->device));
    const uint64_t stage = out_stage_bytes(run->n_bytes);
    WireOut w(fd);
    if (const int rc = w.open(stage, false)) return rc;
    for (int i = 0; i < 2; i++) SF_HIP(hipStreamWaitEvent(w.st[i], run->done, 0));
    return w.run(
        ceil_div(run->n_bytes, stage), n_written,
        [&](uint64_t k, int b) {
          w.stage_of(run->bytes, run->n_bytes, stage, k, b);
          return w.copy_back(b);
        },
        [&](uint64_t, int b) { return w.flush(b); });
  });
}

}  // extern "C"
