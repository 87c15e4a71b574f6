// sf_fds_zpaq.cpp -- sf_index_fds_zpaq (include/syncfast_amd.h): the
// reference's default mode over many files with NO host chunker and every
// file read ONCE.
//
// sf_index_fds_blocks (sf_fds.cpp) takes lists the caller's chunker made by
// streaming every file on a host thread, then reads every file again for the
// device.  Here the files are read with pread by the reader threads into
// packed pinned stages (each file at a 64-byte boundary of its stage), and per
// stage: one H2D copy, one many-file device cut (sf_cdc_files.hip), one
// explicit-list launch over every block of the stage, one D2H of list,
// first_row and digests.
//
// The pipeline (two_stage, sf_stage.hpp).  The cut synchronises its stream once
// per join launch, so it is split over the two halves of a stage:
//   issue(k)    read stage k, stamp its files again, H2D, round 0 of the cut
//               (zpaq_files_begin: asynchronous, and the largest share of the
//               cut);
//   harvest(k)  the join launches and the count (zpaq_files_finish: blocking),
//               emit, the explicit-list launch, D2H; the files that did not
//               settle under max_rounds are cut by the host cutter from the
//               stage's pinned bytes (one file per reader thread), their lists
//               uploaded and hashed by a second explicit-list launch over the
//               same stage in HBM; then the stage's rows and blocks_hash
//               values.
// two_stage runs issue(k + 1) before harvest(k): stage k's H2D and round 0 run
// on the device while the host reads stage k + 1, and stage k's joins, hash and
// rows run while stage k + 1's H2D and round 0 do.
//
// A file larger than a stage is a stage sequence of its own, through
// fd_zpaq_windows (sf_cdc.hip: the window carry of sf_index_fd_zpaq), in its
// place in the file order: the pipeline of the files before it is drained
// first.  HIP runtime API only: built with the host compiler.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <vector>

#include "host_sha1.h"
#include "sf_launch.hpp"
#include "sf_stage.hpp"

using namespace sfi;

namespace {

constexpr uint64_t kFileAlign = 64;

struct Placed {
  uint32_t f;
  uint64_t dst, len;  // where in the stage, how many bytes
};

struct Stage {
  std::vector<Placed> files;
  uint64_t bytes = 0;
};

// A file that did not settle, cut on the host from the pinned stage.
struct HostCut {
  uint32_t j;  // index in the stage's files
  std::vector<uint64_t> off;
  std::vector<uint32_t> size;
  int rc = SF_OK;
};

int host_cut(const uint8_t* data, uint64_t len, uint32_t bits, uint32_t max_size, HostCut* c) {
  uint64_t need = (len >> (bits > 1 ? bits - 1 : 0)) + len / max_size + 16;
  for (int pass = 0; pass < 2; pass++) {
    c->off.resize(need);
    c->size.resize(need);
    const uint64_t cap = need;
    const int rc = sf_zpaq_cut_buffer(data, len, bits, max_size, c->off.data(), c->size.data(), cap, &need);
    if (rc == SF_OK) {
      c->off.resize(need);
      c->size.resize(need);
      return SF_OK;
    }
    if (rc != SF_ENOSPC) return rc;
  }
  return SF_EIO;
}

struct PhaseMs {
  double check = 0, read = 0, issue = 0, cut = 0, hash = 0, host = 0, rows = 0, large = 0;
};

struct Call {
  const int* fds;
  const sf_file_stamp* stamps;
  uint32_t n_files, bits, max_size, max_rounds;
  uint64_t target;
  std::unique_ptr<std::atomic<int>[]> status;
  std::vector<sf_file_stamp> before;
  RowBuf rb;
  uint64_t* first_row;
  uint8_t* blocks_hashes;
  Trace tr;
  PhaseMs ms;
  uint64_t stage_no = 0;                                                  // read_hook's argument
  uint64_t st_L = 0, st_seg = 0, st_launch = 0, st_recut = 0, st_unsettled = 0, st_host = 0;  // the hook's statistics
  uint64_t n_stages = 0;
  explicit Call(bool trace) : tr(trace) {}
};

void set_status(Call& c, uint32_t f, int from, int to) { c.status[f].compare_exchange_strong(from, to); }

// The small files [f0, f1) that passed the check, as one pipeline.  Appends
// their rows in file order and sets first_row[f] for every f in [f0, f1).
int run_group(Call& c, uint32_t f0, uint32_t f1) {
  std::vector<Stage> stages(1);
  for (uint32_t f = f0; f < f1; f++) {
    const uint64_t len = c.before[f].size;
    if (c.status[f].load(std::memory_order_relaxed) != SF_OK || len == 0) continue;
    Stage* st = &stages.back();
    uint64_t dst = (st->bytes + kFileAlign - 1) & ~(kFileAlign - 1);
    if (!st->files.empty() && dst + len > c.target) {
      stages.emplace_back();
      st = &stages.back();
      dst = 0;
    }
    st->files.push_back({f, dst, len});
    st->bytes = dst + len;
  }
  if (stages.back().files.empty()) stages.pop_back();
  uint32_t next_file = f0;  // first_row is filled up to here
  auto rows_up_to = [&](uint32_t f) {
    for (; next_file < f; next_file++) c.first_row[next_file] = c.rb.n;
  };
  if (stages.empty()) {
    rows_up_to(f1);
    return SF_OK;
  }
  uint64_t max_bytes = 16;
  for (const Stage& s : stages) max_bytes = std::max(max_bytes, s.bytes);

  HostLease res;
  hipStream_t* st;
  hipEvent_t* done;
  StageBufs sb[2];
  ZpaqFilesPlan plan[2];
  bool active[2] = {false, false};
  uint64_t have_blocks[2] = {0, 0}, have_aux[2] = {0, 0};
  int rc = res.streams(st, done);
  for (int i = 0; i < 2 && rc == SF_OK; i++) rc = stage_bufs(res, i, max_bytes, kNoBuf, kNoBuf, &sb[i]);
  if (rc != SF_OK) return rc;
  // a plan in flight holds scratch and a host array the stream may still read
  struct Drain {
    ZpaqFilesPlan* plan;
    bool* active;
    hipStream_t* st;
    ~Drain() {
      for (int b = 0; b < 2; b++) {
        if (!active[b]) continue;
        (void)hipStreamSynchronize(st[b]);
        zpaq_files_free(&plan[b], st[b]);
      }
    }
  } drain{plan, active, st};

  auto issue = [&](uint64_t k, int b) {
    const Stage& s = stages[k];
    constexpr uint64_t kSlice = 16ull << 20;
    struct Item { uint32_t j; uint64_t a, e; };
    std::vector<Item> items;
    for (uint32_t j = 0; j < s.files.size(); j++)
      for (uint64_t a = 0; a < s.files[j].len; a += kSlice) items.push_back({j, a, std::min(s.files[j].len, a + kSlice)});
    uint8_t* pin = static_cast<uint8_t*>(sb[b].pin);
    std::atomic<size_t> next{0};
    run_pool(pool_threads(items.size()), [&] {
      for (size_t i; (i = next.fetch_add(1)) < items.size();) {
        const Item& it = items[i];
        const Placed& p = s.files[it.j];
        // an error, or EOF before the size in the stamp (the file shrank)
        if (!read_fully(c.fds[p.f], pin + p.dst + it.a, it.a, it.e - it.a)) set_status(c, p.f, SF_OK, SF_EIO);
      }
    });
    read_hook(c.stage_no++);
    // every file of the stage is whole in it: its stamp again (a short read,
    // or a full one, of a file whose stamp moved is SF_EAGAIN)
    std::vector<uint64_t> offs(s.files.size()), lens(s.files.size());
    bool any = false;
    for (size_t j = 0; j < s.files.size(); j++) {
      const Placed& p = s.files[j];
      sf_file_stamp after{};
      if (!stamp_of(c.fds[p.f], &after, nullptr)) c.status[p.f].store(SF_EIO);
      else if (!same_stamp(c.before[p.f], after)) c.status[p.f].store(SF_EAGAIN);
      offs[j] = p.dst;
      lens[j] = c.status[p.f].load(std::memory_order_relaxed) == SF_OK ? p.len : 0;  // a failed file is not cut
      any |= lens[j] != 0;
    }
    c.tr.lap(c.ms.read);
    active[b] = false;
    if (any) {
      if (hipMemcpyAsync(sb[b].ddata, pin, s.bytes, hipMemcpyHostToDevice, st[b]) != hipSuccess) return SF_ENODEV;
      plan[b] = ZpaqFilesPlan{};
      active[b] = true;
      const int r = zpaq_files_begin(static_cast<const uint8_t*>(sb[b].ddata), offs.data(), lens.data(),
                                     (uint32_t)s.files.size(), c.bits, c.max_size, st[b], &plan[b]);
      if (r != SF_OK) return r;
    }
    c.tr.lap(c.ms.issue);
    return SF_OK;
  };

  auto harvest = [&](uint64_t k, int b) {
    const Stage& s = stages[k];
    const size_t nf = s.files.size();
    c.tr.lap(c.ms.issue);
    if (!active[b]) {  // every file of the stage failed
      rows_up_to(s.files.back().f + 1);
      return SF_OK;
    }
    ZpaqFilesPlan& p = plan[b];
    int r = zpaq_files_finish(&p, c.max_rounds, st[b]);
    c.tr.lap(c.ms.cut);
    if (r != SF_OK) return r;
    c.st_L = p.L;
    c.st_seg += p.nseg;
    c.st_launch += p.launches;
    c.st_recut += p.recut;
    c.st_unsettled += p.n_unsettled;
    // the list, first_row and the digests: aux = offsets[n], first_row[nf + 1], sizes[n]
    const uint64_t n = p.total, aux = n * kListEntry + (nf + 1) * 8;
    if (n > have_blocks[b] || aux > have_aux[b]) {
      have_blocks[b] = std::max(n, 2 * have_blocks[b]);
      have_aux[b] = have_blocks[b] * kListEntry + (nf + 1) * 8;
      if ((r = stage_bufs(res, b, kNoBuf, have_blocks[b], have_aux[b], &sb[b])) != SF_OK) return r;
    }
    uint64_t* d_off = static_cast<uint64_t*>(sb[b].daux);
    uint64_t* d_first = d_off + n;
    uint32_t* d_sz = reinterpret_cast<uint32_t*>(d_first + nf + 1);
    if ((r = zpaq_files_emit(p, d_off, d_sz, d_first, st[b])) != SF_OK) return r;
    if (n && (r = launch_table(sb[b].ddata, s.bytes, d_off, d_sz, n, sb[b].ddig, nullptr, st[b])) != SF_OK) return r;
    if (hipMemcpyAsync(sb[b].paux, sb[b].daux, aux, hipMemcpyDeviceToHost, st[b]) != hipSuccess ||
        (n && hipMemcpyAsync(sb[b].pdig, sb[b].ddig, n * 20, hipMemcpyDeviceToHost, st[b]) != hipSuccess))
      return SF_ENODEV;
    // the files that did not settle, meanwhile: the host cutter over the pinned stage
    std::vector<HostCut> cuts;
    for (uint32_t j = 0; j < nf; j++)
      if (p.unsettled[j]) {
        cuts.emplace_back();
        cuts.back().j = j;
      }
    const uint8_t* pin = static_cast<const uint8_t*>(sb[b].pin);
    if (!cuts.empty()) {
      std::atomic<size_t> next{0};
      run_pool(pool_threads(cuts.size()), [&] {
        for (size_t i; (i = next.fetch_add(1)) < cuts.size();) {
          const Placed& pl = s.files[cuts[i].j];
          cuts[i].rc = host_cut(pin + pl.dst, pl.len, c.bits, c.max_size, &cuts[i]);
        }
      });
    }
    uint64_t extra = 0;
    for (const HostCut& hc : cuts) {
      if (hc.rc != SF_OK) return hc.rc;
      extra += hc.off.size();
    }
    std::vector<uint8_t> xlist(extra * kListEntry), xdig(extra * 20);
    Scratch xd(st[b]);
    if (extra) {
      uint64_t* lo = reinterpret_cast<uint64_t*>(xlist.data());
      uint32_t* lz = reinterpret_cast<uint32_t*>(lo + extra);
      uint64_t at = 0;
      for (const HostCut& hc : cuts)
        for (size_t i = 0; i < hc.off.size(); i++, at++) {
          lo[at] = s.files[hc.j].dst + hc.off[i];
          lz[at] = hc.size[i];
        }
      if ((r = stream_alloc(&xd.p, extra * (kListEntry + 20), st[b])) != SF_OK) return r;
      uint8_t* xl = static_cast<uint8_t*>(xd.p);
      uint8_t* xg = xl + extra * kListEntry;  // 4-byte aligned: kListEntry is 12
      if (hipMemcpyAsync(xl, xlist.data(), xlist.size(), hipMemcpyHostToDevice, st[b]) != hipSuccess) return SF_ENODEV;
      r = launch_table(sb[b].ddata, s.bytes, reinterpret_cast<const uint64_t*>(xl),
                       reinterpret_cast<const uint32_t*>(xl + extra * 8), extra, xg, nullptr, st[b]);
      if (r != SF_OK) return r;
      if (hipMemcpyAsync(xdig.data(), xg, extra * 20, hipMemcpyDeviceToHost, st[b]) != hipSuccess) return SF_ENODEV;
    }
    c.tr.lap(c.ms.host);
    if (hipStreamSynchronize(st[b]) != hipSuccess) return SF_ENODEV;
    c.tr.lap(c.ms.hash);
    c.st_host += cuts.size();
    zpaq_files_free(&p, st[b]);
    active[b] = false;

    // rows and blocks_hash, file by file
    const uint64_t* lo = static_cast<const uint64_t*>(sb[b].paux);
    const uint64_t* first = lo + n;
    const uint32_t* lz = reinterpret_cast<const uint32_t*>(first + nf + 1);
    const uint8_t* dg = static_cast<const uint8_t*>(sb[b].pdig);
    if (!c.rb.grow(c.rb.n + n + extra + 1)) return SF_ENOMEM;
    size_t xc = 0;
    uint64_t xat = 0;
    for (uint32_t j = 0; j < nf; j++) {
      const Placed& pl = s.files[j];
      rows_up_to(pl.f + 1);  // first_row[pl.f] = the rows so far; files skipped before it have none
      if (c.status[pl.f].load(std::memory_order_relaxed) != SF_OK) continue;
      sf_block_sig* o = c.rb.p + c.rb.n;
      uint8_t* bh = c.blocks_hashes + 20ull * pl.f;
      if (p.unsettled[j]) {
        const HostCut& hc = cuts[xc++];
        const uint64_t m = hc.off.size();
        for (uint64_t i = 0; i < m; i++) {
          o[i].offset = hc.off[i];
          o[i].size = hc.size[i];
          memcpy(o[i].sha1, xdig.data() + 20 * (xat + i), 20);
        }
        sf_host_sha1_impl(xdig.data() + 20 * xat, m * 20, bh, 0);
        xat += m;
        c.rb.n += m;
        continue;
      }
      const uint64_t r0 = first[j], m = first[j + 1] - r0;
      for (uint64_t i = 0; i < m; i++) {
        o[i].offset = lo[r0 + i] - pl.dst;
        o[i].size = lz[r0 + i];
        memcpy(o[i].sha1, dg + 20 * (r0 + i), 20);
      }
      sf_host_sha1_impl(dg + 20 * r0, m * 20, bh, 0);
      c.rb.n += m;
    }
    c.tr.lap(c.ms.rows);
    return SF_OK;
  };

  c.n_stages += stages.size();
  rc = two_stage(stages.size(), issue, harvest);
  if (rc == SF_OK) rows_up_to(f1);
  return rc;
}

int index_fds_zpaq_body(const int* fds, const sf_file_stamp* stamps, uint32_t n_files, uint32_t bits, uint32_t max_size,
                        uint32_t max_rounds, uint64_t stage_bytes, sf_block_sig** rows, uint64_t* n_out,
                        uint64_t* first_row, uint8_t* blocks_hashes, int* file_status, uint32_t* bad_file) {
  if (rows) *rows = nullptr;
  if (n_out) *n_out = 0;
  if (bad_file) *bad_file = 0;
  if (!rows || !n_out || zpaq_check_device_params(bits, max_size) != SF_OK) return SF_EINVAL;
  if (n_files && (!fds || !first_row || !blocks_hashes)) return SF_EINVAL;
  Call c(knob(K_TRACE) != 0);
  c.fds = fds;
  c.stamps = stamps;
  c.n_files = n_files;
  c.bits = bits;
  c.max_size = max_size;
  c.max_rounds = max_rounds;
  c.target = stage_bytes ? std::max<uint64_t>((stage_bytes + kFileAlign - 1) & ~(kFileAlign - 1), 2ull * max_size)
                         : (256ull << 20);
  c.first_row = first_row;
  c.blocks_hashes = blocks_hashes;
  if (first_row) first_row[0] = 0;

  // 1. each file's stamp, against the caller's: on the reader threads, 256
  // files per work item.  A file that fails here is not read.
  c.status.reset(new std::atomic<int>[std::max<uint32_t>(n_files, 1)]);
  c.before.resize(n_files);
  {
    constexpr uint32_t kChunk = 256;
    const uint32_t nchunks = (uint32_t)ceil_div(n_files, kChunk);
    std::atomic<uint32_t> next{0};
    run_pool(pool_threads(nchunks), [&] {
      for (uint32_t ch; (ch = next.fetch_add(1)) < nchunks;)
        for (uint32_t f = ch * kChunk; f < std::min<uint32_t>(n_files, (ch + 1) * kChunk); f++) {
          int rc = SF_OK;
          mode_t mode = 0;
          if (fds[f] < 0) rc = SF_EINVAL;
          else if (!stamp_of(fds[f], &c.before[f], &mode)) rc = SF_EIO;
          else if (!S_ISREG(mode)) rc = SF_EINVAL;
          else if (stamps && !same_stamp(c.before[f], stamps[f])) rc = SF_EAGAIN;
          c.status[f].store(rc, std::memory_order_relaxed);
        }
    });
  }
  c.tr.lap(c.ms.check);

  // 2. runs of files that fit a stage as pipelines; a larger file alone, in
  // its place
  int rc = SF_OK;
  uint32_t g0 = 0;
  for (uint32_t f = 0; f <= n_files && rc == SF_OK; f++) {
    const bool large = f < n_files && c.status[f].load(std::memory_order_relaxed) == SF_OK && c.before[f].size > c.target;
    if (f < n_files && !large) continue;
    rc = run_group(c, g0, f);
    g0 = f + 1;
    if (rc != SF_OK || f == n_files) break;
    c.tr.lap(c.ms.rows);
    first_row[f] = c.rb.n;
    const uint64_t n0 = c.rb.n;
    sf_host_sha1_stream bh;
    sf_host_sha1_begin(&bh);
    const int r = stamped(fds[f], &c.before[f], [&](const sf_file_stamp& before, mode_t) {
      return fd_zpaq_windows(fds[f], before.size, bits, max_size, c.rb, &bh);
    });
    if (r == SF_OK) {
      sf_host_sha1_final(&bh, blocks_hashes + 20ull * f);
    } else if (r == SF_EAGAIN || r == SF_EIO) {  // this file's alone
      c.status[f].store(r);
      c.rb.n = n0;
    } else {
      rc = r;
    }
    c.tr.lap(c.ms.large);
  }
  if (rc != SF_OK) return rc;  // a device error: no file's rows are valid
  if (n_files) first_row[n_files] = c.rb.n;

  // Files with no blocks: SHA-1("").  A file that failed: its blocks_hash
  // zeroed, no rows.  The call's result is the first failing file's.
  int first_bad = -1;
  for (uint32_t f = 0; f < n_files; f++) {
    const int s = c.status[f].load(std::memory_order_relaxed);
    if (file_status) file_status[f] = s;
    if (s != SF_OK) {
      memset(blocks_hashes + 20ull * f, 0, 20);
      if (first_bad < 0) first_bad = (int)f;
    } else if (c.before[f].size == 0) {
      sf_host_sha1_impl(reinterpret_cast<const uint8_t*>(""), 0, blocks_hashes + 20ull * f, 0);
    }
  }
  const uint64_t stats[6] = {c.st_L ? c.st_L : zpaq_segment_len(max_size), c.st_seg, c.st_launch, c.st_recut,
                             c.st_unsettled, c.st_host};
  for (int k = 0; k < 6; k++) zpaq_files_stat(k, stats[k]);
  if (c.tr.on) {
    const double tot = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c.tr.t0).count();
    fprintf(stderr,
            "sf_index_fds_zpaq trace: %u files, %llu blocks, %llu stages, %llu join launches, %llu on the host: "
            "check %.2f read %.2f h2d+round0 issue %.2f joins %.2f host cut %.2f hash+d2h wait %.2f rows %.2f large %.2f "
            "total %.2f ms\n",
            n_files, (unsigned long long)c.rb.n, (unsigned long long)c.n_stages, (unsigned long long)c.st_launch,
            (unsigned long long)c.st_host, c.ms.check, c.ms.read, c.ms.issue, c.ms.cut, c.ms.host, c.ms.hash, c.ms.rows,
            c.ms.large, tot);
  }
  if (!c.rb.grow(1)) return SF_ENOMEM;  // no rows: still a pointer that free() takes
  *n_out = c.rb.n;
  *rows = c.rb.release();
  if (first_bad >= 0) {
    if (bad_file) *bad_file = (uint32_t)first_bad;
    return c.status[first_bad].load();
  }
  return SF_OK;
}

}  // namespace

extern "C" {

int sf_index_fds_zpaq(const int* fds, const sf_file_stamp* stamps, uint32_t n_files, uint32_t bits, uint32_t max_size,
                      uint32_t max_rounds, uint64_t stage_bytes, sf_block_sig** rows, uint64_t* n_out,
                      uint64_t* first_row, uint8_t* blocks_hashes, int* file_status, uint32_t* bad_file) {
  return guarded([&] {
    return index_fds_zpaq_body(fds, stamps, n_files, bits, max_size, max_rounds, stage_bytes, rows, n_out, first_row,
                               blocks_hashes, file_status, bad_file);
  });
}

}  // extern "C"
