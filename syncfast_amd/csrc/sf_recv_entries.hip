// sf_recv_entries.hip -- the sink's FilesList state for one received buffer on
// the device (include/syncfast_amd.h: sf_receive_file_entries_device): the
// FILE_ENTRY messages of the source's files list parsed as the reference
// parser reads them (sf_wire_entries.hpp has the rules), every name looked up
// in the destination's name set and every announced blocks_hash compared with
// the recorded one (src/sync/fs.rs:378-446).  Its own translation unit: the
// other parsers and their code objects stay as they are.
//
// Names and hashes are arbitrary bytes, so entry i starts where entry i - 1
// ends, which is serial.  What is parallel:
//
//   candidates, scan   sf_recv_scan.hpp, shared with the other parsers: the
//               bitmap of every position where entry_message holds, and every
//               candidate's index in position order.
//   chain       one lane per word, for each of its candidates at p with length
//               L: the link is good when p + L is a candidate and none lies in
//               (p, p + L).  L reaches 149, so the window is three 64-bit reads
//               of the bitmap.  atomicMin keeps the first candidate whose link
//               is not good, with a bit that says whether a candidate lay
//               inside it.  END_FILES is no candidate: the chain ends before it
//               like before anything else, and the host reads it in the bytes
//               that stand at the chain's end.
//   extract     one lane per word: candidates below the first bad one are the
//               entries, and a candidate's index is its entry's.  Each writes
//               its name's span, its size and its hash, and lowers bad_name
//               when its name is no UTF-8; the last one writes E and the bytes
//               that stand there.
//   (read-back 1: counts, E, bad_name and those bytes)
//   lookup      sf_name_set_lookup over the spans just written.
//   need        one lane per entry: unknown name, no recorded hash, or another
//               hash.
//   scan, list  inclusive scan of the need bytes; one lane per needed entry
//               writes its index at its place.
//   (read-back 2: the number of needed entries; only with a set)
//
// With no candidate strictly inside [0, E) off the chain, the candidates in
// [0, E) ARE the chain and the reference reads exactly that prefix (the
// argument of DESIGN.md 3.13).  A candidate inside the last chained entry (a
// blocks_hash that spells an entry, possibly behind a name that ends in
// FILE_ENTRY) sends the whole buffer to parse_entries_run on the host.  Every
// dependency is a kernel boundary; no lane waits for another; every loop is
// bounded by an entry's 149 bytes or a word's 64 bits.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "sf_recv_scan.hpp"
#include "sf_wire_entries.hpp"
#include "../../include/syncfast_amd_test.h"

using namespace sfrs;

namespace {

constexpr uint64_t kMaxEntriesRun = 1ull << 35;  // bytes per call: fewer than 2^30 entries, a uint32 list

// What the host reads back, in one copy.
struct Result {
  unsigned long long first_bad;  // ((index of the prefix's last entry + 1) << 1) | (no candidate inside it)
  unsigned long long cand, msgs, end, bad_name;
  uint32_t tail_n, n_need;
  uint8_t tail[sfwp::kEntriesTail];  // the bytes at `end`
};
static_assert(offsetof(Result, first_bad) == 0 && sizeof(Result::first_bad) == 8 && sizeof(Result) <= 256,
              "sfrs::Scan::result: 256 bytes that begin with first_bad");

// Every entry begins "FILE_ENTRY\n".  'F' alone as the prefilter: a list is
// names, decimal sizes and 20 hash bytes per entry; the hash bytes hold an 'F'
// once in 256 and a path holds one now and then, so about one position in
// seven that passes is no entry.  A second byte would save those tests (each
// ends at its second or third byte) and cost every lane a second comparison
// of its 16 bytes.  Not measured.
struct EntryRules {
  static constexpr uint32_t kFirst = 'F', kSecond = 0;
  static __device__ __forceinline__ uint32_t message(const uint8_t* b, uint64_t avail, uint32_t* name_len,
                                                     uint64_t* size) {
    return sfwp::entry_message(b, avail, name_len, size);
  }
};

__global__ void __launch_bounds__(256) entries_chain_kernel(const uint8_t* __restrict__ data, uint64_t n,
                                                            const unsigned long long* __restrict__ words,
                                                            const uint64_t* __restrict__ ends, uint64_t nw,
                                                            Result* __restrict__ res) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nw) return;
  unsigned long long m = words[w];
  if (w == 0 && !(m & 1ull)) atomicMin(&res->first_bad, 1ull);  // nothing at byte 0: no entry
  uint64_t i = ends[w] - (uint64_t)__popcll(m);
  for (; m; m &= m - 1, i++) {
    const uint64_t p = (w << 6) + (uint64_t)(__ffsll((long long)m) - 1);
    uint32_t name_len;
    uint64_t size;
    const uint32_t L = sfwp::entry_message(data + p, n - p, &name_len, &size);  // 35..149: p is a candidate
    // positions p + 1 .. p + 64 in v[0], .. p + 128 in v[1], .. p + 192 in v[2]; L - 1 of them lie inside the entry
    const unsigned long long v0 = bits_from(words, nw, p + 1), v1 = bits_from(words, nw, p + 65),
                             v2 = bits_from(words, nw, p + 129);
    const uint32_t in = L - 1;  // 34..148
    bool inside = (v0 & low_bits(in > 64 ? 64 : in)) != 0;
    if (in > 64) inside |= (v1 & low_bits(in > 128 ? 64 : in - 64)) != 0;
    if (in > 128) inside |= (v2 & low_bits(in - 128)) != 0;
    const bool next = ((in < 64 ? v0 : in < 128 ? v1 : v2) >> (in & 63)) & 1ull;  // p + L
    if (inside || !next) atomicMin(&res->first_bad, ((unsigned long long)(i + 1) << 1) | (inside ? 0ull : 1ull));
  }
}

struct EntryOutputs {
  uint64_t* name_at;
  uint32_t* name_len;
  uint64_t* sizes;
  uint32_t* hashes;
  uint64_t cap;
};

__global__ void __launch_bounds__(256) entries_extract_kernel(const uint8_t* __restrict__ data, uint64_t n,
                                                              const unsigned long long* __restrict__ words,
                                                              const uint64_t* __restrict__ ends, uint64_t nw,
                                                              EntryOutputs o, Result* __restrict__ res) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nw) return;
  const uint64_t k = res->first_bad >> 1;  // the entries (written by the chain kernel, one launch earlier)
  if (w == 0) {
    res->cand = ends[nw - 1];
    res->msgs = k;
    if (k == 0) {  // nothing chained: what stands at byte 0
      const uint32_t tn = n < sfwp::kEntriesTail ? (uint32_t)n : sfwp::kEntriesTail;
      for (uint32_t j = 0; j < tn; j++) res->tail[j] = data[j];
      res->tail_n = tn;
    }
  }
  unsigned long long m = words[w];
  uint64_t i = ends[w] - (uint64_t)__popcll(m);
  for (; m && i < k; m &= m - 1, i++) {
    const uint64_t p = (w << 6) + (uint64_t)(__ffsll((long long)m) - 1);
    uint32_t name_len = 0;
    uint64_t size = 0;
    const uint32_t L = sfwp::entry_message(data + p, n - p, &name_len, &size);
    if (i < o.cap) {
      o.name_at[i] = p + sfwp::kEntryTag;
      o.name_len[i] = name_len;
      o.sizes[i] = size;
      store_digest(o.hashes + 5 * i, data + p + L - sfwp::kDigest - 1);
    }
    if (!sfwp::utf8_ok(data + p + sfwp::kEntryTag, name_len)) atomicMin(&res->bad_name, (unsigned long long)i);
    if (i == k - 1) {
      const uint64_t e = p + L;
      res->end = e;
      const uint32_t tn = n - e < sfwp::kEntriesTail ? (uint32_t)(n - e) : sfwp::kEntriesTail;
      for (uint32_t j = 0; j < tn; j++) res->tail[j] = data[e + j];
      res->tail_n = tn;
    }
  }
}

// need[i] = 1 when entry i's file has to be fetched: no row of its name, a row
// with no recorded hash, or a recorded hash that differs in any byte.
__global__ void __launch_bounds__(256) entries_need_kernel(const int64_t* __restrict__ rows,
                                                           const uint32_t* __restrict__ hashes,
                                                           const uint32_t* __restrict__ have,
                                                           const uint8_t* __restrict__ have_ok, uint64_t n,
                                                           uint8_t* __restrict__ need) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t r = rows[i];
  bool want = r < 0 || (have_ok && !have_ok[r]);
  if (!want) {
#pragma unroll
    for (int j = 0; j < 5; j++) want |= hashes[5 * i + j] != have[5 * r + j];
  }
  need[i] = want ? 1 : 0;
}

__global__ void __launch_bounds__(256) entries_list_kernel(const uint8_t* __restrict__ need,
                                                           const uint32_t* __restrict__ upto, uint64_t n,
                                                           uint32_t* __restrict__ list, Result* __restrict__ res) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (need[i]) list[upto[i] - 1] = (uint32_t)i;
  if (i == n - 1) res->n_need = upto[i];
}

sfi::Stats4 g_entries_stats;  // sf_test_file_entries_stats: route, candidates, chained entries, read-backs

}  // namespace

using namespace sfi;

namespace {

constexpr uint64_t kRouteDevice = 0, kRouteForcedHost = 1, kRouteFallback = 2;

struct EntriesArgs {
  const sf_name_set* set;
  const void* d_have_hashes;
  const uint8_t* d_have_hash_ok;
  uint64_t* d_name_at;
  uint32_t* d_name_len;
  uint64_t* d_sizes;
  void* d_hashes;
  int64_t* d_rows;
  uint8_t* d_need;
  uint32_t* d_need_list;
  uint64_t cap;
  uint64_t *n_out, *n_need, *bad_name, *consumed;
  int* stop;
};

// With a set, after the n (> 0) parsed rows are in the caller's arrays: rows,
// need and the list, and *n_need (one read-back).  res: 256 bytes of scratch
// whose n_need word this may write.
int lookup_and_need(const EntriesArgs& a, const uint8_t* d_wire, uint64_t n_bytes, uint64_t n, Result* res,
                    uint64_t* readbacks, hipStream_t s) {
  int rc = sf_name_set_lookup(a.set, d_wire, n_bytes, a.d_name_at, a.d_name_len, n, a.d_rows, s);
  if (rc != SF_OK) return rc;
  rc = launch(entries_need_kernel, grid256(n), dim3(256), s, a.d_rows, static_cast<const uint32_t*>(a.d_hashes),
              static_cast<const uint32_t*>(a.d_have_hashes), a.d_have_hash_ok, n, a.d_need);
  if (rc != SF_OK) return rc;
  size_t tmp = 0;
  if ((rc = scan_inclusive(nullptr, tmp, static_cast<uint8_t*>(nullptr), static_cast<uint32_t*>(nullptr), n, s)) !=
      SF_OK)
    return rc;
  ScratchLayout L;
  const size_t upto_at = L.add(n * 4);
  Scratch ws(s);
  if ((rc = stream_alloc(&ws.p, L.total() + tmp + 8, s)) != SF_OK) return rc;
  uint32_t* upto = L.at<uint32_t>(ws.p, upto_at);
  if ((rc = scan_inclusive(L.at<void>(ws.p, L.total()), tmp, a.d_need, upto, n, s)) != SF_OK) return rc;
  rc = launch(entries_list_kernel, grid256(n), dim3(256), s, a.d_need, upto, n, a.d_need_list, res);
  if (rc != SF_OK) return rc;
  uint32_t n_need = 0;
  SF_HIP(hipMemcpyAsync(&n_need, &res->n_need, 4, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  ++*readbacks;
  *a.n_need = n_need;
  return SF_OK;
}

// The serial parse on the host (the buffer is copied back) and the upload of
// what the device route would have written.  Blocking.
int entries_on_host(const EntriesArgs& a, const uint8_t* d_wire, uint64_t n, uint64_t cap, bool query,
                    uint64_t readbacks, hipStream_t s) {
  std::vector<uint8_t> wire(n);
  SF_HIP(hipMemcpyAsync(wire.data(), d_wire, n, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  readbacks++;
  sfwp::EntriesParsed r;
  sfwp::parse_entries_run(wire.data(), n, sfwp::EntriesOut{}, &r);  // the count
  std::vector<uint64_t> nat(r.count), sizes(r.count);
  std::vector<uint32_t> nlen(r.count);
  std::vector<uint8_t> hashes(r.count * 20);
  sfwp::parse_entries_run(wire.data(), n, sfwp::EntriesOut{nat.data(), nlen.data(), sizes.data(), hashes.data(), r.count},
                          &r);
  uint64_t bad = UINT64_MAX;
  for (uint64_t i = 0; i < r.count && bad == UINT64_MAX; i++)
    if (!sfwp::utf8_ok(wire.data() + nat[i], nlen[i])) bad = i;
  g_entries_stats.set(2, r.count);
  g_entries_stats.set(3, readbacks);
  *a.n_out = r.count;
  *a.bad_name = bad;
  *a.consumed = r.consumed;
  *a.stop = r.stop;
  if (query) return r.count ? SF_ENOSPC : SF_OK;
  const uint64_t up_n = std::min(r.count, cap);
  auto up = [&](void* dst, const void* src, uint64_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
  };
  SF_HIP(up(a.d_name_at, nat.data(), up_n * 8));
  SF_HIP(up(a.d_name_len, nlen.data(), up_n * 4));
  SF_HIP(up(a.d_sizes, sizes.data(), up_n * 8));
  SF_HIP(up(a.d_hashes, hashes.data(), up_n * 20));
  SF_HIP(hipStreamSynchronize(s));  // the vectors go out of scope
  if (r.count > cap) return SF_ENOSPC;
  if (a.set && r.count) {
    Scratch rs(s);
    int rc = stream_alloc(&rs.p, 256, s);
    if (rc != SF_OK) return rc;
    rc = lookup_and_need(a, d_wire, n, r.count, static_cast<Result*>(rs.p), &readbacks, s);
    g_entries_stats.set(3, readbacks);
    return rc;
  }
  return SF_OK;
}

// d_wire[0, n) (n > 0) on s.  Blocking.
int entries_device(const EntriesArgs& a, const uint8_t* d_wire, uint64_t n, hipStream_t s) {
  const bool query = !a.d_name_at || !a.d_name_len || !a.d_sizes || !a.d_hashes ||
                     (a.set && (!a.d_rows || !a.d_need || !a.d_need_list));
  const uint64_t cap = query ? 0 : a.cap;  // a query writes nothing
  if (knob(K_TEST_WIRE_PARSE_HOST) == 1) {
    g_entries_stats.set(0, kRouteForcedHost);
    return entries_on_host(a, d_wire, n, cap, query, 0, s);
  }
  Scan sc(s);
  int rc = scan_candidates<EntryRules>(d_wire, n, s, &sc);
  if (rc != SF_OK) return rc;
  Result* res = static_cast<Result*>(sc.result);
  SF_HIP(hipMemsetAsync(&res->bad_name, 0xFF, 8, s));
  const dim3 gw = grid256(sc.nw);
  rc = launch(entries_chain_kernel, gw, dim3(256), s, d_wire, n, sc.words, sc.ends, sc.nw, res);
  if (rc != SF_OK) return rc;
  const EntryOutputs o{a.d_name_at, a.d_name_len, a.d_sizes, static_cast<uint32_t*>(a.d_hashes), cap};
  rc = launch(entries_extract_kernel, gw, dim3(256), s, d_wire, n, sc.words, sc.ends, sc.nw, o, res);
  if (rc != SF_OK) return rc;
  Result h{};
  SF_HIP(hipMemcpyAsync(&h, res, sizeof(Result), hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  uint64_t readbacks = 1;
  g_entries_stats.set(1, h.cand);
  uint32_t len = 0, name_len = 0;
  uint64_t size = 0;
  const int c = sfwp::classify_entries(h.tail, h.tail_n, &len, &name_len, &size);
  // a candidate inside the last chained entry; or (never, by the rules) a whole entry at the chain's end
  if ((h.msgs && !(h.first_bad & 1ull)) || c == sfwp::kEntry) {
    g_entries_stats.set(0, kRouteFallback);
    return entries_on_host(a, d_wire, n, cap, query, readbacks, s);
  }
  g_entries_stats.set(0, kRouteDevice);
  g_entries_stats.set(2, h.msgs);
  g_entries_stats.set(3, readbacks);
  const uint64_t k = h.msgs;
  *a.n_out = k;
  *a.bad_name = h.bad_name;
  *a.consumed = (k ? h.end : 0) + (c == sfwp::kEndFiles ? sfwp::kEndFilesTag : 0);
  *a.stop = c;
  if (query) return k ? SF_ENOSPC : SF_OK;
  if (k > cap) return SF_ENOSPC;
  if (a.set && k) {
    rc = lookup_and_need(a, d_wire, n, k, res, &readbacks, s);
    g_entries_stats.set(3, readbacks);
    return rc;
  }
  return SF_OK;
}

int receive_entries(const EntriesArgs& a, const void* d_wire, uint64_t n_bytes, hipStream_t s) {
  g_entries_stats.reset();
  if (a.n_out) *a.n_out = 0;
  if (a.n_need) *a.n_need = 0;
  if (a.bad_name) *a.bad_name = UINT64_MAX;
  if (a.consumed) *a.consumed = 0;
  if (a.stop) *a.stop = SF_WIRE_END;
  if (!a.n_out || !a.n_need || !a.bad_name || !a.consumed || !a.stop || (n_bytes && !d_wire) ||
      n_bytes > kMaxEntriesRun)
    return SF_EINVAL;
  if (!a.set && (a.d_rows || a.d_need || a.d_need_list)) return SF_EINVAL;  // a parse only: no lookup output
  if (a.set && !a.d_have_hashes) return SF_EINVAL;
  // dword stores to the name lengths, hashes and the list, 8-B stores to the 64-bit lists, dword loads of the recorded hashes
  if (misaligned(a.d_name_at, 8) || misaligned(a.d_name_len, 4) || misaligned(a.d_sizes, 8) ||
      misaligned(a.d_hashes, 4) || misaligned(a.d_rows, 8) || misaligned(a.d_need_list, 4) ||
      misaligned(a.d_have_hashes, 4))
    return SF_EINVAL;
  if (n_bytes == 0) return SF_OK;
  return entries_device(a, static_cast<const uint8_t*>(d_wire), n_bytes, s);
}

}  // namespace

extern "C" {

int sf_receive_file_entries_device(const sf_name_set* set, const void* d_wire, uint64_t n_bytes,
                                   const void* d_have_hashes, const uint8_t* d_have_hash_ok, uint64_t* d_name_at,
                                   uint32_t* d_name_len, uint64_t* d_sizes, void* d_hashes, int64_t* d_rows,
                                   uint8_t* d_need, uint32_t* d_need_list, uint64_t cap, uint64_t* n_out,
                                   uint64_t* n_need, uint64_t* bad_name, uint64_t* consumed, int* stop, void* stream) {
  return guarded([&]() -> int {
    const EntriesArgs a{set,      d_have_hashes, d_have_hash_ok, d_name_at, d_name_len, d_sizes,
                        d_hashes, d_rows,        d_need,         d_need_list, cap,      n_out,
                        n_need,   bad_name,      consumed,       stop};
    return receive_entries(a, d_wire, n_bytes, as_stream(stream));
  });
}

int sf_test_file_entries_stats(uint64_t out[4]) { return g_entries_stats.read(out); }

}  // extern "C"
