// sf_recv_data.hip -- a received run of BLOCK_DATA messages on the device
// (include/syncfast_amd.h: sf_receive_block_data_device / _buffer): parsed as
// the reference parser reads it, every payload hashed in place and compared
// with the digest its message claims.  Beside sf_recv.hip, in its own
// translation unit: the other kernels' code objects stay as they are.
//
// A message is a header of H = 34 to 48 bytes (sf_wire_data.hpp has the
// rules), `size` payload bytes and a newline.  Unlike a FILE_BLOCK message
// its length is data-dependent and unbounded, and its payload is arbitrary
// file content: whole valid messages may lie inside it, and a header in it
// may announce a length that lands on a later message's end byte.  The steps,
// ordered by kernel boundaries only (no lane waits for another):
//
//   candidates, scan   sf_recv_scan.hpp, shared with sf_recv.hip: the bitmap
//               of every position where data_message holds, and every
//               candidate's index in position order.  The candidate total is
//               read back (the call blocks there).
//   compact     one lane per bitmap word writes pos[i] and len[i] (8 B each)
//               of its candidates, in position order.
//   link        one lane per candidate: i is good when pos[i + 1] == pos[i] +
//               len[i].  atomicMin keeps the first that is not, with a bit
//               that says whether pos[i + 1] lies below pos[i] + len[i]: a
//               candidate inside that message.  With the bit clear the
//               candidates [0, first_bad] are the messages: all before the
//               last end exactly where the next starts, so none lies inside
//               one, and nothing stands at the last one's end E (DESIGN.md
//               3.9, the argument of 3.8).
//   walk        with the bit set the chain may go on past candidates that are
//               payload bytes.  Only pos[] and len[] go back to the host
//               (16 B per candidate; no payload byte), walk_candidates chains
//               them from byte 0, and the chained indices (8 B each, at most
//               n / 35 + 1 of them) go up.
//   extract     one lane per message, through that index list if there is
//               one: the claimed digest as the block set's dwords, the size,
//               the payload's offset pos + H; from the last, E and the up to
//               48 bytes that stand there, which decide the stop class.
//   verify      the explicit-list kernel (launch_table) hashes the payloads
//               where they lie, d_data = d_wire; a compare kernel writes one
//               byte per message and counts the mismatches.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <memory>

#include "sf_launch.hpp"
#include "sf_recv_scan.hpp"
#include "sf_wire_data.hpp"
#include "../../include/syncfast_amd_test.h"

using namespace sfrs;

namespace {

// What the host reads back, in one copy.
struct Result {
  unsigned long long first_bad;  // (index of the first candidate whose link is not good << 1) | (a candidate inside it)
  unsigned long long end;        // E: the end of the last message
  uint32_t too_large, pad;       // a chained size above 2^32 - 1
  uint8_t tail[sfwp::kMaxMessage];  // the run's bytes from E on (to its end, if that comes first)
};

static_assert(offsetof(Result, first_bad) == 0 && sizeof(Result::first_bad) == 8 && sizeof(Result) <= 256,
              "sfrs::Scan::result: 256 bytes that begin with first_bad");

// Only a position that holds 'B' with 'L' after it (the sixteenth: 'B' alone,
// its neighbour is another lane's) is looked at further -- a payload of 'B's
// costs no more than any other.
struct DataRules {
  static constexpr uint32_t kFirst = 'B', kSecond = 'L';
  static __device__ __forceinline__ uint64_t message(const uint8_t* b, uint64_t avail, uint32_t* H, uint64_t* size) {
    return sfwp::data_message(b, avail, H, size);
  }
};

// One lane per bitmap word: position and length of its candidates, at their
// index in position order (ends: the inclusive scan of the counts).
__global__ void __launch_bounds__(256) data_compact_kernel(const uint8_t* __restrict__ data, uint64_t n,
                                                           const unsigned long long* __restrict__ words,
                                                           const uint64_t* __restrict__ ends, uint64_t nw,
                                                           uint64_t total, uint64_t* __restrict__ pos,
                                                           uint64_t* __restrict__ len) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nw) return;
  unsigned long long m = words[w];
  uint64_t i = ends[w] - (uint64_t)__popcll(m);
  for (; m && i < total; m &= m - 1, i++) {
    const uint64_t p = (w << 6) + (uint64_t)(__ffsll((long long)m) - 1);
    uint32_t H;
    uint64_t size;
    pos[i] = p;
    len[i] = sfwp::data_message(data + p, n - p, &H, &size);
  }
}

// One lane per candidate: the first whose successor does not start where it
// ends (total > 0; candidate 0 not at byte 0: no message at all).
__global__ void __launch_bounds__(256) data_link_kernel(const uint64_t* __restrict__ pos,
                                                        const uint64_t* __restrict__ len, uint64_t total,
                                                        Result* __restrict__ res) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const uint64_t end = pos[i] + len[i];
  const bool last = i + 1 == total;
  const uint64_t next = last ? 0 : pos[i + 1];
  if (last || next != end)
    atomicMin(&res->first_bad, ((unsigned long long)i << 1) | (!last && next < end ? 1ull : 0ull));
}

// One lane per message k < count (count > 0): candidate chain[k] (k itself
// without a chain).  The header's length is read again from the size field,
// whose validity made the position a candidate.
__global__ void __launch_bounds__(256) data_extract_kernel(const uint8_t* __restrict__ data, uint64_t n,
                                                           const uint64_t* __restrict__ pos,
                                                           const uint64_t* __restrict__ len,
                                                           const uint64_t* __restrict__ chain, uint64_t count,
                                                           uint32_t* __restrict__ digests, uint32_t* __restrict__ sizes,
                                                           uint64_t* __restrict__ offsets, uint64_t cap,
                                                           Result* __restrict__ res) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const uint64_t c = chain ? chain[k] : k;
  const uint64_t p = pos[c], L = len[c];
  uint64_t size;
  const uint32_t H = sfwp::kSizeAt + sfwp::size_field(data + p + sfwp::kSizeAt, n - p - sfwp::kSizeAt, &size);
  if (k == count - 1) {  // the last message: E, and what stands there for the stop class
    const uint64_t E = p + L;
    res->end = E;
    for (uint32_t j = 0; j < sfwp::kMaxMessage && E + j < n; j++) res->tail[j] = data[E + j];
  }
  if (size > 0xFFFFFFFFull) atomicOr(&res->too_large, 1u);
  if (k >= cap) return;
  store_digest(digests + 5 * k, data + p + sfwp::kTag);
  sizes[k] = (uint32_t)size;
  offsets[k] = p + H;
}

// ok[k] = the payload's SHA-1 is the digest its message claims.  An empty
// payload verifies against SHA-1 of the empty string whatever the list
// kernel wrote for it.
__global__ void __launch_bounds__(256) data_compare_kernel(const uint32_t* __restrict__ claimed,
                                                           const uint32_t* __restrict__ computed,
                                                           const uint32_t* __restrict__ sizes, uint64_t count,
                                                           uint8_t* __restrict__ ok,
                                                           unsigned long long* __restrict__ bad) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  // da39a3ee 5e6b4b0d 3255bfef 95601890 afd80709, as little-endian dwords of its bytes
  const uint32_t empty[5] = {0xeea339dau, 0x0d4b6b5eu, 0xefbf5532u, 0x90186095u, 0x0907d8afu};
  const bool e = sizes[k] == 0;
  bool same = true;
#pragma unroll
  for (int j = 0; j < 5; j++) same &= claimed[5 * k + j] == (e ? empty[j] : computed[5 * k + j]);
  ok[k] = same ? 1 : 0;
  if (!same) atomicAdd(bad, 1ull);
}

sfi::Stats4 g_data_stats;  // sf_test_block_data_stats

}  // namespace

using namespace sfi;

namespace {

struct Outputs {
  void* d_digests = nullptr;
  uint32_t* d_sizes = nullptr;
  uint64_t* d_offsets = nullptr;
  uint8_t* d_ok = nullptr;  // NULL: parse only
  uint64_t cap = 0;
};
// Where `count` messages go: asked once they are counted, so the buffer
// route's device rows are sized by the messages, not by the run.
using Provide = std::function<int(uint64_t count, Outputs* o)>;

struct Parsed {
  uint64_t count = 0, consumed = 0, need = 0, bad = 0;
  int stop = sfwp::kEnd;
};

// Hash the first `count` payloads where they lie and compare; *bad = the
// mismatches.  Blocking.
int verify(const uint8_t* d_wire, uint64_t n, const Outputs& o, uint64_t count, uint64_t* bad, hipStream_t s) {
  Scratch comp(s);  // the mismatch counter, then the computed digests
  ScratchLayout L;
  const size_t bad_at = L.add(8);
  int rc = stream_alloc(&comp.p, L.total() + count * 20, s);
  if (rc != SF_OK) return rc;
  unsigned long long* d_bad = L.at<unsigned long long>(comp.p, bad_at);
  uint32_t* computed = L.at<uint32_t>(comp.p, L.total());
  SF_HIP(hipMemsetAsync(d_bad, 0, sizeof(*d_bad), s));
  rc = launch_table(d_wire, n, o.d_offsets, o.d_sizes, count, computed, nullptr, s);
  if (rc == SF_OK)
    rc = launch(data_compare_kernel, grid256(count), dim3(256), s, static_cast<const uint32_t*>(o.d_digests), computed,
                o.d_sizes, count, o.d_ok, d_bad);
  if (rc != SF_OK) return rc;
  unsigned long long h = 0;
  SF_HIP(hipMemcpyAsync(&h, d_bad, sizeof(h), hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  *bad = h;
  return SF_OK;
}

// What stands at E, from the first min(avail, 48) bytes there (avail: the
// bytes from E to the end of the run).  The end byte of a whole header whose
// message fits in the run is not read: with '\n' there, E would be a candidate
// and chained, so it is a wrong end byte.
void classify_tail(const uint8_t* tail, uint64_t avail, Parsed* out) {
  uint32_t H;
  uint64_t size;
  const int c = sfwp::data_header(tail, avail, &H, &size);
  out->stop = c;
  if (c != sfwp::kData) return;
  const uint64_t total = (uint64_t)H + size + 1;
  if (total > avail) {
    out->stop = sfwp::kIncomplete;
    out->need = total;
  } else {
    out->stop = sfwp::kMalformed;  // "Invalid data end byte"
  }
}

// The serial parse of the caller's own bytes (the buffer route with
// SF_TEST_BLOCK_DATA_WALK = 2) and the upload of its first min(count, cap)
// entries.
int parse_on_host(const uint8_t* h_wire, uint64_t n, const Provide& provide, Outputs* o, Parsed* out, hipStream_t s,
                  HostLease* lease) {
  bool too_large = false;
  sfwp::parse_data_run(h_wire, n, nullptr, nullptr, nullptr, 0, &out->count, &out->consumed, &out->stop, &out->need,
                       &too_large);  // the count first: it sizes the outputs
  g_data_stats.set(1, out->count);
  if (too_large) return SF_ERANGE;
  int rc = provide(out->count, o);
  if (rc != SF_OK) return rc;
  const uint64_t up = std::min(out->count, o->cap);
  if (up == 0) return SF_OK;
  void *pdig = nullptr, *paux = nullptr;
  if ((rc = lease->pin(kSlotDigests + 1, up * 20, &pdig)) != SF_OK) return rc;
  if ((rc = lease->pin(kSlotAux + 1, up * 12, &paux)) != SF_OK) return rc;
  uint64_t* po = static_cast<uint64_t*>(paux);
  uint32_t* pz = reinterpret_cast<uint32_t*>(po + up);
  Parsed again;
  sfwp::parse_data_run(h_wire, n, static_cast<uint8_t*>(pdig), pz, po, up, &again.count, &again.consumed, &again.stop,
                       &again.need, &too_large);
  SF_HIP(hipMemcpyAsync(o->d_digests, pdig, up * 20, hipMemcpyHostToDevice, s));
  SF_HIP(hipMemcpyAsync(o->d_sizes, pz, up * 4, hipMemcpyHostToDevice, s));
  SF_HIP(hipMemcpyAsync(o->d_offsets, po, up * 8, hipMemcpyHostToDevice, s));
  SF_HIP(hipStreamSynchronize(s));  // the pinned stages go back to the cache
  return SF_OK;
}

int find_messages(const uint8_t* d_wire, const uint8_t* h_wire, uint64_t n, const Provide& provide, Outputs* o,
                  Parsed* out, hipStream_t s, HostLease* lease);

// The messages of d_wire[0, n) (n > 0): found, counted, the first
// min(count, cap) written to the outputs `provide` names for that count, and
// with d_ok every payload verified; the result into *out.  Blocking.
int parse_run_device(const uint8_t* d_wire, const uint8_t* h_wire, uint64_t n, const Provide& provide, Outputs* o,
                     Parsed* out, hipStream_t s, HostLease* lease) {
  const int rc = knob(K_TEST_BLOCK_DATA_WALK) == 2 && h_wire && lease
                     ? parse_on_host(h_wire, n, provide, o, out, s, lease)
                     : find_messages(d_wire, h_wire, n, provide, o, out, s, lease);
  if (rc != SF_OK) return rc;
  if (o->d_ok && out->count && out->count <= o->cap) return verify(d_wire, n, *o, out->count, &out->bad, s);
  return SF_OK;
}

// The device parse: candidates, scan, compact, link, (walk,) extract, stop.
int find_messages(const uint8_t* d_wire, const uint8_t* h_wire, uint64_t n, const Provide& provide, Outputs* o,
                  Parsed* out, hipStream_t s, HostLease* lease) {
  const int64_t force = knob(K_TEST_BLOCK_DATA_WALK);
  Scan sc(s);
  int rc = scan_candidates<DataRules>(d_wire, n, s, &sc);
  if (rc != SF_OK) return rc;
  Result* res = static_cast<Result*>(sc.result);
  uint64_t total = 0;
  SF_HIP(hipMemcpyAsync(&total, sc.ends + sc.nw - 1, 8, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  g_data_stats.set(0, total);
  if (total > n / sfwp::kTag + 1) return SF_EIO;  // cannot be: two candidates' tags do not overlap

  uint64_t count = 0;
  Result r{};
  Scratch list(s), idx(s);
  if (total) {
    if ((rc = stream_alloc(&list.p, total * 16, s)) != SF_OK) return rc;
    uint64_t* pos = static_cast<uint64_t*>(list.p);
    uint64_t* len = pos + total;
    rc = launch(data_compact_kernel, grid256(sc.nw), dim3(256), s, d_wire, n, sc.words, sc.ends, sc.nw, total, pos,
                len);
    if (rc == SF_OK) rc = launch(data_link_kernel, grid256(total), dim3(256), s, pos, len, total, res);
    if (rc != SF_OK) return rc;
    struct {
      unsigned long long first_bad;
      uint64_t pos0;
    } h{};
    SF_HIP(hipMemcpyAsync(&h.first_bad, &res->first_bad, 8, hipMemcpyDeviceToHost, s));
    SF_HIP(hipMemcpyAsync(&h.pos0, pos, 8, hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    const uint64_t* chain = nullptr;
    if (h.pos0 != 0) {
      count = 0;  // nothing stands at byte 0
    } else if (!(h.first_bad & 1ull) && force == 0) {
      count = (h.first_bad >> 1) + 1;  // candidates [0, first_bad] are the messages
    } else {
      // a candidate lies inside a chained message: the exact chain, on the
      // host, over the candidate list alone
      std::unique_ptr<HostLease> own;
      if (!lease) {
        own.reset(new HostLease);
        lease = own.get();
      }
      void *plist = nullptr, *pchain = nullptr;
      if ((rc = lease->pin(kSlotDigests + 1, total * 16, &plist)) != SF_OK) return rc;
      if ((rc = lease->pin(kSlotAux + 1, total * 8, &pchain)) != SF_OK) return rc;
      SF_HIP(hipMemcpyAsync(plist, list.p, total * 16, hipMemcpyDeviceToHost, s));
      SF_HIP(hipStreamSynchronize(s));
      const uint64_t* hp = static_cast<const uint64_t*>(plist);
      count = sfwp::walk_candidates(hp, hp + total, total, static_cast<uint64_t*>(pchain));
      g_data_stats.set(2, 1);
      g_data_stats.set(3, total * 16);
      if (count) {
        if ((rc = stream_alloc(&idx.p, count * 8, s)) != SF_OK) return rc;
        SF_HIP(hipMemcpyAsync(idx.p, pchain, count * 8, hipMemcpyHostToDevice, s));
        SF_HIP(hipStreamSynchronize(s));  // the pinned stages go back to the cache
        chain = static_cast<const uint64_t*>(idx.p);
      }
    }
    if ((rc = provide(count, o)) != SF_OK) return rc;
    if (count) {
      rc = launch(data_extract_kernel, grid256(count), dim3(256), s, d_wire, n, pos, len, chain, count,
                  static_cast<uint32_t*>(o->d_digests), o->d_sizes, o->d_offsets, o->cap, res);
      if (rc != SF_OK) return rc;
      SF_HIP(hipMemcpyAsync(&r, res, sizeof(Result), hipMemcpyDeviceToHost, s));
      SF_HIP(hipStreamSynchronize(s));
      if (r.too_large) return SF_ERANGE;
    }
  } else if ((rc = provide(0, o)) != SF_OK) {
    return rc;
  }
  g_data_stats.set(1, count);
  out->count = count;
  out->consumed = count ? r.end : 0;
  // what stands at E: after a message the extract kernel brought its bytes
  // along; with no message E is byte 0
  const uint64_t avail = n - out->consumed;
  if (count == 0) {
    const uint64_t tn = std::min<uint64_t>(avail, sizeof(r.tail));
    if (h_wire) {
      memcpy(r.tail, h_wire, tn);
    } else {
      SF_HIP(hipMemcpyAsync(r.tail, d_wire, tn, hipMemcpyDeviceToHost, s));
      SF_HIP(hipStreamSynchronize(s));
    }
  }
  classify_tail(r.tail, avail, out);
  return SF_OK;
}

struct Results {
  uint64_t *n_out, *consumed;
  int* stop;
  uint64_t *need, *n_bad;
};

int check_args(const Results& r, const void* wire, uint64_t n_bytes) {
  g_data_stats.reset();
  if (r.n_out) *r.n_out = 0;
  if (r.consumed) *r.consumed = 0;
  if (r.stop) *r.stop = SF_WIRE_END;
  if (r.need) *r.need = 0;
  if (r.n_bad) *r.n_bad = 0;
  if (!r.n_out || !r.consumed || !r.stop || !r.need || !r.n_bad || (n_bytes && !wire) || n_bytes > kMaxRun)
    return SF_EINVAL;
  return SF_OK;
}

int report(const Results& r, const Parsed& p, uint64_t cap) {
  *r.n_out = p.count;
  *r.consumed = p.consumed;
  *r.stop = p.stop;
  *r.need = p.need;
  *r.n_bad = p.bad;
  return p.count > cap ? SF_ENOSPC : SF_OK;
}

int receive_buffer(const uint8_t* wire, uint64_t n_bytes, sf_block_sig* out, uint8_t* ok, uint64_t cap,
                   const Results& r) {
  int rc = check_args(r, wire, n_bytes);
  if (rc != SF_OK || n_bytes == 0) return rc;
  if (!out) cap = 0;
  HostLease res;
  hipStream_t* st;
  hipEvent_t* ev;
  if ((rc = res.streams(st, ev)) != SF_OK) return rc;
  hipStream_t s = st[0];
  const uint8_t* d_wire = nullptr;
  if ((rc = upload_run(res, wire, n_bytes, s, ev, &d_wire)) != SF_OK) return rc;
  // device rows for the messages once they are counted (none when the
  // caller has no room for them: SF_ENOSPC): offsets, sizes, ok bytes
  void *ddig = nullptr, *daux = nullptr;
  const Provide provide = [&](uint64_t count, Outputs* o) -> int {
    if (count == 0 || count > cap) return SF_OK;
    int prc = res.dev(kSlotDigests, count * 20, &ddig);
    if (prc == SF_OK) prc = res.dev(kSlotAux, count * 13, &daux);
    if (prc != SF_OK) return prc;
    o->d_digests = ddig;
    o->d_offsets = static_cast<uint64_t*>(daux);
    o->d_sizes = reinterpret_cast<uint32_t*>(o->d_offsets + count);
    if (ok) o->d_ok = reinterpret_cast<uint8_t*>(o->d_sizes + count);
    o->cap = count;
    return SF_OK;
  };
  Outputs o;
  Parsed p;
  rc = parse_run_device(d_wire, wire, n_bytes, provide, &o, &p, s, &res);
  if (rc != SF_OK) return rc;
  if ((rc = report(r, p, cap)) != SF_OK) return rc;
  const uint64_t n = p.count;
  if (n == 0) return SF_OK;
  void *pdig = nullptr, *paux = nullptr;
  if ((rc = res.pin(kSlotDigests, n * 20, &pdig)) != SF_OK) return rc;
  if ((rc = res.pin(kSlotAux, n * 13, &paux)) != SF_OK) return rc;
  SF_HIP(hipMemcpyAsync(pdig, ddig, n * 20, hipMemcpyDeviceToHost, s));
  SF_HIP(hipMemcpyAsync(paux, daux, n * (ok ? 13 : 12), hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  const uint64_t* po = static_cast<const uint64_t*>(paux);
  const uint32_t* pz = reinterpret_cast<const uint32_t*>(po + n);
  for (uint64_t i = 0; i < n; i++) {
    out[i].offset = po[i];
    out[i].size = pz[i];
    memcpy(out[i].sha1, static_cast<const uint8_t*>(pdig) + 20 * i, 20);
  }
  if (ok) memcpy(ok, pz + n, n);
  return SF_OK;
}

}  // namespace

extern "C" {

int sf_receive_block_data_device(const void* d_wire, uint64_t n_bytes, void* d_digests, uint32_t* d_sizes,
                                 uint64_t* d_data_offsets, uint8_t* d_ok, uint64_t cap, uint64_t* n_out,
                                 uint64_t* consumed, int* stop, uint64_t* need, uint64_t* n_bad, void* stream) {
  return guarded([&]() -> int {
    const Results r{n_out, consumed, stop, need, n_bad};
    const int rc = check_args(r, d_wire, n_bytes);
    if (rc != SF_OK) return rc;
    // dword stores to the digests and sizes, 8-B stores to the offsets; d_ok is bytes
    if (misaligned(d_digests, 4) || misaligned(d_sizes, 4) || misaligned(d_data_offsets, 8)) return SF_EINVAL;
    if (n_bytes == 0) return SF_OK;
    if (!d_digests || !d_sizes || !d_data_offsets) cap = 0;  // a query
    const Provide provide = [&](uint64_t, Outputs* o) -> int {  // the caller's, whatever the count
      o->d_digests = d_digests;
      o->d_sizes = d_sizes;
      o->d_offsets = d_data_offsets;
      o->d_ok = d_ok;
      o->cap = cap;
      return SF_OK;
    };
    Outputs o;
    Parsed p;
    const int prc = parse_run_device(static_cast<const uint8_t*>(d_wire), nullptr, n_bytes, provide, &o, &p,
                                     as_stream(stream), nullptr);
    if (prc != SF_OK) return prc;
    return report(r, p, cap);
  });
}

int sf_receive_block_data_buffer(const void* wire, uint64_t n_bytes, sf_block_sig* out, uint8_t* ok, uint64_t cap,
                                 uint64_t* n_out, uint64_t* consumed, int* stop, uint64_t* need, uint64_t* n_bad) {
  return guarded([&] {
    return receive_buffer(static_cast<const uint8_t*>(wire), n_bytes, out, ok, cap,
                          Results{n_out, consumed, stop, need, n_bad});
  });
}

int sf_test_block_data_stats(uint64_t out[4]) { return g_data_stats.read(out); }

}  // extern "C"
