// sf_recv.hip -- the receiving side of a FILE_BLOCK run on the device
// (include/syncfast_amd.h: sf_wire_parse_blocks_device, sf_receive_blocks_device,
// sf_receive_blocks_buffer): the inverse of sf_wire.hip.  Its own translation
// unit: the other kernels' code objects stay as they are.
//
// A message is "FILE_BLOCK\n" + 20 raw digest bytes + "\n" + a size field of
// 1 to 15 bytes + "\n" (34 to 48 bytes; sf_wire_parse.hpp has the rules).
// Digests are arbitrary bytes, so a message start cannot be told from a digest
// that happens to hold the same bytes: message i starts where message i - 1
// ends, which is serial.  What is parallel:
//
//   candidates, scan   sf_recv_scan.hpp, shared with sf_recv_data.hip: the
//               bitmap of every position where block_message holds, and every
//               candidate's index in position order.
//   chain       one lane per word, for each of its candidates at p with
//               length L: the link is good when p + L is a candidate and no
//               candidate lies in (p, p + L).  The first candidate whose link
//               is not good is the last message of the prefix that chains
//               from byte 0 (atomicMin on its index + 1, with a bit that says
//               whether a candidate lay inside it); candidate 0 not at byte 0
//               is an empty prefix.
//   extract     one lane per word again: candidates below that index are the
//               messages; lane writes digest, size and, for the last one, the
//               end offset E.
//
// With no candidate strictly inside [0, E) off the chain, the candidates in
// [0, E) ARE the chain, E is not a candidate, and the reference parser --
// which reads message after message from byte 0 -- reads exactly that prefix
// and stops at E.  A candidate inside the last chained message (the only
// place one can hide: the chain check stops at the first) means a digest
// forged a message start; then the call parses the run on the host, serially
// and exactly (parse_run).  Every dependency is a kernel boundary; no lane
// waits for another; every loop is bounded by a message's 48 bytes or a
// word's 64 bits.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <memory>

#include <rocprim/iterator/transform_iterator.hpp>

#include "sf_recv_scan.hpp"
#include "sf_wire_parse.hpp"
#include "../../include/syncfast_amd_test.h"

using namespace sfrs;

namespace {

// What the host reads back, in one copy.
struct Result {
  unsigned long long first_bad;  // ((index of the prefix's last message + 1) << 1) | (no candidate inside it)
  unsigned long long cand, msgs, end;
  uint32_t too_large, pad;
};
static_assert(offsetof(Result, first_bad) == 0 && sizeof(Result::first_bad) == 8 && sizeof(Result) <= 256,
              "sfrs::Scan::result: 256 bytes that begin with first_bad");

// Only a position that holds 'F' is looked at further: most lanes have one (a
// message is about 37 bytes).
struct BlockRules {
  static constexpr uint32_t kFirst = 'F', kSecond = 0;
  static __device__ __forceinline__ uint32_t message(const uint8_t* b, uint64_t avail, uint32_t*, uint64_t* size) {
    return sfwp::block_message(b, avail, size);
  }
};

// The length (34..48) and size of the message at candidate position p: the
// tag and the digest's newline were checked when p became a candidate.
__device__ __forceinline__ uint32_t message_len(const uint8_t* __restrict__ data, uint64_t n, uint64_t p,
                                                uint64_t* size) {
  return sfwp::kSizeAt + sfwp::size_field(data + p + sfwp::kSizeAt, n - p - sfwp::kSizeAt, size);
}

__global__ void __launch_bounds__(256) recv_chain_kernel(const uint8_t* __restrict__ data, uint64_t n,
                                                         const unsigned long long* __restrict__ words,
                                                         const uint64_t* __restrict__ ends, uint64_t nw,
                                                         Result* __restrict__ res) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nw) return;
  unsigned long long m = words[w];
  if (w == 0 && !(m & 1ull)) atomicMin(&res->first_bad, 1ull);  // nothing at byte 0: no message
  uint64_t i = ends[w] - (uint64_t)__popcll(m);
  for (; m; m &= m - 1, i++) {
    const uint64_t p = (w << 6) + (uint64_t)(__ffsll((long long)m) - 1);
    uint64_t size;
    const uint32_t L = message_len(data, n, p, &size);
    const unsigned long long v = bits_from(words, nw, p + 1);        // positions p + 1 ...
    const bool inside = (v & ((1ull << (L - 1)) - 1)) != 0;          // ... to p + L - 1
    const bool next = (v >> (L - 1)) & 1ull;                         // p + L
    if (inside || !next) atomicMin(&res->first_bad, ((unsigned long long)(i + 1) << 1) | (inside ? 0ull : 1ull));
  }
}

__global__ void __launch_bounds__(256) recv_extract_kernel(const uint8_t* __restrict__ data, uint64_t n,
                                                           const unsigned long long* __restrict__ words,
                                                           const uint64_t* __restrict__ ends, uint64_t nw,
                                                           uint32_t* __restrict__ digests, uint32_t* __restrict__ sizes,
                                                           uint64_t cap, Result* __restrict__ res) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nw) return;
  const uint64_t k = res->first_bad >> 1;  // the messages (written by the chain kernel, a launch earlier)
  if (w == 0) {
    res->cand = ends[nw - 1];
    res->msgs = k;
  }
  unsigned long long m = words[w];
  uint64_t i = ends[w] - (uint64_t)__popcll(m);
  for (; m && i < k; m &= m - 1, i++) {
    const uint64_t p = (w << 6) + (uint64_t)(__ffsll((long long)m) - 1);
    uint64_t size;
    const uint32_t L = message_len(data, n, p, &size);
    if (i == k - 1) res->end = p + L;
    if (size > 0xFFFFFFFFull) atomicOr(&res->too_large, 1u);
    if (i >= cap) continue;
    store_digest(digests + 5 * i, data + p + sfwp::kTag);
    sizes[i] = (uint32_t)size;
  }
}

sfi::Stats4 g_parse_stats;  // sf_test_wire_parse_stats

}  // namespace

using namespace sfi;

namespace {

struct Parsed {
  uint64_t count = 0, consumed = 0;
  int stop = sfwp::kEnd;
};

// The serial parse on the host and the upload of its first min(count, cap)
// entries.  h_wire: the run in host memory if the caller has it there, else
// it is copied back from d_wire through a pinned stage.
int parse_on_host(const uint8_t* d_wire, const uint8_t* h_wire, uint64_t n, uint8_t* d_digests, uint32_t* d_sizes,
                  uint64_t cap, Parsed* out, hipStream_t s, HostLease* lease) {
  std::unique_ptr<HostLease> own;
  if (!lease) {
    own.reset(new HostLease);
    lease = own.get();
  }
  const uint64_t most = n / sfwp::kMinMessage + 1;
  StageBufs sb;
  int rc = stage_bufs(*lease, 1, h_wire ? kNoBuf : n, kNoBuf, kNoBuf, &sb);
  void *pdig = nullptr, *psz = nullptr;
  if (rc == SF_OK) rc = lease->pin(kSlotDigests + 1, most * 20, &pdig);
  if (rc == SF_OK) rc = lease->pin(kSlotAux + 1, most * 4, &psz);
  if (rc != SF_OK) return rc;
  if (!h_wire) {
    SF_HIP(hipMemcpyAsync(sb.pin, d_wire, n, hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    h_wire = static_cast<const uint8_t*>(sb.pin);
  }
  bool too_large = false;
  sfwp::parse_run(h_wire, n, static_cast<uint8_t*>(pdig), static_cast<uint32_t*>(psz), most, &out->count,
                  &out->consumed, &out->stop, &too_large);
  g_parse_stats.set(1, out->count);
  g_parse_stats.set(2, 1);
  if (too_large) return SF_ERANGE;
  const uint64_t up = std::min(out->count, cap);
  if (up) {
    SF_HIP(hipMemcpyAsync(d_digests, pdig, up * 20, hipMemcpyHostToDevice, s));
    SF_HIP(hipMemcpyAsync(d_sizes, psz, up * 4, hipMemcpyHostToDevice, s));
    SF_HIP(hipStreamSynchronize(s));  // the pinned stages go back to the cache
  }
  return SF_OK;
}

// The messages of d_wire[0, n) (n > 0): the first min(count, cap) into
// d_digests / d_sizes, the count, the bytes and the stop into *out.  Blocking.
int parse_run_device(const uint8_t* d_wire, const uint8_t* h_wire, uint64_t n, uint8_t* d_digests, uint32_t* d_sizes,
                     uint64_t cap, Parsed* out, hipStream_t s, HostLease* lease) {
  if (knob(K_TEST_WIRE_PARSE_HOST) == 1) return parse_on_host(d_wire, h_wire, n, d_digests, d_sizes, cap, out, s, lease);
  Scan sc(s);
  int rc = scan_candidates<BlockRules>(d_wire, n, s, &sc);
  if (rc != SF_OK) return rc;
  Result* res = static_cast<Result*>(sc.result);
  const dim3 gw = grid256(sc.nw);
  rc = launch(recv_chain_kernel, gw, dim3(256), s, d_wire, n, sc.words, sc.ends, sc.nw, res);
  if (rc == SF_OK)
    rc = launch(recv_extract_kernel, gw, dim3(256), s, d_wire, n, sc.words, sc.ends, sc.nw,
                reinterpret_cast<uint32_t*>(d_digests), d_sizes, cap, res);
  if (rc != SF_OK) return rc;
  Result h{};
  SF_HIP(hipMemcpyAsync(&h, res, sizeof(Result), hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  g_parse_stats.set(0, h.cand);
  if (h.msgs && !(h.first_bad & 1ull))  // a candidate inside the last chained message
    return parse_on_host(d_wire, h_wire, n, d_digests, d_sizes, cap, out, s, lease);
  g_parse_stats.set(1, h.msgs);
  if (h.too_large) return SF_ERANGE;
  out->count = h.msgs;
  out->consumed = h.end;
  // what stands at E: at most one message's bytes decide it
  uint8_t tail[sfwp::kMaxMessage];
  const uint64_t tn = std::min<uint64_t>(n - h.end, sizeof(tail));
  if (tn) {
    if (h_wire) {
      memcpy(tail, h_wire + h.end, tn);
    } else {
      SF_HIP(hipMemcpyAsync(tail, d_wire + h.end, tn, hipMemcpyDeviceToHost, s));
      SF_HIP(hipStreamSynchronize(s));
    }
  }
  uint32_t len;
  uint64_t size;
  // (a whole message cannot stand at E: E would be a candidate and chained)
  const int c = sfwp::classify(tail, tn, &len, &size);
  out->stop = c == sfwp::kBlock ? sfwp::kMalformed : c;
  return SF_OK;
}

int parse_blocks_device(const void* d_wire, uint64_t n_bytes, void* d_digests, uint32_t* d_sizes, uint64_t cap,
                        uint64_t* n_out, uint64_t* consumed, int* stop, hipStream_t s) {
  g_parse_stats.reset();
  if (n_out) *n_out = 0;
  if (consumed) *consumed = 0;
  if (stop) *stop = SF_WIRE_END;
  if (!n_out || !consumed || !stop || (n_bytes && !d_wire) || n_bytes > kMaxRun ||
      misaligned(d_digests, 4) || misaligned(d_sizes, 4))
    return SF_EINVAL;
  if (n_bytes == 0) return SF_OK;
  if (!d_digests || !d_sizes) cap = 0;
  Parsed p;
  const int rc = parse_run_device(static_cast<const uint8_t*>(d_wire), nullptr, n_bytes,
                                  static_cast<uint8_t*>(d_digests), d_sizes, cap, &p, s, nullptr);
  if (rc != SF_OK) return rc;
  *n_out = p.count;
  *consumed = p.consumed;
  *stop = p.stop;
  return p.count > cap ? SF_ENOSPC : SF_OK;
}

struct ReceiveArgs {
  const sf_block_set* set;
  uint64_t base_offset;
  void* d_digests;
  uint32_t* d_sizes;
  uint64_t* d_offsets;
  int64_t* d_rows;
  uint64_t cap;
  uint64_t *n_out, *consumed;
  int* stop;
  uint64_t* end_offset;
};

int check_receive_args(const ReceiveArgs& a, const void* wire, uint64_t n_bytes) {
  g_parse_stats.reset();
  if (a.n_out) *a.n_out = 0;
  if (a.consumed) *a.consumed = 0;
  if (a.stop) *a.stop = SF_WIRE_END;
  if (a.end_offset) *a.end_offset = a.base_offset;
  if (!a.n_out || !a.consumed || !a.stop || !a.end_offset || (n_bytes && !wire) || n_bytes > kMaxRun)
    return SF_EINVAL;
  return SF_OK;
}

// Parse, then the running offsets, then the lookup, on s.  Blocking.
int receive_device(const ReceiveArgs& a, const uint8_t* d_wire, const uint8_t* h_wire, uint64_t n_bytes,
                   hipStream_t s, HostLease* lease) {
  uint64_t cap = a.cap;
  if (!a.d_digests || !a.d_sizes || !a.d_offsets || (a.set && !a.d_rows)) cap = 0;  // a query
  Parsed p;
  int rc = parse_run_device(d_wire, h_wire, n_bytes, static_cast<uint8_t*>(a.d_digests), a.d_sizes, cap, &p, s, lease);
  if (rc != SF_OK) return rc;
  *a.n_out = p.count;
  *a.consumed = p.consumed;
  *a.stop = p.stop;
  if (p.count > cap) return SF_ENOSPC;
  if (p.count == 0) return SF_OK;
  // d_offsets[i] = base_offset + sizes[0] + ... + sizes[i - 1], in 64 bits
  auto in = rocprim::make_transform_iterator(a.d_sizes, Widen());
  size_t tmp = 0;
  if ((rc = scan_exclusive(nullptr, tmp, in, a.d_offsets, a.base_offset, p.count, s)) != SF_OK) return rc;
  Scratch ws(s);
  if ((rc = stream_alloc(&ws.p, tmp + 8, s)) != SF_OK) return rc;
  if ((rc = scan_exclusive(ws.p, tmp, in, a.d_offsets, a.base_offset, p.count, s)) != SF_OK) return rc;
  if (a.set && (rc = sf_block_set_lookup(a.set, a.d_digests, p.count, a.d_rows, s)) != SF_OK) return rc;
  uint64_t last_off = 0;
  uint32_t last_size = 0;
  SF_HIP(hipMemcpyAsync(&last_off, a.d_offsets + p.count - 1, 8, hipMemcpyDeviceToHost, s));
  SF_HIP(hipMemcpyAsync(&last_size, a.d_sizes + p.count - 1, 4, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  *a.end_offset = last_off + last_size;
  return SF_OK;
}

int receive_buffer(const sf_block_set* set, const uint8_t* wire, uint64_t n_bytes, uint64_t base_offset,
                   sf_block_sig* out, int64_t* src_rows, uint64_t cap, uint64_t* n_out, uint64_t* consumed,
                   int* stop, uint64_t* end_offset) {
  ReceiveArgs a{set, base_offset, nullptr, nullptr, nullptr, nullptr, 0, n_out, consumed, stop, end_offset};
  int rc = check_receive_args(a, wire, n_bytes);
  if (rc != SF_OK || n_bytes == 0) return rc;
  if (!out || (set && !src_rows)) cap = 0;
  HostLease res;
  hipStream_t* st;
  hipEvent_t* ev;
  if ((rc = res.streams(st, ev)) != SF_OK) return rc;
  hipStream_t s = st[0];
  const uint8_t* d_wire = nullptr;
  if ((rc = upload_run(res, wire, n_bytes, s, ev, &d_wire)) != SF_OK) return rc;
  // device rows for every message the run can hold: offsets, rows, sizes
  const uint64_t most = n_bytes / sfwp::kMinMessage + 1;
  void *ddig = nullptr, *daux = nullptr;
  if ((rc = res.dev(kSlotDigests, most * 20, &ddig)) != SF_OK) return rc;
  if ((rc = res.dev(kSlotAux, most * 20, &daux)) != SF_OK) return rc;
  a.d_digests = ddig;
  a.d_offsets = static_cast<uint64_t*>(daux);
  a.d_rows = reinterpret_cast<int64_t*>(a.d_offsets + most);
  a.d_sizes = reinterpret_cast<uint32_t*>(a.d_rows + most);
  a.cap = most;
  if ((rc = receive_device(a, d_wire, wire, n_bytes, s, &res)) != SF_OK) return rc;
  const uint64_t n = *n_out;
  if (n > cap) return SF_ENOSPC;
  if (n == 0) return SF_OK;
  void *pdig = nullptr, *paux = nullptr;
  if ((rc = res.pin(kSlotDigests, n * 20, &pdig)) != SF_OK) return rc;
  if ((rc = res.pin(kSlotAux, most * 20, &paux)) != SF_OK) return rc;
  SF_HIP(hipMemcpyAsync(pdig, ddig, n * 20, hipMemcpyDeviceToHost, s));
  SF_HIP(hipMemcpyAsync(paux, daux, (2 * most + n) * 8 - n * 4, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  const uint64_t* po = static_cast<const uint64_t*>(paux);
  const int64_t* pr = reinterpret_cast<const int64_t*>(po + most);
  const uint32_t* pz = reinterpret_cast<const uint32_t*>(pr + most);
  for (uint64_t i = 0; i < n; i++) {
    out[i].offset = po[i];
    out[i].size = pz[i];
    memcpy(out[i].sha1, static_cast<const uint8_t*>(pdig) + 20 * i, 20);
    if (src_rows) src_rows[i] = set ? pr[i] : -1;
  }
  return SF_OK;
}

}  // namespace

extern "C" {

int sf_wire_parse_blocks_device(const void* d_wire, uint64_t n_bytes, void* d_digests, uint32_t* d_sizes,
                                uint64_t cap, uint64_t* n_out, uint64_t* consumed, int* stop, void* stream) {
  return guarded(
      [&] { return parse_blocks_device(d_wire, n_bytes, d_digests, d_sizes, cap, n_out, consumed, stop, as_stream(stream)); });
}

int sf_receive_blocks_device(const sf_block_set* set, const void* d_wire, uint64_t n_bytes, uint64_t base_offset,
                             void* d_digests, uint32_t* d_sizes, uint64_t* d_offsets, int64_t* d_rows, uint64_t cap,
                             uint64_t* n_out, uint64_t* consumed, int* stop, uint64_t* end_offset, void* stream) {
  return guarded([&]() -> int {
    const ReceiveArgs a{set, base_offset, d_digests, d_sizes, d_offsets, d_rows, cap, n_out, consumed, stop, end_offset};
    const int rc = check_receive_args(a, d_wire, n_bytes);
    if (rc != SF_OK) return rc;
    // dword stores to the digests and sizes, 8-B stores to the offsets (the scan) and rows
    if (misaligned(d_digests, 4) || misaligned(d_sizes, 4) || misaligned(d_offsets, 8) || misaligned(d_rows, 8))
      return SF_EINVAL;
    if (n_bytes == 0) return SF_OK;
    return receive_device(a, static_cast<const uint8_t*>(d_wire), nullptr, n_bytes, as_stream(stream), nullptr);
  });
}

int sf_receive_blocks_buffer(const sf_block_set* set, const void* wire, uint64_t n_bytes, uint64_t base_offset,
                             sf_block_sig* out, int64_t* src_rows, uint64_t cap, uint64_t* n_out, uint64_t* consumed,
                             int* stop, uint64_t* end_offset) {
  return guarded([&] {
    return receive_buffer(set, static_cast<const uint8_t*>(wire), n_bytes, base_offset, out, src_rows, cap, n_out,
                          consumed, stop, end_offset);
  });
}

int sf_test_wire_parse_stats(uint64_t out[4]) { return g_parse_stats.read(out); }

}  // extern "C"
