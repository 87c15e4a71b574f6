// sf_recv_files.hip -- a whole GetFiles stream received on the device
// (include/syncfast_amd.h: sf_receive_files_device): many files' FILE_START,
// FILE_BLOCK and FILE_END messages in one buffer, parsed as the reference
// parser reads them and accepted in its sink's order (sf_wire_files.hpp has
// the rules).  Its own translation unit: sf_recv.hip, sf_recv_data.hip and
// their code objects stay as they are.
//
// Names and digests are arbitrary bytes, so message i starts where message
// i - 1 ends, which is serial.  What is parallel:
//
//   candidates, scan   sf_recv_scan.hpp, shared with the other two parsers:
//               the bitmap of every position where files_message holds, and
//               every candidate's index in position order.
//   chain       one lane per word, for each of its candidates at p with
//               length L and kind K: the link is good when p + L is a
//               candidate, none lies in (p, p + L) and the sink takes the
//               kind at p + L after K.  L reaches 112, so the window is two
//               64-bit reads of the bitmap (three words).  atomicMin keeps
//               the first candidate whose link is not good, with a bit that
//               says whether a candidate lay inside it; the candidate at byte
//               0 is checked against the state carried in.  The lane also
//               counts its word's FILE_STARTs and FILE_BLOCKs, the two halves
//               of one 64-bit count.
//   scan        of those counts: every candidate's file and block index.
//   extract     one lane per word: candidates below the first bad one are
//               the messages.  A FILE_BLOCK writes digest, size and section, a
//               FILE_START the name's span and the section's first block; the
//               last message writes E, the state after it, the totals and the
//               bytes that stand at E.
//   (one read-back: totals, E, flags and those bytes)
//   offsets     one 64-bit exclusive scan G of all sizes, then one lane per
//               block and per section: offset[i] = G[i] - G[first[file(i)]],
//               file_size[f] = G[first[f + 1]] - G[first[f]], + base_offset
//               in the section carried in.
//   lookup      one sf_block_set_lookup over all digests of all files.
//
// With no candidate strictly inside [0, E) off the chain, the candidates in
// [0, E) ARE the chain and the reference reads exactly that prefix (DESIGN.md
// 3.13).  A candidate inside the last chained message (a digest that spells a
// tag, a name that holds one) sends the whole buffer to parse_files_run on
// the host.  Every dependency is a kernel boundary; no lane waits for
// another; every loop is bounded by a message's 112 bytes or a word's 64 bits.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include <rocprim/iterator/transform_iterator.hpp>

#include "sf_recv_scan.hpp"
#include "sf_wire_files.hpp"
#include "../../include/syncfast_amd_test.h"

using namespace sfrs;

namespace {

// Files and blocks are counted in the high and the low half of one 64-bit
// scan: at most 2^35 / 12 < 2^32 FILE_STARTs and 2^35 / 34 < 2^32 FILE_BLOCKs.
constexpr uint64_t kMaxFilesRun = 1ull << 35;

// What the host reads back, in one copy.
struct Result {
  unsigned long long first_bad;  // ((index of the prefix's last message + 1) << 1) | (no candidate inside it)
  unsigned long long cand, msgs, end, blocks, files;
  unsigned long long end_offset;  // the offsets kernel's, read back on its own
  uint32_t too_large, open_out, tail_n;
  uint8_t tail[sfwp::kFilesTail];  // the bytes at `end`
};
static_assert(offsetof(Result, first_bad) == 0 && sizeof(Result::first_bad) == 8 && sizeof(Result) <= 256,
              "sfrs::Scan::result: 256 bytes that begin with first_bad");

// Every tag begins "FILE_".  'F' alone as the prefilter: a stream is mostly
// FILE_BLOCK messages of about 37 bytes, whose digests hold an 'F' once in
// 256 bytes, so a second byte would save one test in seven and cost every
// lane a second comparison of its 16 bytes.
struct FilesRules {
  static constexpr uint32_t kFirst = 'F', kSecond = 0;
  static __device__ __forceinline__ uint32_t message(const uint8_t* b, uint64_t avail, uint32_t* kind,
                                                     uint64_t* size) {
    return sfwp::files_message(b, avail, kind, size);
  }
};

constexpr unsigned long long kOneFile = 1ull << 32, kOneBlock = 1ull;

__global__ void __launch_bounds__(256) files_chain_kernel(const uint8_t* __restrict__ data, uint64_t n,
                                                          const unsigned long long* __restrict__ words,
                                                          const uint64_t* __restrict__ ends, uint64_t nw, int open,
                                                          unsigned long long* __restrict__ kinds,
                                                          Result* __restrict__ res) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nw) return;
  unsigned long long m = words[w], count = 0;
  if (w == 0 && !(m & 1ull)) atomicMin(&res->first_bad, 1ull);  // nothing at byte 0: no message
  uint64_t i = ends[w] - (uint64_t)__popcll(m);
  for (; m; m &= m - 1, i++) {
    const uint64_t p = (w << 6) + (uint64_t)(__ffsll((long long)m) - 1);
    uint32_t K = 0;
    uint64_t size;
    const uint32_t L = sfwp::files_message(data + p, n - p, &K, &size);  // 9..112: p is a candidate
    count += K == sfwp::kStart ? kOneFile : K == sfwp::kFileBlock ? kOneBlock : 0ull;
    if (p == 0 && !sfwp::accepts(open != 0, K)) atomicMin(&res->first_bad, 1ull);  // the state does not take it
    // positions p + 1 .. p + 64 in v0, p + 65 .. p + 128 in v1; L - 1 of them lie inside the message
    const unsigned long long v0 = bits_from(words, nw, p + 1), v1 = bits_from(words, nw, p + 65);
    const uint32_t in = L - 1;
    const bool inside = in <= 64 ? (v0 & low_bits(in)) != 0 : (v0 | (v1 & low_bits(in - 64))) != 0;
    bool next = in < 64 ? (v0 >> in) & 1ull : (v1 >> (in - 64)) & 1ull;  // p + L
    // a candidate at p + L is a whole message: its sixth byte is there and says its kind
    if (next) {
      const uint8_t c = data[p + L + 5];
      const uint32_t K2 = c == 'S' ? sfwp::kStart : c == 'B' ? sfwp::kFileBlock : sfwp::kFileEnd;
      next = sfwp::accepts(K != sfwp::kFileEnd, K2);
    }
    if (inside || !next) atomicMin(&res->first_bad, ((unsigned long long)(i + 1) << 1) | (inside ? 0ull : 1ull));
  }
  kinds[w] = count;
}

struct FilesOutputs {
  uint32_t* digests;
  uint32_t* sizes;
  uint32_t* block_file;
  uint64_t block_cap;
  uint64_t* name_at;
  uint32_t* name_len;
  uint64_t* first;
  uint64_t file_cap;
};

__global__ void __launch_bounds__(256) files_extract_kernel(const uint8_t* __restrict__ data, uint64_t n,
                                                            const unsigned long long* __restrict__ words,
                                                            const uint64_t* __restrict__ ends,
                                                            const unsigned long long* __restrict__ kinds,
                                                            const unsigned long long* __restrict__ kends, uint64_t nw,
                                                            int open, FilesOutputs o, Result* __restrict__ res) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nw) return;
  const uint64_t k = res->first_bad >> 1;  // the messages (written by the chain kernel, two launches earlier)
  const uint64_t carried = open ? 1u : 0u;
  if (w == 0) {
    res->cand = ends[nw - 1];
    res->msgs = k;
    if (carried && o.file_cap) {  // section 0: the file that was open when the buffer began
      o.name_at[0] = ~0ull;
      o.name_len[0] = 0;
      o.first[0] = 0;
    }
    if (k == 0) {  // nothing accepted: the state as it came, and what stands at byte 0
      res->files = carried;
      res->open_out = (uint32_t)carried;
      const uint32_t tn = n < sfwp::kFilesTail ? (uint32_t)n : sfwp::kFilesTail;
      for (uint32_t j = 0; j < tn; j++) res->tail[j] = data[j];
      res->tail_n = tn;
    }
  }
  unsigned long long m = words[w];
  uint64_t i = ends[w] - (uint64_t)__popcll(m);
  const unsigned long long before = kends[w] - kinds[w];
  uint64_t nf = (before >> 32) + carried, nb = before & 0xFFFFFFFFull;  // sections and blocks before this word
  for (; m && i < k; m &= m - 1, i++) {
    const uint64_t p = (w << 6) + (uint64_t)(__ffsll((long long)m) - 1);
    uint32_t K = 0;
    uint64_t size = 0;
    const uint32_t L = sfwp::files_message(data + p, n - p, &K, &size);
    if (K == sfwp::kFileBlock) {
      if (size > 0xFFFFFFFFull) atomicOr(&res->too_large, 1u);
      if (nb < o.block_cap) {
        store_digest(o.digests + 5 * nb, data + p + sfwp::kTag);
        o.sizes[nb] = (uint32_t)size;
        o.block_file[nb] = (uint32_t)(nf - 1);
      }
      nb++;
    } else if (K == sfwp::kStart) {
      if (nf < o.file_cap) {
        o.name_at[nf] = p + sfwp::kStartTag;
        o.name_len[nf] = L - sfwp::kStartTag - 1;
        o.first[nf] = nb;
      }
      nf++;
    }
    if (i == k - 1) {
      const uint64_t e = p + L;
      res->end = e;
      res->blocks = nb;
      res->files = nf;
      res->open_out = K != sfwp::kFileEnd;
      const uint32_t tn = n - e < sfwp::kFilesTail ? (uint32_t)(n - e) : sfwp::kFilesTail;
      for (uint32_t j = 0; j < tn; j++) res->tail[j] = data[e + j];
      res->tail_n = tn;
    }
  }
}

// One lane per block and per section (and one more for first's last entry).
// G: the exclusive scan of all sizes (NULL with no block).
__global__ void __launch_bounds__(256) files_offsets_kernel(const uint64_t* __restrict__ G,
                                                            const uint32_t* __restrict__ sizes,
                                                            const uint32_t* __restrict__ block_file, uint64_t nb,
                                                            uint64_t* __restrict__ first, uint64_t nf, int open,
                                                            uint64_t base_offset, uint64_t* __restrict__ offsets,
                                                            uint64_t* __restrict__ file_size,
                                                            unsigned long long* __restrict__ end_offset) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nb) {
    const uint32_t f = block_file[t];
    offsets[t] = G[t] - G[first[f]] + (open && f == 0 ? base_offset : 0);
  }
  if (t < nf) {
    const uint64_t total = nb ? G[nb - 1] + sizes[nb - 1] : 0;
    const uint64_t lo = first[t], hi = t + 1 < nf ? first[t + 1] : nb;
    const uint64_t size = (hi < nb ? G[hi] : total) - (lo < nb ? G[lo] : total) + (open && t == 0 ? base_offset : 0);
    file_size[t] = size;
    if (t == nf - 1) *end_offset = size;
  }
  if (t == nf) first[nf] = nb;
}

sfi::Stats4 g_files_stats;  // sf_test_recv_files_stats

}  // namespace

using namespace sfi;

namespace {

struct FilesArgs {
  const sf_block_set* set;
  int open;
  uint64_t base_offset;
  void* d_digests;
  uint32_t* d_sizes;
  uint64_t* d_offsets;
  int64_t* d_rows;
  uint32_t* d_block_file;
  uint64_t block_cap;
  uint64_t* d_name_at;
  uint32_t* d_name_len;
  uint64_t* d_first;
  uint64_t* d_file_size;
  uint64_t file_cap;
  uint64_t *n_blocks, *n_files, *consumed;
  int *stop, *open_out;
  uint64_t* end_offset;
};

// The serial parse on the host (the buffer is copied back) and the upload of
// what the device route would have written.  Blocking.
int files_on_host(const FilesArgs& a, const uint8_t* d_wire, uint64_t n, uint64_t block_cap, uint64_t file_cap,
                  bool query, hipStream_t s) {
  std::vector<uint8_t> wire(n);
  SF_HIP(hipMemcpyAsync(wire.data(), d_wire, n, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  sfwp::FilesParsed r;
  sfwp::parse_files_run(wire.data(), n, a.open != 0, a.base_offset, sfwp::FilesOut{}, &r);  // the counts
  std::vector<uint8_t> dig(r.n_blocks * 20);
  std::vector<uint32_t> sizes(r.n_blocks), bfile(r.n_blocks), nlen(r.n_files);
  std::vector<uint64_t> offs(r.n_blocks), nat(r.n_files), first(r.n_files + 1), fsize(r.n_files);
  const sfwp::FilesOut o{dig.data(), sizes.data(), offs.data(), bfile.data(), r.n_blocks, nat.data(),
                         nlen.data(), first.data(), fsize.data(), r.n_files};
  sfwp::parse_files_run(wire.data(), n, a.open != 0, a.base_offset, o, &r);
  g_files_stats.set(1, r.messages);
  g_files_stats.set(2, 1);
  *a.n_blocks = r.n_blocks;
  *a.n_files = r.n_files;
  *a.consumed = r.consumed;
  *a.stop = r.stop;
  *a.open_out = r.open ? 1 : 0;
  if (r.too_large) return SF_ERANGE;
  if (query) return r.n_blocks || r.n_files ? SF_ENOSPC : SF_OK;
  const bool fits = r.n_blocks <= block_cap && r.n_files <= file_cap;
  const uint64_t ub = std::min(r.n_blocks, block_cap), uf = std::min(r.n_files, file_cap);
  auto up = [&](void* dst, const void* src, uint64_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
  };
  SF_HIP(up(a.d_digests, dig.data(), ub * 20));
  SF_HIP(up(a.d_sizes, sizes.data(), ub * 4));
  SF_HIP(up(a.d_block_file, bfile.data(), ub * 4));
  SF_HIP(up(a.d_name_at, nat.data(), uf * 8));
  SF_HIP(up(a.d_name_len, nlen.data(), uf * 4));
  SF_HIP(up(a.d_first, first.data(), (fits ? uf + 1 : uf) * 8));
  if (fits) {
    SF_HIP(up(a.d_offsets, offs.data(), ub * 8));
    SF_HIP(up(a.d_file_size, fsize.data(), uf * 8));
  }
  SF_HIP(hipStreamSynchronize(s));  // the vectors go out of scope
  if (!fits) return SF_ENOSPC;
  *a.end_offset = r.end_offset;
  if (a.set && r.n_blocks) {
    const int rc = sf_block_set_lookup(a.set, a.d_digests, r.n_blocks, a.d_rows, s);
    if (rc != SF_OK) return rc;
    SF_HIP(hipStreamSynchronize(s));
  }
  return SF_OK;
}

// d_wire[0, n) (n > 0) on s.  Blocking.
int files_device(const FilesArgs& a, const uint8_t* d_wire, uint64_t n, hipStream_t s) {
  uint64_t block_cap = a.block_cap, file_cap = a.file_cap;
  const bool query = !a.d_digests || !a.d_sizes || !a.d_offsets || !a.d_block_file || !a.d_name_at ||
                     !a.d_name_len || !a.d_first || !a.d_file_size;
  if (query) block_cap = file_cap = 0;  // nothing is written
  if (knob(K_TEST_WIRE_PARSE_HOST) == 1) return files_on_host(a, d_wire, n, block_cap, file_cap, query, s);
  Scan sc(s);
  int rc = scan_candidates<FilesRules>(d_wire, n, s, &sc);
  if (rc != SF_OK) return rc;
  Result* res = static_cast<Result*>(sc.result);
  // the kinds' counts per word and their scan
  size_t tmp = 0;
  unsigned long long* const nul = nullptr;
  if ((rc = scan_inclusive(nullptr, tmp, nul, nul, sc.nw, s)) != SF_OK) return rc;
  ScratchLayout KL;
  const size_t kinds_at = KL.add(sc.nw * 8), kends_at = KL.add(sc.nw * 8);
  Scratch ks(s);
  if ((rc = stream_alloc(&ks.p, KL.total() + tmp + 8, s)) != SF_OK) return rc;
  unsigned long long* kinds = KL.at<unsigned long long>(ks.p, kinds_at);
  unsigned long long* kends = KL.at<unsigned long long>(ks.p, kends_at);
  const dim3 gw = grid256(sc.nw);
  rc = launch(files_chain_kernel, gw, dim3(256), s, d_wire, n, sc.words, sc.ends, sc.nw, a.open, kinds, res);
  if (rc == SF_OK) rc = scan_inclusive(KL.at<void>(ks.p, KL.total()), tmp, kinds, kends, sc.nw, s);
  if (rc != SF_OK) return rc;
  const FilesOutputs o{static_cast<uint32_t*>(a.d_digests), a.d_sizes, a.d_block_file, block_cap, a.d_name_at,
                       a.d_name_len, a.d_first, file_cap};
  rc = launch(files_extract_kernel, gw, dim3(256), s, d_wire, n, sc.words, sc.ends, kinds, kends, sc.nw, a.open, o,
              res);
  if (rc != SF_OK) return rc;
  Result h{};
  SF_HIP(hipMemcpyAsync(&h, res, sizeof(Result), hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  g_files_stats.set(0, h.cand);
  if (h.msgs && !(h.first_bad & 1ull))  // a candidate inside the last chained message
    return files_on_host(a, d_wire, n, block_cap, file_cap, query, s);
  g_files_stats.set(1, h.msgs);
  const uint64_t nb = h.blocks, nf = h.files;
  *a.n_blocks = nb;
  *a.n_files = nf;
  *a.consumed = h.end;
  *a.open_out = (int)h.open_out;
  // what stands at E: a whole message there is one the chain did not take
  uint32_t kind, len;
  uint64_t size;
  const int c = sfwp::classify_files(h.tail, h.tail_n, &kind, &len, &size);
  *a.stop = c == sfwp::kMessage ? sfwp::kUnexpected : c;
  if (h.too_large) return SF_ERANGE;
  if (query) return nb || nf ? SF_ENOSPC : SF_OK;
  if (nb > block_cap || nf > file_cap) return SF_ENOSPC;
  // G = the exclusive scan of all sizes in 64 bits, then the offsets within each section
  Scratch gs(s);
  uint64_t* G = nullptr;
  if (nb) {
    auto in = rocprim::make_transform_iterator(a.d_sizes, Widen());
    size_t gtmp = 0;
    if ((rc = scan_exclusive(nullptr, gtmp, in, G, 0, nb, s)) != SF_OK) return rc;
    ScratchLayout GL;
    const size_t g_at = GL.add(nb * 8);
    if ((rc = stream_alloc(&gs.p, GL.total() + gtmp + 8, s)) != SF_OK) return rc;
    G = GL.at<uint64_t>(gs.p, g_at);
    if ((rc = scan_exclusive(GL.at<void>(gs.p, GL.total()), gtmp, in, G, 0, nb, s)) != SF_OK) return rc;
  }
  rc = launch(files_offsets_kernel, grid256(std::max(nb, nf + 1)), dim3(256), s, G, a.d_sizes, a.d_block_file, nb,
              a.d_first, nf, a.open, a.base_offset, a.d_offsets, a.d_file_size, &res->end_offset);
  if (rc != SF_OK) return rc;
  if (a.set && nb && (rc = sf_block_set_lookup(a.set, a.d_digests, nb, a.d_rows, s)) != SF_OK) return rc;
  unsigned long long end_offset = a.base_offset;
  if (nf) SF_HIP(hipMemcpyAsync(&end_offset, &res->end_offset, 8, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  *a.end_offset = end_offset;
  return SF_OK;
}

int receive_files(const FilesArgs& a, const void* d_wire, uint64_t n_bytes, hipStream_t s) {
  g_files_stats.reset();
  const uint64_t carried = a.open ? 1 : 0;
  if (a.n_blocks) *a.n_blocks = 0;
  if (a.n_files) *a.n_files = carried;
  if (a.consumed) *a.consumed = 0;
  if (a.stop) *a.stop = SF_WIRE_END;
  if (a.open_out) *a.open_out = (int)carried;
  if (a.end_offset) *a.end_offset = a.base_offset;
  if (!a.n_blocks || !a.n_files || !a.consumed || !a.stop || !a.open_out || !a.end_offset || (n_bytes && !d_wire) ||
      n_bytes > kMaxFilesRun || (a.set && !a.d_rows))
    return SF_EINVAL;
  // dword stores to the digests, sizes, sections and name lengths, 8-B stores to the 64-bit lists
  if (misaligned(a.d_digests, 4) || misaligned(a.d_sizes, 4) || misaligned(a.d_block_file, 4) ||
      misaligned(a.d_name_len, 4) || misaligned(a.d_offsets, 8) || misaligned(a.d_rows, 8) ||
      misaligned(a.d_name_at, 8) || misaligned(a.d_first, 8) || misaligned(a.d_file_size, 8))
    return SF_EINVAL;
  if (n_bytes == 0) return SF_OK;
  return files_device(a, static_cast<const uint8_t*>(d_wire), n_bytes, s);
}

}  // namespace

extern "C" {

int sf_receive_files_device(const sf_block_set* set, const void* d_wire, uint64_t n_bytes, int open,
                            uint64_t base_offset, void* d_digests, uint32_t* d_sizes, uint64_t* d_offsets,
                            int64_t* d_rows, uint32_t* d_block_file, uint64_t block_cap, uint64_t* d_file_name_at,
                            uint32_t* d_file_name_len, uint64_t* d_file_first, uint64_t* d_file_size, uint64_t file_cap,
                            uint64_t* n_blocks, uint64_t* n_files, uint64_t* consumed, int* stop, int* open_out,
                            uint64_t* end_offset, void* stream) {
  return guarded([&]() -> int {
    const FilesArgs a{set,          open,           base_offset,  d_digests,       d_sizes,  d_offsets, d_rows,
                      d_block_file, block_cap,      d_file_name_at, d_file_name_len, d_file_first, d_file_size,
                      file_cap,     n_blocks,       n_files,      consumed,        stop,     open_out,  end_offset};
    return receive_files(a, d_wire, n_bytes, as_stream(stream));
  });
}

int sf_test_recv_files_stats(uint64_t out[4]) { return g_files_stats.read(out); }

}  // extern "C"
