// sf_wire_get_files.hpp -- the framing rules of the source's side of the
// GET_FILE requests (src/sync/fs.rs:177-231 answers them, proto.rs:365-376
// reads them): a received run of "GET_FILE\n" + name + "\n" messages parsed,
// and the plan of the answer sf_serve_get_files_device builds from it.  Beside
// sf_wire_entries.hpp, which writes the same message, and built on its pieces:
// one request at a known start (get_file_message), what stands at a stop
// (classify_get_files), the serial parse of a whole buffer
// (parse_get_files_run), the same parse told by lines (a request is two lines:
// line_is_tag, line_is_name, requests_of_lines -- what the kernels of
// sf_serve_files.hip run), and the answer's plan: where answering stops
// (serve_over, the SF_SERVE_* reasons) and the serial definition of the whole
// call (build_serve_files_serial).
//
//   GET_FILE    "GET_FILE\n" + 0..100 name bytes holding no '\n' + "\n"    10..110 bytes
//
// A name cannot hold '\n'.  So while every earlier request is whole and valid,
// request k is exactly lines 2k and 2k + 1 of the buffer (a line: the bytes
// from behind the previous '\n', or from byte 0, up to the next one): line 2k
// is the 8 bytes "GET_FILE", line 2k + 1 at most 100 bytes.  The requests the
// reference parser reads are therefore (the first terminated line that fails
// its test) / 2, or all whole pairs of terminated lines, and nothing a name or
// a later message holds can change that: no position is guessed, so nothing
// can be forged and there is no fallback.
//
// No HIP and no library header here (tests/native/wire_get_files.cpp tests it
// on a CPU).  Everything but the classes and the serial definitions is
// constexpr: the kernels call the same functions, so host and device cannot
// disagree.
#pragma once
#include "sf_wire_entries.hpp"

namespace sfwp {

// Not a stop: a whole GET_FILE (classify_get_files).
constexpr int kRequest = kHeader;

constexpr uint32_t kGetFileWord = kGetFileTag - 1;             // 8: "GET_FILE" without its newline
constexpr uint32_t kMinGetFile = kGetFileTag + 1;              // 10
constexpr uint32_t kMaxGetFile = kGetFileTag + kNameMax + 1;   // 110
constexpr uint32_t kGetFilesTail = 112;  // bytes at a stop that decide its class (110 and room to spare)

constexpr bool is_get_file_word(const uint8_t* b) {
  return (b[0] == 'G') & (b[1] == 'E') & (b[2] == 'T') & (b[3] == '_') & (b[4] == 'F') & (b[5] == 'I') &
         (b[6] == 'L') & (b[7] == 'E');
}

// A whole GET_FILE at b, of which `avail` bytes may be read: its length (10
// to 110) with the name's length in *name_len, else 0.  The name's newline
// must stand among the first 101 bytes behind the tag
// (read_line(FILENAME_MAX)).  Reads no byte at or past b + avail.  The name
// is the name_len bytes at b + 9.
constexpr uint32_t get_file_message(const uint8_t* b, uint64_t avail, uint32_t* name_len) {
  if (avail < kMinGetFile || !(is_get_file_word(b) & (b[kGetFileWord] == '\n'))) return 0;
  const uint64_t left = avail - kGetFileTag;
  const uint32_t room = left > kNameMax + 1 ? kNameMax + 1 : (uint32_t)left;
  uint32_t n = 0;
  while (n < room && b[kGetFileTag + n] != '\n') n++;
  if (n == room) return 0;
  *name_len = n;
  return kGetFileTag + n + 1;
}

// What stands at b (avail bytes to the end of the buffer, of which the first
// min(avail, 110) are read), as the parser rules it: kRequest with its length
// and name length, or kEnd (nothing), kIncomplete (a prefix that more bytes
// could complete), kOther (the complete command line of one of the other eight
// commands, whatever follows it) or kMalformed (the parser raises:
// "Unterminated command" with 20 bytes and no newline among 21, "Unknown
// command", "Unterminated filename" with 100 name bytes and no newline among
// 101 -- also when only those 100 are there yet, the parser's own boundary).
inline int classify_get_files(const uint8_t* b, uint64_t avail, uint32_t* len, uint32_t* name_len) {
  *len = 0;
  if (avail == 0) return kEnd;
  bool raise = false;
  const int c = line_end(b, avail, kCommandMax, &raise);
  if (c < 0) return raise ? kMalformed : kIncomplete;
  if (c != (int)kGetFileWord || !is_get_file_word(b)) return is_command(b, (size_t)c) ? kOther : kMalformed;
  const int e = line_end(b + kGetFileTag, avail - kGetFileTag, kNameMax, &raise);
  if (e < 0) return raise ? kMalformed : kIncomplete;
  *name_len = (uint32_t)e;
  *len = kGetFileTag + (uint32_t)e + 1;
  return kRequest;
}

// The outputs of parse_get_files_run: one row per request; both lists may be
// NULL with cap = 0.
struct GetFilesOut {
  uint64_t* name_at;   // [cap] the name's first byte in the buffer
  uint32_t* name_len;  // [cap]
  uint64_t cap;
};

struct GetFilesParsed {
  uint64_t count = 0, consumed = 0;
  int stop = kEnd;
};

// The buffer at b[0, n), request after request as the reference parser reads
// it: the first min(count, cap) rows are written, r->stop = what stands after
// the requests.
inline void parse_get_files_run(const uint8_t* b, uint64_t n, const GetFilesOut& o, GetFilesParsed* r) {
  uint64_t p = 0, k = 0;
  for (;;) {
    uint32_t len = 0, name_len = 0;
    const int c = classify_get_files(b + p, n - p, &len, &name_len);
    if (c != kRequest) {
      r->stop = c;
      break;
    }
    if (k < o.cap) {
      o.name_at[k] = p + kGetFileTag;
      o.name_len[k] = name_len;
    }
    p += len;
    k++;
  }
  r->count = k;
  r->consumed = p;
}

// ---- the same parse, told by lines ----

// Line j ends at the j-th '\n' of the buffer, at position p, and is `len`
// bytes long (len <= p; the caller may give any value above 100 for a longer
// one).  An even line must be the request's tag, an odd one a name.
constexpr bool line_is_tag(const uint8_t* b, uint64_t p, uint64_t len) {
  return len == kGetFileWord && is_get_file_word(b + p - kGetFileWord);
}
constexpr bool line_is_name(uint64_t len) { return len <= kNameMax; }
constexpr bool line_ok(const uint8_t* b, uint64_t j, uint64_t p, uint64_t len) {
  return (j & 1) ? line_is_name(len) : line_is_tag(b, p, len);
}

// The requests of a buffer with `lines` terminated lines whose first failing
// line is first_bad (any value >= lines: none fails).
constexpr uint64_t requests_of_lines(uint64_t lines, uint64_t first_bad) {
  return (first_bad < lines ? first_bad : lines) / 2;
}

// The same result as parse_get_files_run's count and consumed, line by line:
// the definition the device parse is held against on the host.
inline void parse_get_files_lines(const uint8_t* b, uint64_t n, uint64_t* count, uint64_t* consumed) {
  uint64_t lines = 0, first_bad = ~0ull, start = 0;
  for (uint64_t p = 0; p < n; p++) {
    if (b[p] != '\n') continue;
    if (first_bad == ~0ull && !line_ok(b, lines, p, p - start)) first_bad = lines;
    lines++;
    start = p + 1;
  }
  const uint64_t k = requests_of_lines(lines, first_bad);
  uint64_t seen = 0, end = 0;
  for (uint64_t p = 0; p < n && seen < 2 * k; p++)
    if (b[p] == '\n' && ++seen == 2 * k) end = p + 1;
  *count = k;
  *consumed = end;
}

// ---- the plan of the answer ----

// SF_SERVE_* of include/syncfast_amd.h: why answering stopped.
constexpr int kServeAll = 0, kServeBadName = 1, kServeUnknown = 2, kServeFull = 3;
constexpr uint64_t kServeMaxMessages = 1ull << 32;

// Whether row r of the source's CSR holds: first[r] <= first[r + 1] <= n_blocks.
constexpr bool serve_row_ok(const uint64_t* first, uint64_t n_blocks, uint64_t r) {
  return first[r] <= first[r + 1] && first[r + 1] <= n_blocks;
}

// Whether the answers of requests [0, k1) -- `blocks` FILE_BLOCK messages of
// block_bytes bytes in all, name_bytes of names -- leave the run's bounds:
// more than 2^32 messages, or more than max_run_bytes bytes (0: no bound).
// With block_bytes = 34 * blocks, the shortest a block can be, it is the
// coarse test that bounds the blocks whose lengths are scanned at all; with
// the scan's own value it is the exact one.
constexpr bool serve_over(uint64_t blocks, uint64_t block_bytes, uint64_t name_bytes, uint64_t k1,
                          uint64_t max_run_bytes) {
  if (blocks > kServeMaxMessages || blocks + 2 * k1 > kServeMaxMessages) return true;
  return max_run_bytes != 0 && files_run_total(block_bytes, name_bytes, k1) > max_run_bytes;
}
constexpr uint64_t serve_coarse_bytes(uint64_t blocks) {  // blocks <= 2^32
  return (uint64_t)kMinMessage * blocks;
}

// Block j of the answer, which belongs to request k (req_first: the CSR of the
// requests over the answer's blocks), in the source's table.
constexpr uint64_t serve_block_src(const uint64_t* first, const uint64_t* req_first, const int64_t* rows, uint64_t k,
                                   uint64_t j) {
  return first[(uint64_t)rows[k]] + (j - req_first[k]);
}

struct ServePlan {
  uint64_t n_answered = 0, answered_bytes = 0, total = 0, messages = 0, bad_row = ~0ull;
  int why = kServeAll;
};

// The serial definition of sf_serve_get_files_device behind its parse and its
// lookup: requests k in [0, n) are the spans (name_at[k], name_len[k]) of
// req[], rows[k] the set's answer.  Request after request: a name that is no
// UTF-8 stops with kServeBadName, a row of -1 with kServeUnknown, a row whose
// CSR entries do not hold sets bad_row (the caller returns SF_EINVAL), an
// answer that would leave the bounds stops with kServeFull; else the answer is
// written at out (NULL: the plan alone).  answered_bytes: the bytes of req[]
// the answered requests occupy.
inline ServePlan build_serve_files_serial(const uint8_t* req, const uint64_t* name_at, const uint32_t* name_len,
                                          uint64_t n, const int64_t* rows, const uint64_t* first,
                                          const uint8_t* digests, const uint32_t* sizes, uint64_t n_blocks,
                                          uint64_t max_run_bytes, uint8_t* out) {
  ServePlan p;
  uint64_t blocks = 0, block_bytes = 0, name_bytes = 0;
  for (uint64_t k = 0; k < n; k++) {
    const uint8_t* name = req + name_at[k];
    if (!utf8_ok(name, name_len[k])) { p.why = kServeBadName; break; }
    if (rows[k] < 0) { p.why = kServeUnknown; break; }
    const uint64_t r = (uint64_t)rows[k];
    if (!serve_row_ok(first, n_blocks, r)) { p.bad_row = r; break; }
    uint64_t bytes = 0;
    for (uint64_t i = first[r]; i < first[r + 1]; i++) bytes += file_block_len(sizes[i]);
    const uint64_t cnt = first[r + 1] - first[r];
    if (serve_over(blocks + cnt, block_bytes + bytes, name_bytes + name_len[k], k + 1, max_run_bytes)) {
      p.why = kServeFull;
      break;
    }
    if (out) {
      uint8_t* o = out + files_run_total(block_bytes, name_bytes, k);
      o += write_file_start(o, name, name_len[k]);
      for (uint64_t i = first[r]; i < first[r + 1]; i++) o += write_file_block(o, digests + kDigest * i, sizes[i]);
      write_file_end(o);
    }
    blocks += cnt;
    block_bytes += bytes;
    name_bytes += name_len[k];
    p.n_answered = k + 1;
    p.answered_bytes = name_at[k] + name_len[k] + 1;
  }
  p.total = files_run_total(block_bytes, name_bytes, p.n_answered);
  p.messages = blocks + 2 * p.n_answered;
  return p;
}

}  // namespace sfwp
