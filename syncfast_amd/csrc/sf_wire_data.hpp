// sf_wire_data.hpp -- the framing rules of the reference's message parser
// (src/sync/ssh/proto.rs:419-446, written by :175-181; mirrored by
// syncfast_amd/wire.py's Parser) for a run of BLOCK_DATA messages, beside
// sf_wire_parse.hpp's for FILE_BLOCK runs and built on its pieces: one
// message at a known start (data_message), what stops a run (classify_data),
// the serial parse of a whole run (parse_data_run) and the exact chain over a
// list of candidate starts (walk_candidates).  Below them the sending side's
// rules: the length and the header writer of a BLOCK_DATA message (written by
// :175-181) and the serial definition of a run of GET_BLOCK requests.
//
// A message is "BLOCK_DATA\n" + 20 digest bytes + "\n" + a length field of 1
// to 15 bytes + "\n" (the header, H = 34 to 48 bytes) + `length` payload bytes
// + "\n": H + length + 1 bytes.  The payload is arbitrary: it may hold whole
// messages of its own.
//
// No HIP and no library header here (tests/native/wire_data.cpp tests it on a
// CPU).  data_message is constexpr: the kernels of sf_recv_data.hip call the
// same function, so host and device cannot disagree about what a message is.
#pragma once
#include "sf_wire_parse.hpp"

namespace sfwp {

// Not a stop: a whole BLOCK_DATA message (classify_data) or a whole header
// (data_header) stands there.
constexpr int kData = kHeader;

constexpr uint32_t kMinData = kMinMessage + 1;  // 35: an empty payload and its end byte

constexpr bool is_data_tag(const uint8_t* b) {
  return (b[0] == 'B') & (b[1] == 'L') & (b[2] == 'O') & (b[3] == 'C') & (b[4] == 'K') & (b[5] == '_') &
         (b[6] == 'D') & (b[7] == 'A') & (b[8] == 'T') & (b[9] == 'A') & (b[10] == '\n');
}

// A whole, valid BLOCK_DATA message at b, of which `avail` bytes may be read:
// its length H + size + 1 with the header's length in *H (34 to 48) and the
// payload's in *size, else 0.  Reads no byte at or past b + avail, and of the
// payload only the end byte after it.
constexpr uint64_t data_message(const uint8_t* b, uint64_t avail, uint32_t* H, uint64_t* size) {
  if (avail < kMinData) return 0;
  if (!(is_data_tag(b) & (b[kTag + kDigest] == '\n'))) return 0;
  const uint32_t f = size_field(b + kSizeAt, avail - kSizeAt, size);
  if (!f) return 0;
  const uint64_t h = kSizeAt + f;  // size < 10^15: no sum below overflows
  if (h + *size + 1 > avail) return 0;
  if (b[h + *size] != '\n') return 0;  // "Invalid data end byte"
  *H = (uint32_t)h;
  return h + *size + 1;
}

// The header at b, read from its first min(avail, 48) bytes alone (avail: the
// bytes to the end of the buffer): kData with its length and the payload's
// when a whole valid header stands there, else why a BLOCK_DATA run stops
// here -- FILE_BLOCK is one of the other commands now.
inline int data_header(const uint8_t* b, uint64_t avail, uint32_t* H, uint64_t* size) {
  return header(b, avail, "BLOCK_DATA", H, size);
}

// What stands at b (avail bytes to the end of the buffer): kData with the
// header's and the payload's length, or why the run stops here.  A whole
// header whose payload or end byte is not all there yet is kIncomplete with
// *need = the message's full length H + size + 1; *need is 0 otherwise.
inline int classify_data(const uint8_t* b, uint64_t avail, uint32_t* H, uint64_t* size, uint64_t* need) {
  *need = 0;
  const int c = data_header(b, avail, H, size);
  if (c != kData) return c;
  const uint64_t total = (uint64_t)*H + *size + 1;
  if (total > avail) {
    *need = total;
    return kIncomplete;
  }
  return b[*H + *size] == '\n' ? kData : kMalformed;  // "Invalid data end byte"
}

// The run at b[0, n), message after message as the reference parser reads it:
// the claimed digests (20 B each), payload sizes and payload offsets (from b)
// of the first min(count, cap) messages (the three may be NULL with cap = 0),
// *count = the whole messages, *consumed = their bytes, *stop and *need = what
// stands after them (classify_data).  *too_large: a size above 2^32 - 1 was
// met (its entry holds the low 32 bits).
inline void parse_data_run(const uint8_t* b, uint64_t n, uint8_t* digests, uint32_t* sizes, uint64_t* offsets,
                           uint64_t cap, uint64_t* count, uint64_t* consumed, int* stop, uint64_t* need,
                           bool* too_large) {
  uint64_t p = 0, k = 0;
  *too_large = false;
  for (;;) {
    uint32_t H = 0;
    uint64_t size = 0;
    const int c = classify_data(b + p, n - p, &H, &size, need);
    if (c != kData) {
      *stop = c;
      break;
    }
    if (size > 0xFFFFFFFFull) *too_large = true;
    if (k < cap) {
      memcpy(digests + kDigest * k, b + p + kTag, kDigest);
      sizes[k] = (uint32_t)size;
      offsets[k] = p + H;
    }
    p += H + size + 1;
    k++;
  }
  *count = k;
  *consumed = p;
}

// The exact chain from byte 0 over a position-ordered list of candidates
// (every position where data_message holds, with its length): candidate 0
// must stand at byte 0; from a chained candidate at p of length L the next is
// the candidate that stands exactly at p + L, those below p + L (inside the
// message: payload bytes) are passed over; the chain ends where none stands
// there.  chain[k] = the list index of message k (chain may be NULL to
// count); returns the messages.  Linear in count; touches no wire byte.
inline uint64_t walk_candidates(const uint64_t* pos, const uint64_t* len, uint64_t count, uint64_t* chain) {
  if (count == 0 || pos[0] != 0) return 0;
  uint64_t k = 0, i = 0;
  for (;;) {
    if (chain) chain[k] = i;
    k++;
    const uint64_t next = pos[i] + len[i];
    uint64_t j = i + 1;
    while (j < count && pos[j] < next) j++;
    if (j == count || pos[j] != next) return k;
    i = j;
  }
}

// ---- the sending side: BLOCK_DATA messages written, GET_BLOCK runs read ----
// (sf_send.hip's kernels call the constexpr functions; tests/native/
// block_data_write.cpp runs all of them on a CPU)

constexpr uint32_t digits10(uint32_t v) {
  uint32_t d = 1;
  while (v >= 10) { v /= 10; ++d; }
  return d;
}

// Header and whole message of a payload of `size` bytes as write_message
// writes them (proto.rs:175-181): 11 for the tag, 20 for the digest, 1, the
// decimal size, 1; then the payload and 1.
constexpr uint32_t block_data_header_len(uint32_t size) { return kSizeAt + digits10(size) + 1; }
constexpr uint64_t block_data_len(uint32_t size) { return (uint64_t)block_data_header_len(size) + size + 1; }

// Everything of a message but its payload, byte stores only: the header at
// `head` ("BLOCK_DATA\n" + digest[0, 20) + "\n" + size in decimal + "\n") and
// the "\n" that ends the message at `end` (= head + header + size for a
// message in one piece).  Returns the header's length; no byte between
// head + that and `end` is touched.
constexpr uint32_t write_block_data(uint8_t* head, uint8_t* end, const uint8_t* digest, uint32_t size) {
  const char tag[kTag] = {'B', 'L', 'O', 'C', 'K', '_', 'D', 'A', 'T', 'A', '\n'};
  for (uint32_t k = 0; k < kTag; k++) head[k] = (uint8_t)tag[k];
  for (uint32_t k = 0; k < kDigest; k++) head[kTag + k] = digest[k];
  head[kTag + kDigest] = '\n';
  const uint32_t nd = digits10(size);
  uint32_t v = size;
  for (uint32_t k = nd; k-- > 0;) { head[kSizeAt + k] = (uint8_t)('0' + v % 10); v /= 10; }
  head[kSizeAt + nd] = '\n';
  *end = '\n';
  return kSizeAt + nd + 1;
}

// A GET_BLOCK message (proto.rs:170-174): "GET_BLOCK\n" + 20 digest bytes of
// any value + "\n", 31 bytes, so message k of a run stands at 31 k.
constexpr uint32_t kGetTag = 10, kGetBlock = kGetTag + kDigest + 1;

// The test one lane makes of one 31-byte slot: the tag line and the end byte.
constexpr bool is_get_block(const uint8_t* b) {
  return (b[0] == 'G') & (b[1] == 'E') & (b[2] == 'T') & (b[3] == '_') & (b[4] == 'B') & (b[5] == 'L') &
         (b[6] == 'O') & (b[7] == 'C') & (b[8] == 'K') & (b[9] == '\n') & (b[kGetTag + kDigest] == '\n');
}

// What stands at b (avail bytes to the end of the buffer, of which the first
// min(avail, 31) are read) in a run of GET_BLOCK messages: kHeader for a whole
// message, else why the run stops here.
inline int classify_get_block(const uint8_t* b, uint64_t avail) {
  if (avail == 0) return kEnd;
  bool raise = false;
  const int c = line_end(b, avail, kCommandMax, &raise);
  if (c < 0) return raise ? kMalformed : kIncomplete;  // "Unterminated command"
  if (c != (int)kGetTag - 1 || memcmp(b, "GET_BLOCK", kGetTag - 1) != 0)
    return is_command(b, (size_t)c) ? kOther : kMalformed;  // "Unknown command"
  if (avail < kGetBlock) return kIncomplete;
  return b[kGetTag + kDigest] == '\n' ? kHeader : kMalformed;  // "Unterminated digest"
}

// The run at b[0, n) as the reference parser reads it: *count = the leading
// GetBlock messages (their digests at b + 31 k + 10), *consumed = 31 * count,
// *stop = what stands after them.
inline void parse_get_block_run(const uint8_t* b, uint64_t n, uint64_t* count, uint64_t* consumed, int* stop) {
  uint64_t k = 0;
  int c;
  while ((c = classify_get_block(b + kGetBlock * k, n - kGetBlock * k)) == kHeader) k++;
  *count = k;
  *consumed = kGetBlock * k;
  *stop = c;
}

}  // namespace sfwp
