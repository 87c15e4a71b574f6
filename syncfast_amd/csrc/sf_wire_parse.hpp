// sf_wire_parse.hpp -- the framing rules of the reference's message parser
// (src/sync/ssh/proto.rs:189-477, mirrored by syncfast_amd/wire.py's Parser)
// for a run of FILE_BLOCK messages, restated in C++: one message at a known
// start (block_message), what stops a run (classify, through header, which
// reads a BLOCK_DATA header for sf_wire_data.hpp too) and the serial parse of
// a whole run on the host (parse_run) -- the fallback of
// sf_wire_parse_blocks_device and the parser of sf_receive_blocks_buffer's.
//
// No HIP and no library header here, so a stand-alone program can test it on
// a CPU (tests/native/wire_parse.cpp).  block_message is constexpr: the
// device parser (sf_recv.hip) calls the same function from its kernels, so
// host and device cannot disagree about what a message is.
#pragma once
#include <stdint.h>
#include <string.h>

namespace sfwp {

// SF_WIRE_* of include/syncfast_amd.h
constexpr int kEnd = 0, kIncomplete = 1, kOther = 2, kMalformed = 3;
// Not a stop: a whole header of the run's own tag stands there (header);
// for a FILE_BLOCK run that is a whole message (classify only).
constexpr int kHeader = -1, kBlock = kHeader;

// Limits of the reference parser (proto.rs:249-251) and what follows from
// them: "FILE_BLOCK\n" + 20 digest bytes + "\n" + a size field of 1 to 15
// bytes + "\n".
constexpr uint32_t kCommandMax = 20, kSizeMax = 15, kDigest = 20, kTag = 11;
constexpr uint32_t kSizeAt = kTag + kDigest + 1;  // 32: the size field's first byte
constexpr uint32_t kMinMessage = kSizeAt + 2, kMaxMessage = kSizeAt + kSizeMax + 1;  // 34, 48

// (& and not &&: the eleven loads do not wait for one another on the device)
constexpr bool is_tag(const uint8_t* b) {
  return (b[0] == 'F') & (b[1] == 'I') & (b[2] == 'L') & (b[3] == 'E') & (b[4] == '_') & (b[5] == 'B') &
         (b[6] == 'L') & (b[7] == 'O') & (b[8] == 'C') & (b[9] == 'K') & (b[10] == '\n');
}

// The size field f[0, n) as Rust's usize::from_str reads it: "+"? [0-9]+
// (n <= 15, so the value is below 2^64).  false: "Invalid block size".
constexpr bool size_value(const uint8_t* f, uint32_t n, uint64_t* value) {
  uint32_t i = n && f[0] == '+' ? 1u : 0u;
  if (i == n) return false;
  uint64_t v = 0;
  for (; i < n; i++) {
    if (f[i] < '0' || f[i] > '9') return false;
    v = v * 10 + (uint64_t)(f[i] - '0');
  }
  *value = v;
  return true;
}

// A terminated, valid size field at f, of which avail bytes may be read: its
// bytes with the newline (2 to 16) and its value in *size, else 0.
constexpr uint32_t size_field(const uint8_t* f, uint64_t avail, uint64_t* size) {
  const uint32_t room = avail > kSizeMax + 1 ? kSizeMax + 1 : (uint32_t)avail;
  uint32_t n = 0;
  while (n < room && f[n] != '\n') n++;
  if (n == room || !size_value(f, n, size)) return 0;
  return n + 1;
}

// A whole, valid FILE_BLOCK message at b, of which `avail` bytes may be read:
// its length (34 to 48) with its size in *size, else 0.  Reads no byte at or
// past b + avail.
constexpr uint32_t block_message(const uint8_t* b, uint64_t avail, uint64_t* size) {
  if (avail < kMinMessage) return 0;
  if (!(is_tag(b) & (b[kTag + kDigest] == '\n'))) return 0;
  const uint32_t f = size_field(b + kSizeAt, avail - kSizeAt, size);
  return f ? kSizeAt + f : 0;
}

// The parser's read of one line: the index of the first '\n' among the first
// min(avail, limit + 1) bytes, or -1 with *raise = whether the parser gives up
// ("Unterminated ...": `limit` bytes without one) or waits for more.
inline int line_end(const uint8_t* b, uint64_t avail, uint32_t limit, bool* raise) {
  const uint32_t room = avail > limit + 1 ? limit + 1 : (uint32_t)avail;
  for (uint32_t i = 0; i < room; i++)
    if (b[i] == '\n') return (int)i;
  *raise = avail >= limit;
  return -1;
}

// Whether the c bytes at b are one of the parser's nine command names.
inline bool is_command(const uint8_t* b, size_t c) {
  static const char* const commands[9] = {"FILE_ENTRY", "END_FILES",  "GET_FILE",   "FILE_START", "FILE_END",
                                          "GET_BLOCK",  "FILE_BLOCK", "BLOCK_DATA", "COMPLETE"};
  for (const char* o : commands)
    if (strlen(o) == c && memcmp(b, o, c) == 0) return true;
  return false;
}

// The header at b, read from its first min(avail, 48) bytes alone (avail: the
// bytes to the end of the buffer), for a run of `tag` messages ("FILE_BLOCK"
// or "BLOCK_DATA": ten bytes, digest and size field laid out alike): kHeader
// with its length and the value of its size field when a whole valid header
// of that tag stands there, else why the run stops here.  The other of the
// two tags is one of the other commands then.
inline int header(const uint8_t* b, uint64_t avail, const char* tag, uint32_t* len, uint64_t* size) {
  *len = 0;
  if (avail == 0) return kEnd;
  bool raise = false;
  const int c = line_end(b, avail, kCommandMax, &raise);
  if (c < 0) return raise ? kMalformed : kIncomplete;  // "Unterminated command"
  if (c != (int)kTag - 1 || memcmp(b, tag, kTag - 1) != 0) {
    return is_command(b, (size_t)c) ? kOther : kMalformed;  // "Unknown command"
  }
  if (avail < kTag + kDigest + 1) return kIncomplete;
  if (b[kTag + kDigest] != '\n') return kMalformed;  // "Unterminated digest"
  const int s = line_end(b + kSizeAt, avail - kSizeAt, kSizeMax, &raise);
  if (s < 0) return raise ? kMalformed : kIncomplete;  // "Unterminated size" / "Unterminated length"
  if (!size_value(b + kSizeAt, (uint32_t)s, size)) return kMalformed;  // "Invalid block size" / "Invalid block length"
  *len = kSizeAt + (uint32_t)s + 1;
  return kHeader;
}

// What stands at b (avail bytes to the end of the buffer): kBlock with its
// length and size, or why a FILE_BLOCK run stops here.
inline int classify(const uint8_t* b, uint64_t avail, uint32_t* len, uint64_t* size) {
  return header(b, avail, "FILE_BLOCK", len, size);
}

// The run at b[0, n), message after message as the reference parser reads it:
// the digests (20 B each) and sizes of the first min(count, cap) messages
// (both may be NULL with cap = 0), *count = the whole messages, *consumed =
// their bytes, *stop = what stands after them.  *too_large: a size above
// 2^32 - 1 was met (its entry holds the low 32 bits).
inline void parse_run(const uint8_t* b, uint64_t n, uint8_t* digests, uint32_t* sizes, uint64_t cap, uint64_t* count,
                      uint64_t* consumed, int* stop, bool* too_large) {
  uint64_t p = 0, k = 0;
  *too_large = false;
  for (;;) {
    uint32_t len = 0;
    uint64_t size = 0;
    const int c = classify(b + p, n - p, &len, &size);
    if (c != kBlock) {
      *stop = c;
      break;
    }
    if (size > 0xFFFFFFFFull) *too_large = true;
    if (k < cap) {
      memcpy(digests + kDigest * k, b + p + kTag, kDigest);
      sizes[k] = (uint32_t)size;
    }
    p += len;
    k++;
  }
  *count = k;
  *consumed = p;
}

}  // namespace sfwp
