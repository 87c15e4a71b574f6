// sf_wire_entries.hpp -- the framing rules of the first phase of a sync, the
// exchange of the files list (src/sync/fs.rs:133-164 sends it, fs.rs:378-446
// takes it): one FILE_ENTRY per file, then END_FILES, and the destination's
// GET_FILE requests for the files it needs.  Beside sf_wire_files.hpp and built
// on sf_wire_parse.hpp's pieces: one entry at a known start (entry_message),
// what stands at a stop (classify_entries), the serial parse of a whole buffer
// (parse_entries_run) -- the definition, the fallback and the forced-host route
// of sf_receive_file_entries_device -- Rust's String::from_utf8 (utf8_ok), the
// three messages' lengths and writers with the test of what the protocol can
// carry (entry_ok, pick_ok), their serial definitions, and the hash of a name
// that the name set's host and device code share (name_hash).
//
//   FILE_ENTRY  "FILE_ENTRY\n" + 0..100 name bytes holding no '\n' + "\n" +
//               a size field of 1..15 bytes + "\n" + 20 raw bytes + "\n"    35..149 bytes
//   END_FILES   "END_FILES\n"                                               10
//   GET_FILE    "GET_FILE\n" + name + "\n"                                  10 + name
//
// No HIP and no library header here (tests/native/wire_entries.cpp tests it on
// a CPU).  Everything but the classes and the serial definitions is constexpr:
// the kernels of sf_recv_entries.hip, sf_send_entries.hip and sf_names.hip call
// the same functions, so host and device cannot disagree.
#pragma once
#include "sf_wire_send_files.hpp"

namespace sfwp {

// SF_WIRE_END_FILES of include/syncfast_amd.h: "END_FILES\n" stood after the
// last entry and is counted in the consumed bytes.
constexpr int kEndFiles = 5;
// Not a stop: a whole FILE_ENTRY (classify_entries).
constexpr int kEntry = kHeader;

constexpr uint32_t kEntryTag = 11, kEndFilesTag = 10, kGetFileTag = 9;  // "FILE_ENTRY\n", "END_FILES\n", "GET_FILE\n"
constexpr uint32_t kMinEntry = kEntryTag + 1 + 2 + kDigest + 1;                                 // 35
constexpr uint32_t kMaxEntry = kEntryTag + kNameMax + 1 + kSizeMax + 1 + kDigest + 1;           // 149
constexpr uint32_t kEntriesTail = 152;  // bytes at a stop that decide its class (149 and room to spare)
constexpr uint64_t kEntrySizeLimit = 1000000000000000ull;  // 10^15: the first size whose field has 16 digits

constexpr bool is_entry_tag(const uint8_t* b) {
  return (b[0] == 'F') & (b[1] == 'I') & (b[2] == 'L') & (b[3] == 'E') & (b[4] == '_') & (b[5] == 'E') &
         (b[6] == 'N') & (b[7] == 'T') & (b[8] == 'R') & (b[9] == 'Y') & (b[10] == '\n');
}

constexpr bool is_end_files(const uint8_t* b) {
  return (b[0] == 'E') & (b[1] == 'N') & (b[2] == 'D') & (b[3] == '_') & (b[4] == 'F') & (b[5] == 'I') &
         (b[6] == 'L') & (b[7] == 'E') & (b[8] == 'S') & (b[9] == '\n');
}

// A whole, valid FILE_ENTRY at b, of which `avail` bytes may be read: its
// length (35 to 149) with the name's length in *name_len and the size field's
// value in *size, else 0.  Reads no byte at or past b + avail.  The name is
// the name_len bytes at b + 11, the hash the 20 bytes at b + length - 21.
constexpr uint32_t entry_message(const uint8_t* b, uint64_t avail, uint32_t* name_len, uint64_t* size) {
  if (avail < kMinEntry || !is_entry_tag(b)) return 0;
  const uint64_t left = avail - kEntryTag;
  const uint32_t room = left > kNameMax + 1 ? kNameMax + 1 : (uint32_t)left;
  uint32_t n = 0;
  while (n < room && b[kEntryTag + n] != '\n') n++;
  if (n == room) return 0;
  const uint32_t s = kEntryTag + n + 1;
  const uint32_t f = size_field(b + s, avail - s, size);
  if (!f) return 0;
  const uint32_t d = s + f;
  if (avail - d < kDigest + 1 || b[d + kDigest] != '\n') return 0;
  *name_len = n;
  return d + kDigest + 1;
}

// What stands at b (avail bytes to the end of the buffer, of which the first
// min(avail, 149) are read), as the parser rules it: kEntry with its length,
// name length and size, kEndFiles with *len = 10, or kEnd (nothing),
// kIncomplete (a prefix that more bytes could complete), kOther (the complete
// command line of one of the other seven commands, whatever follows it) or
// kMalformed (the parser raises: "Unterminated command", "Unknown command",
// "Unterminated filename" with 100 name bytes and no newline among 101,
// "Unterminated size" with 15 and none among 16, "Invalid file size",
// "Unterminated digest" with another byte than '\n' behind the 20).  The
// parser reads field after field, so a bad size raises before the digest has
// arrived.
inline int classify_entries(const uint8_t* b, uint64_t avail, uint32_t* len, uint32_t* name_len, uint64_t* size) {
  *len = 0;
  if (avail == 0) return kEnd;
  bool raise = false;
  const int c = line_end(b, avail, kCommandMax, &raise);
  if (c < 0) return raise ? kMalformed : kIncomplete;
  if (c == (int)kEndFilesTag - 1 && memcmp(b, "END_FILES", kEndFilesTag - 1) == 0) {
    *len = kEndFilesTag;
    return kEndFiles;
  }
  if (c != (int)kEntryTag - 1 || memcmp(b, "FILE_ENTRY", kEntryTag - 1) != 0)
    return is_command(b, (size_t)c) ? kOther : kMalformed;
  const int e = line_end(b + kEntryTag, avail - kEntryTag, kNameMax, &raise);
  if (e < 0) return raise ? kMalformed : kIncomplete;
  const uint32_t s = kEntryTag + (uint32_t)e + 1;
  const int z = line_end(b + s, avail - s, kSizeMax, &raise);
  if (z < 0) return raise ? kMalformed : kIncomplete;
  if (!size_value(b + s, (uint32_t)z, size)) return kMalformed;
  const uint32_t d = s + (uint32_t)z + 1;
  if (avail - d < kDigest + 1) return kIncomplete;
  if (b[d + kDigest] != '\n') return kMalformed;
  *name_len = (uint32_t)e;
  *len = d + kDigest + 1;
  return kEntry;
}

// The outputs of parse_entries_run: one row per entry; every list may be NULL
// with cap = 0.
struct EntriesOut {
  uint64_t* name_at;   // [cap] the name's first byte in the buffer
  uint32_t* name_len;  // [cap]
  uint64_t* sizes;     // [cap]
  uint8_t* hashes;     // [cap][20]
  uint64_t cap;
};

struct EntriesParsed {
  uint64_t count = 0, consumed = 0;
  int stop = kEnd;
};

// The buffer at b[0, n), entry after entry as the reference parser reads it:
// the first min(count, cap) rows are written, r->stop = what stands after the
// entries; kEndFiles: "END_FILES\n" stood there and is among r->consumed.
inline void parse_entries_run(const uint8_t* b, uint64_t n, const EntriesOut& o, EntriesParsed* r) {
  uint64_t p = 0, k = 0;
  for (;;) {
    uint32_t len = 0, name_len = 0;
    uint64_t size = 0;
    const int c = classify_entries(b + p, n - p, &len, &name_len, &size);
    if (c != kEntry) {
      if (c == kEndFiles) p += len;
      r->stop = c;
      break;
    }
    if (k < o.cap) {
      o.name_at[k] = p + kEntryTag;
      o.name_len[k] = name_len;
      o.sizes[k] = size;
      memcpy(o.hashes + kDigest * k, b + p + len - kDigest - 1, kDigest);
    }
    p += len;
    k++;
  }
  r->count = k;
  r->consumed = p;
}

// Rust's String::from_utf8 on name[0, len): no overlong form, no surrogate,
// nothing above U+10FFFF, nothing truncated (core::str::from_utf8's table:
// C2..DF 80..BF | E0 A0..BF 80..BF | E1..EC, EE..EF 80..BF 80..BF |
// ED 80..9F 80..BF | F0 90..BF + 2 | F1..F3 80..BF + 2 | F4 80..8F + 2).
constexpr bool utf8_ok(const uint8_t* name, uint32_t len) {
  uint32_t i = 0;
  while (i < len) {
    const uint8_t c = name[i];
    if (c < 0x80) {
      i++;
      continue;
    }
    uint32_t more = 0;
    uint8_t lo = 0x80, hi = 0xBF;
    if (c >= 0xC2 && c <= 0xDF) more = 1;
    else if (c >= 0xE0 && c <= 0xEF) {
      more = 2;
      if (c == 0xE0) lo = 0xA0;
      if (c == 0xED) hi = 0x9F;
    } else if (c >= 0xF0 && c <= 0xF4) {
      more = 3;
      if (c == 0xF0) lo = 0x90;
      if (c == 0xF4) hi = 0x8F;
    } else {
      return false;
    }
    if (len - i <= more) return false;
    if (name[i + 1] < lo || name[i + 1] > hi) return false;
    for (uint32_t k = 2; k <= more; k++)
      if ((name[i + k] & 0xC0) != 0x80) return false;
    i += more + 1;
  }
  return true;
}

// ---- the writers ----

constexpr uint32_t digits10_64(uint64_t v) {
  uint32_t d = 1;
  while (v >= 10) { v /= 10; ++d; }
  return d;
}

constexpr uint32_t file_entry_len(uint32_t name_len, uint64_t size) { return 34 + name_len + digits10_64(size); }
constexpr uint32_t end_files_len() { return kEndFilesTag; }
constexpr uint32_t get_file_len(uint32_t name_len) { return kGetFileTag + name_len + 1; }

// "FILE_ENTRY\n" + name + "\n" + size in decimal + "\n" + hash[0, 20) + "\n" at o, byte stores.
constexpr uint32_t write_file_entry(uint8_t* o, const uint8_t* name, uint32_t len, uint64_t size,
                                    const uint8_t* hash) {
  const char tag[kEntryTag] = {'F', 'I', 'L', 'E', '_', 'E', 'N', 'T', 'R', 'Y', '\n'};
  for (uint32_t k = 0; k < kEntryTag; k++) o[k] = (uint8_t)tag[k];
  for (uint32_t k = 0; k < len; k++) o[kEntryTag + k] = name[k];
  uint32_t at = kEntryTag + len;
  o[at++] = '\n';
  const uint32_t nd = digits10_64(size);
  uint64_t v = size;
  for (uint32_t k = nd; k-- > 0;) { o[at + k] = (uint8_t)('0' + v % 10); v /= 10; }
  at += nd;
  o[at++] = '\n';
  for (uint32_t k = 0; k < kDigest; k++) o[at + k] = hash[k];
  o[at + kDigest] = '\n';
  return at + kDigest + 1;
}

constexpr uint32_t write_end_files(uint8_t* o) {
  const char tag[kEndFilesTag] = {'E', 'N', 'D', '_', 'F', 'I', 'L', 'E', 'S', '\n'};
  for (uint32_t k = 0; k < kEndFilesTag; k++) o[k] = (uint8_t)tag[k];
  return kEndFilesTag;
}

constexpr uint32_t write_get_file(uint8_t* o, const uint8_t* name, uint32_t len) {
  const char tag[kGetFileTag] = {'G', 'E', 'T', '_', 'F', 'I', 'L', 'E', '\n'};
  for (uint32_t k = 0; k < kGetFileTag; k++) o[k] = (uint8_t)tag[k];
  for (uint32_t k = 0; k < len; k++) o[kGetFileTag + k] = name[k];
  o[kGetFileTag + len] = '\n';
  return kGetFileTag + len + 1;
}

// Whether file f of a list can be sent as a FILE_ENTRY the peer's parser
// takes: its CSR entries hold (name_at[0] == 0, name_at[f] <= name_at[f + 1] <=
// name_at[n]), its name is name_ok (at most 100 bytes, no '\n') and its size is
// below 10^15 (a field of at most 15 digits).  One lane's test.
constexpr bool entry_ok(const uint8_t* names, const uint64_t* name_at, const uint64_t* sizes, uint64_t n, uint64_t f) {
  const uint64_t a0 = name_at[f], a1 = name_at[f + 1];
  if (f == 0 && a0 != 0) return false;
  if (a0 > a1 || a1 > name_at[n]) return false;
  if (sizes[f] >= kEntrySizeLimit) return false;
  const uint64_t len = a1 - a0;
  if (len > kNameMax) return false;
  if (len == 0) return true;
  return names && name_ok(names + a0, (uint32_t)len);
}

// Whether pick k of a GET_FILE run can be sent: its index is below n, its span
// lies in bytes[0, n_bytes), its name is name_ok.  pick == NULL: index k.
// *index = the index it names (when below n).
constexpr bool pick_ok(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* at, const uint32_t* len, uint64_t n,
                       const uint32_t* pick, uint64_t k, uint64_t* index) {
  const uint64_t i = pick ? pick[k] : k;
  if (i >= n) return false;
  *index = i;
  const uint64_t a = at[i], l = len[i];
  if (a > n_bytes || l > n_bytes - a || l > kNameMax) return false;
  return l == 0 || name_ok(bytes + a, (uint32_t)l);
}

// ---- the serial definitions of the two runs ----

// The first file whose entries do not hold, kNoFile when all do.
inline uint64_t first_bad_entry(const uint8_t* names, const uint64_t* name_at, const uint64_t* sizes, uint64_t n) {
  for (uint64_t f = 0; f < n; f++)
    if (!entry_ok(names, name_at, sizes, n, f)) return f;
  return kNoFile;
}

// The whole list at out (NULL: only the length is returned), for entries that
// hold: every FILE_ENTRY and, with end_files, "END_FILES\n".
inline uint64_t build_entries_run_serial(const uint8_t* names, const uint64_t* name_at, const uint64_t* sizes,
                                         const uint8_t* hashes, uint64_t n, bool end_files, uint8_t* out) {
  uint64_t at = 0;
  for (uint64_t f = 0; f < n; f++) {
    const uint32_t len = (uint32_t)(name_at[f + 1] - name_at[f]);
    if (out) write_file_entry(out + at, len ? names + name_at[f] : names, len, sizes[f], hashes + kDigest * f);
    at += file_entry_len(len, sizes[f]);
  }
  if (end_files) {
    if (out) write_end_files(out + at);
    at += kEndFilesTag;
  }
  return at;
}

inline uint64_t first_bad_pick(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* at, const uint32_t* len,
                               uint64_t n, const uint32_t* pick, uint64_t n_pick) {
  uint64_t i = 0;
  for (uint64_t k = 0; k < n_pick; k++)
    if (!pick_ok(bytes, n_bytes, at, len, n, pick, k, &i)) return k;
  return kNoFile;
}

inline uint64_t build_get_files_run_serial(const uint8_t* bytes, const uint64_t* at, const uint32_t* len,
                                           const uint32_t* pick, uint64_t n_pick, uint8_t* out) {
  uint64_t o = 0;
  for (uint64_t k = 0; k < n_pick; k++) {
    const uint64_t i = pick ? pick[k] : k;
    if (out) write_get_file(out + o, bytes + at[i], len[i]);
    o += get_file_len(len[i]);
  }
  return o;
}

// ---- the name hash ----

// 64-bit FNV-1a over the name's bytes, finished with a 64-bit mix (so that
// the low bits, which choose the slot, depend on every byte), then ANDed with
// `mask` unless that is 0 (SF_TEST_NAME_HASH_MASK: the tests put every name
// into a few probe sequences).  The slot comes from the low bits, the
// fingerprint kept beside a row id from bits 40..63.
constexpr uint64_t name_hash(const uint8_t* name, uint64_t len, uint64_t mask) {
  uint64_t h = 0xCBF29CE484222325ull;
  for (uint64_t k = 0; k < len; k++) h = (h ^ name[k]) * 0x100000001B3ull;
  h ^= h >> 33;
  h *= 0xFF51AFD7ED558CCDull;
  h ^= h >> 33;
  h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 33;
  return mask ? h & mask : h;
}

}  // namespace sfwp
