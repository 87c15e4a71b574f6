// sf_wire_files.hpp -- the framing rules of the reference's message parser
// (src/sync/ssh/proto.rs:189-477, mirrored by syncfast_amd/wire.py's Parser)
// and the order its sink accepts (src/sync/fs.rs:449-500) for a whole
// GetFiles stream: any number of files, each FILE_START + FILE_BLOCK* +
// FILE_END, back to back in one buffer that may begin and end anywhere.
// Beside sf_wire_parse.hpp's rules for one file's FILE_BLOCK run and built on
// its pieces: one message at a known start (files_message), what stands at a
// stop (classify_files), which message may follow which (accepts) and the
// serial parse of a whole buffer (parse_files_run) -- the definition, the
// fallback and the forced-host route of sf_receive_files_device.
//
//   FILE_START  "FILE_START\n" + 0..100 name bytes holding no '\n' + "\n"   12..112 bytes
//   FILE_BLOCK  exactly what block_message accepts                          34..48
//   FILE_END    "FILE_END\n"                                                9
//
// No HIP and no library header here (tests/native/wire_files.cpp tests it on
// a CPU).  files_message is constexpr: the kernels of sf_recv_files.hip call
// the same function, so host and device cannot disagree about what a message
// is.
#pragma once
#include "sf_wire_parse.hpp"

namespace sfwp {

// SF_WIRE_UNEXPECTED of include/syncfast_amd.h: a whole, valid message of the
// three kinds stands there and the sink's state does not take it.
constexpr int kUnexpected = 4;
// Not a stop: a whole message of one of the three kinds (classify_files).
constexpr int kMessage = kHeader;

constexpr uint32_t kStart = 1, kFileBlock = 2, kFileEnd = 3;  // a message's kind

constexpr uint32_t kNameMax = 100;                                     // FILENAME_MAX of proto.rs:250
constexpr uint32_t kStartTag = 11, kEndTag = 9;                        // "FILE_START\n", "FILE_END\n"
constexpr uint32_t kMinFiles = kEndTag, kMaxFiles = kStartTag + kNameMax + 1;  // 9, 112
constexpr uint32_t kFilesTail = kMaxFiles + 1;  // bytes at a stop that decide its class

constexpr bool is_start_tag(const uint8_t* b) {
  return (b[0] == 'F') & (b[1] == 'I') & (b[2] == 'L') & (b[3] == 'E') & (b[4] == '_') & (b[5] == 'S') &
         (b[6] == 'T') & (b[7] == 'A') & (b[8] == 'R') & (b[9] == 'T') & (b[10] == '\n');
}

constexpr bool is_end_tag(const uint8_t* b) {
  return (b[0] == 'F') & (b[1] == 'I') & (b[2] == 'L') & (b[3] == 'E') & (b[4] == '_') & (b[5] == 'E') &
         (b[6] == 'N') & (b[7] == 'D') & (b[8] == '\n');
}

// A whole, valid message of one of the three kinds at b, of which `avail`
// bytes may be read: its length with its kind in *kind (and, for a
// FILE_BLOCK, its size in *size), else 0.  Reads no byte at or past
// b + avail.  The name's newline is searched among the first 101 bytes after
// the tag (read_line(FILENAME_MAX), proto.rs:271-290).
constexpr uint32_t files_message(const uint8_t* b, uint64_t avail, uint32_t* kind, uint64_t* size) {
  if (avail < kMinFiles) return 0;
  if (b[5] == 'B') {
    *kind = kFileBlock;
    return block_message(b, avail, size);
  }
  if (b[5] == 'E') {
    *kind = kFileEnd;
    return is_end_tag(b) ? kEndTag : 0;
  }
  if (avail < kStartTag + 1 || !is_start_tag(b)) return 0;
  *kind = kStart;
  const uint64_t left = avail - kStartTag;
  const uint32_t room = left > kNameMax + 1 ? kNameMax + 1 : (uint32_t)left;
  for (uint32_t n = 0; n < room; n++)
    if (b[kStartTag + n] == '\n') return kStartTag + n + 1;
  return 0;
}

// Whether the sink takes a message of `kind` in state `open` (a file is open:
// its FILE_START was read and its FILE_END was not): FILE_START only with no
// file open, FILE_BLOCK and FILE_END only with one (fs.rs:450-499; anything
// else is "Unexpected message from source").  For two adjacent messages:
// accepts(first != kFileEnd, second) -- START->BLOCK, START->END,
// BLOCK->BLOCK, BLOCK->END and END->START are the good pairs.
constexpr bool accepts(bool open, uint32_t kind) { return (kind == kStart) != open; }

// What stands at b (avail bytes to the end of the buffer, of which the first
// min(avail, 112) are read), as the parser rules it: kMessage with its kind,
// length and size, or kEnd (nothing), kIncomplete (a prefix that more bytes
// could complete), kOther (the complete command line of one of the other six
// commands, whatever follows it) or kMalformed (the parser raises: with 100
// name bytes or more and no newline among the first 101 it gives
// "Unterminated filename", it does not wait).
inline int classify_files(const uint8_t* b, uint64_t avail, uint32_t* kind, uint32_t* len, uint64_t* size) {
  *len = 0;
  *kind = 0;
  if (avail == 0) return kEnd;
  bool raise = false;
  const int c = line_end(b, avail, kCommandMax, &raise);
  if (c < 0) return raise ? kMalformed : kIncomplete;  // "Unterminated command"
  if (c == (int)kEndTag - 1 && memcmp(b, "FILE_END", kEndTag - 1) == 0) {
    *kind = kFileEnd;
    *len = kEndTag;
    return kMessage;
  }
  if (c == (int)kStartTag - 1 && memcmp(b, "FILE_START", kStartTag - 1) == 0) {
    const int e = line_end(b + kStartTag, avail - kStartTag, kNameMax, &raise);
    if (e < 0) return raise ? kMalformed : kIncomplete;  // "Unterminated filename"
    *kind = kStart;
    *len = kStartTag + (uint32_t)e + 1;
    return kMessage;
  }
  const int h = header(b, avail, "FILE_BLOCK", len, size);
  if (h == kHeader) *kind = kFileBlock;
  return h;
}

// The outputs of parse_files_run: block rows and file rows (sections), each
// list may be NULL with its cap = 0.  first has file_cap + 1 entries.
struct FilesOut {
  uint8_t* digests;      // [block_cap][20]
  uint32_t* sizes;       // [block_cap]
  uint64_t* offsets;     // [block_cap] the running offset within the block's file
  uint32_t* block_file;  // [block_cap] the block's section
  uint64_t block_cap;
  uint64_t* name_at;   // [file_cap] the name's first byte in the buffer; UINT64_MAX for a section carried in
  uint32_t* name_len;  // [file_cap]
  uint64_t* first;     // [file_cap + 1] the section's first block; entry n_files = n_blocks
  uint64_t* file_size; // [file_cap] the running offset at the section's end
  uint64_t file_cap;
};

struct FilesParsed {
  uint64_t n_blocks = 0, n_files = 0, messages = 0, consumed = 0, end_offset = 0;
  int stop = kEnd;
  bool open = false, too_large = false;
};

// The buffer at b[0, n), message after message as the reference parser reads
// it and its sink takes it, from the state carried in: `open` with the open
// file's running offset `base_offset` (section 0 then: no name, offsets from
// base_offset; it exists even with no message).  Every FILE_START opens the
// next section; a FILE_BLOCK gets its section and the running offset of
// fs.rs:477; FILE_END closes the section.  The first min(count, cap) rows of
// each list are written; first[n_files] = n_blocks when n_files <= file_cap.
// r->stop = what stands after the accepted messages (kUnexpected: a whole
// message the state does not take), r->open / r->end_offset = the state to
// carry on with.  r->too_large: a size above 2^32 - 1 was met (its entry
// holds the low 32 bits).
inline void parse_files_run(const uint8_t* b, uint64_t n, bool open, uint64_t base_offset, const FilesOut& o,
                            FilesParsed* r) {
  uint64_t p = 0, nb = 0, nf = 0, nm = 0, run = open ? base_offset : 0;
  auto section = [&](uint64_t at, uint32_t len) {
    if (nf < o.file_cap) {
      o.name_at[nf] = at;
      o.name_len[nf] = len;
      o.first[nf] = nb;
      o.file_size[nf] = 0;
    }
    nf++;
  };
  if (open) {
    section(UINT64_MAX, 0);
    if (o.file_cap) o.file_size[0] = run;
  }
  r->too_large = false;
  for (;;) {
    uint32_t kind = 0, len = 0;
    uint64_t size = 0;
    const int c = classify_files(b + p, n - p, &kind, &len, &size);
    if (c != kMessage) {
      r->stop = c;
      break;
    }
    if (!accepts(open, kind)) {
      r->stop = kUnexpected;
      break;
    }
    if (kind == kStart) {
      section(p + kStartTag, len - kStartTag - 1);
      open = true;
      run = 0;
    } else if (kind == kFileBlock) {
      if (size > 0xFFFFFFFFull) r->too_large = true;
      if (nb < o.block_cap) {
        memcpy(o.digests + kDigest * nb, b + p + kTag, kDigest);
        o.sizes[nb] = (uint32_t)size;
        o.offsets[nb] = run;
        o.block_file[nb] = (uint32_t)(nf - 1);
      }
      nb++;
      run += size;
      if (nf <= o.file_cap) o.file_size[nf - 1] = run;
    } else {
      open = false;
    }
    p += len;
    nm++;
  }
  if (nf <= o.file_cap && o.first) o.first[nf] = nb;
  r->n_blocks = nb;
  r->n_files = nf;
  r->messages = nm;
  r->consumed = p;
  r->open = open;
  r->end_offset = nf ? run : base_offset;
}

}  // namespace sfwp
