// sf_wire_send_files.hpp -- the framing rules of the source's answer to a list
// of GET_FILE requests, the sending side of sf_wire_files.hpp.  The
// reference's source answers file after file: "FILE_START\n" + name + "\n",
// one FILE_BLOCK per block, "FILE_END\n" (src/sync/fs.rs:177-231, written by
// write_message, src/sync/ssh/proto.rs:157-169).  Here: which names the
// protocol can carry (name_ok), the three messages' lengths and writers, where
// every message of a whole answer stands (start_at, block_at, end_at, total),
// which file a block belongs to (file_of_block), what makes a file's entries
// bad (file_ok), and the serial definition of the whole run
// (build_files_run_serial).
//
//   FILE_START  12 + name bytes          kStartTag + name + "\n"
//   FILE_BLOCK  33 + digits(size)        as sf_wire.hip writes it
//   FILE_END    9
//
// The files are a CSR over the block table (first[0, n_files], file f owns
// blocks [first[f], first[f + 1])) and a CSR over the packed name bytes
// (name_at[0, n_files], file f's name is names[name_at[f], name_at[f + 1])).
// With E[i] the inclusive end offsets of the FILE_BLOCK messages alone -- the
// scan sf_wire.hip's plan already gives -- and Bex(i) = i ? E[i - 1] : 0, every
// message's place follows without a second scan: before file f's FILE_START
// stand Bex(first[f]) block bytes, name_at[f] name bytes and f pairs of
// FILE_START's 12 and FILE_END's 9 fixed bytes.
//
// No HIP and no library header here (tests/native/send_files.cpp tests it on a
// CPU).  Everything but the serial definition is constexpr: the kernels of
// sf_send_files.hip call the same functions, so host and device cannot
// disagree about where a message stands or what it holds.
#pragma once
#include "sf_wire_data.hpp"
#include "sf_wire_files.hpp"

namespace sfwp {

constexpr uint32_t kStartFixed = kStartTag + 1;        // 12: FILE_START without its name
constexpr uint32_t kFileFixed = kStartFixed + kEndTag;  // 21: a file's bytes beside names and blocks
constexpr uint64_t kNoFile = ~0ull;

// The names a GET_FILE can have carried and a FILE_START can carry
// (read_line(FILENAME_MAX), proto.rs:271-290): at most 100 bytes, no '\n'.
constexpr bool name_ok(const uint8_t* name, uint32_t len) {
  if (len > kNameMax) return false;
  bool ok = true;
  for (uint32_t k = 0; k < len; k++) ok &= name[k] != '\n';
  return ok;
}

constexpr uint32_t file_start_len(uint32_t name_len) { return kStartFixed + name_len; }
constexpr uint32_t file_end_len() { return kEndTag; }
constexpr uint32_t file_block_len(uint32_t size) { return kSizeAt + digits10(size) + 1; }

// Bytes of FILE_BLOCK messages before block i.
constexpr uint64_t bex(const uint64_t* E, uint64_t i) { return i ? E[i - 1] : 0; }

constexpr uint64_t start_at(const uint64_t* E, const uint64_t* first, const uint64_t* name_at, uint64_t f) {
  return bex(E, first[f]) + name_at[f] + (uint64_t)kFileFixed * f;
}
// Block i of file f.
constexpr uint64_t block_at(const uint64_t* E, const uint64_t* name_at, uint64_t f, uint64_t i) {
  return bex(E, i) + name_at[f + 1] + (uint64_t)kFileFixed * f + kStartFixed;
}
constexpr uint64_t end_at(const uint64_t* E, const uint64_t* first, const uint64_t* name_at, uint64_t f) {
  return bex(E, first[f + 1]) + name_at[f + 1] + (uint64_t)kFileFixed * f + kStartFixed;
}
// The run's length from the three numbers that come back from the device.
constexpr uint64_t files_run_total(uint64_t block_bytes, uint64_t name_bytes, uint64_t n_files) {
  return block_bytes + name_bytes + (uint64_t)kFileFixed * n_files;
}

// The file of block i: the last f in [0, n_files) with first[f] <= i (an
// upper-bound search, so of several files that begin at i -- empty ones and
// the one that owns i -- the last is taken).  first[0] == 0 and n_files >= 1.
constexpr uint64_t file_of_block(const uint64_t* first, uint64_t n_files, uint64_t i) {
  uint64_t lo = 0, hi = n_files;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Whether file f's entries of the two CSRs hold: first[0] == 0, first[f] <=
// first[f + 1], first[n_files] == n_blocks; name_at[0] == 0, name_at[f] <=
// name_at[f + 1] <= name_at[n_files] (the names are name_at[n_files] bytes: no
// byte past them is read) and the name is name_ok (with names == NULL only the
// empty name is).  One lane's test: it reads first[f, f + 1], name_at[f, f + 1],
// name_at[n_files] and, when all of that holds, the name's bytes.
constexpr bool file_ok(const uint64_t* first, const uint8_t* names, const uint64_t* name_at, uint64_t n_files,
                       uint64_t n_blocks, uint64_t f) {
  const uint64_t b0 = first[f], b1 = first[f + 1], a0 = name_at[f], a1 = name_at[f + 1];
  if (f == 0 && (b0 != 0 || a0 != 0)) return false;
  if (f + 1 == n_files && b1 != n_blocks) return false;
  if (b0 > b1 || a0 > a1 || a1 > name_at[n_files]) return false;
  const uint64_t len = a1 - a0;
  if (len > kNameMax) return false;
  if (len == 0) return true;
  return names && name_ok(names + a0, (uint32_t)len);
}

// "FILE_START\n" + name[0, len) + "\n" at o: 12 + len byte stores.
constexpr uint32_t write_file_start(uint8_t* o, const uint8_t* name, uint32_t len) {
  const char tag[kStartTag] = {'F', 'I', 'L', 'E', '_', 'S', 'T', 'A', 'R', 'T', '\n'};
  for (uint32_t k = 0; k < kStartTag; k++) o[k] = (uint8_t)tag[k];
  for (uint32_t k = 0; k < len; k++) o[kStartTag + k] = name[k];
  o[kStartTag + len] = '\n';
  return kStartFixed + len;
}

constexpr uint32_t write_file_end(uint8_t* o) {
  const char tag[kEndTag] = {'F', 'I', 'L', 'E', '_', 'E', 'N', 'D', '\n'};
  for (uint32_t k = 0; k < kEndTag; k++) o[k] = (uint8_t)tag[k];
  return kEndTag;
}

// "FILE_BLOCK\n" + digest[0, 20) + "\n" + size in decimal + "\n" at o
// (sf_wire.hip's wire_blocks_kernel writes the same bytes).
constexpr uint32_t write_file_block(uint8_t* o, const uint8_t* digest, uint32_t size) {
  const char tag[kTag] = {'F', 'I', 'L', 'E', '_', 'B', 'L', 'O', 'C', 'K', '\n'};
  for (uint32_t k = 0; k < kTag; k++) o[k] = (uint8_t)tag[k];
  for (uint32_t k = 0; k < kDigest; k++) o[kTag + k] = digest[k];
  o[kTag + kDigest] = '\n';
  const uint32_t nd = digits10(size);
  uint32_t v = size;
  for (uint32_t k = nd; k-- > 0;) { o[kSizeAt + k] = (uint8_t)('0' + v % 10); v /= 10; }
  o[kSizeAt + nd] = '\n';
  return kSizeAt + nd + 1;
}

// ---- the serial definition ----

// The first file whose entries do not hold, kNoFile when all do.
inline uint64_t first_bad_file(const uint64_t* first, const uint8_t* names, const uint64_t* name_at, uint64_t n_files,
                               uint64_t n_blocks) {
  for (uint64_t f = 0; f < n_files; f++)
    if (!file_ok(first, names, name_at, n_files, n_blocks, f)) return f;
  return kNoFile;
}

// E[0, n_blocks): the inclusive end offsets of the FILE_BLOCK messages alone.
inline void file_block_ends(const uint32_t* sizes, uint64_t n_blocks, uint64_t* E) {
  uint64_t at = 0;
  for (uint64_t i = 0; i < n_blocks; i++) E[i] = at += file_block_len(sizes[i]);
}

// The whole answer, message by message at its formula's place: out[0, total)
// with total returned, for CSRs that hold (first_bad_file == kNoFile) and E
// from file_block_ends.  Every byte of out[0, total) is written exactly once.
inline uint64_t build_files_run_serial(const uint8_t* digests, const uint32_t* sizes, uint64_t n_blocks,
                                       const uint64_t* first, const uint8_t* names, const uint64_t* name_at,
                                       uint64_t n_files, const uint64_t* E, uint8_t* out) {
  for (uint64_t f = 0; f < n_files; f++) {
    const uint32_t len = (uint32_t)(name_at[f + 1] - name_at[f]);
    write_file_start(out + start_at(E, first, name_at, f), len ? names + name_at[f] : names, len);
    for (uint64_t i = first[f]; i < first[f + 1]; i++)
      write_file_block(out + block_at(E, name_at, f, i), digests + kDigest * i, sizes[i]);
    write_file_end(out + end_at(E, first, name_at, f));
  }
  return files_run_total(bex(E, n_blocks), n_files ? name_at[n_files] : 0, n_files);
}

}  // namespace sfwp
