// wire_files.cpp -- the GetFiles framing rules (syncfast_amd/csrc/sf_wire_files.hpp)
// alone: a stand-alone program, built with ASan + UBSan by
// tests/test_wire_files.py and run directly.  No GPU, no library.
//
//   wire_files CASES    CASES holds records of <u32 open> <u64 base_offset>
//                       <u64 length> <length bytes> (little endian).  Each
//                       record's bytes are parsed by parse_files_run from a
//                       heap copy of their exact length into outputs of
//                       exactly the needed entries (a read or a write past
//                       either is an ASan report), again with each capacity
//                       one short and with none (the program fails unless the
//                       counts, the stop and the rows that fit are the same),
//                       and files_message is asked at every position.  Per
//                       record it prints
//                         R n_blocks n_files messages consumed stop open end_offset too_large
//                         B digest-hex size offset section          per block
//                         F name_at name_len first size             per section
//                         L first[n_files]
//                         C position length kind                    per candidate
//                       which the driver holds against its model of
//                       syncfast_amd.wire.Parser and the sink's rule.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../syncfast_amd/csrc/sf_wire_files.hpp"

namespace {

[[noreturn]] void die(const char* what, size_t record) {
  fprintf(stderr, "record %zu: %s\n", record, what);
  exit(1);
}

template <class T>
T* exact(uint64_t n) {  // n entries on the heap and not one more (NULL for none)
  return n ? static_cast<T*>(malloc(n * sizeof(T))) : nullptr;
}

struct Rows {
  uint64_t bcap, fcap;
  uint8_t* digests;
  uint32_t *sizes, *block_file, *name_len;
  uint64_t *offsets, *name_at, *first, *file_size;
  Rows(uint64_t b, uint64_t f, bool with_first)
      : bcap(b), fcap(f), digests(exact<uint8_t>(20 * b)), sizes(exact<uint32_t>(b)), block_file(exact<uint32_t>(b)),
        name_len(exact<uint32_t>(f)), offsets(exact<uint64_t>(b)), name_at(exact<uint64_t>(f)),
        first(with_first ? exact<uint64_t>(f + 1) : nullptr), file_size(exact<uint64_t>(f)) {}
  ~Rows() {
    free(digests); free(sizes); free(block_file); free(name_len);
    free(offsets); free(name_at); free(first); free(file_size);
  }
  sfwp::FilesOut out() const {
    return {digests, sizes, offsets, block_file, bcap, name_at, name_len, first, file_size, fcap};
  }
};

bool same_state(const sfwp::FilesParsed& a, const sfwp::FilesParsed& b) {
  return a.n_blocks == b.n_blocks && a.n_files == b.n_files && a.messages == b.messages && a.consumed == b.consumed &&
         a.end_offset == b.end_offset && a.stop == b.stop && a.open == b.open && a.too_large == b.too_large;
}

void record(size_t k, const uint8_t* bytes, uint64_t n, bool open, uint64_t base) {
  uint8_t* run = static_cast<uint8_t*>(malloc(n ? n : 1));
  if (n) memcpy(run, bytes, n);
  sfwp::FilesParsed q, r, s;
  sfwp::parse_files_run(run, n, open, base, sfwp::FilesOut{}, &q);  // the query form
  Rows full(q.n_blocks, q.n_files, true);
  sfwp::parse_files_run(run, n, open, base, full.out(), &r);
  if (!same_state(q, r)) die("the query form and the full form differ", k);
  for (int which = 0; which < 3; which++) {  // blocks one short, files one short, both
    const uint64_t b = q.n_blocks - (which != 1 && q.n_blocks), f = q.n_files - (which != 0 && q.n_files);
    Rows part(b, f, true);
    sfwp::parse_files_run(run, n, open, base, part.out(), &s);
    if (!same_state(q, s)) die("a short capacity changes the counts", k);
    if ((b && memcmp(part.digests, full.digests, 20 * b)) || (b && memcmp(part.sizes, full.sizes, 4 * b)) ||
        (b && memcmp(part.offsets, full.offsets, 8 * b)) || (b && memcmp(part.block_file, full.block_file, 4 * b)) ||
        (f && memcmp(part.name_at, full.name_at, 8 * f)) || (f && memcmp(part.name_len, full.name_len, 4 * f)) ||
        (f && memcmp(part.first, full.first, 8 * f)))
      die("a short capacity changes the rows that fit", k);
    if (f == q.n_files && (part.first[f] != full.first[f] || (f && memcmp(part.file_size, full.file_size, 8 * f))))
      die("blocks one short change the sections", k);
  }
  printf("R %llu %llu %llu %llu %d %d %llu %d\n", (unsigned long long)r.n_blocks, (unsigned long long)r.n_files,
         (unsigned long long)r.messages, (unsigned long long)r.consumed, r.stop, (int)r.open,
         (unsigned long long)r.end_offset, (int)r.too_large);
  for (uint64_t i = 0; i < r.n_blocks; i++) {
    printf("B ");
    for (int j = 0; j < 20; j++) printf("%02x", full.digests[20 * i + j]);
    printf(" %u %llu %u\n", full.sizes[i], (unsigned long long)full.offsets[i], full.block_file[i]);
  }
  for (uint64_t f = 0; f < r.n_files; f++)
    printf("F %llu %u %llu %llu\n", (unsigned long long)full.name_at[f], full.name_len[f],
           (unsigned long long)full.first[f], (unsigned long long)full.file_size[f]);
  printf("L %llu\n", (unsigned long long)full.first[r.n_files]);
  for (uint64_t p = 0; p < n; p++) {
    uint32_t kind = 0;
    uint64_t size = 0;
    const uint32_t len = sfwp::files_message(run + p, n - p, &kind, &size);
    if (len) printf("C %llu %u %u\n", (unsigned long long)p, len, kind);
  }
  free(run);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> all;
  uint8_t buf[1 << 16];
  for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + got);
  fclose(f);
  size_t at = 0, k = 0;
  while (at < all.size()) {
    if (all.size() - at < 20) die("a short record header", k);
    uint32_t open;
    uint64_t base, n;
    memcpy(&open, &all[at], 4);
    memcpy(&base, &all[at + 4], 8);
    memcpy(&n, &all[at + 12], 8);
    at += 20;
    if (all.size() - at < n) die("a short record", k);
    record(k++, all.data() + at, n, open != 0, base);
    at += n;
  }
  printf("ok %zu\n", k);
  return 0;
}
