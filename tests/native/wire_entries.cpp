// wire_entries.cpp -- the files-list rules (syncfast_amd/csrc/sf_wire_entries.hpp)
// alone: a stand-alone program, built with ASan + UBSan by
// tests/test_wire_entries.py and run directly.  No GPU, no library.
//
//   wire_entries CASES   CASES holds records, each one byte of kind and its
//                        fields (little endian); every buffer a rule reads or
//                        writes is a heap copy of its exact length, so a read
//                        or a write past it is an ASan report.
//     'P' <u64 n> <n bytes>      parse_entries_run: the query form, the full
//                                form and one row short must agree; prints
//                                  R count consumed stop bad_name(-1: none)
//                                  E name_at name_len size hash-hex     per entry
//                                  C position length name_len           per candidate
//                                (entry_message asked at every position, and
//                                classify_entries must say kEntry exactly there)
//     'U' <u64 n> <n bytes>      utf8_ok: prints  U 0|1
//     'W' <u32 n> <u32 end> n x (<u32 name_len> <u64 size> <name> <20 B>)
//                                first_bad_entry, then build_entries_run_serial
//                                into a buffer of exactly its length: prints
//                                  W bad <file>  |  W ok <hex>
//     'G' <u64 n_bytes> <bytes> <u32 n> n x (<u64 at> <u32 len>)
//         <u32 has_pick> <u32 n_pick> n_pick x <u32>
//                                first_bad_pick, then build_get_files_run_serial:
//                                  G bad <pick>  |  G ok <hex>
//     'H' <u64 mask> <u64 n> <n bytes>   name_hash: prints  H <16 hex digits>
//   and "ok <records>" at the end.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../syncfast_amd/csrc/sf_wire_entries.hpp"

namespace {

size_t g_record = 0;

[[noreturn]] void die(const char* what) {
  fprintf(stderr, "record %zu: %s\n", g_record, what);
  exit(1);
}

template <class T>
T* exact(uint64_t n) {  // n entries on the heap and not one more (NULL for none)
  return n ? static_cast<T*>(malloc(n * sizeof(T))) : nullptr;
}

uint8_t* copy_of(const uint8_t* b, uint64_t n) {  // never NULL: a rule may form b + 0
  uint8_t* p = static_cast<uint8_t*>(malloc(n ? n : 1));
  if (n) memcpy(p, b, n);
  return p;
}

void hex(const uint8_t* b, uint64_t n) {
  for (uint64_t i = 0; i < n; i++) printf("%02x", b[i]);
}

struct Reader {
  const std::vector<uint8_t>& all;
  size_t at = 0;
  template <class T>
  T get() {
    if (all.size() - at < sizeof(T)) die("a short record");
    T v;
    memcpy(&v, &all[at], sizeof(T));
    at += sizeof(T);
    return v;
  }
  const uint8_t* bytes(uint64_t n) {
    if (all.size() - at < n) die("a short record");
    const uint8_t* p = all.data() + at;
    at += n;
    return p;
  }
};

struct Rows {
  uint64_t cap;
  uint64_t *name_at, *sizes;
  uint32_t* name_len;
  uint8_t* hashes;
  explicit Rows(uint64_t c)
      : cap(c), name_at(exact<uint64_t>(c)), sizes(exact<uint64_t>(c)), name_len(exact<uint32_t>(c)),
        hashes(exact<uint8_t>(20 * c)) {}
  ~Rows() { free(name_at); free(sizes); free(name_len); free(hashes); }
  sfwp::EntriesOut out() const { return {name_at, name_len, sizes, hashes, cap}; }
};

void parse(const uint8_t* bytes, uint64_t n) {
  uint8_t* run = copy_of(bytes, n);
  sfwp::EntriesParsed q, r, s;
  sfwp::parse_entries_run(run, n, sfwp::EntriesOut{}, &q);
  Rows full(q.count);
  sfwp::parse_entries_run(run, n, full.out(), &r);
  if (q.count != r.count || q.consumed != r.consumed || q.stop != r.stop) die("the query form and the full form differ");
  if (q.count) {
    const uint64_t c = q.count - 1;
    Rows part(c);
    sfwp::parse_entries_run(run, n, part.out(), &s);
    if (q.count != s.count || q.consumed != s.consumed || q.stop != s.stop) die("a short capacity changes the counts");
    if (c && (memcmp(part.name_at, full.name_at, 8 * c) || memcmp(part.name_len, full.name_len, 4 * c) ||
              memcmp(part.sizes, full.sizes, 8 * c) || memcmp(part.hashes, full.hashes, 20 * c)))
      die("a short capacity changes the rows that fit");
  }
  long long bad = -1;
  for (uint64_t i = 0; i < r.count && bad < 0; i++)
    if (!sfwp::utf8_ok(run + full.name_at[i], full.name_len[i])) bad = (long long)i;
  printf("R %llu %llu %d %lld\n", (unsigned long long)r.count, (unsigned long long)r.consumed, r.stop, bad);
  for (uint64_t i = 0; i < r.count; i++) {
    printf("E %llu %u %llu ", (unsigned long long)full.name_at[i], full.name_len[i], (unsigned long long)full.sizes[i]);
    hex(full.hashes + 20 * i, 20);
    printf("\n");
  }
  for (uint64_t p = 0; p < n; p++) {
    uint32_t name_len = 0, len2 = 0, name_len2 = 0;
    uint64_t size = 0, size2 = 0;
    const uint32_t len = sfwp::entry_message(run + p, n - p, &name_len, &size);
    const int c = sfwp::classify_entries(run + p, n - p, &len2, &name_len2, &size2);
    if ((len != 0) != (c == sfwp::kEntry)) die("entry_message and classify_entries disagree about an entry");
    if (len && (len != len2 || name_len != name_len2 || size != size2)) die("they disagree about its fields");
    if (len) printf("C %llu %u %u\n", (unsigned long long)p, len, name_len);
  }
  free(run);
}

void write_entries(Reader& in) {
  const uint32_t n = in.get<uint32_t>(), end = in.get<uint32_t>();
  std::vector<uint64_t> at(n + 1, 0), sizes(n);
  std::vector<uint8_t> names, hashes;
  for (uint32_t f = 0; f < n; f++) {
    const uint32_t len = in.get<uint32_t>();
    sizes[f] = in.get<uint64_t>();
    const uint8_t* nm = in.bytes(len);
    names.insert(names.end(), nm, nm + len);
    at[f + 1] = names.size();
    const uint8_t* h = in.bytes(20);
    hashes.insert(hashes.end(), h, h + 20);
  }
  uint8_t* nm = copy_of(names.data(), names.size());
  uint8_t* hs = copy_of(hashes.data(), hashes.size());
  uint64_t* a = exact<uint64_t>(n + 1);
  uint64_t* z = exact<uint64_t>(n);
  memcpy(a, at.data(), 8 * (n + 1));
  if (n) memcpy(z, sizes.data(), 8 * n);
  const uint64_t bad = sfwp::first_bad_entry(nm, a, z, n);
  if (bad != sfwp::kNoFile) {
    printf("W bad %llu\n", (unsigned long long)bad);
  } else {
    const uint64_t total = sfwp::build_entries_run_serial(nm, a, z, hs, n, end != 0, nullptr);
    uint8_t* out = static_cast<uint8_t*>(malloc(total ? total : 1));
    if (sfwp::build_entries_run_serial(nm, a, z, hs, n, end != 0, out) != total) die("the two lengths differ");
    printf("W ok ");
    hex(out, total);
    printf("\n");
    free(out);
  }
  free(nm); free(hs); free(a); free(z);
}

void write_get_files(Reader& in) {
  const uint64_t nb = in.get<uint64_t>();
  uint8_t* bytes = copy_of(in.bytes(nb), nb);
  const uint32_t n = in.get<uint32_t>();
  uint64_t* at = exact<uint64_t>(n);
  uint32_t* len = exact<uint32_t>(n);
  for (uint32_t i = 0; i < n; i++) {
    at[i] = in.get<uint64_t>();
    len[i] = in.get<uint32_t>();
  }
  const uint32_t has_pick = in.get<uint32_t>(), n_pick = in.get<uint32_t>();
  uint32_t* pick = has_pick ? exact<uint32_t>(n_pick ? n_pick : 1) : nullptr;
  for (uint32_t k = 0; k < n_pick; k++) pick[k] = in.get<uint32_t>();
  const uint64_t m = has_pick ? n_pick : n;
  const uint64_t bad = sfwp::first_bad_pick(bytes, nb, at, len, n, pick, m);
  if (bad != sfwp::kNoFile) {
    printf("G bad %llu\n", (unsigned long long)bad);
  } else {
    const uint64_t total = sfwp::build_get_files_run_serial(bytes, at, len, pick, m, nullptr);
    uint8_t* out = static_cast<uint8_t*>(malloc(total ? total : 1));
    if (sfwp::build_get_files_run_serial(bytes, at, len, pick, m, out) != total) die("the two lengths differ");
    printf("G ok ");
    hex(out, total);
    printf("\n");
    free(out);
  }
  free(bytes); free(at); free(len); free(pick);
}

// The rules are constexpr: a few of them hold at compile time.
constexpr uint8_t kOne[] = "FILE_ENTRY\nab\n+07\n01234567890123456789\n";
constexpr uint32_t one_len() {
  uint32_t name_len = 0;
  uint64_t size = 0;
  const uint32_t len = sfwp::entry_message(kOne, sizeof(kOne) - 1, &name_len, &size);
  return len * 1000 + name_len * 100 + (uint32_t)size;
}
static_assert(one_len() == 39 * 1000 + 2 * 100 + 7, "entry_message at compile time");
static_assert(sfwp::file_entry_len(2, 7) == 37 && sfwp::get_file_len(3) == 13 && sfwp::end_files_len() == 10, "lengths");
static_assert(sfwp::kMinEntry == 35 && sfwp::kMaxEntry == 149 && sfwp::kEndFiles == 5, "limits");

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> all;
  uint8_t buf[1 << 16];
  for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + got);
  fclose(f);
  Reader in{all};
  while (in.at < all.size()) {
    const uint8_t kind = in.get<uint8_t>();
    if (kind == 'P') {
      const uint64_t n = in.get<uint64_t>();
      parse(in.bytes(n), n);
    } else if (kind == 'U') {
      const uint64_t n = in.get<uint64_t>();
      uint8_t* name = copy_of(in.bytes(n), n);
      printf("U %d\n", (int)sfwp::utf8_ok(name, (uint32_t)n));
      free(name);
    } else if (kind == 'W') {
      write_entries(in);
    } else if (kind == 'G') {
      write_get_files(in);
    } else if (kind == 'H') {
      const uint64_t mask = in.get<uint64_t>(), n = in.get<uint64_t>();
      uint8_t* name = copy_of(in.bytes(n), n);
      printf("H %016llx\n", (unsigned long long)sfwp::name_hash(name, n, mask));
      free(name);
    } else {
      die("an unknown record kind");
    }
    g_record++;
  }
  printf("ok %zu\n", g_record);
  return 0;
}
