// The framing rules of a whole GetFiles answer (syncfast_amd/csrc/
// sf_wire_send_files.hpp: name_ok, the lengths and writers, start_at, block_at,
// end_at, file_of_block, file_ok, build_files_run_serial) alone, on a CPU: a
// stand-alone program built with ASan + UBSan by tests/test_send_files_rules.py.
// Every array is a heap copy of its exact length and every run is written into
// a heap buffer of exactly its length, so a read or store one byte out is a
// report.
//
//   (no argument)  checks name_ok, the writers, the search and file_ok; "ok"
//   FILE           any number of cases, each
//                    n_files n_blocks
//                    first[0] ... first[n_files]
//                    name_at[0] ... name_at[n_files]
//                    names-hex (or -)
//                    n_blocks lines "size digest-hex"
//                  and per case one line "bad F" for a case whose first bad
//                  file is F, else "ok total run-hex | starts | ends | blocks"
//                  with the places the formulas give, space separated.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../syncfast_amd/csrc/sf_wire_send_files.hpp"

using namespace sfwp;

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);         \
      fails++;                                                \
    }                                                         \
  } while (0)

static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
  return n ? s : "-";
}

static std::vector<uint8_t> unhex(const char* s) {
  std::vector<uint8_t> v;
  if (s[0] == '-') return v;
  auto nib = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : c - 'a' + 10); };
  for (size_t i = 0; s[i] && s[i + 1]; i += 2) v.push_back((uint8_t)(nib(s[i]) << 4 | nib(s[i + 1])));
  return v;
}

// A heap copy of exactly v's length (NULL for none): what the rules may read.
template <typename T>
static T* exact(const std::vector<T>& v) {
  if (v.empty()) return nullptr;
  T* p = static_cast<T*>(malloc(v.size() * sizeof(T)));
  memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

static void check_name_ok() {
  for (uint32_t len : {0u, 1u, 99u, 100u, 101u, 1000u}) {
    std::vector<uint8_t> v(len, 'n');
    uint8_t* p = exact(v);
    CHECK(name_ok(p, len) == (len <= 100));
    // a newline at the first, a middle and the last byte
    for (uint32_t at : {0u, len / 2, len ? len - 1 : 0u}) {
      if (!len || len > 100) continue;
      p[at] = '\n';
      CHECK(!name_ok(p, len));
      p[at] = 'n';
      CHECK(name_ok(p, len));
    }
    free(p);
  }
  const uint8_t other[] = {0, 0xFF, '\r', ' ', '/', 'F'};  // every byte but '\n' is a name byte
  CHECK(name_ok(other, sizeof other));
}

static void check_writers() {
  CHECK(file_start_len(0) == 12 && file_start_len(100) == 112 && file_end_len() == 9);
  CHECK(file_block_len(0) == 34 && file_block_len(9) == 34 && file_block_len(10) == 35);
  CHECK(file_block_len(99999) == 38 && file_block_len(4294967295u) == 43);
  for (uint32_t len : {0u, 1u, 99u, 100u}) {
    std::vector<uint8_t> name(len);
    for (uint32_t k = 0; k < len; k++) name[k] = (uint8_t)('a' + k % 26);
    uint8_t* n = exact(name);
    uint8_t* o = static_cast<uint8_t*>(malloc(12 + len));
    CHECK(write_file_start(o, n, len) == 12 + len);
    uint32_t kind = 0;
    uint64_t size = 0;
    CHECK(files_message(o, 12 + len, &kind, &size) == 12 + len && kind == kStart);
    CHECK(memcmp(o, "FILE_START\n", 11) == 0 && (len == 0 || memcmp(o + 11, n, len) == 0) && o[11 + len] == '\n');
    free(o);
    free(n);
  }
  uint8_t* e = static_cast<uint8_t*>(malloc(9));
  CHECK(write_file_end(e) == 9 && memcmp(e, "FILE_END\n", 9) == 0);
  free(e);
  for (uint32_t size : {0u, 9u, 10u, 99999u, 100000u, 4294967295u}) {
    uint8_t d[20];
    for (uint32_t k = 0; k < 20; k++) d[k] = (uint8_t)(size * 7 + k);
    d[3] = '\n';
    const uint32_t len = file_block_len(size);
    uint8_t* o = static_cast<uint8_t*>(malloc(len));
    CHECK(write_file_block(o, d, size) == len);
    uint64_t back = 0;
    CHECK(block_message(o, len, &back) == len && back == size && memcmp(o + 11, d, 20) == 0);
    free(o);
  }
}

static void check_search_and_file_ok() {
  // empty files before, between and after: the last file that begins at or before i
  const std::vector<uint64_t> first{0, 0, 0, 3, 3, 4, 4, 4};
  uint64_t* f = exact(first);
  const uint64_t want[4] = {2, 2, 2, 4};
  for (uint64_t i = 0; i < 4; i++) CHECK(file_of_block(f, 7, i) == want[i]);
  free(f);
  for (uint64_t n = 1; n <= 70; n++) {  // every count around the search's halvings, one block per file
    std::vector<uint64_t> one(n + 1);
    for (uint64_t k = 0; k <= n; k++) one[k] = k;
    uint64_t* p = exact(one);
    for (uint64_t i = 0; i < n; i++) CHECK(file_of_block(p, n, i) == i);
    free(p);
  }
  // file_ok reads its own entries, name_at[n_files] and -- only when those hold -- its name
  const std::vector<uint64_t> b{0, 1, 1}, a{0, 2, 5};
  const std::vector<uint8_t> names{'a', 'b', 'c', '\n', 'd'};
  uint64_t *pb = exact(b), *pa = exact(a);
  uint8_t* pn = exact(names);
  CHECK(file_ok(pb, pn, pa, 2, 1, 0) && !file_ok(pb, pn, pa, 2, 1, 1));
  CHECK(first_bad_file(pb, pn, pa, 2, 1) == 1 && first_bad_file(pb, pn, pa, 2, 2) == 1);
  CHECK(!file_ok(pb, nullptr, pa, 2, 1, 0));  // a name and no bytes for it
  pa[1] = 1ull << 60;                         // a name that would lie outside the names: its bytes are not read
  CHECK(!file_ok(pb, pn, pa, 2, 1, 0) && !file_ok(pb, pn, pa, 2, 1, 1));
  pa[1] = 0, pa[2] = 0;
  CHECK(file_ok(pb, nullptr, pa, 2, 1, 0) && file_ok(pb, nullptr, pa, 2, 1, 1));
  free(pb);
  free(pa);
  free(pn);
}

static bool next_u64(FILE* in, uint64_t* v) {
  unsigned long long x = 0;
  if (fscanf(in, "%llu", &x) != 1) return false;
  *v = x;
  return true;
}

static int cases(const char* path) {
  FILE* in = fopen(path, "r");
  if (!in) return 2;
  uint64_t nf = 0, nb = 0;
  std::vector<char> word(1 << 20);
  while (next_u64(in, &nf) && next_u64(in, &nb)) {
    std::vector<uint64_t> first(nf + 1), name_at(nf + 1);
    for (auto& v : first) if (!next_u64(in, &v)) return 2;
    for (auto& v : name_at) if (!next_u64(in, &v)) return 2;
    if (fscanf(in, "%1048575s", word.data()) != 1) return 2;
    const std::vector<uint8_t> names = unhex(word.data());
    std::vector<uint32_t> sizes(nb);
    std::vector<uint8_t> digests;
    for (uint64_t i = 0; i < nb; i++) {
      uint64_t s = 0;
      if (!next_u64(in, &s) || fscanf(in, "%1048575s", word.data()) != 1) return 2;
      sizes[i] = (uint32_t)s;
      const std::vector<uint8_t> d = unhex(word.data());
      if (d.size() != 20) return 2;
      digests.insert(digests.end(), d.begin(), d.end());
    }
    uint64_t *pf = exact(first), *pa = exact(name_at);
    uint32_t* ps = exact(sizes);
    uint8_t *pd = exact(digests), *pn = exact(names);
    const uint64_t bad = first_bad_file(pf, pn, pa, nf, nb);
    if (bad != kNoFile) {
      printf("bad %llu\n", (unsigned long long)bad);
    } else {
      std::vector<uint64_t> ends(nb);
      file_block_ends(ps, nb, ends.data());
      uint64_t* E = exact(ends);
      const uint64_t total = files_run_total(bex(E, nb), nf ? pa[nf] : 0, nf);
      uint8_t* out = static_cast<uint8_t*>(malloc(total ? total : 1));
      memset(out, 0x5A, total);
      CHECK(build_files_run_serial(pd, ps, nb, pf, pn, pa, nf, E, out) == total);
      printf("ok %llu %s |", (unsigned long long)total, hex(out, total).c_str());
      for (uint64_t f = 0; f < nf; f++) printf(" %llu", (unsigned long long)start_at(E, pf, pa, f));
      printf(" |");
      for (uint64_t f = 0; f < nf; f++) printf(" %llu", (unsigned long long)end_at(E, pf, pa, f));
      printf(" |");
      for (uint64_t i = 0; i < nb; i++) {
        const uint64_t f = file_of_block(pf, nf, i);
        CHECK(pf[f] <= i && i < pf[f + 1]);
        printf(" %llu", (unsigned long long)block_at(E, pa, f, i));
      }
      printf("\n");
      free(out);
      free(E);
    }
    free(pf);
    free(pa);
    free(ps);
    free(pd);
    free(pn);
  }
  fclose(in);
  return fails ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return cases(argv[1]);
  check_name_ok();
  check_writers();
  check_search_and_file_ok();
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
