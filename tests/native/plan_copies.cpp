// The per-block rules of sf_plan_copies.hip (syncfast_amd/csrc/
// sf_plan_copies.hpp: classify, row_ok, file_ok, section_ok, dst_of, in_arena,
// present, same_digest) alone, on a CPU: a stand-alone program built with
// ASan + UBSan by tests/test_plan_copies_rules.py.  Every list lives in a heap
// buffer of its exact length, so a read one entry out is a report.
//
//   (no argument)  checks the rules against their definitions; prints "ok"
//   FILE           the plan of the case in FILE, serially, as the kernels make
//                  it: "ERANGE", or the counts, every block's "class present
//                  ask dst", the jobs' "src dst size block" and the local
//                  files' job counts.
//                  FILE: "n n_files n_table n_local query verify src_len", then
//                  n lines "row size offset section digest-hex computed-hex"
//                  (computed: what the block's local bytes hash to), n_files
//                  bases, n_table lines "file offset size", n_local lines
//                  "base size".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../syncfast_amd/csrc/sf_plan_copies.hpp"

using namespace sfpc;

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);         \
      fails++;                                                \
    }                                                         \
  } while (0)

template <typename T>
struct Heap {  // exactly n entries
  T* p;
  explicit Heap(size_t n) : p(static_cast<T*>(calloc(n ? n : 1, n ? sizeof(T) : 1))) {}
  ~Heap() { free(p); }
  T& operator[](size_t i) { return p[i]; }
};

static bool unhex(const char* s, uint32_t* words) {
  uint8_t b[kDigest];
  for (uint32_t k = 0; k < kDigest; k++) {
    unsigned v = 0;
    if (sscanf(s + 2 * k, "%2x", &v) != 1) return false;
    b[k] = (uint8_t)v;
  }
  memcpy(words, b, kDigest);
  return true;
}

static int from_file(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return 2;
  unsigned long long n = 0, n_files = 0, n_table = 0, n_local = 0, src_len = 0;
  int query = 0, verify = 0;
  if (fscanf(f, "%llu %llu %llu %llu %d %d %llu", &n, &n_files, &n_table, &n_local, &query, &verify, &src_len) != 7)
    return 2;
  Heap<int64_t> rows(n);
  Heap<uint32_t> sizes(n), section(n), digests(5 * n), computed(5 * n), t_file(n_table), t_size(n_table);
  Heap<uint64_t> offsets(n), file_base(n_files), t_off(n_table), l_base(n_local), l_size(n_local);
  for (uint64_t i = 0; i < n; i++) {
    long long r = 0;
    unsigned long long o = 0;
    unsigned z = 0, s = 0;
    char d[41] = {0}, c[41] = {0};
    if (fscanf(f, "%lld %u %llu %u %40s %40s", &r, &z, &o, &s, d, c) != 6) return 2;
    rows[i] = r, sizes[i] = z, offsets[i] = o, section[i] = s;
    if (!unhex(d, &digests[5 * i]) || !unhex(c, &computed[5 * i])) return 2;
  }
  for (uint64_t k = 0; k < n_files; k++) {
    unsigned long long v = 0;
    if (fscanf(f, "%llu", &v) != 1) return 2;
    file_base[k] = v;
  }
  for (uint64_t k = 0; k < n_table; k++) {
    unsigned long long o = 0;
    unsigned j = 0, z = 0;
    if (fscanf(f, "%u %llu %u", &j, &o, &z) != 3) return 2;
    t_file[k] = j, t_off[k] = o, t_size[k] = z;
  }
  for (uint64_t k = 0; k < n_local; k++) {
    unsigned long long b = 0, z = 0;
    if (fscanf(f, "%llu %llu", &b, &z) != 2) return 2;
    l_base[k] = b, l_size[k] = z;
  }
  fclose(f);

  // the class pass
  Heap<uint8_t> cls(n);
  Heap<uint64_t> dst(n);
  bool bad = false;
  for (uint64_t i = 0; i < n; i++) {
    const int64_t r = rows[i];
    if (!section_ok(section[i], n_files) || !dst_of(file_base[section[i]], offsets[i], &dst[i])) bad = true;
    cls[i] = kMissing;
    if (!row_ok(r, n_table)) {
      bad = true;
    } else if (r >= 0) {
      const uint32_t j = t_file[r];
      if (!file_ok(j, n_local)) {
        bad = true;
      } else {
        const uint64_t base = query ? 0 : l_base[j];
        cls[i] = classify(r, sizes[i], t_size[r], t_off[r], l_size[j], base);
        if (cls[i] == kCandidate && verify && !query && !in_arena(base, t_off[r], sizes[i], src_len)) bad = true;
      }
    }
  }
  if (bad) {
    printf("ERANGE\n");
    return 0;
  }
  // verification, then the emit pass
  uint8_t job_class = kCandidate;
  if (verify && !query) {
    job_class = kJob;
    for (uint64_t i = 0; i < n; i++)
      if (cls[i] == kCandidate) cls[i] = same_digest(&digests[5 * i], &computed[5 * i]) ? kJob : kUnverified;
  }
  uint64_t counts[8] = {};
  Heap<uint32_t> local_jobs(n_local);
  for (uint64_t i = 0; i < n; i++) {
    if (cls[i] == job_class) {
      counts[0]++, counts[1] += sizes[i], local_jobs[t_file[rows[i]]]++;
    } else {
      const int at[8] = {2, 3, 4, 5, 7, -1, -1, 6};  // the class's place in the counts
      counts[at[cls[i]]]++;
    }
  }
  for (int k = 0; k < 8; k++) printf("%llu%c", (unsigned long long)counts[k], k == 7 ? '\n' : ' ');
  for (uint64_t i = 0; i < n; i++) {
    const bool here = present(cls[i], job_class);
    printf("%u %d %d %llu\n", cls[i] == job_class ? (unsigned)kJob : (unsigned)cls[i], here, !here,
           (unsigned long long)dst[i]);
  }
  for (uint64_t i = 0; i < n; i++)
    if (cls[i] == job_class) {
      const int64_t r = rows[i];
      printf("%llu %llu %u %llu\n", (unsigned long long)((query ? 0 : l_base[t_file[r]]) + t_off[r]),
             (unsigned long long)dst[i], sizes[i], (unsigned long long)i);
    }
  for (uint64_t k = 0; k < n_local; k++) printf("%u\n", local_jobs[k]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2) return from_file(argv[1]);
  const uint64_t M = UINT64_MAX;
  // every class, each with the smallest change from a candidate
  CHECK(classify(3, 10, 10, 90, 100, 0) == kCandidate);
  CHECK(classify(-1, 10, 10, 90, 100, 0) == kMissing && classify(INT64_MIN, 0, 0, 0, 0, 0) == kMissing);
  CHECK(classify(3, 10, 11, 90, 100, 0) == kSizeMismatch && classify(3, 11, 10, 0, 100, 0) == kSizeMismatch);
  CHECK(classify(3, 10, 10, 91, 100, 0) == kStale);
  CHECK(classify(3, 10, 10, 90, 100, kNotLoaded) == kUnavailable);
  CHECK(classify(3, 0, 0, 90, 100, 0) == kEmpty);
  // the table offset + size at the file's size and one past it, at the ends of the range too
  CHECK(classify(0, 1, 1, 99, 100, 0) == kCandidate && classify(0, 1, 1, 100, 100, 0) == kStale);
  CHECK(classify(0, 0, 0, 100, 100, 0) == kEmpty && classify(0, 0, 0, 101, 100, 0) == kStale);
  CHECK(classify(0, 100, 100, 0, 100, 0) == kCandidate && classify(0, 101, 101, 0, 100, 0) == kStale);
  CHECK(classify(0, 1, 1, M, M, 0) == kStale && classify(0, 1, 1, M - 1, M, 0) == kCandidate);
  CHECK(classify(0, 0xFFFFFFFFu, 0xFFFFFFFFu, M - 0xFFFFFFFFull, M, 0) == kCandidate);
  CHECK(classify(0, 0xFFFFFFFFu, 0xFFFFFFFFu, M - 0xFFFFFFFEull, M, 0) == kStale);  // the sum passes 2^64
  // the first match: each class hides the ones after it
  CHECK(classify(-1, 10, 11, 95, 100, kNotLoaded) == kMissing);
  CHECK(classify(3, 0, 1, 101, 100, kNotLoaded) == kSizeMismatch);
  CHECK(classify(3, 0, 0, 101, 100, kNotLoaded) == kStale);
  CHECK(classify(3, 0, 0, 100, 100, kNotLoaded) == kUnavailable);
  CHECK(classify(3, 0, 0, 100, 100, 5) == kEmpty);
  // the destination sum at 2^64 - 1 and one past it
  uint64_t d = 7;
  CHECK(dst_of(M - 5, 5, &d) && d == M);
  d = 7;
  CHECK(!dst_of(M - 5, 6, &d) && d == 7 && !dst_of(M, 1, &d) && !dst_of(1, M, &d));
  CHECK(dst_of(0, 0, &d) && d == 0 && dst_of(M, 0, &d) && d == M && dst_of(0, M, &d) && d == M);
  // a candidate in the arena: its last byte at the arena's last, and one past it
  CHECK(in_arena(256, 90, 10, 356) && !in_arena(256, 91, 10, 356) && !in_arena(256, 90, 11, 356));
  CHECK(in_arena(0, 0, 0, 0) && !in_arena(0, 1, 0, 0) && !in_arena(M, 1, 0, M) && !in_arena(1, M, 1, M));
  CHECK(in_arena(M - 1, 0, 1, M) && !in_arena(M - 1, 1, 1, M));
  // bad input
  CHECK(row_ok(-1, 0) && row_ok(INT64_MIN, 0) && row_ok(4, 5) && !row_ok(5, 5) && !row_ok(0, 0) &&
        !row_ok(INT64_MAX, 1ull << 31));
  CHECK(file_ok(0, 1) && !file_ok(1, 1) && !file_ok(0, 0) && section_ok(2, 3) && !section_ok(3, 3));
  // present, with and without verification
  CHECK(present(kJob, kJob) && present(kEmpty, kJob) && !present(kCandidate, kJob) && !present(kUnverified, kJob));
  CHECK(present(kCandidate, kCandidate) && present(kEmpty, kCandidate) && !present(kMissing, kCandidate) &&
        !present(kSizeMismatch, kJob) && !present(kStale, kJob) && !present(kUnavailable, kJob));
  // digests: every single bit decides
  {
    Heap<uint32_t> a(5), b(5);
    for (uint32_t w = 0; w < 5; w++) a[w] = b[w] = 0x01020304u * (w + 1);
    CHECK(same_digest(a.p, b.p));
    for (uint32_t bit = 0; bit < 160; bit++) {
      b[bit / 32] ^= 1u << (bit % 32);
      CHECK(!same_digest(a.p, b.p));
      b[bit / 32] ^= 1u << (bit % 32);
    }
  }
  static_assert(classify(0, 1, 1, 0, 1, 0) == kCandidate && kCandidate == 5 && kJob == 6, "the scans count these");
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
