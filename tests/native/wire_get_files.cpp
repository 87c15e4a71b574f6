// wire_get_files.cpp -- the rules of a received GET_FILE run and of its answer
// (syncfast_amd/csrc/sf_wire_get_files.hpp) alone: a stand-alone program, built
// with ASan + UBSan by tests/test_wire_get_files.py and run directly.  No GPU,
// no library.
//
//   wire_get_files CASES   CASES holds records, each one byte of kind and its
//                          fields (little endian); every buffer a rule reads or
//                          writes is a heap copy of its exact length, so a read
//                          or a write past it is an ASan report.
//     'P' <u64 n> <n bytes>      parse_get_files_run: the query form, the full
//                                form and one row short must agree, and so must
//                                the parse told by lines (parse_get_files_lines);
//                                prints
//                                  R count consumed stop bad_name(-1: none)
//                                  E name_at name_len                  per request
//                                  C position length name_len          per candidate
//                                (get_file_message asked at every position, and
//                                classify_get_files must say kRequest exactly there)
//     'S' <u64 n> <n bytes> <u64 max_run_bytes> <i64 broken row, -1: none>
//         <u32 rows> rows x (<u32 name_len> <name> <u8 present> <u32 blocks>
//                            blocks x (<20 B> <u32 size>))
//                                the requests parsed, every name looked up (the
//                                lowest present row of that name), then
//                                build_serve_files_serial for the plan alone and
//                                into a buffer of exactly its length: prints
//                                  S n_requests n_answered answered_bytes why bad_row(-1) messages consumed stop <hex>
//   and "ok <records>" at the end.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../syncfast_amd/csrc/sf_wire_get_files.hpp"

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
  uint64_t* name_at;
  uint32_t* name_len;
  explicit Rows(uint64_t c) : cap(c), name_at(exact<uint64_t>(c)), name_len(exact<uint32_t>(c)) {}
  ~Rows() { free(name_at); free(name_len); }
  sfwp::GetFilesOut out() const { return {name_at, name_len, cap}; }
};

void parse(const uint8_t* bytes, uint64_t n) {
  uint8_t* run = copy_of(bytes, n);
  sfwp::GetFilesParsed q, r, s;
  sfwp::parse_get_files_run(run, n, sfwp::GetFilesOut{}, &q);
  Rows full(q.count);
  sfwp::parse_get_files_run(run, n, full.out(), &r);
  if (q.count != r.count || q.consumed != r.consumed || q.stop != r.stop) die("the query form and the full form differ");
  if (q.count) {
    const uint64_t c = q.count - 1;
    Rows part(c);
    sfwp::parse_get_files_run(run, n, part.out(), &s);
    if (q.count != s.count || q.consumed != s.consumed || q.stop != s.stop) die("a short capacity changes the counts");
    if (c && (memcmp(part.name_at, full.name_at, 8 * c) || memcmp(part.name_len, full.name_len, 4 * c)))
      die("a short capacity changes the rows that fit");
  }
  uint64_t lcount = 0, lconsumed = 0;
  sfwp::parse_get_files_lines(run, n, &lcount, &lconsumed);
  if (lcount != r.count || lconsumed != r.consumed) die("the parse by lines and the parse by messages differ");
  long long bad = -1;
  for (uint64_t i = 0; i < r.count && bad < 0; i++)
    if (!sfwp::utf8_ok(run + full.name_at[i], full.name_len[i])) bad = (long long)i;
  printf("R %llu %llu %d %lld\n", (unsigned long long)r.count, (unsigned long long)r.consumed, r.stop, bad);
  for (uint64_t i = 0; i < r.count; i++) printf("E %llu %u\n", (unsigned long long)full.name_at[i], full.name_len[i]);
  for (uint64_t p = 0; p < n; p++) {
    uint32_t name_len = 0, len2 = 0, name_len2 = 0;
    const uint32_t len = sfwp::get_file_message(run + p, n - p, &name_len);
    const int c = sfwp::classify_get_files(run + p, n - p, &len2, &name_len2);
    if ((len != 0) != (c == sfwp::kRequest)) die("get_file_message and classify_get_files disagree about a request");
    if (len && (len != len2 || name_len != name_len2)) die("they disagree about its fields");
    if (len) printf("C %llu %u %u\n", (unsigned long long)p, len, name_len);
  }
  free(run);
}

void serve(Reader& in) {
  const uint64_t n = in.get<uint64_t>();
  uint8_t* req = copy_of(in.bytes(n), n);
  const uint64_t max_run_bytes = in.get<uint64_t>();
  const int64_t broken = in.get<int64_t>();
  const uint32_t n_rows = in.get<uint32_t>();
  std::vector<std::vector<uint8_t>> names(n_rows);
  std::vector<uint8_t> present(n_rows), digests;
  std::vector<uint32_t> sizes;
  std::vector<uint64_t> first(n_rows + 1, 0);
  for (uint32_t r = 0; r < n_rows; r++) {
    const uint32_t len = in.get<uint32_t>();
    const uint8_t* nm = in.bytes(len);
    names[r].assign(nm, nm + len);
    present[r] = in.get<uint8_t>();
    const uint32_t blocks = in.get<uint32_t>();
    for (uint32_t i = 0; i < blocks; i++) {
      const uint8_t* d = in.bytes(20);
      digests.insert(digests.end(), d, d + 20);
      sizes.push_back(in.get<uint32_t>());
    }
    first[r + 1] = sizes.size();
  }
  const uint64_t n_blocks = sizes.size();
  if (broken >= 0) first[(size_t)broken] = n_blocks + 5;  // above its successor: the row's entries do not hold

  sfwp::GetFilesParsed q;
  sfwp::parse_get_files_run(req, n, sfwp::GetFilesOut{}, &q);
  Rows spans(q.count);
  sfwp::parse_get_files_run(req, n, spans.out(), &q);
  int64_t* rows = exact<int64_t>(q.count);
  for (uint64_t k = 0; k < q.count; k++) {
    rows[k] = -1;
    for (uint32_t r = 0; r < n_rows && rows[k] < 0; r++)
      if (present[r] && names[r].size() == spans.name_len[k] &&
          (spans.name_len[k] == 0 || memcmp(names[r].data(), req + spans.name_at[k], spans.name_len[k]) == 0))
        rows[k] = r;
  }
  uint64_t* f = exact<uint64_t>(n_rows + 1);
  memcpy(f, first.data(), 8 * (n_rows + 1));
  uint8_t* dg = copy_of(digests.data(), digests.size());
  uint32_t* sz = exact<uint32_t>(n_blocks);
  if (n_blocks) memcpy(sz, sizes.data(), 4 * n_blocks);

  const sfwp::ServePlan plan = sfwp::build_serve_files_serial(req, spans.name_at, spans.name_len, q.count, rows, f, dg,
                                                              sz, n_blocks, max_run_bytes, nullptr);
  uint8_t* out = static_cast<uint8_t*>(malloc(plan.total ? plan.total : 1));
  const sfwp::ServePlan again = sfwp::build_serve_files_serial(req, spans.name_at, spans.name_len, q.count, rows, f, dg,
                                                               sz, n_blocks, max_run_bytes, out);
  if (again.total != plan.total || again.n_answered != plan.n_answered || again.why != plan.why ||
      again.messages != plan.messages || again.answered_bytes != plan.answered_bytes || again.bad_row != plan.bad_row)
    die("the plan alone and the build differ");
  printf("S %llu %llu %llu %d %lld %llu %llu %d ", (unsigned long long)q.count, (unsigned long long)plan.n_answered,
         (unsigned long long)plan.answered_bytes, plan.why, plan.bad_row == ~0ull ? -1ll : (long long)plan.bad_row,
         (unsigned long long)plan.messages, (unsigned long long)q.consumed, q.stop);
  hex(out, plan.total);
  printf("\n");
  free(out); free(req); free(rows); free(f); free(dg); free(sz);
}

// The rules are constexpr: a few of them hold at compile time.
constexpr uint8_t kOne[] = "GET_FILE\nab\nGET_FILE\n";
constexpr uint32_t one_len() {
  uint32_t name_len = 9;
  const uint32_t len = sfwp::get_file_message(kOne, sizeof(kOne) - 1, &name_len);
  return len * 100 + name_len;
}
static_assert(one_len() == 12 * 100 + 2, "get_file_message at compile time");
static_assert(sfwp::kMinGetFile == 10 && sfwp::kMaxGetFile == 110 && sfwp::get_file_len(100) == 110, "limits");
static_assert(sfwp::line_ok(kOne, 0, 8, 8) && sfwp::line_ok(kOne, 1, 11, 2) && !sfwp::line_ok(kOne, 2, 11, 2) &&
                  !sfwp::line_ok(kOne, 1, 200, 101) && sfwp::line_ok(kOne, 2, 20, 8),
              "lines by parity");
static_assert(sfwp::requests_of_lines(5, ~0ull) == 2 && sfwp::requests_of_lines(5, 3) == 1 &&
                  sfwp::requests_of_lines(6, 6) == 3 && sfwp::requests_of_lines(0, 0) == 0,
              "requests of lines");
static_assert(sfwp::serve_over((1ull << 32) - 1, 0, 0, 1, 0) && !sfwp::serve_over((1ull << 32) - 2, 0, 0, 1, 0) &&
                  sfwp::serve_over(1, 34, 1, 1, 55) && !sfwp::serve_over(1, 34, 1, 1, 56) && !sfwp::serve_over(1, 34, 1, 1, 0),
              "the run's bounds");

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
    } else if (kind == 'S') {
      serve(in);
    } else {
      die("an unknown record kind");
    }
    g_record++;
  }
  printf("ok %zu\n", g_record);
  return 0;
}
