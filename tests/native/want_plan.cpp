// The per-row rules of sf_want.hip (syncfast_amd/csrc/sf_want_plan.hpp: asks,
// write_get_block, place) alone, on a CPU: a stand-alone program built with
// ASan + UBSan by tests/test_want_capi.py.  Every list lives in a heap buffer
// of its exact length and every run is written into one of exactly 31 bytes
// per asking row, so a read or store one byte out is a report.
//
//   (no argument)  checks the rules against their definitions; prints "ok"
//   FILE           the request run of the table in FILE, as hex ("-": empty).
//                  FILE: "has_rows has_take n", then n lines "row take digest-hex"
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../syncfast_amd/csrc/sf_want_plan.hpp"

using namespace sfwt;

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

template <typename T>
static T* heap(const std::vector<T>& v) {
  T* p = static_cast<T*>(malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0)));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

// The run the kernels write: the flags, their running count, and message
// count - 1 of every asking row.
static std::string run_of(const int64_t* rows, const uint8_t* take, const uint8_t* digests, uint64_t n) {
  uint64_t count = 0;
  for (uint64_t i = 0; i < n; i++) count += asks(rows, take, i);
  uint8_t* out = static_cast<uint8_t*>(malloc(count ? sfwp::kGetBlock * count : 1));
  uint64_t k = 0;
  for (uint64_t i = 0; i < n; i++)
    if (asks(rows, take, i)) write_get_block(out + sfwp::kGetBlock * k++, digests + sfwp::kDigest * i);
  const std::string s = hex(out, sfwp::kGetBlock * count);
  free(out);
  return s;
}

static int from_file(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return 2;
  int has_rows = 0, has_take = 0;
  unsigned long long n = 0;
  if (fscanf(f, "%d %d %llu", &has_rows, &has_take, &n) != 3) return 2;
  std::vector<int64_t> rows(n);
  std::vector<uint8_t> take(n), digests(n * sfwp::kDigest);
  for (uint64_t i = 0; i < n; i++) {
    long long row = 0;
    int t = 0;
    char d[41] = {0};
    if (fscanf(f, "%lld %d %40s", &row, &t, d) != 3) return 2;
    rows[i] = row;
    take[i] = (uint8_t)t;
    for (uint32_t k = 0; k < sfwp::kDigest; k++) {
      unsigned v = 0;
      if (sscanf(d + 2 * k, "%2x", &v) != 1) return 2;
      digests[sfwp::kDigest * i + k] = (uint8_t)v;
    }
  }
  fclose(f);
  int64_t* r = heap(rows);
  uint8_t *t = heap(take), *d = heap(digests);
  printf("%s\n", run_of(has_rows ? r : nullptr, has_take ? t : nullptr, d, n).c_str());
  free(r);
  free(t);
  free(d);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2) return from_file(argv[1]);
  // asks: every combination of the two optional lists
  {
    int64_t* rows = heap(std::vector<int64_t>{-1, 0, 5, -7, INT64_MIN, INT64_MAX});
    uint8_t* take = heap(std::vector<uint8_t>{1, 1, 0, 0, 255, 255});
    const bool by_rows[6] = {true, false, false, true, true, false};
    const bool by_take[6] = {true, true, false, false, true, true};
    for (uint64_t i = 0; i < 6; i++) {
      CHECK(asks(nullptr, nullptr, i));
      CHECK(asks(rows, nullptr, i) == by_rows[i]);
      CHECK(asks(nullptr, take, i) == by_take[i]);
      CHECK(asks(rows, take, i) == (by_rows[i] && by_take[i]));
    }
    free(rows);
    free(take);
  }
  // write_get_block: 31 bytes, the serial rule reads them back as one request, whatever the digest holds
  {
    const char* hostile[3] = {"GET_BLOCK\nGET_BLOCK\n", "\n\n\n\n\n\n\n\n\n\n\n\n\n\n\n\n\n\n\n\n",
                              "BLOCK_DATA\n12345678\n"};
    for (int c = 0; c < 4; c++) {
      uint8_t* d = static_cast<uint8_t*>(malloc(sfwp::kDigest));
      for (uint32_t k = 0; k < sfwp::kDigest; k++) d[k] = c < 3 ? (uint8_t)hostile[c][k] : (uint8_t)(200 + k);
      uint8_t* out = static_cast<uint8_t*>(malloc(sfwp::kGetBlock));
      memset(out, 0x5A, sfwp::kGetBlock);
      write_get_block(out, d);
      CHECK(memcmp(out, "GET_BLOCK\n", 10) == 0 && memcmp(out + 10, d, 20) == 0 && out[30] == '\n');
      CHECK(sfwp::is_get_block(out));
      CHECK(sfwp::classify_get_block(out, sfwp::kGetBlock) == sfwp::kHeader);
      free(out);
      free(d);
    }
  }
  // place: a present row and a row without a message do nothing; sizes decide the rest
  CHECK(place(1, 3, 10, 10) == kNone && place(255, 3, 10, 11) == kNone);
  CHECK(place(0, -1, 10, 10) == kNone && place(0, INT64_MIN, 0, 0) == kNone);
  CHECK(place(0, 0, 10, 10) == kJob && place(0, 7, 0, 0) == kJob && place(0, 7, 0xFFFFFFFFu, 0xFFFFFFFFu) == kJob);
  CHECK(place(0, 0, 10, 11) == kMismatch && place(0, 5, 0, 0xFFFFFFFFu) == kMismatch);
  static_assert(place(0, 0, 1, 1) == kJob && kJob == 1, "the scan counts the rows of class 1");
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
