// The sending side's framing rules (syncfast_amd/csrc/sf_wire_data.hpp:
// block_data_len, write_block_data, is_get_block, classify_get_block,
// parse_get_block_run) alone, on a CPU: a stand-alone program built with
// ASan + UBSan by tests/test_block_data_write.py.  Every input is parsed from
// a heap copy of its exact length and every header written into a heap buffer
// of its exact length, so a read or store one byte out is a report.
//
//   (no argument)  checks the writer and the fixed table; prints "ok"
//   --writer       "size length header-hex" per size of the writer's list
//   --table        "name run-hex count consumed stop" per row of the table
//   FILE           "count consumed stop" of the run in FILE
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../syncfast_amd/csrc/sf_wire_data.hpp"

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

// The digest every written header carries: a newline and a 'B' among its bytes.
static void digest_of(uint32_t size, uint8_t d[20]) {
  for (uint32_t k = 0; k < 20; k++) d[k] = (uint8_t)(size * 31 + k * 13 + 1);
  d[5] = '\n';
  d[6] = 'B';
}

static std::vector<uint32_t> writer_sizes() {
  std::vector<uint32_t> v{0};
  for (uint64_t p = 10; p <= 1000000000ull; p *= 10) { v.push_back((uint32_t)(p - 1)); v.push_back((uint32_t)p); }
  v.push_back(0xFFFFFFFFu);
  return v;
}

// The header in a heap buffer of exactly its length and the end byte in one of
// its own; for sizes a test can afford, the whole message in one buffer too.
static std::string written(uint32_t size, uint64_t* len) {
  uint8_t d[20];
  digest_of(size, d);
  const uint32_t H = block_data_header_len(size);
  *len = block_data_len(size);
  uint8_t* head = static_cast<uint8_t*>(malloc(H));
  uint8_t* end = static_cast<uint8_t*>(malloc(1));
  *end = 0;
  CHECK(write_block_data(head, end, d, size) == H);
  CHECK(*end == '\n');
  CHECK(*len == (uint64_t)H + size + 1);
  const std::string h = hex(head, H);
  if (size <= 1000000) {
    uint8_t* msg = static_cast<uint8_t*>(malloc(*len));
    memset(msg, 0x5A, *len);
    CHECK(write_block_data(msg, msg + *len - 1, d, size) == H);
    CHECK(memcmp(msg, head, H) == 0 && msg[*len - 1] == '\n');
    for (uint64_t i = H; i + 1 < *len; i++)
      if (msg[i] != 0x5A) { CHECK(!"a payload byte was written"); break; }
    // what the writer wrote, the receiving rule reads
    uint32_t H2 = 0;
    uint64_t s2 = 0;
    CHECK(data_message(msg, *len, &H2, &s2) == *len && H2 == H && s2 == size);
    free(msg);
  }
  free(head);
  free(end);
  return h;
}

struct Row {
  std::string name, run;
};

static std::string get(uint8_t fill) { return "GET_BLOCK\n" + std::string(20, (char)fill) + "\n"; }

static std::vector<Row> table() {
  std::vector<Row> t;
  const std::string three = get(1) + get(0xFF) + get('G');
  t.push_back({"empty", ""});
  t.push_back({"one", get(7)});
  t.push_back({"three", three});
  for (size_t k = 1; k < kGetBlock; k++) t.push_back({"prefix", three.substr(0, 2 * kGetBlock + k)});
  for (size_t k = 1; k < kGetBlock; k++) t.push_back({"prefix-first", three.substr(0, k)});
  std::string bad = three;
  bad[2 * kGetBlock + 30] = 'x';
  t.push_back({"end-byte", bad});
  bad = three + get(9);
  bad[kGetBlock + 30] = 0;
  t.push_back({"end-byte-middle", bad});
  t.push_back({"digest-of-tags", "GET_BLOCK\nGET_BLOCK\nGET_BLOCK\n\n" + get(3)});
  t.push_back({"digest-of-newlines", "GET_BLOCK\n" + std::string(20, '\n') + "\n" + get(4) + "GET_BLOCK\n" +
                                         std::string(20, '\n') + "\n"});
  t.push_back({"digest-of-newlines-cut", "GET_BLOCK\n" + std::string(20, '\n')});
  const char* others[8] = {"FILE_ENTRY", "END_FILES", "GET_FILE", "FILE_START", "FILE_END", "FILE_BLOCK", "BLOCK_DATA",
                           "COMPLETE"};
  for (const char* o : others) {
    t.push_back({"other", three + o + "\n"});
    t.push_back({"other-more", get(2) + o + "\nname\n12\n" + std::string(20, 'd') + "\n"});
    t.push_back({"other-cut", three + std::string(o).substr(0, strlen(o) - 1)});
  }
  t.push_back({"other-first", "COMPLETE\n"});
  t.push_back({"unknown", three + "NOPE\n"});
  t.push_back({"lower-case", three + "get_block\n" + std::string(21, '\n')});
  t.push_back({"tag-space", three + "GET_BLOCK \n" + std::string(21, 'x')});
  t.push_back({"no-newline-19", three + std::string(19, 'A')});
  t.push_back({"no-newline-20", three + std::string(20, 'A')});
  t.push_back({"no-newline-40", three + std::string(40, 'A')});
  t.push_back({"newline-at-20", three + std::string(20, 'A') + "\n"});
  t.push_back({"empty-line", three + "\n"});
  return t;
}

static void parse(const std::string& run, uint64_t* count, uint64_t* consumed, int* stop) {
  uint8_t* b = static_cast<uint8_t*>(malloc(run.size() ? run.size() : 1));
  memcpy(b, run.data(), run.size());
  parse_get_block_run(b, run.size(), count, consumed, stop);
  CHECK(*consumed == kGetBlock * *count && *consumed <= run.size());
  // the one-lane test of a slot and the serial rule agree on every whole slot
  for (uint64_t k = 0; k < run.size() / kGetBlock; k++)
    CHECK(is_get_block(b + kGetBlock * k) == (classify_get_block(b + kGetBlock * k, run.size() - kGetBlock * k) == kHeader));
  // the stop is decided from at most 128 bytes there, the rest unseen
  const uint64_t avail = run.size() - *consumed, nt = avail < 128 ? avail : 128;
  uint8_t* tail = static_cast<uint8_t*>(malloc(nt ? nt : 1));
  memcpy(tail, b + *consumed, nt);
  CHECK(classify_get_block(tail, avail) == *stop);
  free(tail);
  free(b);
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "--writer" || mode.empty()) {
    for (uint32_t size : writer_sizes()) {
      uint64_t len = 0;
      const std::string h = written(size, &len);
      if (!mode.empty()) printf("%u %llu %s\n", size, (unsigned long long)len, h.c_str());
    }
  }
  if (mode == "--table" || mode.empty()) {
    bool seen[4] = {false, false, false, false};
    for (const Row& r : table()) {
      uint64_t count = 0, consumed = 0;
      int stop = -9;
      parse(r.run, &count, &consumed, &stop);
      CHECK(stop >= 0 && stop <= 3);
      if (stop >= 0 && stop <= 3) seen[stop] = true;
      if (!mode.empty())
        printf("%s %s %llu %llu %d\n", r.name.c_str(), hex(reinterpret_cast<const uint8_t*>(r.run.data()), r.run.size()).c_str(),
               (unsigned long long)count, (unsigned long long)consumed, stop);
    }
    CHECK(seen[0] && seen[1] && seen[2] && seen[3]);
  }
  if (!mode.empty() && mode[0] != '-') {
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::string run;
    char buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) run.append(buf, n);
    fclose(f);
    uint64_t count = 0, consumed = 0;
    int stop = -9;
    parse(run, &count, &consumed, &stop);
    printf("%llu %llu %d\n", (unsigned long long)count, (unsigned long long)consumed, stop);
  }
  if (fails) return 1;
  if (mode.empty()) printf("ok\n");
  return 0;
}
