// wire_data.cpp -- the BLOCK_DATA framing rules (syncfast_amd/csrc/sf_wire_data.hpp)
// alone: a stand-alone program, built with ASan + UBSan by
// tests/test_wire_data.py and run directly.  No GPU, no library.
//
//   wire_data           checks classify_data, data_message, parse_data_run
//                       and walk_candidates against the table below and
//                       prints "ok".  The expected values are what
//                       syncfast_amd.wire.Parser (the mirror of the
//                       reference's proto.rs:189-477) gives for these inputs,
//                       not the code under test's: the driver holds the
//                       table (wire_data --table prints it: name, run in
//                       hex, count, consumed, stop, need, offset:size pairs)
//                       against that parser.  Every input is parsed from a
//                       heap copy of its exact length, so a read past the end
//                       is an ASan report.
//   wire_data FILE      parses FILE twice -- parse_data_run, and
//                       walk_candidates over the candidates data_message
//                       finds at every position -- fails if the two differ,
//                       and prints "count consumed stop need too_large
//                       walk_needed candidates" and one "digest-hex size
//                       offset" line per message.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../syncfast_amd/csrc/sf_wire_data.hpp"

namespace {

using Bytes = std::string;

const Bytes kD1(20, '\x11'), kD2 = Bytes("\n\n\n\n\n", 5) + Bytes(15, 'B');

Bytes msg(const Bytes& digest, const Bytes& field, const Bytes& payload, const Bytes& end = "\n") {
  return "BLOCK_DATA\n" + digest + "\n" + field + "\n" + payload + end;
}

struct Case {
  const char* name;
  Bytes run;
  uint64_t count, consumed;
  int stop;
  uint64_t need;
  bool too_large;
  std::vector<uint64_t> sizes, offsets;
};

std::vector<Case> cases() {
  const Bytes m1 = msg(kD1, "5", "hello"), m0 = msg(kD2, "0", ""), m3 = msg(kD1, "3", "a\nb");
  const uint64_t a = m1.size(), b = a + m0.size();  // 40, 75
  std::vector<Case> c = {
      {"empty", "", 0, 0, 0, 0, false, {}, {}},
      {"one", m1, 1, 40, 0, 0, false, {5}, {34}},
      {"zero_length", m0, 1, 35, 0, 0, false, {0}, {34}},
      {"three", m1 + m0 + m3, 3, 113, 0, 0, false, {5, 0, 3}, {34, a + 34, b + 34}},
      {"plus", msg(kD1, "+5", "hello"), 1, 41, 0, 0, false, {5}, {35}},
      {"zeros", msg(kD1, "007", "1234567"), 1, 44, 0, 0, false, {7}, {36}},
      {"fifteen_digits", msg(kD1, "000000000000002", "ab"), 1, 51, 0, 0, false, {2}, {48}},
      {"sixteen_digits", m1 + msg(kD1, "0000000000000002", "ab"), 1, 40, 3, 0, false, {5}, {34}},
      {"empty_field", m1 + msg(kD1, "", ""), 1, 40, 3, 0, false, {5}, {34}},
      {"field_1a", m1 + msg(kD1, "1a", "x"), 1, 40, 3, 0, false, {5}, {34}},
      {"field_plus_only", m1 + msg(kD1, "+", ""), 1, 40, 3, 0, false, {5}, {34}},
      {"field_minus", m1 + msg(kD1, "-1", "x"), 1, 40, 3, 0, false, {5}, {34}},
      {"wrong_end_byte", m1 + msg(kD1, "5", "hello", "X"), 1, 40, 3, 0, false, {5}, {34}},
      {"wrong_end_byte_first", msg(kD1, "5", "hello", "X") + m1, 0, 0, 3, 0, false, {}, {}},
      {"end_byte_missing", m1 + msg(kD1, "5", "hello", ""), 1, 40, 1, 40, false, {5}, {34}},
      {"fifteen_digits_open", m1 + "BLOCK_DATA\n" + kD1 + "\n999999999999999\n", 1, 40, 1, 48 + 999999999999999ull + 1,
       false, {5}, {34}},
      {"fifteen_open", m1 + "BLOCK_DATA\n" + kD1 + "\n111111111111111", 1, 40, 3, 0, false, {5}, {34}},
      {"fourteen_open", m1 + "BLOCK_DATA\n" + kD1 + "\n11111111111111", 1, 40, 1, 0, false, {5}, {34}},
      {"digest_unterminated", m1 + "BLOCK_DATA\n" + kD1 + "x1\nx\n", 1, 40, 3, 0, false, {5}, {34}},
      {"file_end", m1 + "FILE_END\n", 1, 40, 2, 0, false, {5}, {34}},
      {"file_block", m1 + "FILE_BLOCK\n" + kD1 + "\n5\n", 1, 40, 2, 0, false, {5}, {34}},
      {"get_block", m1 + "GET_BLOCK\n", 1, 40, 2, 0, false, {5}, {34}},
      {"file_entry", "FILE_ENTRY\nx", 0, 0, 2, 0, false, {}, {}},
      {"end_files", "END_FILES\n", 0, 0, 2, 0, false, {}, {}},
      {"get_file", "GET_FILE\n", 0, 0, 2, 0, false, {}, {}},
      {"file_start", "FILE_START\nname", 0, 0, 2, 0, false, {}, {}},
      {"complete", m1 + "COMPLETE\n", 1, 40, 2, 0, false, {5}, {34}},
      {"unknown", m1 + "BOGUS\n", 1, 40, 3, 0, false, {5}, {34}},
      {"lowercase", "block_data\n" + kD1 + "\n0\n\n", 0, 0, 3, 0, false, {}, {}},
      {"x20", m1 + Bytes(20, 'X'), 1, 40, 3, 0, false, {5}, {34}},
      {"x19", m1 + Bytes(19, 'X'), 1, 40, 1, 0, false, {5}, {34}},
      {"newline_first", "\n" + m1, 0, 0, 3, 0, false, {}, {}},
      {"too_large", "BLOCK_DATA\n" + kD1 + "\n4294967296\n", 0, 0, 1, 43 + 4294967296ull + 1, false, {}, {}},
      // a whole message as payload, and the tag alone: read as payload bytes
      {"nested", msg(kD1, "40", m1) + m0, 2, 111, 0, 0, false, {40, 0}, {35, 110}},
      {"tags", msg(kD1, "22", "BLOCK_DATA\nBLOCK_DATA\n"), 1, 58, 0, 0, false, {22}, {35}},
      // a header in the first payload announces 43 bytes and lands on the second message's end byte
      {"crossing", msg(kD1, "38", "BLOCK_DATA\n" + kD1 + "\n43\nxyz") + m1, 2, 114, 0, 0, false, {38, 5}, {35, 108}},
  };
  // every proper prefix of the last message: incomplete, with the need once
  // the header is whole (35 bytes: a two-digit length)
  const Bytes last = msg(kD2, "12", "payload\nmore");
  for (size_t t = 1; t < last.size(); t++)
    c.push_back({"prefix", m1 + last.substr(0, t), 1, 40, 1, t >= 35 ? last.size() : 0, false, {5}, {34}});
  return c;
}

struct Parse {
  std::vector<uint8_t> digests;
  std::vector<uint32_t> sizes;
  std::vector<uint64_t> offsets;
  uint64_t count = 0, consumed = 0, need = 77;
  int stop = -9;
  bool too_large = false;
};

uint8_t* heap_copy(const uint8_t* run, uint64_t n) {
  uint8_t* copy = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(copy, run, n);
  return copy;
}

// parse_data_run over a heap copy of exactly n bytes, outputs of exactly `cap` entries
Parse parse(const uint8_t* run, uint64_t n, uint64_t cap) {
  uint8_t* copy = heap_copy(run, n);
  Parse p;
  p.digests.resize(cap * 20);
  p.sizes.resize(cap);
  p.offsets.resize(cap);
  sfwp::parse_data_run(copy, n, cap ? p.digests.data() : nullptr, cap ? p.sizes.data() : nullptr,
                       cap ? p.offsets.data() : nullptr, cap, &p.count, &p.consumed, &p.stop, &p.need, &p.too_large);
  free(copy);
  return p;
}

// The same run through the parallel form's definition: candidates by
// data_message at every position of a heap copy, the chain by
// walk_candidates, the stop by classify_data at its end.  *walk_needed: the
// link test finds a candidate inside the first unlinked message.
Parse walk(const uint8_t* run, uint64_t n, bool* walk_needed, uint64_t* n_cand) {
  uint8_t* copy = heap_copy(run, n);
  std::vector<uint64_t> pos, len, hdr;
  for (uint64_t at = 0; at < n; at++) {
    uint32_t H = 0;
    uint64_t size = 0;
    const uint64_t L = sfwp::data_message(copy + at, n - at, &H, &size);
    if (L) {
      pos.push_back(at);
      len.push_back(L);
      hdr.push_back(H);
    }
  }
  *n_cand = pos.size();
  *walk_needed = false;
  if (!pos.empty() && pos[0] == 0)
    for (size_t i = 0; i < pos.size(); i++)
      if (i + 1 == pos.size() || pos[i + 1] != pos[i] + len[i]) {
        *walk_needed = i + 1 < pos.size() && pos[i + 1] < pos[i] + len[i];
        break;
      }
  std::vector<uint64_t> chain(pos.size() + 1);
  Parse p;
  p.count = sfwp::walk_candidates(pos.data(), len.data(), pos.size(), chain.data());
  if (sfwp::walk_candidates(pos.data(), len.data(), pos.size(), nullptr) != p.count) p.count = ~0ull;
  for (uint64_t k = 0; k < p.count && k < pos.size(); k++) {
    const uint64_t c = chain[k], size = len[c] - hdr[c] - 1;
    p.digests.insert(p.digests.end(), copy + pos[c] + 11, copy + pos[c] + 31);
    p.sizes.push_back((uint32_t)size);
    p.offsets.push_back(pos[c] + hdr[c]);
    p.consumed = pos[c] + len[c];
    if (size > 0xFFFFFFFFull) p.too_large = true;
  }
  uint32_t H = 0;
  uint64_t size = 0;
  p.stop = sfwp::classify_data(copy + p.consumed, n - p.consumed, &H, &size, &p.need);
  free(copy);
  return p;
}

bool same(const Parse& a, const Parse& b) {
  return a.count == b.count && a.consumed == b.consumed && a.stop == b.stop && a.need == b.need &&
         a.too_large == b.too_large && a.digests == b.digests && a.sizes == b.sizes && a.offsets == b.offsets;
}

int fail(const char* name, const char* what) {
  printf("FAIL %s: %s\n", name, what);
  return 1;
}

int check_table() {
  for (const Case& c : cases()) {
    const uint8_t* run = reinterpret_cast<const uint8_t*>(c.run.data());
    const uint64_t n = c.run.size();
    const Parse p = parse(run, n, n / 35 + 1);
    if (p.count != c.count) return fail(c.name, "count");
    if (p.consumed != c.consumed) return fail(c.name, "consumed");
    if (p.stop != c.stop) return fail(c.name, "stop");
    if (p.need != c.need) return fail(c.name, "need");
    if (p.too_large != c.too_large) return fail(c.name, "too_large");
    for (uint64_t i = 0; i < c.count; i++)
      if (p.sizes[i] != (uint32_t)c.sizes[i] || p.offsets[i] != c.offsets[i]) return fail(c.name, "sizes or offsets");
    // the digests are the 20 bytes after each message's tag
    uint64_t at = 0;
    for (uint64_t i = 0; i < c.count; i++) {
      if (memcmp(p.digests.data() + 20 * i, run + at + 11, 20) != 0) return fail(c.name, "digests");
      at = c.offsets[i] + c.sizes[i] + 1;
    }
    // the query form and a short capacity: the same count, the first entries only
    const Parse q = parse(run, n, 0);
    if (q.count != c.count || q.consumed != c.consumed || q.stop != c.stop || q.need != c.need)
      return fail(c.name, "query form");
    if (c.count > 1) {
      const Parse h = parse(run, n, c.count - 1);
      if (h.count != c.count || memcmp(h.digests.data(), p.digests.data(), 20 * (c.count - 1)) != 0)
        return fail(c.name, "short capacity");
    }
    // the candidates' chain is the serial parse
    bool walk_needed = false;
    uint64_t n_cand = 0;
    Parse w = walk(run, n, &walk_needed, &n_cand);
    Parse full = p;
    full.digests.resize(20 * p.count);
    full.sizes.resize(p.count);
    full.offsets.resize(p.count);
    if (!same(w, full)) return fail(c.name, "walk_candidates and parse_data_run differ");
    // data_message at every position of a heap copy: a whole message stands
    // exactly where classify_data says one does, with the same lengths
    uint8_t* copy = heap_copy(run, n);
    for (uint64_t k = 0; k < n; k++) {
      uint64_t s1 = 0, s2 = 0, need = 0;
      uint32_t h1 = 0, h2 = 0;
      const uint64_t m = sfwp::data_message(copy + k, n - k, &h1, &s1);
      const int cl = sfwp::classify_data(copy + k, n - k, &h2, &s2, &need);
      if ((m != 0) != (cl == sfwp::kData) || (m && (h1 != h2 || s1 != s2 || m != h1 + s1 + 1 || h1 < 34 || h1 > 48))) {
        free(copy);
        return fail(c.name, "data_message and classify_data differ");
      }
    }
    free(copy);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    if (check_table()) return 1;
    printf("ok\n");
    return 0;
  }
  if (strcmp(argv[1], "--table") == 0) {
    for (const Case& c : cases()) {
      printf("%s ", c.name);
      for (unsigned char ch : c.run) printf("%02x", ch);
      if (c.run.empty()) printf("-");
      printf(" %llu %llu %d %llu", (unsigned long long)c.count, (unsigned long long)c.consumed, c.stop,
             (unsigned long long)c.need);
      for (size_t i = 0; i < c.sizes.size(); i++)
        printf(" %llu:%llu", (unsigned long long)c.offsets[i], (unsigned long long)c.sizes[i]);
      printf("\n");
    }
    return 0;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> run;
  uint8_t buf[4096];
  for (size_t r; (r = fread(buf, 1, sizeof(buf), f)) > 0;) run.insert(run.end(), buf, buf + r);
  fclose(f);
  Parse p = parse(run.data(), run.size(), run.size() / 35 + 1);
  p.digests.resize(20 * p.count);
  p.sizes.resize(p.count);
  p.offsets.resize(p.count);
  bool walk_needed = false;
  uint64_t n_cand = 0;
  const Parse w = walk(run.data(), run.size(), &walk_needed, &n_cand);
  if (!same(w, p)) return fail(argv[1], "walk_candidates and parse_data_run differ");
  printf("%llu %llu %d %llu %d %d %llu\n", (unsigned long long)p.count, (unsigned long long)p.consumed, p.stop,
         (unsigned long long)p.need, (int)p.too_large, (int)walk_needed, (unsigned long long)n_cand);
  for (uint64_t i = 0; i < p.count; i++) {
    for (int k = 0; k < 20; k++) printf("%02x", p.digests[20 * i + k]);
    printf(" %u %llu\n", p.sizes[i], (unsigned long long)p.offsets[i]);
  }
  return 0;
}
