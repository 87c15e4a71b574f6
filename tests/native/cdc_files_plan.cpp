// The plan of the many-file device ZPAQ cut (syncfast_amd/csrc/
// sf_cdc_files_plan.hpp) executed serially on a CPU: a stand-alone program
// built with ASan + UBSan by tests/test_zpaq_files_plan.py, together with the
// host cutter (sf_zpaq.cpp), which is the definition of the boundaries.
//
// One loop iteration stands for one lane of sf_cdc_files.hip's kernels --
// round 0, the join launches, count, scan, emit, first_row -- with the
// geometry taken from the plan header and the per-byte step from
// sf_zpaq_step.hpp.  Every array has its exact length on the heap, and every
// store to a bitmap or a row goes through a checker:
//   - a bitmap word is stored only by the segment that owns it, lies inside
//     the bitmaps, and in round 0 every word is stored by exactly one segment;
//   - every row is written exactly once and lies inside [0, total);
//   - every settled file's rows are sf_zpaq_cut_buffer's of its bytes;
//   - under a cap the unsettled files are exactly those whose own round count
//     (the file cut alone, no cap) is at least max_rounds, and with no cap the
//     launches made are the largest round count plus one.
// Prints "ok <batches> <files>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/syncfast_amd.h"
#include "../../syncfast_amd/csrc/sf_cdc_files_plan.hpp"
#include "../../syncfast_amd/csrc/sf_zpaq_step.hpp"

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      if (fails < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
      fails++;                                                \
    }                                                         \
  } while (0)

static uint64_t gcd64(uint64_t a, uint64_t b) { return b ? gcd64(b, a % b) : a; }
static uint64_t segment_len(uint32_t max_size) { return (uint64_t)max_size / gcd64(max_size, 32) * 32; }

// A lane's chunker, byte by byte.
struct Chunker {
  uint32_t lim, max_size, h, c1, run;
  uint8_t o1[256];
  void fresh() {
    h = sfz::kFreshH;
    c1 = run = 0;
    memset(o1, 0, sizeof o1);
  }
  bool feed(uint8_t b) {
    h = sfz::step(h, b, o1[c1]);
    o1[c1] = b;
    c1 = b;
    run++;
    if (!sfz::cuts(h, lim, run, max_size)) return false;
    fresh();
    return true;
  }
};

// The bitmaps: heap arrays of exactly nwords words; a store names its segment.
struct Bitmaps {
  uint64_t nwords;
  uint32_t *spec, *cur;
  std::vector<int64_t> spec_by, cur_by;  // the segment that stored the word in this pass, or -1
  uint64_t lo = 0, hi = 0;               // global words the storing segment owns: [lo, hi]
  int64_t seg = -1;
  explicit Bitmaps(uint64_t n) : nwords(n), spec_by(n, -1), cur_by(n, -1) {
    spec = static_cast<uint32_t*>(malloc(n * 4 + !n));
    cur = static_cast<uint32_t*>(malloc(n * 4 + !n));
    memset(spec, 0xA5, n * 4);
    memset(cur, 0x5A, n * 4);
  }
  ~Bitmaps() {
    free(spec);
    free(cur);
  }
  void new_pass() {
    std::fill(spec_by.begin(), spec_by.end(), -1);
    std::fill(cur_by.begin(), cur_by.end(), -1);
  }
  void owner(int64_t s, uint64_t base, const sfzf::Seg& g) {
    seg = s;
    lo = base + g.w0;
    hi = base + g.wend;
  }
  bool mine(uint64_t w) {
    CHECK(w < nwords);
    CHECK(w >= lo && w <= hi);
    return w < nwords && w >= lo && w <= hi;
  }
  void store_spec(uint64_t w, uint32_t v) {
    if (!mine(w)) return;
    CHECK(spec_by[w] == -1);
    spec_by[w] = seg;
    spec[w] = v;
  }
  void store_cur(uint64_t w, uint32_t v, bool again = false) {  // again: the same lane's OR of the last bit
    if (!mine(w)) return;
    CHECK(again ? cur_by[w] == seg : cur_by[w] == -1);
    cur_by[w] = seg;
    cur[w] = v;
  }
};

// CutWriter of sf_cdc_lane.hpp, its stores through the checker.  base: the
// file's first word.
struct Writer {
  Bitmaps& B;
  uint64_t base;
  bool both;
  uint64_t w;
  uint32_t acc;
  void store(uint64_t k, uint32_t v) {
    B.store_cur(base + k, v);
    if (both) B.store_spec(base + k, v);
  }
  void advance(uint64_t wi) {
    store(w, acc);
    for (uint64_t k = w + 1; k < wi; k++) store(k, 0u);
    w = wi;
    acc = 0;
  }
  void put(uint64_t i) {
    if ((i >> 5) != w) advance(i >> 5);
    acc |= 1u << (i & 31);
  }
  void finish(uint64_t wend) { advance(wend + 1); }
};

struct Result {
  uint32_t launches = 0;
  uint64_t total = 0;
  std::vector<uint8_t> unsettled;
  std::vector<uint64_t> first_row, offsets;
  std::vector<uint32_t> sizes, round;
};

// The whole call, one iteration per lane.
static Result run(const uint8_t* data, const std::vector<uint64_t>& off, const std::vector<uint64_t>& len, uint32_t bits,
                  uint32_t max_size, uint32_t max_rounds) {
  const uint32_t n = (uint32_t)len.size();
  const uint64_t L = segment_len(max_size);
  const uint32_t lim = sfz::limit(bits);
  std::vector<uint64_t> seg_first(n + 1), word_first(n + 1);
  sfzf::fill_firsts(len.data(), n, L, seg_first.data(), word_first.data());
  const uint64_t nseg = seg_first[n];
  uint64_t most = 0;
  for (uint32_t f = 0; f < n; f++) {
    most = std::max(most, seg_first[f + 1] - seg_first[f]);
    CHECK(seg_first[f + 1] - seg_first[f] == (len[f] + L - 1) / L);
    CHECK(word_first[f + 1] - word_first[f] == (len[f] + 31) / 32);
  }
  Result R;
  R.unsettled.assign(n, 0);
  R.first_row.assign(n + 1, 0);
  R.round.assign(n, 0);
  if (nseg == 0) return R;
  Bitmaps B(word_first[n]);
  std::vector<uint64_t> last[2] = {std::vector<uint64_t>(nseg), std::vector<uint64_t>(nseg)}, lastspec(nseg), used(nseg),
                        counts(nseg), ends(nseg);
  auto seg_of = [&](uint64_t s) {
    const uint32_t f = sfzf::file_of(seg_first.data(), n, s);
    CHECK(seg_first[f] <= s && s < seg_first[f + 1]);
    const sfzf::Seg g = sfzf::segment(f, seg_first[f], len[f], L, s);
    CHECK(g.s0 < g.s1 && g.s1 <= len[f] && g.s1 - g.s0 <= L && g.s0 % 32 == 0);
    return g;
  };
  // round 0
  for (uint64_t s = 0; s < nseg; s++) {
    const sfzf::Seg g = seg_of(s);
    const uint8_t* fdata = data + off[g.file];
    B.owner((int64_t)s, word_first[g.file], g);
    Chunker z{lim, max_size, 0, 0, 0, {}};
    z.fresh();
    Writer wr{B, word_first[g.file], true, g.w0, 0u};
    uint64_t lastcut = g.s0;
    for (uint64_t p = g.s0; p < g.s1; p++)
      if (z.feed(fdata[p])) {
        wr.put(p);
        lastcut = p + 1;
      }
    wr.finish(g.wend);
    if (g.last(len[g.file])) {
      const uint64_t w = word_first[g.file] + ((len[g.file] - 1) >> 5);
      B.store_cur(w, B.cur[w] | 1u << ((len[g.file] - 1) & 31), true);
    }
    last[0][s] = lastspec[s] = lastcut;
    used[s] = g.s0;
  }
  for (uint64_t w = 0; w < B.nwords; w++) CHECK(B.spec_by[w] >= 0 && B.cur_by[w] >= 0);  // every word, once
  // the join launches
  int in = 0;
  uint32_t changed = 0;
  while (most > 1 && (max_rounds == 0 || R.launches < max_rounds)) {
    CHECK(R.launches <= most);
    B.new_pass();
    changed = 0;
    const uint32_t r = R.launches + 1;
    for (uint64_t s = 0; s < nseg; s++) {
      const sfzf::Seg g = seg_of(s);
      const uint32_t f = g.file;
      if (g.first()) {
        last[in ^ 1][s] = last[in][s];
        continue;
      }
      CHECK(sfzf::incoming_from(s) >= seg_first[f]);  // the same file's
      const uint64_t inc = last[in][sfzf::incoming_from(s)];
      CHECK(inc <= g.s0 && inc + max_size > g.s0);
      if (inc == used[s]) {
        last[in ^ 1][s] = last[in][s];
        continue;
      }
      used[s] = inc;
      R.round[f] = r;
      changed++;
      const uint8_t* fdata = data + off[f];
      const uint64_t wb = word_first[f];
      B.owner((int64_t)s, wb, g);
      Chunker z{lim, max_size, 0, 0, 0, {}};
      z.fresh();
      Writer wr{B, wb, false, g.w0, 0u};
      uint64_t lastcut = inc, p = inc;
      bool synced = false;
      while (p < g.s1) {
        const bool cut = z.feed(fdata[p]);
        p++;
        if (!cut || p <= g.s0) continue;
        const uint64_t i = p - 1;
        wr.put(i);
        lastcut = p;
        if (B.spec[wb + (i >> 5)] & (1u << (i & 31))) {
          synced = true;
          break;
        }
      }
      if (synced) {
        const uint64_t i = p - 1, w = i >> 5;
        B.store_cur(wb + w, wr.acc | (B.spec[wb + w] & sfzf::above_bit(i)));
        for (uint64_t k = w + 1; k <= g.wend; k++) B.store_cur(wb + k, B.spec[wb + k]);
        lastcut = lastspec[s];
      } else {
        wr.finish(g.wend);
      }
      if (g.last(len[f])) {
        const uint64_t w = wb + ((len[f] - 1) >> 5);
        B.store_cur(w, B.cur[w] | 1u << ((len[f] - 1) & 31), true);
      }
      last[in ^ 1][s] = lastcut;
    }
    R.launches++;
    in ^= 1;
    if (!changed) break;
  }
  // count, scan
  for (uint32_t f = 0; f < n; f++) R.unsettled[f] = sfzf::unsettled(R.round[f], R.launches);
  for (uint64_t s = 0; s < nseg; s++) {
    const sfzf::Seg g = seg_of(s);
    uint64_t c = 0;
    if (!R.unsettled[g.file])
      for (uint64_t w = g.w0; w <= g.wend; w++) c += (uint64_t)__builtin_popcount(B.cur[word_first[g.file] + w]);
    counts[s] = c;
  }
  for (uint64_t s = 0, acc = 0; s < nseg; s++) ends[s] = acc += counts[s];
  R.total = ends[nseg - 1];
  // emit: heap rows of exactly `total`, each written once
  uint64_t* offsets = static_cast<uint64_t*>(malloc(R.total * 8 + !R.total));
  uint32_t* sizes = static_cast<uint32_t*>(malloc(R.total * 4 + !R.total));
  std::vector<uint8_t> written(R.total, 0);
  for (uint64_t s = 0; s < nseg; s++) {
    uint64_t row = sfzf::row_base(ends.data(), s);
    const uint64_t row_end = ends[s];
    if (row == row_end) continue;
    const sfzf::Seg g = seg_of(s);
    uint64_t prev = g.first() ? 0 : last[in][sfzf::incoming_from(s)];
    for (uint64_t w = g.w0; w <= g.wend; w++) {
      uint32_t m = B.cur[word_first[g.file] + w];
      while (m && row < row_end) {
        const uint64_t end = (w << 5) + (uint64_t)__builtin_ffs((int)m);
        m &= m - 1;
        CHECK(row < R.total);
        if (row < R.total) {
          CHECK(!written[row]);
          written[row] = 1;
          offsets[row] = off[g.file] + prev;
          sizes[row] = (uint32_t)(end - prev);
        }
        prev = end;
        row++;
      }
    }
    CHECK(row == row_end);
  }
  for (uint64_t k = 0; k < R.total; k++) CHECK(written[k]);
  R.offsets.assign(offsets, offsets + R.total);
  R.sizes.assign(sizes, sizes + R.total);
  free(offsets);
  free(sizes);
  for (uint32_t f = 0; f <= n; f++) R.first_row[f] = sfzf::first_row(seg_first.data(), ends.data(), f);
  CHECK(R.first_row[n] == R.total);
  return R;
}

// rows [first_row[f], first_row[f + 1]) of R against the host cutter
static void check_rows(const Result& R, const uint8_t* data, const std::vector<uint64_t>& off,
                       const std::vector<uint64_t>& len, uint32_t bits, uint32_t max_size) {
  for (uint32_t f = 0; f < len.size(); f++) {
    const uint64_t a = R.first_row[f], b = R.first_row[f + 1];
    CHECK(a <= b && b <= R.total);
    if (R.unsettled[f]) {
      CHECK(a == b);
      continue;
    }
    uint64_t need = 0;
    sf_zpaq_cut_buffer(data + off[f], len[f], bits, max_size, nullptr, nullptr, 0, &need);
    std::vector<uint64_t> o(need + 1);
    std::vector<uint32_t> z(need + 1);
    CHECK(sf_zpaq_cut_buffer(data + off[f], len[f], bits, max_size, o.data(), z.data(), need, &need) == SF_OK);
    CHECK(b - a == need);
    for (uint64_t k = 0; k < need && b - a == need; k++)
      CHECK(R.offsets[a + k] == off[f] + o[k] && R.sizes[a + k] == z[k]);
  }
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

enum Kind { RANDOM, ZEROS, PERIOD7, ISLANDS, KINDS };

static void fill(uint8_t* p, uint64_t n, int kind, uint64_t L) {
  static const uint8_t pat7[7] = {3, 141, 59, 26, 53, 58, 97};
  switch (kind) {
    case RANDOM:
      for (uint64_t i = 0; i < n; i++) p[i] = (uint8_t)rnd();
      break;
    case ZEROS:
      memset(p, 0, n);
      break;
    case PERIOD7:
      for (uint64_t i = 0; i < n; i++) p[i] = pat7[i % 7];
      break;
    default: {  // stretches of random bytes alternating with stretches of a repeated pattern
      static const uint32_t periods[7] = {1, 2, 3, 7, 13, 32, 33};
      uint64_t i = 0;
      while (i < n) {
        for (uint64_t m = L / 2 + rnd() % (3 * L + L / 2 + 1); m && i < n; m--) p[i++] = (uint8_t)rnd();
        const uint32_t per = periods[rnd() % 7];
        uint8_t pat[33];
        for (uint32_t k = 0; k < per; k++) pat[k] = (uint8_t)rnd();
        uint64_t k = 0;
        for (uint64_t m = L + rnd() % (5 * L + 1); m && i < n; m--) p[i++] = pat[k++ % per];
      }
    }
  }
}

static uint64_t batches = 0, files = 0;

// One batch: files of `lens` and `kinds` placed at base offsets whose low five
// bits are phase, phase + 1, ... with gaps, in a heap buffer of the exact
// length; with no cap, then under caps.
static void batch(const std::vector<uint64_t>& lens, const std::vector<int>& kinds, uint32_t phase, uint32_t bits,
                  uint32_t max_size) {
  const uint64_t L = segment_len(max_size);
  const uint32_t n = (uint32_t)lens.size();
  std::vector<uint64_t> off(n);
  uint64_t at = 0;
  for (uint32_t f = 0; f < n; f++) {
    at += 3;  // a gap
    while ((at & 31) != ((phase + f) & 31)) at++;
    off[f] = at;
    at += lens[f];
  }
  uint8_t* data = static_cast<uint8_t*>(malloc(at + !at));
  memset(data, 0xEE, at);
  for (uint32_t f = 0; f < n; f++) fill(data + off[f], lens[f], kinds[f], L);
  // every file's own round count: cut alone, no cap
  std::vector<uint32_t> own(n);
  uint32_t most_rounds = 0;
  bool multi = false;
  for (uint32_t f = 0; f < n; f++) {
    const Result one = run(data, {off[f]}, {lens[f]}, bits, max_size, 0);
    own[f] = one.round.empty() ? 0 : one.round[0];
    CHECK(!one.unsettled[0]);
    CHECK(lens[f] <= L ? one.launches == 0 : one.launches == own[f] + 1);
    most_rounds = std::max(most_rounds, own[f]);
    multi |= lens[f] > L;
  }
  const Result all = run(data, off, lens, bits, max_size, 0);
  CHECK(all.launches == (multi ? most_rounds + 1 : 0));
  for (uint32_t f = 0; f < n; f++) CHECK(!all.unsettled[f] && all.round[f] == own[f]);
  check_rows(all, data, off, lens, bits, max_size);
  for (uint32_t cap : {1u, 2u, 6u}) {
    const Result c = run(data, off, lens, bits, max_size, cap);
    CHECK(c.launches == (multi ? std::min(most_rounds + 1, cap) : 0));
    for (uint32_t f = 0; f < n; f++) CHECK(c.unsettled[f] == (own[f] >= cap));
    check_rows(c, data, off, lens, bits, max_size);
  }
  free(data);
  batches++;
  files += n;
}

int main() {
  const uint32_t params[3][2] = {{4, 16}, {6, 256}, {5, 48}};
  for (const auto& pm : params) {
    const uint32_t bits = pm[0], max_size = pm[1];
    const uint64_t L = segment_len(max_size);
    const std::vector<uint64_t> lengths = {0, 1, 15, 16, L - 1, L, L + 1, 2 * L, 9 * L + L / 2, 40 * L};
    // every length with every content, one batch per content; empty files
    // first, last and three in a row
    for (int kind = 0; kind < KINDS; kind++) {
      std::vector<uint64_t> lens = {0};
      for (uint64_t v : lengths) lens.push_back(v);
      lens.insert(lens.begin() + 5, {0, 0, 0});
      lens.push_back(0);
      batch(lens, std::vector<int>(lens.size(), kind), 0, bits, max_size);
    }
    // every byte phase 0..31 of a file's base, contents mixed
    for (uint32_t phase = 0; phase < 32; phase++) {
      std::vector<uint64_t> lens;
      std::vector<int> kinds;
      for (uint32_t k = 0; k < 6; k++) {
        lens.push_back(lengths[(phase + 3 * k) % lengths.size()] + (k & 1) * (rnd() % (2 * L)));
        kinds.push_back((int)((phase + k) % KINDS));
      }
      batch(lens, kinds, phase, bits, max_size);
    }
    batch({}, {}, 0, bits, max_size);               // no file
    batch({0, 0, 0}, {0, 0, 0}, 5, bits, max_size);  // only empty files
  }
  // the range test: also where off + len passes 2^64
  CHECK(sfzf::in_range(0, 0, 0) && sfzf::in_range(5, 0, 5) && sfzf::in_range(2, 3, 5));
  CHECK(!sfzf::in_range(6, 0, 5) && !sfzf::in_range(2, 4, 5) && !sfzf::in_range(~0ull, 2, ~0ull));
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("ok %llu %llu\n", (unsigned long long)batches, (unsigned long long)files);
  return 0;
}
