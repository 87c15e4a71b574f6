// inplace_regions.cpp -- the page-lock regions of the in-place routes
// (syncfast_amd/csrc/sf_inplace.hpp) executed on a CPU: a stand-alone program,
// built with ASan + UBSan by tests/test_inplace_regions.py and run directly.
//
// The addresses are numbers only (nothing is dereferenced); lock and unlock
// record their calls.  Every run is driven as the pipelines drive it: region 0
// settled first, then per stage k "issue k, lock_ahead(k + 1)".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <utility>
#include <vector>

#include "../../syncfast_amd/csrc/sf_inplace.hpp"

using namespace sfi;

#define REQUIRE(c)                                                 \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

static uint64_t g_cases = 0;
static const uint64_t kPage = 4096;
static const uintptr_t kBase = (uintptr_t)0x7f12345ull * kPage;  // a page edge

static uintptr_t down(uintptr_t a) { return a - a % kPage; }
static uintptr_t up(uintptr_t a) { return down(a + kPage - 1); }

typedef std::vector<std::pair<uintptr_t, uintptr_t>> Ranges;

static bool inside_one(const Ranges& locked, uintptr_t a, uintptr_t e) {  // [a, e) wholly in one locked range
  for (const auto& r : locked)
    if (r.first <= a && e <= r.second) return true;
  return false;
}

// One run over stages of `lens` bytes from kBase + 3.  fail_at: the test hook;
// refuse: the region whose lock() answers kNotLocked (< 0: none); pinned:
// every lock() answers kPinnedByCaller.
static void drive(const std::vector<uint64_t>& lens, int64_t fail_at, int64_t refuse, bool pinned) {
  const size_t n = lens.size();
  std::vector<uintptr_t> starts(n);
  uintptr_t end = kBase + 3;
  for (size_t k = 0; k < n; k++) {
    starts[k] = end;
    end += lens[k];
  }
  // the edges, worked out here: below the first start, above every other and the end
  std::vector<uintptr_t> edge(n + 1);
  for (size_t k = 0; k <= n; k++) edge[k] = k == 0 ? down(starts[0]) : up(k < n ? starts[k] : end);
  // F: the first region that fails (n: none)
  size_t F = n;
  if (fail_at >= 0 && (uint64_t)fail_at < n) F = (size_t)fail_at;
  if (refuse >= 0 && (uint64_t)refuse < n && edge[refuse + 1] > edge[refuse]) F = (size_t)refuse;

  Ranges asked, locked;  // lock()'s calls; those answered "locked" or "pinned"
  std::vector<uintptr_t> unlocked;
  auto lock = [&](uintptr_t a, uintptr_t e) {
    REQUIRE(a < e && a % kPage == 0 && e % kPage == 0);
    for (const auto& r : asked) REQUIRE(e <= r.first || r.second <= a);  // overlaps no earlier call
    asked.push_back({a, e});
    if (refuse >= 0 && (uint64_t)refuse < n && a == edge[refuse]) return kNotLocked;
    locked.push_back({a, e});
    return pinned ? kPinnedByCaller : kLockedByUs;
  };
  auto unlock = [&](uintptr_t a) { unlocked.push_back(a); };
  {
    InplaceRegions regions(kPage, starts, end, lock, unlock, fail_at);
    REQUIRE(regions.size() == n);
    for (size_t k = 0; k <= n; k++) REQUIRE(regions.edge(k) == edge[k]);
    REQUIRE(!regions.direct(0));  // nothing is settled yet
    regions.lock_ahead(0);
    for (size_t k = 0; k < n; k++) {
      // stage k is issued: its regions were settled before
      REQUIRE(regions.direct(k) == (k < F));
      const uintptr_t src = starts[k];
      const uint64_t head = regions.head(k, src, lens[k]);
      REQUIRE(head <= lens[k]);
      if (k == 0) REQUIRE(head == 0);
      if (regions.direct(k)) {  // both pieces of the copy: each inside ONE range locked by now
        if (head) REQUIRE(inside_one(locked, src, src + head));
        if (head) REQUIRE(src + head <= edge[k]);  // region k-1
        if (lens[k] > head) REQUIRE(inside_one(locked, src + head, src + lens[k]));
        if (lens[k] > head) REQUIRE(src + head >= edge[k] && src + lens[k] <= edge[k + 1]);  // region k
      }
      const size_t calls = asked.size();
      regions.lock_ahead(k + 1);
      regions.lock_ahead(k + 1);  // settled once: a second call asks nothing
      REQUIRE(asked.size() <= calls + 1);
      if (k + 1 > F || k + 1 >= n) REQUIRE(asked.size() == calls);  // after a failure, and past the end: no call
    }
    REQUIRE(unlocked.empty());
  }
  // the calls: the non-empty regions up to the failure, in order (the refused one included)
  Ranges want;
  for (size_t k = 0; k < n && k <= F; k++)
    if (edge[k + 1] > edge[k] && (k < F || refuse >= 0)) want.push_back({edge[k], edge[k + 1]});
  REQUIRE(asked == want);
  if (F == n) {  // they tile [page_down(first start), page_up(end)) exactly and in order
    REQUIRE(!asked.empty() && asked.front().first == down(starts[0]) && asked.back().second == up(end));
    for (size_t i = 1; i < asked.size(); i++) REQUIRE(asked[i].first == asked[i - 1].second);
  }
  // unlocked: exactly what was locked by us, by its start, once each
  std::vector<uintptr_t> want_unlocked;
  if (!pinned)
    for (const auto& r : locked) want_unlocked.push_back(r.first);
  REQUIRE(unlocked == want_unlocked);
  g_cases++;
}

// The serial form: one start, one region over the whole range.
static void serial(const std::vector<uint64_t>& lens) {
  uintptr_t end = kBase + 3;
  for (uint64_t l : lens) end += l;
  Ranges asked;
  std::vector<uintptr_t> unlocked;
  auto lock = [&](uintptr_t a, uintptr_t e) {
    asked.push_back({a, e});
    return kLockedByUs;
  };
  auto unlock = [&](uintptr_t a) { unlocked.push_back(a); };
  {
    InplaceRegions regions(kPage, std::vector<uintptr_t>{kBase + 3}, end, lock, unlock);
    regions.lock_ahead(0);
    REQUIRE(regions.size() == 1 && regions.direct(0));
    uintptr_t src = kBase + 3;
    for (uint64_t l : lens) {  // every stage is copied from region 0, whole
      REQUIRE(regions.head(0, src, l) == 0);
      regions.lock_ahead(1);
      src += l;
    }
  }
  REQUIRE(asked == Ranges({{kBase, up(end)}}));
  REQUIRE(unlocked == std::vector<uintptr_t>({kBase}));
  g_cases++;
}

// No stage in place: no region, nothing asked, nothing direct.
static void none() {
  bool called = false;
  auto lock = [&](uintptr_t, uintptr_t) {
    called = true;
    return kLockedByUs;
  };
  auto unlock = [&](uintptr_t) { called = true; };
  {
    InplaceRegions regions(kPage, std::vector<uintptr_t>(), kBase + 99, lock, unlock, 0);
    regions.lock_ahead(0);
    regions.lock_ahead(1);
    REQUIRE(regions.size() == 0 && !regions.direct(0) && !regions.direct(1));
  }
  REQUIRE(!called);
  g_cases++;
}

int main() {
  // a whole number of pages, not a page multiple, two pages and a byte; and, last only, one byte
  const uint64_t kinds[] = {256 * kPage, 1048000, 2 * kPage + 1, 1};
  for (size_t n = 1; n <= 4; n++) {
    size_t combos = 4;
    for (size_t i = 1; i < n; i++) combos *= 3;
    for (size_t c = 0; c < combos; c++) {
      std::vector<uint64_t> lens(n);
      size_t v = c;
      lens[n - 1] = kinds[v % 4];
      v /= 4;
      for (size_t k = 0; k + 1 < n; k++, v /= 3) lens[k] = kinds[v % 3];
      const int64_t last = (int64_t)n - 1;
      drive(lens, -1, -1, false);
      drive(lens, -1, -1, true);  // pinned by the caller: direct, and never unlocked
      for (int64_t f : {(int64_t)0, (int64_t)1, (int64_t)2, last}) {
        drive(lens, f, -1, false);
        drive(lens, -1, f, false);
      }
      serial(lens);
    }
  }
  none();
  printf("ok %llu\n", (unsigned long long)g_cases);
  return 0;
}
