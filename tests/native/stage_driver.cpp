// stage_driver.cpp -- the host pipelines' stage driver and file reader
// (syncfast_amd/csrc/sf_stage.hpp) alone, as a stand-alone program: no HIP, no
// other part of the library.  tests/test_stage_driver.py builds it with
// ASan + UBSan and runs it; it prints "ok" and exits 0, or names what failed.
#include "../../syncfast_amd/csrc/sf_stage.hpp"

#include <stdio.h>
#include <string.h>

#include <functional>
#include <thread>
#include <vector>

using namespace sfi;

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                        \
  do {                                          \
    if (!(cond)) {                              \
      g_failed++;                               \
      fprintf(stderr, "FAILED %s: ", #cond);    \
      fprintf(stderr, __VA_ARGS__);             \
      fprintf(stderr, "\n");                    \
    }                                           \
  } while (0)

struct Call {
  char kind;  // 'i' or 'h'
  uint64_t k;
  int b;
};

// Runs two_stage(n, ...) with recording callables.  issue(k) answers
// issue_rc at k == issue_at, harvest(k) answers harvest_rc at k == harvest_at
// (at = UINT64_MAX: never).  Checks on every call what holds for every run:
// b = k & 1, stages issued and harvested in increasing k, each once,
// harvest(k-2) before issue(k), a buffer set never issued while its previous
// stage is unharvested, nothing harvested that was not issued.
struct Run {
  std::vector<Call> calls;
  uint64_t issued = 0, harvested = 0;
  int rc = 0;
  Run(uint64_t n, uint64_t issue_at, int issue_rc, uint64_t harvest_at, int harvest_rc) {
    bool busy[2] = {false, false};
    bool over = false;  // a callable has answered something other than SF_OK
    rc = two_stage(
        n,
        [&](uint64_t k, int b) {
          CHECK(!over, "issue(%llu) after a result that ends the run", (unsigned long long)k);
          CHECK(b == (int)(k & 1) && k == issued && k < n, "issue(%llu, %d), %llu issued", (unsigned long long)k, b,
                (unsigned long long)issued);
          CHECK(k < 2 || harvested >= k - 1, "issue(%llu) before harvest(%llu)", (unsigned long long)k,
                (unsigned long long)(k - 2));
          CHECK(!busy[b], "set %d issued while its previous stage is unharvested", b);
          calls.push_back({'i', k, b});
          if (k == issue_at) {
            over = issue_rc != kNoMoreStages;
            return issue_rc;
          }
          busy[b] = true;
          issued++;
          return SF_OK;
        },
        [&](uint64_t k, int b) {
          CHECK(!over, "harvest(%llu) after a result that ends the run", (unsigned long long)k);
          CHECK(b == (int)(k & 1) && k == harvested && k < issued, "harvest(%llu, %d), %llu harvested, %llu issued",
                (unsigned long long)k, b, (unsigned long long)harvested, (unsigned long long)issued);
          calls.push_back({'h', k, b});
          busy[b] = false;
          harvested++;
          if (k == harvest_at) {
            over = true;
            return harvest_rc;
          }
          return SF_OK;
        });
  }
};

constexpr uint64_t kNever = UINT64_MAX;

void test_driver() {
  for (uint64_t n = 0; n <= 5; n++) {  // every stage issued, then harvested, once and in order
    Run r(n, kNever, 0, kNever, 0);
    CHECK(r.rc == SF_OK && r.issued == n && r.harvested == n && r.calls.size() == 2 * n,
          "n=%llu: rc %d, %llu issued, %llu harvested", (unsigned long long)n, r.rc, (unsigned long long)r.issued,
          (unsigned long long)r.harvested);
  }
  const int codes[] = {SF_EIO, SF_ENODEV, SF_ENOMEM};
  for (uint64_t n = 1; n <= 4; n++)
    for (uint64_t k = 0; k < n; k++)
      for (int code : codes) {
        {  // an error from issue(k): the last call, and the result
          Run r(n, k, code, kNever, 0);
          CHECK(r.rc == code && r.calls.back().kind == 'i' && r.calls.back().k == k && r.issued == k,
                "n=%llu issue(%llu) -> %d: rc %d", (unsigned long long)n, (unsigned long long)k, code, r.rc);
          // what was harvested before it: the stages whose buffer sets were needed, no more
          CHECK(r.harvested == (k >= 2 ? k - 1 : 0), "n=%llu issue(%llu) fails: %llu harvested", (unsigned long long)n,
                (unsigned long long)k, (unsigned long long)r.harvested);
        }
        {  // an error from harvest(k): the last call, and the result
          Run r(n, kNever, 0, k, code);
          CHECK(r.rc == code && r.calls.back().kind == 'h' && r.calls.back().k == k && r.harvested == k + 1,
                "n=%llu harvest(%llu) -> %d: rc %d", (unsigned long long)n, (unsigned long long)k, code, r.rc);
        }
      }
  for (uint64_t k = 0; k <= 3; k++) {  // input that ends before stage k: stages [0, k) all harvested
    Run r(UINT64_MAX, k, kNoMoreStages, kNever, 0);
    CHECK(r.rc == SF_OK && r.issued == k && r.harvested == k && r.calls.size() == 2 * k + 1,
          "no stage %llu: rc %d, %llu issued, %llu harvested", (unsigned long long)k, r.rc,
          (unsigned long long)r.issued, (unsigned long long)r.harvested);
  }
}

// the library's workers, for this program: plain threads
void run_threads(unsigned n, const std::function<void()>& worker) {
  std::vector<std::thread> t;
  for (unsigned i = 1; i < n; i++) t.emplace_back(worker);
  worker();
  for (auto& x : t) x.join();
}

bool same(const uint8_t* a, const uint8_t* b, uint64_t n) { return n == 0 || memcmp(a, b, n) == 0; }

void test_readers() {
  const uint64_t sizes[] = {0, 1, (4ull << 20) - 1, (4ull << 20) + 1};
  for (uint64_t n : sizes) {
    char path[] = "/tmp/sf_stage_XXXXXX";
    const int fd = mkstemp(path);
    CHECK(fd >= 0, "mkstemp");
    if (fd < 0) return;
    unlink(path);
    std::vector<uint8_t> want(n), got(n + 1);
    for (uint64_t i = 0; i < n; i++) want[i] = (uint8_t)((i * 2654435761u) >> 13);
    for (uint64_t done = 0; done < n;) {
      const ssize_t w = pwrite(fd, want.data() + done, n - done, (off_t)done);
      CHECK(w > 0, "pwrite");
      if (w <= 0) return;
      done += (uint64_t)w;
    }
    CHECK(read_fully(fd, got.data(), 0, n) && same(got.data(), want.data(), n), "read_fully, %llu bytes",
          (unsigned long long)n);
    CHECK(!read_fully(fd, got.data(), 0, n + 1), "read_fully past EOF of %llu bytes", (unsigned long long)n);
    if (n > 1) {
      CHECK(read_fully(fd, got.data(), 1, n - 1) && same(got.data(), want.data() + 1, n - 1),
            "read_fully from byte 1 of %llu", (unsigned long long)n);
      CHECK(!read_fully(fd, got.data(), 1, n), "read_fully from byte 1 past EOF of %llu", (unsigned long long)n);
    }
    for (unsigned threads : {1u, 3u}) {
      memset(got.data(), 0, got.size());
      CHECK(read_slices(fd, got.data(), 0, n, threads, run_threads) == SF_OK &&
                same(got.data(), want.data(), n),
            "read_slices, %llu bytes, %u threads", (unsigned long long)n, threads);
      CHECK(read_slices(fd, got.data(), 0, n + 1, threads, run_threads) == SF_EIO,
            "read_slices past EOF of %llu bytes, %u threads", (unsigned long long)n, threads);
    }
    // the slices: at least 4 MiB each but the last, disjoint, all of [0, n)
    uint64_t end = 0, count = 0;
    const int rc = for_slices(n, 3, [](unsigned, auto& worker) { worker(); }, [&](uint64_t a, uint64_t e) {
      CHECK(a == end && e > a && e <= n && (e - a >= kMinSlice || e == n), "slice [%llu, %llu) of %llu",
            (unsigned long long)a, (unsigned long long)e, (unsigned long long)n);
      end = e;
      count++;
      return SF_OK;
    });
    CHECK(rc == SF_OK && end == n && count <= 3, "slices of %llu end at %llu", (unsigned long long)n,
          (unsigned long long)end);
    // the first failure stops the rest and is returned
    count = 0;
    CHECK(for_slices(3 * kMinSlice, 3, [](unsigned, auto& worker) { worker(); }, [&](uint64_t, uint64_t) {
            count++;
            return SF_EIO;
          }) == SF_EIO && count == 1, "a failing slice: %llu slices ran", (unsigned long long)count);
    close(fd);
  }
}

}  // namespace

int main() {
  test_driver();
  test_readers();
  if (g_failed) return 1;
  printf("ok\n");
  return 0;
}
