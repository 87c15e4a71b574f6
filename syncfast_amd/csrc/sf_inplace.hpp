// sf_inplace.hpp -- the page-lock regions of the in-place routes
// (index_inplace and index_list_pipeline, sf_host.cpp).  A caller's pages are
// page-locked region by region, one region ahead of the copy that reads them;
// no copy spans two registrations and no page is registered twice.  Host
// arithmetic only (no HIP include): what locks and unlocks is handed in, so
// tests/native/inplace_regions.cpp executes the rule under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace sfi __attribute__((visibility("hidden"))) {

// What page-locking a range gave (lock_pages, sf_pagelock.cpp): locked by this
// call, which unlocks it; already page-locked by the caller, copied from as it
// is; or neither, and the bytes go through a pinned stage.
enum PageLock { kLockedByUs, kPinnedByCaller, kNotLocked };

// n stages that start at starts[0] < ... < starts[n-1] and end at `end`.
// Region k = [edge(k), edge(k+1)): edge(0) the page edge at or below the first
// start, edge(k) the page edge at or above start k, edge(n) the one at or
// above the end.  So stage k's bytes lie in region k-1 (its head, up to
// edge(k)) and region k, and the regions tile the pages of the range.  One
// start is one region over the whole range (the serial form); none, no region.
// lock(a, e) -> PageLock and unlock(a) are the registry's, or a test's.
template <typename Lock, typename Unlock>
class InplaceRegions {
 public:
  // fail_at: region fail_at "cannot be locked" (a test hook; < 0: none).
  InplaceRegions(uint64_t page, const std::vector<uintptr_t>& starts, uintptr_t end, Lock lock, Unlock unlock,
                 int64_t fail_at = -1)
      : lock_(lock), unlock_(unlock), fail_at_(fail_at), edge_(starts.size() + 1), state_(starts.size(), kUnsettled) {
    const uintptr_t mask = ~(uintptr_t)(page - 1);
    for (size_t k = 0; k < starts.size(); k++) edge_[k] = k ? (starts[k] + page - 1) & mask : starts[0] & mask;
    edge_[starts.size()] = (end + page - 1) & mask;
  }
  // Unlocks what it locked, once each.  Copies that read the pages must be
  // over by then: declare the tracker before the HostLease whose release
  // waits for the streams.
  ~InplaceRegions() {
    for (size_t k = 0; k < size(); k++)
      if (state_[k] == kLocked) unlock_(edge_[k]);
  }
  InplaceRegions(const InplaceRegions&) = delete;
  InplaceRegions& operator=(const InplaceRegions&) = delete;

  size_t size() const { return state_.size(); }
  uintptr_t edge(size_t k) const { return edge_[k]; }

  // Settles region k, once, after region k-1 (the callers run one region
  // ahead of the stage they issue); past the last region there is nothing to
  // do.  Failure is sticky: after a region that could not be locked every
  // later one is failed without asking, since a stage straddles the page it
  // shares with the region before.
  void lock_ahead(size_t k) {
    if (k >= size() || state_[k] != kUnsettled || (k && state_[k - 1] == kUnsettled)) return;
    if ((k && state_[k - 1] == kFailed) || (int64_t)k == fail_at_) {
      state_[k] = kFailed;
    } else if (edge_[k + 1] <= edge_[k]) {  // a short last stage inside the previous region's last page
      state_[k] = kEmpty;
    } else {
      const PageLock pl = lock_(edge_[k], edge_[k + 1]);
      state_[k] = pl == kLockedByUs ? kLocked : pl == kPinnedByCaller ? kPinned : kFailed;
    }
  }
  // Stage k may be copied from the caller's pages: the regions that hold its
  // bytes are settled and page-locked (or hold none of them).
  bool direct(size_t k) const { return usable(k) && (k == 0 || usable(k - 1)); }
  // The bytes of stage k = [src, src + n) that lie in region k-1: copied apart
  // from the rest, so that each copy lies inside ONE registration.
  uint64_t head(size_t k, uintptr_t src, uint64_t n) const {
    return k == 0 ? 0 : std::min<uint64_t>(n, edge_[k] - src);
  }

 private:
  enum State : uint8_t { kUnsettled, kLocked, kPinned, kEmpty, kFailed };
  bool usable(size_t k) const { return k < size() && state_[k] != kUnsettled && state_[k] != kFailed; }
  Lock lock_;
  Unlock unlock_;
  int64_t fail_at_;
  std::vector<uintptr_t> edge_;
  std::vector<State> state_;
};

}  // namespace sfi
