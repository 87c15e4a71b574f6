// sf_pagelock.cpp -- the process-wide registry of the host ranges this library
// page-locked for its in-place routes (sf_host.cpp asks it through
// InplaceRegions, sf_inplace.hpp), and the rule of what may be page-locked at
// all.  HIP runtime API only: built with the host compiler.
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <sys/ioctl.h>
#include <unistd.h>

#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "sf_internal.hpp"

namespace sfi {

namespace {

// Host ranges page-locked by this library's in-place routes, process-wide.
// hipHostRegister refuses a range that overlaps a registered one
// (AlreadyRegistered).  If that registration is one of ours, the concurrent
// call that made it will unregister it while our copies may still read it,
// so such a range is bounced through pinned stages instead; a registration
// the caller made stays for the length of the call and is copied from.
std::mutex g_lock_mu;
std::vector<std::pair<uintptr_t, uintptr_t>> g_locked;

bool locked_by_us(uintptr_t a, uintptr_t e) {  // caller holds g_lock_mu
  for (const auto& r : g_locked)
    if (r.first < e && a < r.second) return true;
  return false;
}

// PROCMAP_QUERY (Linux 6.11+, include/uapi/linux/fs.h): one ioctl on
// /proc/self/maps answers "the first VMA at or after addr with these
// properties".  Declared here: the image's kernel headers predate it.
struct ProcmapQuery {
  uint64_t size, query_flags, query_addr;
  uint64_t vma_start, vma_end, vma_flags, vma_page_size, vma_offset, inode;
  uint32_t dev_major, dev_minor, vma_name_size, build_id_size;
  uint64_t vma_name_addr, build_id_addr;
};
constexpr uint64_t kQueryCoveringOrNext = 0x10, kQueryFileBacked = 0x20;
constexpr unsigned long kProcmapQuery = _IOWR('f', 17, ProcmapQuery);

// Is [a, e) private anonymous memory only (heap, anonymous mmap, stack)?
// The in-place routes page-lock the caller's pages (hipHostRegister makes
// them a GPU userptr).  For a file mapping -- and shared memory, which has a
// file behind it too -- a concurrent truncation invalidates that userptr under
// the copies in flight, and on MI355X the process's queues then never resumed
// (tests/test_gpu_robustness.py).  Such ranges are never
// page-locked: they go through the pinned stages.  The ioctl where the kernel
// has it, else /proc/self/maps parsed.
bool private_anonymous(uintptr_t a, uintptr_t e) {
  const Fd maps{open("/proc/self/maps", O_RDONLY | O_CLOEXEC)};
  const int fd = maps.fd;
  if (fd < 0) return false;
  ProcmapQuery q{};
  q.size = sizeof(q);
  q.query_flags = kQueryCoveringOrNext | kQueryFileBacked;
  q.query_addr = a;
  // the first file-backed VMA at or after a starts past the range, or there is none
  if (ioctl(fd, kProcmapQuery, &q) == 0) return q.vma_start >= e;
  if (errno == ENOENT) return true;
  // Older kernel: scan the text.  A VMA overlapping [a, e) must be anonymous
  // (inode 0, device 00:00) and private ('p').
  std::string txt;
  char buf[1 << 16];
  for (ssize_t r; (r = read(fd, buf, sizeof(buf))) != 0;) {
    if (r < 0 && errno == EINTR) continue;
    if (r < 0) return false;
    txt.append(buf, (size_t)r);
  }
  bool covered = true;
  for (size_t pos = 0; pos < txt.size();) {
    size_t nl = txt.find('\n', pos);
    if (nl == std::string::npos) nl = txt.size();
    unsigned long lo = 0, hi = 0, off = 0, ino = 0;
    unsigned maj = 0, mnr = 0;
    char perms[8] = {0};
    if (sscanf(txt.c_str() + pos, "%lx-%lx %7s %lx %x:%x %lu", &lo, &hi, perms, &off, &maj, &mnr, &ino) == 7 &&
        lo < e && a < hi && (ino != 0 || maj != 0 || mnr != 0 || perms[3] != 'p'))
      covered = false;
    pos = nl + 1;
  }
  return covered;
}

}  // namespace

// Memory the caller page-locked itself (hipHostMalloc, hipHostRegister):
// copied from as it is.
bool pinned_by_hip(uintptr_t a, uintptr_t e) {
  for (uintptr_t p : {a, e - 1}) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, (const void*)p) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    if (at.type != hipMemoryTypeHost) return false;
  }
  return true;
}

PageLock lock_pages(uintptr_t a, uintptr_t e) {
  std::lock_guard<std::mutex> lk(g_lock_mu);
  if (locked_by_us(a, e)) return kNotLocked;
  if (!private_anonymous(a, e)) {
    if (pinned_by_hip(a, e)) return kPinnedByCaller;
    stat_add(S_NOT_ANON_REFUSED);
    return kNotLocked;
  }
  const hipError_t err = hipHostRegister((void*)a, e - a, hipHostRegisterReadOnly);
  if (err == hipSuccess) {
    g_locked.push_back({a, e});
    stat_add(S_PAGES_LOCKED);
    return kLockedByUs;
  }
  (void)hipGetLastError();
  return err == hipErrorHostMemoryAlreadyRegistered ? kPinnedByCaller : kNotLocked;
}

void unlock_pages(uintptr_t a) {
  std::lock_guard<std::mutex> lk(g_lock_mu);
  (void)hipHostUnregister((void*)a);
  for (size_t i = 0; i < g_locked.size(); i++)
    if (g_locked[i].first == a) {
      g_locked.erase(g_locked.begin() + (long)i);
      break;
    }
}

bool range_locked_by_us(uintptr_t a, uintptr_t e) {
  std::lock_guard<std::mutex> lk(g_lock_mu);
  return locked_by_us(a, e);
}

}  // namespace sfi
