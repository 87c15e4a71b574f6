// sf_zpaq.cpp -- the reference's content-defined chunker on the host
// (include/syncfast_amd.h: sf_zpaq_cut_buffer, sf_zpaq_chunker_ops).
//
// cdchunking's ZPAQ as index_file uses it (src/index.rs:622-625: 13 bits, a
// 32 KiB cap), one byte at a time with the step of sf_zpaq_step.hpp.  This
// sequential loop is the library's DEFINITION of the boundaries: the device
// cutter (sf_cdc.hip) and the threaded host route (sf_cut_fd over the ops
// below) must return exactly its list.  It reproduces the reference's
// known-answer test (tests/golden/golden.json, reference_kat) and restarts
// with a fresh state after every cut.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/syncfast_amd.h"
#include "sf_zpaq_step.hpp"

namespace {

struct Zpaq {
  uint32_t lim, max_size;
  uint32_t h, c1, run;
  uint8_t o1[256];
  void fresh() {
    h = sfz::kFreshH;
    c1 = 0;
    run = 0;
    memset(o1, 0, sizeof o1);
  }
  // feeds one byte; true: the chunk ends after it (and the state is fresh)
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

inline bool params_ok(uint32_t bits, uint32_t max_size) { return bits >= 1 && bits <= 31 && max_size >= 1; }

// The parameters travel in sf_chunker_ops.ctx itself (bits in the low 8 bits,
// max_size above them: a pointer holds at least 40 bits on every target of
// this library), so the ops own no memory and need no release.
inline void* pack_ctx(uint32_t bits, uint32_t max_size) {
  return reinterpret_cast<void*>((uintptr_t)(((uint64_t)max_size << 8) | bits));
}

void* zpaq_create(void* ctx) {
  const uint64_t v = (uint64_t)(uintptr_t)ctx;
  const uint32_t bits = (uint32_t)(v & 0xFF), max_size = (uint32_t)(v >> 8);
  if (!params_ok(bits, max_size)) return nullptr;
  Zpaq* z = static_cast<Zpaq*>(malloc(sizeof(Zpaq)));
  if (!z) return nullptr;
  z->lim = sfz::limit(bits);
  z->max_size = max_size;
  z->fresh();
  return z;
}

size_t zpaq_next(void* chunker, const uint8_t* p, size_t n) {
  Zpaq* z = static_cast<Zpaq*>(chunker);
  for (size_t i = 0; i < n; i++)
    if (z->feed(p[i])) return i + 1;
  return 0;
}

void zpaq_destroy(void* chunker) { free(chunker); }

}  // namespace

extern "C" {

int sf_zpaq_cut_buffer(const uint8_t* data, uint64_t len, uint32_t bits, uint32_t max_size, uint64_t* offsets,
                       uint32_t* sizes, uint64_t cap, uint64_t* n_blocks) {
  if (n_blocks) *n_blocks = 0;
  if (!params_ok(bits, max_size) || !n_blocks || (len && !data)) return SF_EINVAL;
  Zpaq z;
  z.lim = sfz::limit(bits);
  z.max_size = max_size;
  z.fresh();
  uint64_t n = 0, start = 0;
  auto emit = [&](uint64_t end) {
    if (n < cap && offsets && sizes) {
      offsets[n] = start;
      sizes[n] = (uint32_t)(end - start);  // <= max_size
    }
    n++;
    start = end;
  };
  for (uint64_t i = 0; i < len; i++)
    if (z.feed(data[i])) emit(i + 1);
  if (start < len) emit(len);  // the last chunk ends with the data
  *n_blocks = n;
  return n > cap || (n && (!offsets || !sizes)) ? SF_ENOSPC : SF_OK;
}

int sf_zpaq_chunker_ops(uint32_t bits, uint32_t max_size, sf_chunker_ops* out) {
  if (!out || !params_ok(bits, max_size)) return SF_EINVAL;
  out->create = zpaq_create;
  out->next = zpaq_next;
  out->destroy = zpaq_destroy;
  out->ctx = pack_ctx(bits, max_size);
  return SF_OK;
}

}  // extern "C"
