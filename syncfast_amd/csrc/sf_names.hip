// sf_names.hip -- the destination's lookup of files by name on the device
// (include/syncfast_amd.h, sf_name_set_*), the sibling of sf_match.hip's
// lookup of blocks by digest.
//
// For every FILE_ENTRY of an incoming files list the sink asks its index for
// the file of that name (Index::get_file, src/index.rs of the reference, called
// at src/sync/fs.rs:385):
//   SELECT file_id, ... FROM files WHERE name = ?;
// and takes the first row.  SQLite answers from idx_files_name, in (name,
// rowid) order, and the schema has no UNIQUE on name: "first" is the row with
// that name and the smallest rowid.  Here the destination's names (packed
// bytes and a CSR, in file_id order, with an optional present flag per row)
// become an open-addressing table in HBM, built once, and a whole list is
// answered in one launch: the lowest present row of that name, or -1.
//
// Table: capacity = a power of two >= 2 x rows (load <= 1/2), 8 B per slot:
// bits 0-31 = row + 1 (0 = empty; rows <= 2^31), bits 32-63 = the high half of
// the name's hash (sf_wire_entries.hpp: name_hash), so a probe rejects most
// slots of another name without reading a byte of it.  The slot index comes
// from the hash's low bits.
//
//   build   one lane per row: its CSR entries are tested (the first bad row is
//           an atomicMin), and a present row whose entries hold is inserted
//           with one atomicCAS per probe into the first empty slot of its probe
//           sequence.  Keys are never compared: a name that stands in three
//           rows takes three slots, in whatever order the lanes arrive.
//   lookup  one lane per query: it walks its probe sequence to the first empty
//           slot and keeps the smallest row whose fingerprint, length and
//           bytes are the query's.  Every row of a name lies in that name's
//           probe sequence before its first empty slot (nothing is ever
//           removed), so the minimum does not depend on the insertion order,
//           and no lane waits for another.
//
// Linear probing; every loop is bounded by the capacity and the table is never
// full, so every wave exits.  Names and query spans are read as bytes: no
// alignment.  Random-access, latency-bound integer work: no MFMA, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_device.hpp"
#include "sf_wire_entries.hpp"

namespace sfn {

constexpr uint64_t kRowMask = 0xFFFFFFFFull;
constexpr uint64_t kMaxRows = 1ull << 31;

__device__ __forceinline__ unsigned long long tag_of(uint64_t h) { return h & ~kRowMask; }

// Rows [0, n): bad (starts at UINT64_MAX) = the first row whose entries do not
// hold: at[0] == 0, at[r] <= at[r + 1] <= at[n].  A row whose entries hold
// reads only names[at[r], at[r + 1]), which lies inside names[0, at[n]).
__global__ void __launch_bounds__(256)
name_set_insert_kernel(const uint8_t* __restrict__ names, const uint64_t* __restrict__ at,
                       const uint8_t* __restrict__ present, uint64_t n, uint64_t hash_mask,
                       unsigned long long* slots, uint64_t mask, unsigned long long* __restrict__ bad) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = r < n;
  uint64_t a0 = 0, a1 = 0;
  bool ok = true;
  if (in) {
    a0 = at[r];
    a1 = at[r + 1];
    ok = a0 <= a1 && a1 <= at[n] && (r != 0 || a0 == 0);
  }
  const unsigned long long m = __ballot(in && !ok);
  if (m && (threadIdx.x & 63u) == (uint32_t)__ffsll(m) - 1) atomicMin(bad, (unsigned long long)r);
  if (!in || !ok || (present && !present[r])) return;
  const uint64_t h = sfwp::name_hash(names + a0, a1 - a0, hash_mask);
  const unsigned long long mine = tag_of(h) | (r + 1);
  uint64_t i = h & mask;
  for (uint64_t probes = 0; probes <= mask; ++probes, i = (i + 1) & mask) {
    if (slots[i] != 0) continue;
    if (atomicCAS(&slots[i], 0ull, mine) == 0) return;  // claimed an empty slot
  }
}

// Queries [0, nq): span (q_at[q], q_len[q]) of bytes[0, n_bytes).  A span that
// leaves the buffer matches nothing and is not read.
__global__ void __launch_bounds__(256)
name_set_lookup_kernel(const uint8_t* __restrict__ names, const uint64_t* __restrict__ at,
                       const unsigned long long* __restrict__ slots, uint64_t mask, uint64_t hash_mask,
                       const uint8_t* __restrict__ bytes, uint64_t n_bytes, const uint64_t* __restrict__ q_at,
                       const uint32_t* __restrict__ q_len, uint64_t nq, int64_t* __restrict__ rows) {
  const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const uint64_t a = q_at[q], len = q_len[q];
  int64_t found = -1;
  if (a <= n_bytes && len <= n_bytes - a) {
    const uint8_t* key = bytes + a;
    const uint64_t h = sfwp::name_hash(key, len, hash_mask);
    const unsigned long long tag = tag_of(h);
    uint64_t i = h & mask;
    for (uint64_t probes = 0; probes <= mask; ++probes, i = (i + 1) & mask) {
      const unsigned long long cur = slots[i];
      if (cur == 0) break;
      const int64_t row = (int64_t)(cur & kRowMask) - 1;
      if ((cur & ~kRowMask) != tag || (found >= 0 && row > found)) continue;
      const uint64_t r0 = at[row];
      if (at[row + 1] - r0 != len) continue;
      bool same = true;
      for (uint64_t k = 0; k < len && same; k++) same = names[r0 + k] == key[k];
      if (same) found = row;
    }
  }
  rows[q] = found;
}

}  // namespace sfn

using namespace sfi;

// The opaque handle of include/syncfast_amd.h.
struct sf_name_set {
  const uint8_t* names;  // the caller's packed names and CSR (kept alive by the caller)
  const uint64_t* at;
  uint64_t rows;
  unsigned long long* slots;  // device, 8 B per slot
  uint64_t mask;              // capacity - 1
  uint64_t hash_mask;         // SF_TEST_NAME_HASH_MASK when the set was built
};

namespace {

int name_set_build(const void* d_names, const uint64_t* d_name_at, const uint8_t* d_present, uint64_t n_rows,
                   sf_name_set** out, uint64_t* bad_row, hipStream_t s) {
  if (out) *out = nullptr;
  if (bad_row) *bad_row = UINT64_MAX;
  if (!out || !bad_row || n_rows > sfn::kMaxRows || (n_rows && !d_name_at) || misaligned(d_name_at, 8))
    return SF_EINVAL;
  const uint64_t hash_mask = (uint64_t)knob(K_TEST_NAME_HASH_MASK);
  if (n_rows == 0) {  // no row: every lookup answers -1, nothing on the device
    *out = new sf_name_set{nullptr, nullptr, 0, nullptr, 0, hash_mask};
    return SF_OK;
  }
  uint64_t cap = 1024;
  while (cap < 2 * n_rows) cap <<= 1;
  ScratchLayout L;
  const size_t slots_at = L.add(cap * 8), bad_at = L.add(8);
  Scratch ws(s);
  int rc = stream_alloc(&ws.p, L.total(), s);
  if (rc != SF_OK) return rc;
  unsigned long long* slots = L.at<unsigned long long>(ws.p, slots_at);
  unsigned long long* d_bad = L.at<unsigned long long>(ws.p, bad_at);
  SF_HIP(hipMemsetAsync(slots, 0, cap * 8, s));
  SF_HIP(hipMemsetAsync(d_bad, 0xFF, 8, s));
  rc = launch(sfn::name_set_insert_kernel, grid256(n_rows), dim3(256), s, static_cast<const uint8_t*>(d_names),
              d_name_at, d_present, n_rows, hash_mask, slots, cap - 1, d_bad);
  if (rc != SF_OK) return rc;
  uint64_t bad = 0;
  SF_HIP(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  if (bad != UINT64_MAX) {
    *bad_row = bad;
    return SF_EINVAL;  // ws goes back: nothing is kept
  }
  *out = new sf_name_set{static_cast<const uint8_t*>(d_names), d_name_at, n_rows, slots, cap - 1, hash_mask};
  ws.p = nullptr;  // the set owns the allocation now (slots is its first part)
  return SF_OK;
}

}  // namespace

extern "C" {

int sf_name_set_build(const void* d_names, const uint64_t* d_name_at, const uint8_t* d_present, uint64_t n_rows,
                      sf_name_set** out, uint64_t* bad_row, void* stream) {
  return guarded([&] { return name_set_build(d_names, d_name_at, d_present, n_rows, out, bad_row, as_stream(stream)); });
}

int sf_name_set_lookup(const sf_name_set* set, const void* d_bytes, uint64_t n_bytes, const uint64_t* d_at,
                       const uint32_t* d_len, uint64_t n_query, int64_t* d_rows, void* stream) {
  if (!set || (n_query && (!d_at || !d_len || !d_rows)) || (n_bytes && !d_bytes)) return SF_EINVAL;
  if (misaligned(d_at, 8) || misaligned(d_len, 4) || misaligned(d_rows, 8)) return SF_EINVAL;
  if (n_query == 0) return SF_OK;
  hipStream_t s = as_stream(stream);
  if (set->rows == 0) return hip_err(hipMemsetAsync(d_rows, 0xFF, n_query * 8, s));  // -1 everywhere
  const uint64_t per = 1ull << 31;  // queries per launch (< 2^32 work-items)
  return for_pieces(n_query, per, [&](uint64_t q0, uint64_t nq) {
    return launch(sfn::name_set_lookup_kernel, grid256(nq), dim3(256), s, set->names, set->at, set->slots, set->mask,
                  set->hash_mask, static_cast<const uint8_t*>(d_bytes), n_bytes, d_at + q0, d_len + q0, nq,
                  d_rows + q0);
  });
}

int sf_name_set_free(sf_name_set* set, void* stream) {
  if (!set) return SF_OK;
  const int rc = set->slots ? hip_err(hipFreeAsync(set->slots, as_stream(stream))) : SF_OK;  // stream_free, with its error
  delete set;
  return rc;
}

}  // extern "C"
