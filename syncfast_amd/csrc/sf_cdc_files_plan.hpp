// sf_cdc_files_plan.hpp -- the geometry of the many-file device ZPAQ cut
// (sf_cdc_files.hip, include/syncfast_amd.h: sf_cut_device_zpaq_files):
// how a batch of files is divided into segments and bitmap words, which file
// a segment belongs to, which bytes and words it owns, where its incoming cut
// comes from, when a file counts as unsettled under a round cap, and where a
// segment's and a file's rows start.
//
// Everything here is integer arithmetic over plain arrays.  No HIP and no
// library header (tests/native/cdc_files_plan.cpp executes the plan on a CPU,
// one loop iteration per lane), and every function is constexpr: the kernels
// call the same ones, so what the host test proves about the words stored and
// the rows written holds for the kernels'.
//
//   files     file f is bytes [off_f, off_f + len_f) of one buffer; no
//             alignment, and files may abut, leave gaps or overlap.
//   segments  segment k of file f is its file-relative bytes
//             [k L, min(len_f, k L + L)), L = lcm(max_size, 32).  Segments are
//             numbered globally in file order: file f's are
//             [seg_first[f], seg_first[f + 1]).  An empty file has none.
//   words     the cut bitmaps are per file, from a word-aligned base:
//             word_first[f] = sum over g < f of ceil(len_g / 32); bit i of
//             file f's part = a chunk of f ends after its byte i.  As L is a
//             multiple of 32 a segment owns whole words, [k L / 32,
//             ceil(s1 / 32)) of its file's part, whatever the file's position
//             in the buffer.
//   join      a file's segment 0 is true from round 0; segment k > 0 takes its
//             incoming cut from global segment s - 1, which is segment k - 1 of
//             the same file.
//   rounds    the join kernel of launch r (1, 2, ...) stores r at round[f] for
//             every segment of f that cuts again.  A segment can only cut
//             again in launch r + 1 if its predecessor did in launch r, so a
//             file that was quiet in the last launch made is final; one that
//             was not is unsettled, and emits no rows.
//   rows      an inclusive scan of the segments' counts (an unsettled file's
//             forced to 0) gives ends[]; segment s writes rows
//             [ends[s - 1], ends[s]) and file f starts at the row of its
//             first segment.
#pragma once
#include <stdint.h>

namespace sfzf {

constexpr uint64_t seg_count(uint64_t len, uint64_t L) { return len / L + (len % L != 0); }
constexpr uint64_t word_count(uint64_t len) { return (len >> 5) + ((len & 31) != 0); }

// [off, off + len) lies in [0, data_len]: also when off + len passes 2^64.
constexpr bool in_range(uint64_t off, uint64_t len, uint64_t data_len) { return off <= data_len && len <= data_len - off; }

// seg_first[0 .. n] and word_first[0 .. n] of the files' lengths.
constexpr void fill_firsts(const uint64_t* lens, uint32_t n, uint64_t L, uint64_t* seg_first, uint64_t* word_first) {
  uint64_t s = 0, w = 0;
  for (uint32_t f = 0; f < n; f++) {
    seg_first[f] = s;
    word_first[f] = w;
    s += seg_count(lens[f], L);
    w += word_count(lens[f]);
  }
  seg_first[n] = s;
  word_first[n] = w;
}

// The file of global segment s < seg_first[n]: the f with
// seg_first[f] <= s < seg_first[f + 1] (never an empty file).  A search, at
// most 32 steps.
constexpr uint32_t file_of(const uint64_t* seg_first, uint32_t n, uint64_t s) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (seg_first[mid] <= s) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Global segment s as a part of its file: file-relative bytes [s0, s1), and
// the words [w0, wend] of the file's part of the bitmaps that it owns.
struct Seg {
  uint32_t file;
  uint64_t k, s0, s1, w0, wend;
  constexpr bool first() const { return k == 0; }                   // true from round 0; no incoming cut
  constexpr bool last(uint64_t len) const { return s1 == len; }     // the file's last block ends at s1
};
constexpr Seg segment(uint32_t file, uint64_t first_seg, uint64_t len, uint64_t L, uint64_t s) {
  const uint64_t k = s - first_seg, s0 = k * L, s1 = s0 + L < len ? s0 + L : len;
  return Seg{file, k, s0, s1, s0 >> 5, (s1 - 1) >> 5};
}

// The global segment whose last cut is segment s's incoming cut (s not a
// file's first): segment k - 1 of the same file.
constexpr uint64_t incoming_from(uint64_t s) { return s - 1; }

// A synced join adopts the round-0 bits of its word above bit i.
constexpr uint32_t above_bit(uint64_t i) { return (i & 31) == 31 ? 0u : ~0u << ((i & 31) + 1); }

// After `launches` join launches: a file whose last store was `round`.
constexpr bool unsettled(uint32_t round, uint32_t launches) { return launches != 0 && round == launches; }

// First row of global segment s (s may be the segment count: the total).
constexpr uint64_t row_base(const uint64_t* ends, uint64_t s) { return s ? ends[s - 1] : 0; }
// First row of file f (f may be n: the total).
constexpr uint64_t first_row(const uint64_t* seg_first, const uint64_t* ends, uint32_t f) {
  return row_base(ends, seg_first[f]);
}

}  // namespace sfzf
