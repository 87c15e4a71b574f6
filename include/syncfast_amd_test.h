/* syncfast_amd_test.h -- test hooks of libsyncfast_amd (not part of the
 * drop-in surface; no reference interface corresponds).
 *
 * The library reads its environment knobs once, when it is loaded
 * (syncfast_amd/csrc/sf_knobs.cpp); nothing on a launch or copy path reads
 * the environment.  A test that needs another value inside the same process
 * sets it here.  Names are the environment variables' (INTEGRATION.md,
 * "Environment knobs"): SF_* performance knobs and SF_TEST_* hooks.
 */
#ifndef SYNCFAST_AMD_TEST_H
#define SYNCFAST_AMD_TEST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Set knob `name` to `value`; the previous value goes to *old_value (may be
 * NULL).  SF_EINVAL for an unknown name.  Not synchronised with calls in
 * flight on other threads: set knobs between calls. */
int sf_test_set_knob(const char* name, int64_t value, int64_t* old_value);

/* Current value of knob `name`. */
int sf_test_get_knob(const char* name, int64_t* value);

/* Process-wide counters of the routes the host entry points took:
 *   "pages_locked"      caller ranges the library page-locked (hipHostRegister)
 *   "not_anon_refused"  caller ranges it did not page-lock because they are not
 *                       private anonymous memory (a file mapping, shared
 *                       memory): those are copied through the pinned stages. */
int sf_test_get_stat(const char* name, int64_t* value);

/* The processing order sha1_table_kernel gets for a sorted explicit list:
 * d_order[0, n) (device uint32) receives the block indices ordered by
 * length class (4 mantissa bits, 8-bit key), descending, list order within
 * a class -- the counting sort of sf_sort.hip.  d_sizes: n device uint32.
 * Asynchronous on `stream`; SF_EINVAL for n >= 2^32 or a d_order that is not
 * 4-B aligned. */
int sf_test_table_order(const uint32_t* d_sizes, uint64_t n, uint32_t* d_order, void* stream);

/* The same with `mbits` mantissa bits (1..6) of the length class: the key
 * is clamped at (16 << max(mbits, 4)) - 1 (8, 9 or 10 bits), as the
 * SF_TABLE_CLASS_BITS knob sorts.  SF_EINVAL for mbits outside 1..6. */
int sf_test_table_order_bits(const uint32_t* d_sizes, uint64_t n, uint32_t mbits, uint32_t* d_order, void* stream);

/* Called by the descriptor and path routes that pread a regular file
 * (sf_index_fd_blocks, sf_index_fd_fixed, sf_index_file_blocks,
 * sf_index_file) after each window has been read, on the calling thread,
 * with the window's index: a test changes the file at a known point of a
 * call.  NULL removes it.  Not synchronised with calls in flight. */
typedef void (*sf_test_read_hook_fn)(void* arg, uint64_t window);
int sf_test_set_read_hook(sf_test_read_hook_fn fn, void* arg);

/* The gather plan of sf_index_device_multi / _ex for n_devices shards of a
 * file_len-byte file at block_size, gathered to `root` (self_gather: the
 * one-device self send/recv of SF_TEST_MULTI_SELF_GATHER, n_devices == 1
 * only).  Per device r (n_devices entries each): table_offset[r] = where its
 * rows start in d_table (bytes), bytes[r] = its digest bytes, route[r] = 0
 * (empty shard: nothing hashed or sent), 1 (the root's rows, hashed in place
 * into d_table) or 2 (hashed into d_digests[r] and sent to the root, which
 * receives them at table_offset[r]).  Host only. */
int sf_test_multi_plan(uint64_t file_len, uint32_t block_size, uint32_t n_devices, uint32_t root, int self_gather,
                       uint64_t *table_offset, uint64_t *bytes, int *route);

/* Cross-XCD counter litmus (sf_litmus.hip): does a read of a counter see
 * adds made on other XCDs after the reading XCD's L2 holds its line?
 * mode 0 reads with a relaxed agent-scope atomic load (round 5's fused
 * launch polled that way), mode 1 with an agent-scope atomic add of an
 * opaque zero.  One launch on the current device,
 * synchronous.  out[8]: status (0 ok, 1 a hand-shake wait ran out), the
 * reader's XCD id, adds made from other XCDs, first read, read after every
 * add returned, a read-modify-write read after that, mode, 0.  A stale form
 * gives out[4] == out[3] < out[2] == out[5]. */
int sf_test_xcd_litmus(int mode, uint32_t out[8]);

/* What the device ZPAQ cutter (sf_cut_device_zpaq and the calls built on it)
 * did in its most recent cut in this process: out[0] the segment length in
 * bytes (lcm(max_size, 32)), out[1] the number of segments, out[2] the join
 * rounds in which a segment cut again, out[3] the bytes cut again in all of
 * them.  Host only; not synchronised with cuts in flight. */
int sf_test_zpaq_device_stats(uint64_t out[4]);

/* What the many-file device ZPAQ cutter (sf_cut_device_zpaq_files and the
 * calls built on it) did in its most recent call in this process: out[0] the
 * segment length in bytes, out[1] the segments of all files, out[2] the join
 * launches made (one more than the rounds in which a segment cut again when
 * the joins ended by themselves; max_rounds when the bound was reached; 0
 * when no file has two segments), out[3] the bytes cut again in all of them,
 * out[4] the unsettled files, out[5] the files finished on the host (0 for
 * the calls over HBM).  Host only; not synchronised with cuts in flight. */
int sf_test_zpaq_files_stats(uint64_t out[6]);

/* What the last FILE_BLOCK parse of this process did (sf_wire_parse_blocks_device
 * and the calls built on it): out[0] the candidate positions the device found
 * (0 when the parse was forced to the host), out[1] the messages, out[2] 1 if
 * the host fallback ran (a forged message start, or SF_TEST_WIRE_PARSE_HOST),
 * out[3] reserved (0).  Host only; not synchronised with calls in flight. */
int sf_test_wire_parse_stats(uint64_t out[4]);

/* What the last sf_receive_files_device of this process did: out[0] the
 * candidate positions the device found (0 when the parse was forced to the
 * host), out[1] the accepted messages of all three kinds, out[2] 1 if the
 * host fallback ran (a message start inside the last chained message, or
 * SF_TEST_WIRE_PARSE_HOST), out[3] reserved (0).  Host only; not synchronised
 * with calls in flight. */
int sf_test_recv_files_stats(uint64_t out[4]);

/* What the last sf_receive_file_entries_device of this process did: out[0] the
 * route (0 the chain on the device, 1 forced to the host by
 * SF_TEST_WIRE_PARSE_HOST, 2 the host fallback after an entry's start inside
 * the last chained entry), out[1] the candidate positions the device found (0
 * when forced to the host), out[2] the chained entries, out[3] the read-backs
 * (synchronisations of the call: 1 for a parse on the device, 2 with a set).
 * Host only; not synchronised with calls in flight. */
int sf_test_file_entries_stats(uint64_t out[4]);

/* What the last sf_serve_get_files_device of this process did: out[0] the route
 * (0 nothing launched: no bytes or an argument error; 1 parsed, and no request
 * answered: an empty run; 2 a run built), out[1] the requests parsed, out[2]
 * the requests answered, out[3] the read-backs (synchronisations of the call:
 * 3 for a run built, whatever the number of requests; 1 when no request was
 * parsed, 2 or 3 when none is answered).  Host only; not
 * synchronised with calls in flight. */
int sf_test_serve_files_stats(uint64_t out[4]);

/* What the last BLOCK_DATA parse of this process did (sf_receive_block_data_device
 * / _buffer): out[0] the candidate positions the device found, out[1] the
 * messages, out[2] 1 if the host walked the candidate list (a candidate inside
 * a chained message, or SF_TEST_BLOCK_DATA_WALK), out[3] the bytes of that list
 * copied back for it (16 per candidate; never payload bytes).  Host only; not
 * synchronised with calls in flight. */
int sf_test_block_data_stats(uint64_t out[4]);

/* What the last sf_copy_blocks_device of this process did: out[0] T, the tile
 * size in bytes (also without a call, and without a device), out[1] the jobs
 * it copied (taken and in range; empty ones count), out[2] their tiles,
 * out[3] the launches of the copy kernel (0: n_blocks == 0 or an argument
 * error).  out[1] and out[2] are counted on the device: the call's device is
 * synchronised to read them.  Not synchronised with calls in flight on other
 * threads. */
int sf_test_copy_stats(uint64_t out[4]);

/* What the last sf_plan_copies_device of this process did: out[0] the
 * read-backs (synchronisations of the call: 1 without verification or without
 * a candidate, 2 with both; 0 when nothing was launched), out[1] the
 * candidates hashed (0 without verification), out[2] the jobs, out[3] 1 for a
 * query.  Host only; not synchronised with calls in flight. */
int sf_test_plan_copies_stats(uint64_t out[4]);

#ifdef __cplusplus
}
#endif

#endif /* SYNCFAST_AMD_TEST_H */
