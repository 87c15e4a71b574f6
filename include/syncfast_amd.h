/*
 * syncfast_amd.h -- C-ABI of the MI355X block-signature indexing path.
 *
 * Drop-in boundary for the hot path of syncfast's Index::index_file
 * (/root/reference/src/index.rs:610-659): file bytes -> one
 * (offset, size, SHA-1) row per block, plus the per-file blocks_hash
 * (src/index.rs:661-682).  The reference exposes no FFI of its own; the seam
 * it replaces is the loop at src/index.rs:621-647 that hands
 * (HashDigest, offset, size) tuples to Index::add_block (src/index.rs:387-408).
 * INTEGRATION.md shows the Rust `extern "C"` binding a maintainer would add.
 *
 * Conventions
 *  - Plain pointers and sizes only.  "d_" pointers are device (HBM) pointers
 *    on the current HIP device; `stream` is a hipStream_t passed as void*
 *    (NULL = the null stream).  Device entry points are asynchronous on
 *    `stream` and may be called from several host threads on different
 *    streams.
 *  - Return 0 on success, a negative errno-style SF_E* code otherwise; the
 *    Rust side maps them to Error::Io (src/lib.rs:25), as the reference
 *    propagates I/O errors with `?` (src/index.rs:615,630) and exposes no
 *    partial results.
 *  - Digests are the 20 bytes of sha1.digest().bytes() (big-endian SHA-1),
 *    exactly HashDigest's field (src/lib.rs:72-76), stored back to back:
 *    block i at byte 20*i.
 *  - Output alignment.  A device output must be aligned to the widest store
 *    a kernel makes to it; each entry point names it, and a pointer that is
 *    not (NULL is) gives SF_EINVAL before anything is launched:
 *      4 B  digest tables and blocks_hash tables (d_digests, d_file_hashes:
 *           five 32-bit stores per row, and a 20-B row pitch keeps every row
 *           4-B aligned), uint32 / int32 arrays and a written d_status;
 *      8 B  uint64 / int64 arrays (d_offsets, d_data_offsets, d_rows);
 *      1 B  wire bytes (d_out), d_ok, and the destination of a block copy.
 *    Inputs need no alignment beyond their element type's unless stated.
 *  - Written extent.  A call writes the rows of its outputs it reports (or
 *    the first cap of them, where stated) and no other byte of the caller's
 *    memory: not the rows past them, not a byte before or after an output,
 *    and never an input.
 *  - Fixed tiling: block i = bytes [i*B, min((i+1)*B, len)).  No empty
 *    blocks: len == 0 gives 0 blocks, and there is no trailing empty block
 *    when len % B == 0 (the reference only emits a block on ChunkInput::End
 *    after data, src/index.rs:629-646).
 *  - blocks_hash of a file with no blocks is SHA1("") =
 *    da39a3ee5e6b4b0d3255bfef95601890afd80709.
 */
#ifndef SYNCFAST_AMD_H
#define SYNCFAST_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SF_HASH_DIGEST_LEN 20 /* HASH_DIGEST_LEN, src/lib.rs:72 */
#define SF_MAX_BLOCK_SIZE (32u << 20) /* fixed-tiling block size limit (32 MiB) */

#define SF_OK 0
#define SF_EIO (-5)      /* file read failed */
#define SF_EAGAIN (-11)  /* the file changed under the call (fd routes): cut it again and retry */
#define SF_ENOMEM (-12)  /* device, pinned or host allocation failed, or the system refused a thread */
#define SF_ENODEV (-19)  /* no HIP device, or a HIP runtime error */
#define SF_EINVAL (-22)  /* bad argument */
#define SF_ENOSPC (-28)  /* output capacity too small; *n_out holds the need */
#define SF_ERANGE (-34)  /* a block lies outside [0, len) */
#define SF_ETIMEDOUT (-110) /* kept for callers: no call returns it since round 6 (no kernel waits) */

/* One signature row: what index_file passes to add_block
 * (src/index.rs:636-642) and what FILE_BLOCK carries on the wire
 * (src/sync/ssh/proto.rs:162-166).  32 bytes. */
typedef struct sf_block_sig {
    uint64_t offset;
    uint32_t size;
    uint8_t sha1[SF_HASH_DIGEST_LEN];
} sf_block_sig;

/* A file inside one device buffer (many-file batch, BASELINE config 3). */
typedef struct sf_file_desc {
    uint64_t offset; /* byte offset of the file in the batch buffer */
    uint64_t len;    /* file length in bytes */
} sf_file_desc;

/* ------------------------------------------------------------ runtime */
const char *sf_version(void);
const char *sf_strerror(int code);
/* Number of visible HIP devices (0 on a machine without one). */
int sf_device_count(int *n);
int sf_set_device(int device);
/* The host-memory entry points (sf_index_buffer, sf_index_file) keep their
 * per-device streams, stage buffers and digest tables between calls (setting
 * them up costs ~8 ms per call).  This frees them; the next call sets them up
 * again.  Blocks while another thread is inside such a call. */
int sf_release_host_cache(void);

/* --------------------------------------- device-resident hot path ---- */

/* Scratch: calls that need device workspace on `stream` (an explicit list's
 * length sort, a batch's chain states, wire offsets, block-set slots) take it
 * stream-ordered from a memory pool of the library's own per device, which
 * keeps every freed block for later calls (it holds its peak use: at most
 * ~1 GiB, for a sort of 2^27 blocks) and reuses a block only on the stream
 * that freed it.  The device's default pool is not used: its blocks, given
 * back at every synchronisation and mapped again, made calls read wrong data
 * (DESIGN.md 3.4).  The caller's own allocations are not touched. */

/* Fixed tiling of d_data[0, len) into block_size-byte blocks; writes
 * ceil(len/block_size) digests to d_digests (20 B each).  Replaces the
 * chunk loop of src/index.rs:621-647 for fixed-size blocks.
 * SF_ENOSPC (with *n_blocks set, nothing written) when cap_blocks is too
 * small.  d_digests: 4-B aligned (each digest is five 32-bit stores). */
int sf_index_device_fixed(const void *d_data, uint64_t len, uint32_t block_size,
                          void *d_digests, uint64_t cap_blocks, uint64_t *n_blocks,
                          void *stream);

/* Explicit block list: block i = d_data[d_offsets[i], d_offsets[i] + d_sizes[i]).
 * Used for content-defined boundaries (src/index.rs:622-625 produces them
 * in the reference), the reference KAT boundaries and ragged batches.
 * Blocks need not be sorted, aligned or disjoint.  A block outside
 * [0, len) is not read: its digest is zeroed and, if d_status != NULL,
 * *d_status (device int32, caller-initialised to 0) is set to SF_ERANGE.
 * d_digests: 4-B aligned (digests and the zeroing are 32-bit stores);
 * d_status: 4-B aligned. */
int sf_index_device_blocks(const void *d_data, uint64_t len, const uint64_t *d_offsets,
                           const uint32_t *d_sizes, uint64_t n_blocks, void *d_digests,
                           int *d_status, void *stream);

/* Opt-in weak checksum -- NOT part of the reference (SURVEY.md 8a row a8:
 * syncfast stores and sends no weak sum); north_star names an "Adler32-style"
 * weak sum beside the strong hash.  As sf_index_device_fixed /
 * sf_index_device_blocks, plus d_weak[i] = zlib Adler-32 (RFC 1950) of block
 * i's bytes, fused into the same pass over HBM (uint32 per block; 0 for an
 * out-of-range explicit block).  d_digests, d_weak and d_status: 4-B aligned. */
int sf_index_device_fixed_weak(const void *d_data, uint64_t len, uint32_t block_size,
                               void *d_digests, uint32_t *d_weak, uint64_t cap_blocks,
                               uint64_t *n_blocks, void *stream);
int sf_index_device_blocks_weak(const void *d_data, uint64_t len, const uint64_t *d_offsets,
                                const uint32_t *d_sizes, uint64_t n_blocks, void *d_digests,
                                uint32_t *d_weak, int *d_status, void *stream);

/* Many-file batch: files[] (host array) describes n_files files inside
 * d_data[0, len).  Writes every file's fixed-size block digests, file after
 * file, to d_digests (cap_blocks rows) and, if d_file_hashes != NULL, each
 * file's blocks_hash (20 B per file, src/index.rs:661-682) computed on the
 * device.  first_block (host, n_files+1 entries, may be NULL) receives the
 * index of each file's first digest row; *n_blocks the total.  Asynchronous
 * on `stream` (ragged batches upload a small block table, stream-ordered).
 * Equal-size batches with d_file_hashes are hashed in two column halves, the
 * first half of every file's blocks_hash chain beside the second half's
 * blocks, then the chains' second half (the batch stream's last batch,
 * sf_index_device_batch_chained_cols): no wave waits for another, so no
 * bound and no timeout (round 6; until then one fused launch whose chain
 * lanes polled and, once, gave up).  d_status (device int32, may be NULL) is
 * accepted for source compatibility and is not written: no error of this
 * call is reported on the device.  (SF_BATCH_FUSED=0: the block kernel, then
 * a chain kernel.)  d_digests and d_file_hashes: 4-B aligned (every route
 * writes them as 32-bit words; a table that is also 16-B aligned takes the
 * faster chain kernels). */
int sf_index_device_batch(const void *d_data, uint64_t len, const sf_file_desc *files,
                          uint32_t n_files, uint32_t block_size, void *d_digests,
                          uint64_t cap_blocks, void *d_file_hashes, uint64_t *first_block,
                          uint64_t *n_blocks, int *d_status, void *stream);

/* Per-file blocks_hash (src/index.rs:661-682) of a batch of equal-size files
 * already hashed into d_digests (n_files files x blocks rows, blocks a
 * multiple of 4): part 0 = whole chains -> d_hashes (20 B per file);
 * part 1 = first half of every chain -> d_state (20 B per file);
 * part 2 = second half, resumed from d_state -> d_hashes.
 * The chain kernels read the runs in 16-B pieces and the states and hashes
 * as 32-bit words: d_digests must be 16-B aligned, d_state and d_hashes 4-B
 * aligned.  A job with n_files != 0 that breaks one of these rules, has
 * blocks = 0, not a multiple of 4 or more than 214,748,364 (20 * blocks above
 * 0xFFFFFFF0), part > 2, no d_digests, no d_state in part 1 or 2, or no
 * d_hashes in part 0 or 2 is SF_EINVAL, and nothing is launched.  A job with
 * n_files = 0 is skipped, whatever its other fields hold. */
typedef struct sf_chain_job {
    const void *d_digests;
    uint32_t n_files;
    uint32_t part;
    uint64_t blocks;
    void *d_state;
    void *d_hashes;
} sf_chain_job;

/* Equal-size many-file batches as a stream (BASELINE config 3, batch after
 * batch, the shape of index_path over a large tree): ONE launch on `stream`
 * hashes every block of this batch -- n_files files of file_len bytes (a
 * multiple of block_size) back to back at d_data -- into d_digests
 * (file-major rows) and, in the same launch, up to two chain jobs of EARLIER
 * batches (digests and states written by earlier launches on the same
 * stream), so their blocks_hash latency hides behind this batch's blocks.
 * n_files = 0 runs only the jobs.  A batch of more than 2^31 blocks is
 * SF_EINVAL (one launch per batch; the other entry points split such inputs
 * into several launches themselves). */
int sf_index_device_batch_chained(const void *d_data, uint32_t n_files, uint64_t file_len,
                                  uint32_t block_size, void *d_digests, const sf_chain_job *jobs,
                                  uint32_t n_jobs, void *stream);

/* The same launch over block columns [col_lo, col_hi) of every file only
 * (rows f * (file_len / block_size) + col of d_digests; the other rows are
 * not written).  col_lo = 0, col_hi = file_len / block_size is
 * sf_index_device_batch_chained; any other range needs 64 | blocks per file,
 * 64 | col_lo, 64 | col_hi and col_lo < col_hi <= blocks per file, else
 * SF_EINVAL.  A stream's LAST batch in two column halves lets the first half
 * of its chains run inside the second launch (device.BatchStream.push_last). */
int sf_index_device_batch_chained_cols(const void *d_data, uint32_t n_files, uint64_t file_len,
                                       uint32_t block_size, uint64_t col_lo, uint64_t col_hi,
                                       void *d_digests, const sf_chain_job *jobs, uint32_t n_jobs,
                                       void *stream);

/* ------------------------------------ the receiving side of a sync ---- */

/* Block lookup of a sync destination.  For every FILE_BLOCK of an incoming
 * file, FsDestinationInner::sink (src/sync/fs.rs:461-476) asks its index
 * whether it holds that block: Index::get_block (src/index.rs:77-103), the
 * first row with that hash and present = 1, SQLite's (hash, rowid) index
 * order.  A block set is that question for a whole table at once: built on
 * the device from the destination's rows -- d_table, n_rows x 20-B digests in
 * rowid order (4-B aligned; the caller keeps it alive while the set is used),
 * d_present, one byte per row (non-zero = present; NULL = all present) --
 * then sf_block_set_lookup writes, for each of n_query digests at d_query,
 * the index of the first present row with that digest, or -1, to d_rows
 * (device int64, 8-B aligned; d_query 4-B aligned).  Asynchronous on `stream`; n_rows <= 2^31.  Lookups only
 * read the set: any number may run at once, on any streams ordered after the
 * build.  sf_block_set_free releases the set (stream-ordered: after the
 * lookups on that stream). */
typedef struct sf_block_set sf_block_set;
int sf_block_set_build(const void *d_table, const uint8_t *d_present, uint64_t n_rows,
                       sf_block_set **out, void *stream);
int sf_block_set_lookup(const sf_block_set *set, const void *d_query, uint64_t n_query,
                        int64_t *d_rows, void *stream);
int sf_block_set_free(sf_block_set *set, void *stream);

/* The signature table as the reference's wire messages, on the device:
 * n_blocks FILE_BLOCK messages, "FILE_BLOCK\n" + 20 digest bytes + "\n" +
 * decimal block size + "\n" (write_message, src/sync/ssh/proto.rs:162-166),
 * what FsSource sends per block after FILE_START (src/sync/fs.rs:217-233).
 * Fixed tiling of a file_len-byte file.  *n_out = bytes written (the need,
 * with SF_ENOSPC and nothing written, when cap is too small).  d_out needs no
 * alignment (byte stores). */
int sf_wire_file_blocks_device(const void *d_digests, uint64_t n_blocks, uint32_t block_size,
                               uint64_t file_len, void *d_out, uint64_t cap, uint64_t *n_out,
                               void *stream);

/* The FILE_BLOCK run of an explicit block list -- the reference's default,
 * content-defined blocks, each with its own size -- built in HBM: message i =
 * "FILE_BLOCK\n" + digest i + "\n" + decimal d_sizes[i] + "\n"
 * (src/sync/ssh/proto.rs:162-166), back to back in list order.  The message
 * offsets come from a scan on the device; the total is read back, so the call
 * blocks until it is known.  *n_out = bytes (the need); SF_ENOSPC (nothing
 * written) when cap is too small or d_out is NULL (a query).  d_out needs no
 * alignment (byte stores). */
int sf_wire_blocks_device(const void *d_digests, const uint32_t *d_sizes, uint64_t n_blocks,
                          void *d_out, uint64_t cap, uint64_t *n_out, void *stream);

/* The same FILE_BLOCK run written to a file descriptor (the SSH pipe of
 * src/sync/ssh/mod.rs, or a file), streamed: the device builds ~1M messages
 * at a time, each chunk comes back by DMA into pinned memory and is written
 * while the device builds the next.  d_digests may still be in production on
 * `stream` (the copy waits for it).  *n_written = bytes written.  Blocking. */
int sf_wire_file_blocks_fd(const void *d_digests, uint64_t n_blocks, uint32_t block_size,
                           uint64_t file_len, int fd, uint64_t *n_written, void *stream);

/* The explicit list's FILE_BLOCK run (sf_wire_blocks_device) streamed to a
 * file descriptor in chunks of messages, each built on the device, copied
 * back and written while the next is built.  *n_written = bytes written.
 * Blocking. */
int sf_wire_blocks_fd(const void *d_digests, const uint32_t *d_sizes, uint64_t n_blocks, int fd,
                      uint64_t *n_written, void *stream);

/* ------------------------------ receiving a FILE_BLOCK run, on the device ---- */

/* Why the parse of a run stopped (what stands after the last whole message). */
enum {
    SF_WIRE_END = 0,        /* the run ends with the buffer */
    SF_WIRE_INCOMPLETE = 1, /* the start of a message: more bytes could complete it */
    SF_WIRE_OTHER = 2,      /* a complete command line of another message (FILE_END, ...):
                               the caller's parser takes over there */
    SF_WIRE_MALFORMED = 3,  /* the reference parser would raise there */
    SF_WIRE_UNEXPECTED = 4, /* sf_receive_files_device only: a whole, valid FILE_START, FILE_BLOCK or
                               FILE_END that the sink's state does not take there */
    SF_WIRE_END_FILES = 5   /* sf_receive_file_entries_device only: "END_FILES\n" stood after the last
                               entry and is counted in *consumed */
};

/* The inverse of sf_wire_blocks_device: the longest prefix of whole FILE_BLOCK
 * messages of d_wire[0, n_bytes), as the reference parser reads them
 * (src/sync/ssh/proto.rs:189-477): message i = "FILE_BLOCK\n" + 20 digest
 * bytes + "\n" + a size field + "\n", the field what usize::from_str takes
 * ("+"? [0-9]+, leading zeros allowed) in at most 15 bytes.  Digest i goes to
 * d_digests + 20 * i (4-B aligned, the table sf_block_set_lookup takes), the
 * size to d_sizes[i].  *n_out = the messages, *consumed = their bytes, *stop =
 * SF_WIRE_* for what stands at d_wire + *consumed: nothing, a message's start
 * (a command line under 20 bytes with no newline included), one of the eight
 * other commands' complete line (whatever follows it), or bytes the parser
 * rejects (an unknown or unterminated command, an unterminated digest or
 * size, an invalid size).  Every byte position is tested for a whole message
 * in parallel, and the positions that chain from byte 0 are the messages
 * (sf_recv.hip); a digest that forges a message start inside
 * a message is noticed, and the run is then copied back and parsed on the
 * host, serially -- the result is the reference parser's for any input.  d_wire needs no alignment.
 * Unlike the reference (usize), sizes are uint32 here as in every other entry
 * point: a size above 2^32 - 1 gives SF_ERANGE.  SF_ENOSPC with *n_out = the
 * need (the first cap entries written) when cap is too small or an output is
 * NULL (a query).  n_bytes == 0 gives 0 messages; n_bytes <= 2^38.
 * d_digests and d_sizes: 4-B aligned.
 * Scratch: n_bytes / 3 from the library's stream-ordered pool.  Blocking. */
int sf_wire_parse_blocks_device(const void *d_wire, uint64_t n_bytes, void *d_digests /* 4-B aligned */,
                                uint32_t *d_sizes, uint64_t cap, uint64_t *n_out,
                                uint64_t *consumed, int *stop, void *stream);

/* The body of the sink's GetFiles state for one run (src/sync/fs.rs:461-478)
 * in one call: sf_wire_parse_blocks_device, then d_offsets[i] = base_offset +
 * d_sizes[0] + ... + d_sizes[i - 1] (the running offset of fs.rs:477, a 64-bit
 * scan), then sf_block_set_lookup of the digests into d_rows (the row to copy
 * from, or -1: add_missing_block) unless set is NULL.  *end_offset = the
 * offset after the last message -- what FILE_END passes to
 * set_file_size_and_compute_blocks_hash (fs.rs:480), and the base_offset of
 * the next call when a run arrives in pieces (the unconsumed tail + the new
 * bytes).  cap entries per output; SF_ENOSPC with *n_out = the need when it
 * is smaller or an output is NULL (the first cap digests and sizes written,
 * no offset and no row).  d_digests and d_sizes: 4-B aligned; d_offsets and
 * d_rows: 8-B aligned.  Blocking. */
int sf_receive_blocks_device(const sf_block_set *set /* NULL: no lookup */, const void *d_wire, uint64_t n_bytes,
                             uint64_t base_offset, void *d_digests, uint32_t *d_sizes, uint64_t *d_offsets,
                             int64_t *d_rows, uint64_t cap, uint64_t *n_out, uint64_t *consumed, int *stop,
                             uint64_t *end_offset, void *stream);

/* The same from host memory: the run goes to HBM through the pinned stages,
 * out[i] = {offset, size, digest} and src_rows[i] (may be NULL without a
 * set) come back.  When the host parse is needed it reads the caller's own
 * bytes: nothing is copied back.  Blocking. */
int sf_receive_blocks_buffer(const sf_block_set *set, const void *wire /* host */, uint64_t n_bytes,
                             uint64_t base_offset, sf_block_sig *out, int64_t *src_rows, uint64_t cap,
                             uint64_t *n_out, uint64_t *consumed, int *stop, uint64_t *end_offset);

/* The sink's whole GetFiles state (src/sync/fs.rs:449-500) for a buffer of
 * MANY files in one call.  The destination sends every GET_FILE at once, so
 * the source answers back to back and one received buffer holds
 *   FILE_START\n<name>\n (FILE_BLOCK\n<20 B>\n<size>\n)* FILE_END\n FILE_START\n...
 * beginning and ending anywhere.  d_wire[0, n_bytes) is parsed as the
 * reference parser reads it (FILE_START: a name of 0 to 100 bytes holding no
 * newline, read_line(FILENAME_MAX) of proto.rs:271-290 -- 100 name bytes or
 * more with no newline among the first 101 are "Unterminated filename", not a
 * prefix; FILE_BLOCK as sf_wire_parse_blocks_device; FILE_END) and accepted in
 * the sink's order: FILE_START only with no file open, FILE_BLOCK and FILE_END
 * only with one; `open` != 0 says that a file was open when the buffer began.
 *
 * Sections: the files of the call, numbered in stream order.  With open != 0
 * section 0 is the file carried in (its FILE_START came in an earlier call):
 * d_file_name_at[0] = UINT64_MAX, d_file_name_len[0] = 0, its offsets start at
 * base_offset, and it exists even with no message at all (*n_files >= 1).
 * Every FILE_START opens the next section f: its name is the
 * d_file_name_len[f] bytes at d_wire + d_file_name_at[f] (bytes as they came:
 * String::from_utf8 and get_temp_file stay with the caller).  d_file_first[f]
 * = the section's first block; d_file_first has *n_files + 1 entries, the
 * last = *n_blocks (an empty file: first[f] == first[f + 1], size 0).
 * d_file_size[f] = the running offset at the section's end: what FILE_END
 * passes to set_file_size_and_compute_blocks_hash (fs.rs:480).  Every section
 * but the last is closed; the last is closed exactly when *open_out == 0.
 * Blocks: block i is digest d_digests + 20 * i, d_sizes[i], section
 * d_block_file[i], d_offsets[i] = the running offset of fs.rs:477 within its
 * section (restarted at every FILE_START; + base_offset in a section carried
 * in) and, with a set, d_rows[i] = sf_block_set_lookup's row or -1 (one lookup
 * of all digests of all files).
 *
 * *consumed = the bytes of the accepted messages, *stop = SF_WIRE_* for what
 * stands at d_wire + *consumed: the other six commands' complete line is
 * SF_WIRE_OTHER whatever follows it, a whole message of the three kinds that
 * the sink's state does not take is SF_WIRE_UNEXPECTED.  *end_offset = the
 * running offset of the last section (base_offset unchanged when there is no
 * section).  A buffer that arrives in pieces is continued with the unconsumed
 * tail + the new bytes, open = *open_out and base_offset = *end_offset.
 *
 * Every byte position is tested for a whole message in parallel, and the
 * positions that chain from byte 0 in the sink's order are the messages
 * (sf_recv_files.hip).  A message start inside the last
 * chained message -- a digest that spells a tag, a file named "x/FILE_END", a
 * name that ends in "FILE_START" in front of a FILE_BLOCK -- is noticed, and
 * the buffer is then copied back and parsed on the host, serially: the result
 * is the reference's for any input.
 *
 * SF_ENOSPC with both needs in *n_blocks / *n_files (and *consumed, *stop,
 * *open_out) when block_cap or file_cap is too small or one of the
 * outputs but d_rows is NULL (a query: nothing is written then).  With a capacity too small, the first min(need, cap) entries of
 * d_digests, d_sizes and d_block_file and of d_file_name_at, d_file_name_len
 * and d_file_first (without its last entry) are written; no offset, no file
 * size, no row.  Nothing past block_cap / file_cap entries (file_cap + 1 of
 * d_file_first) is ever written.  A size above 2^32 - 1 gives SF_ERANGE.
 * SF_EINVAL before any device call: a NULL result pointer, a NULL buffer with
 * n_bytes > 0, n_bytes > 2^35 (the files and the blocks before a position are
 * counted in the two halves of one 64-bit scan), d_rows NULL with a set;
 * d_digests, d_sizes, d_block_file, d_file_name_len not 4-B aligned;
 * d_offsets, d_rows, d_file_name_at, d_file_first, d_file_size not 8-B
 * aligned.  n_bytes == 0 launches nothing, needs no device, writes no entry
 * and hands the state back: *open_out = (open != 0), *end_offset =
 * base_offset, *n_files = that.  d_wire needs no alignment.
 * Scratch: n_bytes * 0.8 at the most from the library's stream-ordered pool.  Blocking. */
int sf_receive_files_device(const sf_block_set *set /* NULL: no lookup */, const void *d_wire, uint64_t n_bytes,
                            int open, uint64_t base_offset, void *d_digests /* 4-B aligned */, uint32_t *d_sizes,
                            uint64_t *d_offsets, int64_t *d_rows, uint32_t *d_block_file, uint64_t block_cap,
                            uint64_t *d_file_name_at, uint32_t *d_file_name_len, uint64_t *d_file_first,
                            uint64_t *d_file_size, uint64_t file_cap, uint64_t *n_blocks, uint64_t *n_files,
                            uint64_t *consumed, int *stop, int *open_out, uint64_t *end_offset, void *stream);

/* ------------------------------ receiving a BLOCK_DATA run, on the device ---- */

/* The messages that carry the bytes: after GET_BLOCK the source answers with
 * BLOCK_DATA messages (written by src/sync/ssh/proto.rs:175-181, parsed by
 * :419-446), and the sink's GetBlocks state writes each payload to every
 * location that wants it (src/sync/fs.rs:503-516) -- without hashing it
 * (fs.rs:505-510): a corrupt payload is written and marked present.  This
 * call parses a received run on the device exactly as the reference parser
 * reads it and, unlike the reference, checks every payload against the digest
 * its message claims.
 *
 * Message i = "BLOCK_DATA\n" + 20 digest bytes + "\n" + a length field (what
 * usize::from_str takes, at most 15 bytes) + "\n" + `length` payload bytes +
 * "\n".  The longest prefix of whole messages of d_wire[0, n_bytes): the
 * claimed digest of message i goes to d_digests + 20 * i (4-B aligned, the
 * table sf_block_set_lookup takes), its payload's length to d_sizes[i] and
 * its payload's offset from d_wire to d_data_offsets[i].  *n_out = the
 * messages, *consumed = their bytes, *stop = SF_WIRE_* for what stands at
 * d_wire + *consumed (FILE_BLOCK is one of the other commands here; a wrong
 * byte after a payload, "Invalid data end byte", is SF_WIRE_MALFORMED).  With
 * SF_WIRE_INCOMPLETE after a whole header, *need = that message's full length
 * (the bytes from *consumed on that complete it), else 0.
 *
 * With d_ok, every payload is hashed where it lies (the explicit-list kernel
 * of sf_index_device_blocks over d_wire) and d_ok[i] = 1 when its SHA-1 is the
 * claimed digest, else 0; *n_bad = the payloads that did not verify.  d_ok
 * NULL: parse only, nothing is hashed.
 *
 * A payload is arbitrary file content and may hold whole BLOCK_DATA messages
 * of its own, or headers whose length lands on a later message's end byte.
 * Every byte position is tested for a whole message in parallel; when no such
 * candidate lies inside a chained message the chain is found on the device,
 * else only the candidates' positions and lengths (16 B each, no payload
 * byte) go to the host, which walks them (sf_recv_data.hip).
 * The result is the reference parser's for any input.
 *
 * d_wire needs no alignment.  A chained length above 2^32 - 1 gives
 * SF_ERANGE.  SF_ENOSPC with *n_out = the need (the first cap entries
 * written, nothing hashed) when cap is too small or one of d_digests,
 * d_sizes, d_data_offsets is NULL (a query).  n_bytes == 0 gives 0 messages
 * and launches nothing; n_bytes <= 2^38.  d_digests and d_sizes: 4-B aligned;
 * d_data_offsets: 8-B aligned; d_ok: bytes, any address.  Blocking. */
int sf_receive_block_data_device(const void *d_wire, uint64_t n_bytes, void *d_digests /* 4-B aligned */,
                                 uint32_t *d_sizes, uint64_t *d_data_offsets,
                                 uint8_t *d_ok /* NULL: parse only */, uint64_t cap,
                                 uint64_t *n_out, uint64_t *consumed, int *stop, uint64_t *need,
                                 uint64_t *n_bad, void *stream);

/* The same from host memory: the run goes to HBM through the pinned stages,
 * out[i] = {offset = the payload's offset in wire, size, sha1 = the claimed
 * digest} and ok[i] (NULL: parse only) come back; no payload byte does.
 * SF_ENOSPC with the need when cap is too small or out is NULL.  SF_ENODEV
 * without a device.  Blocking. */
int sf_receive_block_data_buffer(const void *wire /* host */, uint64_t n_bytes, sf_block_sig *out, uint8_t *ok,
                                 uint64_t cap, uint64_t *n_out, uint64_t *consumed, int *stop,
                                 uint64_t *need, uint64_t *n_bad);

/* ------------------------------ sending a BLOCK_DATA run, from the device ---- */

/* The source's answer to GET_BLOCK: for every request FsSource looks the
 * digest up (Index::get_block), reads the block (read_block) and writes one
 * BLOCK_DATA message (src/sync/fs.rs:199-208, src/sync/ssh/proto.rs:175-181).
 * Here a whole run of such messages is built in HBM in one call.
 *
 * A run is owned by the library: its length is known only after a scan of the
 * message lengths on the device, so the library allocates it (from its
 * stream-ordered pool, which keeps the block for later runs on that stream)
 * and hands out a handle.  sf_wire_run_info gives the device pointer (NULL for
 * an empty run), the bytes and the messages; the bytes are complete once the
 * building stream has run past the building call, and sf_wire_run_read /
 * sf_wire_run_to_fd wait for exactly that themselves.  sf_wire_run_free
 * releases the run stream-ordered (after the work `stream` holds, as
 * sf_block_set_free); NULL is fine. */
typedef struct sf_wire_run sf_wire_run;

/* Message i = "BLOCK_DATA\n" + the 20 bytes at d_digests + 20 * i + "\n" +
 * decimal d_sizes[i] + "\n" + src[d_src_offsets[i], + d_sizes[i]) + "\n",
 * 34 + digits + size bytes, back to back in list order: byte for byte what
 * write_message gives.  The reference cuts the file again in read_block to
 * find the block's end; here the size the index holds is taken as given.
 * Sizes are any uint32 (0: a 35-byte message), offsets any uint64, nothing is
 * aligned beyond the lists' element types and the digest table (4 B, as
 * everywhere); sources may overlap or repeat.  A job whose source does not lie
 * in [0, src_len) (offset + size past 2^64 included) gives SF_ERANGE: *out =
 * NULL, nothing is built and no byte outside the buffer is loaded.
 * One lane per job writes the lengths, a uint64 scan turns them into end
 * offsets, the total and the range flag come back in one 16-byte copy (the
 * call blocks there, once), one lane per message writes its header and end
 * byte with byte stores, and the payloads go through the block copy kernel of
 * sf_copy_blocks_device (sf_send.hip).  Scratch: 24 n_blocks
 * bytes plus the scan's and the copy's.  n_blocks == 0 gives an empty run,
 * launches nothing and needs no device.  SF_EINVAL, before any device call,
 * for a NULL out, for n_blocks > 2^32 and for a NULL or misaligned list or a
 * NULL buffer with n_blocks > 0. */
int sf_wire_block_data_device(const void *d_src, uint64_t src_len, const void *d_digests,
                              const uint64_t *d_src_offsets, const uint32_t *d_sizes,
                              uint64_t n_blocks, sf_wire_run **out, void *stream);

/* A received run of GET_BLOCK requests answered in one call.  d_requests[0,
 * n_bytes) is parsed as the reference parser reads it: message k is the 31
 * bytes at 31 k, "GET_BLOCK\n" + 20 digest bytes of any value + "\n";
 * *n_requests = the leading messages, *consumed = 31 * *n_requests, *stop =
 * SF_WIRE_* for what stands at d_requests + *consumed (every proper prefix of
 * a request is SF_WIRE_INCOMPLETE, COMPLETE and the other seven commands
 * SF_WIRE_OTHER, a wrong byte after the digest SF_WIRE_MALFORMED).  Each
 * digest is looked up in `set` (sf_block_set_lookup: the first present row
 * holding it, Index::get_block) and request k becomes message k of *out with
 * the bytes src[d_row_offsets[row], + d_row_sizes[row]) -- two device arrays
 * with one entry per row of the set.  A repeated request is answered each
 * time.  Requests [0, *n_answered) are answered: up to the first whose digest
 * the set does not hold, where the reference, having answered the earlier
 * ones, fails with "Requested block is unknown" -- the caller raises that when
 * *n_answered < *n_requests.  A row whose block leaves [0, src_len) gives
 * SF_ERANGE as above.  One lane per 31-byte slot tests the tag line and the
 * end byte; the stop is decided on the host from at most 128 bytes copied
 * back.  n_bytes == 0 gives an empty run and SF_WIRE_END; n_bytes <= 2^38.
 * SF_EINVAL for a NULL result pointer and for a NULL set or run with
 * n_bytes > 0.  Blocking. */
int sf_serve_get_blocks_device(const sf_block_set *set, const uint64_t *d_row_offsets,
                               const uint32_t *d_row_sizes, const void *d_src, uint64_t src_len,
                               const void *d_requests, uint64_t n_bytes, sf_wire_run **out,
                               uint64_t *n_requests, uint64_t *n_answered, uint64_t *consumed,
                               int *stop, void *stream);

/* The run's device pointer and counts (each result pointer may be NULL).
 * SF_EINVAL for a NULL run. */
int sf_wire_run_info(const sf_wire_run *run, const void **bytes, uint64_t *n_bytes, uint64_t *n_messages);

/* Bytes [offset, offset + len) of the run to host memory.  SF_ERANGE when
 * they do not lie in the run.  Blocking. */
int sf_wire_run_read(const sf_wire_run *run, uint64_t offset, void *out /* host */, uint64_t len);

/* The run written to fd with write(), in order, so a pipe works: the source's
 * SSH pipe (src/sync/ssh/mod.rs).  The bytes come back in stages (64 MiB) by
 * DMA into pinned buffers; stage k is copied while stage k - 2 is written.
 * *n_written (may be NULL) = the bytes known written.  SF_EIO on a failed
 * write (a closed pipe: with SIGPIPE ignored or handled, EPIPE).  Blocking. */
int sf_wire_run_to_fd(const sf_wire_run *run, int fd, uint64_t *n_written);

int sf_wire_run_free(sf_wire_run *run, void *stream);

/* ------------------------- answering GET_FILE requests, from the device ---- */

/* The source's answer to a list of GET_FILE requests.  The destination sends
 * every GET_FILE at once, and FsSource answers them back to back: for each
 * file "FILE_START\n" + name + "\n", one FILE_BLOCK per row of
 * list_file_blocks, "FILE_END\n" (src/sync/fs.rs:177-231, written by
 * src/sync/ssh/proto.rs:157-169).  Here the whole answer -- the stream
 * sf_receive_files_device takes -- is built in HBM in one call.
 *
 * Blocks: d_digests + 20 * i and d_sizes[i], any uint32, for all files
 * together in answer order.  Files: d_file_first[0, n_files] is the CSR into
 * them (file f owns blocks [d_file_first[f], d_file_first[f + 1]); an empty
 * file owns none) and d_name_at[0, n_files] the CSR into the packed name
 * bytes d_names[0, d_name_at[n_files]) (any address; may be NULL when every
 * name is empty).  With E the inclusive end offsets of the FILE_BLOCK
 * messages alone (33 + digits(size) bytes each) and Bex(i) = i ? E[i - 1] : 0:
 *   FILE_START of file f   at Bex(first[f]) + name_at[f] + 21 f
 *   FILE_BLOCK i of file f at Bex(i) + name_at[f + 1] + 21 f + 12
 *   FILE_END of file f     at Bex(first[f + 1]) + name_at[f + 1] + 21 f + 12
 *   the run's length       = Bex(n_blocks) + name_at[n_files] + 21 n_files
 * byte for byte what write_message gives, n_blocks + 2 n_files messages.
 *
 * File f is refused when its entries do not hold: first[0] == 0, first[f] <=
 * first[f + 1], first[n_files] == n_blocks, name_at[0] == 0, name_at[f] <=
 * name_at[f + 1] <= name_at[n_files], and a name of at most 100 bytes with no
 * '\n' in it -- the names the protocol can carry (read_line(FILENAME_MAX),
 * proto.rs:271-290); no other name can have arrived in a GET_FILE, and the
 * receiver could not parse one.  Then the call returns SF_EINVAL with
 * *bad_file = the first such file and *run = NULL, and keeps nothing
 * allocated; no byte outside the arrays as described is loaded.  *bad_file =
 * UINT64_MAX in every other case.
 *
 * *run is the handle above (sf_wire_run_info, _read, _to_fd, _free).  The
 * block lengths are scanned as for sf_wire_blocks_device, one lane per file
 * tests its entries and its name (the first failing file is an atomic
 * minimum, one atomic per wave), the scan's total, name_at[n_files] and that
 * word come back in one 24-byte copy (the call blocks there, once), then one
 * lane per file writes its FILE_START and FILE_END and one lane per block
 * finds its file by an upper-bound binary search of d_file_first and writes
 * its FILE_BLOCK, all with byte stores (sf_send_files.hip).
 * No array is written; all may still be in production on `stream`.  Scratch:
 * 16 n_blocks bytes plus the scan's.  n_files == 0 with n_blocks == 0 gives an
 * empty run, launches nothing and needs no device.  SF_EINVAL, before any
 * device call, for a NULL run or bad_file, for n_blocks + 2 n_files > 2^32,
 * for blocks without a file, for a NULL d_file_first or d_name_at with
 * n_files > 0, for a NULL d_digests or d_sizes with n_blocks > 0, for a
 * d_digests or d_sizes that is not 4-B aligned and for a d_file_first or
 * d_name_at that is not 8-B aligned. */
int sf_wire_files_device(const void *d_digests /* n_blocks x 20 B: 4-B aligned */,
                         const uint32_t *d_sizes, uint64_t n_blocks,
                         const uint64_t *d_file_first /* n_files + 1 */, const void *d_names,
                         const uint64_t *d_name_at /* n_files + 1 */, uint64_t n_files,
                         sf_wire_run **run, uint64_t *bad_file, void *stream);

/* ------------------------------ exchanging the files list, on the device ---- */

/* The first phase of a sync (src/sync/fs.rs).  The source sends its files
 * list, one "FILE_ENTRY\n" + name + "\n" + size + "\n" + 20 B blocks_hash +
 * "\n" per file and "END_FILES\n" (fs.rs:133-164, proto.rs:142-151); the
 * destination looks every name up in its index, compares the announced
 * blocks_hash with the recorded one and asks for the files that differ or are
 * unknown, one "GET_FILE\n" + name + "\n" each (fs.rs:378-446, proto.rs:152-156)
 * -- the requests sf_wire_files_device answers.  Here: the lookup by name for
 * a whole list (a name set), the list built in one call, the list received in
 * one call, and the request run built in one call (sf_names.hip,
 * sf_send_entries.hip, sf_recv_entries.hip). */

/* Index::get_file for a whole list at once, the sibling of the block set:
 * the destination's names as an open-addressing table in HBM.  Row r's name is
 * d_names[d_name_at[r], d_name_at[r + 1]): packed bytes at any address and
 * their CSR (n_rows + 1 entries, 8-B aligned), rows in file_id order; a name
 * may have any length, 0 and more than 100 included.  d_present (optional, one
 * byte per row, the mirror of temporary = 0): a row with 0 is not in the set.
 * Both arrays must stay as they are while the set is used.  A CSR that does
 * not hold (d_name_at[0] != 0, an entry above its successor or above the last
 * one) gives SF_EINVAL with *bad_row = the first such row, and nothing is kept
 * allocated; *bad_row = UINT64_MAX in every other case.  One lane per row
 * tests its entries and inserts its row id with one atomic compare-and-swap per
 * probe; the first bad row comes back (the call blocks there, once).  Memory:
 * 16 to 32 bytes per row from the library's stream-ordered pool, until
 * sf_name_set_free (stream-ordered).  n_rows == 0 gives a set that answers -1
 * everywhere, launches nothing and needs no device.  SF_EINVAL, before any
 * device call, for a NULL out or bad_row, n_rows > 2^31, a NULL d_name_at with
 * n_rows > 0 or one that is not 8-B aligned. */
typedef struct sf_name_set sf_name_set;
int sf_name_set_build(const void *d_names, const uint64_t *d_name_at /* n_rows + 1 */,
                      const uint8_t *d_present /* may be NULL */, uint64_t n_rows, sf_name_set **out,
                      uint64_t *bad_row, void *stream);

/* Query i is the d_len[i] bytes at d_bytes + d_at[i] -- spans anywhere in
 * d_bytes[0, n_bytes), no alignment: the shape sf_receive_files_device and
 * sf_receive_file_entries_device write.  d_rows[i] = the lowest present row
 * whose name has the same length and the same bytes, or -1: what get_file's
 * rows.next() gives through idx_files_name (the schema has no UNIQUE on name).
 * A span that leaves d_bytes[0, n_bytes) is not read and gives -1.  The set is
 * only read; asynchronous on `stream`.  SF_EINVAL, before any device call,
 * for a NULL set, a NULL array with n_query > 0, a NULL d_bytes with
 * n_bytes > 0, a d_at or d_rows that is not 8-B aligned or a d_len that is not
 * 4-B aligned. */
int sf_name_set_lookup(const sf_name_set *set, const void *d_bytes, uint64_t n_bytes, const uint64_t *d_at,
                       const uint32_t *d_len, uint64_t n_query, int64_t *d_rows, void *stream);
int sf_name_set_free(sf_name_set *set, void *stream);

/* The source's ListFiles state in one call: for file f write_message's
 * FILE_ENTRY of its name d_names[d_name_at[f], d_name_at[f + 1]) (packed bytes
 * at any address, CSR of n_files + 1 entries), d_sizes[f] and the 20 bytes at
 * d_hashes + 20 f, file after file, and "END_FILES\n" behind them when
 * end_files != 0: 34 + name + digits(size) bytes per entry, byte for byte what
 * the reference writes.  *run is the handle above (sf_wire_run_info, _read,
 * _to_fd, _free).
 * File f is refused when its CSR entries do not hold (as for
 * sf_wire_files_device), when its name is over 100 bytes or holds '\n', or
 * when its size is 10^15 or more (a field of 16 digits, which the receiver's
 * read_line(SIZE_MAX) cannot take).  The reference would send such an entry,
 * and its peer would raise in the middle of the list.  Then the call returns
 * SF_EINVAL with *bad_file = the first such file and *run = NULL and keeps
 * nothing allocated; *bad_file = UINT64_MAX in every other case.
 * One lane per file tests it and gives its entry's length, a scan places the
 * entries, the first bad file and the total come back (the call blocks there,
 * once), then one lane per entry writes it with byte stores.  Scratch: 12
 * n_files bytes plus the scan's.  n_files == 0 gives an empty run, launches
 * nothing and needs no device -- or, with end_files, the 10-byte run.
 * SF_EINVAL, before any device call, for a NULL run or bad_file, n_files >
 * 2^31, a NULL d_name_at, d_sizes or d_hashes with n_files > 0, a d_name_at or
 * d_sizes that is not 8-B aligned or a d_hashes that is not 4-B aligned. */
int sf_wire_file_entries_device(const void *d_names, const uint64_t *d_name_at /* n_files + 1 */,
                                const uint64_t *d_sizes, const void *d_hashes /* n_files x 20 B: 4-B aligned */,
                                uint64_t n_files, int end_files, sf_wire_run **run, uint64_t *bad_file,
                                void *stream);

/* The sink's FilesList state for one received buffer in one call.  The
 * longest prefix of whole FILE_ENTRY messages of d_wire[0, n_bytes) (any
 * address) is parsed as the reference parser reads them (proto.rs:337-364): a
 * name of 0 to 100 bytes with its newline among the first 101, a size field
 * that usize::from_str takes in at most 15 bytes with its newline among the
 * first 16, 20 raw bytes, "\n"; 35 to 149 bytes.  Per entry i, cap rows each:
 * d_name_at[i] = the name's offset in d_wire, d_name_len[i], d_sizes[i],
 * d_hashes + 20 i.  *n_out = the entries, *consumed = their bytes, *stop =
 * SF_WIRE_* for what stands behind them; SF_WIRE_END_FILES: "END_FILES\n"
 * stood there and is counted in *consumed.  100 name bytes with no newline
 * among 101, 15 size bytes with none among 16 and another byte than "\n"
 * behind the hash are SF_WIRE_MALFORMED, not a prefix.  *bad_name = the first
 * entry whose name is not what Rust's String::from_utf8 takes ("Bad filename
 * encoding", fs.rs:381-383), UINT64_MAX if none; the entries behind it are
 * parsed and written all the same, the caller stops there.
 * With a set, three more outputs: d_rows[i] = sf_name_set_lookup of the name;
 * d_need[i] = 1 when that is -1, when the row has no recorded hash
 * (d_have_hash_ok[row] == 0; NULL: every row has one) or when the 20 bytes at
 * d_have_hashes + 20 row differ from the announced hash in any byte, else 0;
 * d_need_list[0, *n_need) = the entries with need 1, ascending: the d_pick
 * sf_wire_get_files_device takes.  With set == NULL the three must be NULL
 * and the call is a parse only (*n_need = 0).
 * SF_ENOSPC with *n_out = the need when cap is smaller or an output is NULL:
 * the first cap rows of the four parsed lists are written (none when an
 * output is NULL), no row, need or list entry.  Nothing past cap rows is ever
 * written.  A list that arrives in pieces is continued with the unconsumed
 * tail plus the new bytes: there is no state to carry.
 * Every byte position is tested for a whole entry in parallel and the
 * positions that chain from byte 0 are the entries; a blocks_hash that forges
 * an entry's start inside the last chained entry is noticed, and the buffer is
 * then copied back and parsed on the host, serially: the result is the
 * reference parser's for any input.  Blocking: one read-back for the parse, a
 * second for *n_need.  n_bytes == 0 launches nothing and needs no device;
 * n_bytes <= 2^35.  SF_EINVAL, before any device call, for a NULL result
 * pointer, a NULL d_wire with n_bytes > 0, a lookup output without a set, a
 * set without d_have_hashes, a d_name_at, d_sizes or d_rows that is not 8-B
 * aligned, a d_name_len, d_hashes, d_need_list or d_have_hashes that is not
 * 4-B aligned. */
int sf_receive_file_entries_device(const sf_name_set *set /* NULL: no lookup */, const void *d_wire,
                                   uint64_t n_bytes, const void *d_have_hashes /* rows x 20 B: 4-B aligned */,
                                   const uint8_t *d_have_hash_ok /* may be NULL */, uint64_t *d_name_at,
                                   uint32_t *d_name_len, uint64_t *d_sizes, void *d_hashes, int64_t *d_rows,
                                   uint8_t *d_need, uint32_t *d_need_list, uint64_t cap, uint64_t *n_out,
                                   uint64_t *n_need, uint64_t *bad_name, uint64_t *consumed, int *stop,
                                   void *stream);

/* The destination's request run: message k is "GET_FILE\n" + name + "\n" of
 * the name d_bytes[d_name_at[i], + d_name_len[i]) with i = d_pick[k] -- the
 * spans sf_receive_file_entries_device wrote, read in place from the received
 * list d_bytes[0, n_bytes) -- for k in [0, n_pick); d_pick == NULL: all n
 * spans in order (n_pick is not read).  Byte for byte write_message.  *run is
 * the handle above.  SF_EINVAL with *bad = the first pick whose index is not
 * below n, whose span leaves the buffer or whose name is over 100 bytes or
 * holds '\n', and *run = NULL; *bad = UINT64_MAX in every other case.  Lengths,
 * scan, one read-back, byte stores, as for sf_wire_file_entries_device.  No
 * message gives an empty run, launches nothing and needs no device.
 * SF_EINVAL, before any device call, for a NULL run or bad, n or n_pick >
 * 2^31, a NULL span array with n > 0, a NULL d_bytes with n_bytes > 0, a
 * d_name_at that is not 8-B aligned, a d_name_len or d_pick that is not 4-B
 * aligned. */
int sf_wire_get_files_device(const void *d_bytes, uint64_t n_bytes, const uint64_t *d_name_at,
                             const uint32_t *d_name_len, uint64_t n, const uint32_t *d_pick /* may be NULL */,
                             uint64_t n_pick, sf_wire_run **run, uint64_t *bad, void *stream);

/* ------------------- answering a received GET_FILE run, on the device ---- */

/* The source's side of those requests (src/sync/fs.rs:177-231): a received run
 * of GET_FILE messages parsed, and answered, in one call each
 * (sf_serve_files.hip).  With sf_serve_get_blocks_device every
 * request the source receives is then answered in HBM from the received bytes. */

/* The inverse of sf_wire_get_files_device.  The longest prefix of whole
 * GET_FILE messages of d_wire[0, n_bytes) (any address) is parsed as the
 * reference parser reads them (proto.rs:365-376): "GET_FILE\n", a name of 0 to
 * 100 bytes with its newline among the first 101; 10 to 110 bytes.  Per
 * request i, cap rows each: d_name_at[i] = the name's offset in d_wire,
 * d_name_len[i] -- the spans sf_name_set_lookup takes.  *n_out = the requests,
 * *consumed = their bytes, *stop = SF_WIRE_* for what stands behind them: 100
 * name bytes with no newline (also when only those 100 are there yet), 20
 * command bytes with none and an unknown command are SF_WIRE_MALFORMED, the
 * complete command line of one of the other eight commands SF_WIRE_OTHER.
 * *bad_name = the first request whose name is not what Rust's String::from_utf8
 * takes ("Bad filename encoding", fs.rs:181-183), UINT64_MAX if none; the
 * requests behind it are parsed and written all the same.
 * SF_ENOSPC with *n_out = the need when cap is smaller or an output is NULL:
 * the first cap rows are written (none when an output is NULL).  Nothing past
 * cap rows is ever written.  A run that arrives in pieces is continued with
 * the unconsumed tail plus the new bytes: there is no state to carry.
 * A name holds no newline, so request k is lines 2k and 2k + 1 of the buffer:
 * the newlines are found and counted in parallel, one lane per 64 positions
 * judges its newlines' lines by the parity of their index, and the first
 * failing line is an atomic minimum.  No position is guessed, so no input can
 * forge a request and there is no host fallback: the result is the reference
 * parser's for any input.  Blocking: one read-back.  n_bytes == 0 launches
 * nothing and needs no device; n_bytes <= 2^35.  SF_EINVAL, before any device
 * call, for a NULL result pointer, a NULL d_wire with n_bytes > 0, a d_name_at
 * that is not 8-B aligned or a d_name_len that is not 4-B aligned. */
int sf_wire_parse_get_files_device(const void *d_wire, uint64_t n_bytes, uint64_t *d_name_at,
                                   uint32_t *d_name_len, uint64_t cap, uint64_t *n_out,
                                   uint64_t *bad_name, uint64_t *consumed, int *stop, void *stream);

/* Why sf_serve_get_files_device stopped answering (*why). */
enum {
    SF_SERVE_ALL = 0,      /* every request was answered */
    SF_SERVE_BAD_NAME = 1, /* the next request's name is not UTF-8 ("Bad filename encoding"; the
                              reference checks this first, so it wins over SF_SERVE_UNKNOWN) */
    SF_SERVE_UNKNOWN = 2,  /* the set does not hold the next request's name ("Requested file is
                              unknown") */
    SF_SERVE_FULL = 3      /* with the next answer the run would exceed max_run_bytes, or 2^32
                              messages: send the run and call again from *answered_bytes */
};

/* A received run of GET_FILE requests answered in one call.  The source's
 * tables stay in HBM for the whole sync: `set`, the name set over its
 * non-temporary files in file_id order, and a CSR of those rows into the
 * index's own block table: row r owns blocks [d_file_first[r], d_file_first[r
 * + 1]) of d_digests (20 B each) and d_sizes, in list_file_blocks order.
 * Nothing is gathered on the host and no digest is copied in HBM: the kernels
 * read the table through request -> row -> block.
 * d_requests[0, n_bytes) is parsed as by sf_wire_parse_get_files_device:
 * *n_requests, *consumed and *stop describe the whole parsed prefix.  Every
 * name is looked up in the set (sf_name_set_lookup: the lowest present row,
 * Index::get_file) and request k becomes FILE_START with the name's bytes
 * (read in place from d_requests), one FILE_BLOCK per block of its row and
 * FILE_END -- the messages of sf_wire_files_device, byte for byte what the
 * reference writes.  A repeated request is answered each time; an empty file
 * gives two messages.  Requests [0, *n_answered) are answered, up to the first
 * that cannot be, and *why (SF_SERVE_*) says what stopped it; *answered_bytes
 * = the bytes of d_requests those requests occupy.  The caller sends the run
 * and then raises what *why names, as the reference does, or after
 * SF_SERVE_FULL calls again with the requests from *answered_bytes on.
 * max_run_bytes (0: no bound) bounds the run: a peer can repeat one large
 * file's name, the reference streams its answer, and this call allocates it.
 * The answered prefix is the longest whose run fits.
 * The row of the request where answering stops, when its name is UTF-8 and
 * known, must hold: d_file_first[r] <= d_file_first[r + 1] <= n_blocks.  Else
 * SF_EINVAL with *bad_row = that row and *run = NULL; nothing is kept allocated
 * and no byte outside the arrays as described is loaded (such a row's blocks
 * are never read).  *bad_row = UINT64_MAX in every other case.  Rows no request
 * names are never read.
 * Parse, lookup, per-request block counts and their scan, a coarse stop (every
 * block at its shortest) and the stop before it, the block sizes gathered in
 * answer order and their lengths' 64-bit scan, the exact stop, allocation,
 * frames, blocks: every step a kernel, each block finding its request by an
 * upper-bound binary search of the request CSR, every first-stop an atomic
 * minimum with one atomic per wave.  Blocking: THREE read-backs, whatever the
 * number of requests (the parse; the coarse stop and its block count; the
 * answered requests and the run's length) -- one when no request was parsed,
 * two or three when none is answered.  Scratch: 20 bytes per 10 request bytes, 32 per
 * request, 20 per answered block, plus the scans'.  n_bytes == 0 gives an
 * empty run and SF_WIRE_END, launches nothing and needs no device; no
 * answered request gives an empty run too.  n_bytes <= 2^35, n_blocks <= 2^32.
 * SF_EINVAL, before any device call, for a NULL result pointer, a NULL set,
 * d_requests or d_file_first with n_bytes > 0, a NULL d_digests or d_sizes
 * with n_bytes > 0 and n_blocks > 0, a d_file_first that is not 8-B aligned, a
 * d_digests or d_sizes that is not 4-B aligned. */
int sf_serve_get_files_device(const sf_name_set *set, const uint64_t *d_file_first /* set rows + 1 */,
                              const void *d_digests /* n_blocks x 20 B: 4-B aligned */,
                              const uint32_t *d_sizes, uint64_t n_blocks, const void *d_requests,
                              uint64_t n_bytes, uint64_t max_run_bytes /* 0: no bound */,
                              sf_wire_run **run, uint64_t *n_requests, uint64_t *n_answered,
                              uint64_t *answered_bytes, int *why, uint64_t *bad_row,
                              uint64_t *consumed, int *stop, void *stream);

/* ----------------------- the destination's missing blocks, on the device ---- */

/* The two steps between the runs.  After the FILE_BLOCK runs the sink lists
 * its rows with present = 0 and sends one GET_BLOCK per row
 * (Index::list_missing_blocks and src/sync/fs.rs:485-493, written by
 * src/sync/ssh/proto.rs:170-174); for every BLOCK_DATA that comes back it
 * asks the index where that hash is wanted (list_block_locations), writes the
 * payload at each such row and marks it present, one query and one update per
 * message (fs.rs:505-510).  Here the list of missing rows stays in HBM: its
 * request run is built there, and a parsed BLOCK_DATA run is joined against
 * it there, straight into the lists sf_copy_blocks_device takes
 * (sf_want.hip). */

/* The request run of a table of n_rows rows, d_digests + 20 * i the digest of
 * row i (4-B aligned, rowid order).  Row i asks when d_rows is NULL or
 * d_rows[i] < 0 -- d_rows is the array sf_receive_blocks_device wrote (8-B
 * aligned) -- and d_take is NULL or d_take[i] != 0 (bytes, any address; for
 * instance the negation of a present array).  Message k of *out is the 31
 * bytes "GET_BLOCK\n" + digest + "\n" of the k-th asking row, in row order:
 * with distinct == 0 byte for byte write_message over list_missing_blocks,
 * whose SELECT has no DISTINCT -- a digest missing in three rows is requested
 * three times, and answered three times.  With distinct != 0 only the first
 * asking row of each digest asks (a block set over the asking rows, a lookup
 * of every row's own digest: a row asks when the answer is itself).  A digest
 * is 20 bytes of any value.
 * *out is the run handle above (sf_wire_run_info, _read, _to_fd, _free);
 * *n_requests (may be NULL) = its messages.  One lane per row writes a flag,
 * a uint64 scan numbers the asking rows, the count comes back (the call
 * blocks there, once), the run is allocated from the stream-ordered pool and
 * one lane per row writes its message with byte stores.  Scratch: 9 n_rows
 * bytes (17 with distinct, plus the set's 16 to 32) plus the scan's.
 * n_rows == 0 gives an empty run, launches nothing and needs no device; no
 * row asking gives an empty run too.  SF_EINVAL, before any device call, for
 * a NULL out, for n_rows > 2^31, for a NULL or 4-B misaligned d_digests with
 * n_rows > 0 and for a d_rows that is not 8-B aligned. */
int sf_wire_get_blocks_device(const void *d_digests /* n_rows x 20 B: 4-B aligned */,
                              const int64_t *d_rows /* may be NULL */, const uint8_t *d_take /* may be NULL */,
                              uint64_t n_rows, int distinct, sf_wire_run **out, uint64_t *n_requests,
                              void *stream);

/* The sink's GetBlocks state (fs.rs:503-516) for a whole parsed run, as one
 * join.  Rows: the destination's incomplete rows in rowid order --
 * d_row_digests (20 B each, 4-B aligned), d_row_sizes, d_row_dst[r] = where
 * row r's block lies in the image allocation (its file's base plus its
 * offset; 8-B aligned), d_row_present[r] (bytes; 0 = the row still waits).
 * Messages: exactly the outputs of sf_receive_block_data_device, d_msg_ok its
 * d_ok (NULL: all ok, an unverified run).
 *
 * For a waiting row r, m = the lowest-numbered ok message whose digest is the
 * row's (sf_block_set_build over the messages, a lookup of the row digests).
 * When d_msg_sizes[m] == d_row_sizes[r] the row yields a job; jobs are
 * numbered in row order, and job k is d_src_offsets[k] =
 * d_msg_data_offsets[m], d_dst_offsets[k] = d_row_dst[r], d_sizes[k],
 * d_job_rows[k] = r, d_job_msgs[k] = m; d_row_present[r] becomes 1 and
 * d_msg_uses[m] (may be NULL; n_msgs entries, all written: 0 for a message no
 * row wants) counts it.  When the sizes differ the row stays missing and
 * *n_size_mismatch counts it.  That is stricter than the reference, which
 * writes the payload whatever the row says; it is what makes the jobs'
 * destinations disjoint whenever the rows' own ranges are -- rows tile their
 * files -- so the first *n_jobs entries of the three lists are ONE
 * sf_copy_blocks_device call, with no sort.  *n_left = the rows still 0
 * afterwards (what check_temp_files asks for).
 *
 * For a verified run equal digests mean equal payloads, so the image is the
 * reference's: every payload at every location, the later write winning.  In
 * an unverified run that carries two different payloads under one digest the
 * FIRST is taken here; the reference keeps the last.
 *
 * SF_ENOSPC with *n_jobs = the need when the jobs exceed cap or one of the
 * five job lists is NULL (a query): then nothing is marked, no job and no
 * d_msg_uses entry is written, and *n_left counts the rows that wait now.
 * One lane per row classes it, the waiting rows and the mismatches are
 * counted with one atomic per wave, a uint64 scan numbers the jobs, the three
 * counts come back in one 24-byte copy (the call blocks there, once), and one
 * lane per row writes its job.  Scratch: 17 n_rows bytes plus the set's (16
 * to 32 per message) and the scan's.  n_rows == 0 launches nothing but the
 * clearing of d_msg_uses; n_msgs == 0 nothing but the count for *n_left.
 * SF_EINVAL, before any device call, for a NULL n_jobs, n_left or
 * n_size_mismatch, for a count above 2^31, for a NULL row list with
 * n_rows > 0 or message list with n_msgs > 0, and for a misaligned list (4 B
 * for digests, sizes and d_msg_uses, 8 B for the 64-bit lists).  Blocking. */
int sf_place_block_data_device(const void *d_row_digests, const uint32_t *d_row_sizes, const uint64_t *d_row_dst,
                               uint8_t *d_row_present /* in/out */, uint64_t n_rows,
                               const void *d_msg_digests, const uint32_t *d_msg_sizes,
                               const uint64_t *d_msg_data_offsets, const uint8_t *d_msg_ok /* NULL: all */,
                               uint64_t n_msgs, uint64_t *d_src_offsets, uint64_t *d_dst_offsets,
                               uint32_t *d_sizes, int64_t *d_job_rows, int64_t *d_job_msgs, uint64_t cap,
                               uint32_t *d_msg_uses /* may be NULL */, uint64_t *n_jobs, uint64_t *n_left,
                               uint64_t *n_size_mismatch, void *stream);

/* --------------------------- assembling the incoming files, on the device ---- */

/* What the two sink states exist for: every block the destination already
 * holds is read from its local file and written into the incoming one
 * (read_block + write_block, src/sync/fs.rs:463-470), every received payload
 * is written to each location that wants it (fs.rs:505-510).  Here a whole
 * copy or write list is carried out in one launch, from HBM to HBM: d_src is
 * the received run (or a local file's bytes), d_dst the image of the incoming
 * files.
 *
 * dst[d_dst_offsets[i], +d_sizes[i]) = src[d_src_offsets[i], +d_sizes[i]) for
 * every i in [0, n_blocks) with d_take[i] != 0 (d_take NULL: all) -- the d_ok
 * of sf_receive_block_data_device goes straight in when jobs and messages are
 * one to one.  Sizes are any uint32 (0: nothing is written), offsets any
 * uint64; neither buffer nor any offset needs an alignment.  Source ranges may
 * overlap or repeat.  The DESTINATION RANGES OF THE TAKEN JOBS MUST BE
 * DISJOINT: jobs are written concurrently, and where two overlap each byte
 * there comes from one of them, unspecified which.  Ranges that abut byte to
 * byte are fine: no store touches a byte outside its own job's range (edges
 * are byte stores, everything between 16-byte stores aligned in the
 * destination), and no load leaves [d_src, d_src + src_len).
 *
 * A taken job whose source does not lie in [0, src_len) or whose destination
 * does not lie in [0, dst_len) (offset + size past 2^64 included) is not
 * copied and *d_status (a device int32 the caller initialised to 0, may be
 * NULL; the convention of sf_index_device_blocks) is set to SF_ERANGE; every
 * other job is still copied exactly.
 *
 * Work is split by bytes, not jobs (tiles of 4 KiB of the destination, found
 * through a uint64 scan of per-job tile counts; sf_copy.hip),
 * the grid is sized from the device's CU count and nothing is read back:
 * asynchronous on `stream`.  Scratch: 8 (n_blocks + 1) bytes plus the scan's,
 * from the library's stream-ordered pool; the first call on a device also
 * allocates 256 bytes of counters that are kept (sf_test_copy_stats reads
 * them).  n_blocks == 0 launches nothing.
 * SF_EINVAL, before any device call, for a NULL list or buffer with
 * n_blocks > 0, for n_blocks > 2^32, when [d_src, +src_len) and
 * [d_dst, +dst_len) overlap, and for a d_status that is not 4-B aligned. */
int sf_copy_blocks_device(const void *d_src, uint64_t src_len, void *d_dst, uint64_t dst_len,
                          const uint64_t *d_src_offsets, const uint64_t *d_dst_offsets,
                          const uint32_t *d_sizes, const uint8_t *d_take /* NULL: all */,
                          uint64_t n_blocks, int *d_status /* may be NULL */, void *stream);

/* d_data[0, len) written at file_offset of fd with pwrite (the position is
 * not used or moved): the way of a finished image to its temp file, before
 * the rename of fs.rs:529-548.  The bytes come back in stages (64 MiB) by DMA
 * into pinned buffers, after what `stream` holds at the call; stage k is
 * copied while stage k - 2 is written in slices by the library's reader
 * threads.  *n_written (may be NULL) = the bytes of the whole stages known
 * written.  SF_EIO on a failed or short write, SF_EINVAL for fd < 0, a
 * descriptor that cannot seek (a pipe: pwrite's ESPIPE) or a NULL d_data with
 * len > 0.  Blocking. */
int sf_write_device_fd(const void *d_data, uint64_t len, int fd, uint64_t file_offset,
                       uint64_t *n_written, void *stream);

/* The local half of the GetFiles state in one call: the outputs of
 * sf_receive_files_device become the copy list sf_copy_blocks_device takes and
 * the row arrays sf_wire_get_blocks_device (d_ask is its d_take) and
 * sf_place_block_data_device (d_present, d_dst are its d_row_present,
 * d_row_dst) take, with no host pass over the blocks.  The reference copies
 * every block get_block finds, on trust (read_block + write_block,
 * fs.rs:463-470); here a local block is hashed and compared with the digest
 * the source announced before it is used, so a file edited after it was
 * indexed costs a request, not a wrong image.
 *
 * Blocks (n_blocks entries each, as sf_receive_files_device wrote them):
 * d_digests, d_sizes, d_offsets, d_rows and d_block_file; d_file_base[f] is
 * where byte 0 of section f lies in the image allocation.  The table the block
 * set was built from, in rowid order (n_table entries each): d_table_file[r]
 * the local file that holds row r, in the caller's numbering, d_table_offset[r]
 * and d_table_size[r] the row's place in it.  Local files (n_local entries
 * each): d_local_size[j] the file's size now, d_local_base[j] where its byte 0
 * lies in the arena d_src[0, src_len), or UINT64_MAX for a file that is not
 * loaded.
 *
 * Block i with r = d_rows[i] and j = d_table_file[r] gets the first class that
 * applies:
 *   missing        r < 0
 *   size mismatch  d_table_size[r] != d_sizes[i] (the reference would copy the
 *                  chunk it cuts again at that offset; a job longer than its
 *                  block would overlap the next block's range)
 *   stale          d_table_offset[r] + d_sizes[i] > d_local_size[j]
 *   unavailable    d_local_base[j] == UINT64_MAX
 *   empty          d_sizes[i] == 0: present, and no job
 *   candidate      everything else.
 * With d_src the candidates' bytes, d_src[d_local_base[j] + d_table_offset[r],
 * + d_sizes[i]), are hashed by the explicit-list kernel, as a list of the
 * candidates alone; a candidate whose digest is d_digests[20 i, + 20) is a
 * job, any other is unverified.  With d_src NULL every candidate is a job.
 *
 * For every block: d_dst[i] = d_file_base[d_block_file[i]] + d_offsets[i],
 * d_present[i] = 1 for a job and an empty block, else 0, d_ask[i] =
 * !d_present[i].  The jobs, numbered in block order: d_src_offsets[k],
 * d_dst_offsets[k], d_job_sizes[k] and d_job_blocks[k] = i.  Blocks tile their
 * sections, so the first counts[SF_PLAN_JOBS] entries are one
 * sf_copy_blocks_device call with no sort.  d_local_jobs[j] (may be NULL) =
 * the jobs that read local file j.  counts (host, SF_PLAN_COUNTS entries):
 * the SF_PLAN_* numbers below.
 *
 * A query -- d_local_base or one of the four job lists NULL -- and a call
 * whose cap is below the job count return SF_ENOSPC with counts filled and
 * d_local_jobs written, and nothing else of the caller's is written (the
 * per-block outputs may be NULL in a query).  d_local_jobs is the query's
 * answer: which local files to load.  With d_local_base NULL no file is
 * unavailable and nothing is verified: a candidate counts as a job.
 *
 * SF_ERANGE, with nothing written and counts untouched, when any block has
 * r >= n_table, d_table_file[r] >= n_local, d_block_file[i] >= n_files, a
 * destination sum past 2^64 - 1 or, with d_src, a candidate outside
 * [0, src_len).  SF_EINVAL, before any device call, for a NULL input list
 * with entries to read, a NULL per-block output outside a query, a list off
 * its alignment (4 B: d_digests, d_sizes, d_block_file, d_table_file,
 * d_table_size, d_job_sizes, d_local_jobs; 8 B: the 64-bit lists), a count
 * above 2^31 or a NULL counts.  n_blocks == 0 launches nothing but the
 * clearing of d_local_jobs (no device call at all when that is NULL).
 *
 * Blocking: one read-back without verification (the candidate count), two
 * with it (then the job count).  Scratch: 9 n_blocks bytes, 32 per candidate
 * and the scan's, from the library's stream-ordered pool (sf_plan_copies.hip,
 * DESIGN.md 3.18). */
#define SF_PLAN_JOBS 0          /* blocks copied from local files */
#define SF_PLAN_BYTES 1         /* their bytes */
#define SF_PLAN_MISSING 2
#define SF_PLAN_SIZE_MISMATCH 3
#define SF_PLAN_STALE 4
#define SF_PLAN_UNAVAILABLE 5
#define SF_PLAN_UNVERIFIED 6
#define SF_PLAN_EMPTY 7
#define SF_PLAN_COUNTS 8
int sf_plan_copies_device(const void *d_digests /* 4-B aligned */, const uint32_t *d_sizes,
                          const uint64_t *d_offsets, const int64_t *d_rows, const uint32_t *d_block_file,
                          uint64_t n_blocks, const uint64_t *d_file_base, uint64_t n_files,
                          const uint32_t *d_table_file, const uint64_t *d_table_offset,
                          const uint32_t *d_table_size, uint64_t n_table,
                          const uint64_t *d_local_base /* NULL: a query */, const uint64_t *d_local_size,
                          uint64_t n_local, const void *d_src /* NULL: no verification */, uint64_t src_len,
                          uint8_t *d_present, uint8_t *d_ask, uint64_t *d_dst, uint64_t *d_src_offsets,
                          uint64_t *d_dst_offsets, uint32_t *d_job_sizes, int64_t *d_job_blocks, uint64_t cap,
                          uint32_t *d_local_jobs /* may be NULL */,
                          uint64_t *counts /* host: SF_PLAN_COUNTS entries */, void *stream);

/* Deterministic synthetic input (bench / tests): bytes [start, start+len)
 * of the splitmix64 stream with this seed.  d_out needs no
 * alignment (16-B stores when d_out and start are 16-B aligned, else bytes). */
int sf_fill_splitmix_device(void *d_out, uint64_t len, uint64_t seed, uint64_t start, void *stream);

/* ------------------------------------------------ host-memory entries */


/* End to end from host memory: H2D in pipelined chunks, fixed-tiling kernel,
 * D2H of the signature rows.  Blocking.  out has cap rows. */
int sf_index_buffer(const uint8_t *data, uint64_t len, uint32_t block_size,
                    sf_block_sig *out, uint64_t cap, uint64_t *n_out);

/* End to end from host memory with an explicit block list: block i =
 * data[offsets[i], offsets[i] + sizes[i]) -- the boundaries a chunker on the
 * host produced (the reference's default is cdchunking's ZPAQ,
 * src/index.rs:622-625: a Rust caller keeps that crate, runs it over the
 * file's bytes and hands the bytes + boundaries here).  Replaces the
 * Sha1::update / digest loop of src/index.rs:628-644 for every block.
 * Blocks must be in non-decreasing offset order (a chunker's output; they
 * may overlap and need not cover the buffer); sizes may be 0 (SHA-1 of no
 * bytes).  The list is checked before anything runs: SF_ERANGE if a block
 * passes len, SF_EINVAL if the offsets go backwards.  Stages of about
 * 256 MiB of whole blocks are copied (16 threads) into pinned buffers, moved
 * to HBM with their part of the list and hashed by the explicit-list kernel
 * while the next stage is copied.  out[i] = {offsets[i], sizes[i], digest};
 * blocks_hash (may be NULL) = SHA-1 over the digests in list order
 * (compute_blocks_hash, src/index.rs:661-682).  n_blocks rows; blocking. */
int sf_index_buffer_blocks(const uint8_t *data, uint64_t len, const uint64_t *offsets,
                           const uint32_t *sizes, uint64_t n_blocks, sf_block_sig *out,
                           uint8_t blocks_hash[SF_HASH_DIGEST_LEN]);

/* The same list over a regular file on disk: the caller's chunker streamed
 * the file once to find the boundaries (cdchunking's stream(file),
 * src/index.rs:625), and the library reads each ~256 MiB window again with
 * pread (16 threads) into the pinned stages -- the file is never held whole
 * in memory.  List checked against the file's size first (SF_ERANGE /
 * SF_EINVAL as above); SF_EIO if it cannot be opened or is not a regular
 * file; SF_EAGAIN if it changes while being read (stamps as in
 * sf_index_fd_blocks).  Rows in list order + blocks_hash; blocking.
 * The path is opened a second time here, after the chunker's open: a file
 * renamed over the path in between is hashed with the old file's
 * boundaries.  The drop-in splice uses sf_index_fd_blocks on the chunker's
 * own descriptor instead. */
int sf_index_file_blocks(const char *path, const uint64_t *offsets, const uint32_t *sizes,
                         uint64_t n_blocks, sf_block_sig *out, uint8_t blocks_hash[SF_HASH_DIGEST_LEN]);

/* What fstat says about an open file's contents: the identity of the bytes a
 * chunker read through that descriptor.  Two stamps match when dev, ino,
 * size and mtime are equal and, unless the link count changed, ctime too:
 * ctime moves on every write and cannot be set back by the writer (mtime
 * can), but it also moves when a link is added or removed -- a file renamed
 * over the path unlinks the open one, which changes nothing it holds.
 * Timestamps are only as fine as the filesystem's clock tick: a write within
 * the same tick as the stamp is not seen. */
typedef struct sf_file_stamp {
    uint64_t dev, ino, size, nlink;
    int64_t mtime_sec, mtime_nsec;
    int64_t ctime_sec, ctime_nsec;
} sf_file_stamp;

/* fstat(fd) as a stamp.  SF_EIO if fstat fails. */
int sf_file_stamp_fd(int fd, sf_file_stamp *out);

/* The loader of the destination's local files, the twin of
 * sf_write_device_fd: bytes [file_offset, + len) of fd go to d_dst[0, len).
 * They are read with pread (the position is not used or moved), in slices by
 * the library's reader threads, into two pinned stages (64 MiB) and copied to
 * the device stage by stage on `stream`, after what it holds at the call;
 * stage k is read while stage k - 1 is copied.  *n_read (may be NULL) = the
 * bytes of the whole stages known copied.  `expect` (may be NULL) is the stamp
 * the caller took of the file: SF_EAGAIN when the file's stamp is another
 * before the read or has moved after it -- d_dst[0, len) is then unspecified,
 * and nothing outside it is touched.  SF_EIO for a file shorter than
 * file_offset + len, SF_EINVAL, before any device call, for fd < 0, a
 * descriptor that cannot seek (a pipe) or a NULL d_dst with len > 0.
 * Blocking; launches no kernel. */
int sf_read_fd_device(int fd, const sf_file_stamp *expect /* may be NULL */, uint64_t file_offset,
                      uint64_t len, void *d_dst, uint64_t *n_read /* may be NULL */, void *stream);

/* The explicit list over the regular file OPEN on fd -- the handle the caller's
 * chunker just streamed (index_file opens the file once and takes the mtime,
 * the boundaries and the bytes from that one handle, src/index.rs:615-625).
 * Reads with pread only (the descriptor's position is not used or moved), by
 * ~256 MiB windows as sf_index_file_blocks.  A rename over the path after the
 * open changes nothing: the descriptor still reads the file the chunker cut.
 * expect (may be NULL): the stamp taken before the chunker read the file
 * (sf_file_stamp_fd); if the file's stamp differs when the call starts, or
 * changes between then and the last window read (an in-place write, append
 * or truncation), the call returns SF_EAGAIN and the rows are not valid: the
 * caller takes a new stamp and cuts the file again.  SF_EINVAL if fd is not a
 * regular file (a pipe cannot be read twice: use sf_index_buffer_blocks);
 * SF_ERANGE / SF_EINVAL for the list as sf_index_file_blocks.  Blocking. */
int sf_index_fd_blocks(int fd, const sf_file_stamp *expect, const uint64_t *offsets, const uint32_t *sizes,
                       uint64_t n_blocks, sf_block_sig *out, uint8_t blocks_hash[SF_HASH_DIGEST_LEN]);

/* Fixed tiling of the regular file open on fd, [0, size at the call), through
 * the pread pipeline of sf_index_file, with the same stamp checks as
 * sf_index_fd_blocks (SF_EAGAIN: the file changed; the rows are not valid).
 * SF_ENOSPC with *n_out = the need when cap is too small (nothing is read).
 * SF_EINVAL if fd is not a regular file (use sf_index_fd).  Blocking. */
int sf_index_fd_fixed(int fd, const sf_file_stamp *expect, uint32_t block_size, sf_block_sig *out,
                      uint64_t cap, uint64_t *n_out, uint8_t blocks_hash[SF_HASH_DIGEST_LEN]);

/* End to end from a file on disk (the reference's input, src/index.rs:615):
 * pread into pinned buffers, overlapped H2D + kernel, D2H.  Writes the
 * rows and the file's blocks_hash.  Blocking.  A path that cannot seek (FIFO,
 * socket, character device) is read sequentially to EOF like File::open +
 * read (src/index.rs:615,625); its input is consumed, so when the rows
 * exceed cap the call returns SF_ENOSPC with *n_out = the need and the rows
 * are lost -- use sf_index_fd for such inputs. */
int sf_index_file(const char *path, uint32_t block_size, sf_block_sig *out, uint64_t cap,
                  uint64_t *n_out, uint8_t blocks_hash[SF_HASH_DIGEST_LEN]);

/* One shard of a file on disk: bytes [start, start+len) of a regular file
 * (start a multiple of block_size unless len == 0; the shard's last block
 * may be short only where the file ends), through the same pread pipeline
 * as sf_index_file.
 * Row offsets are FILE offsets, so the shards' rows concatenated in order
 * are the file's rows (src/index.rs:629-656).  No blocks_hash: it chains
 * over every digest of the file, so the rank that gathers the shards'
 * digests computes it (sf_blocks_hash).  SF_ERANGE if the range passes the
 * end of the file.  Blocking. */
int sf_index_file_range(const char *path, uint64_t start, uint64_t len, uint32_t block_size,
                        sf_block_sig *out, uint64_t cap, uint64_t *n_out);

/* Sequential input from an open file descriptor (pipe, FIFO, socket, or a
 * file read from its current position), read to EOF: the rows of its fixed
 * tiling, offsets from the first byte read, in a buffer the library
 * allocates and grows (*rows; release it with sf_free_rows), and its
 * blocks_hash.  Pinned double-buffered stages, each copied and hashed on
 * the device while the next is read.  Does not close fd.  Blocking. */
int sf_index_fd(int fd, uint32_t block_size, sf_block_sig **rows, uint64_t *n_out,
                uint8_t blocks_hash[SF_HASH_DIGEST_LEN]);
void sf_free_rows(sf_block_sig *rows);

/* Many files from disk: what index_path (src/index.rs:685-715) does by calling
 * index_file (src/index.rs:610-659) once per file, as ONE pipeline.  Fixed
 * tiling of every file.  Files are packed at 16-B aligned offsets into pinned
 * stages of about stage_bytes (0 = 256 MiB) by a pool of pread threads; each
 * stage is copied to HBM and hashed (blocks + every file's blocks_hash,
 * src/index.rs:661-682) while the next stage is read.  A file larger than a
 * stage goes through the one-file pipeline of sf_index_file.
 * out: the rows of file 0, then file 1, ... (offsets relative to each file);
 * first_row (n_files+1 entries): where each file's rows start;
 * blocks_hashes: 20 B per file.  *n_out = total rows (the need, with
 * SF_ENOSPC, checked before any file is read).  On SF_EIO (open, stat or a
 * short read: the file changed while being indexed) *bad_file (may be NULL)
 * is the index of the failing file.  Each stage's blocks and blocks_hash
 * chains go through sf_index_device_batch.  Blocking. */
int sf_index_files(const char *const *paths, uint32_t n_files, uint32_t block_size, uint64_t stage_bytes,
                   sf_block_sig *out, uint64_t cap, uint64_t *first_row, uint8_t *blocks_hashes,
                   uint64_t *n_out, uint32_t *bad_file);

/* Many files in the reference's default mode: what index_path
 * (src/index.rs:685-715) does with one index_file (src/index.rs:610-659) per
 * file, each file cut by the caller's chunker (cdchunking's ZPAQ,
 * src/index.rs:622-625) on its own open descriptor, as ONE pipeline.  File f
 * is the regular file open on fds[f]; stamps[f] (stamps may be NULL) its
 * sf_file_stamp_fd taken before the chunker read it; its list is block i =
 * [offsets[f][i], offsets[f][i] + sizes[f][i]) for i < n_blocks[f],
 * offset-ordered (a chunker's output).  The files are read again with pread
 * only (the descriptors' positions are not used or moved), by windows packed
 * into pinned stages of about stage_bytes (0 = 256 MiB; a window of one
 * larger block is a stage of its own) by a pool of reader threads; per stage
 * one H2D copy, one length-class sort + one explicit-list kernel launch over
 * every block of every file in it, one D2H, overlapped with the reading of
 * the next stage.  out: file 0's rows, then file 1's, ... (offsets relative
 * to each file); first_row (n_files + 1 entries): where each file's rows
 * start (written first, from n_blocks); blocks_hashes: 20 B per file,
 * compute_blocks_hash (src/index.rs:661-682) over its digests in list order
 * (SHA1("") for a file with no blocks).  SF_ENOSPC (nothing read) when cap <
 * first_row[n_files].  Each file succeeds or fails alone: file_status (may be
 * NULL, n_files entries) receives SF_OK or, for that file, SF_EAGAIN (its
 * stamp differs from stamps[f] at the call, or moved before its last window
 * was read: cut it again), SF_ERANGE / SF_EINVAL (its list: past the end of
 * the file / offsets going backwards), SF_EINVAL (fds[f] is not an open
 * regular file), SF_EIO (fstat or a read failed); a failed file's rows are not
 * valid and its blocks_hash is zeroed, every other file's are complete.  The
 * call returns SF_OK, or the first failing file's code with *bad_file (may be
 * NULL) = its index; a device error fails the whole call.  Blocking. */
int sf_index_fds_blocks(const int *fds, const sf_file_stamp *stamps, uint32_t n_files,
                        const uint64_t *const *offsets, const uint32_t *const *sizes, const uint64_t *n_blocks,
                        uint64_t stage_bytes, sf_block_sig *out, uint64_t cap, uint64_t *first_row,
                        uint8_t *blocks_hashes, int *file_status, uint32_t *bad_file);

/* -------------------------------- the caller's chunker, on N threads ---- */

/* A content-defined chunker of the caller's (cdchunking's ZPAQ with its
 * max_size cap, src/index.rs:622-625, on the Rust side), as three functions:
 *   create(ctx)       a fresh chunker: the state at a chunk's first byte;
 *   next(ch, p, n)    feeds p[0, n): the number of bytes up to and including
 *                     the next boundary, or 0 if the chunk goes on past p + n;
 *                     after a boundary the state is a fresh chunk's again;
 *   destroy(ch).
 * The chunker must restart at every boundary (its state after a boundary is a
 * fresh chunker's, which read_block relies on, src/sync/fs.rs:26-40): then
 * the boundaries are a function of where a chunk starts, which is what lets
 * sf_cut_fd cut one file on several threads and still return exactly the
 * sequential boundaries.  Called from the library's threads, one chunker
 * per thread at a time. */
typedef struct sf_chunker_ops {
    void *(*create)(void *ctx);
    size_t (*next)(void *chunker, const uint8_t *p, size_t n);
    void (*destroy)(void *chunker);
    void *ctx;
} sf_chunker_ops;

/* The boundaries of the regular file open on fd (pread only; the position is
 * not used), cut by `ops`, exactly as one chunker streaming the file from its
 * first byte would cut it (the loop of src/index.rs:629-647 without the
 * SHA-1).  With threads > 1 (0 = the library's reader count) the file is
 * split into up to `threads` segments of at least 4 MiB (a file under 8 MiB is
 * cut on one thread); a chunker starts
 * fresh at each segment's first byte and cuts speculatively; the segments are
 * then joined left to right: from the last boundary known to be right, the
 * file is cut again on one thread only until a boundary coincides with one of
 * the next segment's, after which (the chunker restarting at every boundary)
 * the two agree.  The result never depends on the thread count.  *offsets /
 * *sizes (n_blocks entries; allocated by the library, release both with
 * sf_free_cuts) are the blocks in file order; an empty file has none.
 * expect (may be NULL): the caller's sf_file_stamp_fd; the file's stamp is
 * compared with it at the start and with the one taken at the start after the
 * last read: SF_EAGAIN if it changed (cut it again).  SF_EINVAL if fd is not
 * a regular file or ops is incomplete, SF_EIO on a failed or short read,
 * SF_ENOMEM.  Host only (no device).  Blocking. */
int sf_cut_fd(int fd, const sf_file_stamp *expect, const sf_chunker_ops *ops, uint32_t threads,
              uint64_t **offsets, uint32_t **sizes, uint64_t *n_blocks);
void sf_free_cuts(void *p);

/* index_file (src/index.rs:610-659) in the default mode for one regular file
 * open on fd, with the caller's chunker on several threads: the boundaries
 * of sf_cut_fd (exactly the one-stream ones) and every block's SHA-1 and the
 * blocks_hash on the device, with the file read ONCE: each segment is read
 * into a pinned copy of the file by the thread that cuts it, copied to HBM
 * while the segments are cut and joined, and the joined list is hashed from
 * there -- by windows of up to 512 MiB, each ending at the last boundary
 * inside it (the next window starts there).  *rows (n_out entries, allocated by
 * the library, release with sf_free_rows) and blocks_hash as sf_index_fd_blocks
 * gives them.  expect / SF_EAGAIN / errors as sf_cut_fd.  Blocking. */
int sf_index_fd_cut(int fd, const sf_file_stamp *expect, const sf_chunker_ops *ops, uint32_t threads,
                    sf_block_sig **rows, uint64_t *n_out, uint8_t blocks_hash[SF_HASH_DIGEST_LEN]);

/* ------------------- the reference's chunker itself: host and device ---- */

/* cdchunking's ZPAQ chunker as index_file configures it (src/index.rs:622-625:
 * bits = 13, max_size = 32768), in the library.  Per input byte b, with h
 * (32 bits), c1 (the previous byte) and o1[256] (the byte that last followed
 * each byte):  h = h * (b == o1[c1] ? M : 2 * M) + b + 1, M = 123456791;
 * o1[c1] = b; c1 = b;  the chunk ends AFTER b when h < 2^(32 - bits) or its
 * length reaches max_size.  A chunk starts with h = M, c1 = 0, o1 all 0, and
 * the state is that again after every cut.  This reproduces the reference's
 * known-answer test (src/index.rs:761-792) exactly; the restart at a cut is
 * the one point that test does not pin.
 *
 * sf_zpaq_cut_buffer: the blocks of data[0, len), sequentially, on the calling
 * thread -- the library's definition of the boundaries; every other route
 * (sf_cut_fd over the ops below, the device cutter) returns exactly this
 * list.  offsets / sizes: cap entries; *n_blocks = the count (the need, with
 * SF_ENOSPC and the first cap rows written, when cap is too small or the
 * arrays are NULL).  The last block ends at len; len == 0 gives 0 blocks.
 * SF_EINVAL unless 1 <= bits <= 31 and max_size >= 1.  Host only. */
int sf_zpaq_cut_buffer(const uint8_t *data, uint64_t len, uint32_t bits, uint32_t max_size,
                       uint64_t *offsets, uint32_t *sizes, uint64_t cap, uint64_t *n_blocks);

/* The same chunker as an sf_chunker_ops: with it sf_cut_fd, sf_index_fd_cut
 * and (per file) sf_index_fds_blocks produce the reference's boundaries on N
 * host threads, and a Rust caller needs no chunker of its own.  The
 * parameters are carried in out->ctx itself (packed into the pointer's value:
 * nothing is allocated, there is nothing to release, and the struct may be
 * copied freely); each create() allocates one chunker state, freed by
 * destroy().  SF_EINVAL as above. */
int sf_zpaq_chunker_ops(uint32_t bits, uint32_t max_size, sf_chunker_ops *out);

/* The same boundaries for bytes already in HBM, cut on the device: blocks of
 * d_data[0, len) as (d_offsets uint64, d_sizes uint32) in file order --
 * exactly the list sf_index_device_blocks takes -- with the last block ending
 * at len.  The buffer is cut speculatively in segments (one lane each) whose
 * lists are then joined in rounds, each a kernel (sf_cdc.hip); the result is
 * sf_zpaq_cut_buffer's for any input.  BLOCKING: `stream` is synchronised
 * once per join round and once for the count.  Random or text-like data
 * joins in 1-3 rounds; constant or periodic data needs one round per segment
 * (segments are lcm(max_size, 32) bytes) and is cut at the speed of a single
 * lane -- still exact.  d_data needs no alignment.  *n_blocks = the count;
 * SF_ENOSPC (nothing written) when cap_blocks is smaller or an output is NULL.
 * len == 0 gives 0 blocks.  SF_EINVAL unless 1 <= bits <= 31 and
 * 16 <= max_size <= 1048576 (the device range).  d_offsets: 8-B aligned;
 * d_sizes: 4-B aligned.  Scratch: len / 4 bytes plus
 * 56 bytes per segment, from the library's stream-ordered pool. */
int sf_cut_device_zpaq(const void *d_data, uint64_t len, uint32_t bits, uint32_t max_size,
                       uint64_t *d_offsets, uint32_t *d_sizes, uint64_t cap_blocks,
                       uint64_t *n_blocks, void *stream);

/* index_file's default mode (src/index.rs:621-656) for bytes already in HBM:
 * sf_cut_device_zpaq, then the explicit-list kernel over that list
 * (sf_index_device_blocks) into d_digests (cap_blocks x 20 B), then, if
 * blocks_hash (a HOST pointer, may be NULL) is given, the digests are copied
 * back and chained on the host (compute_blocks_hash, src/index.rs:661-682).
 * d_digests: 4-B aligned (32-bit stores); with SF_ENOSPC no digest is written
 * either.  Blocking as sf_cut_device_zpaq; errors as there. */
int sf_index_device_zpaq(const void *d_data, uint64_t len, uint32_t bits, uint32_t max_size,
                         uint64_t *d_offsets, uint32_t *d_sizes, void *d_digests, uint64_t cap_blocks,
                         uint64_t *n_blocks, uint8_t *blocks_hash, void *stream);

/* index_file in the default mode for one regular file open on fd, with no
 * host chunker at all: the file is read once (pread, the library's reader
 * threads) into pinned memory and copied to HBM by windows of up to 512 MiB;
 * each window is cut (sf_cut_device_zpaq) and hashed on the device.  A
 * non-final window's last block was closed by the window's end, so it is
 * dropped and the next window starts at its offset -- a true cut, so the rows
 * are exactly sf_index_fd_cut's with sf_zpaq_chunker_ops.  *rows (n_out
 * entries, release with sf_free_rows) and blocks_hash as there; expect,
 * SF_EAGAIN and the other errors as sf_cut_fd; bits / max_size as
 * sf_cut_device_zpaq.  Blocking. */
int sf_index_fd_zpaq(int fd, const sf_file_stamp *expect, uint32_t bits, uint32_t max_size,
                     sf_block_sig **rows, uint64_t *n_out, uint8_t blocks_hash[SF_HASH_DIGEST_LEN]);

/* sf_cut_device_zpaq over MANY files of one buffer in HBM, in one call: file f
 * is bytes d_data[file_offsets[f], + file_lens[f]) (HOST arrays of n_files
 * entries; files need no alignment and may abut, leave gaps or overlap), and
 * every file is cut from a fresh chunker, as a file of its own.  The rows of
 * all files come out in file order -- d_offsets are positions in d_data, so
 * the list is exactly what sf_index_device_blocks takes -- and
 * d_first_row[f] (n_files + 1 entries) is the row where file f starts.  The
 * segments of all files fill the lanes together (sf_cdc_files.hip): a batch of
 * small files is cut like one huge one, with no join across files.
 *
 * max_rounds bounds the join launches (0 = no bound).  A file that still cut
 * again in the last launch made is UNSETTLED: it has no rows
 * (d_first_row[f] == d_first_row[f + 1]), unsettled[f] = 1 (HOST, n_files
 * bytes, may be NULL; 0 for every other file) and *n_unsettled (may be NULL)
 * counts such files.  When the bound was reached these are exactly the files
 * that need at least max_rounds rounds (constant or periodic data: one round
 * per segment); when the joins ended by themselves there is none.  For every
 * settled file the rows minus file_offsets[f] are sf_zpaq_cut_buffer's list of
 * the file's bytes, for any input.
 *
 * BLOCKING: `stream` is synchronised once per join launch and once for the
 * count.  *n_blocks = the rows of the settled files; SF_ENOSPC (no device
 * output written) when cap_blocks is smaller or a device output is NULL.
 * n_files == 0, or every file empty: SF_OK, 0 blocks, d_first_row (when given)
 * all zeros.  SF_ERANGE with *bad_file (may be NULL) = the first file that does
 * not lie in d_data[0, data_len).  SF_EINVAL for bits / max_size outside
 * sf_cut_device_zpaq's range or a misaligned output: d_offsets and
 * d_first_row 8-B aligned, d_sizes 4-B aligned.  Both are returned before any
 * device call.  Scratch, from the library's stream-ordered pool: two bitmaps
 * of sum ceil(len_f / 32) words, 56 bytes per segment, 36 bytes per file. */
int sf_cut_device_zpaq_files(const void *d_data, uint64_t data_len, const uint64_t *file_offsets,
                             const uint64_t *file_lens, uint32_t n_files, uint32_t bits, uint32_t max_size,
                             uint32_t max_rounds, uint64_t *d_offsets, uint32_t *d_sizes, uint64_t cap_blocks,
                             uint64_t *d_first_row, uint64_t *n_blocks, uint8_t *unsettled,
                             uint32_t *n_unsettled, uint32_t *bad_file, void *stream);

/* The many-file form of sf_index_device_zpaq: sf_cut_device_zpaq_files, then
 * the explicit-list kernel over the whole list into d_digests
 * (cap_blocks x 20 B, 4-B aligned; with SF_ENOSPC no digest is written
 * either, and a NULL d_digests is SF_ENOSPC like any other missing output).
 * If blocks_hashes (HOST, 20 x n_files bytes, may be NULL) is given, the
 * digests are copied back and every file's blocks_hash is chained on the
 * host: SHA-1("") for a file with no blocks, 20 zero bytes for an unsettled
 * file.  Blocking and errors as sf_cut_device_zpaq_files. */
int sf_index_device_zpaq_files(const void *d_data, uint64_t data_len, const uint64_t *file_offsets,
                               const uint64_t *file_lens, uint32_t n_files, uint32_t bits, uint32_t max_size,
                               uint32_t max_rounds, uint64_t *d_offsets, uint32_t *d_sizes, void *d_digests,
                               uint64_t cap_blocks, uint64_t *d_first_row, uint64_t *n_blocks,
                               uint8_t *blocks_hashes, uint8_t *unsettled, uint32_t *n_unsettled,
                               uint32_t *bad_file, void *stream);

/* index_path's default mode (src/index.rs:685-715 over 610-659) for many
 * regular files open on fds[0 .. n_files), with no host chunker and no lists
 * handed in: sf_index_fds_blocks without its second read.  Each file is read
 * ONCE, with pread by the library's reader threads, into packed pinned stages
 * of about stage_bytes (0 = 256 MiB; each file at a 64-byte boundary of its
 * stage); per stage one H2D copy, one many-file cut
 * (sf_cut_device_zpaq_files, at most max_rounds join launches, 0 = no bound),
 * one explicit-list launch over every block of the stage and one D2H of list
 * and digests.  Stage k's copy and the first, largest part of its cut run
 * while stage k + 1 is read.  A file that did not settle under max_rounds is
 * finished inside the call: it is cut by the host cutter
 * (sf_zpaq_cut_buffer's code, on the reader threads, one file per thread) from
 * the stage's pinned bytes and hashed by a second launch over the same stage
 * in HBM -- the result is complete and exact whatever max_rounds is.  A file
 * larger than a stage goes through sf_index_fd_zpaq's windows, in its place in
 * the file order.
 *
 * *rows (allocated by the library, *n_out entries, release with sf_free_rows;
 * also set when the call returns a file's own failure) holds file 0's rows,
 * then file 1's, ...: file f's are [first_row[f], first_row[f + 1])
 * (n_files + 1 entries), offsets relative to the file.  blocks_hashes
 * (20 x n_files): every file's blocks_hash, SHA-1("") for an empty file.
 * stamps (may be NULL), file_status (may be NULL) and bad_file as in
 * sf_index_fds_blocks: each file succeeds or fails alone -- SF_EINVAL for a
 * descriptor that is not a regular file, SF_EAGAIN when its stamp differs from
 * stamps[f] or moved while it was read, SF_EIO -- a failed file has no rows
 * and a zeroed blocks_hash, and the call returns the first failing file's
 * code with *bad_file naming it.  SF_EINVAL for bits / max_size outside
 * sf_cut_device_zpaq's range.  n_files == 0 needs no device.  Blocking. */
int sf_index_fds_zpaq(const int *fds, const sf_file_stamp *stamps, uint32_t n_files, uint32_t bits,
                      uint32_t max_size, uint32_t max_rounds, uint64_t stage_bytes, sf_block_sig **rows,
                      uint64_t *n_out, uint64_t *first_row, uint8_t *blocks_hashes, int *file_status,
                      uint32_t *bad_file);

/* ------------------------------------------- one process, N devices ---- */

/* Contiguous, block-aligned shard `shard` of n_shards of a file_len-byte file:
 * bytes [*start, *start + *len).  Blocks are dealt as evenly as possible (the
 * first nblocks % n_shards shards get one more); a shard may be empty.  The
 * shards' rows concatenated in shard order are the file's rows.  The
 * partition every multi-device form below uses (and syncfast_amd.shard's
 * shard_range, one process per GPU). */
int sf_shard_range(uint64_t file_len, uint32_t block_size, uint32_t n_shards, uint32_t shard, uint64_t *start,
                   uint64_t *len);

/* index_file (src/index.rs:610-659) of one regular file on N devices of this
 * process: fixed tiling, shard r (sf_shard_range) read with pread from ONE
 * open of the file and hashed on device r by a host thread of its own (each
 * device on its own PCIe link, through the staged pipeline of sf_index_file),
 * rows written straight into out at the shard's first row; then blocks_hash
 * over every digest in order on the host (it chains over the whole file).
 * n_devices = 0: every visible device; devices 0 .. n_devices-1 are used.
 * The file is stamped at the open and again after the last read: SF_EAGAIN
 * if it changed (the rows are not valid).  SF_ENOSPC with *n_out = the need
 * when cap is too small (nothing read); SF_EINVAL if path is not a regular
 * file or n_devices exceeds the visible devices.  The calling thread's current
 * device is left as it was.  Blocking. */
int sf_index_file_multi(const char *path, uint32_t block_size, uint32_t n_devices, sf_block_sig *out, uint64_t cap,
                        uint64_t *n_out, uint8_t blocks_hash[SF_HASH_DIGEST_LEN]);

/* The device-resident form on N devices of this process, the gather over
 * xGMI inside the library: d_shards[r] (on device r) holds shard r
 * (sf_shard_range of file_len, block_size, n_devices) of one logical file;
 * each shard is hashed on its own device, on streams[r] (streams may be NULL:
 * each device's null stream), the root's straight into its rows of d_table
 * (device `root`, ceil(file_len / block_size) x 20 B), every other device's
 * into d_digests[r] (its own scratch, its shard's rows x 20 B) and from there
 * to its rows of d_table with RCCL (one communicator per device list,
 * ncclCommInitAll on first use, kept; grouped ncclSend / ncclRecv, since the
 * shards' row counts may differ by one).  Asynchronous: d_table is complete
 * once streams[root] has run past the call.  Devices 0 .. n_devices-1; the
 * caller's current device is left as it was.  SF_ENODEV if RCCL cannot be
 * loaded or a communicator not made. */
int sf_index_device_multi(uint32_t n_devices, const void *const *d_shards, uint64_t file_len, uint32_t block_size,
                          void *const *d_digests, uint32_t root, void *d_table, void *const *streams);

/* sf_index_device_multi with the exchange on streams of its own: shard r is
 * hashed on hash_streams[r] (NULL: each device's null stream) and sent -- and,
 * on the root, received -- on gather_streams[r], which first waits for device
 * r's hashing (an event the library records on hash_streams[r]; NULL
 * gather_streams: the hash streams, i.e. sf_index_device_multi).  A caller
 * indexing file after file (each file's table gathered to its owner, config
 * 4 of BASELINE.json over and over) can then hash file i+1 while file i's
 * tables are in flight: d_digests[r] may be written again, and d_table read,
 * once gather_streams[r] / gather_streams[root] have run past the call.
 * Errors as sf_index_device_multi. */
int sf_index_device_multi_ex(uint32_t n_devices, const void *const *d_shards, uint64_t file_len,
                             uint32_t block_size, void *const *d_digests, uint32_t root, void *d_table,
                             void *const *hash_streams, void *const *gather_streams);

/* compute_blocks_hash (src/index.rs:661-682) on the host: SHA-1 over the
 * n 20-byte digests in order.  Sequential by definition; runs on a host
 * core (SHA-NI when the CPU has it). */
int sf_blocks_hash(const uint8_t *digests, uint64_t n, uint8_t out[SF_HASH_DIGEST_LEN]);
int sf_blocks_hash_sigs(const sf_block_sig *sigs, uint64_t n, uint8_t out[SF_HASH_DIGEST_LEN]);

/* Host SHA-1 of an arbitrary byte range (the same function as the
 * reference's sha1 crate; used for blocks_hash and host-side checks). */
int sf_sha1_host(const uint8_t *data, uint64_t len, uint8_t out[SF_HASH_DIGEST_LEN]);

#ifdef __cplusplus
}
#endif

#endif /* SYNCFAST_AMD_H */
