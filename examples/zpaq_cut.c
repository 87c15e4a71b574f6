/* zpaq_cut.c -- the library's ZPAQ chunker from plain C, host only (no device,
 * no HIP): prints the reference's content-defined blocks of each file and
 * checks that the two host forms agree,
 *   sf_zpaq_cut_buffer   the whole buffer in one call, and
 *   sf_zpaq_chunker_ops  create / next / destroy, fed in odd-sized pieces
 *                        (how sf_cut_fd drives a chunker),
 * plus the capacity contract (SF_ENOSPC reports the need, nothing is written
 * past cap).  Built with the sanitizers by `make -C examples asan-zpaq`
 * (examples/build/asan/zpaq_cut: this file + syncfast_amd/csrc/sf_zpaq.cpp,
 * nothing else), which is how the host cutter runs under ASan + UBSan.
 *
 * usage: zpaq_cut [-b bits] [-m max_size] [-p piece_bytes] [file ...]
 *        (no file: built-in inputs -- pseudo-random, zeros, periodic)
 * output per input: "<name> <n_blocks> blocks", then "<offset> <size>" lines. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "syncfast_amd.h"

static int fail(const char *name, const char *what) {
    fprintf(stderr, "zpaq_cut: %s: %s\n", name, what);
    return 1;
}

static int run(const char *name, const uint8_t *data, uint64_t len, uint32_t bits, uint32_t max_size, size_t piece,
               int print) {
    uint64_t n = 0, need = 0;
    int rc = sf_zpaq_cut_buffer(data, len, bits, max_size, NULL, NULL, 0, &n); /* a query */
    if (rc != (n ? SF_ENOSPC : SF_OK)) return fail(name, "query failed");
    /* exact-size arrays: a write past cap is a heap overflow the sanitizer sees */
    uint64_t *offs = malloc((n ? n : 1) * sizeof *offs);
    uint32_t *sizes = malloc((n ? n : 1) * sizeof *sizes);
    if (!offs || !sizes) return fail(name, "out of memory");
    if (sf_zpaq_cut_buffer(data, len, bits, max_size, offs, sizes, n, &need) != SF_OK || need != n)
        return fail(name, "cut failed");
    if (n > 1) { /* one row too few: the need again, the first n - 1 rows written */
        uint64_t *o2 = malloc((n - 1) * sizeof *o2);
        uint32_t *s2 = malloc((n - 1) * sizeof *s2);
        if (!o2 || !s2) return fail(name, "out of memory");
        if (sf_zpaq_cut_buffer(data, len, bits, max_size, o2, s2, n - 1, &need) != SF_ENOSPC || need != n ||
            memcmp(o2, offs, (n - 1) * sizeof *o2) || memcmp(s2, sizes, (n - 1) * sizeof *s2))
            return fail(name, "capacity contract broken");
        free(o2);
        free(s2);
    }
    /* the same chunker through its three functions, in pieces */
    sf_chunker_ops ops;
    if (sf_zpaq_chunker_ops(bits, max_size, &ops) != SF_OK) return fail(name, "ops failed");
    void *ch = ops.create(ops.ctx);
    if (!ch) return fail(name, "create failed");
    uint64_t k = 0, start = 0, pos = 0;
    int bad = 0;
    while (pos < len && !bad) {
        size_t m = len - pos < piece ? (size_t)(len - pos) : piece;
        for (size_t q = 0; q < m;) {
            size_t c = ops.next(ch, data + pos + q, m - q);
            if (c == 0) break;
            q += c;
            if (k >= n || offs[k] != start || sizes[k] != pos + q - start) { bad = 1; break; }
            start = pos + q;
            k++;
        }
        pos += m;
    }
    ops.destroy(ch);
    if (!bad && start < len) { /* the last chunk ends with the data */
        bad = k >= n || offs[k] != start || sizes[k] != len - start;
        k++;
    }
    if (bad || k != n) return fail(name, "the ops and the buffer cut differ");
    printf("%s %llu blocks\n", name, (unsigned long long)n);
    for (uint64_t i = 0; print && i < n; i++)
        printf("%llu %u\n", (unsigned long long)offs[i], sizes[i]);
    free(offs);
    free(sizes);
    return 0;
}

int main(int argc, char **argv) {
    uint32_t bits = 13, max_size = 32768;
    size_t piece = 4099;
    int i = 1, rc = 0;
    for (; i + 1 < argc && argv[i][0] == '-'; i += 2) {
        if (!strcmp(argv[i], "-b")) bits = (uint32_t)strtoul(argv[i + 1], NULL, 10);
        else if (!strcmp(argv[i], "-m")) max_size = (uint32_t)strtoul(argv[i + 1], NULL, 10);
        else if (!strcmp(argv[i], "-p")) piece = (size_t)strtoull(argv[i + 1], NULL, 10);
        else break;
    }
    if (piece == 0) piece = 1;
    sf_chunker_ops none;
    uint64_t n = 0;
    if (sf_zpaq_chunker_ops(0, 1, &none) != SF_EINVAL || sf_zpaq_chunker_ops(32, 1, &none) != SF_EINVAL ||
        sf_zpaq_chunker_ops(13, 0, &none) != SF_EINVAL || sf_zpaq_cut_buffer(NULL, 0, 13, 0, NULL, NULL, 0, &n) != SF_EINVAL ||
        sf_zpaq_cut_buffer(NULL, 0, 13, 32768, NULL, NULL, 0, &n) != SF_OK || n != 0)
        return fail("arguments", "validation broken");
    if (i >= argc) { /* built-in inputs */
        const size_t len = 300000;
        uint8_t *buf = malloc(len);
        if (!buf) return fail("builtin", "out of memory");
        uint64_t x = 0x5EED;
        for (size_t j = 0; j < len; j++) {
            x += 0x9E3779B97F4A7C15ull;
            uint64_t z = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            buf[j] = (uint8_t)(z ^ (z >> 31));
        }
        const uint32_t params[][2] = {{bits, max_size}, {6, 256}, {1, 16}, {31, 4096}};
        for (size_t p = 0; p < sizeof params / sizeof params[0]; p++) {
            rc |= run("random", buf, len, params[p][0], params[p][1], piece, 0);
            rc |= run("random-odd", buf + 1, len - 3, params[p][0], params[p][1], 1, 0);
        }
        memset(buf, 0, len);
        rc |= run("zeros", buf, len, bits, max_size, piece, 0);
        for (size_t j = 0; j < len; j++) buf[j] = (uint8_t)"Test content\n"[j % 13];
        rc |= run("periodic", buf, len, bits, max_size, piece, 0);
        rc |= run("empty", buf, 0, bits, max_size, piece, 0);
        free(buf);
        return rc;
    }
    for (; i < argc; i++) {
        FILE *f = fopen(argv[i], "rb");
        if (!f) { rc |= fail(argv[i], "cannot open"); continue; }
        size_t cap = 1 << 20, len = 0, got;
        uint8_t *buf = malloc(cap);
        while (buf && (got = fread(buf + len, 1, cap - len, f)) > 0) {
            len += got;
            if (len == cap) buf = realloc(buf, cap *= 2);
        }
        fclose(f);
        if (!buf) return fail(argv[i], "out of memory");
        rc |= run(argv[i], buf, len, bits, max_size, piece, 1);
        free(buf);
    }
    return rc;
}
