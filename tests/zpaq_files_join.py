"""The join of the many-file device ZPAQ cut (syncfast_amd/csrc/
sf_cdc_files.hip), restated over tests/zpaq_join.restate applied per file.

Test helper: no GPU.  Every file of a batch is cut as a file of its own --
segments of different files never join -- so a batch's join is the per-file
joins side by side, in the same launches:

rounds_f   zpaq_join.restate(file).rounds: the rounds in which a segment of
           the file cuts again.  They are rounds 1 .. rounds_f without a gap (a
           segment can only change in round r + 1 if its predecessor changed
           in round r), so rounds_f is also the last launch that touches f.
launches   the join launches the host loop makes, as it counts them: none when
           no file has two segments; else one per round in which any file
           changes plus the one that finds nothing changed,
           max(rounds_f) + 1 -- or max_rounds, if that is smaller (0: no cap).
unsettled  the files that cut again in the last launch made: under a cap M
           those with rounds_f >= M; none when the loop ended by itself.
recut      the bytes cut again in all launches: the sum of the files' when no
           file is unsettled; None otherwise (a capped join stops part-way and
           this restatement does not say where).
rows       first_row[f] and the total, from the true lists of the settled
           files; an unsettled file has no rows.
"""
from collections import namedtuple

import zpaq_join as zj

FilesJoin = namedtuple("FilesJoin", "L segments rounds launches recut unsettled first_row true_ends")

# The batch of the many-file tests at (6, 256), L = 256: (name, content, length
# in bytes or None, rounds) -- tests/test_zpaq_files_join.py pins the rounds
# with the pure-Python chunker.
L_TABLE = 256


def table_files():
    """[(name, bytes, rounds)] of the table above."""
    import numpy as np
    L = L_TABLE

    def rnd(n):
        return np.random.default_rng(7).integers(0, 256, n, dtype=np.uint8).tobytes()
    return [("zeros-40L", bytes(40 * L), 39),
            ("zeros-12L+5", bytes(12 * L + 5), 12),
            ("period7-20L", (bytes(range(1, 8)) * (20 * L // 7 + 1))[:20 * L], 18),
            ("random-9.5L", rnd(9 * L + L // 2), 1),
            ("random-L", rnd(L), 0),
            ("random-L+1", rnd(L + 1), 1),
            ("islands", zj.islands(L, 3, pairs=3), 5)]


def restate_files(files, bits, max_size, max_rounds=0, ends=zj.host_ends):
    """FilesJoin of the batch `files` (a sequence of bytes objects)."""
    joins = [zj.restate(d, bits, max_size, ends=ends) for d in files]
    rounds = [j.rounds for j in joins]
    free = max(rounds) + 1 if any(j.nseg > 1 for j in joins) else 0
    launches = min(free, max_rounds) if max_rounds else free
    unsettled = [bool(max_rounds) and r >= max_rounds for r in rounds]
    first_row = [0]
    for j, u in zip(joins, unsettled):
        first_row.append(first_row[-1] + (0 if u else len(j.true_ends)))
    return FilesJoin(zj.segment_len(max_size), sum(j.nseg for j in joins), rounds, launches,
                     None if any(unsettled) else sum(j.recut for j in joins), unsettled, first_row,
                     [j.true_ends for j in joins])
