"""The join of the device ZPAQ cut (syncfast_amd/csrc/sf_cdc.hip), restated in
plain Python over the host cutter.

Test helper: no GPU.  Which way a segment's join goes -- no work, a sync
part-way, a walk to the segment's end -- depends on the bytes, not on
shapes, so a test that means to reach one of them asks here first and asserts
the answer before it calls the library; afterwards it holds the device's own
round and byte counters (sf_test_zpaq_device_stats) against the simulation.

What is restated, and where it stands in sf_cdc.hip's header:

segments  L = lcm(max_size, 32), nseg = ceil(len / L); segment s is bytes
          [s0, s1) = [s L, min(len, s L + L)) and owns the cuts ("a chunk ends
          after byte i", written here as the end offset i + 1) in (s0, s1].
round 0   every segment is cut from s0 with a fresh state: its speculative
          list.  Here: the host cut of data[s0 : s1 + 1], ends <= s1 kept --
          the extra byte keeps a block closed only by the slice's end from
          counting.  For the last segment the end at len counts (the last
          block ends at len in every list).  last[s] = the list's last cut, or
          s0 for an empty list; used[s] = s0.
join      one round reads last[] of the round before (double-buffered).
          Segment s >= 1 whose incoming cut last[s - 1] differs from used[s]
          cuts again from it with a fresh state (cuts at or before s0, the
          run-in, restart the chunker and are otherwise ignored) and stops at
          its first cut that is a round-0 cut of the segment: last[s] becomes
          the round-0 list's last cut.  If none coincides it stops at s1 and
          last[s] is its own last cut.  The bytes fed, run-in included, are
          added to `recut`.  The host repeats while a round changed a segment;
          `rounds` counts the rounds that did.
classes   from the true (sequential) list alone: segment s >= 1 is `aligned`
          when s0 is a true cut, `synced` when some true cut in (s0, s1] is a
          speculative cut of the segment, else `unsynced`.
"""
import math
import random
from collections import namedtuple

import numpy as np

from syncfast_amd import host

ALIGNED, SYNCED, UNSYNCED = "aligned", "synced", "unsynced"
PERIODS = (1, 2, 3, 7, 13, 32, 33)

Join = namedtuple("Join", "L nseg classes rounds recut true_ends spec")


def segment_len(max_size):
    return max_size // math.gcd(max_size, 32) * 32


def host_ends(data, bits, max_size):
    """End offsets of the host cutter's blocks of `data`, in order."""
    offs, sizes = host.zpaq_cut_buffer(data, bits, max_size)
    return (offs.astype(np.int64) + sizes.astype(np.int64)).tolist()


def islands(L, seed, pairs=6):
    """Stretches of random bytes, 0.5 L to 4 L long, alternating with
    stretches of a repeated pattern, 1 L to 6 L long, whose period is drawn
    from PERIODS; `pairs` of each."""
    rng = random.Random(seed)
    out = bytearray()
    for _ in range(pairs):
        out += rng.randbytes(rng.randint(L // 2, 4 * L))
        pattern = rng.randbytes(rng.choice(PERIODS))
        n = rng.randint(L, 6 * L)
        out += (pattern * (n // len(pattern) + 1))[:n]
    return bytes(out)


def longest_run(classes, what):
    best = run = 0
    for c in classes:
        run = run + 1 if c == what else 0
        best = max(best, run)
    return best


def restate(data, bits, max_size, ends=host_ends):
    """Join(L, nseg, classes, rounds, recut, true_ends, spec) of `data`:
    classes[s] for s >= 1 (classes[0] is None), spec[s] the speculative ends
    of segment s.  `ends(data, bits, max_size)` is the sequential cutter."""
    n = len(data)
    L = segment_len(max_size)
    nseg = -(-n // L)
    view = memoryview(data)

    def cut_from(a, s1):  # the cuts in (a, s1] of a chunker started fresh at a
        return [a + e for e in ends(view[a:min(s1 + 1, n)], bits, max_size) if a + e <= s1]

    bounds = [(s * L, min(n, s * L + L)) for s in range(nseg)]
    spec = [cut_from(s0, s1) for s0, s1 in bounds]
    true_ends = ends(view, bits, max_size)
    true_set = set(true_ends)
    classes = [None]
    for s in range(1, nseg):
        s0, s1 = bounds[s]
        if s0 in true_set:
            classes.append(ALIGNED)
        elif any(e in true_set for e in spec[s]):
            classes.append(SYNCED)
        else:
            classes.append(UNSYNCED)

    lastspec = [sp[-1] if sp else s0 for sp, (s0, _s1) in zip(spec, bounds)]
    last = list(lastspec)
    used = [s0 for s0, _s1 in bounds]
    spec_sets = [set(sp) for sp in spec]
    rounds = recut = 0
    while nseg > 1:
        out = list(last)
        changed = 0
        for s in range(1, nseg):
            inc = last[s - 1]
            if inc == used[s]:
                continue
            used[s] = inc
            changed += 1
            s0, s1 = bounds[s]
            lastcut, stop = inc, s1
            for e in cut_from(inc, s1):
                if e <= s0:
                    continue
                lastcut = e
                if e in spec_sets[s]:
                    lastcut, stop = lastspec[s], e
                    break
            recut += stop - inc
            out[s] = lastcut
        last = out
        if not changed:
            break
        rounds += 1
        assert rounds <= nseg
    return Join(L, nseg, classes, rounds, recut, true_ends, spec)
