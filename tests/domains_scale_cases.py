"""Crafted planes for `pileup -D` beyond one slice per carry thread, in plain numpy: build(u) for the scan unit u.

hm_pileup.hip's row scans work on SCAN_ROWS = 1024 rows per workgroup and ONE workgroup of 1024 threads scans the workgroups'
aggregates, each thread a contiguous slice of per = ceil(nagg / 1024) of them.  With u = 1024 the ranges below give per = 2 and 3;
with a small u the same construction -- u rows per "workgroup", u "threads" -- is cheap enough for the textbook reference, which
is how test_pileup_domains_scale_cpu.py checks that the planes hold what this file claims.

Layout.  CpG candidate k sits at locus 4 k + 1, a CHG row at every locus 4 k, the loci 4 k + 2 and 4 k + 3 stay uncovered: row
index, locus index and 4096-locus block index all differ.  Spacing 4 links under max_gap 7.  R = 2 u^2 + 3 u + 5 CpG rows; two
candidates less between rows u^2 - 1 | u^2 and two between rows u^2 | u^2 + 1 (a gap of 12 loci: a break), so row u^2 is a
one-row segment between two breaks.  The break-delimited ranges, as loci [lo, hi) and CpG rows:

    A   rows [0, u^2)          u^2              nagg = u: every carry thread one aggregate; with the reduce-only passes' extra
                                                identity slot u + 1 slots, per = 2
    B   rows [0, u^2 + 1)      u^2 + 1          nagg = u + 1, per = 2; the last workgroup holds one row, thread u / 2 one aggregate
    C   rows [u^2 + 1, R)      u^2 + 3 u + 4    nagg = u + 4, per = 2; lo is odd
    W   all                    R                nagg = 2 u + 4, per = 3

Content.  Noise: counts 0 .. 3 in stretches of mostly-high and mostly-low rows 20 .. 120 rows long, thousands of segments at u = 1024: the
aggregates' P and N differ and a segment lies across nearly every workgroup edge.  Four NO-CLAMP STRETCHES of 7 u rows, two in A and two in C: rows of
e = +4 and -4 under the rule TIE = (4, -4, 8, 7), alternating but with a sign repeated about every tenth row, d kept within +-8.
No clamp acts inside and every back-pointer is KEEP, so d has to travel forward and the end state backward through every slice
edge the stretch crosses (a stretch of 7 u rows holds a whole slice and crosses two edges for per = 2 and for per = 3, wherever the
slices start); the repeated signs make d differ from one workgroup edge to the next, so that an aggregate left out of a carry
moves d.  Each stretch is
    entered by three rows (0, 3) -- d = -20 whatever came before -- and one row (3, 0) or (2, 0): d = 4 (stretches 0 and 2) or 0,
    left through ONE row chosen from the d the stretch ends with, so that d is exactly S + 4 = 12 (stretches 0 and 2) or -12 there,
    followed by four decisive rows of the OTHER sign: (0, 3) behind d = 12, (3, 0) behind d = -12.
That row's back-pointer is constant (d beyond +-S), the stretch takes its state; had d arrived 4 nearer to 0 the back-pointer
would be KEEP and the whole stretch would take the state of the rows behind it.  So stretches 0 and 2 are HIGH in front of LOW
rows, 1 and 3 LOW in front of HIGH rows.
Near the end of C: a counter above 2^20 on either plane inside segments of their own sign, and a locus 4 k + 2 with a negative
counter (a covered locus, never a row) inside the high one."""
import numpy as np

TIE = (4, -4, 8, 7)                                           # (A, B, S, max_gap); e = 4 (pcov - ncov)
BIG = (1 << 20) + 5
STRETCH_PRE, STRETCH_POST = 4, 5                              # rows in front of a stretch, and behind it (the row that leaves it + 4)


def _noise(n, seed):
    """n rows, none of them empty: stretches 20 .. 120 rows long, high (1 .. 3 : 0 .. 1) or low (0 .. 1 : 1 .. 3)"""
    rng = np.random.default_rng(seed)
    m = n // 20 + 2
    run = np.repeat(rng.integers(0, 2, m), rng.integers(20, 121, m))[:n]
    p = np.where(run, rng.integers(1, 4, n), rng.integers(0, 2, n))
    q = np.where(run, rng.integers(0, 2, n), rng.integers(1, 4, n))
    return p, q


def _stretch(p, q, first, length, d_in, seed):
    """writes rows [first - STRETCH_PRE, first + length + STRETCH_POST): the stretch is rows [first, first + length).  d_in = 4:
    entered with d = 4 and left high in front of low rows; d_in = 0: entered with d = 0 and left low in front of high rows"""
    S = TIE[2]
    rng = np.random.default_rng(seed)
    p[first - 4:first - 1], q[first - 4:first - 1] = 0, 3
    p[first - 1], q[first - 1] = 2 + d_in // 4, 0
    again = rng.random(length) < 0.1
    d, up = d_in, True
    for t in range(length):
        if not again[t]:
            up = not up
        if abs(d + (4 if up else -4)) > S:
            up = not up
        d += 4 if up else -4
        p[first + t], q[first + t] = (2, 1) if up else (1, 2)
    t = first + length
    if d_in:
        p[t], q[t] = (S + 4 - d) // 4, 0                      # d = S + 4: constant 1
        p[t + 1:t + 5], q[t + 1:t + 5] = 0, 3
    else:
        p[t], q[t] = 0, (S + 4 + d) // 4                      # d = -S - 4: constant 0
        p[t + 1:t + 5], q[t + 1:t + 5] = 3, 0


def build(u):
    """-> ((pcov, ncov, key) int32 planes, info).  info: u, R, n (loci), row_locus (int64 [R]: the locus of CpG row r), ranges
    {name: (lo, hi, first row, rows)} and stretches [(first row, last row, range name, d_in)]"""
    assert u >= 16 and u % 2 == 0
    L = 7 * u
    R = 2 * u * u + 3 * u + 5
    K = R + 4                                                 # candidates
    n = 4 * K
    cand = np.delete(np.arange(K), [u * u, u * u + 1, u * u + 3, u * u + 4])
    row_locus = 4 * cand + 1
    assert len(cand) == R
    p, q = _noise(R, 1000 + u)
    starts = [u * u // 128 + 3 + STRETCH_PRE, u * u // 2 - 2 + STRETCH_PRE,
              u * u + 1 + u // 2 + STRETCH_PRE, u * u + 1 + u * u // 2 + 5 + STRETCH_PRE]   # the third: rows u^2 + 2 u of W lie in it
    stretches = []
    for k, first in enumerate(starts):
        d_in = 4 if k % 2 == 0 else 0
        _stretch(p, q, first, L, d_in, 2000 + u + k)
        stretches.append((first, first + L - 1, "A" if k < 2 else "C", d_in))
    assert starts[0] + L + STRETCH_POST <= starts[1] - STRETCH_PRE and starts[1] + L + STRETCH_POST <= u * u - 3
    assert starts[2] + L + STRETCH_POST <= starts[3] - STRETCH_PRE and starts[3] + L + STRETCH_POST <= R - 30
    p[u * u - 3:u * u], q[u * u - 3:u * u] = 3, 0             # high rows in front of the first break: d != 0 at the range's end
    p[u * u], q[u * u] = 0, 3                                 # the one-row segment
    p[R - 30:R - 23], q[R - 30:R - 23] = 3, 0                 # a high segment with a counter above 2^20 ...
    p[R - 27] = BIG
    p[R - 20:R - 13], q[R - 20:R - 13] = 0, 3                 # ... and a low one
    q[R - 17] = 2 * BIG
    P, Q, key = np.zeros(n, np.int64), np.zeros(n, np.int64), (np.arange(n, dtype=np.int64) % 100003) << 2
    P[row_locus], Q[row_locus] = p, q
    P[0::4], Q[0::4] = _noise(K, 3000 + u)                    # CHG rows
    key[0::4] |= 1
    neg = int(row_locus[R - 29]) + 1                          # ... and, one locus behind a row of the high segment, a negative counter
    P[neg], Q[neg] = -1, 70
    first_c = int(row_locus[u * u + 1])
    ranges = {"A": (0, 4 * u * u, 0, u * u), "B": (0, 4 * (u * u + 3), 0, u * u + 1), "C": (first_c, n, u * u + 1, u * u + 3 * u + 4),
              "W": (0, n, 0, R)}
    info = {"u": u, "R": R, "n": n, "row_locus": row_locus, "ranges": ranges, "stretches": stretches, "negative": neg}
    return (P.astype(np.int32), Q.astype(np.int32), key.astype(np.int32)), info


def slice_edges(first, last, origin, width):
    """carry slices of `width` rows counted from row `origin` (a range's first row for the forward scan; one behind its last row
    for the backward scan, which counts from the end) -> the edges e, first <= e <= last + 1, an edge lying between rows e - 1
    and e.  Two neighbours are a whole slice inside rows [first, last]; an edge with first < e <= last is crossed by them."""
    return [e for e in range(first, last + 2) if (e - origin) % width == 0]
