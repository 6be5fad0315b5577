"""Crafted samples for `groupdmr` beyond one slice per scan thread, in plain numpy: build(B, T) for the device's units.

hm_dmr_fetch_regions runs the selection skeleton of hm_pileup.hip three times: over the loci of the range (the context's rows),
and twice over the ROW INDICES [0, R) (the hits, the chains).  A selection workgroup takes B = LOCI_PER_BLOCK = 4096 indices, and
the ONE workgroup of loci_scan_kernel gives each of its T = 1024 threads a slice of per = ceil(blocks / T) block counts.  With
(B, T) = (4096, 1024) the geometry below gives per = 2 over the rows and per = 3 over the loci; with (16, 8) the same
construction is small enough for the loop restatements, which is how test_group_regions_scale_cases_cpu.py checks that the
samples hold what this file claims.

Geometry.  R = B T + 3 B + 5 rows of context 0 (T + 4 blocks, the last of 5 rows: per = 2, the threads from T / 2 + 2 on without a
slice; the first sequence alone has T + 3 blocks, so its last used thread has a short slice, and a range of B T rows has per = 1
with every thread used) on n = (2 T + 4) B - 1 bases (2 T + 4 blocks of loci: per = 3).  Row 0 is base 0, row R - 1 is base
n - 1.  Rows lie two bases apart, except: the gaps the cases below set, and the last 2 B + 17 other rows, one base apart, which
make n come out.  Loci that are no rows of context 0 -- untested, of context 1 or 2 -- lie on the base in front of a row.  Two
sequences; the second begins inside the chain "sequence boundary".

Samples.  2 + 2, and a third sample of group 1 that has rows only where a kind gives it some; min_cov 5, min_reps 2.  KINDS gives
per kind the motif and every sample's (pcov, ncov); SIGN its sign as a hit at max_p 0.01 (the rows' p is checked where the rows
are made: the hits' below 0.008, 'N' and 'o' at D = 0 and p = 1, 'A' at 0.46: a hit at max_p 1 only).

Crafted chains, by first and last row of context 0, named in info["chains"] (at max_p 0.01, min_diff 0, max_gap MAX_GAP):
    "row 0"                 rows 0 .. 1
    "min_loci - 1"          from row B - 1, min_loci - 1 rows, min_loci = B + 904 B / 4096: across rows B (an untested locus between
                            rows B - 1 and B) and 2 B (a locus of context 1 between rows 2 B - 1 and 2 B): neither links nor breaks
    "min_loci"              from row 3 B - 1; rows 3 B - 1 and 3 B exactly MAX_GAP apart
    "min_loci + 1"          from row 5 B - 1
    "gap + 1, left / right" rows 7 B - 2 .. 7 B - 1 and 7 B .. 7 B + 1, MAX_GAP + 1 apart
    "row B T"               rows B T - 2 .. B T + 2: the first row of the block that makes per 2
    "long heavy"            from row 9 B - 1, long_n rows of kind 'H' (every sample a million calls): 70 001 rows at B = 4096,
                            each of the four sums above 2^32; B + 2 rows at a smaller B
    "sequence boundary"     rows (T + 2) B + 4 .. + 7, the second sequence beginning with the third of them
    "sign flip, left"       rows (T + 3) B - 2 .. (T + 3) B - 1
    "row R - 1"             rows (T + 3) B .. R - 1, of the other sign
Every one has a tested non-hit on either side, but for the two pairs that meet at rows 7 B and (T + 3) B.  Elsewhere: seeded runs of 1 .. 10 hits of one sign, B / 40 .. B / 10 non-hits
between them, and seeded runs of loci of the other contexts."""
import numpy as np

import groups_ref as G
import group_regions_ref as RR

MIN_COV, MIN_REPS, MAX_GAP = 5, 2, 5
SAMPLES = ((1, 0), (1, 1), (1, 2), (2, 0), (2, 1))            # (group, index within it), in the order they are opened
_UP, _DOWN, _LEVEL = [(40, 0), (40, 0), None], [(0, 40), (0, 40)], [(10, 10), (10, 10)]
# kind -> (motif, the three samples of group 1, the two of group 2), a sample (pcov, ncov) or None (no row)
KINDS = {
    "P": (0, _UP, _DOWN),                                                 # a hit, group 1 above
    "M": (0, _DOWN + [None], _UP[:2]),                                    # a hit, group 2 above
    "N": (0, _LEVEL + [None], _LEVEL),                                    # tested, no hit: D = 0, p = 1
    "U": (0, _UP, [(0, 40), None]),                                       # not tested: one counting sample in group 2
    "O": (1, _UP, _DOWN),                                                 # a hit of context 1
    "o": (1, _LEVEL + [None], _LEVEL),                                    # ... and a tested non-hit of it
    "C": (3, _DOWN + [None], _UP[:2]),                                    # a hit of context 2 by motif 3
    "A": (0, [(12, 8), (12, 8), None], _LEVEL),                           # diff 10, p = 0.46: a hit at max_p 1 only
    "q": (0, [(400, 0), (396, 4), None], [(0, 400), (4, 396)]),           # a hit with phi > 1
    "p": (0, [(40, 0)] * 3, _DOWN),                                       # a hit with m1 = 3
    "b": (0, [(40, 0), (40, 0), (3, 1)], _DOWN),                          # a third sample below the coverage: the row of 'P'
    "H": (0, [(700000, 300000)] * 2 + [None], [(300000, 700000)] * 2),    # heavy: a million calls per sample, diff 40
}
SIGN = {"P": 1, "M": -1, "N": 0, "O": 1, "o": 0, "C": -1, "A": 0, "q": 1, "p": 1, "b": 1, "H": 1}     # at max_p 0.01; 'U' is no row


def thresholds(min_loci):
    """(max_p, min_diff, max_gap, min_loci): the first is the one the number of chains is asserted at; the last leaves 'H' out"""
    return ((0.01, 0.0, MAX_GAP, 3), (0.01, 0.0, MAX_GAP, min_loci), (1.0, 0.0, MAX_GAP, 1), (0.01, 50.0, MAX_GAP + 1, 2))


def _codes(text):
    return np.frombuffer(text.encode(), np.uint8)


def _table(of, dtype=np.int64):
    t = np.zeros(256, dtype)
    for k in KINDS:
        t[ord(k)] = of(k)
    return t


def kind_chains(gpos, kind, max_gap, weak=False):
    """the chains of the rows (gpos, kind codes) of one context from SIGN alone ('A' a hit of sign + when weak) -> first, last, sign"""
    sign = _table(lambda k: SIGN.get(k, 0) or (k == "A" and weak))[kind]
    hit = sign != 0
    link = hit[1:] & (sign[1:] == sign[:-1]) & (np.diff(gpos) <= max_gap)
    head, tail = hit.copy(), hit.copy()
    head[1:] &= ~link
    tail[:-1] &= ~link
    first = np.flatnonzero(head)
    return first, np.flatnonzero(tail), sign[first]


def build(B, T, seed=5):
    """-> (samples {(group, index): (gpos, pcov, ncov, motif)}, info).  info: B, T, R, n, lengths, min_loci, long_n, thresholds,
    gpos / kind (every locus, ascending, kind as the character's code), row_gpos / row_kind (the rows of context 0), chains
    {name: (first row, last row, sign, flags)}, long_sums (the four sums of "long heavy"), n_chains and its bounds"""
    assert B >= 16 and B % 8 == 0 and T >= 8 and T % 2 == 0
    full = B * T >= 1 << 22
    R, n = B * T + 3 * B + 5, (2 * T + 4) * B - 1
    min_loci = B + max(3, 904 * B // 4096)
    long_n = 70001 if full else B + 2
    rng = np.random.default_rng(seed)
    kind = np.full(R, ord("N"), np.uint8)
    gap = np.full(R, 2, np.int64)                             # gap[r]: from row r - 1 to row r
    gap[0] = 0
    fixed, claimed = np.zeros(R, bool), np.zeros(R, bool)     # the gap in front of the row is part of a case; the row is
    fixed[0] = True
    chains, extras = {}, []                                   # extras: (row, kind): a locus on the base in front of the row

    def put(first, kinds):
        k = _codes(kinds)
        lo, hi = max(first - 1, 0), min(first + len(k), R - 1)      # with a non-hit on either side
        assert not claimed[lo:hi + 1].any(), first
        kind[first:first + len(k)] = k
        claimed[lo:hi + 1] = True

    def mixed(length):
        return "".join("p" if k % 7 == 3 else "q" if k % 5 == 2 else "b" if k % 11 == 6 else "P" for k in range(length))

    put(0, "PP")
    chains["row 0"] = (0, 1, 1, RR.FIRST)
    for name, first, length in (("min_loci - 1", B - 1, min_loci - 1), ("min_loci", 3 * B - 1, min_loci), ("min_loci + 1", 5 * B - 1, min_loci + 1)):
        put(first, mixed(length))
        chains[name] = (first, first + length - 1, 1, 0)
    assert chains["min_loci - 1"][1] >= 2 * B and chains["min_loci + 1"][1] < 7 * B - 4
    extras += [(B, "U"), (2 * B, "O")]
    fixed[[B, 2 * B]] = True
    gap[3 * B], fixed[3 * B] = MAX_GAP, True
    put(7 * B - 2, "PPPP")
    gap[7 * B], fixed[7 * B] = MAX_GAP + 1, True
    chains["gap + 1, left"], chains["gap + 1, right"] = (7 * B - 2, 7 * B - 1, 1, 0), (7 * B, 7 * B + 1, 1, 0)
    put(B * T - 2, "PPqPP")
    chains["row B T"] = (B * T - 2, B * T + 2, 1, 0)
    put(9 * B - 1, "H" * long_n)
    chains["long heavy"] = (9 * B - 1, 9 * B - 2 + long_n, 1, 0)
    at = (T + 2) * B + 4
    put(at, "PPPP")
    chains["sequence boundary"] = (at, at + 3, 1, 0)
    put((T + 3) * B - 2, "PPMMMMM")
    chains["sign flip, left"], chains["row R - 1"] = ((T + 3) * B - 2, (T + 3) * B - 1, 1, 0), ((T + 3) * B, R - 1, -1, RR.LAST)
    assert (T + 3) * B + 4 == R - 1

    # elsewhere: runs of hits between runs of non-hits
    m = R // max(1, B // 40) + 2
    hit_len, non_len = rng.integers(1, 11, m), rng.integers(max(1, B // 40), max(2, B // 10) + 1, m)
    run_sign = rng.choice([1, -1], m)
    pattern = np.repeat(np.stack([np.zeros(m, np.int64), run_sign], axis=1).ravel(), np.stack([non_len, hit_len], axis=1).ravel())[:R]
    assert len(pattern) == R
    up = _codes("PPPPPPPqqpbA")[rng.integers(0, 12, R)]
    kind = np.where(claimed, kind, np.where(pattern > 0, up, np.where(pattern < 0, ord("M"), ord("N")))).astype(np.uint8)

    # the rows one base apart that make n come out
    dense = np.flatnonzero(~fixed)[-(2 * (R - 1) + int((gap[fixed] - 2).sum()) + 2 - (n - 1)):]
    gap[dense] = 1
    row_gpos = np.cumsum(gap)
    assert row_gpos[0] == 0 and row_gpos[-1] == n - 1 and len(dense) < R // 2 and (gap[[B, 2 * B]] == 2).all()

    # loci of the other contexts and untested ones, in runs, in front of rows two bases behind their neighbour
    m = R // max(2, B // 200) + 2
    ext_len, off_len = rng.integers(1, 7, m), rng.integers(max(2, B // 200), max(6, B // 20) + 1, m)
    run_kind = _codes("OOOOoCCU")[rng.integers(0, 8, m)]
    ext = np.repeat(np.stack([np.zeros(m, np.uint8), run_kind], axis=1).ravel(), np.stack([off_len, ext_len], axis=1).ravel())[:R]
    ext = np.where((ext == ord("O")) & (rng.random(R) < 0.15), ord("o"), ext)
    ext[claimed | (gap != 2)] = 0
    for row, k in extras:
        ext[row] = ord(k)
    at_rows = np.flatnonzero(ext)
    gpos = np.concatenate([row_gpos, row_gpos[at_rows] - 1])
    order = np.argsort(gpos, kind="stable")
    gpos, all_kind = gpos[order], np.concatenate([kind, ext[at_rows]]).astype(np.uint8)[order]
    assert (np.diff(gpos) > 0).all()

    first_of_two = int(row_gpos[chains["sequence boundary"][0] + 2])
    info = dict(B=B, T=T, R=R, n=n, lengths=(first_of_two, n - first_of_two), min_loci=min_loci, long_n=long_n, thresholds=thresholds(min_loci),
                gpos=gpos, kind=all_kind, row_gpos=row_gpos, row_kind=kind, chains=chains)

    # what the tests rely on, from the kinds alone
    first, last, sign = kind_chains(row_gpos, kind, MAX_GAP)
    found = {(int(a), int(b)): int(s) for a, b, s in zip(first, last, sign)}
    for name, (a, b, s, flags) in chains.items():
        assert found.get((a, b)) == s and flags == (RR.FIRST if a == 0 else 0) | (RR.LAST if b == R - 1 else 0), name
        assert not name.startswith("min_loci") or (a % B == B - 1 and kind[a - 1] == kind[b + 1] == ord("N")), name
    assert chains["long heavy"][0] % B == B - 1 and (kind[chains["long heavy"][0]:chains["long heavy"][1] + 1] == ord("H")).all()
    info["n_chains"] = int(np.count_nonzero(last - first + 1 >= 3))
    info["n_chains_bounds"] = (5000, 30000) if full else (5, R // 3)
    assert info["n_chains_bounds"][0] <= info["n_chains"] <= info["n_chains_bounds"][1], info["n_chains"]
    per_row = [sum(s[j] for s in KINDS["H"][g][:2]) for g in (1, 2) for j in (0, 1)]      # P1, N1, P2, N2 of a row of 'H'
    info["long_sums"] = tuple(long_n * v for v in per_row)
    assert not full or (long_n > 1 << 16 and min(info["long_sums"]) > 1 << 32)
    assert (T + 4, 2 * T + 4) == (-(-R // B), -(-n // B)) and -(-(T + 4) // T) == 2 and -(-(2 * T + 4) // T) == 3

    samples = {}
    for g, s in SAMPLES:
        here = _table(lambda k: KINDS[k][g][s] is not None, bool)[all_kind]
        k = all_kind[here]
        rows = (gpos[here], _table(lambda k: (KINDS[k][g][s] or (0, 0))[0])[k], _table(lambda k: (KINDS[k][g][s] or (0, 0))[1])[k],
                _table(lambda k: KINDS[k][0])[k])
        samples[(g, s)] = tuple(x[::-1].copy() for x in rows) if (g, s) == (2, 1) else rows      # one sample in descending order
    return samples, info


def counted(samples):
    """the rows of a sample that count: pcov + ncov >= MIN_COV"""
    return {key: int((rows[1] + rows[2] >= MIN_COV).sum()) for key, rows in samples.items()}


def expected_rows(samples, n):
    """the hm_group_t rows of the samples over [0, n) at MIN_REPS with everything that is an integer, and diff: the counting
    samples' sums per group, vectorised (a sample gives a locus once).  D, phi and pvalue stay 0."""
    m, P, N = np.zeros((2, n), np.int32), np.zeros((2, n), np.int32), np.zeros((2, n), np.int32)
    motif = np.zeros(n, np.uint32)
    for (g, _s), (gpos, p, q, mo) in samples.items():
        ok = p + q >= MIN_COV
        m[g - 1][gpos[ok]] += 1
        P[g - 1][gpos[ok]] += p[ok].astype(np.int32)
        N[g - 1][gpos[ok]] += q[ok].astype(np.int32)
        motif[gpos[ok]] = np.maximum(motif[gpos[ok]], mo[ok].astype(np.uint32))
    at = np.flatnonzero((m[0] >= MIN_REPS) & (m[1] >= MIN_REPS) & (m[0] + m[1] >= 3))
    rows = np.zeros(len(at), RR.ROW_DTYPE)
    rows["gpos"], rows["motif"], rows["m1"], rows["m2"] = at, motif[at], m[0][at], m[1][at]
    rows["pcov1"], rows["ncov1"], rows["pcov2"], rows["ncov2"] = P[0][at], N[0][at], P[1][at], N[1][at]
    rows["diff"] = G.np_diff(rows["pcov1"], rows["pcov1"].astype(np.int64) + rows["ncov1"], rows["pcov2"], rows["pcov2"].astype(np.int64) + rows["ncov2"])
    return rows


def kind_sums(kind):
    """-> (K1, N1, Q1, m1, K2, N2, Q2, m2) of a locus of the kind: the arguments of groups_ref.stat_f64 and stat_mp"""
    return G.sums_of(*([(s[0], s[0] + s[1]) for s in KINDS[kind][g] if s is not None] for g in (1, 2)), min_cov=MIN_COV)
