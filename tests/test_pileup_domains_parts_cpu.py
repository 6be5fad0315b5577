"""Methylation domains from pieces (`pileup_dist -D`), host side: chain_domain_parts and stitch_domains over the sequential
stand-in of the three device passes (domains_parts_ref) against textbook Viterbi over the whole row list (domains_ref), byte for
byte.  No GPU and no tolerance: everything is Python ints, and level / score are the same four fp64 operations on both sides."""
import numpy as np
import pytest

from domains_parts_ref import CODES, KEEP, SEGMENTS, SUMMARY, clamp, piece
from domains_ref import AFTER_BREAK, BEFORE_BREAK, COV_CLAMP, domains, emissions, switch_costs

LOCUS = np.dtype([("gpos", "<i8"), ("pcov", "<i4"), ("ncov", "<i4"), ("motif", "<u4"), ("reserved", "<u4")])
TIE = (4, -4, 8, 7)                                           # e = 4 (pcov - ncov): planted ties are exact
SCORES = (136278, -98571, 524288, 1000)                       # domain_scores(0.1, 0.8, 8)
BOUNDS = (1 << 24, -(1 << 24), 1 << 24, 1)


def _loci(rows, ctx=0):
    a = np.zeros(len(rows), LOCUS)
    for i, (g, p, n) in enumerate(rows):
        a[i] = (g, p, n, ctx, 0)
    return a


def _chain(rows, cuts, rule, ctx=0):
    """the rows cut before the row indices `cuts` (ascending, repeats give empty pieces) -> (stitched, per-piece segments)"""
    from hifimeth_amd.pileup import chain_domain_parts, stitch_domains
    edges = [0, *cuts, len(rows)]
    parts = chain_domain_parts([piece(rows[a:b], ctx) for a, b in zip(edges, edges[1:])], *rule)
    assert len(parts) == len(edges) - 1
    return stitch_domains(parts, rule[0], rule[1]), parts


def _check(rows, cuts, rule, ctx=0):
    got, parts = _chain(rows, cuts, rule, ctx)
    want, R = domains(_loci(rows, ctx), ctx, *rule)
    assert R == len(rows) and got.dtype == want.dtype
    assert got.tobytes() == want.tobytes(), (rows, cuts, rule)
    return got, parts


def _random_rows(rng, R, max_gap, big=False):
    gpos = np.cumsum(rng.choice([1, 2, max_gap, max_gap + 1, 3 * max_gap], R, p=[0.5, 0.2, 0.1, 0.1, 0.1])) + int(rng.integers(0, 50))
    run = np.repeat(rng.integers(0, 2, R), rng.integers(1, 6, R))[:R]            # stretches of high and low rows, with noise
    p = np.where(run, rng.integers(1, 5, R), rng.integers(0, 2, R))
    n = np.where(run, rng.integers(0, 2, R), rng.integers(1, 5, R))
    n = np.where(p + n == 0, 1, n)
    if big:
        p = np.where(rng.random(R) < 0.1, (1 << 20) + rng.integers(0, 9, R), p)
    return [(int(g), int(a), int(b)) for g, a, b in zip(gpos, p, n)]


def _d(rows, A, B, S, max_gap):
    e = emissions([r[1] for r in rows], [r[2] for r in rows], A, B)
    cost = switch_costs([r[0] for r in rows], S, max_gap)
    d, x = [], 0
    for t in range(len(rows)):
        x = clamp(x, -cost[t], cost[t]) + e[t]
        d.append(x)
    return d, cost


@pytest.mark.parametrize("rule", [TIE, SCORES, (4, -4, 0, 7)], ids=["tie", "scores", "S=0"])
def test_every_cut_and_every_pair_of_cuts(rule):
    rng = np.random.default_rng(11)
    states = set()
    for R in (1, 2, 3, 7, 12):
        for _ in range(3):
            rows = _random_rows(rng, R, rule[3])
            for a in range(R + 1):                            # a == 0 and a == R: an empty piece at an end
                states |= {int(z) for z in _check(rows, [a], rule)[0]["state"]}
                for b in range(a, R + 1):                     # b == a: an empty piece in the middle
                    _check(rows, [a, b], rule)
    assert states == {0, 1}


@pytest.mark.parametrize("rule", [TIE, SCORES, (4, -4, 0, 7), BOUNDS], ids=["tie", "scores", "S=0", "bounds"])
def test_random_partitions_of_up_to_40_rows(rule):
    rng = np.random.default_rng(5)
    crossing = 0
    for _ in range(60):
        R = int(rng.integers(1, 41))
        rows = _random_rows(rng, R, rule[3], big=rule is BOUNDS)
        for a in range(R + 1):
            _check(rows, [a], rule)
        for _ in range(6):
            cuts = sorted(int(c) for c in rng.integers(0, R + 1, int(rng.integers(1, 9))))
            got, parts = _check(rows, cuts, rule)
            crossing += sum(len(p) for p in parts) - len(got)
    assert crossing > 100                                     # segments were joined across cuts, many times


def test_empty_and_one_row_pieces():
    rng = np.random.default_rng(3)
    rows = _random_rows(rng, 9, TIE[3])
    _check(rows, [0, 0, 4, 4, 4, 9, 9], TIE)                  # empty pieces at the start, in the middle and at the end
    _check(rows, list(range(1, 9)), TIE)                      # nothing but one-row pieces
    _check(rows, [0, 1, 1, 2, 8, 8], SCORES)
    got, parts = _chain([], [0, 0], TIE)
    assert len(got) == 0 and all(len(p) == 0 for p in parts)
    assert len(_check([(5, 1, 0)], [0], TIE)[0]) == 1


def test_ties_on_a_piece_boundary():
    A, B, S, max_gap = TIE
    # d == S at the last row of a piece, low rows behind it: the back-pointer across the cut is the identity, not "1"
    up = [(10, 2, 0), (11, 0, 3), (12, 0, 3), (13, 0, 3)]
    d, cost = _d(up, *TIE)
    assert d[0] == S == cost[1]
    got, _ = _check(up, [1], TIE)
    assert len(got) == 1 and got[0]["state"] == 0             # one more methylated read and row 0 would be a segment of its own
    assert len(_check([(10, 3, 0)] + up[1:], [1], TIE)[0]) == 2
    # d == -S, high rows behind it
    down = [(10, 0, 2), (11, 3, 0), (12, 3, 0), (13, 3, 0)]
    d, cost = _d(down, *TIE)
    assert d[0] == -S == -cost[1]
    got, _ = _check(down, [1], TIE)
    assert len(got) == 1 and got[0]["state"] == 1
    # the tie deeper in: d == S_t again at a cut after the clamp has acted
    rows = [(10, 3, 0), (11, 3, 0), (12, 1, 1), (13, 0, 3), (14, 0, 3), (15, 0, 3), (16, 0, 3)]
    d, cost = _d(rows, *TIE)
    assert d[1] == 20 and d[2] == S == cost[3]
    for cut in range(len(rows) + 1):
        _check(rows, [cut], TIE)
    # d == 0 at the very end and at a cut
    flat = [(10, 1, 1), (11, 1, 1), (12, 1, 1)]
    assert _d(flat, *TIE)[0] == [0, 0, 0]
    got, _ = _check(flat, [1, 2], TIE)
    assert len(got) == 1 and got[0]["state"] == 0


def test_breaks_and_gaps_on_a_piece_boundary():
    A, B, S, max_gap = TIE
    for gap, n_seg in ((max_gap, 1), (max_gap + 1, 2)):
        rows = [(100, 3, 0), (101, 3, 0), (101 + gap, 3, 0), (102 + gap, 3, 0)]
        got, parts = _check(rows, [2], TIE)
        assert len(got) == n_seg
        assert int(parts[0][-1]["flags"]) & BEFORE_BREAK == (BEFORE_BREAK if n_seg == 2 else 0)
        assert int(parts[1][0]["flags"]) & AFTER_BREAK == (AFTER_BREAK if n_seg == 2 else 0)
        _check(rows, [2, 2], TIE)                             # an empty piece inside the gap
        _check(rows, [1], TIE)
        _check(rows, [3], TIE)
    # a low row right behind a break: without the break the penalty would keep it high
    rows = [(100 + k, 3, 0) for k in range(4)] + [(104 + max_gap, 0, 1), (105 + max_gap, 3, 0)]
    for cut in range(len(rows) + 1):
        _check(rows, [cut], TIE)


def test_saturated_counters_give_a_constant_composite():
    A, B, S, max_gap = BOUNDS
    big = (1 << 20) + 5
    rows = [(k, 0, 1) for k in range(3)] + [(3 + k, big, 0) for k in range(20)] + [(23 + k, 0, big) for k in range(40)] + [(63, 1, 0)]
    e_big = COV_CLAMP * A
    assert 17 * e_big >= 1 << 48 > 16 * e_big
    for cut in (3, 23):
        s = piece(rows[cut:cut + 20], 0)(SUMMARY, {}, *BOUNDS)
        assert s["lo"] == s["hi"] and abs(s["c"]) == 1 << 48  # the constant form: c no longer enters
    s = piece(rows[3:19], 0)(SUMMARY, {}, *BOUNDS)
    assert s["c"] == 15 * e_big < 1 << 48                     # a few rows fewer: still exact in c
    for cut in range(len(rows) + 1):
        _check(rows, [cut], BOUNDS)
    _check(rows, [3, 23, 43], BOUNDS)
    _check(rows, [2, 24, 62], BOUNDS)


def test_carries_are_what_the_whole_scan_holds():
    """the carries themselves, not only the stitched result: prev_d is d of the row before the piece, last_state its path state"""
    from hifimeth_amd.pileup import domain_backward_carries, domain_forward_carries
    from domains_ref import viterbi
    rng = np.random.default_rng(8)
    for _ in range(40):
        R = int(rng.integers(2, 30))
        rows = _random_rows(rng, R, TIE[3])
        d, cost = _d(rows, *TIE)
        z = viterbi(emissions([r[1] for r in rows], [r[2] for r in rows], TIE[0], TIE[1]), cost)
        cuts = sorted(int(c) for c in rng.integers(0, R + 1, 4))
        edges = [0, *cuts, R]
        ps = [piece(rows[a:b], 0) for a, b in zip(edges, edges[1:])]
        sums = [p(SUMMARY, {}, *TIE) for p in ps]
        fwd = domain_forward_carries(sums, TIE[2], TIE[3])
        codes = [p(CODES, f, *TIE) for p, f in zip(ps, fwd)]
        bwd = domain_backward_carries(sums, codes, TIE[2], TIE[3])
        for (a, b), f, c, w in zip(zip(edges, edges[1:]), fwd, codes, bwd):
            assert f["has_prev"] == (a > 0) and w["has_next"] == (b < R)
            if a > 0:
                assert (f["prev_gpos"], f["prev_d"]) == (rows[a - 1][0], d[a - 1])
            if b < R:
                assert w["next_gpos"] == rows[b][0]
            if b > a:
                assert c["d_last"] == d[b - 1] and w["last_state"] == z[b - 1] and c["back"] in (0, 1, KEEP)
        for p, f, w, (a, b) in zip(ps, fwd, bwd, zip(edges, edges[1:])):
            states = [int(g["state"]) for g in p(SEGMENTS, {**f, **w}, *TIE)["segments"] for _ in range(int(g["n_loci"]))]
            assert states == z[a:b]
